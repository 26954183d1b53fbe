"""The batched chessboard structure recovery on the GPU: k_board_seeds (one workgroup per (image, seed), wave s = side s) against
the serial instantiation of the same definition (tscm_calib_amd/csrc/tscm_boards_core.h) on the host, per seed and bit for bit --
status, rows, cols, steps and cells equal, the energy as uint64 -- and in the final boards; then end to end through
find_chessboards(recover="device") and tscm::findCorners of the C++ mirror.  Largest set: a 12 x 9 grid plus 20 clutter points."""
import functools

import numpy as np
import pytest

from tests import boards_cases as B
from tests import test_gpu_cpp_mirror as M
from tests.test_gpu_cpp_mirror import bin_dir  # noqa: F401  (fixture)
from tscm_calib_amd import corners, synth

pytestmark = pytest.mark.gpu


def _assert_same_stages(dev, host, where):
    assert dev["n"] == host["n"], where
    for key in ("status", "rows", "cols", "steps", "offset", "cells"):
        assert np.array_equal(dev[key], host[key]), (where, key, np.flatnonzero(dev["status"] != host["status"])[:5])
    assert np.array_equal(dev["energy"].view(np.uint64), host["energy"].view(np.uint64)), where


def _check_batch(sets, hip_device, name):
    """Stages and boards of one device call against one host call; returns the device stages."""
    dev = corners.chessboards_batch_stages(sets, where="device", device=hip_device)
    host = corners.chessboards_batch_stages(sets, where="host")
    assert len(dev) == len(host) == len(sets)
    for k, (d, h) in enumerate(zip(dev, host)):
        _assert_same_stages(d, h, f"{name} image {k}")
        assert d["on_device"] == (9 <= d["n"] <= 1024) and not h["on_device"], (name, k)
    bd = corners.chessboards_from_corners_batch(sets, where="device", device=hip_device)
    bh = corners.chessboards_from_corners_batch(sets, where="host")
    for k, (u, v, s, st) in enumerate(zip(bd, bh, sets, dev)):
        assert len(u) == len(v), (name, k)
        for a, b in zip(u, v):
            assert a.shape == b.shape and np.array_equal(a, b), (name, k)
        B.check_stages(s[0], s[1], st, u, f"{name} image {k}")
    return dev


def test_twelve_random_sets_in_one_batch(hip_device):
    sets = [B.random_candidates(s)[:4] for s in range(12)]
    dev = _check_batch(sets, hip_device, "random")
    status = np.concatenate([d["status"] for d in dev])
    assert all(np.any(status == s) for s in range(4))                       # the batch reaches every exit of a job
    assert corners.chessboards_batch_seconds() > 0


def test_edge_inputs_in_one_mixed_batch(hip_device):
    """Variable n per image (0, 8, 9, 12, 70, ...) exercises the flat seed list."""
    names = sorted(B.edge_sets())
    _check_batch([B.edge_sets()[k] for k in names], hip_device, "edge")


def test_batch_of_one(hip_device):
    _check_batch([B.random_candidates(17)[:4]], hip_device, "one")


def test_identical_images_give_identical_records(hip_device):
    a, b, c = (B.random_candidates(s)[:4] for s in (21, 22, 23))
    dev = _check_batch([a, b, a, c, b], hip_device, "twins")
    _assert_same_stages(dev[0], dev[2], "twins 0/2")
    _assert_same_stages(dev[1], dev[4], "twins 1/4")


@pytest.mark.parametrize("n", [64, 65, 130])
def test_lane_tails_of_the_reductions(hip_device, n):
    _check_batch([B._sized(n, n)], hip_device, f"n{n}")


def test_more_than_1024_candidates_take_the_host_route_inside_a_device_call(hip_device):
    big, small = B._sized(1025, 1), B.random_candidates(30)[:4]
    dev = _check_batch([big, small], hip_device, "n1025")
    assert not dev[0]["on_device"] and dev[1]["on_device"]


def test_largest_set_12_by_9_grid_with_clutter(hip_device):
    dev = _check_batch([B.grid(12, 9, clutter=20, seed=2)], hip_device, "12x9")
    assert dev[0]["steps"].max() == 15                                        # a seed grows to the whole 12 x 9 grid


def test_the_same_call_twice_gives_the_same_bytes(hip_device):
    sets = [B.random_candidates(s)[:4] for s in (40, 41, 42)] + [B.grid(12, 9, clutter=20, seed=2)]
    a = corners.chessboards_batch_stages(sets, where="device", device=hip_device)
    b = corners.chessboards_batch_stages(sets, where="device", device=hip_device)
    for k, (u, v) in enumerate(zip(a, b)):
        for key in ("status", "rows", "cols", "steps", "offset", "cells"):
            assert u[key].tobytes() == v[key].tobytes(), (k, key)
        assert u["energy"].tobytes() == v["energy"].tobytes(), k


# ------------------------------------------------------------------------------------------------ end to end
SIGMA = 2            # half-size renderings: the board's squares are about 22 pixels


@functools.lru_cache(maxsize=None)
def _views():
    """Three rendered 640 x 540 views of a 9 x 6 board.  Never written to."""
    p = synth.make_problem(1, 6, 3, noise_px=0.0, perturb=False)
    intr = p.meta["gt_intr"][0].copy()
    intr[0] /= 2
    intr[1] /= 2
    intr[2], intr[3] = (intr[2] + 0.5) / 2 - 0.5, (intr[3] + 0.5) / 2 - 0.5
    return tuple(synth.render_chessboard(intr, p.meta["gt_board_rt"][v], 9, 6, 45.0, 640, 540, supersample=2) for v in range(3))


def test_find_chessboards_on_the_device_equals_the_host_route(hip_device):
    imgs = list(_views())
    host = corners.find_chessboards(imgs, 9, 6, sigma=SIGMA, device=hip_device, recover="host")
    dev = corners.find_chessboards(imgs, 9, 6, sigma=SIGMA, device=hip_device, recover="device")
    hb = corners.find_chessboards(imgs, 9, 6, sigma=SIGMA, device=hip_device, recover="host-batch")
    for k, (a, b, c) in enumerate(zip(host, dev, hb)):
        assert a is not None and a.shape == (54, 2), k
        assert b is not None and np.array_equal(a, b), k
        assert c is not None and np.array_equal(a, c), k
    one = corners.find_chessboard(imgs[1], 9, 6, sigma=SIGMA, device=hip_device, recover="device")
    assert np.array_equal(one, host[1])


def test_cpp_mirror_find_corners_equals_find_corner_per_image(hip_device, bin_dir):  # noqa: F811
    exe = M._exe(bin_dir, "tests/native/mirror_boards.cpp")
    files = []
    for k, img in enumerate(_views()):
        files.append(str(bin_dir / f"view{k}.pgm"))
        with open(files[-1], "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
            f.write(img.tobytes())
    r = M._run_child([exe, "device", SIGMA, *files], bin_dir)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    want = corners.find_chessboards(list(_views()), 9, 6, sigma=SIGMA, device=hip_device, recover="device")
    assert len(lines) == 3 * 55
    for k in range(3):
        assert lines[55 * k] == f"image {k} candidates 54 boards 1 same 1", lines[55 * k]
        got = np.array([[float(t) for t in ln.split()] for ln in lines[55 * k + 1:55 * k + 55]])
        assert np.array_equal(got, want[k]), k
