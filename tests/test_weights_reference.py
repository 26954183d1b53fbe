"""Corner weights and corner masks on the CPU: the reference of tests/weights_ref.py against robust_ref and the oracle, the
Python layer's conversions, and every refusal of the C ABI -- all of which return before a device is touched."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import lib, synth
from tscm_calib_amd.problem import shard_frames
from tests import helpers as H
from tests import robust_ref as R
from tests import weights_ref as W

BLOCKS = ("board_gram", "board_grad", "view_cross", "cam_gram", "cam_grad")


def _p():
    return synth.make_problem(4, 6, 41).normalised()


def test_unit_weights_reproduce_the_plain_and_the_robust_reference():
    p = _p()
    jets = orc.evaluate(p, jets=True)
    one = np.ones(p.n_corners)
    o = H.normal_equations_from(p, *jets[1:])
    g = W.weighted_normal_equations(p, one, jets=jets)
    for k in BLOCKS:
        assert np.array_equal(g[k], o[k]), k
    assert g["cost"] == 0.5 * float(np.sum(np.sum(jets[1].reshape(-1, 2) ** 2, axis=1)))
    a = R.median_scale(p)
    for kind in ("huber", "soft_l1", "cauchy"):
        o = R.robust_normal_equations(p, kind, a, jets=jets)
        g = W.weighted_normal_equations(p, one, kind, a, jets=jets)
        for k in BLOCKS:
            assert np.array_equal(g[k], o[k]), (kind, k)
        assert g["cost"] == o["cost"]


@pytest.mark.parametrize("kind", [None, "huber", "cauchy"])
def test_a_suffix_mask_is_the_oracle_on_the_shortened_problem(kind):
    p = synth.make_problem(4, 10, 42).normalised()
    n = p.n_points
    pattern = np.array([n, 1, n - 1, 2, n // 2, 3, n - 5, 0])
    keep = pattern[(p.view_board // p.n_cameras) % pattern.size]
    w, q = W.suffix_mask(p, keep)
    assert q.n_corners == int(w.sum()) < p.n_corners
    a = R.median_scale(p)
    g = W.weighted_normal_equations(p, w, kind, a)
    o = H.normal_equations_from(q, *orc.evaluate(q, jets=True)[1:]) if kind is None else R.robust_normal_equations(q, kind, a)
    assert abs(g["cost"] - o["cost"]) <= 1e-14 * o["cost"]
    e = H.block_errors(g, o, False)
    assert max(e.values()) <= 1e-14, e          # the same rows, summed in another grouping
    assert abs(W.weighted_rmse(p, w) - orc.rmse(q)) <= 1e-14 * orc.rmse(q)


def test_python_layer_carries_and_converts_weights():
    p = _p()
    w = W.scattered_weights(p, 3)
    p.weights = w
    assert np.array_equal(p.copy().weights, w) and p.copy().weights is not w
    assert np.array_equal(p.normalised().weights, w)
    # the sharding slice keeps each rank's own corners' weights
    parts = [shard_frames(p, r, 2) for r in range(2)]
    assert sum(q.weights.size for q in parts) == w.size and all(q.weights.size == q.n_corners for q in parts)
    assert np.isclose(sum(q.weights.sum() for q in parts), w.sum())
    # a bool mask is 0 / 1; a view whose weights are all 0 goes in with count 0 and loses its entries
    m = w > 0
    q, ww = lib.corner_weights(p, m)
    assert q is p and ww.dtype == np.float64 and np.array_equal(ww, m.astype(np.float64))
    m[:p.view_count[0]] = False
    q, ww = lib.corner_weights(p, m)
    assert q.view_count[0] == 0 and np.array_equal(q.view_count[1:], p.view_count[1:]) and p.view_count[0] > 0
    assert ww.size == q.n_corners and q.obs_u is p.obs_u and q.intr is p.intr
    with pytest.raises(ValueError):
        lib.corner_weights(p, np.ones(3))


def _refusals(p):
    """(weights, fragment of the message) of every refusal of a weight array"""
    n0 = int(p.view_count[0])
    out = []
    for bad, frag in ((-1.0, "corner weight"), (np.nan, "corner weight"), (np.inf, "corner weight")):
        w = np.ones(p.n_corners)
        w[n0 + 2] = bad
        out.append((w, frag, "view 1, corner 2"))
    w = np.ones(p.n_corners)
    w[n0:n0 + int(p.view_count[1])] = 0.0
    out.append((w, "view_count = 0", "view 1"))
    return out


def test_every_refusal_returns_its_code_without_a_device():
    p = _p()
    L = lib.lib()
    cp = lib.c_problem(p)
    o = lib.default_options(False)
    s = lib.CSummary()
    Cn, B, V = p.n_cameras, p.n_boards, p.n_views
    bg, bd, vx, cg, cd = np.zeros((B, 6, 6)), np.zeros((B, 6)), np.zeros((V, 6, 15)), np.zeros((Cn, 15, 15)), np.zeros((Cn, 15))
    cost, valid = C.c_double(0.0), C.c_int(0)
    cam, intr, board = np.zeros_like(p.cam_rt), np.zeros_like(p.intr), np.zeros_like(p.board_rt)
    info = lib.CCovarianceInfo(struct_size=C.sizeof(lib.CCovarianceInfo))
    d = lib.dptr

    def calls(w, opt):
        return [
            lambda: L.tscm_solve_weighted(C.byref(cp), C.byref(opt), d(w), None, 0, 0.0, C.byref(s)),
            lambda: L.tscm_solve_weighted(C.byref(cp), C.byref(opt), d(w), None, lib.LOSS_HUBER, 1.0, C.byref(s)),
            lambda: L.tscm_eval_normal_equations_weighted(C.byref(cp), 0, C.byref(opt), d(w), 0, 0.0, d(bg), d(bd), d(vx), d(cg), d(cd), C.byref(cost)),
            lambda: L.tscm_eval_step_weighted(C.byref(cp), 0, C.byref(opt), d(w), None, 0, 0.0, d(cam), d(intr), d(board), C.byref(valid), C.byref(s)),
        ]

    for w, frag, where in _refusals(p):
        for f in calls(w, o) + [lambda: L.tscm_covariance_weighted(C.byref(cp), 0, None, d(w), 0, 0.0, None, None, None, None, None, C.byref(info))]:
            assert f() == -1
            msg = L.tscm_last_error().decode()
            assert frag in msg and where in msg, msg
    # weights with the 16x16 Gram kernel: unsupported, as for a loss
    o16 = lib.default_options(False, exec_flags=lib.EXEC_GRAM_16X16)
    for f in calls(np.ones(p.n_corners), o16):
        assert f() == -5, L.tscm_last_error().decode()
    assert L.tscm_solver_set_corner_weights(None, None) == -1
    # the batched mono route names the problem
    m = synth.make_problem(1, 4, 43).normalised()
    cps = (lib.CProblem * 2)(lib.c_problem(m), lib.c_problem(m))
    sums = (lib.CSummary * 2)()
    om = lib.default_options(True)
    dp = C.POINTER(C.c_double)
    for w, frag, where in _refusals(m):
        wp = (dp * 2)(dp(), d(w))
        assert L.tscm_solve_mono_batch_weighted(cps, 2, 0, C.byref(om), None, wp, 0, 0.0, sums) == -1
        msg = L.tscm_last_error().decode()
        assert "problem 1" in msg and frag in msg and where in msg, msg
    # the Python layer converts a view whose weights are all 0 instead of passing it on
    w = np.ones(p.n_corners)
    w[:int(p.view_count[0])] = 0.0
    q, ww = lib.corner_weights(p, w)
    assert q.view_count[0] == 0 and ww.size == p.n_corners - int(p.view_count[0])


def test_weights_on_a_solver_created_without_some_views():
    """lib.corner_weights with the counts a solver was built with (Solver.set_corner_weights): the dropped views stay out whatever
    their weights are now, and another view whose weights are all 0 is refused."""
    p = _p()
    n0, n1 = int(p.view_count[0]), int(p.view_count[1])
    w = W.scattered_weights(p, 5)
    w[:n0] = 0.0
    built, w_built = lib.corner_weights(p, w)
    assert built.view_count[0] == 0
    # the same dead view: the same array
    _, again = lib.corner_weights(p, w, built.view_count)
    assert np.array_equal(again, w_built)
    # the dropped view has weights now: they are left out, the rest goes through
    w2 = W.scattered_weights(p, 6)
    assert np.any(w2[:n0] > 0)
    q, got = lib.corner_weights(p, w2, built.view_count)
    assert np.array_equal(got, w2[n0:]) and got.size == built.n_corners and np.array_equal(q.view_count, built.view_count)
    # another view all 0: refused, with and without a dropped view
    w3 = w2.copy()
    w3[n0:n0 + n1] = 0.0
    for counts in (built.view_count, p.view_count):
        with pytest.raises(ValueError, match="create the Solver with weights="):
            lib.corner_weights(p, w3, counts)
    # a solver built with every view and weights that kill none: unchanged
    q, got = lib.corner_weights(p, w2, p.view_count)
    assert q is p and np.array_equal(got, w2)
