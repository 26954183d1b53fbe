"""Above the batched mono refinement's C ABI: pipeline.calibrate_rig(..., batch_mono=True) on the rendered two-camera rig
of test_gpu_pipeline.py recovers the rig of the per-camera flow, and a C++ host built against the mirror header runs
TripleSphereCamera::refinement_batch on two cameras."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tscm_calib_amd import pipeline, synth
from tests import helpers as H
from tests.test_gpu_pipeline import _render_rig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_calibrate_rig_batch_mono(hip_device):
    _, _, images = _render_rig(31, 10)
    seq = pipeline.calibrate_rig(images, 9, 6, 45.0, device=hip_device)
    bat = pipeline.calibrate_rig(images, 9, 6, 45.0, device=hip_device, batch_mono=True)
    for m in range(2):
        a, b = seq["mono"][m], bat["mono"][m]
        assert np.array_equal(a["has"], b["has"])
        for key in ("first", "second"):
            assert a[key]["num_iterations"] == b[key]["num_iterations"] and a[key]["termination_type"] == b[key]["termination_type"]
        assert H.rel_err(b["intr"][:7], a["intr"][:7]) < 1e-6
    assert bat["summary"]["termination_type"] == 0
    assert bat["summary"]["num_iterations"] == seq["summary"]["num_iterations"]
    assert H.rel_err(bat["problem"].intr[:, :7], seq["problem"].intr[:, :7]) < 1e-6
    assert H.param_rel_err(bat["problem"], seq["problem"])["cam_rt"] < 1e-6


def test_cpp_refinement_batch(hip_device, tmp_path):
    csrc = os.path.join(ROOT, "tscm_calib_amd", "csrc")
    exe = str(tmp_path / "refinement_batch_demo")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "refinement_batch_demo.cpp"), "-L", csrc, "-ltscm_hip", "-Wl,-rpath," + csrc, "-o", exe])
    ps = [synth.make_problem(1, 20, 611, noise_px=0.1), synth.make_problem(1, 20, 612, noise_px=0.3)]
    V, n = ps[0].n_boards, ps[0].n_points
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("3i", 2, V, n))
        f.write(np.concatenate([ps[0].board_xy, np.zeros((n, 1))], axis=1).astype(np.float64).tobytes())
        for p in ps:
            f.write(np.ascontiguousarray(p.intr[0], dtype=np.float64).tobytes())
            f.write(np.ones(V, dtype=np.uint8).tobytes())
            f.write(np.ascontiguousarray(p.board_rt, dtype=np.float64).tobytes())
            f.write(np.stack([p.obs_u, p.obs_v], axis=1).astype(np.float64).tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert b"mixed losses refused" in out.stdout
    raw = open(tmp_path / "out.bin", "rb").read()
    rec = 8 * (9 + 6 * V) + 8
    res = []
    for r in range(4):                                     # batch camera 0, 1, then solo camera 0, 1
        b = raw[r * rec:(r + 1) * rec]
        intr = np.frombuffer(b[:72], dtype=np.float64)
        rt = np.frombuffer(b[72:72 + 48 * V], dtype=np.float64).reshape(V, 6)
        conv, its = struct.unpack("2i", b[-8:])
        res.append((intr, rt, conv, its))
    for m in range(2):
        (bi, br, bc, bn), (si, sr, sc, sn) = res[m], res[2 + m]
        assert bc == sc and bn == sn and bn > 1
        assert H.rel_err(bi[:7], si[:7]) < 1e-6
        assert np.max(np.abs(br - sr)) / np.max(np.abs(sr)) < 1e-6
    assert res[1][0][5] == ps[1].intr[0, 5] and res[3][0][5] == ps[1].intr[0, 5]        # camera 1: lambda held (TSCM_MODEL_DS)
    assert not np.array_equal(res[0][0], ps[0].intr[0])
