"""RANSAC start poses through include/tscm/tscm_calib.hpp on the GPU: TripleSphereCamera::estimate_extrinsic_ransac, called by
tests/native/mirror_ransac.cpp, gives the bytes of rig.estimate_extrinsic_ransac.  Built and run the way
tests/test_gpu_cpp_mirror.py does (one fresh child at a time, none after an abnormal end)."""
import numpy as np
import pytest

from tests import init_ransac_ref as Q
from tests import test_gpu_cpp_mirror as M
from tests.test_gpu_cpp_mirror import bin_dir  # noqa: F401  (fixture)
from tscm_calib_amd import rig

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("option", [None, "3.5,64,20"], ids=["file", "option"])
def test_estimate_extrinsic_ransac_equals_the_python_wrapper(hip_device, bin_dir, option):  # noqa: F811
    intr, pu, pv, count, W, cols, Hn, seed, thr, kinds, moved = Q.case("b9x6_v6_h32")
    V, n = pu.shape
    exe = M._exe(bin_dir, "tests/native/mirror_ransac.cpp")
    src, dst = str(bin_dir / "ransac_in.bin"), str(bin_dir / "ransac_out.bin")
    with open(src, "wb") as f:
        f.write(np.array([V, n, cols, Hn, 0, seed], np.int32).tobytes())
        f.write(np.array([thr]).tobytes() + intr.tobytes() + W.tobytes())
        f.write((count > 0).astype(np.int32).tobytes() + pu.tobytes() + pv.tobytes())
    r = M._run_child([exe, src, dst, *([option] if option else [])], bin_dir)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(dst, "rb").read()
    done = int(np.frombuffer(raw, np.int32, 1)[0])
    code = np.frombuffer(raw, np.int32, V, 4)
    Rt = np.frombuffer(raw, np.float64, 9 * V, 4 + 4 * V).reshape(V, 3, 3)
    inl = np.frombuffer(raw, np.uint8, V * n, 4 + 4 * V + 72 * V).reshape(V, n)
    prm = rig.ransac_params(threshold_px=thr, n_hypotheses=Hn, seed=seed) if option is None else \
        rig.ransac_params(threshold_px=3.5, n_hypotheses=64, min_inliers=20, seed=seed)
    wRt, winl, _, wcode, wdone = rig.estimate_extrinsic_ransac(intr, pu, pv, count, W, cols, prm, hip_device)
    assert done == wdone > 0
    M._assert_same(code, wcode, "code")
    M._assert_same(Rt, wRt, "Rt")
    M._assert_same(inl.astype(bool), winl, "inlier")
    assert len(set(code.tolist())) >= 3                                    # a pose, a view without a board, one without hypothesis
