"""The covariance stage on the GPU (tscm_covariance, tscm_covariance_from_normal_equations) against the
extended-precision reference of tests/cov_ref.py.  Tolerance: a device result may differ from the longdouble reference by
8 max(e64, n_free 2^-52) in cov_ref.cov_errors' measure, e64 being what the same reference loses in float64 on the same
case (cov_ref.tolerance); the CPU test test_covariance_reference.py shows that this bound rejects every `mistake`.  Each
test prints the measured errors next to e64."""
import ctypes as C

import numpy as np
import pytest

from tests import cov_ref as CR
from tests import helpers as H
from tscm_calib_amd import api, lib, pipeline

pytestmark = pytest.mark.gpu


def _compare(name, got, ref, e64, tol):
    e = CR.cov_errors(got, ref)
    print(f"{name}: n_free {ref['n_free']}, device error {e}, e64 {e64}, tolerance {tol:.3e}, min_pivot_ratio {got['min_pivot_ratio']:.3e} "
          f"(reference {ref['min_pivot_ratio']:.3e}), kernel seconds {got['seconds_kernel']}")
    assert got["status"] == 0 and got["where"] == -1
    assert CR.worst(e) <= tol, (name, e, tol)
    return e


def _assert_not_free_is_zero(got, ref):
    nf = ~ref["cam_free"].ravel()
    n15 = nf.size
    cc = got["cam_cov"].reshape(n15, n15)
    assert not cc[nf].any() and not cc[:, nf].any()
    assert not got["board_cov"][~ref["board_free"]].any() and not got["board_rt_std"][~ref["board_free"]].any()
    assert not got["cam_rt_std"][~ref["cam_free"][:, :6]].any() and not got["intr_std"][~ref["cam_free"][:, 6:]].any()
    assert np.all(got["intr_std"][ref["cam_free"][:, 6:]] > 0) and np.all(got["board_rt_std"][ref["board_free"]] > 0)
    assert np.array_equal(cc, cc.T) and np.array_equal(got["board_cov"], np.swapaxes(got["board_cov"], 1, 2))


@pytest.mark.parametrize("name", list(CR.CASES))
def test_covariance_against_extended_precision(hip_device, name):
    """Cases 1-7 of the feature: full visibility, 1-4 cameras per board with lane and chunk tails, absent pair tiles, several
    panels of the reduced inverse (chain12: 150 camera columns), mono, masks with holes, constant / unseen boards, a camera
    without views, a robust loss.  sigma2, n_free and dof against the reference as well."""
    p, kw, ref, e64, tol = CR.case(name)
    got = api.covariance(p, hip_device, **kw)
    _compare(name, got, ref, e64, tol)
    assert got["n_free"] == ref["n_free"] and got["dof"] == ref["dof"] == 2 * p.n_corners - ref["n_free"]
    assert abs(got["min_pivot_ratio"] - ref["min_pivot_ratio"]) <= 1e-3 * ref["min_pivot_ratio"]
    _assert_not_free_is_zero(got, ref)


def test_two_calls_give_the_same_bytes(hip_device):
    p, kw, ref, e64, tol = CR.case("mixed65-cx_cy")
    a, b = api.covariance(p, hip_device, **kw), api.covariance(p, hip_device, **kw)
    for key in ("cam_cov", "board_cov", "cam_rt_std", "intr_std", "board_rt_std"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert (a["sigma2"], a["min_pivot_ratio"], a["n_free"]) == (b["sigma2"], b["min_pivot_ratio"], b["n_free"])


def test_no_degrees_of_freedom_is_nan(hip_device):
    """One corner per view: fewer residuals than free columns.  sigma2 is NaN whatever the blocks are (here they are
    singular as well: every array NaN, rc 0)."""
    p = H.small_rig(2, 3)
    q = CR._with(p, view_count=np.minimum(p.view_count, 1))
    got = api.covariance(q, hip_device)
    assert got["dof"] == 2 * q.n_views - got["n_free"] <= 0 and np.isnan(got["sigma2"])
    assert got["status"] in (1, 2) and np.isnan(got["cam_cov"]).all() and np.isnan(got["intr_std"]).all() and np.isnan(got["board_rt_std"]).all()


def _crafted():
    """Small-integer blocks: 2 cameras with 2 free columns each, 3 boards, 4 views; regular as they stand."""
    vc, vb = np.array([0, 1, 0, 1]), np.array([0, 0, 1, 2])
    cg = np.zeros((2, 15, 15)); cg[:, np.arange(13), np.arange(13)] = 4.0
    cf = np.zeros((2, 15), bool); cf[:, 6:8] = True
    bg = np.zeros((3, 6, 6)); bg[:] = 2 * np.eye(6)
    vx = np.zeros((4, 6, 15)); vx[:, 0, 6] = 1.0; vx[:, 1, 7] = 1.0
    return vc, vb, bg, vx, cg, cf, np.array([True, True, True])


def test_crafted_blocks_regular_and_singular(hip_device):
    vc, vb, bg, vx, cg, cf, bf = _crafted()
    ref = CR.cov_from_blocks(vc, vb, bg, vx, cg, cf, bf)
    got = api.covariance_from_normal_equations(vc, vb, bg, vx, cg, cf, bf, hip_device)
    assert got["status"] == 0 and got["n_free"] == 4 + 18 and got["sigma2"] != got["sigma2"] and got["cost"] == 0.0
    assert CR.worst(CR.cov_errors(got, ref)) <= 8 * 22 * CR.EPS
    # an exactly singular board block: the lowest such board, every array NaN, rc 0
    bad = bg.copy(); bad[1, 5, 5] = 0.0; bad[2, 0, 0] = -1.0
    got = api.covariance_from_normal_equations(vc, vb, bad, vx, cg, cf, bf, hip_device)
    assert (got["status"], got["where"]) == (1, 1) and np.isnan(got["cam_cov"]).all() and np.isnan(got["board_cov"]).all()
    # an exactly singular reduced system: columns 6 and 7 of camera 1 are the same column (all entries powers of two, so
    # the scaling is exact and the second pivot is exactly 0)
    cg2 = cg.copy(); cg2[1, 6, 7] = cg2[1, 7, 6] = 4.0
    vx0 = np.zeros_like(vx)
    got = api.covariance_from_normal_equations(vc, vb, bg, vx0, cg2, cf, bf, hip_device)
    assert (got["status"], got["where"], got["min_pivot_ratio"]) == (2, 15 + 7, 0.0)
    assert np.isnan(got["cam_cov"]).all() and np.isnan(got["board_cov"]).all()
    ref = CR.cov_from_blocks(vc, vb, bg, vx0, cg2, cf, bf)
    assert (ref["status"], ref["where"]) == (2, 15 + 7)


def test_board_block_of_condition_1e10(hip_device):
    """rig4's blocks (float64, from the oracle) with board 0's block made ill-conditioned by a positive semi-definite term
    (the reduced system only gains): within the e64 rule on these blocks."""
    p, kw, _, _, _ = CR.case("rig4")
    blk = CR.blocks_from_terms(p, H.step_terms(p, dtype=np.float64))
    bg = np.array(blk["board_gram"])
    q, _ = np.linalg.qr(np.random.default_rng(1).normal(size=(6, 6)))
    bg[0] = bg[0] + (q * (np.abs(bg[0]).max() * 10.0 ** np.arange(0, 12, 2))) @ q.T
    bg[0] = (bg[0] + bg[0].T) / 2
    assert 1e9 < np.linalg.cond(bg[0]) < 1e12
    cam_free, board_free = CR.free_columns(p)
    args = (p.view_camera, p.view_board, bg, blk["view_cross"], blk["cam_gram"], cam_free, board_free)
    ref = CR.cov_from_blocks(*args)
    e64 = CR.cov_errors(CR.cov_from_blocks(*args, dtype=np.float64), ref)
    got = api.covariance_from_normal_equations(*args, hip_device)
    _compare("rig4-board0-cond1e10", got, ref, e64, CR.tolerance(CR.worst(e64), ref["n_free"]))


def test_refusals_come_before_the_device(hip_device):
    """Every refusal is TSCM_E_INVALID with the argument named, also with a device index that does not exist (which alone is
    TSCM_E_NO_DEVICE): the arguments are checked first."""
    L = lib.lib()
    p, kw, _, _, _ = CR.case("rig4")
    cp = lib.c_problem(p)
    nowhere = 1 << 20
    info = lib.CCovarianceInfo(struct_size=C.sizeof(lib.CCovarianceInfo))
    call = lambda prob, fixed, kind, scale, inf: L.tscm_covariance(prob, nowhere, fixed, kind, scale, None, None, None, None, None, inf)
    msg = lambda: L.tscm_last_error().decode()
    assert call(C.byref(cp), None, 0, 0.0, C.byref(info)) == -2                     # nothing wrong but the device
    assert call(None, None, 0, 0.0, C.byref(info)) == -1 and "problem" in msg()
    assert call(C.byref(cp), None, 0, 0.0, None) == -1 and "info" in msg()
    short = lib.CCovarianceInfo(struct_size=C.sizeof(lib.CCovarianceInfo) - 8)
    assert call(C.byref(cp), None, 0, 0.0, C.byref(short)) == -1 and "struct_size" in msg()
    w = np.zeros(4, np.uint16); w[2] = 1 << 9
    assert call(C.byref(cp), lib.ushort_ptr(w), 0, 0.0, C.byref(info)) == -1 and "fixed[2]" in msg()
    assert call(C.byref(cp), None, 7, 1.0, C.byref(info)) == -1 and "loss_kind" in msg()
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert call(C.byref(cp), None, lib.LOSS_HUBER, scale, C.byref(info)) == -1 and "loss_scale" in msg()
    bad = p.copy().normalised()
    bad.view_camera[3] = 4
    assert call(C.byref(lib.c_problem(bad)), None, 0, 0.0, C.byref(info)) == -1 and "view_camera" in msg()
    bad = p.copy().normalised()
    bad.view_board[3] = -1
    assert call(C.byref(lib.c_problem(bad)), None, 0, 0.0, C.byref(info)) == -1 and "view_board" in msg()
    for n in (0, 33):
        bad = p.copy().normalised()
        bad.n_cameras = n
        assert call(C.byref(lib.c_problem(bad)), None, 0, 0.0, C.byref(info)) == -1 and "n_cameras" in msg()
    # the block entry
    vc, vb, bg, vx, cg, cf, bf = _crafted()
    ip, ubp = C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    vc, vb, cf8, bf8 = vc.astype(np.int32), vb.astype(np.int32), cf.astype(np.uint8), bf.astype(np.uint8)
    base = dict(n_cameras=2, view_camera=vc, view_board=vb, board_gram=bg, view_cross=vx, cam_gram=cg, cam_free=cf8, board_free=bf8, info=info)

    def blocks(**over):
        a = dict(base, **over)
        ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)
        return L.tscm_covariance_from_normal_equations(a["n_cameras"], 3, 4, ptr(a["view_camera"], ip), ptr(a["view_board"], ip), lib.dptr(a["board_gram"]),
                                                       lib.dptr(a["view_cross"]), lib.dptr(a["cam_gram"]), ptr(a["cam_free"], ubp), ptr(a["board_free"], ubp),
                                                       nowhere, None, None, None if a["info"] is None else C.byref(a["info"]))
    assert blocks() == -2
    for key in ("view_camera", "view_board", "board_gram", "view_cross", "cam_gram", "cam_free", "board_free", "info"):
        assert blocks(**{key: None}) == -1 and key in msg(), key
    assert blocks(info=short) == -1 and "struct_size" in msg()
    assert blocks(n_cameras=0) == -1 and "n_cameras" in msg()
    assert blocks(n_cameras=33) == -1 and "n_cameras" in msg()
    assert blocks(view_camera=np.array([0, 1, 0, 2], np.int32)) == -1 and "view_camera[3]" in msg()
    assert blocks(view_board=np.array([0, 3, 1, 2], np.int32)) == -1 and "view_board[1]" in msg()
    cfb = cf8.copy(); cfb[0, 14] = 1
    assert blocks(cam_free=cfb) == -1 and "cam_free" in msg()


def test_pipeline_covariance_is_api_covariance(hip_device):
    """calibrate_rig(..., covariance=True) on the two-camera rendered rig of test_gpu_pipeline.py: api.covariance on the
    returned problem, byte for byte; without the argument the result has no such key."""
    from tests.test_gpu_pipeline import _render_rig
    _, _, images = _render_rig(31, 10)
    out = pipeline.calibrate_rig(images, 9, 6, 45.0, device=hip_device, covariance=True)
    cov = out["covariance"]
    again = api.covariance(out["problem"], hip_device)
    for key in ("cam_cov", "board_cov", "cam_rt_std", "intr_std", "board_rt_std"):
        assert cov[key].tobytes() == again[key].tobytes(), key
    assert cov["status"] == 0 and cov["sigma2"] == again["sigma2"] and cov["dof"] > 0
    assert np.all(cov["intr_std"][:, :7] > 0) and not cov["cam_rt_std"][0].any() and np.all(cov["cam_rt_std"][1] > 0)
    print("rendered rig: sigma", np.sqrt(cov["sigma2"]), "intr_std", cov["intr_std"], "min_pivot_ratio", cov["min_pivot_ratio"])
    import inspect
    assert inspect.signature(pipeline.calibrate_rig).parameters["covariance"].default is False
