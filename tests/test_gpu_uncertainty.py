"""The projection uncertainty stage on the GPU (tscm_projection_uncertainty) against the longdouble restatement
of tests/uncert_ref.py.  Sigma comes from cov_ref (rounded to float64: the same input for the device and the restatement),
so Sigma's own error stays out; one end-to-end case takes it from api.covariance.  Tolerance: a device result may differ
from the reference by 8 max(e64, 26 2^-52 amp) in uncert_ref.uncertainty_errors' measure (uncert_ref.tolerance);
tests/test_uncertainty_reference.py shows on the CPU that this bound rejects every planted mistake.  Flags must be equal
except at the (at most 1 %) pixels whose deciding quantity is within 1e-9 of its threshold.  Each test prints its figures."""
import numpy as np
import pytest

from tests import cov_ref as CR
from tests import uncert_ref as U
from tscm_calib_amd import api, pipeline

pytestmark = pytest.mark.gpu


def _run(inp, grid, device):
    cam_rt, intr, cam_cov, sigma2, requests = inp
    return api.projection_uncertainty(cam_rt, intr, dict(cam_cov=cam_cov, sigma2=sigma2), requests, grid, device)


def _compare(label, got, ref, e64, amp, tol):
    same, near = U.flags_agree(got["flags"], ref)
    e = U.uncertainty_errors(got["planes"], ref)
    print(f"{label}: device error {e}, e64 {e64}, amp {amp:.3e}, tolerance {tol:.3e}, device / tolerance {U.worst(e) / tol:.3g}, near pixels {near:.4f}, "
          f"flags {dict(zip(*np.unique(got['flags'], return_counts=True)))}, kernel {got['seconds_kernel']:.2e} s")
    assert same and near <= 0.01
    assert U.worst(e) <= tol, (label, e, tol)
    # without bits 0 and 1 every double is NaN; with them the first six are numbers
    valid = (got["flags"] & 3) == 3
    assert np.isnan(got["planes"][~np.broadcast_to(valid[:, None], got["planes"].shape)]).all()
    assert not np.isnan(got["planes"][:, :6][np.broadcast_to(valid[:, None], got["planes"][:, :6].shape)]).any()
    for r, (a, b, _) in enumerate(got["requests"]):
        if a == b:
            assert np.isnan(got["sd_across"][r]).all()
    # the summary is a numpy reduction of the planes, exactly
    s = U.summary(got["planes"], got["flags"])
    assert np.array_equal(got["n_valid"], s["n_valid"]) and got["max_sd"].tobytes() == s["max_sd"].tobytes()
    return e


@pytest.mark.parametrize("name,grid", U.GPU_CASES)
def test_uncertainty_against_extended_precision(hip_device, name, grid):
    """rig4, mixed65 with cx, cy held, mixed65 with Double Sphere on camera 1, mono7 (observe only); every call has five or
    more requests (three for mono7) that mix the modes, the cameras (camera 0: w = 0, the small-angle branch; the others
    Rodrigues) and inverse distances 0, 1/5000, 1/300; grids 67 x 5 and 1 x 1 (no multiple of the 256-pixel block; 67 x 5 has
    two blocks), 24 x 16 over the whole image and 9 x 7 reaching outside it -- both leave the disc of pixels that unproject."""
    inp, g, ref, e64, amp, tol = U.case(name, grid)
    got = _run(inp, g, hip_device)
    _compare(f"{name} {grid}", got, ref, e64, amp, tol)
    assert len(inp[4]) >= (5 if inp[0].shape[0] > 1 else 3)


def test_a_point_behind_the_target_camera(hip_device):
    """alpha of camera 2 below 1/2: k <= 0 for part of the other cameras' rays.  Bit 1 is off there and every double NaN."""
    inp, g, ref, e64, amp, tol = U.case("behind", "24x16")
    got = _run(inp, g, hip_device)
    _compare("behind 24x16", got, ref, e64, amp, tol)
    assert (got["flags"] == 1).sum() >= 10


def test_two_calls_give_the_same_bytes(hip_device):
    inp, g, _, _, _, _ = U.case("rig4", "24x16")
    a, b = _run(inp, g, hip_device), _run(inp, g, hip_device)
    for key in ("planes", "flags", "max_sd", "n_valid"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_end_to_end_from_api_covariance(hip_device):
    """Sigma and sigma2 from the device's own tscm_covariance on rig4: against the restatement on that same Sigma."""
    p, kw, _, _, _ = CR.case("rig4")
    cov = api.covariance(p, hip_device, **kw)
    assert cov["status"] == 0
    grid = U.grids()["67x5"]
    requests = U.rig_requests(p.n_cameras)
    got = api.projection_uncertainty(p.cam_rt, p.intr, cov, requests, grid, hip_device)
    args = (p.cam_rt, p.intr, cov["cam_cov"], cov["sigma2"], requests, grid)
    ref = U.uncertainty_ref(*args)
    e64 = U.uncertainty_errors(U.uncertainty_ref(*args, dtype=np.float64)["planes"], ref)
    amp = float(ref["amp"][((ref["flags"] & 3) == 3) & ~ref["near"]].max())
    _compare("rig4 end to end", got, ref, e64, amp, U.tolerance(U.worst(e64), amp))
    assert set(api.UNCERTAINTY_PLANES) <= set(got) and got["u_b"].shape == (len(requests), 5, 67)


def test_pipeline_uncertainty_is_api_projection_uncertainty(hip_device):
    """calibrate_rig(..., uncertainty=dict(step, inv_distances)) on the two-camera rendered rig of test_gpu_pipeline.py:
    implies the covariance; one observe request per camera and one transfer per ordered adjacent pair and distance; the
    bytes of the API call.  Without the argument the result has no such key."""
    from tests.test_gpu_pipeline import _render_rig
    _, _, images = _render_rig(31, 10)
    out = pipeline.calibrate_rig(images, 9, 6, 45.0, device=hip_device, uncertainty=dict(step=40, inv_distances=(0.0, 1.0 / 300)))
    unc, cov = out["uncertainty"], out["covariance"]
    assert unc["requests"] == [(0, 0, 0.0), (1, 1, 0.0), (0, 1, 0.0), (1, 0, 0.0), (0, 1, 1.0 / 300), (1, 0, 1.0 / 300)]
    h, w = images[0][0].shape[:2]
    assert unc["grid"] == api.uncertainty_grid((w - 1) // 40 + 1, (h - 1) // 40 + 1, 0.0, 0.0, 40.0, 40.0, w, h)
    again = api.projection_uncertainty(out["problem"].cam_rt, out["problem"].intr, cov, unc["requests"], unc["grid"], hip_device)
    for key in ("planes", "flags", "max_sd", "n_valid"):
        assert unc[key].tobytes() == again[key].tobytes(), key
    assert cov["status"] == 0 and np.all(unc["n_valid"] > 0) and np.all(unc["max_sd"] > 0)
    print("rendered rig: max sd_worst per request", unc["max_sd"], "median sd_across", [float(np.nanmedian(x)) for x in unc["sd_across"][2:]])
    import inspect
    assert inspect.signature(pipeline.calibrate_rig).parameters["uncertainty"].default is None
    assert pipeline.uncertainty_requests(4, (0.5,))[:4] == [(m, m, 0.5) for m in range(4)] and len(pipeline.uncertainty_requests(4, (0.5, 0.1))) == 4 + 2 * 8
