"""The reference of the projection uncertainty stage (tests/uncert_ref.py) checked on the CPU, and the argument
checks of tscm_projection_uncertainty through the C ABI (they come before any device is touched).  No GPU.

  * J of the longdouble restatement against central differences of the whole chain in 50-digit mpmath;
  * the predicted 2 x 2 covariance against a Monte Carlo of exact transfers under draws from N(theta, sigma2 Sigma_cc);
  * properties of the definition;
  * every planted mistake exceeds the tolerance the GPU tests allow, on every GPU case it can show in;
  * the grids of the GPU tests keep the share of pixels with a flag decided within 1e-9 of its threshold below 1 %."""
import ctypes as C

import numpy as np
import pytest

from tests import cov_ref as CR
from tests import helpers as H
from tests import uncert_ref as U
from tscm_calib_amd import lib

LD = np.longdouble
GPU_CASES = U.GPU_CASES          # (case, grid) of tests/test_gpu_uncertainty.py


# ----------------------------------------------------------------------------- J against 50 digits
# 2^-63 is the longdouble's rounding; the chain is a few hundred operations whose roundings add up, each entry of J measured
# against its row's largest entry: 512 roundings is the bound (5.6e-17, still below one rounding of a double).
J_BOUND = 512 * 2.0 ** -63


@pytest.mark.parametrize("a,b", [(0, 1), (1, 0), (2, 3), (0, 0), (3, 3)])
def test_jacobian_against_50_digit_differences(a, b):
    """Both modes, both rotation branches (rig4's camera 0 has w = 0: the small-angle branch; the others Rodrigues), one
    pixel near the centre and one far out, at a finite distance so that the translation columns count."""
    cam_rt, intr, _, _, _ = U.inputs("rig4")
    assert not cam_rt[0, :3].any() and np.all(np.sum(cam_rt[1:, :3] ** 2, axis=1) > U.DBL_EPSILON)
    worst = 0.0
    for q in ((600.25, 500.5), (330.75, 400.125)):
        j = U.jacobian(cam_rt, intr, a, b, 1.0 / 300, np.array([q[0]]), np.array([q[1]]))
        assert j["ok1"][0]
        want = U.mp_jacobian(cam_rt, intr, a, b, 1.0 / 300, q)
        err = np.max(np.abs(j["J"][0] - want) / np.max(np.abs(want), axis=1, keepdims=True))
        print(f"J ({a}, {b}) at {q}: {j['J'].shape[2]} columns, error {float(err):.3e} of the row's largest entry (bound {J_BOUND:.3e})")
        worst = max(worst, float(err))
        assert np.all(np.max(np.abs(want), axis=0) > 0)     # no column is idle: pose of camera 0 included (it is free in J)
    assert worst <= J_BOUND


def test_float64_restatement_is_the_same_definition():
    """e64 is the float64 run of the same code: close to the longdouble run, far from exact."""
    _, _, ref, e64, amp, tol = U.case("rig4", "67x5")
    assert 0 < U.worst(e64) < 1e-4 and tol < 1e-3


# ----------------------------------------------------------------------------- Monte Carlo
MC_N = 4000
MC_SIGMA2 = 1e-24                 # pixel deviations of 1e-12 px: second-order terms are far below the sampling error


def _monte_carlo(sigma2, n=MC_N):
    cam_rt, intr, cam_cov, _, _ = U.inputs("rig4")
    p, kw, ref, _, _ = CR.case("rig4")
    fm = ref["cam_free"].ravel()
    S = np.asarray(cam_cov, dtype=LD).reshape(60, 60)[np.ix_(fm, fm)]
    L = H._chol(S)
    assert L is not None
    z = np.random.default_rng(20260101).normal(size=(n, int(fm.sum())))
    delta = np.zeros((n, 60), LD)
    delta[:, fm] = (z.astype(LD) @ L.T) * np.sqrt(LD(sigma2))
    delta = delta.reshape(n, 4, 15)
    px, py = np.array([600.25, 215.75, 905.5]), np.array([500.5, 340.125, 610.25])
    a, b, iota = 1, 2, 1.0 / 300
    base = U.jacobian(cam_rt, intr, a, b, iota, px, py)
    d = np.zeros((n, 3, 2), LD)
    for k in range(n):
        rt = np.asarray(cam_rt, dtype=LD) + delta[k, :, :6]
        I = np.asarray(intr, dtype=LD).copy()
        I[:, :7] += delta[k, :, 6:13]
        j = U.jacobian(rt, I, a, b, iota, px, py)
        d[k, :, 0], d[k, :, 1] = j["u"] - base["u"], j["v"] - base["v"]
    emp = np.einsum("npe,npf->pef", d, d) / (n - 1)          # the mean is known to be 0 to first order
    Sth = U.sigma_theta(cam_cov, a, b)
    pred = LD(sigma2) * np.einsum("pei,ij,pfj->pef", base["J"], Sth, base["J"])
    return emp, pred


def test_monte_carlo_agrees_with_the_prediction():
    """The sampling error of a variance from N draws is sqrt(2 / (N - 1)) relative; six of those is the bound, on the two
    variances relatively and on the covariance against sqrt(c_uu c_vv).  N = 4000: 13 %."""
    bound = 6 * np.sqrt(2.0 / (MC_N - 1))
    emp, pred = _monte_carlo(MC_SIGMA2)
    for p in range(3):
        s = np.sqrt(pred[p, 0, 0] * pred[p, 1, 1])
        e = [float(abs(emp[p, 0, 0] - pred[p, 0, 0]) / pred[p, 0, 0]), float(abs(emp[p, 1, 1] - pred[p, 1, 1]) / pred[p, 1, 1]),
             float(abs(emp[p, 0, 1] - pred[p, 0, 1]) / s)]
        print(f"pixel {p}: predicted sd {float(np.sqrt(pred[p, 0, 0])):.3e} {float(np.sqrt(pred[p, 1, 1])):.3e}, empirical / predicted errors {e}, bound {bound:.3f}")
        assert max(e) <= bound
    # halving sigma2 with the same normal draws halves the empirical covariance: the draws are in the linear range
    half, _ = _monte_carlo(MC_SIGMA2 / 2, n=400)
    full, _ = _monte_carlo(MC_SIGMA2, n=400)
    lin = float(np.max(np.abs(full - 2 * half) / np.sqrt(np.einsum("pii->p", full) ** 2)[:, None, None]))
    print("linearisation: |emp(s2) - 2 emp(s2 / 2)| relative", lin)
    assert lin <= 1e-3 * bound


# ----------------------------------------------------------------------------- properties
def _planes(name="rig4", grid="67x5", **kw):
    inp = U.inputs(name)
    return inp, U.uncertainty_ref(*inp[:4], inp[4], U.grids()[grid], **kw)


def test_quadrupling_sigma2_doubles_every_sd():
    inp, one = _planes()
    four = U.uncertainty_ref(inp[0], inp[1], inp[2], 4 * inp[3], inp[4], U.grids()["67x5"])
    v = (one["flags"] & 3) == 3
    for k in (5, 6):
        x, y = one["planes"][:, k][v], four["planes"][:, k][v]
        has = ~np.isnan(x)
        assert np.array_equal(np.isnan(x), np.isnan(y)) and np.max(np.abs(y[has] - 2 * x[has]) / x[has]) < 1e-17


def test_at_infinity_the_translations_contribute_exactly_nothing():
    cam_rt, intr, cam_cov, _, _ = U.inputs("rig4")
    px, py = U.grid_pixels(U.grids()["67x5"])
    for a, b in ((0, 1), (2, 1), (3, 3)):
        j = U.jacobian(cam_rt, intr, a, b, 0.0, px, py)
        ok = j["ok1"]
        cols = [3, 4, 5] + ([16, 17, 18] if a != b else [])
        assert ok.any() and not j["J"][ok][:, :, cols].any()
        moved = np.array(cam_rt); moved[:, 3:] *= 7.0        # and the result does not depend on them at all
        j2 = U.jacobian(moved, intr, a, b, 0.0, px, py)
        assert np.array_equal(j["u"][ok], j2["u"][ok]) and np.array_equal(j["J"][ok], j2["J"][ok])


def test_a_constant_pose_contributes_nothing():
    """rig4's camera 0 has a constant pose: its pose rows of Sigma are zero, so its pose columns of J may be anything."""
    cam_rt, intr, cam_cov, sigma2, _ = U.inputs("rig4")
    assert not cam_cov[0, :6].any() and not cam_cov[:, :, 0, :6].any()
    px, py = U.grid_pixels(U.grids()["67x5"])
    for a, b in ((0, 1), (1, 0), (0, 0)):
        j = U.jacobian(cam_rt, intr, a, b, 1.0 / 300, px, py)
        S = U.sigma_theta(cam_cov, a, b)
        ok = j["ok1"]
        J = j["J"][ok]
        J0 = J.copy()
        off = 0 if (a == 0) else 13
        J0[:, :, off:off + 6] = 0
        assert np.any(J[:, :, off:off + 6] != 0)
        assert np.array_equal(np.einsum("pei,ij,pfj->pef", J, S, J), np.einsum("pei,ij,pfj->pef", J0, S, J0))
    # a mono problem: the intrinsics alone
    rt1, I1, cc1, _, _ = U.inputs("mono7")
    assert not cc1[0, :6].any() and cc1[0, 6:13, 0, 6:13].all()


def test_across_and_along_add_up_and_sd_worst_is_the_larger_eigenvalue():
    inp = U.inputs("rig4")
    grid = U.grids()["24x16"]
    for rq in inp[4]:
        r = U.request_ref(*inp[:4], rq, grid)
        v = (r["flags"] & 3) == 3
        cuu, cuv, cvv, sw, sa = (r["planes"][k][v] for k in (2, 3, 4, 5, 6))
        lam = np.array([np.linalg.eigvalsh(np.array([[x, y], [y, z]], dtype=np.float64))[1] for x, y, z in zip(cuu, cuv, cvv)])
        assert np.max(np.abs(np.asarray(sw, dtype=np.float64) ** 2 - lam) / lam) < 1e-7          # (eigvalsh is float64; c has cancellation of its own)
        assert np.all(sw ** 2 <= (cuu + cvv) * (1 + 1e-15)) and np.all(sw ** 2 >= (cuu + cvv) / 2 * (1 - 1e-15))
        if rq[0] != rq[1]:
            al = r["sd_along"][v]
            assert not np.isnan(sa).any() and np.max(np.abs(sa ** 2 + al ** 2 - (cuu + cvv)) / (cuu + cvv)) < 1e-15
            assert np.all(sa <= sw * (1 + 1e-15))
        else:
            assert np.isnan(sa).all()


def test_observe_mode_projects_the_pixel_onto_itself():
    inp = U.inputs("rig4")
    grid = U.grids()["24x16"]
    px, py = U.grid_pixels(grid)
    for m, iota in ((0, 0.0), (2, 1.0 / 300), (3, 1.0 / 5000)):
        r = U.request_ref(*inp[:4], (m, m, iota), grid)
        v = ((r["flags"] & 3) == 3).ravel()
        assert v.any() and np.array_equal(r["flags"].ravel() & 3 == 3, r["flags"].ravel() & 1 == 1)
        assert np.max(np.hypot(r["planes"][0].ravel()[v] - px[v], r["planes"][1].ravel()[v] - py[v])) < 1e-12      # pixels; the disc's rim is ill-conditioned


# ----------------------------------------------------------------------------- negative controls
@pytest.mark.parametrize("name,grid", GPU_CASES)
def test_the_tolerance_rejects_every_mistake(name, grid):
    inp, g, ref, e64, amp, tol = U.case(name, grid)
    transfers = any(a != b for a, b, _ in inp[4])
    ratios = {}
    for m in U.MISTAKES:
        if m in U.TRANSFER_ONLY and not transfers:
            continue                                        # (mono7: there is no camera a, no pair, and camera 0 starts at row 0)
        bad = U.uncertainty_ref(*inp[:4], inp[4], g, mistake=m)
        ratios[m] = U.worst(U.uncertainty_errors(bad["planes"], ref)) / tol
    print(f"{name} {grid}: e64 {U.worst(e64):.3e} amp {amp:.3e} tolerance {tol:.3e}; mistake / tolerance", {k: f"{v:.3g}" for k, v in ratios.items()})
    assert "sigma2_forgotten" in ratios and all(r > 1 for r in ratios.values()), ratios


@pytest.mark.parametrize("name,grid", GPU_CASES + [("behind", "24x16")])
def test_few_pixels_sit_on_a_threshold(name, grid):
    if name == "behind":
        inp = U.behind_inputs()
        ref = U.uncertainty_ref(*inp[:4], inp[4], U.grids()[grid])
        assert (ref["flags"] == 1).sum() >= 10               # the target camera sees these points behind it: k <= 0
    else:
        ref = U.case(name, grid)[2]
    assert ref["near"].mean() <= 0.01
    if grid in ("24x16", "wide9x7"):
        assert (ref["flags"] == 0).any() and ((ref["flags"] & 3) == 3).any()     # reaches outside the disc that unprojects


# ----------------------------------------------------------------------------- refusals
def _call(L, **over):
    cam_rt, intr, cam_cov, sigma2, _ = U.inputs("rig4")
    a = dict(n_cameras=4, cam_rt=cam_rt, intr=intr, cam_cov=cam_cov, sigma2=sigma2, grid=dict(U.grids()["67x5"]), requests=[(0, 1, 0.0), (2, 2, 1e-3)],
             n_requests=None, struct_size=C.sizeof(lib.CUncertaintyGrid), planes=True, flags=True, device=1 << 20)
    a.update(over)
    g = None if a["grid"] is None else lib.CUncertaintyGrid(struct_size=a["struct_size"], **a["grid"])
    rq = a["requests"]
    n = len(rq) if a["n_requests"] is None and rq is not None else (a["n_requests"] or 0)
    req = None if rq is None else (lib.CUncertaintyRequest * max(len(rq), 1))(*[lib.CUncertaintyRequest(*r) for r in rq])
    planes, flags = np.zeros((max(n, 1), 7, 5, 67)), np.zeros((max(n, 1), 5, 67), np.uint8)
    ptr = lambda x: None if x is None else lib.dptr(np.ascontiguousarray(x))
    return L.tscm_projection_uncertainty(a["n_cameras"], ptr(a["cam_rt"]), ptr(a["intr"]), ptr(a["cam_cov"]), a["sigma2"], None if g is None else C.byref(g), req, n,
                                         a["device"], lib.dptr(planes) if a["planes"] else None,
                                         flags.ctypes.data_as(C.POINTER(C.c_ubyte)) if a["flags"] else None, None, None)


def test_refusals_come_before_the_device():
    """Every refusal is TSCM_E_INVALID (-1) with the argument named, with a device index that does not exist (which alone is
    TSCM_E_NO_DEVICE, -2): the arguments are checked first."""
    L = lib.lib()
    msg = lambda: L.tscm_last_error().decode()
    assert _call(L) == -2
    for key in ("cam_rt", "intr", "cam_cov", "grid", "requests"):
        assert _call(L, **{key: None}) == -1 and key in msg(), key
    for key in ("planes", "flags"):
        assert _call(L, **{key: False}) == -1 and key in msg(), key
    assert _call(L, struct_size=C.sizeof(lib.CUncertaintyGrid) - 8) == -1 and "struct_size" in msg()
    g = U.grids()["67x5"]
    for key in ("nx", "ny"):
        for bad in (0, -3):
            assert _call(L, grid=dict(g, **{key: bad})) == -1 and key in msg(), key
    for bad in (0, -1):
        assert _call(L, n_requests=bad) == -1 and "n_requests" in msg()
    for key in ("dx", "dy"):
        for bad in (float("nan"), float("inf")):
            assert _call(L, grid=dict(g, **{key: bad})) == -1 and key in msg(), key
    for bad in ((4, 0, 0.0), (-1, 0, 0.0)):
        assert _call(L, requests=[(0, 1, 0.0), bad]) == -1 and "requests[1]" in msg() and "camera_a" in msg()
    for bad in ((0, 4, 0.0), (0, -1, 0.0)):
        assert _call(L, requests=[bad]) == -1 and "requests[0]" in msg() and "camera_b" in msg()
    for bad in (-1e-9, float("nan"), float("inf")):
        assert _call(L, requests=[(0, 1, bad)]) == -1 and "inv_distance" in msg()
    for bad in (-1.0, float("nan")):
        assert _call(L, sigma2=bad) == -1 and "sigma2" in msg()
    for bad in (0, 33):
        assert _call(L, n_cameras=bad) == -1 and "n_cameras" in msg()
    assert _call(L, sigma2=0.0) == -2 and _call(L, sigma2=float("inf")) == -2


def test_the_symbols_are_exported():
    assert "tscm_projection_uncertainty" in lib.EXPORTS
    assert lib.lib().tscm_abi_version() == 6
