"""CPU tests of tests/init_ref.py, the extended-precision reference of the mono initialisation (TS.cpp:110-203):
the reference against mpmath at 50 digits, the C oracle within the reference's bounds, kernel-shaped mistakes
far outside them, and the reach of the GPU case table, from the case definitions alone."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

from oracle import pyoracle as orc
from tests import init_ref as R


def _mp50_null_vector(xs, ys, cx, cy):
    with mp.workdps(50):
        A = mp.matrix([[mp.mpf(float(x)) - mp.mpf(cx), mp.mpf(float(y)) - mp.mpf(cy), mp.mpf("0.5"),
                        -((mp.mpf(float(x)) - mp.mpf(cx)) ** 2 + (mp.mpf(float(y)) - mp.mpf(cy)) ** 2) / 2] for x, y in zip(xs, ys)])
        _, S, V = mp.svd_r(A)
        j = min(range(4), key=lambda i: S[i])
        c1, c2, c3, c4 = (V[j, r] for r in range(4))
        t = c1 * c1 + c2 * c2 + c3 * c4
        if t < 0:
            return -2.0
        d = mp.sqrt(1 / t)
        nx, ny = c1 * d, c2 * d
        if nx * nx + ny * ny > mp.mpf("0.95"):
            return -2.0
        return float(abs(c3 * d / mp.sqrt(1 - nx * nx - ny * ny)))


def test_focal_reference_matches_mpmath_svd_at_50_digits():
    pu, pv, count, w, h, cx, cy, kinds = R.focal_case("w5_rows63")
    n = 0
    for k in range(4):
        if count[k] == 0:
            continue
        for i in range(h):
            xs, ys = pu[k, i * w:(i + 1) * w], pv[k, i * w:(i + 1) * w]
            r = R.focal_row(xs, ys, cx, cy)
            if np.isnan(r["value"]):
                continue
            want = _mp50_null_vector(xs, ys, cx, cy)
            if want < 0:
                assert r["value"] == -2.0
            else:
                assert abs(r["value"] - want) <= 1e-12 * want
                n += 1
    assert n > 0


def _mp50_column_pose(H):
    """lambda, M, polar factor (SVD at 50 digits) and the generic Rodrigues formula."""
    with mp.workdps(50):
        Hm = mp.matrix([[mp.mpf(float(H[i, j])) for j in range(3)] for i in range(3)])
        n1 = mp.sqrt(sum(Hm[i, 0] ** 2 for i in range(3)))
        n2 = mp.sqrt(sum(Hm[i, 1] ** 2 for i in range(3)))
        lam = 2 / (n1 + n2) * (-1 if Hm[2, 2] < 0 else 1)
        M = mp.matrix(3, 3)
        for i in range(3):
            M[i, 0], M[i, 1] = lam * Hm[i, 0], lam * Hm[i, 1]
        M[0, 2] = M[1, 0] * M[2, 1] - M[2, 0] * M[1, 1]
        M[1, 2] = M[2, 0] * M[0, 1] - M[0, 0] * M[2, 1]
        M[2, 2] = M[0, 0] * M[1, 1] - M[1, 0] * M[0, 1]
        Um, _, Vt = mp.svd_r(M)
        X = Um * Vt
        rx, ry, rz = X[2, 1] - X[1, 2], X[0, 2] - X[2, 0], X[1, 0] - X[0, 1]
        s = mp.sqrt(rx * rx + ry * ry + rz * rz) / 2
        th = mp.acos((X[0, 0] + X[1, 1] + X[2, 2] - 1) / 2)
        return np.array([float(v * th / (2 * s)) for v in (rx, ry, rz)]), np.array([float(lam * Hm[i, 2]) for i in range(3)])


def test_extrinsic_reference_matches_mpmath_at_50_digits():
    intr, pu, pv, count, W, cols, kinds = R.extrinsic_case("v12_9x6")
    n = 0
    for k in range(count.shape[0]):
        if kinds[k] != "generic":
            continue
        r = R.extrinsic_view(intr, pu[k], pv[k], W, cols)
        rv0, t0 = _mp50_column_pose(r["H"].astype(np.float64))
        # H itself is rounded to fp64 on the way to mpmath: the column step's condition (bpose0) bounds that
        assert np.all(np.abs(rv0 - r["rv0"].astype(np.float64)) <= r["bpose0"][:3])
        assert np.all(np.abs(t0 - r["t0"].astype(np.float64)) <= r["bpose0"][3:])
        # T is a rotation that turns the reference corner onto the z axis
        T = r["T"].astype(np.float64)
        assert np.max(np.abs(T @ T.T - np.eye(3))) < 1e-15
        p = R.unit_sphere(intr, pu[k, W.shape[0] // 2 - cols // 2 - 1], pv[k, W.shape[0] // 2 - cols // 2 - 1])
        q = T @ p.astype(np.float64)
        assert abs(q[0]) < 1e-15 and abs(q[1]) < 1e-15
        n += 1
    assert n >= 5


def test_oracle_focal_sample_within_reference_bounds():
    worst, n = 0.0, 0
    for name, w, h, V in R.FOCAL_SMALL:
        pu, pv, count, w, h, cx, cy, kinds = R.focal_case(name)
        for k in range(V):
            if count[k] == 0:
                continue
            for i in range(h):
                xs, ys = pu[k, i * w:(i + 1) * w], pv[k, i * w:(i + 1) * w]
                r = R.focal_row(xs, ys, cx, cy)
                g = orc.focal_sample(xs, ys, cx, cy)
                if np.isnan(r["value"]):
                    assert g is not None and np.isnan(g)
                    continue
                if not r["decisive"]:
                    continue
                if r["value"] < 0:
                    assert g is None
                    continue
                assert g is not None
                ratio = abs(g - r["value"]) / r["bound"]
                assert ratio <= 1.0, (name, k, i, ratio)
                worst, n = max(worst, ratio), n + 1
    assert n > 20
    print(f"\n[init reference] orc_focal_sample: worst |oracle - reference| / bound = {worst:.3g} over {n} samples")


def _orc_planar_pnp(W, x, y):
    L = orc.lib()
    f = L.orc_planar_pnp
    dp = C.POINTER(C.c_double)
    f.argtypes = [dp, dp, dp, C.c_int, dp, dp]
    f.restype = C.c_int
    W, x, y = (np.ascontiguousarray(a, dtype=np.float64) for a in (W, x, y))
    Rm, t = np.zeros(9), np.zeros(3)
    ok = f(W.ctypes.data_as(dp), x.ctypes.data_as(dp), y.ctypes.data_as(dp), W.shape[0], Rm.ctypes.data_as(dp), t.ctypes.data_as(dp))
    return ok, Rm.reshape(3, 3), t


def test_oracle_planar_pnp_within_reference_bounds():
    """orc_planar_pnp (central-difference Jacobian) on the reference's normalised points reaches the same minimiser."""
    worst = {}
    for name in ("v12_9x6", "v3_grazing"):
        intr, pu, pv, count, W, cols, kinds = R.extrinsic_case(name)
        for k in range(count.shape[0]):
            if count[k] == 0 or kinds[k] == "nan_pixel":
                continue
            r = R.extrinsic_view(intr, pu[k], pv[k], W, cols)
            assert r["code"] == R.CONVERGED
            q = R.unit_sphere(intr, pu[k], pv[k]) @ r["T"].T
            ok, Rm, t = _orc_planar_pnp(W, (q[:, 0] / q[:, 2]).astype(np.float64), (q[:, 1] / q[:, 2]).astype(np.float64))
            assert ok
            Rr, _ = R.rotation(r["rv"])
            # rotation compared through R (the oracle returns R), within the rv bound (|dR| <= |d rv|)
            dr = np.max(np.abs(Rm - Rr.astype(np.float64)))
            dt = np.abs(t - r["t"].astype(np.float64))
            for kind, ratio in (("R", dr / r["bpose"][:3].max()), ("t", np.max(dt / r["bpose"][3:]))):
                assert ratio <= 1.0, (name, k, kind, ratio)
                worst[kind] = max(worst.get(kind, 0.0), ratio)
    for kind, v in worst.items():
        print(f"\n[init reference] orc_planar_pnp {kind}: worst |oracle - reference| / bound = {v:.3g}")


# ------------------------------------------------------------------------------------------------ negative controls
def _focal_mistake_ratio(mistake):
    worst = 0.0
    for name, w, h, V in R.FOCAL_SMALL:
        pu, pv, count, w, h, cx, cy, kinds = R.focal_case(name)
        for k in range(V):
            if count[k] == 0:
                continue
            for i in range(h):
                xs, ys = pu[k, i * w:(i + 1) * w], pv[k, i * w:(i + 1) * w]
                r, m = R.focal_row(xs, ys, cx, cy), R.focal_row(xs, ys, cx, cy, mistake)
                if not r["decisive"] or np.isnan(r["value"]):
                    continue
                if (r["value"] < 0) != (m["value"] < 0):
                    return np.inf                                       # a marker flips
                if r["value"] > 0:
                    worst = max(worst, abs(m["value"] - r["value"]) / r["bound"])
    return worst


def _extrinsic_mistake_ratio(mistake, quantity):
    worst = 0.0
    for name in ("v12_9x6",):
        intr, pu, pv, count, W, cols, kinds = R.extrinsic_case(name)
        for k in range(count.shape[0]):
            if count[k] == 0 or kinds[k] == "nan_pixel":
                continue
            r = R.extrinsic_view(intr, pu[k], pv[k], W, cols)
            m = R.extrinsic_view(intr, pu[k], pv[k], W, cols, mistake)
            if quantity == "T":
                d = np.max(np.abs((m["T"] - r["T"]).astype(np.float64))) / r["bT"]
            elif quantity == "H":
                E = ((m["H"] - r["H"]) @ np.linalg.inv(r["Nt"].astype(np.float64))).astype(np.float64)
                d = np.max(np.abs(E)) / r["bHn"]
            elif quantity == "pose0":
                d = np.max(np.abs(np.concatenate([m["rv0"] - r["rv0"], m["t0"] - r["t0"]]).astype(np.float64)) / r["bpose0"])
            elif quantity == "pose":
                d = np.max(np.abs(np.concatenate([m["rv"] - r["rv"], m["t"] - r["t"]]).astype(np.float64)) / r["bpose"])
            else:
                scale = np.concatenate([np.full(2, r["bpose"][:3].max()), [r["bpose"][3:].max()]])
                d = np.max(np.abs((m["Rt"] - r["Rt"]).astype(np.float64)) / scale)
            worst = max(worst, float(d))
    return worst


NEGATIVE_CONTROLS = [
    ("right singular vector of the largest sigma", lambda: _focal_mistake_ratio("largest_sigma")),
    ("c3*c3 in place of c3*c4", lambda: _focal_mistake_ratio("c3c3")),
    ("reference corner n/2 - w/2 (no -1): T", lambda: _extrinsic_mistake_ratio("ref_corner", "T")),
    ("H de-normalised without the -s (h . c) shift", lambda: _extrinsic_mistake_ratio("no_denormalise_shift", "H")),
    ("r3 = r2 x r1 in the pose from the columns", lambda: _extrinsic_mistake_ratio("cross_order", "pose0")),
    ("near-pi sign rule dropped", lambda: _extrinsic_mistake_ratio("no_sign_rule", "pose0")),
    ("one Gauss-Newton parameter frozen", lambda: _extrinsic_mistake_ratio("freeze_param", "pose")),
    ("output multiplied by T instead of T^T", lambda: _extrinsic_mistake_ratio("T_not_transposed", "Rt")),
]


@pytest.mark.parametrize("name,ratio", NEGATIVE_CONTROLS, ids=[n for n, _ in NEGATIVE_CONTROLS])
def test_negative_control_exceeds_the_bound(name, ratio):
    r = ratio()
    print(f"\n[init reference] negative control '{name}': worst |mistake - reference| / bound = {r:.3g}")
    assert r >= 100.0, (name, r)


# ------------------------------------------------------------------------------------------------ coverage
def test_gpu_case_table_reaches_every_path():
    widths = {w for _, w, _, _ in R.FOCAL_CASES}
    assert {4, 5, 31, 32} <= widths and R.MAX_WIDTH == 32          # 33 is refused (test_gpu_init_stages)
    rows = [V * h for _, _, h, V in R.FOCAL_CASES]
    assert any(r % 64 == 63 for r in rows) and any(r % 64 == 0 for r in rows) and any(r % 64 == 1 for r in rows)
    views = [c[1] for c in R.EXTRINSIC_CASES]
    assert 63 in views and 64 in views and 65 in views
    # focal rows: images without a board between boards, the 0.95 rule decisively both ways, a NaN row
    seen = set()
    for name, w, h, V in R.FOCAL_CASES:
        pu, pv, count, w, h, cx, cy, kinds = R.focal_case(name)
        assert any(count[k] == 0 and 0 < k < V - 1 for k in range(V)), name
        for k in range(V):
            for i in range(h):
                kind = kinds[k][i]
                if kind in ("far_arc", "near_arc", "nan") and kind not in seen:
                    r = R.focal_row(pu[k, i * w:(i + 1) * w], pv[k, i * w:(i + 1) * w], cx, cy)
                    if kind == "nan":
                        assert np.isnan(r["value"])
                    else:
                        assert r["decisive"] and (r["value"] == -2.0) == (kind == "far_arc"), (name, k, i, r)
                    seen.add(kind)
    assert seen == {"far_arc", "near_arc", "nan"}
    # extrinsic views: every exit code but ZERO_COLUMN (see init_ref), both Rodrigues branches, the sign rule with
    # X[5] of both signs, theta within 1e-6 of pi, boards of more than 64 points
    codes, branches, x5, close_to_pi = set(), set(), set(), False
    for name, V, cols, rows_, scale, kind in R.EXTRINSIC_CASES:
        refs = R.extrinsic_refs(name)
        if cols * rows_ > 64:
            assert any(r["code"] == R.CONVERGED for r in refs)
        for r in refs:
            if r["decisive_code"]:
                codes.add(r["code"])
            rod = r.get("rod")
            if rod is not None and r.get("rod_decisive"):
                branches.add(rod["branch"])
                if rod["branch"] == "pi":
                    close_to_pi |= bool(np.pi - float(mp.acos(rod["c"])) < 1e-6)
                    if rod["sign_rule"]:
                        x5.add(bool(rod["x5"] > 0))
    assert {R.NO_BOARD, R.DEGENERATE_BOARD, R.DLT_FAILED, R.CONVERGED, R.GN_CHOLESKY} <= codes, codes
    assert {"identity", "pi", "generic"} <= branches and x5 == {True, False} and close_to_pi
    assert max(c[2] * c[3] for c in R.EXTRINSIC_CASES) > 64
