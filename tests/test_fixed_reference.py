"""Held intrinsics without a GPU: the extended-precision reference step with a column mask, the Double Sphere / UCM
conversions and the parsing of the masks the Python layer takes.

The GPU tests of the feature (tests/test_gpu_fixed.py) compare the solver's first step with held intrinsics against
helpers.reference_step(p, cols=masked).  That reference eliminates the boards (Schur complement) as the solver does; here
it is checked against the plainest statement of a held coordinate in Ceres' SubsetManifold: the full damped normal
equations in np.longdouble with the held columns deleted, solved directly.
"""
import numpy as np
import pytest

from tscm_calib_amd import calib_io, lib, synth
from tests import helpers as H


def masked_columns(p, fixed):
    """helpers.step_columns with the intrinsics of `fixed` ([C] mask words) held."""
    cols = H.step_columns(p)
    cf = cols["cam_free"].copy()
    for m, w in enumerate(fixed):
        for k in range(H.N_INTR_FREE):
            if (int(w) >> k) & 1:
                cf[m, 6 + k] = False
    cols["cam_free"] = cf
    return cols


def direct_step(p, cols, radius=1e4, lo=1e-6, hi=1e32):
    """The first LM step on the full system [cameras x 13 | boards x 6] with the held and constant columns deleted: Jacobi
    scaling and LM diagonal of the kept columns, one Cholesky of the whole damped matrix, no elimination."""
    t = H.step_terms(p)
    ld = t["EE"].dtype
    C, B, W = p.n_cameras, p.n_boards, H.CAM_W
    n = C * W + 6 * B
    A = np.zeros((n, n), ld)
    g = np.zeros(n, ld)
    vc, vb = np.asarray(p.view_camera), np.asarray(p.view_board)
    for v in range(p.n_views):
        if p.view_count[v] <= 0:
            continue
        c0, b0 = W * vc[v], C * W + 6 * vb[v]
        A[c0:c0 + W, c0:c0 + W] += t["FF"][v]
        A[b0:b0 + 6, b0:b0 + 6] += t["EE"][v]
        A[b0:b0 + 6, c0:c0 + W] += t["EF"][v]
        A[c0:c0 + W, b0:b0 + 6] += t["EF"][v].T
        g[c0:c0 + W] += t["Fr"][v]
        g[b0:b0 + 6] += t["Er"][v]
    keep = np.concatenate([cols["cam_free"].ravel(), np.repeat(cols["board_free"], 6)])
    A, g = A[np.ix_(keep, keep)], g[keep]
    d = np.diagonal(A).copy()
    s = 1 / (1 + np.sqrt(d))
    As = s[:, None] * A * s[None, :]
    As[np.arange(len(d)), np.arange(len(d))] += np.clip(s * s * d, ld.type(lo), ld.type(hi)) / ld.type(radius)
    L = H._chol(As)
    y = H._chol_solve(L, s * g)
    full = np.zeros(n, ld)
    full[keep] = -s * y
    return full[:C * W].reshape(C, W), full[C * W:].reshape(B, 6)


MASKS = {
    "ds": lambda C: np.full(C, lib.MODEL_DS, np.uint16),
    "ucm": lambda C: np.full(C, lib.MODEL_UCM, np.uint16),
    "cx_cy": lambda C: np.full(C, lib.FIX["cx"] | lib.FIX["cy"], np.uint16),
    "last_cam_all": lambda C: np.array([lib.FIX_INTRINSICS if m == C - 1 else 0 for m in range(C)], np.uint16),
    "per_camera": lambda C: np.array([(1 << (m % 7)) | (lib.FIX["alpha"] if m % 2 else 0) for m in range(C)], np.uint16),
}


@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("prob", ["ring3", "mono"])
def test_masked_reference_is_the_direct_solve(prob, mask):
    p = (synth.make_problem(3, 4, 3) if prob == "ring3" else synth.make_problem(1, 6, 20241)).normalised()
    fixed = MASKS[mask](p.n_cameras)
    cols = masked_columns(p, fixed)
    ref = H.reference_step(p, cols=cols)
    assert ref["ok"]
    dc, db = direct_step(p, cols)
    scale = max(float(np.max(np.abs(dc))), 1e-300)
    assert np.max(np.abs(np.asarray(ref["cam"] - dc, dtype=np.float64))) <= 1e-9 * scale
    bscale = max(float(np.max(np.abs(db))), 1e-300)
    assert np.max(np.abs(np.asarray(ref["board"] - db, dtype=np.float64))) <= 1e-9 * bscale
    # held columns do not move; the free ones do
    held = ~cols["cam_free"] & H.step_columns(p)["cam_free"]
    assert held.any() and np.all(np.asarray(ref["cam"])[held] == 0)
    assert np.all(np.asarray(ref["cam"])[cols["cam_free"]] != 0)


def _rays(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d[:, 2] = np.abs(d[:, 2]) + 0.3             # in front of the camera, up to ~70 degrees off axis
    return d * rng.uniform(200.0, 2000.0, size=(n, 1))


def _usenko_ds(ds, P):
    fx, fy, cx, cy, xi, al = ds
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    d1 = np.sqrt(x * x + y * y + z * z)
    d2 = np.sqrt(x * x + y * y + (xi * d1 + z) ** 2)
    den = al * d2 + (1 - al) * (xi * d1 + z)
    return fx * x / den + cx, fy * y / den + cy


def _usenko_ucm(ucm, P):
    fx, fy, cx, cy, al = ucm
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    d = np.sqrt(x * x + y * y + z * z)
    den = al * d + (1 - al) * z
    return fx * x / den + cx, fy * y / den + cy


@pytest.mark.parametrize("cam", range(4))
def test_double_sphere_and_ucm_conversions(cam):
    intr = synth.rig(4)[0][cam].copy()
    P = _rays(500, cam)
    ds_intr = intr.copy(); ds_intr[5] = 0.0
    u, v, _ = synth.ts_project(ds_intr, P)
    du, dv = _usenko_ds(calib_io.to_double_sphere(ds_intr), P)
    assert np.max(np.abs(du - u) / np.abs(u)) <= 1e-12 and np.max(np.abs(dv - v) / np.abs(v)) <= 1e-12
    ucm_intr = ds_intr.copy(); ucm_intr[4] = 0.0
    u, v, _ = synth.ts_project(ucm_intr, P)
    uu, uv = _usenko_ucm(calib_io.to_ucm(ucm_intr), P)
    assert np.max(np.abs(uu - u) / np.abs(u)) <= 1e-12 and np.max(np.abs(uv - v) / np.abs(v)) <= 1e-12
    # batched
    assert calib_io.to_double_sphere(np.stack([ds_intr, ds_intr])).shape == (2, 6)
    assert calib_io.to_ucm(np.stack([ucm_intr] * 3)).shape == (3, 5)


def test_conversions_refuse_other_models():
    intr = synth.rig(4)[0][0].copy()                    # lambda != 0
    with pytest.raises(ValueError):
        calib_io.to_double_sphere(intr)
    intr[5] = 0.0
    with pytest.raises(ValueError):                     # xi != 0
        calib_io.to_ucm(intr)
    intr[7] = 1e-3
    with pytest.raises(ValueError):                     # skew
        calib_io.to_double_sphere(intr)
    with pytest.raises(ValueError):
        calib_io.to_double_sphere(np.zeros(7))


def test_mask_parsing():
    f = lib.fixed_masks
    assert f(None, 3).tolist() == [0, 0, 0] and f(None, 3).dtype == np.uint16
    assert f(("cx", "cy"), 2).tolist() == [12, 12]
    assert f("lambda", 1).tolist() == [lib.MODEL_DS]
    assert f(["xi", "lambda"], 2).tolist() == [lib.MODEL_UCM] * 2
    assert f(lib.FIX_INTRINSICS, 2).tolist() == [127, 127]
    assert f(np.array([0, 3, 511]), 3).tolist() == [0, 3, 511]
    b = np.zeros((2, 9), bool); b[0, 5] = True; b[1, :7] = True
    assert f(b, 2).tolist() == [32, 127]
    assert [lib.FIX[n] for n in lib.INTRINSIC_NAMES] == [1, 2, 4, 8, 16, 32, 64, 128, 256]


@pytest.mark.parametrize("bad", [("cz",), "focal", np.array([512]), np.array([-1]), np.array([1, 2]), np.zeros((1, 7), bool),
                                 np.zeros((1,), float), 1024])
def test_mask_parsing_refuses(bad):
    with pytest.raises(ValueError):
        lib.fixed_masks(bad, 1)


def test_pipeline_models():
    from tscm_calib_amd import pipeline
    assert pipeline._model_masks("ts", None, 2).tolist() == [0, 0]
    assert pipeline._model_masks("ds", None, 2).tolist() == [lib.MODEL_DS] * 2
    assert pipeline._model_masks("ucm", ("cx", "cy"), 1).tolist() == [lib.MODEL_UCM | 12]
    with pytest.raises(ValueError):
        pipeline._model_masks("kb4", None, 1)
    intr = np.tile(synth.rig(4)[0][:1], (2, 1))
    pipeline._start_in_model(intr, "ucm")
    assert np.all(intr[:, 4:6] == 0.0) and np.all(intr[:, 6] != 0.0)
