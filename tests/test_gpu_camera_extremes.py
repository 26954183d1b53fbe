"""Every evaluation kernel against the extended-precision camera model on the fan problems (tests/fan_problems.py):
incidence 0 .. 170 degrees, Double Sphere, UCM, pinhole limit, alpha = 0.9, xi > 0, alpha < 0, free cameras and boards
with rotation vectors of length 0, 1e-9, 1.2e-8, 1.6e-8 (both sides of theta^2 = DBL_EPSILON), 1e-4 and next to pi, a
corner exactly on the optical axis, a board exactly in the plane Z = 0, single-corner views, outliers of 25 px.

Reference: tests/camera_ref.py (np.longdouble, dual numbers; against mpmath in tests/test_camera_reference.py).
Bound: K cond 2^-53 with K = 8 K_ORACLE = 80 (K_ORACLE: what the fp64 oracle needs, test_camera_reference.py) and
cond = cond_ext of the view's worst corner, plus the rotation's own term in the columns of a Rodrigues rotation
(fan_problems.column_cond); the margin of 8 is for the device's operation order, its FMAs and its 2-ulp square roots in
a chain of three.
  tscm_eval_functor                   residuals and the three Jacobians per corner (fan_problems.row_ratios); -X / k = -Y / k = 0
                                      exactly on the optical axis
  tscm_eval_normal_equations_ex       k_eval_gram4 per entry in Cauchy-Schwarz units (fan_problems.gram_ratios);
                                      TSCM_EXEC_GRAM_16X16 the same bits; jacobian_fp32 within TOL_F32 max(1, cond);
                                      cost within 1e-13 max cond
  tscm_eval_normal_equations_robust   Huber, soft-L1, Cauchy at 1 px against rows scaled by sqrt(rho') in longdouble, the same
                                      bound times the weight's own amplification (fan_problems.robust_weights)
  rotation cases                      camera-pose and board-pose columns apart, and for the three lengths around DBL_EPSILON
                                      the device is closer to the branch the reference took than to the other one
  tscm_project_points / tscm_unproject_pixels (skewed set, to 170 degrees), tscm_reprojection_error (1e-12 per camera),
  tscm_solve_mono_batch with max_num_iterations = 0 (k_mb_eval: initial_cost within 1e-13 max cond)

Measured on an MI355X, largest ratio to cond 2^-53 over all nine fan problems (bound: 80):
  tscm_eval_functor     camera rotation 2.2, camera translation 2.4, board rotation 3.5, board translation 2.1, fx fy 2.7,
                        cx cy 0 (exact), xi lambda alpha 2.8, residual 0.62
                        by lens set: calibrated 2.2, DS 1.7, UCM 1.7, pinhole 2.3, large alpha 3.5, positive xi 2.7,
                        negative alpha 1.9, skewed 1.3
  k_eval_gram4          view_cross 7.9, board_gram 19, board_grad 0.24, cam_gram 0.63, cam_grad 0.072
                        by lens set: calibrated 5.4, DS 5.0, UCM 3.2, pinhole 3.8, large alpha 19, positive xi 5.6,
                        negative alpha 1.9, skewed 2.8;  k_eval_gram: the same bits
  robust k_eval_gram4   Huber 5.4, soft-L1 1.6, Cauchy 1.2 (with the weight's amplification, up to 7,300; without it up to 650)
  k_eval_gram_f32       0.11 of TOL_F32 max(1, cond) (view_cross 0.029, board_gram 0.11): the figure of test_gpu_gram_kernels.py
                        carries over
  rotation cases        |w| = 0: 2.2 / 3.8 (functor / gram4), 1e-9: 1.6 / 3.5, 1.2e-8: 1.9 / 4.8, 1.6e-8: 0.2 / 1.2 (of a bound
                        that holds rotation_cond = 6e7 there), 1e-4: 0.3 / 2.2, next to pi: 2.2 / 7.9; the other branch is
                        at least 9 x (functor) and 4.9 x (gram4) further away than the branch taken
  tscm_project_points 0.9, tscm_unproject_pixels 1.9; tscm_reprojection_error 6.3e-15 relative; tscm_solve_mono_batch's
  initial_cost 5.4e-16 relative

One finding, explained from the code and left as it is: the t_b x t_b block of a board's E^T E is not accumulated but derived
after the sum, R_c^T (sum n n^T) R_c (tscm_geometry.h: store_view_record rotates the rows, tb_tb the columns).  Where a
view's rays run next to an axis of the rig frame the diagonal entry of that axis is a small difference of the sum's large
entries, and rotating the sum squares the amplification |n| / |n_l| that rotating each row (the oracle, the functor) has
once: before the condition number carried cond_rig, k_eval_gram4 stood at 98 (alpha = 0.9, behind a camera rotated by
pi - 1e-6) where the oracle stood at 7; a CPU emulation of the rotated sum in fp64 gives 74 on the same data.  With cond_rig
the oracle is at 3.9 there and the kernel at 19.  The block's error stays at 2^-53 of the block's norm.
"""
import numpy as np
import pytest

from tscm_calib_amd import api, lib
from tests import camera_ref as R
from tests import fan_problems as F
from tests import helpers as H
from tests.test_camera_reference import K, K_ORACLE, projection_ratios
from tests.test_gpu_gram_kernels import TOL_F32

assert K == 8 * K_ORACLE and K <= 1000

pytestmark = pytest.mark.gpu
KEYS = ("board_gram", "board_grad", "view_cross", "cam_gram", "cam_grad")


def _fmt(d):
    return ", ".join(f"{k} {v:.2g}" for k, v in d.items())


def _by_lens(p, ref, per_corner):
    lens = p.meta["view_lens"][ref["view"]]
    return {l: float(per_corner[lens == l].max()) for l in p.meta["lenses"]}


@pytest.mark.parametrize("name", F.NAMES)
def test_functor_rows(hip_device, name):
    p, ref = F.fan_problem(name), F.reference(name)
    cost, res, Jc, Jb, Ji = api.evaluate_functor(p, hip_device)
    rows = F.row_ratios(p, ref, res, Jc, Jb, Ji)
    worst = {k: float(v.max()) for k, v in rows.items()}
    print(f"\n[extremes] functor {name}: {_fmt(worst)}; by lens {_fmt(_by_lens(p, ref, np.max(np.stack(list(rows.values())), axis=0)))}")
    assert max(worst.values()) <= K, worst
    assert not Ji[:, :, 7:].any()              # (a mono problem's Jc is that of an identity camera: no such block, not compared)
    want = 0.5 * float(np.sum(ref["res"] ** 2))
    assert abs(cost - want) <= 1e-13 * ref["cond_view"].max() * want
    axis = np.nonzero((ref["Pc"][:, 0] == 0) & (ref["Pc"][:, 1] == 0))[0]
    if p.mono or not p.cam_rt[0].any():
        assert axis.size, "the exact on-axis view is missing"
    for i in axis:
        assert Ji[i, 0, 0] == 0.0 and Ji[i, 1, 1] == 0.0 and Ji[i, 0, 4:7].tolist() == [0.0] * 3 and Ji[i, 1, 4:7].tolist() == [0.0] * 3
        assert res[i, 0] == p.obs_u[p.view_offset[ref["view"][i]]] - p.intr[p.view_camera[ref["view"][i]], 2]


@pytest.mark.parametrize("name", F.NAMES)
def test_gram_kernels(hip_device, name):
    p, ref = F.fan_problem(name), F.reference(name)
    o = F.reference_normal_equations(p, ref)
    g = api.normal_equations(p, hip_device)
    g16 = api.normal_equations(p, hip_device, exec_flags=lib.EXEC_GRAM_16X16)
    g32 = api.normal_equations(p, hip_device, jacobian_fp32=1)
    r64 = F.gram_ratios(p, ref, g, o)
    r32 = F.gram_ratios(p, ref, g32, o, unit=TOL_F32)
    w64, w32 = {k: float(v.max()) for k, v in r64.items()}, {k: float(v.max()) for k, v in r32.items()}
    lens_of = dict(view_cross=p.meta["view_lens"], board_gram=p.meta["view_lens"])
    by_lens = {l: float(max(r64[k][lens_of[k] == l].max() for k in lens_of)) for l in p.meta["lenses"]}
    print(f"\n[extremes] gram4 {name}: {_fmt(w64)}; by lens {_fmt(by_lens)}\n[extremes] fp32 tier {name} (units of TOL_F32 max(1, cond)): {_fmt(w32)}")
    assert max(w64.values()) <= K, w64
    for key in KEYS + ("cost",):
        assert np.array_equal(g16[key], g[key]), key
    if max(w32.values()) > 1.0:
        v = r32["view_cross"]
        for i in np.argsort(-v)[:8]:
            print(f"[extremes]   view {i}: {v[i]:.2f} lens {p.meta['view_lens'][i]} kind {p.meta['view_kind'][i]} angle {p.meta['view_angle'][i]} cond {ref['cond_view'][i]:.1f} corners {p.view_count[i]}")
    assert max(w32.values()) <= 1.0, w32
    cmax = ref["cond_view"].max()
    assert abs(g["cost"] - o["cost"]) <= 1e-13 * cmax * o["cost"] and abs(g32["cost"] - o["cost"]) <= 1e-13 * cmax * o["cost"]


@pytest.mark.parametrize("kind", ["huber", "soft_l1", "cauchy"])
@pytest.mark.parametrize("name", F.NAMES)
def test_robust_gram_kernels(hip_device, name, kind):
    p, ref = F.fan_problem(name), F.reference(name)
    w, cost, amp, s = F.robust_weights(p, ref, kind, 1.0)
    assert not (np.abs(np.asarray(s, dtype=np.float64) - 1.0) <= 1e-9).any()          # no corner on Huber's knee
    assert (s > 1).any() and (s < 1).any()
    o = F.reference_normal_equations(p, ref, weights=w)
    g = api.normal_equations(p, hip_device, loss=(kind, 1.0))
    r = F.gram_ratios(p, ref, g, o, weights=w, amplify=amp)
    plain = F.gram_ratios(p, ref, g, o, weights=w)
    worst = {k: float(v.max()) for k, v in r.items()}
    print(f"\n[extremes] robust {kind} {name}: {_fmt(worst)}; without the weight's amplification (up to {amp.max():.0f}) {_fmt({k: float(v.max()) for k, v in plain.items()})}")
    assert max(worst.values()) <= K, worst          # (TSCM_EXEC_GRAM_16X16 has no robust kernel: TSCM_E_UNSUPPORTED)
    assert abs(g["cost"] - cost) <= 1e-13 * ref["cond_view"].max() * cost


def _rot_err(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


@pytest.mark.parametrize("name", ["2x2-A", "9x6-A", "9x6-B", "11x8-B", "9x6-mono"])
def test_rotation_cases(hip_device, name):
    """Camera-pose and board-pose columns apart, by rotation case; and around DBL_EPSILON the branch: the device's
    columns of that rotation are at least twice as close to the branch the reference took as to the other branch
    (|w| = 1e-9 and 1.2e-8: p + w x p; 1.6e-8: Rodrigues, whose fp64 form is 1e-9 off where the other branch is 8e-9 off)."""
    p, ref = F.fan_problem(name), F.reference(name)
    cost, res, Jc, Jb, Ji = api.evaluate_functor(p, hip_device)
    rows = F.row_ratios(p, ref, res, Jc, Jb, Ji)
    g = api.normal_equations(p, hip_device)
    o = F.reference_normal_equations(p, ref)
    ent = H.gram_entry_errors(g, o, p)
    cE, cF, _ = F.column_cond(p, ref)
    # the other branch for |w| <= 1.2e-8 (threshold below 1e-18) and for |w| = 1.6e-8 (threshold above 2.56e-16)
    other = {1: R.evaluate(p, eps_cam=1e-19, eps_board=1e-19), 2: None, 3: R.evaluate(p, eps_cam=3e-16, eps_board=3e-16)}
    other[2] = other[1]
    length = [float(np.linalg.norm(F.rotation_vector(i))) for i in range(len(F.ROTATION_LENGTHS))]
    view = ref["view"]
    seen = set()
    for side, w_of_view, block, J, key in (("camera", None if p.mono else np.linalg.norm(p.cam_rt[p.view_camera, :3], axis=1), "cam_rot", Jc, "Jc"),
                                           ("board", np.linalg.norm(p.board_rt[p.view_board, :3], axis=1), "board_rot", Jb, "Jb")):
        if w_of_view is None:
            continue
        for i, L in enumerate(length):
            vs = np.nonzero(w_of_view == L)[0]
            if not vs.size:
                continue
            seen.add((side, i))
            corners = np.isin(view, vs)
            worst = float(rows[block][corners].max())
            # the Gram kernel's columns of this rotation: rows 0-2 of view_cross for a board, columns 0-2 for a camera
            e = ent["view_cross"][vs]
            c = np.maximum(cE[vs][:, :, None], cF[vs][:, ent["columns"]][:, None, :])
            gw = float((e[:, :3, :] / (c[:, :3, :] * F.U)).max()) if side == "board" else float((e[:, :, :3] / (c[:, :, :3] * F.U)).max())
            print(f"[extremes] {name} {side} |w| = {L:.3g}: functor {worst:.2g}, gram4 {gw:.2g} x cond 2^-53")
            assert worst <= K and gw <= K, (side, L, worst, gw)
            small = bool((ref["small_cam"] if side == "camera" else ref["small_board"])[corners].all())
            assert small == (L * L <= R.DBL_EPSILON)
            if i in other:
                taken = _rot_err(J[corners][:, :, :3], ref[key][corners][:, :, :3])
                wrong = _rot_err(J[corners][:, :, :3], other[i][key][corners][:, :, :3])
                oo = F.reference_normal_equations(p, ref, rows=(other[i]["res"], other[i]["Jc"], other[i]["Jb"], other[i]["Ji"]))
                eo = H.gram_entry_errors(g, oo, p)["view_cross"][vs]              # Cauchy-Schwarz units, as e
                # this rotation's entries against the other side's translation and intrinsic columns (not its rotation's)
                gt, gwr = (float(x[:, :3, (0 if p.mono else 3):].max()) if side == "board" else float(x[:, 3:, :3].max()) for x in (e, eo))
                print(f"[extremes]     functor: to the branch taken {taken:.2g}, to the other {wrong:.2g}; gram4: {gt:.2g}, {gwr:.2g}")
                assert 2 * taken <= wrong and 2 * gt <= gwr, (side, L, taken, wrong, gt, gwr)
    assert {i for s, i in seen if s == "board"} == set(range(len(length)))
    if not p.mono:
        assert len({i for s, i in seen if s == "camera"}) == 4


def test_projection_and_unprojection_with_skew(hip_device):
    p, ref = F.fan_problem("9x6-B"), F.reference("9x6-B")
    mine = np.nonzero((p.meta["view_lens"] == "skewed")[ref["view"]])[0]
    I = F.LENS["skewed"]
    assert I[7] != 0 and I[8] != 0
    P = np.ascontiguousarray(np.asarray(ref["Pc"][mine], dtype=np.float64))
    ang = np.degrees(np.arccos(P[:, 2] / np.linalg.norm(P, axis=1)))
    assert ang.max() > 169.0 and ang.min() < 2.0 and (P[:, 2] < 0).any()
    pr, ur = projection_ratios(I, P, api.project(I, P, hip_device), lambda px: api.unproject(I, px, hip_device))
    print(f"\n[extremes] tscm_project_points {pr.max():.2g}, tscm_unproject_pixels {ur.max():.2g} x cond 2^-53 ({len(P)} points)")
    assert pr.max() <= K and ur.max() <= K


@pytest.mark.parametrize("name", ["9x6-A", "9x6-B", "2x2-B", "11x8-mono"])
def test_reprojection_error(hip_device, name):
    p, ref = F.fan_problem(name), F.reference(name)
    vc = p.view_camera[ref["view"]]
    I = np.asarray(p.intr, dtype=np.longdouble)[vc]
    X, Y, k = ref["Pc"][:, 0], ref["Pc"][:, 1], ref["k"]
    u = I[:, 0] * X / k + I[:, 7] * Y / k + I[:, 2]
    v = I[:, 8] * X / k + I[:, 1] * Y / k + I[:, 3]
    _, _, at = R.corner_index(p)
    e = np.sqrt((p.obs_u[at] - u) ** 2 + (p.obs_v[at] - v) ** 2)
    per, glob, rmse = api.reprojection_error(p, hip_device)
    want = np.array([float(np.mean(e[vc == m])) for m in range(p.n_cameras)])
    err = np.abs(per - want) / want
    print(f"\n[extremes] reprojection error {name}: per camera {want}, relative error {err}")
    assert (err <= 1e-12).all(), err
    assert abs(glob - float(np.mean(e))) <= 1e-12 * float(np.mean(e))


@pytest.mark.parametrize("name", [n for n in F.NAMES if n.endswith("mono")])
def test_mono_batch_initial_cost(hip_device, name):
    """k_mb_eval on the fan geometry: Z <= 0, Z = 0 exactly, a corner on the optical axis."""
    p, ref = F.fan_problem(name), F.reference(name)
    q = p.copy().normalised()
    (conv, s), = api.refinement_batch([q], hip_device, max_num_iterations=0)
    want = 0.5 * float(np.sum(ref["res"] ** 2))
    print(f"\n[extremes] mono batch {name}: initial_cost {s['initial_cost']!r}, reference {want!r}, relative error {abs(s['initial_cost'] - want) / want:.2g}")
    assert s["num_iterations"] == 0 or len(s["iterations"]) == 1
    assert abs(s["initial_cost"] - want) <= 1e-13 * ref["cond_view"].max() * want
    assert np.array_equal(q.intr, p.intr) and np.array_equal(q.board_rt, p.board_rt)
