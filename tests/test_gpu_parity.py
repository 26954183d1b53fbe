"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle.

Tolerances: the whole path is fp64; north_star asks for 1e-6 relative on intrinsics,
extrinsics and RMSE.  Per-corner quantities are held to ~1e-11.
"""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import api, lib, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _cmp_trace(gs, os_, rtol=1e-6):
    assert gs["termination_type"] == os_["termination_type"], (gs["message"], os_["message"])
    assert gs["message"] == os_["message"]
    assert gs["num_iterations"] == os_["num_iterations"]
    for a, b in zip(gs["iterations"], os_["iterations"]):
        assert a["iteration"] == b["iteration"]
        assert a["step_is_successful"] == b["step_is_successful"]
        assert abs(a["cost"] - b["cost"]) <= rtol * abs(b["cost"])
        assert abs(a["trust_region_radius"] - b["trust_region_radius"]) <= 1e-4 * abs(b["trust_region_radius"])


def test_native_library_is_loaded(hip_device):
    from tscm_calib_amd import lib
    assert lib.lib().tscm_abi_version() == 6
    assert lib.lib().tscm_device_count() >= 1


# ------------------------------------------------------------------ camera model KATs
def test_project_unproject_kat(hip_device):
    import json, os
    kat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "kat_ts.json")))
    intr = np.array(kat["intrinsics"] + [0.0, 0.0])
    P = np.array([c["P"] for c in kat["project"]])
    uv = api.project(intr, P)
    exp = np.array([[float(c["u"]), float(c["v"])] for c in kat["project"]])
    assert np.max(np.abs(uv - exp) / np.abs(exp)) < 1e-13
    rays = api.unproject(intr, exp)
    unit = P / np.linalg.norm(P, axis=1, keepdims=True)
    assert np.max(np.abs(rays - unit)) < 1e-12


def test_project_with_skew_matches_oracle(hip_device):
    rng = np.random.default_rng(3)
    intr = synth.CALIB_INTR[1].copy()
    intr[7], intr[8] = 0.8, -0.6
    P = rng.normal(size=(257, 3)) * [300, 300, 200] + [0, 0, 400]
    uv = api.project(intr, P)
    exp = np.array([orc.project(intr, p) for p in P])
    assert np.max(np.abs(uv - exp)) < 1e-9
    back = api.unproject(intr, uv)
    expb = np.array([orc.unproject(intr, q) for q in exp])
    assert np.max(np.abs(back - expb)) < 1e-11


# ------------------------------------------------------------------ functor / Jacobian
@pytest.mark.parametrize("kind", ["mono", "multi"])
def test_functor_residuals_and_jacobians(hip_device, kind):
    p = synth.make_config(1) if kind == "mono" else H.small_rig(4, 6, seed=11)
    cost, res, Jc, Jb, Ji = api.evaluate_functor(p)
    ocost, ores, oJc, oJb, oJi = orc.evaluate(p, jets=True)
    assert res.shape == ores.shape
    assert np.max(np.abs(res - ores)) < 1e-9          # pixels
    assert abs(cost - ocost) <= 1e-12 * ocost
    scale = lambda J: np.maximum(np.abs(J).max(axis=(0, 1), keepdims=True), 1e-300)
    assert np.max(np.abs(Jb - oJb) / scale(oJb)) < 1e-11
    assert np.max(np.abs(Ji - oJi) / scale(oJi)) < 1e-11
    if kind == "multi":
        assert np.max(np.abs(Jc - oJc) / scale(oJc)) < 1e-11


def test_functor_small_angle_branch(hip_device):
    """Board / camera rotations at and around the AngleAxisRotatePoint threshold
    (theta^2 <= DBL_EPSILON uses pt + w x pt; camera 0 is exactly zero)."""
    p = H.small_rig(4, 4, seed=5)
    p.board_rt[0, :3] = 0.0
    p.board_rt[1, :3] = [1e-9, -2e-9, 5e-10]
    p.board_rt[2, :3] = [1.2e-8, 0.0, 0.0]        # theta^2 = 1.44e-16 < eps
    p.board_rt[3, :3] = [1.6e-8, 0.0, 0.0]        # theta^2 = 2.56e-16 > eps
    cost, res, Jc, Jb, Ji = api.evaluate_functor(p)
    ocost, ores, oJc, oJb, oJi = orc.evaluate(p, jets=True)
    assert np.max(np.abs(res - ores)) < 1e-8
    for J, oJ in ((Jc, oJc), (Jb, oJb), (Ji, oJi)):
        s = np.maximum(np.abs(oJ).max(axis=(0, 1), keepdims=True), 1e-300)
        assert np.max(np.abs(J - oJ) / s) < 1e-9


@pytest.mark.parametrize("kind", ["mono", "multi"])
def test_normal_equations(hip_device, kind):
    """MFMA Gram tiles (E^T E, E^T F, F^T F, J^T r) against dense numpy products of the
    oracle's autodiff Jacobian."""
    p = synth.make_config(1) if kind == "mono" else H.small_rig(4, 10, seed=3)
    g = api.normal_equations(p)
    o = H.oracle_normal_equations(p)
    assert abs(g["cost"] - o["cost"]) <= 1e-12 * o["cost"]
    for key in ("board_gram", "board_grad", "cam_gram", "cam_grad", "view_cross"):
        a, b = g[key], o[key].copy()
        if key == "view_cross":
            b[:, :, 13:] = 0.0              # b, c columns are structurally zero
            if kind == "mono":
                b[:, :, :6] = 0.0
                a = a.copy(); a[:, :, :6] = 0.0
        if key in ("cam_gram", "cam_grad") and kind == "mono":
            a = a.copy(); b = b.copy()
            if key == "cam_gram":
                a[:, :6, :] = 0; a[:, :, :6] = 0; b[:, :6, :] = 0; b[:, :, :6] = 0
            else:
                a[:, :6] = 0; b[:, :6] = 0
        s = np.abs(b).max()
        assert np.max(np.abs(a - b)) <= 1e-11 * s, key


# ------------------------------------------------------------------ LM solves
def _solve_both(p, **opts):
    pg, po = p.copy().normalised(), p.copy().normalised()
    with api.Solver(pg) as s:
        gs = s.solve(**opts)
    os_ = orc.solve(po, **opts)
    return pg, po, gs, os_


def test_lm_mono_config1(hip_device):
    """BASELINE config 1: single fisheye, 20 views (TS.cpp:247-282 path)."""
    p = synth.make_config(1)
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_)
    e = H.param_rel_err(pg, po)
    assert e["intr"] < 1e-6 and e["board_rt"] < 1e-6, e
    assert abs(gs["rmse"] - orc.rmse(po)) <= 1e-6 * orc.rmse(po)
    assert gs["termination"] == "CONVERGENCE"
    # b, c inert and returned unchanged
    assert np.all(pg.intr[:, 7:] == p.intr[:, 7:])


def test_lm_mono_zero_noise(hip_device):
    p = synth.make_problem(1, 20, 99, noise_px=0.0)
    pg, po, gs, os_ = _solve_both(p)
    assert gs["rmse"] < 1e-4 and orc.rmse(po) < 1e-4
    costs = [it["cost"] for it in gs["iterations"] if it["step_is_successful"]]
    assert all(b <= a for a, b in zip(costs, costs[1:]))


def test_lm_multi_small(hip_device):
    p = H.small_rig(4, 30, seed=21)
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_)
    e = H.param_rel_err(pg, po)
    assert max(e.values()) < 1e-6, e
    # camera 0 is constant (multi_calib.cpp:186)
    assert np.all(pg.cam_rt[0] == p.cam_rt[0])


def test_lm_multi_config3(hip_device):
    """BASELINE config 3: 4-camera rig, 500 views/cam, joint intrinsics + extrinsics."""
    p = synth.make_config(3)
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_)
    e = H.param_rel_err(pg, po)
    assert max(e.values()) < 1e-6, e
    og, oper = orc.mean_reprojection_error(po)
    per, g, rmse = api.reprojection_error(pg)
    assert abs(g - og) <= 1e-6 * og and np.max(np.abs(per - oper) / oper) < 1e-6
    assert abs(rmse - orc.rmse(po)) <= 1e-6 * orc.rmse(po)


def test_lm_mono_config2(hip_device):
    """BASELINE config 2: single fisheye, 2000 views x 54 corners -- the reference's mono problem (TS.cpp:247-282:
    9 intrinsics + a pose block per view) at full size, trace and parameters against the oracle."""
    p = synth.make_config(2)
    assert p.mono and p.n_views == 2000 and p.n_corners == 108000
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_)
    e = H.param_rel_err(pg, po)
    assert e["intr"] < 1e-6 and e["board_rt"] < 1e-6, e
    assert abs(gs["rmse"] - orc.rmse(po)) <= 1e-6 * orc.rmse(po)
    assert gs["termination"] == "CONVERGENCE"


def test_constant_board_poses(hip_device):
    """board_pose_constant (SetParameterBlockConstant on pose blocks; the reference never does it -- SURVEY 8d's
    poses-fixed switch): all views fixed (mono: 7 free intrinsics, the Schur complement vanishes), and a rig with every
    second board fixed, against the oracle."""
    p = synth.make_config(1, poses_fixed=True)
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_)
    assert H.param_rel_err(pg, po)["intr"] < 1e-6
    assert np.array_equal(pg.board_rt, p.board_rt)                  # constant blocks come back bit for bit
    q = H.small_rig(4, 16, seed=9)
    c = np.zeros(q.n_boards, dtype=np.uint8)
    c[::2] = 1
    q.board_pose_constant = c
    qg, qo, gs, os_ = _solve_both(q)
    _cmp_trace(gs, os_)
    assert max(H.param_rel_err(qg, qo).values()) < 1e-6
    assert np.array_equal(qg.board_rt[::2], q.board_rt[::2])
    # sharded: the flags follow the boards to their ranks
    qs = q.copy().normalised()
    with api.Group(qs, 3) as g:
        sums = g.solve()
    assert sums[0]["num_iterations"] == os_["num_iterations"]
    assert max(H.param_rel_err(qs, qo).values()) < 1e-6 and np.array_equal(qs.board_rt[::2], q.board_rt[::2])


def test_lm_mono_config2_poses_fixed(hip_device):
    """BASELINE config 2 in its "intrinsics-only" form: 2000 views x 54 corners, every view pose held constant."""
    p = synth.make_config(2, poses_fixed=True)
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_)
    assert H.param_rel_err(pg, po)["intr"] < 1e-6
    assert abs(gs["rmse"] - orc.rmse(po)) <= 1e-6 * orc.rmse(po)
    assert np.array_equal(pg.board_rt, p.board_rt)


def test_lm_multi_config4_vs_oracle(hip_device):
    """BASELINE config 4 (the headline: 4 cameras x 10k views, 2.16 M corners) at FULL size against the sequential
    oracle: whole iteration trace, termination, every parameter block and the error report.  ~30 s of oracle."""
    p = synth.make_config(4)
    assert p.n_corners == 2160000
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_)
    e = H.param_rel_err(pg, po)
    assert max(e.values()) < 1e-6, e
    og, oper = orc.mean_reprojection_error(po)
    per, g, rmse = api.reprojection_error(pg)
    assert abs(g - og) <= 1e-6 * og and np.max(np.abs(per - oper) / oper) < 1e-6
    assert abs(rmse - orc.rmse(po)) <= 1e-6 * orc.rmse(po)
    assert abs(gs["rmse"] - rmse) <= 1e-9 * rmse


def test_lm_multi_config5_vs_oracle(hip_device):
    """BASELINE config 5 (8 cameras x 20k views, 8.64 M corners, 114-column reduced system) at FULL size.  The oracle
    runs its OpenMP passes here (orc_set_num_threads: same arithmetic, sums associated per thread -- checked against
    the sequential path in tests/test_oracle.py) so that the 2.9 GB Jacobian is processed in seconds, not minutes."""
    import os
    p = synth.make_config(5)
    assert p.n_cameras == 8 and p.n_corners == 8640000
    L = orc.lib()
    import bench
    L.orc_set_num_threads(min(int(L.orc_max_threads()), bench._usable_cores(), 64))
    try:
        pg, po, gs, os_ = _solve_both(p)
    finally:
        L.orc_set_num_threads(1)
    _cmp_trace(gs, os_)
    e = H.param_rel_err(pg, po)
    assert max(e.values()) < 1e-6, e
    assert abs(gs["rmse"] - orc.rmse(po)) <= 1e-6 * orc.rmse(po)


def test_lm_one_shot_entry_points(hip_device):
    """tscm_solve_mono / tscm_solve_multi (the drop-in calls of INTEGRATION.md)."""
    p = synth.make_config(1)
    pg = p.copy().normalised()
    ok, s = api.refinement(pg)
    assert ok and s["termination"] == "CONVERGENCE"
    po = p.copy().normalised()
    orc.solve(po)
    assert H.param_rel_err(pg, po)["intr"] < 1e-6
    q = H.small_rig(4, 8, seed=2)
    qg = q.copy().normalised()
    s2 = api.calibrate(qg)
    qo = q.copy().normalised()
    orc.solve(qo)
    assert max(H.param_rel_err(qg, qo).values()) < 1e-6
    with pytest.raises(ValueError):
        api.calibrate(pg)


def test_cpp_host_program_through_c_abi(hip_device, tmp_path):
    """examples/dropin_demo.cpp: a C++11 host (the reference's language) linked against the C ABI,
    doing what the rewritten MultiCalib::calibrate() of INTEGRATION.md does."""
    import os, struct, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "dropin_demo")
    csrc = os.path.join(root, "tscm_calib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "dropin_demo.cpp"),
                           "-L", csrc, "-ltscm_hip", "-Wl,-rpath," + csrc, "-o", exe])
    p = H.small_rig(4, 12, seed=13)
    with open(tmp_path / "problem.bin", "wb") as f:
        f.write(struct.pack("6i", p.n_cameras, p.n_boards, p.n_points, p.n_views, p.n_corners, int(p.mono)))
        for a in (p.board_xy, p.view_camera, p.view_board, p.view_offset, p.view_count, p.obs_u, p.obs_v,
                  p.cam_rt, p.intr, p.board_rt, p.cam_pose_constant):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")]).decode()
    assert "Function tolerance reached." in out or "tolerance" in out
    raw = open(tmp_path / "result.bin", "rb").read()
    C, B = p.n_cameras, p.n_boards
    vals = np.frombuffer(raw[:8 * (15 * C + 6 * B)], dtype=np.float64)
    po = p.copy().normalised()
    os_ = orc.solve(po)
    assert np.max(np.abs(vals[6 * C:15 * C].reshape(C, 9)[:, :7] - po.intr[:, :7]) / np.abs(po.intr[:, :7])) < 1e-6
    term, iters = struct.unpack("2i", raw[8 * (15 * C + 6 * B):8 * (15 * C + 6 * B) + 8])
    assert term == os_["termination_type"] and iters == os_["num_iterations"]


def test_lm_rejected_steps_at_tiny_and_huge_initial_radius(hip_device):
    """A tiny initial radius forces heavily damped steps and a huge one an aggressive first
    step; the accept/reject bookkeeping must follow the oracle either way."""
    p = H.small_rig(4, 10, seed=4)
    for r0 in (1e-2, 1e12):
        pg, po, gs, os_ = _solve_both(p, initial_trust_region_radius=r0, max_num_iterations=12)
        assert gs["num_iterations"] == os_["num_iterations"]
        assert [i["step_is_successful"] for i in gs["iterations"]] == [i["step_is_successful"] for i in os_["iterations"]]
        # r0 = 1e12 is a nearly undamped Gauss-Newton start on an ill-conditioned system: the cost
        # visits 1e14 and round-off differences are amplified, so only 1e-4 is asked for there
        assert abs(gs["final_cost"] - os_["final_cost"]) <= (1e-6 if r0 < 1 else 1e-4) * os_["final_cost"]


# ------------------------------------------------------------------ edge cases
def test_ragged_views_and_missing_detections(hip_device):
    """Empty views (no detection: main.cpp:35-37), a board seen by one camera only, a board
    nobody sees and partially detected views (prefix of the corner list)."""
    p = H.small_rig(4, 10, seed=8)
    cnt = p.view_count.copy()
    cnt[3] = 0            # empty view
    cnt[4] = 0
    cnt[5] = 0            # views 4,5 -> board 2 unseen by anybody
    cnt[7] = 31           # partial view
    p.view_count = cnt
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_)
    assert max(H.param_rel_err(pg, po).values()) < 1e-6
    assert np.all(pg.board_rt[2] == p.board_rt[2])       # untouched parameter block


def test_big_board_more_than_64_corners(hip_device):
    """11x8 = 88 corners per view (the author's own board: main.cpp:191) -> two 64-corner passes."""
    p = synth.make_problem(4, 6, 17, cols=11, rows=8, pitch=30.0)
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_)
    assert max(H.param_rel_err(pg, po).values()) < 1e-6


def test_boards_seen_by_one_to_four_cameras(hip_device):
    """Frames seen by 1, 2, 3 and 4 cameras: every Schur-complement path (per-signature board
    tiles for <= 3 views, explicit pair list above that)."""
    p = H.mixed_visibility_rig(seed=5, n_frames=24)
    assert sorted(set(np.bincount(p.view_board))) == [1, 2, 3, 4]
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_)
    assert max(H.param_rel_err(pg, po).values()) < 1e-6


def test_eight_camera_rig(hip_device):
    """C = 8 (BASELINE config 5 shape, small): k_solve_nd along the ring of 8 cameras, two tiles per thread."""
    p = synth.make_problem(8, 6, 23)
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_)
    assert max(H.param_rel_err(pg, po).values()) < 1e-6
    g = api.normal_equations(p)
    o = H.oracle_normal_equations(p)
    assert np.max(np.abs(g["cam_gram"] - o["cam_gram"])) <= 1e-11 * np.abs(o["cam_gram"]).max()


@pytest.mark.parametrize("C,free_gauge", [(2, False), (3, False), (4, True), (5, False), (6, False), (7, False), (7, True), (8, False), (8, True)])
def test_reduced_solver_geometries(hip_device, C, free_gauge):
    """Ring rigs of 2-8 cameras: the dense k_solve_reduced up to 4 cameras (13 panels with no constant pose: the last panel
    row shares a wave with the look-ahead thread), k_solve_nd along the ring from 5 (one tile per thread up to 7 cameras,
    two at 8).  With no constant camera pose the system has a gauge freedom that only the LM damping removes (Ceres accepts
    that too)."""
    p = synth.make_problem(C, 8, 40 + C)
    if free_gauge:
        p.cam_pose_constant[:] = 0
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_, rtol=1e-5 if free_gauge else 1e-6)
    assert abs(gs["final_cost"] - os_["final_cost"]) <= 1e-5 * os_["final_cost"]
    if not free_gauge:
        assert max(H.param_rel_err(pg, po).values()) < 1e-6


GRAPHS = {
    "chain4": (4, [(0, 1), (1, 2), (2, 3)]),
    "complete4": (4, [(a, b) for a in range(4) for b in range(a + 1, 4)]),
    "chain8": (8, [(i, i + 1) for i in range(7)]),
    "star6": (6, [(0, m) for m in range(1, 6)]),
    "two_rings8": (8, [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4)]),
    "complete8": (8, [(a, b) for a in range(8) for b in range(a + 1, 8)]),
}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_reduced_solver_along_the_camera_pair_graph(hip_device, name):
    """Rigs of 5-8 cameras factor the reduced camera system along the camera-pair graph (k_solve_nd on the nested-dissection
    plan of tscm_nd_plan.h; rings are covered by BASELINE config 5 and test_eight_camera_rig), rigs of up to 4 as one dense
    block (k_solve_reduced).  Chains, stars, two coupled rings and complete graphs (= one dense block) against the oracle's
    dense Cholesky, and the three code paths against each other -- default, k_solve_nd along the graph
    (TSCM_EXEC_GRAPH_REDUCED_ORDER: what a rig of up to 4 cameras would not run otherwise), k_solve_nd on the dense order
    (TSCM_EXEC_DENSE_REDUCED_ORDER): they agree to rounding, iteration by iteration."""
    C, pairs = GRAPHS[name]
    p = H.rig_with_pairs(C, pairs, frames_per_pair=8 if len(pairs) < 20 else 2, seed=50 + C)
    opts = dict(max_num_iterations=12)
    pg, po, gs, os_ = _solve_both(p, **opts)
    _cmp_trace(gs, os_)
    assert max(H.param_rel_err(pg, po).values()) < 1e-6
    for flag in (lib.EXEC_GRAPH_REDUCED_ORDER, lib.EXEC_DENSE_REDUCED_ORDER):
        pd = p.copy().normalised()
        with api.Solver(pd) as s:
            ds = s.solve(exec_flags=flag, **opts)
        _cmp_trace(ds, gs, rtol=1e-9)
        assert max(H.param_rel_err(pd, pg).values()) < 1e-8


def test_eight_free_cameras_on_a_dense_incomplete_graph_take_the_dense_plan(hip_device):
    """8 cameras, NO constant pose (legal API: gauge left to the LM damping), every camera pair but (0, 1) shares a board: the
    graph plan's panel padding does not fit k_solve_nd's tile budget, the dense packing of the same 104 columns does
    (tests/test_nd_plan.py) -- the solver must be created on the dense plan (round 4 refused the rig) and agree with the oracle
    and with the explicitly dense order."""
    pairs = [(a, b) for a in range(8) for b in range(a + 1, 8) if (a, b) != (0, 1)]
    p = H.rig_with_pairs(8, pairs, frames_per_pair=2, seed=77)
    p.cam_pose_constant[:] = 0
    opts = dict(max_num_iterations=8)
    pg, po, gs, os_ = _solve_both(p, **opts)
    _cmp_trace(gs, os_, rtol=1e-5)
    assert abs(gs["final_cost"] - os_["final_cost"]) <= 1e-5 * os_["final_cost"]
    pd = p.copy().normalised()
    with api.Solver(pd) as s:
        ds = s.solve(exec_flags=lib.EXEC_DENSE_REDUCED_ORDER, **opts)
    _cmp_trace(ds, gs, rtol=1e-9)


def test_camera_without_views_and_constant_poses_in_a_six_camera_rig(hip_device):
    """k_solve_nd's plan leaves out a camera that has no views (no free columns: Ceres would not even see its blocks) and takes a
    constant pose as a 7-column block wherever it sits: a ring of the cameras 0, 1, 2, 4, 5 of a 6-camera rig -- camera 3 is seen by
    nobody -- with the poses of cameras 0 and 4 held constant, against the oracle and on both orders; the unseen camera's
    parameters come back untouched."""
    p = H.rig_with_pairs(6, [(0, 1), (1, 2), (2, 4), (4, 5), (5, 0)], frames_per_pair=8, seed=61)
    assert np.bincount(p.view_camera, minlength=6)[3] == 0
    p.cam_pose_constant[:] = 0
    p.cam_pose_constant[[0, 4]] = 1
    opts = dict(max_num_iterations=10)
    pg, po, gs, os_ = _solve_both(p, **opts)
    _cmp_trace(gs, os_)
    assert max(H.param_rel_err(pg, po).values()) < 1e-6
    assert np.array_equal(pg.cam_rt[3], p.cam_rt[3]) and np.array_equal(pg.intr[3], p.intr[3])
    assert np.array_equal(pg.cam_rt[[0, 4]], p.cam_rt[[0, 4]])
    pd = p.copy().normalised()
    with api.Solver(pd) as s:
        ds = s.solve(exec_flags=lib.EXEC_DENSE_REDUCED_ORDER, **opts)
    _cmp_trace(ds, gs, rtol=1e-9)
    assert max(H.param_rel_err(pd, pg).values()) < 1e-8


def test_ring_of_four_along_the_graph_and_as_a_dense_block(hip_device):
    """BASELINE config 3 (4-camera ring, 500 views per camera) through k_solve_nd (9 phases along the ring) and through the dense
    k_solve_reduced (12 panels, the default up to 4 cameras): same trace and parameters to rounding, both equal to the oracle's."""
    p = synth.make_config(3)
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_)
    pn = p.copy().normalised()
    with api.Solver(pn) as s:
        ns = s.solve(exec_flags=lib.EXEC_GRAPH_REDUCED_ORDER)
    _cmp_trace(ns, gs, rtol=1e-9)
    assert max(H.param_rel_err(pn, pg).values()) < 1e-8 and max(H.param_rel_err(pn, po).values()) < 1e-6


def test_options_struct_says_how_long_it_is(hip_device):
    """ABI 6: tscm_options starts with struct_size.  A struct that was never initialised (0), one of an older ABI (its
    max_num_iterations sits where the size is: 50 or 100) and one longer than the library's are refused; a struct that ends
    behind exec_flags without the trailing padding is the shortest one the library knows and solves like the full one."""
    import ctypes as C
    from tscm_calib_amd.lib import TscmError
    p = H.small_rig(4, 4, seed=1).normalised()
    with api.Solver(p) as s:
        for bad in (0, 50, 100, C.sizeof(lib.COptions) + 8):
            with pytest.raises(TscmError) as e:
                s.solve(struct_size=bad)
            assert e.value.code == -1 and "struct_size" in str(e.value)
        assert np.array_equal(p.intr, H.small_rig(4, 4, seed=1).normalised().intr)         # a refused call leaves the caller's parameters alone
        s.upload_params()
        a = s.solve_resident()
        b = s.solve_resident(struct_size=lib.COptions.exec_flags.offset + 4)
        assert a["num_iterations"] == b["num_iterations"] and a["final_cost"] == b["final_cost"]


def test_unknown_exec_flags_are_refused(hip_device):
    from tscm_calib_amd.lib import TscmError
    p = H.small_rig(4, 4, seed=1).normalised()
    with api.Solver(p) as s:
        with pytest.raises(TscmError) as e:
            s.solve(exec_flags=0x100)
        assert e.value.code == -1
        s.solve()


def test_rccl_code_path_single_rank(hip_device):
    """The multi-GPU code path (RCCL all-reduce of T, grouped sum/max all-reduce of the staged camera
    tiles, separate k_control) on a one-rank communicator (tscm_options.exec_flags: TSCM_EXEC_KEEP_SINGLE_RANK_COMM):
    must reproduce the single-GPU path bit for bit."""
    p = H.small_rig(4, 10, seed=33)
    ref = p.copy().normalised()
    with api.Solver(ref) as s:
        rs = s.solve()
    comm = api.Comm(api.Comm.unique_id(), 0, 1, 0)
    q = p.copy().normalised()
    with api.Solver(q) as s:
        s.set_comm(comm)
        qs = s.solve(exec_flags=lib.EXEC_KEEP_SINGLE_RANK_COMM)
        s.set_comm(None)
    comm.close()
    assert qs["num_iterations"] == rs["num_iterations"] and qs["message"] == rs["message"]
    assert np.array_equal(q.intr, ref.intr) and np.array_equal(q.cam_rt, ref.cam_rt) and np.array_equal(q.board_rt, ref.board_rt)


def test_ipc_exchange_code_path_single_rank(hip_device):
    """The IPC exchange back-end (tscm_comm_ipc_open / _connect, k_ipc_allreduce) on a one-rank communicator in this
    process: the two all-reduces of every iteration and the board gather run through it (TSCM_EXEC_KEEP_SINGLE_RANK_COMM) and
    must reproduce the single-GPU path bit for bit.  Several rank PROCESSES on this device: tests/test_gpu_bench.py."""
    p = H.small_rig(4, 10, seed=33)
    ref = p.copy().normalised()
    with api.Solver(ref) as s:
        rs = s.solve()
    comm = api.Comm.ipc(0, 1, 0, lambda h: [h], n_cameras=4)
    assert comm.backend_ranks() == 1
    q = p.copy().normalised()
    with api.Solver(q) as s:
        s.set_comm(comm)
        qs = s.solve(exec_flags=lib.EXEC_KEEP_SINGLE_RANK_COMM)
        s.set_comm(None)
    comm.close()
    assert qs["num_iterations"] == rs["num_iterations"] and qs["message"] == rs["message"]
    assert np.array_equal(q.intr, ref.intr) and np.array_equal(q.cam_rt, ref.cam_rt) and np.array_equal(q.board_rt, ref.board_rt)


@pytest.mark.parametrize("cfg", [1, 3])
def test_fused_and_separate_T_reduction_agree_bit_for_bit(hip_device, cfg):
    """One GPU, <= 4 cameras: the T reduction rides in the reduced solve's launch (workgroups behind an arrival counter).
    tscm_options.exec_flags = TSCM_EXEC_SEPARATE_T_REDUCE keeps it a launch of its own (the path every communicator run
    takes); the summation order of a tile entry is the same in both, so the whole solve must be."""
    p = synth.make_config(cfg)
    a, b = p.copy().normalised(), p.copy().normalised()
    with api.Solver(a) as s:
        sa = s.solve()
    with api.Solver(b) as s:
        sb = s.solve(exec_flags=lib.EXEC_SEPARATE_T_REDUCE)
    assert sa["num_iterations"] == sb["num_iterations"] and sa["message"] == sb["message"]
    assert [it["cost"] for it in sa["iterations"]] == [it["cost"] for it in sb["iterations"]]
    assert np.array_equal(a.intr, b.intr) and np.array_equal(a.cam_rt, b.cam_rt) and np.array_equal(a.board_rt, b.board_rt)


@pytest.mark.parametrize("cfg", [1, 3])
def test_gram_on_4x4_blocks_and_on_the_16x16_tile_agree_bit_for_bit(hip_device, cfg):
    """Boards of <= 56 corners run k_eval_gram4 (three v_mfma_f64_4x4x4_4b per four rows, quad-DPP epilogue);
    tscm_options.exec_flags = TSCM_EXEC_GRAM_16X16 selects k_eval_gram<58> (one v_mfma_f64_16x16x4 tile, the kernel of
    rounds 1-3a).  Entries of the two instructions' results are the same bits and the epilogues perform the same
    operations in the same order: the whole solve must be."""
    p = synth.make_config(cfg)
    a, b = p.copy().normalised(), p.copy().normalised()
    with api.Solver(a) as s:
        sa = s.solve()
    with api.Solver(b) as s:
        sb = s.solve(exec_flags=lib.EXEC_GRAM_16X16)
    assert sa["num_iterations"] == sb["num_iterations"] and sa["message"] == sb["message"]
    assert [it["cost"] for it in sa["iterations"]] == [it["cost"] for it in sb["iterations"]]
    assert np.array_equal(a.intr, b.intr) and np.array_equal(a.cam_rt, b.cam_rt) and np.array_equal(a.board_rt, b.board_rt)


@pytest.mark.parametrize("cols,rows", [(11, 8), (8, 6), (6, 5), (7, 6), (9, 7), (12, 9), (14, 10), (17, 12), (5, 4), (3, 3), (2, 2), (19, 3), (8, 7)])
def test_gram4_serves_every_board_size_with_the_bits_of_the_16x16_tile(hip_device, cols, rows):
    """Round 6: k_eval_gram4<KS, MULTI> is the default for EVERY board (rounds 3-5: 49..56 corners only) -- ceil(n / 4)
    k-steps for boards of up to 56 corners, ceil(n / 56) balanced passes of a multiple of four corners above that (the
    reference's 11 x 8: main.cpp:190-191 -> 2 x 44).  The k-steps of a view contract the same groups of four rows in the
    same order as k_eval_gram<0>'s 64-row passes (TSCM_EXEC_GRAM_16X16), so the whole solve must agree bit for bit --
    full views and ragged ones (prefixes of the corner list, an empty view), and both against the oracle."""
    n = cols * rows
    p = synth.make_problem(4, 10, 700 + n, cols=cols, rows=rows, pitch=360.0 / max(cols, rows))
    rng = np.random.default_rng(n)
    q = p.copy()
    q.view_count[::3] = rng.integers(max(1, n // 3), n + 1, size=q.view_count[::3].shape[0])
    if n >= 12:
        q.view_count[7] = 0
    for prob in (p, q):
        a, b, o = prob.copy().normalised(), prob.copy().normalised(), prob.copy().normalised()
        with api.Solver(a) as s:
            sa = s.solve(max_num_iterations=5)
        with api.Solver(b) as s:
            sb = s.solve(max_num_iterations=5, exec_flags=lib.EXEC_GRAM_16X16)
        so = orc.solve(o, max_num_iterations=5)
        assert sa["num_iterations"] == sb["num_iterations"] == so["num_iterations"]
        assert [it["cost"] for it in sa["iterations"]] == [it["cost"] for it in sb["iterations"]]
        assert np.array_equal(a.intr, b.intr) and np.array_equal(a.cam_rt, b.cam_rt) and np.array_equal(a.board_rt, b.board_rt)
        for x, y in zip(sa["iterations"], so["iterations"]):
            assert x["step_is_successful"] == y["step_is_successful"]
            assert abs(x["cost"] - y["cost"]) <= 1e-9 * y["cost"]
        assert max(H.param_rel_err(a, o).values()) < 1e-6


def test_gram4_two_passes_on_the_reference_board_at_size(hip_device):
    """The reference's own board (11 x 8 = 88 corners, main.cpp:190-191) at config-3 size (4 cameras x 500 views,
    176,000 corners): natural solve against the oracle, trace and every parameter block."""
    p = synth.make_config(3, cols=11, rows=8, pitch=36.0)
    pg, po, gs, os_ = _solve_both(p)
    _cmp_trace(gs, os_)
    assert max(H.param_rel_err(pg, po).values()) < 1e-6


@pytest.mark.parametrize("cfg", [1, 3])
def test_backsub_inside_the_solve_launch_and_as_a_launch_of_its_own_agree_bit_for_bit(hip_device, cfg):
    """One GPU, <= 4 cameras: the back-substitution workgroups ride in the reduced solve's launch, load their operands
    and wait for the camera step (y_flag); tscm_options.exec_flags = TSCM_EXEC_SEPARATE_BACKSUB launches k_backsub_prep
    on its own.  Same arithmetic either way: the solves must agree bit for bit."""
    p = synth.make_config(cfg)
    a, b = p.copy().normalised(), p.copy().normalised()
    with api.Solver(a) as s:
        sa = s.solve()
    with api.Solver(b) as s:
        sb = s.solve(exec_flags=lib.EXEC_SEPARATE_BACKSUB)
    assert sa["num_iterations"] == sb["num_iterations"] and sa["message"] == sb["message"]
    assert [it["cost"] for it in sa["iterations"]] == [it["cost"] for it in sb["iterations"]]
    assert np.array_equal(a.intr, b.intr) and np.array_equal(a.cam_rt, b.cam_rt) and np.array_equal(a.board_rt, b.board_rt)


@pytest.mark.parametrize("cfg", [1, 3])
def test_control_step_in_the_schur_kernels_head_and_in_the_reductions_launch_agree_bit_for_bit(hip_device, cfg):
    """One GPU, <= 4 cameras, one Schur kernel per iteration: every workgroup of k_schur_gram takes the control step of
    the evaluation in front of it in its head (same inputs, same bits; workgroup 0 writes), and k_control_tail takes the
    last one of the solve.  tscm_options.exec_flags = TSCM_EXEC_SEPARATE_CONTROL keeps it in k_reduce_control's last
    workgroup.  Same decisions, same log, same bits -- with the termination tests on (natural solve) and with 30
    forced iterations (rejected steps included)."""
    forced = dict(max_num_iterations=30, function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0,
                  min_trust_region_radius=0.0)
    for opts in (dict(), forced):
        p = synth.make_config(cfg)
        a, b = p.copy().normalised(), p.copy().normalised()
        with api.Solver(a) as s:
            sa = s.solve(**opts)
        with api.Solver(b) as s:
            sb = s.solve(exec_flags=lib.EXEC_SEPARATE_CONTROL, **opts)
        assert sa["num_iterations"] == sb["num_iterations"] and sa["message"] == sb["message"]
        assert sa["iterations"] == sb["iterations"]
        assert sa["final_cost"] == sb["final_cost"] and sa["lm_iterations"] == sb["lm_iterations"]
        assert np.array_equal(a.intr, b.intr) and np.array_equal(a.cam_rt, b.cam_rt) and np.array_equal(a.board_rt, b.board_rt)


@pytest.mark.parametrize("cfg", [1, 3, 4, 5])
def test_reductions_riding_in_the_schur_launch_and_in_a_launch_of_their_own_agree_bit_for_bit(hip_device, cfg):
    """One GPU, a Schur-complement grid of one round: the reductions behind a candidate's evaluation (camera-tile sums, board
    statistics, the snapshot of the LM state) are taken by the first workgroups of the next Schur-complement launch in front
    of their own chunks (k_schur_gram<NV, true>: written through, counted in, waited for in front of the control step, the
    records requested meanwhile from the buffer an accepted step makes current -- a rejected step asks again);
    tscm_options.exec_flags = TSCM_EXEC_SEPARATE_STATS keeps them k_reduce_stats, a launch of their own.  Same decisions,
    same log, same bits -- natural solves and forced iterations with rejected steps; configs 1, 3, 4 ride, config 5 (a grid
    of 2.5 rounds) takes the separate launch either way."""
    forced = dict(max_num_iterations=12 if cfg >= 4 else 30, function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0,
                  min_trust_region_radius=0.0)
    for opts in (dict(), forced):
        p = synth.make_config(cfg)
        a, b = p.copy().normalised(), p.copy().normalised()
        with api.Solver(a) as s:
            sa = s.solve(**opts)
        with api.Solver(b) as s:
            sb = s.solve(exec_flags=lib.EXEC_SEPARATE_STATS, **opts)
        assert sa["num_iterations"] == sb["num_iterations"] and sa["message"] == sb["message"]
        assert sa["iterations"] == sb["iterations"]
        assert sa["final_cost"] == sb["final_cost"] and sa["lm_iterations"] == sb["lm_iterations"]
        assert np.array_equal(a.intr, b.intr) and np.array_equal(a.cam_rt, b.cam_rt) and np.array_equal(a.board_rt, b.board_rt)


def test_every_fusion_switched_off_gives_the_same_bits(hip_device):
    """exec_flags = SEPARATE_T_REDUCE | SEPARATE_BACKSUB | SEPARATE_CONTROL: the six-launch iteration of the start of
    round 3 (k_schur_gram, k_T_reduce, k_solve_reduced, k_backsub_prep, Gram kernel, k_reduce_control) against the
    four-launch one -- 30 forced iterations of config 3 with rejected steps, and the natural solve."""
    forced = dict(max_num_iterations=30, function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0,
                  min_trust_region_radius=0.0)
    off = lib.EXEC_SEPARATE_T_REDUCE | lib.EXEC_SEPARATE_BACKSUB | lib.EXEC_SEPARATE_CONTROL
    for opts in (dict(), forced):
        p = synth.make_config(3)
        a, b = p.copy().normalised(), p.copy().normalised()
        with api.Solver(a) as s:
            sa = s.solve(**opts)
        with api.Solver(b) as s:
            sb = s.solve(exec_flags=off, **opts)
        assert sa["iterations"] == sb["iterations"] and sa["message"] == sb["message"]
        assert np.array_equal(a.intr, b.intr) and np.array_equal(a.cam_rt, b.cam_rt) and np.array_equal(a.board_rt, b.board_rt)


def test_fusions_of_an_eight_camera_rig_give_the_same_bits(hip_device):
    """Round 4 lifted the one-GPU fusions from 4 to 8 cameras: T producers and back-substitution workgroups ride in k_solve_nd's
    launch (only as many as are resident next to the solver workgroup; the others follow in a launch of their own) and the
    control step is taken in k_schur_gram's head.  Each switched off on its own and all together: same log, same bits, over
    25 forced iterations of an 8-camera ring (600 views per camera: 2,400 boards = 75 groups of 32) and the natural solve."""
    forced = dict(max_num_iterations=25, function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0,
                  min_trust_region_radius=0.0)
    p = synth.make_problem(8, 600, 81)
    for opts in (dict(), forced):
        ref = None
        for flags in (0, lib.EXEC_SEPARATE_T_REDUCE, lib.EXEC_SEPARATE_BACKSUB, lib.EXEC_SEPARATE_CONTROL, lib.EXEC_SEPARATE_STATS,
                      lib.EXEC_SEPARATE_T_REDUCE | lib.EXEC_SEPARATE_BACKSUB | lib.EXEC_SEPARATE_CONTROL | lib.EXEC_SEPARATE_STATS):
            q = p.copy().normalised()
            with api.Solver(q) as s:
                r = s.solve(exec_flags=flags, **opts)
            cur = (r["iterations"], r["final_cost"], q.intr.tobytes(), q.cam_rt.tobytes(), q.board_rt.tobytes())
            if ref is None:
                ref = cur
            assert cur[0] == ref[0] and cur[1] == ref[1], flags
            assert cur[2:] == ref[2:], flags


def test_repeated_solves_are_the_same_bits_every_time(hip_device):
    """The hand-offs inside the launches (T tiles -> reduced solve, camera step -> waiting back-substitution workgroups)
    order data by completion, not by fences: a lost ordering would show as a solve that differs from the others.  100
    resident solves of 25 forced iterations of config 3 (rejected steps included) must give one and the same log."""
    p = synth.make_config(3).normalised()
    opts = dict(max_num_iterations=25, function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0,
                min_trust_region_radius=0.0, check_every=255)
    with api.Solver(p) as s:
        s.upload_params()
        logs = set()
        for _ in range(100):
            r = s.solve_resident(reset=True, **opts)
            logs.add((r["final_cost"], tuple((it["cost"], it["step_is_successful"], it["trust_region_radius"]) for it in r["iterations"])))
    assert len(logs) == 1


def test_late_handoff_reruns_the_solve_on_separate_launches(hip_device):
    """The reduced solve waits for the Schur-complement tiles of the other workgroups of its launch behind an arrival
    counter.  A hand-off that does not come within its time bound (0.5 s) is not a numerical event -- the solve is stopped on
    the device -- but it need not be the caller's problem either (a debugger, a co-tenant, a context switch stall a workgroup
    just the same): the library runs that solve again from its start point on the launches that hand nothing over inside a
    launch and returns ITS result -- the bits of an undisturbed solve.  With one producer withheld (fault injection)."""
    import time
    p = H.small_rig(4, 10, seed=33)
    ref = p.copy().normalised()
    with api.Solver(ref) as s:
        rs = s.solve()
    q = p.copy().normalised()
    with api.Solver(q) as s:
        assert s.reruns() == 0
        t0 = time.time()
        s.debug_withhold_handoff()
        qs = s.solve()
        assert 0.4 < time.time() - t0 < 10.0 and s.reruns() == 1
        assert "run again on separate launches" in lib.lib().tscm_last_error().decode()
        assert qs["num_iterations"] == rs["num_iterations"] and [it["cost"] for it in qs["iterations"]] == [it["cost"] for it in rs["iterations"]]
        assert np.array_equal(q.intr, ref.intr) and np.array_equal(q.board_rt, ref.board_rt) and np.array_equal(q.cam_rt, ref.cam_rt)
        # a resident solve that CONTINUES from the device's parameters (reset = 0) restarts from where it began, too
        s.upload_params(p.copy().normalised().cam_rt, p.copy().normalised().intr, p.copy().normalised().board_rt)
        a = s.solve_resident(reset=True, max_num_iterations=2)
        s.debug_withhold_handoff()
        b = s.solve_resident(reset=False)
        assert s.reruns() == 2
    with api.Solver(p.copy().normalised()) as s:
        s.upload_params()
        s.solve_resident(reset=True, max_num_iterations=2)
        c = s.solve_resident(reset=False)
    assert a["num_iterations"] == 3 and b["num_iterations"] == c["num_iterations"] and b["final_cost"] == c["final_cost"]


def test_late_riding_reduction_reruns_the_solve_on_separate_launches(hip_device):
    """The other hand-off of an iteration: the reductions behind a candidate's evaluation ride in the next Schur-complement
    launch and every other workgroup waits for them in front of the control step.  One of them never counts itself in
    (fault injection 3): the wait ends at its time bound, the solve is stopped and run again on separate launches -- same
    log, same bits as the undisturbed solve."""
    import time
    p = H.small_rig(4, 10, seed=34)
    ref = p.copy().normalised()
    with api.Solver(ref) as s:
        rs = s.solve()
    q = p.copy().normalised()
    with api.Solver(q) as s:
        t0 = time.time()
        s.debug_withhold_handoff(3)
        qs = s.solve()
        assert 0.4 < time.time() - t0 < 10.0 and s.reruns() == 1
        assert "run again on separate launches" in lib.lib().tscm_last_error().decode()
    assert qs["num_iterations"] == rs["num_iterations"] and qs["iterations"] == rs["iterations"]
    assert np.array_equal(q.intr, ref.intr) and np.array_equal(q.board_rt, ref.board_rt) and np.array_equal(q.cam_rt, ref.cam_rt)


def test_late_handoff_without_a_rerun_is_a_hard_error(hip_device):
    """... and where the re-run is not available (forbidden here by the fault injection; in production: a communicator of several
    ranks, which would have to agree on it) the call must return TSCM_E_HIP within the time bound -- not hang, and not go on as a
    rejected step -- with the caller's parameters untouched, and the same solver must work again afterwards (monotonic
    counter, reset per solve)."""
    import time
    from tscm_calib_amd.lib import TscmError
    p = H.small_rig(4, 10, seed=33)
    ref = p.copy().normalised()
    with api.Solver(ref) as s:
        rs = s.solve()
    q = p.copy().normalised()
    with api.Solver(q) as s:
        t0 = time.time()
        with pytest.raises(TscmError) as e:
            s.debug_withhold_handoff(2)
            s.solve()
        assert e.value.code == -3 and "hand-off" in str(e.value)            # TSCM_E_HIP
        assert time.time() - t0 < 10.0 and s.reruns() == 0
        assert np.array_equal(q.intr, p.copy().normalised().intr)          # the caller's parameters were not touched
        qs = s.solve()                                                      # ... and the next solve is unaffected
    assert qs["num_iterations"] == rs["num_iterations"] and np.array_equal(q.intr, ref.intr) and np.array_equal(q.board_rt, ref.board_rt)


def test_invalid_arguments(hip_device):
    from tscm_calib_amd.lib import TscmError
    p = H.small_rig(4, 4, seed=1)
    bad = p.copy().normalised()
    bad.view_camera = bad.view_camera.copy()
    bad.view_camera[0] = 9
    with pytest.raises((TscmError, ValueError)):
        api.Solver(bad)
    dup = p.copy().normalised()
    dup.view_camera = dup.view_camera.copy(); dup.view_board = dup.view_board.copy()
    dup.view_camera[1] = dup.view_camera[0]; dup.view_board[1] = dup.view_board[0]
    with pytest.raises(TscmError):
        api.Solver(dup)


# ------------------------------------------------------------------ full-size properties
def test_config4_properties(hip_device):
    """BASELINE config 4 (4 cams x 10k views, 2.16 M corners) is too big for the oracle in a
    test; check size-independent properties instead: monotone cost, RMSE at the noise floor,
    recovery of the ground truth, and invariance of the result to the order of the views."""
    p = synth.make_config(4)
    pg = p.copy().normalised()
    with api.Solver(pg) as s:
        gs = s.solve()
    assert gs["termination"] == "CONVERGENCE"
    costs = [it["cost"] for it in gs["iterations"] if it["step_is_successful"]]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert abs(gs["rmse"] - 0.1 * np.sqrt(2.0)) < 2e-3          # sigma = 0.1 px per coordinate
    # fx/fy/xi/lambda/alpha trade off along a near-flat valley of the TS model, so only
    # the principal point is pinned by the data; the fitted MODEL must still agree with the ground
    # truth in pixel space over the image.
    gt = p.meta["gt_intr"]
    assert np.max(np.abs(pg.intr[:, 2:4] - gt[:, 2:4])) < 0.05     # px
    az, el = np.meshgrid(np.linspace(-1.2, 1.2, 25), np.linspace(-1.0, 1.0, 21))
    rays = np.stack([np.sin(az) * np.cos(el), np.sin(el), np.cos(az) * np.cos(el)], -1).reshape(-1, 3) * 500.0
    for m in range(p.n_cameras):
        assert np.max(np.abs(api.project(pg.intr[m], rays) - api.project(gt[m], rays))) < 0.5
    per, g, rmse = api.reprojection_error(pg)
    assert abs(rmse - gs["rmse"]) < 1e-9
    # permute the views: same problem, same answer
    perm = np.random.default_rng(0).permutation(p.n_views)
    q = p.copy().normalised()
    q.view_camera, q.view_board = p.view_camera[perm].copy(), p.view_board[perm].copy()
    q.view_offset, q.view_count = p.view_offset[perm].copy(), p.view_count[perm].copy()
    with api.Solver(q) as s:
        qs = s.solve()
    assert qs["num_iterations"] == gs["num_iterations"]
    assert np.max(np.abs(q.intr - pg.intr) / np.maximum(np.abs(pg.intr), 1e-3)) < 1e-9


def test_no_device_memory_leak_over_repeated_calls(hip_device):
    """Every entry point that allocates device memory gives it back: 40 rounds of create / solve / destroy,
    rig initialisation, remap tables, projection -- free device memory ends where it started."""
    import ctypes
    from tscm_calib_amd import maps, rig
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value
    p = H.small_rig(4, 12, seed=3)
    inp = synth.make_rig_input(p)
    descs = [maps.undistort_desc(synth.CALIB_INTR[0], 300.0, 300.0, 319.5, 239.5, 640, 480)]
    pts = np.random.default_rng(0).normal(size=(1000, 3)) + [0, 0, 5]

    def one_round():
        q = p.copy().normalised()
        with api.Solver(q) as s:
            s.solve()
        api.calibrate(p.copy().normalised(), hip_device)
        rig.rig_init(inp, hip_device)
        maps.build_maps(descs, None, hip_device)
        api.project(synth.CALIB_INTR[0], pts, hip_device)
        api.normal_equations(p.copy().normalised(), hip_device)

    one_round()                                  # warm-up: code objects, runtime pools
    free0 = free_bytes()
    for _ in range(40):
        one_round()
    free1 = free_bytes()
    assert free0 - free1 < 8 << 20, f"device memory shrank by {(free0 - free1) / 2**20:.1f} MiB over 40 rounds"


def test_results_are_bit_reproducible_run_to_run(hip_device):
    """No atomics and fixed reduction orders anywhere on the path: repeated solves of the same problem give
    bit-identical parameters, costs and iteration logs (also across solver instances)."""
    p = synth.make_problem(4, 150, 20243)
    ref = None
    for rep in range(4):
        q = p.copy().normalised()
        if rep < 2:
            s = api.calibrate(q, hip_device)
        else:
            with api.Solver(q) as sv:
                s = sv.solve()
        sig = (q.intr.tobytes(), q.cam_rt.tobytes(), q.board_rt.tobytes(), s["final_cost"], s["num_iterations"],
               tuple(it["cost"] for it in s["iterations"]), tuple(it["gradient_norm"] for it in s["iterations"]))
        if ref is None:
            ref = sig
        assert sig == ref, f"run {rep} differs from run 0"


def test_config5_properties(hip_device):
    """BASELINE config 5 (8 cameras x 20k views, 8.64 M corners): size-independent properties of the solve
    (monotone accepted costs, RMSE at the noise floor, fp32-Jacobian tier within 1e-3 of the fp64 tier)."""
    p = synth.make_config(5)
    p64, p32 = p.copy().normalised(), p.copy().normalised()
    s64 = api.calibrate(p64, hip_device)
    assert s64["termination"] == "CONVERGENCE"
    costs = [it["cost"] for it in s64["iterations"] if it["step_is_successful"]]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    # sigma = 0.1 px per coordinate; the fit absorbs 6 parameters per board (+ 13 per camera) of the 2N residuals
    dof = 1.0 - (6.0 * p.n_boards + 13.0 * p.n_cameras) / (2.0 * p.n_corners)
    assert abs(s64["rmse"] - 0.1 * np.sqrt(2.0 * dof)) < 5e-4
    s32 = api.calibrate(p32, hip_device, jacobian_fp32=1)
    assert s32["termination"] == "CONVERGENCE"
    assert abs(s32["rmse"] - s64["rmse"]) < 1e-3 * s64["rmse"]
    d = H.param_rel_err(p32, p64)
    assert max(d["cam_rt"], d["board_rt"]) < 1e-3, d


def test_chunks_longer_than_one_metadata_block(hip_device):
    """560 k views (6-corner boards) put ~137 views into every chunk of the Gram kernel, i.e. more than the
    64 whose metadata one lane block holds: the multi-block path of the view loop against the oracle."""
    p = synth.make_problem(4, 140000, 4242, cols=3, rows=2, pitch=60.0)
    assert p.n_views == 560000
    pg, po = p.copy().normalised(), p.copy().normalised()
    with api.Solver(pg) as s:
        gs = s.solve(max_num_iterations=1)
    os_ = orc.solve(po, max_num_iterations=1)
    for a, b in zip(gs["iterations"], os_["iterations"]):
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"]
        assert abs(a["gradient_max_norm"] - b["gradient_max_norm"]) <= 1e-8 * b["gradient_max_norm"]
        assert abs(a["step_norm"] - b["step_norm"]) <= 1e-7 * max(b["step_norm"], 1e-12)
    assert np.max(np.abs(pg.intr[:, :7] - po.intr[:, :7]) / np.abs(po.intr[:, :7])) < 1e-7


def test_more_backsub_workgroups_than_the_chip_holds(hip_device):
    """The back-substitution workgroups that ride in the reduced solve's launch WAIT for the solver workgroup, so they ride
    there only if ALL of them are resident next to it (occupancy x CUs, queried at create); otherwise the back-substitution
    is a launch of its own.  4 cameras x 20,000 views = 40,000 boards = 1,250 groups of 32 against 768 resident
    workgroups: the solve must neither hang nor fault (0.5 s hand-off bound) over 25 forced iterations, and agrees bit
    for bit with the path that was told to keep the back-substitution separate."""
    p = synth.make_problem(4, 20000, 77)
    opts = dict(max_num_iterations=25, function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0, min_trust_region_radius=0.0, check_every=25)
    pa, pb = p.copy().normalised(), p.copy().normalised()
    with api.Solver(pa) as s:
        s.upload_params()
        ra = s.solve_resident(**opts)
        ca = s.download_params()
        rb = s.solve_resident(exec_flags=lib.EXEC_SEPARATE_BACKSUB, **opts)
        cb = s.download_params()
    assert ra["lm_iterations"] == rb["lm_iterations"] == 25
    assert [it["cost"] for it in ra["iterations"]] == [it["cost"] for it in rb["iterations"]]
    for x, y in zip(ca, cb):
        assert np.array_equal(x, y)


def test_schur_grid_of_several_rounds_takes_the_control_step_once(hip_device):
    """8 cameras x 6,000 views = 24,000 boards = 750 chunks of 32: more workgroups than k_schur_gram has resident at once
    (2 per CU), so the later rounds read the outcome workgroup 0 publishes instead of taking the control step themselves.
    Same bits as the path with the step in the reductions' launch, over 20 forced iterations."""
    p = synth.make_problem(8, 6000, 78)
    opts = dict(max_num_iterations=20, function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0, min_trust_region_radius=0.0, check_every=20)
    with api.Solver(p.copy().normalised()) as s:
        s.upload_params()
        ra = s.solve_resident(**opts)
        ca = s.download_params()
        rb = s.solve_resident(exec_flags=lib.EXEC_SEPARATE_CONTROL, **opts)
        cb = s.download_params()
    assert ra["lm_iterations"] == rb["lm_iterations"] == 20
    assert [(it["cost"], it["trust_region_radius"], it["step_is_successful"]) for it in ra["iterations"]] == [(it["cost"], it["trust_region_radius"], it["step_is_successful"]) for it in rb["iterations"]]
    for x, y in zip(ca, cb):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("cols,rows", [(7, 8), (8, 7), (9, 6), (10, 6), (8, 8), (13, 5), (5, 4), (3, 3), (5, 2), (7, 5), (4, 3), (9, 5),
                                       (9, 7), (13, 4), (11, 9), (16, 8), (13, 10), (17, 12)])
def test_board_shapes_around_the_tile_limits(hip_device, cols, rows):
    """53..56 corners take the compile-time-pitch kernel, 57..64 the generic one in a single pass, 65 and more
    several passes; corner counts of every residue mod 8 (the MFMA loops consume the tile in pairs of 4-row
    k-steps: a tile with an odd number of k-steps used to read past its rows).  Every shape against the oracle."""
    p = synth.make_problem(4, 10, 100 + cols * rows, cols=cols, rows=rows, pitch=40.0)
    pg, po, gs, os_ = _solve_both(p, max_num_iterations=4)
    assert gs["num_iterations"] == os_["num_iterations"]
    for a, b in zip(gs["iterations"], os_["iterations"]):
        assert a["step_is_successful"] == b["step_is_successful"]
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"]
    assert max(H.param_rel_err(pg, po).values()) < 1e-7


@pytest.mark.parametrize("C,views", [(9, 6), (12, 8), (16, 6), (20, 4), (32, 4)])
def test_rigs_of_more_than_eight_cameras(hip_device, C, views):
    """More than 8 cameras: the reduced camera system (up to 13 C - 6 columns) leaves the register/LDS solver and
    is factored in global memory by k_solve_reduced_big; same iteration trace as the oracle."""
    p = synth.make_problem(C, views, 900 + C)
    pg, po, gs, os_ = _solve_both(p, max_num_iterations=4)
    assert gs["num_iterations"] == os_["num_iterations"]
    for a, b in zip(gs["iterations"], os_["iterations"]):
        assert a["step_is_successful"] == b["step_is_successful"]
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"]
        assert abs(a["step_norm"] - b["step_norm"]) <= 1e-7 * max(b["step_norm"], 1e-12)
    assert max(H.param_rel_err(pg, po).values()) < 1e-7


def test_more_than_32_cameras_is_refused(hip_device):
    p = synth.make_problem(33, 2, 5)
    with pytest.raises(lib.TscmError) as e:
        api.Solver(p.normalised())
    assert e.value.code == -5
