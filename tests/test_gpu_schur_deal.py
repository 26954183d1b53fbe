"""k_schur_gram's deal of board groups over its four waves (schur_group_of, tscm_layout.h), on the GPU.

Two- and three-camera rigs on the smallest board the library takes (3 x 2 corners), with boards seen by one, two and (three
cameras) three of them, so that every rig runs k_schur_gram<1>, <2> (and <3>).  The board counts are chosen so that the
chunks plan_layout makes for the MI355X's 256 CUs (N_CUS of tests/test_step_tolerance.py) are of 16 boards (one group per
wave), 17..20 (five groups, the last one partial), 40 (3, 3, 2, 2 groups) and 64 (4, 4, 4, 4), each with ragged signature
tails of 1..15 boards.  The counts are found
by asking the library's own planner (tests/native/schur_deal_check.cpp, `chunks`: plan_layout on the view tables), not a copy
of its rule; on the 256 CUs of an MI355X they come to about 1,000, 8,200, 20,000 and 32,300 boards -- a 64-board chunk
does not exist below 63 x 2 x 256 boards, which is why the two largest cases take several seconds of CPU reference each
(step terms 3 s + reference step 3 s; the oracle's solve 5 s on 16 threads).

Per rig:
  the first LM step against the extended-precision reference step, measured and bounded exactly as
    tests/test_gpu_step.py::test_step_against_extended_precision does (its measure() and tolerances());
  the natural solve against the oracle as tests/test_gpu_parity.py does (its _solve_both, _cmp_trace and bound);
  the same bits whether every workgroup starts its deal at wave 0 or at wave 2 (tscm_solver_debug_schur_rot).
"""
import functools

import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import api, synth
from tscm_calib_amd.problem import Problem
from tests import helpers as H
from tests import native_check as N
from tests import test_gpu_parity as P
from tests import test_gpu_step as G
from tests.test_step_tolerance import EVAL_WAVES_PER_CU, N_CUS      # the MI355X's figures the coverage tests plan with

pytestmark = [pytest.mark.gpu, N.NEEDS_GXX]

PARAM_RTOL = P._cmp_trace.__defaults__[0]      # tests/test_gpu_parity.py: 1e-6 on the trace and on every parameter block

# case -> (cameras, the chunk sizes the plan must contain: any of the range)
CASES = {
    "two_cams_16": (2, range(16, 17)),
    "three_cams_17_20": (3, range(17, 21)),
    "two_cams_40": (2, range(40, 41)),
    "three_cams_64": (3, range(64, 65)),
}


def visibility(C, B):
    """Which cameras see board b: mostly the pair of adjacent cameras make_problem gives it (b % C, (b + 1) % C), every 7th
    board only the first of them, every 11th only the second, and (three cameras) every 5th all three."""
    b = np.arange(B)
    first, second = np.ones(B, bool), np.ones(B, bool)
    second[b % 7 == 3] = False
    first[(b % 11 == 5) & second] = False
    third = (b % 5 == 1) & first & second if C == 3 else np.zeros(B, bool)
    return first, second, third


def view_tables(C, B):
    first, second, third = visibility(C, B)
    b = np.arange(B)
    cam = np.concatenate([(b % C)[first], ((b + 1) % C)[second], ((b + 2) % C)[third]])
    board = np.concatenate([b[first], b[second], b[third]])
    return cam, board


@functools.lru_cache(maxsize=None)
def planner():
    return N.built("schur_deal_check.cpp", "schur_deal_check")


def planned_chunks(cam, board, C, B, n_points, n_cu):
    rows = np.stack([cam, board, np.full(len(cam), n_points)], axis=1)
    words = [C, B, n_points, len(rows), *rows.ravel().tolist(), n_cu, EVAL_WAVES_PER_CU]
    r = N.run(planner(), "chunks", stdin=" ".join(map(str, words)))
    assert r["slow_boards"] == 0
    return r["chunks"]


@functools.lru_cache(maxsize=None)
def boards_for(C, sizes, n_cu):
    """A board count whose largest planned chunk is one of `sizes` and whose plan has a ragged signature tail of 1..15 boards:
    bisection over the planner's answers for the smallest count that reaches sizes[0] (the largest chunk grows with the board
    count), then the first count behind it with such a tail."""
    def chunk_sizes(B):
        cam, board = view_tables(C, B)
        return [n for _, n in planned_chunks(cam, board, C, B, 6, n_cu)]
    lo, hi = 64, 1 << 18
    if max(chunk_sizes(lo)) in sizes:
        hi = 4 * n_cu          # (the floor of the rule: any small count serves; about one chunk per CU pair)
    else:
        assert max(chunk_sizes(hi)) >= sizes[0]
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if max(chunk_sizes(mid)) >= sizes[0] else (mid, hi)
    for B in range(hi + 3, hi + 3 + 40 * 7, 7):
        s = chunk_sizes(B)
        if max(s) in sizes and any(1 <= n <= 15 for n in s):
            return B
    raise AssertionError(f"no board count behind {hi} gives chunks of {list(sizes)} boards with a ragged tail")


@functools.lru_cache(maxsize=None)
def rig(name, n_cu):
    C, sizes = CASES[name]
    B = boards_for(C, sizes, n_cu)
    base = synth.make_problem(C, -(-2 * B // C) + 2, 4100 + C, cols=3, rows=2)
    assert base.n_boards >= B and base.n_points == 6
    first, second, third = visibility(C, B)
    bv = np.asarray(base.view_board)
    assert np.array_equal(bv[:2 * B], np.repeat(np.arange(B), 2))         # frame-major, camera a then camera b
    u = base.obs_u.reshape(-1, 6)[:2 * B].reshape(B, 2, 6)
    v = base.obs_v.reshape(-1, 6)[:2 * B].reshape(B, 2, 6)
    # the third camera's view of a board seen by all three: the exact projection of the ground truth plus the same noise
    # (image bounds ignored, as tests/helpers.py rig_with_pairs does)
    b3 = np.nonzero(third)[0]
    m3 = (b3 + 2) % C
    gt_i, gt_c, gt_b = base.meta["gt_intr"], base.meta["gt_cam_rt"], base.meta["gt_board_rt"]
    P3 = np.concatenate([base.board_xy, np.zeros((6, 1))], axis=1)
    Pw = np.einsum("bij,nj->bni", synth.rodrigues(gt_b[b3, :3]), P3) + gt_b[b3, None, 3:]
    Pc = np.einsum("bij,bnj->bni", synth.rodrigues(gt_c[m3, :3]), Pw) + gt_c[m3, None, 3:]
    u3, v3, ks = synth.ts_project(gt_i[m3][:, None, :], Pc)
    assert np.all(ks > 1e-3)
    rng = np.random.default_rng(77)
    u3 = u3 + base.meta["noise_px"] * rng.normal(size=u3.shape)
    v3 = v3 + base.meta["noise_px"] * rng.normal(size=v3.shape)
    cam, board = view_tables(C, B)
    obs_u = np.concatenate([u[first, 0].ravel(), u[second, 1].ravel(), u3.ravel()])
    obs_v = np.concatenate([v[first, 0].ravel(), v[second, 1].ravel(), v3.ravel()])
    V = len(cam)
    p = Problem(C, B, base.board_xy, cam.astype(np.int32), board.astype(np.int32), (np.arange(V) * 6).astype(np.int32),
                np.full(V, 6, dtype=np.int32), obs_u, obs_v, base.cam_rt.copy(), base.intr.copy(), base.board_rt[:B].copy(),
                base.cam_pose_constant.copy(), False, meta=dict(base.meta))
    return p.normalised()


def problem(name, device):
    """The rig of a case, registered with tests/test_gpu_step.py's problem table so that its measure() serves it."""
    key = f"schur_deal_{name}"
    if key not in G.BUILDERS:
        G.BUILDERS[key] = lambda: rig(name, N_CUS)
    return key, G.problem(key)


@pytest.mark.parametrize("name", sorted(CASES))
def test_planned_chunks_are_the_sizes_the_case_is_for(hip_device, name):
    C, sizes = CASES[name]
    _, p = problem(name, hip_device)
    chunks = planned_chunks(np.asarray(p.view_camera), np.asarray(p.view_board), C, p.n_boards, 6, N_CUS)
    per_nv = {nv: [n for k, n in chunks if k == nv] for nv in (1, 2, 3)}
    assert all(per_nv[nv] for nv in range(1, C + 1)), per_nv                     # k_schur_gram<1 .. C>
    assert any(n in sizes for n in per_nv[2]) and max(n for _, n in chunks) in sizes, per_nv
    assert any(1 <= n <= 15 for _, n in chunks), per_nv                          # a ragged signature tail
    assert len(chunks) > 1                                                        # more than one workgroup


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_against_extended_precision(hip_device, name):
    key, _ = problem(name, hip_device)
    case = (key, key, {})
    e, d, _ = G.measure(case, hip_device)
    assert d["valid"], d
    tau_b, tau_f, tau_rd = G.tolerances(case, d["kappa"], d["cost"], d["model"])
    print(name, "backward", e["backward"], "forward", {k: e[k] for k in ("forward_cam_pose", "forward_intr", "forward_board")}, "kappa", d["kappa"])
    assert e["backward"] <= tau_b, (e["backward"], d)
    for k in ("forward_cam_pose", "forward_intr", "forward_board"):
        assert not e[k] > tau_f, (k, e[k], tau_f, d)
    assert abs(d["step_norm"] - d["step_norm_ref"]) <= tau_f * d["step_norm_ref"], d
    assert abs(d["relative_decrease"] - d["relative_decrease_ref"]) <= tau_rd * max(1.0, abs(d["relative_decrease_ref"])), (tau_rd, d)


@pytest.mark.parametrize("name", sorted(CASES))
def test_natural_solve_against_the_oracle(hip_device, name):
    import bench
    _, p = problem(name, hip_device)
    L = orc.lib()
    L.orc_set_num_threads(min(int(L.orc_max_threads()), bench._usable_cores(), 64))     # (as the config 5 parity test does)
    try:
        pg, po, gs, os_ = P._solve_both(p)
    finally:
        L.orc_set_num_threads(1)
    P._cmp_trace(gs, os_)
    e = H.param_rel_err(pg, po)
    print(name, "iterations", gs["num_iterations"], "parameter errors", e)
    assert max(e.values()) < PARAM_RTOL, e


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_bits_do_not_depend_on_rot(hip_device, name):
    _, p = problem(name, hip_device)
    out = {}
    for rot in (0, 2):
        q = p.copy().normalised()
        with api.Solver(q, hip_device) as s:
            s.debug_schur_rot(rot)
            r = s.solve(max_num_iterations=3, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
            cam, intr, board = s.download_params()
        out[rot] = (np.array([it["cost"] for it in r["iterations"]]), cam, intr, board)
        assert r["num_iterations"] == 4              # (the initial evaluation and three steps)
    for a, b in zip(out[0], out[2]):
        assert np.array_equal(a, b)
