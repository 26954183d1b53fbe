"""The reference LM step, its tolerances and the reach of tests/test_gpu_step.py (CPU: oracle and numpy only).

1. The longdouble reference step (tests/helpers.py reference_step) agrees with the same step taken at 50 digits (mpmath,
   dense normal equations, no Schur elimination), and with the oracle's own candidate (orc_solve, one iteration) within the
   oracle's fp64 error: the scaling, clamping, sign and column map are the oracle's.
2. Negative control: the reference is taken again with six mistakes a reduced-camera solver could make, and the backward
   error of test_gpu_step must see every one by at least MARGIN x its tolerance, fp64 and fp32 (the smallest signal
   measured is 3.6e-4: the right-hand side scaled twice on the mono problem, against TAU_B32 = 1e-6).
3. Coverage: by the library's own host plan of each problem (tests/native/launch_seq_check.cpp route: no Python copy of a
   dispatch rule), the cases of test_gpu_step reach every solver instantiation and option of its table.
"""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import lib, synth
from tests import helpers as H
from tests import native_check as N
from tests import test_gpu_step as G

MARGIN = 20.0
# Device figures the coverage section plans with (tscm_layout.h: LayoutDevice, tscm_exec_plan.h: ExecDevice), as the library
# measured them at creation on an MI355X for every problem of test_gpu_step: compute units, resident waves per CU of the
# Gram kernel, and resident workgroups per CU of the launches whose workgroups wait for each other
N_CUS, EVAL_WAVES_PER_CU = 256, 16
SCHUR_WGS_PER_CU = SCHUR_RIDE_WGS_PER_CU = (2, 2, 1)    # k_schur_gram<1..3> and k_schur_gram<1..3, true>
DENSE4_WGS_PER_CU = 3                                   # k_solve_reduced<4, 16, 64, true>
# k_solve_nd<tpt, true>: 2 on plans of 16,896 to 59,840 bytes of LDS, 1 on plans of 71,312 and 75,424 (8 cameras, dense)
ND_WGS_PER_CU, ND_LDS_SPLIT = (2, 1), 64 * 1024


def _opt_key(opt):
    return tuple(sorted((k, v) for k, v in opt.items() if k in ("initial_trust_region_radius", "min_lm_diagonal",
                                                                "max_lm_diagonal", "jacobi_scaling")))


# ----------------------------------------------------------------------------- 1. the reference itself
def mp_step(p, radius=1e4, lo=1e-6, hi=1e32, jacobi_scaling=1, dps=50):
    """The first LM step by dense normal equations at `dps` digits: J from the oracle's jets (fp64 values, exact here)."""
    import mpmath as mp
    mp.mp.dps = dps
    cost, res, Jc, Jb, Ji = orc.evaluate(p, jets=True)
    cols = H.step_columns(p)
    cf, bf = cols["cam_free"], cols["board_free"]
    cidx = {}
    for m in range(p.n_cameras):
        for a in range(H.CAM_W):
            if cf[m, a]:
                cidx[("c", m, a)] = len(cidx)
    for b in range(p.n_boards):
        for a in range(6):
            if bf[b]:
                cidx[("b", b, a)] = len(cidx)
    n = len(cidx)
    rows = []
    k = 0
    for v in range(p.n_views):
        m, b = int(p.view_camera[v]), int(p.view_board[v])
        for _ in range(int(p.view_count[v])):
            for r in range(2):
                row = {}
                for a in range(6):
                    if cf[m, a]:
                        row[cidx[("c", m, a)]] = mp.mpf(Jc[k, r, a])
                    if bf[b]:
                        row[cidx[("b", b, a)]] = mp.mpf(Jb[k, r, a])
                for a in range(H.N_INTR_FREE):
                    if cf[m, 6 + a]:
                        row[cidx[("c", m, 6 + a)]] = mp.mpf(Ji[k, r, a])
                rows.append((row, mp.mpf(res[k, r])))
            k += 1
    A = mp.zeros(n, n)
    g = mp.zeros(n, 1)
    for row, rr in rows:
        items = list(row.items())
        for i, a in items:
            g[i] += a * rr
            for j, c in items:
                A[i, j] += a * c
    s = [1 / (1 + mp.sqrt(A[i, i])) if jacobi_scaling else mp.mpf(1) for i in range(n)]
    As = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            As[i, j] = s[i] * A[i, j] * s[j]
        As[i, i] += min(max(As[i, i], mp.mpf(lo)), mp.mpf(hi)) / mp.mpf(radius)
    gs = mp.matrix([s[i] * g[i] for i in range(n)])
    y = mp.lu_solve(As, gs)
    delta = [-s[i] * y[i] for i in range(n)]
    out_c, out_b = np.zeros((p.n_cameras, H.CAM_W)), np.zeros((p.n_boards, 6))
    for key, i in cidx.items():
        (out_c if key[0] == "c" else out_b)[key[1], key[2]] = float(delta[i])
    return out_c, out_b, [delta[i] for i in range(n)], cidx


@pytest.mark.parametrize("opt", [dict(), dict(initial_trust_region_radius=1e-2), dict(jacobi_scaling=0)])
def test_reference_step_against_50_digits(opt):
    """2 cameras, 3 boards of 4 x 3 corners: the longdouble step within max(1e-15, 10 kappa eps_longdouble) (relative,
    2-norm) of the 50-digit one.  Measured: 1.4e-19 at radius 1e-2 (kappa 3), 2.8e-15 at the default radius (kappa 2e4),
    1.9e-15 without jacobi scaling (kappa 2e11) -- three orders under the fp64 error kappa eps_double of a kernel."""
    import mpmath as mp
    p = synth.make_problem(2, 3, 11, cols=4, rows=3)
    assert (p.n_cameras, p.n_boards) == (2, 3)
    ref = H.reference_step(p, **opt)
    assert ref["ok"]
    _, _, d50, cidx = mp_step(p, radius=opt.get("initial_trust_region_radius", 1e4), jacobi_scaling=opt.get("jacobi_scaling", 1))
    num, den = mp.mpf(0), mp.mpf(0)
    for (kind, i, a), j in cidx.items():
        v = ref["cam"][i, a] if kind == "c" else ref["board"][i, a]
        num += (mp.mpf(np.format_float_scientific(v, unique=True)) - d50[j]) ** 2      # (every digit of the longdouble)
        den += d50[j] ** 2
    assert float(mp.sqrt(num / den)) <= max(1e-15, 10 * ref["kappa"] * float(np.finfo(np.longdouble).eps))


@pytest.mark.parametrize("name", ["ring3", "ring4", "ring6", "big12_const3", "mixed6", "const_boards4", "idle_cam4",
                                  "unseen4", "free_gauge3", "mono", "mono_poses_fixed"])
def test_reference_step_is_the_oracles(name):
    """orc_solve's first (accepted) step against the reference: within C_KAPPA kappa eps of fp64, per kind of block."""
    p = G.problem(name)
    ref = G.reference(name, ())
    q = p.copy().normalised()
    s = orc.solve(q, max_num_iterations=1, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    assert s["iterations"][1]["step_is_successful"]
    e = H.step_errors(p, ref, dict(cam_rt=q.cam_rt, intr=q.intr, board_rt=q.board_rt))
    tau = G.C_KAPPA * ref["kappa"] * G.EPS64
    assert e["backward"] <= 1e-14, e
    for k in ("forward_cam_pose", "forward_intr", "forward_board"):
        assert not e[k] > tau, (k, e[k], tau)
    assert abs(s["iterations"][1]["relative_decrease"] - _relative_decrease(p, ref)) <= 1e-9


def _relative_decrease(p, ref):
    rc = H.reference_candidate(p, ref)
    q = p.copy().normalised()
    q.cam_rt[:], q.intr[:], q.board_rt[:] = rc["cam_rt"], rc["intr"], rc["board_rt"]
    return (ref["cost"] - orc.evaluate(q, jets=False)[0]) / ref["model_cost_change"]


# ----------------------------------------------------------------------------- 2. negative control
# mistake -> (problem, options) it is applied on (where the mistake changes something: a camera-pair tile, a board of
# more than three cameras, a constant camera pose next to a compact column, a radius where the damping matters)
MISTAKES = {
    "pair_tile_missing_board": [("ring4", {}), ("mixed6", {}), ("big12", {})],
    # (at radius >= 10 the transposed tile leaves the reduced system indefinite: the linear solve fails, an invalid step)
    "pair_block_transposed": [("ring4", dict(initial_trust_region_radius=1.0)), ("ring8", dict(initial_trust_region_radius=1.0)),
                              ("big12_const3", dict(initial_trust_region_radius=1.0)), ("mixed6", dict(initial_trust_region_radius=1.0))],
    "e_block_undamped": [("mixed4", dict(initial_trust_region_radius=1e-2)), ("mixed6", dict(initial_trust_region_radius=1e-2)),
                         ("mixed12", dict(initial_trust_region_radius=1e-2))],
    "damping_shifted": [("big12_const3", dict(initial_trust_region_radius=1e-2)), ("ring6", dict(initial_trust_region_radius=1e-2))],
    "backsub_other_camera": [("ring4", {}), ("ring8", {}), ("big12", {}), ("mixed6", {})],
    "scale_rhs_twice": [("ring4", {}), ("ring8", {}), ("big12", {}), ("mono", {})],
}


def test_backward_error_sees_every_mistake():
    smallest = np.inf
    for mistake, where in MISTAKES.items():
        for name, opt in where:
            p = G.problem(name)
            ref = G.reference(name, _opt_key(opt))
            bad = H.reference_step(p, terms=G.terms(name), mistake=mistake, **opt)
            assert bad["ok"], (mistake, name)
            e = H.step_errors(p, ref, H.reference_candidate(p, bad))
            assert e["backward"] >= MARGIN * G.TAU_B32, (mistake, name, e["backward"])
            smallest = min(smallest, e["backward"])
    assert smallest >= 3e-4, smallest            # the value recorded in the module docstring


def test_backward_error_of_the_reference_candidate_is_rounding_only():
    """The reference's own fp64 candidate passes far inside TAU_B: the ulp allowance covers the candidate's rounding."""
    for name in ("ring4", "big12_const3", "mixed6", "mono", "many_boards4"):
        p, ref = G.problem(name), G.reference(name, ())
        e = H.step_errors(p, ref, H.reference_candidate(p, ref))
        assert e["backward"] <= 1e-14 and max(e["forward_cam_pose"], e["forward_intr"], e["forward_board"]) <= 1e-15, (name, e)


# ----------------------------------------------------------------------------- 3. coverage
@pytest.fixture(scope="module")
def planner():
    return N.built("launch_seq_check.cpp", "launch_seq_check")


def plan_of(p, opt, planner):
    """What creation and a solve decide on the host for problem p: `launch_seq_check route` runs plan_layout, plan_columns,
    plan_exec and the launch sequence of two iterations on the problem's view tables, flags and the figures above."""
    rows = np.stack([np.asarray(p.view_camera), np.asarray(p.view_board), np.asarray(p.view_count)], axis=1)
    bc = p.board_pose_constant
    words = [p.n_cameras, p.n_boards, p.n_points, int(p.mono), len(rows), *rows.ravel().tolist(),
             *np.asarray(p.cam_pose_constant).tolist(), *([0] if bc is None else [1, *np.asarray(bc).tolist()]), 0,
             opt.get("exec_flags", 0), opt.get("jacobian_fp32", 0), lib.LOSS_NONE, 0,
             N_CUS, EVAL_WAVES_PER_CU, *SCHUR_WGS_PER_CU, *SCHUR_RIDE_WGS_PER_CU, DENSE4_WGS_PER_CU, *ND_WGS_PER_CU, ND_LDS_SPLIT]
    out = N.run(planner, "route", stdin=" ".join(map(str, words)))
    assert out["ok"], out
    return out


def route(case, planner):
    """What a solve of this case runs: the kernels and plan fields `launch_seq_check route` reports for it (the library's
    own host headers), and the facts about the problem and its options that the table names."""
    name, prob, opt = case
    p = G.problem(prob)
    cols = H.step_columns(p)
    out = plan_of(p, opt, planner)
    x = out["plan"]
    kernels = set(out["begin"] + out["first"] + out["iteration"] + out["finish"])
    r = set()
    if x["solver"] == "dense4":
        r.add("k_solve_reduced<4,16,64>")
    elif x["solver"] == "nd":
        r.add(f"k_solve_nd<{out['nd_tpt']}>" + (" dense plan" if out["nd_dense"] else " graph plan") + (f" C<={out['dense4_cams']}" if p.n_cameras <= out["dense4_cams"] else ""))
    elif x["solver"] == "big":
        r.add("k_solve_reduced_big")
        r.add("compact columns % 16 == 0" if out["n_act"] % 16 == 0 else "compact columns % 16 != 0")
        if p.cam_pose_constant[1:].any():
            r.add("constant camera pose after camera 0")
    # T reduction and back-substitution: in the reduced solve's launch, or launches of their own
    if x["t_in_solve"]:
        r.add("k_T_reduce fused")
    if "T_reduce" in kernels:
        r.add("k_T_reduce")
    if x["n_bs"]:
        r.add("k_backsub_prep fused")
    elif out["bs_ride_refused"]:
        r.add("fused back-substitution does not fit resident")
    r.add(f"k_backsub_prep<{out['bs_threads']}>")
    r |= {f"k_schur_gram<{nv}>" for nv in (1, 2, 3) if {f"schur{nv}", f"schur_ride{nv}"} & kernels}
    if "schur_factor" in kernels and "pair_gram" in kernels:
        r.add("k_schur_factor + k_pair_gram")
    bf = cols["board_free"]
    if (~bf & cols["board_seen"]).any():
        r.add("constant board poses")
    if not cols["board_seen"].all():
        r.add("unseen boards")
    if not cols["cam_free"][:, 6].all():
        r.add("camera without views")
    if not p.mono and not p.cam_pose_constant.any():
        r.add("free gauge")
    if p.mono:
        r.add("mono" + (", poses fixed" if not bf.any() else ""))
    rad = opt.get("initial_trust_region_radius", 1e4)
    r.add(f"radius {rad:g}")
    r.add(f"jacobi_scaling {opt.get('jacobi_scaling', 1)}")
    if opt.get("clamps"):
        o = G.options(case)
        ref = G.reference(prob, ())
        sc2 = ref["sc"] ** 2 if opt.get("jacobi_scaling", 1) else 1
        sb2 = ref["sb"] ** 2 if opt.get("jacobi_scaling", 1) else 1
        nrm = np.concatenate([np.asarray((sc2 * ref["nc"])[ref["cam_free"]], dtype=np.float64),
                              np.asarray((sb2 * ref["nb"])[ref["board_free"]], dtype=np.float64).ravel()])
        if (nrm < o["min_lm_diagonal"]).any() and (nrm > o["max_lm_diagonal"]).any():
            r.add("both LM diagonal clamps bind")
    if opt.get("jacobian_fp32"):
        r = {x + " fp32" for x in r if x.startswith("k_solve") or x.startswith("k_schur") or x == "mono"} | r
    return r


EXPECTED = {
    "k_solve_reduced<4,16,64>", "k_T_reduce fused", "k_T_reduce", "k_backsub_prep fused", "k_backsub_prep<256>",
    "k_solve_nd<1> graph plan C<=4", "k_solve_nd<1> graph plan", "k_solve_nd<2> graph plan", "k_solve_nd<1> dense plan",
    "k_solve_nd<2> dense plan", "k_solve_reduced_big", "k_backsub_prep<128>", "compact columns % 16 == 0",
    "compact columns % 16 != 0", "constant camera pose after camera 0", "k_schur_gram<1>", "k_schur_gram<2>",
    "k_schur_gram<3>", "k_schur_factor + k_pair_gram", "constant board poses", "camera without views", "free gauge",
    "unseen boards", "mono", "mono, poses fixed", "fused back-substitution does not fit resident", "radius 0.01",
    "radius 10000", "radius 1e+12", "jacobi_scaling 0", "jacobi_scaling 1", "both LM diagonal clamps bind",
    "k_solve_reduced<4,16,64> fp32", "k_solve_nd<1> graph plan fp32", "k_solve_nd<2> graph plan fp32",
    "k_solve_nd<2> dense plan fp32", "k_solve_reduced_big fp32", "k_schur_gram<1> fp32", "k_schur_gram<2> fp32",
    "k_schur_gram<3> fp32", "k_schur_factor + k_pair_gram fp32", "mono fp32",
}


def test_cases_reach_every_row_of_the_table(planner):
    reached = {}
    for case in G.CASES:
        for x in route(case, planner):
            reached.setdefault(x, []).append(case[0])
    missing = EXPECTED - set(reached)
    assert not missing, missing
    # the solver rows each have a case of their own (distinct instantiation or option)
    assert "ring4-separate" in reached["k_T_reduce"] and "ring4" in reached["k_T_reduce fused"]
    assert "ring4" in reached["k_solve_reduced<4,16,64>"] and "ring4-graph" in reached["k_solve_nd<1> graph plan C<=4"]
    assert "many_boards4" in reached["fused back-substitution does not fit resident"]
    assert set(G.VARIANT_CASES) <= set(G.CASE_BY_ID)
