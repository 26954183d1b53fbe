"""The reference LM step, its tolerances and the reach of tests/test_gpu_step.py (CPU: oracle and numpy only).

1. The longdouble reference step (tests/helpers.py reference_step) agrees with the same step taken at 50 digits (mpmath,
   dense normal equations, no Schur elimination), and with the oracle's own candidate (orc_solve, one iteration) within the
   oracle's fp64 error: the scaling, clamping, sign and column map are the oracle's.
2. Negative control: the reference is taken again with six mistakes a reduced-camera solver could make, and the backward
   error of test_gpu_step must see every one by at least MARGIN x its tolerance, fp64 and fp32 (the smallest signal
   measured is 3.6e-4: the right-hand side scaled twice on the mono problem, against TAU_B32 = 1e-6).
3. Coverage: from the problem definitions alone (camera count, flags, camera-pair graph, cameras per board, constant
   blocks), the cases of test_gpu_step reach every solver instantiation and option of its table.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import lib, synth
from tests import helpers as H
from tests import test_gpu_step as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 20.0
N_CUS = 256          # MI355X compute units: what the solver's residency rules are evaluated with


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
def nd_plan():
    exe = os.path.join(ROOT, "tmp", "nd_plan_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "nd_plan_check.cpp")])
    return exe


def cams_per_board(p):
    cnt = np.asarray(p.view_count)
    return [tuple(sorted(set(np.asarray(p.view_camera)[(np.asarray(p.view_board) == b) & (cnt > 0)].tolist()))) for b in range(p.n_boards)]


def route(case, nd_plan):
    """What a solve of this case runs, mirrored from tscm_solver.hip (tscm_solver_create_sharded, run_lm_inner,
    enqueue_iteration) from the problem's definition alone."""
    name, prob, opt = case
    p = G.problem(prob)
    C, B = p.n_cameras, p.n_boards
    fl = opt.get("exec_flags", 0)
    cpb = cams_per_board(p)
    seen = [c for c in cpb if c]
    cols = H.step_columns(p)
    r = set()
    variant = 0 if C <= 4 else 1 if C <= 8 else 3
    nd = 1 if fl & lib.EXEC_DENSE_REDUCED_ORDER else 0
    graph = bool(fl & lib.EXEC_GRAPH_REDUCED_ORDER) or (variant == 0 and nd)
    if variant == 0 and not graph:
        r.add("k_solve_reduced<4,16,64>")
    elif variant <= 1:
        pairs = sorted({(a, b) for c in seen for a in c for b in c if a < b})
        gdesc = "pairs:" + ",".join(f"{a}-{b}" for a, b in pairs) if pairs else "pairs:"
        const_mask = sum(1 << m for m in range(C) if p.cam_pose_constant[m]) if not p.mono else (1 << C) - 1
        inactive = sum(1 << m for m in range(C) if not cols["cam_free"][m, 6])
        out = json.loads(subprocess.check_output([nd_plan, str(C), gdesc, str(const_mask), str(inactive), str(nd), "1"], text=True))
        assert out["ok"], (name, out)
        r.add(f"k_solve_nd<{out['tpt']}>" + (" dense plan" if out["dense"] else " graph plan") + (" C<=4" if C <= 4 else ""))
    else:
        r.add("k_solve_reduced_big")
        n_compact = int(cols["cam_free"].sum())
        r.add("compact columns % 16 == 0" if n_compact % 16 == 0 else "compact columns % 16 != 0")
        if p.cam_pose_constant[1:].any():
            r.add("constant camera pose after camera 0")
    # T reduction and back-substitution: fused into the reduced solve's launch on <= 8 cameras unless separated
    small = C <= 8
    r.add("k_T_reduce fused" if small and not fl & lib.EXEC_SEPARATE_T_REDUCE else "k_T_reduce")
    bs_threads = 256 if (B + 15) // 16 > 5 * N_CUS * 3 // 2 or small else 128
    n_bs = (B + (32 if bs_threads == 256 else 16) - 1) // (32 if bs_threads == 256 else 16)
    resident = 3 * N_CUS            # (k_solve_reduced / k_solve_nd fused launch: three workgroups per CU)
    if small and not fl & lib.EXEC_SEPARATE_BACKSUB and n_bs > resident - 1:
        r.add("fused back-substitution does not fit resident")
    elif small and not fl & lib.EXEC_SEPARATE_BACKSUB:
        r.add("k_backsub_prep fused")
    r.add(f"k_backsub_prep<{bs_threads}>")
    bf = cols["board_free"]
    for b, c in enumerate(cpb):
        if c and bf[b]:
            r.add(f"k_schur_gram<{len(c)}>" if len(c) <= 3 else "k_schur_factor + k_pair_gram")
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


def test_cases_reach_every_row_of_the_table(nd_plan):
    reached = {}
    for case in G.CASES:
        for x in route(case, nd_plan):
            reached.setdefault(x, []).append(case[0])
    missing = EXPECTED - set(reached)
    assert not missing, missing
    # the solver rows each have a case of their own (distinct instantiation or option)
    assert "ring4-separate" in reached["k_T_reduce"] and "ring4" in reached["k_T_reduce fused"]
    assert "many_boards4" in reached["fused back-substitution does not fit resident"]
    assert set(G.VARIANT_CASES) <= set(G.CASE_BY_ID)
