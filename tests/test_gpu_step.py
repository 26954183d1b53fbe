"""The LM step of every reduced-camera solver against an extended-precision Schur solve.

tscm_eval_step_ex runs a solve's first iteration (the solve itself, stopped after one step) and returns its candidate
x + delta.  The cases below reach every solver path of that step (CASES: the route each one takes is asserted from the
problem definitions alone by tests/test_step_tolerance.py):
  k_solve_reduced<4, 16, 64> (fused and separate launches), k_solve_nd<1|2> on the camera-pair-graph plan and on the
  dense plan, k_solve_reduced_big with compact column counts divisible and not divisible by 16, k_schur_gram<1, 2, 3>,
  k_schur_factor + k_pair_gram, k_T_reduce fused and separate, k_backsub_prep<128 | 256> fused and separate (and fused
  back-substitution that does not fit resident), constant and absent blocks, mono, three radii, both clamps of the LM
  diagonal, jacobi_scaling 0 and 1, and the fp32-Jacobian tier.

Reference: tests/helpers.py reference_step -- the oracle's dual-number Jacobian, Ceres' LM scaling and damping, the Schur
elimination of every board, a Cholesky factorisation of the reduced system and back-substitution, all in np.longdouble
(validated against mpmath at 50 digits and against the oracle's own candidate by tests/test_step_tolerance.py).
Per case (helpers.step_errors, in the scaled space of the reference system A y = g):
  backward error, blockwise (each camera's free columns, each board): <= TAU_B (fp64), TAU_B32 (fp32 tier);
  forward error per kind of block (camera pose, intrinsics, board): <= max(TAU_F, C_KAPPA * kappa * eps), kappa = kappa_2
    of the scaled, damped reduced system, eps = 2^-53 (fp64) or TAU_F32 of the Gram kernels (fp32 tier);
  the summary's step norm and relative decrease against the reference's (the candidate cost = the oracle's cost at
    x + delta_ref);
  the fusion flags and the 16x16 Gram tile give the candidate's bits of the default launches (VARIANT_CASES);
  an accepted step is what Solver.solve(max_num_iterations=1) leaves in the parameters, bit for bit.
Measured on an MI355X (largest over the cases):
  fp64: backward error 2.8e-13 (radius 1e-2, where the rounding of x + delta is all there is: the reference's own fp64
        candidate has the same backward error on those cases), <= 3.5e-15 at the other radii; forward error 7e-12 where
        kappa < 1e6, at most 14 kappa eps everywhere (4.6e-5 at radius 1e12, kappa 4e12); step norm within 5e-5 relative.
  fp32 tier: backward error 5.7e-8; forward error 3.1e-3 (0.03 kappa TAU_F32); relative decrease within 4e-6.
tests/test_step_tolerance.py shows, without a GPU, that TAU_B and TAU_B32 see each of six kernel-shaped mistakes by at
least 20x (smallest signal 3.6e-4).  No kernel bug was found.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import api, lib, synth
from tests import helpers as H
from tests.test_gpu_gram_kernels import TAU_F32

# backward error: fp64 measured <= 2.8e-13 (the candidate's own rounding), fp32 tier <= 5.7e-8 (TAU_B32 = TAU_F32 / 10)
TAU_B, TAU_B32 = 1e-12, 1e-6
TAU_F, TAU_F32_FWD = 1e-9, 1e-3
C_KAPPA = 100.0
EPS64 = 2.0 ** -53
FLAG_SEP = lib.EXEC_SEPARATE_T_REDUCE | lib.EXEC_SEPARATE_BACKSUB
FUSION_FLAGS = (lib.EXEC_SEPARATE_T_REDUCE, lib.EXEC_SEPARATE_BACKSUB, lib.EXEC_SEPARATE_CONTROL, lib.EXEC_SEPARATE_STATS,
                lib.EXEC_SEPARATE_T_REDUCE | lib.EXEC_SEPARATE_BACKSUB | lib.EXEC_SEPARATE_CONTROL | lib.EXEC_SEPARATE_STATS,
                lib.EXEC_GRAM_16X16)


# ----------------------------------------------------------------------------- problems
def ring(C, vpc=6, seed=3, **kw):
    return synth.make_problem(C, vpc, seed, **kw)


def with_const_cams(p, cams):
    p.cam_pose_constant = np.zeros(p.n_cameras, dtype=np.uint8)
    p.cam_pose_constant[list(cams)] = 1
    return p.normalised()


def with_const_boards(p, every=3):
    p.board_pose_constant = (np.arange(p.n_boards) % every == 0).astype(np.uint8)
    return p.normalised()


def chain(C):
    return [(i, i + 1) for i in range(C - 1)]


def star(C):
    return [(0, i) for i in range(1, C)]


def complete(C):
    return list(itertools.combinations(range(C), 2))


def dense_incomplete(C):
    return [e for e in complete(C) if e != (0, 1)]


# problems by name (built once per session)
BUILDERS = {
    "ring2": lambda: ring(2),
    "ring3": lambda: ring(3),
    "ring4": lambda: ring(4),
    "ring5": lambda: ring(5),
    "ring6": lambda: ring(6),
    "chain5": lambda: H.rig_with_pairs(5, chain(5), frames_per_pair=4),
    "star6": lambda: H.rig_with_pairs(6, star(6), frames_per_pair=4),
    "complete6": lambda: H.rig_with_pairs(6, complete(6), frames_per_pair=2),
    "ring7": lambda: ring(7),
    "chain7": lambda: H.rig_with_pairs(7, chain(7), frames_per_pair=4),
    "ring8": lambda: ring(8),
    "complete8": lambda: H.rig_with_pairs(8, complete(8), frames_per_pair=2),
    "dense_incomplete8": lambda: with_const_cams(H.rig_with_pairs(8, dense_incomplete(8), frames_per_pair=2), []),
    "big9": lambda: ring(9, 4),
    "big12": lambda: ring(12, 4),
    "big12_const3": lambda: with_const_cams(ring(12, 4), [0, 5, 11]),
    "big16_free": lambda: with_const_cams(ring(16, 4), []),
    "big20": lambda: ring(20, 4),
    "big32": lambda: ring(32, 4),
    "mixed4": lambda: H.mixed_visibility_rig(5, n_frames=24, n_cameras=4),
    "mixed6": lambda: H.mixed_visibility_rig(6, n_frames=24, n_cameras=6),
    "mixed12": lambda: H.mixed_visibility_rig(7, n_frames=36, n_cameras=12),
    "const_boards4": lambda: with_const_boards(ring(4)),
    "const_boards6": lambda: with_const_boards(ring(6)),
    "idle_cam4": lambda: H.rig_with_pairs(4, [(0, 1), (1, 2)], frames_per_pair=6),
    "idle_cam6": lambda: H.rig_with_pairs(6, chain(5), frames_per_pair=4),
    "free_gauge3": lambda: with_const_cams(ring(3), []),
    "free_gauge6": lambda: with_const_cams(ring(6), []),
    "unseen4": lambda: H.rig_with_unseen_boards(ring(4), 3),
    "unseen9": lambda: H.rig_with_unseen_boards(ring(9, 4), 2),
    "mono": lambda: synth.make_problem(1, 20, 20241),
    "mono_poses_fixed": lambda: synth.make_config(1, poses_fixed=True),
    "many_boards4": lambda: synth.make_problem(4, 20000, 77, cols=3, rows=2),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    return BUILDERS[name]()


def clamp_options(name):
    """min_lm_diagonal / max_lm_diagonal between the quartiles of the scaled squared column norms: both clamps bind."""
    ref = reference(name, ())
    nrm = np.concatenate([np.asarray((ref["sc"] ** 2 * ref["nc"])[ref["cam_free"]], dtype=np.float64),
                          np.asarray((ref["sb"] ** 2 * ref["nb"])[ref["board_free"]], dtype=np.float64).ravel()])
    lo, hi = np.quantile(nrm, [0.25, 0.75])
    return dict(min_lm_diagonal=float(lo), max_lm_diagonal=float(hi))


# (case id, problem, options); options hold exec_flags and jacobian_fp32 as a solve takes them
CASES = []


def _case(name, prob, **opt):
    CASES.append((name, prob, opt))


for C in (2, 3, 4):
    _case(f"ring{C}", f"ring{C}")
    _case(f"ring{C}-separate", f"ring{C}", exec_flags=FLAG_SEP)
for C in (3, 4):
    _case(f"ring{C}-graph", f"ring{C}", exec_flags=lib.EXEC_GRAPH_REDUCED_ORDER)
for prob in ("ring5", "chain5", "ring6", "star6", "complete6", "ring7", "chain7", "ring8", "complete8", "dense_incomplete8"):
    _case(prob, prob)
for prob in ("ring5", "ring8", "star6"):
    _case(f"{prob}-dense", prob, exec_flags=lib.EXEC_DENSE_REDUCED_ORDER)
_case("ring6-separate", "ring6", exec_flags=FLAG_SEP)
_case("ring8-separate", "ring8", exec_flags=FLAG_SEP)
for prob in ("big9", "big12", "big12_const3", "big16_free", "big20", "big32"):
    _case(prob, prob)
for prob in ("mixed4", "mixed6", "mixed12", "const_boards4", "const_boards6", "idle_cam4", "idle_cam6", "free_gauge3",
             "free_gauge6", "unseen4", "unseen9", "mono", "mono_poses_fixed", "many_boards4"):
    _case(prob, prob)
for prob in ("ring4", "ring6", "big12"):
    for r in (1e-2, 1e12):
        _case(f"{prob}-radius{r:g}", prob, initial_trust_region_radius=r)
    _case(f"{prob}-noscale", prob, jacobi_scaling=0)
    _case(f"{prob}-clamps", prob, clamps=True)
_case("ring4-noscale-clamps", "ring4", jacobi_scaling=0, clamps=True)
for prob in ("ring3", "ring4", "ring6", "ring8", "dense_incomplete8", "big12", "big12_const3", "mixed4", "mixed6",
             "mixed12", "const_boards4", "mono", "many_boards4"):
    _case(f"{prob}-fp32", prob, jacobian_fp32=1)
_case("ring4-separate-fp32", "ring4", jacobian_fp32=1, exec_flags=FLAG_SEP)
_case("ring8-dense-fp32", "ring8", jacobian_fp32=1, exec_flags=lib.EXEC_DENSE_REDUCED_ORDER)

# one case per solver and launch shape: the fusion flags must not change a bit of the candidate
VARIANT_CASES = ["ring3", "ring4-graph", "ring6", "ring8", "ring5-dense", "big12_const3", "mixed6", "mono", "many_boards4",
                 "ring4-fp32", "big12-fp32"]


def options(case):
    name, prob, opt = case
    opt = dict(opt)
    if opt.pop("clamps", False):
        opt.update(clamp_options(prob) if "jacobi_scaling" not in opt else clamp_options_unscaled(prob))
    return opt


def clamp_options_unscaled(name):
    ref = reference(name, ())
    nrm = np.concatenate([np.asarray(ref["nc"][ref["cam_free"]], dtype=np.float64),
                          np.asarray(ref["nb"][ref["board_free"]], dtype=np.float64).ravel()])
    lo, hi = np.quantile(nrm, [0.25, 0.75])
    return dict(min_lm_diagonal=float(lo), max_lm_diagonal=float(hi))


@functools.lru_cache(maxsize=None)
def terms(name):
    return H.step_terms(problem(name))


@functools.lru_cache(maxsize=None)
def reference(name, opt_items):
    opt = dict(opt_items)
    r = H.reference_step(problem(name), terms=terms(name), **opt)
    assert r["ok"]
    return r


CASE_BY_ID = {c[0]: c for c in CASES}


def measure(case, device=0):
    """GPU candidate and reference of one case -> (errors, details)."""
    name, prob, _ = case
    opt = options(case)
    p = problem(prob)
    ref = reference(prob, tuple(sorted((k, v) for k, v in opt.items() if k in (
        "initial_trust_region_radius", "min_lm_diagonal", "max_lm_diagonal", "jacobi_scaling"))))
    g = api.step(p, device, **opt)
    e = H.step_errors(p, ref, g)
    rc = H.reference_candidate(p, ref)
    q = p.copy().normalised()
    q.cam_rt[:], q.intr[:], q.board_rt[:] = rc["cam_rt"], rc["intr"], rc["board_rt"]
    cand_cost = orc.evaluate(q, jets=False)[0]
    it = g["summary"]["iterations"][1]
    free = np.concatenate([np.asarray(ref["cam"], dtype=np.float64)[ref["cam_free"]],
                           np.asarray(ref["board"], dtype=np.float64)[ref["board_free"]].ravel()])
    step_norm = float(np.linalg.norm(free))
    rd = (ref["cost"] - cand_cost) / ref["model_cost_change"]
    d = dict(valid=g["valid"], kappa=ref["kappa"], step_norm=it["step_norm"], step_norm_ref=step_norm,
             relative_decrease=it["relative_decrease"], relative_decrease_ref=rd, cost=ref["cost"],
             model=ref["model_cost_change"], accepted=bool(it["step_is_successful"]))
    return e, d, g


def tolerances(case, ref_kappa, cost, model):
    fp32 = bool(case[2].get("jacobian_fp32"))
    tau_b = TAU_B32 if fp32 else TAU_B
    # fp32 tier: the system itself carries the Gram kernel's TAU_F32 (relative to the Cauchy-Schwarz bound of an entry)
    tau_f = max(TAU_F32_FWD, ref_kappa * TAU_F32) if fp32 else max(TAU_F, C_KAPPA * ref_kappa * EPS64)
    # the relative decrease: the candidate's cost change carries the cost's rounding (~1e-13 of it) over the model change;
    # a rejected step's (cost far above the model's: radius 1e12) is relative to its size
    tau_rd = max(tau_f, 1e-12 * cost / abs(model))
    return tau_b, tau_f, tau_rd


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", [c[0] for c in CASES])
def test_step_against_extended_precision(hip_device, case_id):
    case = CASE_BY_ID[case_id]
    e, d, _ = measure(case, hip_device)
    assert d["valid"], d
    tau_b, tau_f, tau_rd = tolerances(case, d["kappa"], d["cost"], d["model"])
    assert e["backward"] <= tau_b, (e["backward"], d)
    for k in ("forward_cam_pose", "forward_intr", "forward_board"):
        assert not e[k] > tau_f, (k, e[k], tau_f, d)
    assert abs(d["step_norm"] - d["step_norm_ref"]) <= tau_f * d["step_norm_ref"], d
    assert abs(d["relative_decrease"] - d["relative_decrease_ref"]) <= tau_rd * max(1.0, abs(d["relative_decrease_ref"])), (tau_rd, d)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", VARIANT_CASES)
def test_fusion_flags_keep_the_candidate_bits(hip_device, case_id):
    case = CASE_BY_ID[case_id]
    p, opt = problem(case[1]), options(case)
    base = api.step(p, hip_device, **opt)
    assert base["valid"]
    for f in FUSION_FLAGS:
        o = dict(opt, exec_flags=opt.get("exec_flags", 0) | f)
        g = api.step(p, hip_device, **o)
        for k in ("cam_rt", "intr", "board_rt"):
            assert np.array_equal(g[k], base[k]), (f, k)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", VARIANT_CASES + ["ring4-radius0.01", "big12-noscale", "unseen9", "free_gauge6"])
def test_accepted_step_is_what_the_solve_leaves(hip_device, case_id):
    """The entry point returns buffer 1; a one-iteration solve that accepts its step leaves the same bits in buffer 0."""
    case = CASE_BY_ID[case_id]
    p, opt = problem(case[1]), options(case)
    g = api.step(p, hip_device, **opt)
    assert g["summary"]["iterations"][1]["step_is_successful"], g["summary"]["iterations"]
    q = p.copy().normalised()
    with api.Solver(q, hip_device) as s:
        r = s.solve(max_num_iterations=1, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0, **opt)
        cam, intr, board = s.download_params()
    assert r["iterations"][1]["step_is_successful"]
    assert np.array_equal(intr, g["intr"]) and np.array_equal(board, g["board_rt"])
    if not p.mono:
        assert np.array_equal(cam, g["cam_rt"])
