"""Batched mono refinement (tscm_solve_mono_batch / api.refinement_batch) against solo solves.

Every problem of a batch must come back as the single-problem entry point returns it alone: the same termination,
iteration and step counts, the per-iteration cost trace to 1e-9 relative and the parameters to 1e-6 (the natural-solve
tier of test_gpu_parity.py).  Problems must not leak into each other (permutation, duplicates, a corrupted neighbour), a
terminated problem is frozen, and the refusals come back before any device is touched."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import api, lib, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu


def mono(views, seed, *, noise=0.1, cols=9, rows=6):
    return synth.make_problem(1, views, seed, noise_px=noise, cols=cols, rows=rows)


def solo(p, loss=None, fixed=None, **opt):
    q = p.copy().normalised()
    s = api.refinement(q, loss=loss, fixed=fixed, **opt)[1]
    return q, s


def batch(ps, loss=None, fixed=None, **opt):
    qs = [p.copy().normalised() for p in ps]
    out = api.refinement_batch(qs, loss=loss, fixed=fixed, **opt)
    return qs, [s for _, s in out]


def costs(s):
    return np.array([it["cost"] for it in s["iterations"]] + [s["final_cost"]])


def assert_solo_tier(qb, sb, qs, ss):
    for key in ("termination_type", "num_iterations", "num_successful_steps", "num_unsuccessful_steps"):
        assert sb[key] == ss[key], (key, sb[key], ss[key])
    assert [it["step_is_successful"] for it in sb["iterations"]] == [it["step_is_successful"] for it in ss["iterations"]]
    assert H.rel_err(costs(sb), costs(ss)) <= 1e-9
    e = H.param_rel_err(qb, qs)
    assert e["intr"] < 1e-6 and e["board_rt"] < 1e-6, e
    assert np.array_equal(qb.intr[:, 7:], qs.intr[:, 7:])           # b, c are inert


def assert_bits(qa, sa, qb, sb):
    assert np.array_equal(qa.intr, qb.intr) and np.array_equal(qa.board_rt, qb.board_rt)
    assert np.array_equal(costs(sa), costs(sb))
    for key in ("termination_type", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "message"):
        assert sa[key] == sb[key]


# ---------------------------------------------------------------------------------------------- 1. parity with solo
def _mixed_9x6():
    return [mono(20, 101), mono(185, 102, noise=0.3), mono(2000, 103), mono(20, 104, noise=0.02), mono(185, 105, noise=0.05),
            mono(60, 106, noise=0.5)]


def _mixed_11x8():
    return [mono(185, 201, cols=11, rows=8), mono(20, 202, cols=11, rows=8, noise=0.3)]


@pytest.mark.parametrize("board", ["9x6", "11x8"])
def test_parity_with_solo_solves(board):
    ps = _mixed_9x6() if board == "9x6" else _mixed_11x8()
    qb, sb = batch(ps)
    for p, q, s in zip(ps, qb, sb):
        qs, ss = solo(p)
        assert_solo_tier(q, s, qs, ss)
    assert len({s["num_iterations"] for s in sb}) > 1 or board == "11x8"      # the problems end at different iterations


def test_parity_with_oracle():
    ps = [mono(20, 301), mono(40, 302, noise=0.2)]
    qb, sb = batch(ps)
    for p, q, s in zip(ps, qb, sb):
        o = p.copy().normalised()
        r = orc.solve(o)
        assert s["num_iterations"] == r["num_iterations"] and s["termination_type"] == r["termination_type"]
        assert abs(s["final_cost"] - r["final_cost"]) <= 1e-9 * r["final_cost"]
        e = H.param_rel_err(q, o)
        assert e["intr"] < 1e-6 and e["board_rt"] < 1e-6, e


# ---------------------------------------------------------------------------------------------- 2. no leakage
def test_permutation_is_bit_identical():
    ps = [mono(20, 401), mono(185, 402, noise=0.2), mono(60, 403), mono(20, 404, noise=0.4)]
    qa, sa = batch(ps)
    perm = [2, 0, 3, 1]
    qb, sb = batch([ps[i] for i in perm])
    for j, i in enumerate(perm):
        assert_bits(qa[i], sa[i], qb[j], sb[j])


def test_duplicates_are_bit_identical():
    p = mono(185, 411, noise=0.2)
    qb, sb = batch([p, mono(20, 412), p])
    assert_bits(qb[0], sb[0], qb[2], sb[2])


def test_corrupted_neighbour_leaves_others_alone():
    ps = [mono(60, 421), mono(60, 422), mono(60, 423)]
    bad = ps[1].copy()
    n = bad.n_points
    for v in range(0, bad.n_views, 3):                   # corner order flipped on every third view
        o = bad.view_offset[v]
        bad.obs_u[o:o + n] = bad.obs_u[o:o + n][::-1].copy()
        bad.obs_v[o:o + n] = bad.obs_v[o:o + n][::-1].copy()
    qa, sa = batch(ps)
    qb, sb = batch([ps[0], bad, ps[2]])
    for i in (0, 2):
        assert_bits(qa[i], sa[i], qb[i], sb[i])
    assert not np.array_equal(qa[1].intr, qb[1].intr)


# ---------------------------------------------------------------------------------------------- 3. freezing
def test_terminated_problem_is_frozen():
    quick = synth.make_problem(1, 20, 431, noise_px=0.01, perturb=False)     # starts at the solution: ends within a few steps
    long_ = mono(185, 432, noise=0.3)
    long_.intr[:, :7] *= 1.1                                                   # far from the solution: runs into the cap
    opt = dict(max_num_iterations=5)
    qa, sa = batch([quick, long_], **opt)
    qb, sb = batch([quick], **opt)
    assert sa[1]["num_iterations"] == 6 and sa[1]["termination"] == "NO_CONVERGENCE"
    assert sa[0]["termination"] == "CONVERGENCE" and sa[0]["lm_iterations"] < sa[1]["lm_iterations"]
    assert_bits(qa[0], sa[0], qb[0], sb[0])
    # nothing moved behind the termination: the problem matches its solo solve, stopped where it stopped
    qs, ss = solo(quick, **opt)
    assert_solo_tier(qa[0], sa[0], qs, ss)


# ---------------------------------------------------------------------------------------------- 4. loss and masks
def test_huber_with_model_masks():
    ps = [mono(60, 441, noise=0.3), mono(185, 442), mono(20, 443, noise=0.2), mono(60, 444)]
    fixed = [0, 32, 16 | 32, 4 | 8]     # TS, DS (TSCM_MODEL_DS), UCM (TSCM_MODEL_UCM), principal point held
    loss = ("huber", 1.0)
    qb, sb = batch(ps, loss=loss, fixed=fixed)
    for p, f, q, s in zip(ps, fixed, qb, sb):
        qs, ss = solo(p, loss=loss, fixed=f)
        assert_solo_tier(q, s, qs, ss)
        held = [j for j in range(9) if (f >> j) & 1]
        assert np.array_equal(q.intr[0, held], p.intr[0, held])
        assert abs(s["rmse"] - ss["rmse"]) <= 1e-9 * ss["rmse"]


# ---------------------------------------------------------------------------------------------- 5. edge cases
def test_batch_of_one():
    p = mono(185, 451, noise=0.2)
    qb, sb = batch([p])
    qs, ss = solo(p)
    assert_solo_tier(qb[0], sb[0], qs, ss)
    assert sb[0]["n_residual_blocks"] == ss["n_residual_blocks"] and abs(sb[0]["rmse"] - ss["rmse"]) <= 1e-9 * ss["rmse"]


def test_no_views_and_all_held():
    empty = mono(20, 461)
    empty.view_count[:] = 0
    p = mono(60, 462)
    full = synth.make_problem(1, 20, 463)
    qb, sb = batch([empty, p, full], fixed=[0, 0, 127])
    qs, ss = solo(empty)
    assert sb[0]["termination_type"] == ss["termination_type"] and sb[0]["num_iterations"] == ss["num_iterations"]
    assert np.array_equal(qb[0].intr, qs.intr) and np.array_equal(qb[0].board_rt, qs.board_rt)
    qs, ss = solo(full, fixed=127)
    assert_solo_tier(qb[2], sb[2], qs, ss)
    assert np.array_equal(qb[2].intr, full.intr)
    qs, ss = solo(p)
    assert_solo_tier(qb[1], sb[1], qs, ss)


def _call(ps, opt=None, fixed=None, kind=0, scale=0.0, n=None):
    cps = (lib.CProblem * max(1, len(ps)))(*[lib.c_problem(p) for p in ps])
    o = opt or lib.default_options(True)
    sums = (lib.CSummary * max(1, len(ps)))()
    w = None if fixed is None else lib.ushort_ptr(np.asarray(fixed, dtype=np.uint16))
    return lib.lib().tscm_solve_mono_batch(cps, len(ps) if n is None else n, 0, C.byref(o), w, kind, scale, sums)


def test_refusals_leave_parameters_alone():
    a, b = mono(20, 471), mono(20, 472)
    keep = [(p.intr.copy(), p.board_rt.copy()) for p in (a, b)]
    assert _call([a, b], n=0) == -1                                   # TSCM_E_INVALID
    assert _call([a, b], fixed=[0, 1 << 12]) == -1
    assert _call([a, b], kind=9, scale=1.0) == -1
    assert _call([a, b], kind=1, scale=-1.0) == -1
    assert _call([a, b], opt=lib.default_options(True, max_num_iterations=300)) == -1
    assert _call([a, b], opt=lib.default_options(True, jacobian_fp32=1)) == -5      # TSCM_E_UNSUPPORTED
    assert _call([a, b], opt=lib.default_options(True, exec_flags=8)) == -5
    assert _call([a, mono(20, 473, cols=11, rows=8)]) == -5
    rig = synth.make_problem(2, 6, 474)
    assert _call([a, rig]) == -5
    dup = b.copy()                                                    # board 0 seen by two views with corners
    dup.view_board = dup.view_board.copy()
    dup.view_board[1] = dup.view_board[0]
    assert _call([a, dup]) == -1                                      # as tscm_solve_mono refuses it alone
    s = lib.CSummary()
    cp = lib.c_problem(dup)
    assert lib.lib().tscm_solve_mono(C.byref(cp), C.byref(lib.default_options(True)), C.byref(s)) == -1
    for p, (i, r) in zip((a, b), keep):
        assert np.array_equal(p.intr, i) and np.array_equal(p.board_rt, r)
