"""Corner weights and corner masks on the GPU against the reference of tests/weights_ref.py.

1. The weighted normal equations of the WEIGHTED instantiations of k_eval_gram4 and k_eval_gram_f32, without and with a loss, at
   the bounds of test_gpu_robust.py, on its problems (single-pass, multi-pass, ragged, mono).
2. NaN in masked observations changes no output bit.
3. A suffix mask is the shortened problem.
4. The first trust-region step through each reduced-camera solver, with the rule of test_gpu_step.py.
5. A whole solve with a suffix mask over planted outliers against the oracle's LM on the shortened problem.
6. Bits: weights cleared is a fresh solver; all-ones weights are the plain Gram.
7. Batched mono, 8. local shards, 9. covariance, 10. refusals.
"""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import api, lib, synth
from tests import helpers as H
from tests import cov_ref as CR
from tests import robust_ref as R
from tests import weights_ref as W
from tests import test_gpu_step as S
from tests import test_gpu_trajectory as T
from tests.test_gpu_gram_kernels import f32_excess, g4_plan, ragged

pytestmark = pytest.mark.gpu

BLOCKS = ("board_gram", "board_grad", "view_cross", "cam_gram", "cam_grad")
LOSSES = [None, "huber", "cauchy"]
NAMES = ["9x6", "11x8", "ragged", "mono"]
# boards at the edges of the Gram kernels' table (eval_kernel), 2 cameras x 2 views each, with the seed of their weights: three
# corners (KS 1; the smallest board scattered_weights takes: it masks a first, a last and an interior corner of views of >= 3),
# 56 (KS 14, the largest single pass), 57 (two passes of KS 8, the first several-pass entry), 112 (two passes of KS 14, the last)
EDGES = {"3x1": (3, 1, 906), "8x7": (8, 7, 900), "19x3": (19, 3, 900), "14x8": (14, 8, 900)}
EDGE_PLANS = {"3x1": (1, 4, 1), "8x7": (1, 56, 14), "19x3": (2, 32, 8), "14x8": (2, 56, 14)}
_cache = {}


def _problem(name):
    """The problems of test_gpu_robust.py, their scattered weights (11x8: zeros on both sides of its pass boundary), the
    oracle's jets and a loss scale -- computed once."""
    if name not in _cache:
        if name == "9x6":
            p = synth.make_problem(4, 16, 501).normalised()
        elif name == "11x8":
            p = synth.make_problem(4, 12, 502, cols=11, rows=8, pitch=32.0).normalised()
        elif name == "ragged":
            p = ragged(synth.make_problem(4, 40, 503), 54, g4_plan(54)[1])
        elif name == "mono":
            p = synth.make_problem(1, 24, 504).normalised()
        else:
            p = synth.make_problem(2, 2, 505, cols=EDGES[name][0], rows=EDGES[name][1], pitch=32.0).normalised()
            assert g4_plan(p.n_points) == EDGE_PLANS[name]
        per = g4_plan(p.n_points)[1]
        seed = EDGES[name][2] if name in EDGES else 900 + sum(k not in EDGES for k in _cache)
        w = W.scattered_weights(p, seed, boundary=per if per < p.n_points else None)
        _cache[name] = (p, w, orc.evaluate(p, jets=True), R.median_scale(p))
    return _cache[name]


def _loss(kind, a):
    return None if kind is None else (kind, a)


def _check(g, o, p, fp32):
    assert abs(g["cost"] - o["cost"]) <= 1e-12 * o["cost"], (g["cost"], o["cost"])
    if fp32:
        e = H.gram_errors(g, o, p)
        print(f"[weights] fp32 excess {f32_excess(e):.3f}")
        assert f32_excess(e) <= 1.0, e
    else:
        e = H.block_errors(g, o, bool(p.mono))
        assert max(e.values()) <= 1e-11, e


@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("mask", [False, True], ids=["weights", "mask"])
@pytest.mark.parametrize("name", [*NAMES, *EDGES])
@pytest.mark.parametrize("kind", LOSSES)
def test_normal_equations(hip_device, kind, name, mask, fp32):
    p, w, jets, a = _problem(name)
    w = (w > 0).astype(np.float64) if mask else w
    assert 0.1 < np.mean(w == 0) < 0.3
    o = W.weighted_normal_equations(p, w, kind, a, jets=jets)
    g = api.normal_equations(p, hip_device, jacobian_fp32=fp32, loss=_loss(kind, a), weights=w)
    _check(g, o, p, fp32)


@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["11x8", "ragged"])
def test_nan_in_masked_observations_changes_nothing(hip_device, name, fp32):
    p, w, _, a = _problem(name)
    q = p.copy().normalised()
    first = np.cumsum(p.view_count) - p.view_count
    idx = np.concatenate([np.arange(o, o + c) for o, c in zip(p.view_offset, p.view_count)])[w == 0]
    assert first.size and idx.size
    q.obs_u[idx[0::3]] = np.nan
    q.obs_v[idx[1::3]] = np.inf
    q.obs_u[idx[2::3]] = -np.inf
    for loss in (None, ("huber", a)):
        g0 = api.normal_equations(p, hip_device, jacobian_fp32=fp32, loss=loss, weights=w)
        g1 = api.normal_equations(q, hip_device, jacobian_fp32=fp32, loss=loss, weights=w)
        for k in BLOCKS:
            assert np.array_equal(g0[k], g1[k]), k
        assert g0["cost"] == g1["cost"] and np.isfinite(g1["cost"])
    s0, s1 = api.step(p, hip_device, weights=w), api.step(q, hip_device, weights=w)
    assert all(np.array_equal(s0[k], s1[k]) for k in ("cam_rt", "intr", "board_rt")) and s0["summary"]["iterations"] == s1["summary"]["iterations"]


@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind", [None, "cauchy"])
@pytest.mark.parametrize("name", ["9x6", "11x8"])
def test_a_suffix_mask_is_the_shortened_problem(hip_device, name, kind, fp32):
    p, _, _, a = _problem(name)
    n, per = p.n_points, g4_plan(p.n_points)[1]
    pattern = np.array([n, 1, n - 1, 2, per, per + 1 if per < n else 3, per - 1, n])
    w, q = W.suffix_mask(p, pattern[(p.view_board // p.n_cameras) % pattern.size])
    o = H.normal_equations_from(q, *orc.evaluate(q, jets=True)[1:]) if kind is None else R.robust_normal_equations(q, kind, a)
    g = api.normal_equations(p, hip_device, jacobian_fp32=fp32, loss=_loss(kind, a), weights=w)
    _check(g, o, q, fp32)
    # ... and the device's own evaluation of the shortened problem, at the same bounds
    d = api.normal_equations(q, hip_device, jacobian_fp32=fp32, loss=_loss(kind, a))
    _check(g, dict(o, **{k: d[k] for k in BLOCKS}, cost=d["cost"]), q, fp32)


STEP_CASES = ["ring4", "ring6", "big12", "mono", "ring4-fp32", "big12-fp32"]


@pytest.mark.parametrize("case_id", STEP_CASES)
@pytest.mark.parametrize("kind", [None, "huber"])
def test_first_step(hip_device, kind, case_id):
    case = S.CASE_BY_ID[case_id]
    p = S.problem(case[1])
    opt = dict(case[2])
    a = R.median_scale(p)
    w = W.scattered_weights(p, 77)
    jets = W.weighted_jets(p, w, kind, a)
    ref = H.reference_step(p, terms=H.step_terms(p, jets=jets), **opt)
    assert ref["ok"]
    g = api.step(p, hip_device, loss=_loss(kind, a), weights=w, **opt)
    assert g["valid"]
    e = H.step_errors(p, ref, g)
    rc = H.reference_candidate(p, ref)
    q = p.copy().normalised()
    q.cam_rt[:], q.intr[:], q.board_rt[:] = rc["cam_rt"], rc["intr"], rc["board_rt"]
    rd_ref = (ref["cost"] - W.weighted_cost(orc.evaluate(q, jets=False)[1], w, kind, a)) / ref["model_cost_change"]
    tau_b, tau_f, tau_rd = S.tolerances(case, ref["kappa"], ref["cost"], ref["model_cost_change"])
    assert e["backward"] <= tau_b, e
    for k in ("forward_cam_pose", "forward_intr", "forward_board"):
        assert not e[k] > tau_f, (k, e[k], tau_f)
    it = g["summary"]["iterations"]
    assert abs(it[0]["cost"] - ref["cost"]) <= 1e-12 * ref["cost"]
    assert abs(it[1]["relative_decrease"] - rd_ref) <= tau_rd * max(1.0, abs(rd_ref)), (it[1]["relative_decrease"], rd_ref, tau_rd)
    assert g["summary"]["n_residual_blocks"] == int(np.sum(w > 0))


def _outlier_problem():
    """make_problem(4, 10): the last 1-6 corners of every view moved by 20-40 px, and the mask that takes them out"""
    p = synth.make_problem(4, 10, 614).normalised()
    rng = np.random.default_rng(8)
    keep = p.view_count - rng.integers(1, 7, p.n_views)
    w, short = W.suffix_mask(p, keep)
    idx = np.concatenate([np.arange(o, o + c) for o, c in zip(p.view_offset, p.view_count)])[w == 0]
    ang, mag = rng.uniform(0, 2 * np.pi, idx.size), rng.uniform(20.0, 40.0, idx.size)
    p.obs_u[idx] += mag * np.cos(ang)
    p.obs_v[idx] += mag * np.sin(ang)
    return p, w, short


def test_whole_solve_with_a_mask_over_outliers(hip_device):
    p, w, short = _outlier_problem()
    po = short.copy().normalised()
    os_ = orc.solve(po, **T.FORCED)
    pg = p.copy().normalised()
    with api.Solver(pg, hip_device, weights=w) as s:
        gs = s.solve(**T.FORCED)
        s.upload_params(p.cam_rt, p.intr, p.board_rt)
        g2 = s.solve_resident(**T.FORCED)
        cam2, intr2, board2 = s.download_params()
    T._compare(gs, os_)
    assert max(H.param_rel_err(pg, po).values()) < 1e-6, H.param_rel_err(pg, po)
    assert abs(gs["rmse"] - orc.rmse(po)) <= 1e-9 * orc.rmse(po)
    assert gs["n_residual_blocks"] == int(w.sum()) == po.n_corners
    assert g2["iterations"] == gs["iterations"] and g2["final_cost"] == gs["final_cost"] and g2["rmse"] == gs["rmse"]
    assert np.array_equal(intr2, pg.intr) and np.array_equal(cam2, pg.cam_rt) and np.array_equal(board2, pg.board_rt)
    # the one-shot entry point is the same solve, and the plain solve of the corrupted problem is another one
    p1 = p.copy().normalised()
    r1 = api.calibrate(p1, weights=w > 0, **T.FORCED)
    assert r1["iterations"] == gs["iterations"] and np.array_equal(p1.intr, pg.intr)
    # with a loss the rmse comes from the weighted reprojection launch
    p3 = p.copy().normalised()
    r3 = api.calibrate(p3, weights=w, loss=("huber", 1.0))
    q3 = short.copy().normalised()
    q3.cam_rt[:], q3.intr[:], q3.board_rt[:] = p3.cam_rt, p3.intr, p3.board_rt
    assert abs(r3["rmse"] - orc.rmse(q3)) <= 1e-12 * orc.rmse(q3) and r3["n_residual_blocks"] == po.n_corners


SUMMARY_FIELDS = ("termination_type", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost", "final_cost",
                  "n_residual_blocks", "lm_iterations", "iterations", "message", "rmse")


@pytest.mark.parametrize("loss", [None, ("cauchy", 0.5)], ids=["plain", "cauchy"])
def test_weights_cleared_is_a_fresh_solver(hip_device, loss):
    p = synth.make_problem(4, 10, 613).normalised()
    w = W.scattered_weights(p, 5)
    q0, q1 = p.copy().normalised(), p.copy().normalised()
    with api.Solver(q0, hip_device) as s:
        if loss:
            s.set_loss(*loss)
        r0 = s.solve()
    with api.Solver(q1, hip_device) as s:
        if loss:
            s.set_loss(*loss)
        s.set_corner_weights(w)
        rw = s.solve()
        q1.cam_rt[:], q1.intr[:], q1.board_rt[:] = p.cam_rt, p.intr, p.board_rt
        s.set_corner_weights(None)
        r1 = s.solve()
    assert rw["n_residual_blocks"] == int(np.sum(w > 0)) and rw["iterations"] != r0["iterations"]
    for k in SUMMARY_FIELDS:
        assert r1[k] == r0[k], k
    assert np.array_equal(q0.intr, q1.intr) and np.array_equal(q0.cam_rt, q1.cam_rt) and np.array_equal(q0.board_rt, q1.board_rt)


@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["9x6", "11x8", "mono"])
def test_unit_weights_are_the_plain_gram(hip_device, name, fp32):
    """All-ones weights without a loss: array_equal Gram blocks and gradients, cost within 1e-12.  On k_eval_gram4 this
    rests on the w_b entries' FMAs being written out in the plain instantiation's pairing (corner_geometry<WC, PIN_WB>):
    left to the compiler they missed the last bit in 7-12 % of the board-side entries."""
    p = _problem(name)[0]
    g0 = api.normal_equations(p, hip_device, jacobian_fp32=fp32)
    g1 = api.normal_equations(p, hip_device, jacobian_fp32=fp32, weights=np.ones(p.n_corners))
    for k in BLOCKS:
        d = np.abs(g0[k] - g1[k])
        print(f"[weights] unit weights {name} fp32={fp32} {k}: {int(np.count_nonzero(d))} of {d.size} entries differ, largest {d.max() / np.abs(g0[k]).max():.1e} of the block's largest entry")
    for k in BLOCKS:
        assert np.array_equal(g0[k], g1[k]), k
    assert abs(g1["cost"] - g0["cost"]) <= 1e-12 * g0["cost"]


@pytest.mark.parametrize("loss", [None, ("huber", 1.0)], ids=["plain", "huber"])
def test_batched_mono(hip_device, loss):
    """Three problems, the second without weights; each against its solo refinement at test_gpu_mono_batch.py's bounds for a
    loss: iteration count and pattern, costs to 1e-9, parameters to 1e-8."""
    ps = [synth.make_problem(1, 8 + 2 * i, 830 + i).normalised() for i in range(3)]
    ws = [W.scattered_weights(ps[0], 1), None, W.scattered_weights(ps[2], 2, mask=True)]
    solo = [p.copy().normalised() for p in ps]
    rs = [api.refinement(q, hip_device, loss=loss, weights=w) for q, w in zip(solo, ws)]
    batch = [p.copy().normalised() for p in ps]
    rb = api.refinement_batch(batch, hip_device, loss=loss, weights=ws)
    for (ok_s, s), (ok_b, b), qs, qb, w in zip(rs, rb, solo, batch, ws):
        assert ok_s == ok_b and s["num_iterations"] == b["num_iterations"]
        for x, y in zip(b["iterations"], s["iterations"]):
            assert x["step_is_successful"] == y["step_is_successful"]
            assert abs(x["cost"] - y["cost"]) <= 1e-9 * abs(y["cost"])
        assert max(H.param_rel_err(qb, qs).values()) < 1e-8
        assert b["n_residual_blocks"] == s["n_residual_blocks"] == (qs.n_corners if w is None else int(np.sum(w > 0)))
        assert abs(b["rmse"] - s["rmse"]) <= 1e-9 * s["rmse"]


@pytest.mark.parametrize("world", [2, 3])
def test_sharded(hip_device, world):
    p = H.small_rig(4, 30, seed=21)
    w = W.scattered_weights(p.normalised(), 9)
    q1 = p.copy().normalised()
    with api.Solver(q1, hip_device, weights=w) as s:
        s.set_loss("huber", 1.0)
        s1 = s.solve()
    q2 = p.copy().normalised()
    with api.Group(q2, world, hip_device, loss=("huber", 1.0), weights=w) as g:
        sums = g.solve()
    assert sums[0]["num_iterations"] == s1["num_iterations"] and sums[0]["message"] == s1["message"]
    for x, y in zip(sums[0]["iterations"], s1["iterations"]):
        assert x["step_is_successful"] == y["step_is_successful"]
        assert abs(x["cost"] - y["cost"]) <= 1e-9 * abs(y["cost"])
    assert max(H.param_rel_err(q2, q1).values()) < 1e-8
    assert abs(sums[0]["rmse"] - s1["rmse"]) <= 1e-10 * s1["rmse"]
    assert all(s["rmse"] == sums[0]["rmse"] and s["n_residual_blocks"] == int(np.sum(w > 0)) for s in sums)


def test_covariance(hip_device):
    p = H.small_rig(4, 8, seed=23).normalised()
    m = W.scattered_weights(p, 4, mask=True) > 0
    c = api.covariance(p, hip_device, weights=m)
    g = api.normal_equations(p, hip_device, weights=m)
    cam_free, board_free = CR.free_columns(p)
    r = api.covariance_from_normal_equations(p.view_camera, p.view_board, g["board_gram"], g["view_cross"], g["cam_gram"], cam_free, board_free, hip_device)
    assert c["status"] == 0 and np.array_equal(c["cam_cov"], r["cam_cov"]) and np.array_equal(c["board_cov"], r["board_cov"])
    assert c["dof"] + c["n_free"] == 2 * int(m.sum()) and c["cost"] == g["cost"]
    plain = api.covariance(p, hip_device)
    assert plain["dof"] + plain["n_free"] == 2 * p.n_corners


def test_refusals(hip_device):
    p = H.small_rig(4, 8, seed=22).normalised()
    w = W.scattered_weights(p, 6)
    with api.Group(p.copy().normalised(), 2, hip_device) as g:
        g.solvers[0].set_corner_weights(w)
        with pytest.raises(lib.TscmError) as e:
            g.solve()
        assert e.value.code == -1
    q = p.copy().normalised()
    for f in (lambda: api.calibrate(q, weights=w, exec_flags=lib.EXEC_GRAM_16X16),
              lambda: api.normal_equations(q, hip_device, exec_flags=lib.EXEC_GRAM_16X16, weights=w),
              lambda: api.step(q, hip_device, exec_flags=lib.EXEC_GRAM_16X16, weights=w)):
        with pytest.raises(lib.TscmError) as e:
            f()
        assert e.value.code == -5
    with api.Solver(q, hip_device) as s:
        s.set_corner_weights(w)
        with pytest.raises(lib.TscmError) as e:
            s.solve(exec_flags=lib.EXEC_GRAM_16X16)
        assert e.value.code == -5
        bad = w.copy()
        bad[7] = -0.5
        with pytest.raises(lib.TscmError) as e:
            s.set_corner_weights(bad)
        assert e.value.code == -1 and "corner weight 7" in str(e.value)


def test_solver_created_without_a_view_takes_later_weights(hip_device):
    """A Solver created with weights that drop view 0 (count 0): later weights go to the views it has, and None is the solve of
    those views without weights -- both equal to solves of the problem with view 0 taken out by hand."""
    p = synth.make_problem(4, 8, 615).normalised()
    n0 = int(p.view_count[0])
    w = W.scattered_weights(p, 11)
    w[:n0] = 0.0
    w2 = W.scattered_weights(p, 12)
    short = p.copy().normalised()
    short.view_count[0] = 0
    a, b = p.copy().normalised(), short.copy().normalised()
    with api.Solver(a, hip_device, weights=w) as s:
        s.set_corner_weights(w2)
        ra = s.solve()
        with pytest.raises(ValueError):
            s.set_corner_weights(np.where(np.arange(w2.size) < n0 + int(p.view_count[1]), 0.0, w2))
    rb = api.calibrate(b, hip_device, weights=w2[n0:])
    assert ra["iterations"] == rb["iterations"] and np.array_equal(a.intr, b.intr) and ra["n_residual_blocks"] == int(np.sum(w2[n0:] > 0))
    a, b = p.copy().normalised(), short.copy().normalised()
    with api.Solver(a, hip_device, weights=w) as s:
        s.set_corner_weights(None)
        ra = s.solve()
    rb = api.calibrate(b, hip_device)
    assert ra["iterations"] == rb["iterations"] and np.array_equal(a.intr, b.intr) and ra["n_residual_blocks"] == p.n_corners - n0
