"""CPU tests of tests/rig_ref.py, the long-double reference and a-priori bound for the rig-initialisation
kernels: the reference against mpmath, the oracle's fp64 errors inside the bound, kernel-shaped mistakes
far outside it, and the host rules that make every row of the GPU case table reach what it is meant to."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tests import rig_ref as R
from tscm_calib_amd import lib, rig


def _case(name):
    row = next(r for r in R.STAGE_CASES if r[0] == name)
    _, K, n, skew, _ = row
    inp = R.stage_rig(K, n, skew, seed=K)
    Rp, tp = R.stage_pose()
    Rs, ts = R.host_hypotheses(inp, 1, Rp, tp)
    return inp, Rp, tp, Rs, ts


_REFS = {}


def _reference(name):
    if name not in _REFS:
        inp, Rp, tp, Rs, ts = _case(name)
        _REFS[name] = (inp, Rp, tp, Rs, ts) + R.stage_reference(inp, 1, Rp, tp, Rs, ts)
    return _REFS[name]


@pytest.fixture(scope="module", autouse=True)
def _report():
    worst = {}
    yield worst
    for k, (r, name) in sorted(worst.items()):
        print(f"\n[rig reference] {k}: largest |value - reference| / bound = {r:.3g} (case {name})")


def _mp_hypothesis_error(inp, i, Rp, tp, Rs, ts):
    """multi_calib.cpp:52-78 for one hypothesis at 50 digits, in the reference's own formulation
    (R_ki = camera_R_k Rs^T, R_k = R_ki R_i, P = R_k w + t_k)."""
    import mpmath as mp
    mp.mp.dps = 50
    M = lambda a: mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.asarray(a).reshape(3, 3)])
    V = lambda a: mp.matrix([mp.mpf(float(x)) for x in np.asarray(a).reshape(3)])
    from tests.helpers import np_Rt_to_R_t
    common = np.nonzero(inp.has[i - 1].astype(bool) & inp.has[i].astype(bool))[0]
    Rp_, tp_, Rs_, ts_ = M(Rp), V(tp), M(Rs), V(ts)
    W = [V(w) for w in inp.worlds]

    def proj(I, P):
        X, Y, Z = P[0], P[1], P[2]
        I = [mp.mpf(float(x)) for x in I]
        d1 = mp.sqrt(X * X + Y * Y + Z * Z)
        z1 = Z + I[4] * d1
        z2 = z1 + I[5] * mp.sqrt(X * X + Y * Y + z1 * z1)
        ks = z2 + I[6] / (1 - I[6]) * mp.sqrt(X * X + Y * Y + z2 * z2)
        return I[0] * X / ks + I[7] * Y / ks + I[2], I[8] * X / ks + I[1] * Y / ks + I[3]

    err = mp.mpf(0)
    for k in common:
        Ri, ti = np_Rt_to_R_t(inp.Rt[i, k]); Rk, tk = np_Rt_to_R_t(inp.Rt[i - 1, k])
        Ri, ti, Rk, tk = M(Ri), V(ti), M(Rk), V(tk)
        Rki = Rp_ * Rs_.T
        tki = tp_ - Rki * ts_
        for (Rv, tv, cam) in ((Rki * Ri, Rki * ti + tki, i - 1), (Rs_ * Rp_.T * Rk, Rs_ * Rp_.T * tk + ts_ - Rs_ * Rp_.T * tp_, i)):
            for c, w in enumerate(W):
                u, v = proj(inp.intr[cam], Rv * w + tv)
                err += mp.sqrt((mp.mpf(float(inp.pix_u[cam, k, c])) - u) ** 2 + (mp.mpf(float(inp.pix_v[cam, k, c])) - v) ** 2)
    return err


@pytest.mark.parametrize("name", ["K2_n4", "K9_n88", "K64_n1"])
def test_reference_agrees_with_mpmath(name, _report):
    import mpmath as mp
    inp, Rp, tp, Rs, ts, ref, bound = _reference(name)
    js = np.unique(np.linspace(0, len(Rs) - 1, 3).astype(int))
    worst = 0.0
    for j in js:
        m = _mp_hypothesis_error(inp, 1, Rp, tp, Rs[j], ts[j])
        d = abs(float(mp.mpf(str(ref[j])) - m))
        assert d < 1e-3 * bound[j], (j, d, bound[j])        # long double sits far inside the fp64 bound
        assert d < 1e-16 * float(m)
        worst = max(worst, d / bound[j])
    if worst >= _report.get("mpmath", (0.0, ""))[0]:
        _report["mpmath"] = (worst, name)


@pytest.mark.parametrize("name", [r[0] for r in R.STAGE_CASES])
def test_oracle_fp64_errors_lie_within_the_bound(name, _report):
    inp, Rp, tp, Rs, ts, ref, bound = _reference(name)
    o = orc.rig_hypothesis_errors(inp, 1, Rp, tp, Rs, ts)
    assert np.all(np.isfinite(o)) and np.all(np.isfinite(bound))
    ratio = np.abs(o - ref.astype(np.float64)) / bound
    assert ratio.max() <= 1.0, (int(np.argmax(ratio)), ratio.max())
    if ratio.max() > _report.get("oracle fp64", (0.0, ""))[0]:
        _report["oracle fp64"] = (float(ratio.max()), name)


def _np_kernel(inp, i, Rp, tp, Rs, ts, mistake=None, ksplit=1):
    """The kernel's chain in plain fp64 numpy, with optional kernel-shaped mistakes.  Returns [J] errors."""
    from tests.helpers import np_Rt_to_R_t
    common = np.nonzero(inp.has[i - 1].astype(bool) & inp.has[i].astype(bool))[0]
    K, n = common.size, inp.n_points
    per_board = np.zeros((len(Rs), K))
    seed = 1.0 + 5e-8 if mistake == "seed_only" else 1.0
    for d, (cam, other) in enumerate(((i, i - 1), (i - 1, i))):
        Rq, tq = np_Rt_to_R_t(inp.Rt[cam, common])
        q = np.einsum("kij,nj->kni", Rq, inp.worlds) + tq[:, None, :]
        I = inp.intr[other].copy()
        if mistake == "swap_intr":
            I = inp.intr[cam].copy()
        if mistake == "drop_skew":
            I[7:9] = 0.0
        beta = I[6] if mistake == "beta_alpha" else I[6] / (1.0 - I[6])
        pu, pv = inp.pix_u[other, common], inp.pix_v[other, common]
        for j in range(len(Rs)):
            A = Rp @ Rs[j].T if d == 0 else Rs[j] @ Rp.T
            a = tp - A @ ts[j] if d == 0 else ts[j] - A @ tp
            P = q @ A.T + a
            X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
            rho2 = X * X + Y * Y
            d1 = np.sqrt(Z * Z + rho2) * seed
            z1 = Z + I[4] * d1
            d2 = np.sqrt(z1 * z1 + rho2) * seed
            z2 = z1 + I[5] * d2
            d3 = np.sqrt(z2 * z2 + rho2) * seed
            ik = seed / (beta * d3 + z2)
            mx, my = X * ik, Y * ik
            du = pu - (I[0] * mx + I[7] * my + I[2])
            dv = pv - (I[8] * mx + I[1] * my + I[3])
            t = np.sqrt(du * du + dv * dv) * seed
            if mistake == "drop_last_corner":
                t = t[:, :-1]
            per_board[j] += t.sum(axis=1)
    if mistake in ("slice_dropped", "slice_twice"):
        per = K // ksplit if mistake == "slice_dropped" else -(-K // ksplit)
        out = np.zeros(len(Rs))
        for b in range(ksplit):
            out += per_board[:, b * per:min(K, b * per + per)].sum(axis=1)
        if mistake == "slice_twice":
            out += per_board[:, 0:per].sum(axis=1)
        return out
    return per_board.sum(axis=1)


MISTAKES = ["seed_only", "drop_skew", "swap_intr", "beta_alpha", "drop_last_corner", "slice_dropped", "slice_twice"]


@pytest.mark.parametrize("name", ["K9_n88", "K64_n1", "K127_n4"])
def test_kernel_shaped_mistakes_exceed_the_bound(name, _report):
    inp, Rp, tp, Rs, ts, ref, bound = _reference(name)
    ref = ref.astype(np.float64)
    plain = _np_kernel(inp, 1, Rp, tp, Rs, ts)
    assert np.max(np.abs(plain - ref) / bound) <= 1.0          # the restatement itself is inside
    K = len(Rs)
    ksplit = 4 if K % 4 else 3                                  # an uneven last slice, so `per` rounded down loses boards
    for m in MISTAKES:
        if m == "drop_skew" and not R.skew_instantiation(inp.intr, 1):
            continue
        got = _np_kernel(inp, 1, Rp, tp, Rs, ts, mistake=m, ksplit=ksplit)
        ratio = np.abs(got - ref) / bound
        assert ratio.min() >= 20.0, (m, ratio.min())
        key = f"mistake {m} (smallest)"
        if key not in _report or ratio.min() < _report[key][0]:
            _report[key] = (float(ratio.min()), name)


def test_case_table_reaches_every_partition_and_rule():
    """Derived from the host's rules alone: the rows of tests/test_gpu_rig_stages.py reach wave edges, both
    SKEW instantiations, every slicing shape, and the tie / NaN / refusal conditions they are built for."""
    Ks = {r[1] for r in R.STAGE_CASES}
    assert {1, 2, 63, 64, 65, 127, 128, 129, 300} <= Ks
    assert {1, 4, 54, 88} <= {r[2] for r in R.STAGE_CASES}
    assert set(R.SKEWS) == {r[3] for r in R.STAGE_CASES}
    lanes_last = set()
    shapes = set()
    for name, K, n, skew, forced in R.STAGE_CASES:
        inp = R.stage_rig(K, n, skew, seed=K)
        assert int(np.count_nonzero(inp.has[0] & inp.has[1])) == K
        assert R.skew_instantiation(inp.intr, 1) == (skew != "none")
        # the rig is of mixed visibility: boards seen by one camera only sit between the common ones
        assert inp.has[0].sum() > K and inp.has[1].sum() > K
        jg, _, _ = R.host_partition(K, 1)
        lanes_last.add(K - 64 * (jg - 1))                       # live lanes of the last hypothesis group
        for ks in forced:
            _, ksplit, slices = R.host_partition(K, ks)
            assert ksplit == ks and 1 <= ks <= K
            sizes = [k1 - k0 for k0, k1 in slices]
            assert sum(max(s, 0) for s in sizes) == K and slices[0][0] == 0
            if ks == 1:
                shapes.add("one slice")
            if ks == K and K > 1:
                shapes.add("one board per slice")
            if any(s <= 0 for s in sizes):
                shapes.add("empty trailing slice")
            if len({s for s in sizes if s > 0}) > 1:
                shapes.add("uneven last slice")
    assert {1, 2, 63, 64} <= lanes_last
    assert shapes == {"one slice", "one board per slice", "empty trailing slice", "uneven last slice"}
    assert R.host_partition(9, 4)[2][-1] == (9, 9)              # K = 9, ksplit = 4: the fourth slice is empty
    # the default rule on a device of 256 CUs at 8 resident waves per CU (the GPU test reads the real ksplit)
    assert R.host_partition(300, 0, resident=256 * 8)[1] == 300 and R.host_partition(5000, 0, resident=2048)[1] == 25
    # selection rules: strict < keeps the first of a tie, NaN is skipped, nothing < 1e10 is a refusal
    assert R.first_min([3.0, 1.0, 1.0]) == 1
    assert R.first_min([np.nan, 2.0, np.nan, 1.0]) == 3
    assert R.first_min([1e10, np.inf, np.nan]) == -1
    tie = R.stage_tie_rig()
    o = orc.rig_init(tie["inp"])
    assert o["rc"] == 0 and o["cam_choice"][1] == tie["first"]
    e = orc.rig_hypothesis_errors(tie["inp"], 1, np.eye(3), np.zeros(3), *R.host_hypotheses(tie["inp"], 1, np.eye(3), np.zeros(3)))
    assert e[tie["first"]] == e[tie["second"]] == e.min()
    nan = R.stage_nan_rig()
    e = orc.rig_hypothesis_errors(nan["inp"], 1, np.eye(3), np.zeros(3), *R.host_hypotheses(nan["inp"], 1, np.eye(3), np.zeros(3)))
    assert np.isnan(e[nan["hyp"]]) and np.isfinite(np.delete(e, nan["hyp"])).all()
    far = R.stage_refused_rig()
    e = orc.rig_hypothesis_errors(far, 1, np.eye(3), np.zeros(3), *R.host_hypotheses(far, 1, np.eye(3), np.zeros(3)))
    assert np.all(e >= 1e10) and orc.rig_init(far)["rc"] != 0


def test_stage_errors_argument_checks_before_the_device():
    inp = R.stage_rig(9, 4, "none", seed=9)
    Rp, tp = np.eye(3), np.zeros(3)
    for ks in (-1, 10):
        with pytest.raises(lib.TscmError) as e:
            rig.stage_errors(inp, 1, Rp, tp, ksplit=ks)
        assert e.value.code == -1 and "ksplit" in str(e.value)
    for i in (0, 2):
        with pytest.raises(lib.TscmError) as e:
            rig.stage_errors(inp, i, Rp, tp)
        assert e.value.code == -1 and "stage index" in str(e.value)
