"""CPU checks of the next-best-view stage's definition (tscm.h: tscm_view_gain) and of the reference the GPU tests
compare with (tests/view_gain_ref.py): the factored form against a direct route and against 50-digit arithmetic with
difference-quotient rows, the chain rule of two views, the tolerance rule against planted mistakes, the mix of the shared
cases, the candidate generator, and every refusal of the library -- through the loaded library, without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import view_gain_ref as V
from tscm_calib_amd import api, lib

MULTI = ("rig4-54x67", "mixed65-cx_cy-65x67", "mixed65-ds1-6x67")


def _some(ref, inp, want: int):
    """up to `want` candidates of each kind of flags (one camera, a pair, a pair of which one contributes, nobody)"""
    fl = ref["flags"] & 3
    pair = np.array([c[0] != c[1] for c in inp["candidates"]])
    picks = []
    for sel in (~pair & (fl == 1), fl == 3, pair & (fl == 1), pair & (fl == 2), fl == 0):
        picks += [int(i) for i in np.nonzero(sel)[0][:want]]
    return picks


# ----------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_factored_form_equals_the_direct_route(name):
    """Sigma' and gain_logdet of the factored form (G, M = L L^T, Y, K) against (Sigma_free^-1 + E dS E^T)^-1 and two slogdets,
    both in longdouble.  The direct route inverts Sigma_free (condition 1e10 and more): it keeps condition * 2^-64."""
    inp, ref, _, _, _ = V.case(name)
    args, kw = V.call_args(inp)
    worst_ld, worst_cov = 0.0, 0.0
    for i in _some(ref, inp, 2):
        cand = inp["candidates"][i]
        r = V.candidate_ref(*args[:5], cand, **kw)
        d = V.direct_route(*args[:5], cand, border=kw["border"], min_corners=kw["min_corners"])
        worst_ld = max(worst_ld, abs(float(r["gain_logdet"] - d["gain_logdet"])) / max(float(r["gain_logdet"]), 1.0))
        worst_cov = max(worst_cov, V.cov_error(d["cam_cov"], r["cam_cov"]))
        zero = ~np.asarray(inp["cam_cov"]).reshape(r["cam_cov"].shape).any(axis=1)
        assert not np.asarray(r["cam_cov"])[zero].any()
    print(f"{name}: factored against direct, gain_logdet {worst_ld:.3e}, Sigma' {worst_cov:.3e}")
    assert worst_ld <= 1e-7 and worst_cov <= 1e-7


def test_one_candidate_against_50_digits():
    """A pair of which both cameras contribute, on the 6-corner board: gain_logdet and the visible counts against mpmath, whose
    rows are difference quotients of the projection chain -- E, F, both rotation branches' derivatives and the factored
    form at once."""
    inp, ref, _, _, _ = V.case("mixed65-ds1-6x67")
    args, kw = V.call_args(inp)
    i = int(np.nonzero((ref["flags"] & 3) == 3)[0][0])
    cand = inp["candidates"][i]
    mp = V.mp_candidate(*args[:5], cand, border=kw["border"], min_corners=kw["min_corners"])
    err = abs(float(ref["gain_logdet"][i] - mp["gain_logdet"])) / max(float(mp["gain_logdet"]), 1.0)
    print(f"candidate {i}: gain_logdet {float(ref['gain_logdet'][i])!r}, 50 digits {float(mp['gain_logdet'])!r}, difference {err:.3e}")
    assert list(ref["n_visible"][i]) == mp["n_visible"] and mp["gain_logdet"] > 0
    assert err <= 1e-9                                       # longdouble on a problem of condition 1e9: 1e9 * 2^-64


@pytest.mark.parametrize("name", MULTI)
def test_chain_rule(name):
    """gain(1) + gain(2 | Sigma after 1) == gain(2) + gain(1 | Sigma after 2), and the two orders leave the same Sigma'', in
    longdouble: four evaluations, each within the case's tolerance scaled from float64's rounding to longdouble's (2^-11)."""
    inp, ref, _, _, tol = V.case(name)
    bound = 4 * tol["logdet"] * 2.0 ** -11
    args, kw = V.call_args(inp)
    i, j = [int(k) for k in np.nonzero((ref["flags"] & 3) == 3)[0][:2]]
    c1, c2 = inp["candidates"][i], inp["candidates"][j]
    one = lambda cov, c: V.candidate_ref(args[0], args[1], cov, args[3], args[4], c, **kw)
    r1, r2 = one(inp["cam_cov"], c1), one(inp["cam_cov"], c2)
    r12, r21 = one(r1["cam_cov"], c2), one(r2["cam_cov"], c1)
    s12, s21 = r1["gain_logdet"] + r12["gain_logdet"], r2["gain_logdet"] + r21["gain_logdet"]
    print(f"{name}: {float(s12)!r} against {float(s21)!r}")
    assert abs(float(s12 - s21)) <= bound * max(float(s12), 1.0)
    assert V.cov_error(r12["cam_cov"], r21["cam_cov"]) <= bound
    assert r12["gain_logdet"] < r2["gain_logdet"]            # the second view gains less on what the first has left


# ----------------------------------------------------------------------------- the cases and the tolerance rule
@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_float64_and_longdouble_agree_on_every_count(name):
    """No candidate has a corner within 1e-9 of a visibility threshold, and the two restatements agree on flags and counts."""
    inp, ref, e64, amp, tol = V.case(name)
    args, kw = V.call_args(inp)
    r64 = V.view_gain_ref(*args, dtype=np.float64, **kw)
    assert not ref["near"].any()
    assert np.array_equal(r64["flags"], ref["flags"]) and np.array_equal(r64["n_visible"], ref["n_visible"])
    assert V.within(e64, tol)
    print(f"{name}: e64 {e64}, amp {amp}, tolerance {tol}")


@pytest.mark.parametrize("name", MULTI)
def test_the_multi_cases_mix_what_they_should(name):
    inp, ref, _, _, _ = V.case(name)
    cands, fl, nv = inp["candidates"], ref["flags"] & 3, ref["n_visible"]
    pair = np.array([c[0] != c[1] for c in cands])
    n, mc = inp["board_xy"].shape[0], inp["min_corners"]
    assert pair.any() and (~pair).any() and len(cands) == 67
    assert any(c[0] == 0 for c in cands) and any(c[0] > 0 for c in cands) and not inp["cam_rt"][0, :3].any() and inp["cam_rt"][1:, :3].any()
    assert any(not np.asarray(c[2])[:3].any() for c in cands)                                # w_board = 0
    assert (nv[:, 0] == n).any() and ((nv[:, 0] > 0) & (nv[:, 0] < n)).any() and (~pair & (nv[:, 0] == 0)).any()
    assert (pair & ((fl == 1) | (fl == 2))).any() and (pair & (fl == 3)).any()
    assert (nv[:, 0] == mc).any() and (nv[:, 0] == mc - 1).any()
    assert ((nv[:, 0] == mc) & (fl & 1 == 1)).any() and ((nv[:, 0] == mc - 1) & (fl & 1 == 0)).any()
    if name == "rig4-54x67":                                                                 # alpha of camera 2 is 0.3 there
        behind = 0
        for a, b, pose in cands:
            if a == 2:
                behind += int(_k_negative(inp, pose))
        assert behind >= 1
        assert inp["border"] == 20.0 and inp["weights"] is not None


def _k_negative(inp, pose) -> bool:
    from tests import uncert_ref as U
    rt, I = np.asarray(inp["cam_rt"], dtype=np.longdouble), np.asarray(inp["intr"], dtype=np.longdouble)[:, :7]
    Rb, _ = U.rotation_and_derivatives(np.asarray(pose[:3], dtype=np.longdouble))
    Rm, _ = U.rotation_and_derivatives(rt[2, :3])
    xy = np.asarray(inp["board_xy"], dtype=np.longdouble)
    P = np.concatenate([xy, np.zeros((xy.shape[0], 1), np.longdouble)], axis=1) @ Rb.T + np.asarray(pose[3:], dtype=np.longdouble)
    k = U.project_jacobian(I[2], P @ Rm.T + rt[2, 3:])[2]
    return bool((k <= 0).any())


def test_the_tolerance_rejects_every_mistake():
    """Each planted mistake leaves the tolerance (or changes a flag or a count) on at least one case; the float64 restatement
    stays within it on every case (test_float64_and_longdouble_agree_on_every_count)."""
    rejected = {m: [] for m in V.MISTAKES}
    for name in V.CASE_NAMES:
        inp, ref, e64, amp, tol = V.case(name)
        args, kw = V.call_args(inp)
        for m in V.MISTAKES:
            bad = V.view_gain_ref(*args, mistake=m, **kw)
            e = V.gain_errors(bad, ref)
            if not V.within(e, tol) or not V.discrete_agree(bad, ref)[0]:
                rejected[m].append((name, {k: f"{e[k] / tol[k]:.3g}" for k in tol}))
    for m, where in rejected.items():
        print(m, "rejected on", where)
    assert all(rejected.values()), [m for m, w in rejected.items() if not w]


# ----------------------------------------------------------------------------- the candidate generator
def test_view_candidates_is_deterministic_and_centred():
    inp = V.inputs("rig4-54x67")
    rt, I, xy = inp["cam_rt"], inp["intr"], inp["board_xy"]
    size = (V.IMG_W, V.IMG_H)
    a, info_a = api.view_candidates(rt, I, 1, size, xy, grid=(5, 3), distances=(300.0, 700.0), tilts_deg=(0.0, 25.0, -25.0), rolls_deg=(0.0, 30.0), pair=2)
    b, _ = api.view_candidates(rt, I, 1, size, xy, grid=(5, 3), distances=(300.0, 700.0), tilts_deg=(0.0, 25.0, -25.0), rolls_deg=(0.0, 30.0), pair=2)
    pixels = sorted({inf["pixel"] for inf in info_a})
    assert len(a) == len(pixels) * 2 * 5 * 2 == len(info_a) and 6 <= len(pixels) <= 15      # the image's corners lie outside the disc that unprojects
    assert all(x[0] == y[0] == 1 and x[1] == y[1] == 2 and x[2].tobytes() == y[2].tobytes() for x, y in zip(a, b))
    centre = np.append(xy.mean(axis=0), 0.0)
    from tests import uncert_ref as U
    for (ca, cb, pose), inf in zip(a, info_a):
        Rb, Rm = api._rotation_matrix(pose[:3]), api._rotation_matrix(rt[1, :3])
        p = Rm @ (Rb @ centre + pose[3:]) + rt[1, 3:]
        u, v, k, _, _, _ = U.project_jacobian(I[1, :7], p[None])
        assert k[0] > 0 and abs(u[0] - inf["pixel"][0]) < 1e-6 and abs(v[0] - inf["pixel"][1]) < 1e-6, inf
        assert abs(np.sqrt(p @ p) - inf["distance"]) < 1e-8
        if inf["tilt_x"] == 0 and inf["tilt_y"] == 0:           # it faces the camera: its normal is the ray
            assert np.allclose(Rm @ Rb[:, 2], p / np.sqrt(p @ p), atol=1e-9)
    alone, _ = api.view_candidates(rt, I, 0, size, xy)
    assert 0 < len(alone) <= 6 * 4 * 2 * 5 and len(alone) % (2 * 5) == 0 and all(c[0] == c[1] == 0 for c in alone)


# ----------------------------------------------------------------------------- refusals
def _call(L, apply=False, **over):
    inp = V.inputs("rig4-54x67")
    a = dict(n_cameras=4, cam_rt=inp["cam_rt"], intr=inp["intr"], cam_cov=inp["cam_cov"], weights=None, n_points=54, board_xy=inp["board_xy"],
             image_size=inp["image_size"], params=True, struct_size=C.sizeof(lib.CViewGainParams), border=0.0, min_corners=8,
             candidates=[(0, 1, inp["candidates"][0][2]), (2, 2, inp["candidates"][1][2])], n_candidates=None, gain_logdet=True, gain_trace=True,
             n_visible=True, flags=True, cam_cov_out=True, device=1 << 20)
    a.update(over)
    cs = a["candidates"]
    n = len(cs) if a["n_candidates"] is None and cs is not None else (a["n_candidates"] or 0)
    arr = None
    if cs is not None:
        arr = (lib.CViewCandidate * max(len(cs), 1))()
        for k, (ca, cb, r) in enumerate(cs):
            arr[k].camera_a, arr[k].camera_b = ca, cb
            arr[k].board_rt[:] = [float(x) for x in r]
    prm = lib.CViewGainParams(struct_size=a["struct_size"], min_corners=a["min_corners"], border=a["border"]) if a["params"] else None
    dp = lambda x: None if x is None else lib.dptr(np.ascontiguousarray(x, dtype=np.float64))
    size = None if a["image_size"] is None else np.ascontiguousarray(a["image_size"], dtype=np.int32)
    ip = C.POINTER(C.c_int)
    m = max(n, 1)
    ld, tr, nv, fl, out = np.zeros(m), np.zeros(m), np.zeros((m, 2), np.int32), np.zeros(m, np.int32), np.zeros((60, 60))
    head = (a["n_cameras"], dp(a["cam_rt"]), dp(a["intr"]), dp(a["cam_cov"]), dp(a["weights"]), a["n_points"], dp(a["board_xy"]),
            None if size is None else size.ctypes.data_as(ip), None if prm is None else C.byref(prm), arr)
    tail = (lib.dptr(ld) if a["gain_logdet"] else None, lib.dptr(tr) if a["gain_trace"] else None, nv.ctypes.data_as(ip) if a["n_visible"] else None,
            fl.ctypes.data_as(ip) if a["flags"] else None)
    if apply:
        return L.tscm_view_gain_apply(*head, a["device"], *tail, lib.dptr(out) if a["cam_cov_out"] else None)
    return L.tscm_view_gain(*head, n, a["device"], *tail)


@pytest.mark.parametrize("apply", [False, True])
def test_refusals_come_before_the_device(apply):
    """Every refusal is TSCM_E_INVALID (-1) with the argument named, with a device index that does not exist (which alone is
    TSCM_E_NO_DEVICE, -2): the arguments are checked first."""
    L = lib.lib()
    msg = lambda: L.tscm_last_error().decode()
    call = lambda **kw: _call(L, apply, **kw)
    inp = V.inputs("rig4-54x67")
    pose = inp["candidates"][0][2]
    assert call() == -2
    assert L.tscm_view_gain_seconds() == 0.0
    for key in ("cam_rt", "intr", "cam_cov", "board_xy", "image_size"):
        assert call(**{key: None}) == -1 and key in msg(), key
    assert call(candidates=None) == -1 and "candidate" in msg()
    for key in ("params", "gain_logdet", "gain_trace", "n_visible", "flags"):
        assert call(**{key: False}) == -1 and key in msg(), key
    if apply:
        assert call(cam_cov_out=False) == -1 and "cam_cov_out" in msg()
    assert call(struct_size=C.sizeof(lib.CViewGainParams) + 8) == -1 and "struct_size" in msg()
    for bad in (0, 33):
        assert call(n_cameras=bad) == -1 and "n_cameras" in msg()
    for bad in (0, 1025):
        assert call(n_points=bad) == -1 and "n_points" in msg()
    if not apply:
        for bad in (0, -1, (1 << 24) + 1):
            assert call(n_candidates=bad) == -1 and "n_candidates" in msg()
        assert call(candidates=[(0, 1, pose), (4, 0, pose)]) == -1 and "candidates[1]" in msg() and "camera_a" in msg()
    for bad in (4, -1):
        assert call(candidates=[(bad, 0, pose)]) == -1 and "camera_a" in msg()
        assert call(candidates=[(0, bad, pose)]) == -1 and "camera_b" in msg()
    for bad in (float("nan"), float("inf")):
        p = np.array(pose); p[4] = bad
        assert call(candidates=[(0, 1, p)]) == -1 and "board_rt[4]" in msg()
        for key, at in (("board_xy", (3, 1)), ("cam_rt", (2, 5)), ("intr", (1, 6))):
            x = np.array(inp[key]); x[at] = bad
            assert call(**{key: x}) == -1 and key in msg(), key
        assert call(border=bad) == -1 and "border" in msg()
        w = np.ones((4, 15)); w[3, 2] = bad
        assert call(weights=w) == -1 and "weights[47]" in msg()
    x = np.array(inp["intr"]); x[2, 8] = float("nan")               # b and c are not read
    assert call(intr=x) == -2
    assert call(border=-0.5) == -1 and "border" in msg()
    assert call(min_corners=3) == -1 and "min_corners" in msg()
    for at, bad in (((1, 0), 0), ((3, 1), -5)):
        s = np.array(inp["image_size"]); s[at] = bad
        assert call(image_size=s) == -1 and "image_size" in msg()
    w = np.ones((4, 15)); w[0, 0] = -1e-300
    assert call(weights=w) == -1 and "weights[0]" in msg()
    assert call(weights=np.zeros((4, 15))) == -2 and call(min_corners=4, border=0.0) == -2


def test_the_symbols_are_exported():
    assert {"tscm_view_gain", "tscm_view_gain_apply", "tscm_view_gain_seconds"} <= set(lib.EXPORTS)
    assert lib.lib().tscm_abi_version() == 6
    assert C.sizeof(lib.CViewGainParams) == 16 and C.sizeof(lib.CViewCandidate) == 56
