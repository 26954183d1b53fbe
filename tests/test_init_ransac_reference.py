"""The restatement of tests/init_ransac_ref.py on its own, and the argument checks of the two RANSAC entry points
through the C ABI (they come before any device is touched)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import init_ransac_ref as Q
from tests import init_ref as R
from tscm_calib_amd import lib, rig, synth


def test_mix_is_murmur3_fmix32():
    # fmix32 is a bijection with fmix32(0) = 0; the second value is the finaliser applied by hand
    assert Q.mix(0) == 0
    h = 1
    h ^= h >> 16; h = h * 0x85EBCA6B % 2**32; h ^= h >> 13; h = h * 0xC2B2AE35 % 2**32; h ^= h >> 16
    assert Q.mix(1) == h
    assert len({Q.mix(i) for i in range(4096)}) == 4096


@pytest.mark.parametrize("n", [4, 5, 6, 54, 65, 1024])
def test_samples_are_distinct_and_in_range(n):
    seen = set()
    for seed, k, h in itertools.product((0, 0xDEADBEEF), (0, 7), range(64)):
        s = Q.sample(seed, k, h, n)
        assert len(s) == 4 and len(set(s)) == 4 and all(0 <= i < n for i in s)
        seen.add(tuple(s))
    assert n == 4 or len(seen) > 32                                  # the draws depend on seed, view and hypothesis


def test_sample_positions_cover_the_range():
    # (word * m) >> 32 reaches both ends of 0 .. m-1
    firsts = {Q.sample(3, 0, h, 6)[0] for h in range(256)}
    assert firsts == set(range(6))


def test_lattice_collinearity_is_exhaustive_on_4x3():
    w, hgt = 4, 3
    for s in itertools.combinations(range(w * hgt), 4):
        pts = np.array([(i % w, i // w) for i in s])
        want = False
        for tri in itertools.combinations(range(4), 3):
            a, b, c = pts[list(tri)]
            want |= int(round(np.linalg.det(np.array([[a[0], a[1], 1], [b[0], b[1], 1], [c[0], c[1], 1]], dtype=float)))) == 0
        for perm in itertools.permutations(s):
            assert Q.collinear(perm, w) == want, s


def _clean_view(cols=9, rows=6, seed=4, noise=0.0):
    rng = np.random.default_rng(seed)
    intr = synth.CALIB_INTR[0].copy()
    bxy = synth.board_points(cols, rows, 40.0)
    n = cols * rows
    u, v = R.turned_view(intr, bxy, 0.3, -0.2, R.axis_angle([0.3, -0.5, 0.2], 0.5), 600.0, n // 2 - cols // 2 - 1)
    W = np.concatenate([bxy, np.zeros((n, 1))], 1)
    return intr, u + noise * rng.normal(size=n), v + noise * rng.normal(size=n), W, cols


def test_outlier_free_view_every_accepted_hypothesis_scores_all():
    intr, u, v, W, cols = _clean_view()
    r = Q.ransac_view(intr, u, v, W, cols, 0, threshold_px=1.0, n_hypotheses=64, seed=2)
    acc = r["score"] >= 0
    assert acc.sum() > 8 and (~acc).sum() > 0
    assert np.all(r["score"][acc] == W.shape[0]) and np.all(r["clean"])
    assert r["winner"] == int(np.flatnonzero(acc)[0]) and r["decisive"]
    assert r["mask"].all() and r["code"] == R.CONVERGED
    assert np.all(r["samples"][~acc] == -1)


def test_planted_outlier_is_never_in_the_mask():
    intr, u, v, W, cols = _clean_view(noise=0.1)
    for j, seed in ((0, 0), (17, 1), (53, 2), (26, 3)):
        uu = u.copy()
        uu[j] += 60.0
        r = Q.ransac_view(intr, uu, v, W, cols, 0, threshold_px=2.0, n_hypotheses=64, seed=seed)
        assert r["code"] == R.CONVERGED and not r["mask"][j] and r["n_inliers"] == W.shape[0] - 1
        # the mask is the winner's own verdict, its 4 corners included
        assert r["mask"][r["samples"][r["winner"]]].all()


def test_ties_go_to_the_lower_index():
    intr, u, v, W, cols = _clean_view()
    r = Q.ransac_view(intr, u, v, W, cols, 5, threshold_px=1.0, n_hypotheses=32, seed=9)
    best = r["score"].max()
    tied = np.flatnonzero(r["score"] == best)
    assert tied.size > 1 and r["winner"] == tied[0]


def test_no_hypothesis_when_every_corner_is_nan():
    intr, u, v, W, cols = _clean_view()
    r = Q.ransac_view(intr, np.full_like(u, np.nan), v, W, cols, 0, n_hypotheses=16)
    assert r["code"] == Q.NO_HYPOTHESIS and r["winner"] == -1 and not r["mask"].any() and np.all(r["score"] == -1)


def test_few_inliers_when_the_threshold_is_tiny():
    intr, u, v, W, cols = _clean_view(noise=0.5)
    r = Q.ransac_view(intr, u, v, W, cols, 0, threshold_px=1e-6, n_hypotheses=16)
    assert r["code"] == Q.FEW_INLIERS and r["winner"] >= 0 and not r["mask"].any() and r["n_inliers"] == 0
    assert 4 <= r["score"].max() < Q.default_min_inliers(W.shape[0])           # the 4 sampled corners fit exactly


@pytest.mark.parametrize("name", [c[0] for c in Q.SMALL])
def test_small_cases_are_decisive(name):
    intr, pu, pv, count, W, cols, Hn, seed, thr, kinds, moved = Q.case(name)
    refs = Q.ransac_refs(intr, pu, pv, count, W, cols, threshold_px=thr, n_hypotheses=Hn, seed=seed)
    assert sum(not r["decisive"] for r in refs) <= 0.05 * len(refs)
    for k, r in enumerate(refs):
        if kinds[k] == "all_nan":
            assert r["code"] == Q.NO_HYPOTHESIS
        if r["code"] in R.ESTIMATED and kinds[k] in ("outlier1", "outliers5") and cols >= 5:
            assert not (r["mask"] & moved[k]).any()


# ------------------------------------------------------------------------------------------------ C ABI, no device
def _call(stages=False, **over):
    """One call of an entry on a 2-view 4 x 3 problem with the arguments in `over` replaced; returns rc, message."""
    L = lib.lib()
    d = (C.c_double * 256)()
    cnt = (C.c_int * 2)(12, 12)
    ib = (C.c_int * 4096)()
    ub = (C.c_ubyte * 64)()
    prm = rig.ransac_params()
    a = dict(intr9=d, pix_u=d, pix_v=d, count=cnt, n_views=2, worlds=d, n_points=12, board_w=4, params=C.byref(prm), device_index=0,
             Rt=d, inlier=ub, n_inliers=ib, exit_code=ib, n_estimated=C.byref(C.c_int(0)), seconds_kernel=None)
    st = dict(samples=ib, score=ib, winner=ib, T=d, H_best=d, H_refit=d, pose0=d, pose=d, steps=ib, rms_px=d)
    tweak = over.pop("params_set", None)
    if tweak:
        for key, val in tweak.items():
            setattr(prm, key, val)
    for key, val in over.items():
        (a if key in a else st)[key] = val
    fn = L.tscm_estimate_extrinsic_ransac_stages if stages else L.tscm_estimate_extrinsic_ransac
    rc = fn(*a.values(), *(st.values() if stages else ()))
    return rc, L.tscm_last_error().decode()


def test_default_params():
    p = lib.CRansacParams()
    lib.lib().tscm_ransac_default_params(C.byref(p))
    assert (p.struct_size, p.threshold_px, p.n_hypotheses, p.min_inliers, p.seed) == (C.sizeof(lib.CRansacParams), 8.0, 256, 0, 0)
    assert C.sizeof(lib.CRansacParams) == 32
    q = rig.ransac_params(threshold_px=2.5, n_hypotheses=64, min_inliers=12, seed=7)
    assert (q.struct_size, q.threshold_px, q.n_hypotheses, q.min_inliers, q.seed) == (32, 2.5, 64, 12, 7)


@pytest.mark.parametrize("stages", [False, True])
def test_refusals_name_the_argument(stages):
    required = ["intr9", "pix_u", "pix_v", "count", "worlds", "params", "Rt", "inlier", "n_estimated"]
    if stages:
        required += ["samples", "score", "winner", "T", "H_best", "H_refit", "pose0", "pose", "steps", "rms_px"]
    for name in required:
        rc, msg = _call(stages, **{name: None})
        assert rc == -1 and name in msg, (name, rc, msg)
    for field, values in (("struct_size", (0, 24, 40)), ("threshold_px", (0.0, -1.0, float("nan"))), ("n_hypotheses", (0, -3, 4097)),
                          ("min_inliers", (-1, 1, 2, 3, 13))):
        for val in values:
            rc, msg = _call(stages, params_set={field: val})
            assert rc == -1 and field in msg, (field, val, rc, msg)
    for val in (4, 12):                                                   # the smallest and the largest min_inliers pass the checks
        assert _call(stages, params_set={"min_inliers": val}, device_index=10**6)[0] == -2
    for bw in (0, -1, 12):                                                # 12 / 2 - 12 / 2 - 1 < 0: the plain entry's rule
        rc, msg = _call(stages, board_w=bw)
        assert rc == -1 and "board" in msg
    rc, msg = _call(stages, n_points=3)
    assert rc == -1 and "n_points" in msg
    rc, msg = _call(stages, n_views=-1)
    assert rc == -1 and "n_views" in msg
    rc, msg = _call(stages, n_points=1025, board_w=32)
    assert rc == -5 and "n_points" in msg


@pytest.mark.parametrize("stages", [False, True])
def test_no_views_and_device_range(stages):
    done = C.c_int(5)
    rc, _ = _call(stages, n_views=0, pix_u=None, pix_v=None, count=None, Rt=None, inlier=None, n_estimated=C.byref(done),
                  device_index=10**6)                                    # nothing to do: no device is asked for
    assert rc == 0 and done.value == 0
    for dv in (-1, 10**6):
        rc, msg = _call(stages, device_index=dv)
        assert rc == -2, (dv, rc, msg)                                     # TSCM_E_NO_DEVICE, with or without a GPU
    rc, msg = _call(stages, device_index=10**6, params=None)                # the argument checks come first
    assert rc == -1 and "params" in msg
