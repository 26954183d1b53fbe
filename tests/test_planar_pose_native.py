"""The planar pose fit (tscm_calib_amd/csrc/tscm_planar_pose.h), the one copy behind k_estimate_extrinsic and the refit of
k_estimate_extrinsic_ransac, on the CPU: tests/native/planar_pose_check.cpp runs its serial instantiation per view, and every
stage is held to the extended-precision references of tests/init_ref.py and tests/init_ransac_ref.py with the assertions and
rounding bounds of the GPU tests (tests/init_stage_checks.py) -- a host build without contraction is a third order of the
same sums.  Built twice: plain, and under AddressSanitizer + UBSan.  No GPU."""
import functools

import numpy as np
import pytest

from tests import init_ransac_ref as Q
from tests import init_ref as R
from tests import init_stage_checks as S
from tests import native_check as N

pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("planar_pose_check.cpp", "planar_pose_check")
PLAIN_ROWS = [c[0] for c in R.EXTRINSIC_CASES + R.EXTRINSIC_SMALL]


@pytest.fixture(scope="module")
def _report():
    worst = {}
    yield worst
    capped = worst.pop("_capped", set())
    for k, (r, name) in sorted(worst.items()):
        print(f"\n[planar pose, host] {k}: largest |host - reference| / bound = {r:.3g} (case {name})")
    for name in sorted(capped):
        print(f"\n[planar pose, host] compared with the reference's iterate (no convergence in 10 steps): {name}")


def test_headers_are_plain_cpp17():
    N.assert_plain_cpp17("tscm_planar_pose.h")
    N.assert_plain_cpp17("tscm_math.h")


def _run(checker, intr, pu, pv, count, W, board_w, masks=None):
    """One view per entry: T, H [3,3], rv0, t0, rv, t, Rt [3,3], steps, code as the check printed them."""
    V, n = pu.shape
    parts = [intr, W.ravel(), count.astype(np.float64), pu.ravel(), pv.ravel()] + ([masks.astype(np.float64).ravel()] if masks is not None else [])
    text = f"{V} {n} {board_w} {int(masks is not None)}\n" + "\n".join(" ".join(float(x).hex() for x in p) for p in parts) + "\n"
    views = N.run(checker, stdin=text)["views"]
    assert len(views) == V
    return [{k: np.array(x, dtype=np.float64).reshape((3, 3) if k in ("T", "H", "Rt") else (3,)) if isinstance(x, list) else x for k, x in v.items()}
            for v in views]


def _assert_turn(v, r, where, name, report):
    if r.get("T") is not None and np.all(np.isfinite(r["T"].astype(np.float64))):
        rt = np.max(np.abs(v["T"] - r["T"].astype(np.float64))) / r["bT"]
        assert rt <= 1.0, (where, rt)
        S.note(report, "T", rt, name)


@functools.lru_cache(maxsize=None)
def _plain_refs(name):
    """The references of a row, computed once and shared (never written to)."""
    return R.extrinsic_refs(name)


@pytest.mark.parametrize("name", PLAIN_ROWS)
def test_all_corners_every_view(checker, name, _report):
    intr, pu, pv, count, W, cols, kinds = R.extrinsic_case(name)
    out = _run(checker, intr, pu, pv, count, W, cols)
    for k, (v, r) in enumerate(zip(out, _plain_refs(name))):
        where = f"{name} view {k} ({kinds[k]})"
        S.assert_exit_code(v["code"], r, where)
        assert np.isnan(v["Rt"]).all() == (v["code"] not in R.ESTIMATED), where      # a pose is written exactly when estimated
        _assert_turn(v, r, where, name, _report)
        S.assert_fit_stages(v, v["code"], r, where, name, _report, S.PLAIN_LABELS)


@functools.lru_cache(maxsize=None)
def _masked_refs(name):
    intr, pu, pv, count, W, cols, Hn, seed, thr = Q.case(name)[:9]
    return Q.ransac_refs(intr, pu, pv, count, W, cols, threshold_px=thr, n_hypotheses=Hn, seed=seed)


@pytest.mark.parametrize("name", [c[0] for c in Q.SMALL])
def test_masked_corners_every_view(checker, name, _report):
    """The refit's path: the corners of the reference's own mask per view.  Every view of both rows is decisive in the
    reference; one without a board or without a mask (no hypothesis, too few inliers) has no refit there, and the fit of no
    corners ends at the board's centre (0 / 0)."""
    intr, pu, pv, count, W, cols = Q.case(name)[:6]
    kinds = Q.case(name)[9]
    refs = _masked_refs(name)
    masks = np.array([r["mask"] if r.get("mask") is not None else np.zeros(W.shape[0], dtype=bool) for r in refs])
    out = _run(checker, intr, pu, pv, count, W, cols, masks)
    for k, (v, r) in enumerate(zip(out, refs)):
        where = f"{name} view {k} ({kinds[k]})"
        assert r["decisive"], where
        if r["code"] == R.NO_BOARD:
            assert v["code"] == R.NO_BOARD and np.isnan(v["T"]).all() and np.isnan(v["Rt"]).all(), where
            continue
        _assert_turn(v, r, where, name, _report)
        if r["refit"] is None:
            assert not masks[k].any() and v["code"] == R.DEGENERATE_BOARD and np.isnan(v["H"]).all() and np.isnan(v["Rt"]).all(), where
            continue
        S.assert_exit_code(v["code"], r["refit"], where)
        S.assert_fit_stages(v, v["code"], r["refit"], where, name, _report, S.RANSAC_LABELS)
