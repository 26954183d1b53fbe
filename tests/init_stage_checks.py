"""The stage assertions every run of the planar pose fit shares (tscm_calib_amd/csrc/tscm_planar_pose.h: k_estimate_extrinsic,
the refit of k_estimate_extrinsic_ransac, and the fit on the host), against a view of init_ref.extrinsic_view or
init_ransac_ref.refit."""
import numpy as np

from tests import init_ref as R

PLAIN_LABELS = dict(H="H (Hartley space)", pose0="rv0, t0 ({branch} branch)", final="rv, t (final)")
RANSAC_LABELS = dict(H="H_refit (Hartley space) / bound", pose0="rv0, t0 / bound", final="rv, t (final) / bound")


def ratio(diff, bound):
    """max |diff| / bound, where an exact match counts 0 (the identity branch's rotation has bound 0)."""
    diff = np.abs(diff)
    return float(np.max(np.where(diff == 0, 0.0, diff / np.where(bound > 0, bound, 1e-300))))


def note(report, kind, value, name):
    if kind not in report or value > report[kind][0]:
        report[kind] = (float(value), name)


def assert_exit_code(code, f, where):
    if f["decisive_code"]:
        assert code == f["code"], (where, code, f["code"])
    else:
        ok = {f["code"]} | ({R.CONVERGED, R.ITERATION_CAP} if f["code"] in (R.CONVERGED, R.ITERATION_CAP) else set())
        assert code in ok, (where, code, f["code"])


def assert_fit_stages(v, code, f, where, name, report, labels):
    """v: T, H, rv0, t0, rv, t, steps, Rt of one view as a run gave them; f: the reference of that view.  H in Hartley
    space, rv0 / t0 (with the alternative Rodrigues branches where the reference's is not decisive), the final pose against
    the reference or, where that is capped, its iterate, and Rt from the run's own stages."""
    if f.get("H") is None:
        return
    E = ((v["H"].astype(R.LD) - f["H"]) @ R.inv3(f["Nt"])).astype(np.float64)
    rh = np.max(np.abs(E)) / f["bHn"]
    assert rh <= 1.0, (where, rh)
    note(report, labels["H"], rh, name)
    if f.get("rv0") is None:
        return
    p0 = np.concatenate([v["rv0"], v["t0"]])
    r0 = np.concatenate([f["rv0"], f["t0"]]).astype(np.float64)
    rp0 = ratio(p0 - r0, f["bpose0"])
    if not f["rod_decisive"]:
        alt = [R.column_pose(f["H"], (b, s))[:2] for b, s in (("identity", None), ("pi", True), ("pi", False), ("generic", None))]
        rp0 = min([rp0] + [ratio(p0 - np.concatenate(a).astype(np.float64), f["bpose0"]) for a in alt])
    assert rp0 <= 1.0, (where, rp0)
    note(report, labels["pose0"].format(branch=f["rod"]["branch"]), rp0, name)
    if code not in R.ESTIMATED:
        return
    pf = np.concatenate([v["rv"], v["t"]])
    if f["code"] == R.GN_CHOLESKY:
        assert np.array_equal(pf, p0), where                               # the iterate before the break is kept
    if f["capped_ref"]:
        hist = f["hist"]
        ref = hist[min(int(v["steps"]), len(hist) - 1)]
        report.setdefault("_capped", set()).add(where)
    else:
        ref = (f["rv"], f["t"])
    rf = ratio(pf - np.concatenate(ref).astype(np.float64), f["bpose"])
    assert rf <= 1.0, (where, rf)
    note(report, labels["final"], rf, name)
    # Rt is what the stages imply: T^T [r1 r2 t] from the run's own T, rv, t
    want = R.rt_from_stages(v["T"], v["rv"], v["t"]).astype(np.float64)
    scale = np.array([1.0, 1.0, max(1.0, float(np.max(np.abs(v["t"]))))])
    assert np.max(np.abs(v["Rt"] - want) / scale) < 1e-13, where
