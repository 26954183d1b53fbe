"""Row- and view-level parity of the mono-initialisation kernels (tscm_init.hip) against the extended-precision
reference of tests/init_ref.py: every row sample of k_focal_rows, and every stage of k_estimate_extrinsic
(look-at turn, homography, pose from the columns, Gauss-Newton result, exit code), on the case tables there."""
import numpy as np
import pytest

from tests import init_ref as R
from tests import init_stage_checks as S
from tscm_calib_amd import lib, rig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _report():
    worst = {}
    yield worst
    capped = worst.pop("_capped", set())
    for k, (r, name) in sorted(worst.items()):
        print(f"\n[init stages] {k}: largest |gpu - reference| / bound = {r:.3g} (case {name})")
    for name in sorted(capped):
        print(f"\n[init stages] compared with the reference's iterate (no convergence in 10 steps): {name}")


_note = S.note
STAGE_KEYS = ("T", "H", "rv0", "t0", "rv", "t", "steps", "Rt")


@pytest.mark.parametrize("case", R.FOCAL_CASES, ids=[c[0] for c in R.FOCAL_CASES])
def test_focal_rows_every_row(hip_device, case, _report):
    pu, pv, count, w, h, cx, cy, kinds = R.focal_case(case[0])
    g = rig.estimate_focal_rows(pu, pv, count, w, h, cx, cy, hip_device)
    val, dec, bnd = R.focal_rows(pu, pv, count, w, h, cx, cy)
    assert g.shape == val.shape
    assert np.all(g[count == 0] == -1.0) and np.all(g[count > 0] != -1.0)
    assert np.array_equal(np.isnan(g), np.isnan(val))
    d = dec & ~np.isnan(val)
    assert np.array_equal(g[d] == -2.0, val[d] == -2.0), np.argwhere(d & ((g == -2.0) != (val == -2.0)))
    acc = d & (val > 0)
    ratio = np.abs(g[acc] - val[acc]) / bnd[acc]
    assert acc.sum() > 0 and ratio.max() <= 1.0, ratio.max()
    _note(_report, "focal gamma", ratio.max(), case[0])
    _note(_report, "focal rows not decisive (count)", float((~dec).sum()), case[0])
    # tscm_estimate_focal's mean and count are those of the row output, bit for bit, in (image, row) order
    f, used = rig.estimate_focal(pu, pv, count, w, h, cx, cy, hip_device)
    s, n = 0.0, 0
    for x in g.ravel():
        if x < 0.0:
            continue
        s += x
        n += 1
    mean = s / n if n else 0.0
    assert used == n and (f == mean or (np.isnan(f) and np.isnan(mean)))
    assert np.isnan(f) == bool(np.isnan(val).any())                       # the NaN row reaches the mean


def test_focal_rows_width_limits(hip_device):
    pu, pv, count, w, h, cx, cy, _ = R.focal_case("w32_rows128")
    wide = np.concatenate([pu.reshape(-1, w), pu.reshape(-1, w)[:, :1]], 1)
    with pytest.raises(lib.TscmError) as e:
        rig.estimate_focal_rows(wide, wide, count, 33, h, cx, cy, hip_device)
    assert e.value.code == -5
    with pytest.raises(lib.TscmError) as e:
        rig.estimate_focal(wide, wide, count, 33, h, cx, cy, hip_device)
    assert e.value.code == -5
    g = rig.estimate_focal_rows(np.zeros((0, 32 * 4)), np.zeros((0, 32 * 4)), np.zeros(0, dtype=np.int32), 32, 4, cx, cy, hip_device)
    assert g.shape == (0, 4)


def _sentinel(V):
    return np.arange(9 * V, dtype=np.float64).reshape(V, 3, 3) * -1.25 - 7.0


@pytest.mark.parametrize("case", R.EXTRINSIC_CASES, ids=[c[0] for c in R.EXTRINSIC_CASES])
def test_extrinsic_stages_every_view(hip_device, case, _report):
    name = case[0]
    intr, pu, pv, count, W, cols, kinds = R.extrinsic_case(name)
    V = count.shape[0]
    init = _sentinel(V)
    g = rig.estimate_extrinsic_stages(intr, pu, pv, count, W, cols, hip_device, Rt_init=init)
    refs = R.extrinsic_refs(name)
    written = 0
    for k, r in enumerate(refs):
        code = int(g["code"][k])
        where = f"{name} view {k} ({kinds[k]})"
        S.assert_exit_code(code, r, where)
        if code not in R.ESTIMATED:
            assert np.array_equal(g["Rt"][k], init[k]), where                # the caller's values stay
        else:
            written += 1
        if r.get("T") is not None and np.all(np.isfinite(r["T"].astype(np.float64))):
            rt = np.max(np.abs(g["T"][k] - r["T"].astype(np.float64))) / r["bT"]
            assert rt <= 1.0, (where, rt)
            _note(_report, "T", rt, name)
        S.assert_fit_stages({key: g[key][k] for key in STAGE_KEYS}, code, r, where, name, _report, S.PLAIN_LABELS)
    assert g["n_estimated"] == written == int(np.isin(g["code"], R.ESTIMATED).sum())
    # the default instantiation writes the same poses and count
    Rt, n = rig.estimate_extrinsic(intr, pu, pv, count, W, cols, hip_device, Rt_init=init)
    assert n == written and np.array_equal(Rt, g["Rt"])
