"""Host restatement of the per-camera visibility at the swept depth defined in include/tscm/tscm.h (tscm_sweep_visibility,
tscm_sweep_compose_visible): hypothesis and rank, the cell of a record, the depth buffers, the test, state and use, and the
composer on the masked alphas.  Records are taken from the tables exactly as k_sweep_prepare packs them: sx = rint(32 mapx) in
float32, ix = sx >> 5 saturated to int16; alpha is pano_ref.alpha.  The composer behind the mask -- sample, gain, label,
coverage, SEAM, FEATHER, the MULTIBAND pyramids -- is tests/pano_ref.py through tests/sweep_compose_ref.py, imported and not
copied.  Integer arithmetic throughout, so the device result is compared with array_equal."""
import numpy as np

from tests import pano_ref
from tests import sweep_compose_ref as CR

SEAM, FEATHER, MULTIBAND = CR.SEAM, CR.FEATHER, CR.MULTIBAND
DEFAULTS = dict(cell_shift=2, tolerance=2, dilate=0, near_is_high=1)


def record_positions(mapx, mapy):
    """(ix, iy) of the packed records of float32 tables of any shape"""
    out = []
    for m in (mapx, mapy):
        s = np.rint(np.asarray(m, dtype=np.float32) * np.float32(32.0)).astype(np.int64)
        out.append(np.clip(s >> 5, -32768, 32767))
    return out[0], out[1]


def grid(width: int, height: int, cell_shift: int):
    return ((width - 1) >> cell_shift) + 1, ((height - 1) >> cell_shift) + 1


def from_records(ix, iy, a, index16, D: int, size, cell_shift=2, tolerance=2, dilate=0, near_is_high=1) -> dict:
    """The definition on the records at the pixels' own hypotheses: ix, iy, a [n, ph, pw] are rec(k, z(p), p) (anything where
    p is not tested), index16 [ph, pw] int16, size = (width, height) of the source images."""
    assert 0 <= cell_shift <= 8 and 0 <= tolerance <= 255 and 0 <= dilate <= 2 and near_is_high in (0, 1)
    ix, iy, a = np.asarray(ix).astype(np.int64), np.asarray(iy).astype(np.int64), np.asarray(a).astype(np.int64)
    idx = np.asarray(index16).astype(np.int64)
    n = a.shape[0]
    w, h = int(size[0]), int(size[1])
    cw, ch = grid(w, h, cell_shift)
    tested = idx >= 0
    z = np.minimum(D - 1, (idx + 8) >> 4)
    q1 = np.where(near_is_high, z, D - 1 - z) + 1                       # rank + 1
    seen = tested[None] & (a > 0)
    cell = (np.clip(iy, 0, h - 1) >> cell_shift) * cw + (np.clip(ix, 0, w - 1) >> cell_shift)
    cell = np.where(seen, cell, -1)
    zbuf = np.zeros((n, ch * cw), dtype=np.int64)
    for k in range(n):
        np.maximum.at(zbuf[k], cell[k][seen[k]], q1[seen[k]])
    zbuf = zbuf.reshape(n, ch, cw)
    # the maximum over the window's cells inside the grid: cells outside count as empty, and an empty cell is 0
    pad = np.zeros((n, ch + 2 * dilate, cw + 2 * dilate), dtype=np.int64)
    pad[:, dilate:dilate + ch, dilate:dilate + cw] = zbuf
    wide = np.zeros_like(zbuf)
    for dy in range(2 * dilate + 1):
        for dx in range(2 * dilate + 1):
            wide = np.maximum(wide, pad[:, dy:dy + ch, dx:dx + cw])
    m = np.stack([wide[k].ravel()[np.maximum(cell[k], 0)] for k in range(n)])
    visible = seen & (m <= q1[None] + tolerance)
    n_seen, n_vis = seen.sum(axis=0), visible.sum(axis=0)
    state = np.where(~tested, 0, np.where(n_seen == 0, 1, np.where(n_vis == n_seen, 2, np.where(n_vis == 0, 4, 3))))
    use = np.where(state[None] == 0, True, np.where(state[None] == 3, visible, seen))
    return dict(hypothesis=np.where(tested, z, 0).astype(np.uint8), depth_buffer=zbuf.astype(np.uint16), cell=cell.astype(np.int32),
                visible=visible.astype(np.uint8), use=use.astype(np.uint8), state=state.astype(np.uint8))


def visibility(weights, mapx, mapy, index16, size, **params) -> dict:
    """Everything tscm_sweep_visibility / _stages give: mapx, mapy [n, D, ph, pw] float32, weights None or n entries (None or
    [h, w] uint8), size = (width, height)."""
    n, D = mapx.shape[:2]
    z = CR.hypothesis(index16, D, 0)                                    # the fallback does not matter: those pixels are not tested
    gx, gy = CR.gather(mapx, z), CR.gather(mapy, z)
    ix, iy = record_positions(gx, gy)
    a = np.stack([pano_ref.alpha(None if weights is None else weights[k], int(size[0]), int(size[1]), gx[k], gy[k]) for k in range(n)])
    return from_records(ix, iy, a, index16, D, size, **{**DEFAULTS, **params})


def compose_masked(images, weights, mapx, mapy, use, mode=MULTIBAND, levels=4, wrap=True, gains=None) -> dict:
    """pano_ref.compose with a_k replaced by use_k ? a_k : 0 ahead of label, coverage and the blends; mapx, mapy [n, ph, pw]"""
    n = len(images)
    h, w = images[0].shape[:2]
    raw = np.stack([pano_ref.sample(images[k], mapx[k], mapy[k]) for k in range(n)])
    a = np.stack([pano_ref.alpha(None if weights is None else weights[k], w, h, mapx[k], mapy[k]) for k in range(n)])
    a = np.where(np.asarray(use) != 0, a, 0).astype(a.dtype)
    g = [256] * n if gains is None else list(gains)
    v = np.stack([pano_ref.apply_gain(raw[k], g[k]) for k in range(n)])
    lab, cov = pano_ref.label_coverage(a)
    res = dict(sampled=v.astype(np.uint8), alpha=a, label=lab, coverage=cov)
    if mode == SEAM:
        res["out"] = pano_ref.seam(v, lab)
    elif mode == FEATHER:
        res["out"] = pano_ref.feather(v, a)
    else:
        res.update(pano_ref.multiband(v, lab, cov, levels, wrap))
    return res


def compose(images, weights, mapx, mapy, index16, visibility_params=None, mode=MULTIBAND, levels=4, wrap=True, gains=None, fallback_index=0) -> dict:
    """Everything tscm_sweep_compose_visible / _stages give for one frame; images: n arrays [h, w] or [h, w, 3]."""
    h, w = images[0].shape[:2]
    vis = visibility(weights, mapx, mapy, index16, (w, h), **(visibility_params or {}))
    z = CR.hypothesis(index16, mapx.shape[1], fallback_index)
    res = compose_masked(images, weights, CR.gather(mapx, z), CR.gather(mapy, z), vis["use"], mode=mode, levels=levels, wrap=wrap, gains=gains)
    res["hypothesis"] = z
    res["use"], res["state"] = vis["use"], vis["state"]
    return res
