"""Host restatement of the disparity post-filter defined in include/tscm/tscm.h (tscm_stereo_filter*): 4-connected
components of the "both valid and within 16 * speckle_range" graph, label = the component's smallest linear index,
size = its pixel count, the speckle rule and the masked median.  Integers throughout, and none of it depends on an order
of traversal, so the device result is compared with array_equal.

components() is array union-find (roots hooked under smaller roots, pointer jumping), fast enough for whole maps;
components_bfs() is a flood fill from each unvisited pixel in raster order, written independently, for small maps."""
from collections import deque

import numpy as np

DEFAULTS = dict(min_disparity=0, speckle_window_size=100, speckle_range=2, median=0)


def invalid_value(min_disparity: int) -> int:
    return 16 * (min_disparity - 1)


def _edges(d: np.ndarray, invalid: int, speckle_range: int):
    """Linear indices (a, b), a < b, of the joined 4-neighbour pairs."""
    h, w = d.shape
    v = d.astype(np.int32)                                           # the difference is taken in 32 bits
    ok = v != invalid
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    thr = 16 * speckle_range
    horiz = ok[:, :-1] & ok[:, 1:] & (np.abs(v[:, :-1] - v[:, 1:]) <= thr)
    vert = ok[:-1] & ok[1:] & (np.abs(v[:-1] - v[1:]) <= thr)
    a = np.concatenate([idx[:, :-1][horiz], idx[:-1][vert]])
    b = np.concatenate([idx[:, 1:][horiz], idx[1:][vert]])
    return a, b


def components(d, min_disparity: int = 0, speckle_range: int = 2):
    """-> (label int32 [h, w], size int32 [h, w]) by array union-find."""
    d = np.asarray(d)
    h, w = d.shape
    invalid = invalid_value(min_disparity)
    a, b = _edges(d, invalid, speckle_range)
    parent = np.arange(h * w, dtype=np.int64)
    while a.size:
        ra, rb = parent[a], parent[b]                                # parent is fully compressed here: these are roots
        open_ = ra != rb
        if not open_.any():
            break
        a, b, ra, rb = a[open_], b[open_], ra[open_], rb[open_]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))   # hook the larger root under the smaller
        while True:                                                  # pointer jumping
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    valid = (d.astype(np.int32) != invalid).ravel()
    label = np.where(valid, parent, -1)
    count = np.bincount(parent[valid], minlength=h * w) if h * w else np.zeros(0, dtype=np.int64)
    size = np.where(valid, count[parent], 0)
    return label.reshape(h, w).astype(np.int32), size.reshape(h, w).astype(np.int32)


def components_bfs(d, min_disparity: int = 0, speckle_range: int = 2):
    """The same two arrays by a flood fill from each unvisited valid pixel in raster order (its seed is then the
    component's smallest index).  A per-pixel Python loop: for small maps."""
    d = np.asarray(d)
    h, w = d.shape
    invalid = invalid_value(min_disparity)
    v = [[int(d[y, x]) for x in range(w)] for y in range(h)]
    label = [[-1] * w for _ in range(h)]
    size = [[0] * w for _ in range(h)]
    for sy in range(h):
        for sx in range(w):
            if v[sy][sx] == invalid or label[sy][sx] >= 0:
                continue
            seed = sy * w + sx
            label[sy][sx] = seed
            queue, members = deque([(sy, sx)]), []
            while queue:
                y, x = queue.popleft()
                members.append((y, x))
                for ny, nx in ((y, x + 1), (y + 1, x), (y, x - 1), (y - 1, x)):
                    if 0 <= ny < h and 0 <= nx < w and label[ny][nx] < 0 and v[ny][nx] != invalid \
                            and abs(v[y][x] - v[ny][nx]) <= 16 * speckle_range:      # against the current pixel, not the seed
                        label[ny][nx] = seed
                        queue.append((ny, nx))
            for y, x in members:
                size[y][x] = len(members)
    return np.array(label, dtype=np.int32).reshape(h, w), np.array(size, dtype=np.int32).reshape(h, w)


def despeckle(d, size, min_disparity: int = 0, speckle_window_size: int = 100) -> np.ndarray:
    d = np.asarray(d)
    if speckle_window_size <= 0:
        return d.copy()
    return np.where(size <= speckle_window_size, invalid_value(min_disparity), d).astype(np.int16)


def masked_median(d, min_disparity: int = 0, median: int = 3) -> np.ndarray:
    d = np.asarray(d)
    if median == 0:
        return d.copy()
    h, w = d.shape
    invalid, r = invalid_value(min_disparity), median // 2
    above = 1 << 16                                                  # sorts behind every int16
    key = np.where(d.astype(np.int32) != invalid, d.astype(np.int32), above)
    pad = np.full((h + 2 * r, w + 2 * r), above, dtype=np.int32)     # outside the image: not part of the window
    pad[r:r + h, r:r + w] = key
    win = np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(median) for dx in range(median)], axis=-1)
    win.sort(axis=-1)
    n = (win != above).sum(axis=-1)
    pick = np.take_along_axis(win, (np.maximum(n, 1) - 1 >> 1)[..., None], axis=-1)[..., 0]
    return np.where(key != above, pick, invalid).astype(np.int16)


def stages(d, **params) -> dict:
    p = dict(DEFAULTS, **params)
    d = np.asarray(d)
    if d.size == 0:
        z = np.zeros(d.shape, dtype=np.int32)
        return dict(label=z, size=z.copy(), despeckled=d.copy(), out=d.copy(), params=p)
    label, size = components(d, p["min_disparity"], p["speckle_range"])
    desp = despeckle(d, size, p["min_disparity"], p["speckle_window_size"])
    return dict(label=label, size=size, despeckled=desp, out=masked_median(desp, p["min_disparity"], p["median"]), params=p)


def filter(d, **params) -> np.ndarray:
    return stages(d, **params)["out"]
