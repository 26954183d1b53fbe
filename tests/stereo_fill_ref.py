"""Host restatement of the hole filling defined in include/tscm/tscm.h (tscm_stereo_fill*): per pixel and path direction
the nearest valid value and its distance, then for the invalid pixels the lowest, second-lowest or median candidate.
Integers throughout and every candidate comes from the input map, so the device result is compared with array_equal.

The candidates are written twice.  candidates_walk() is the definition taken literally, a Python loop per pixel, direction
and step, for small maps.  candidates_scan() is vectorised and shaped differently: a diagonal becomes a column by shearing
the rows, a row becomes a non-cyclic line by laying it out twice, the nearest valid position behind each element is a
running maximum of positions, and what a walk without wrap_x must not see is thrown out afterwards by its distance."""
import numpy as np

DEFAULTS = dict(min_disparity=0, rule=2, paths=8, max_distance=0, min_directions=1, wrap_x=0)
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))      # (dx, dy), the matcher's order
LOWEST, SECOND_LOWEST, MEDIAN = 0, 1, 2
RULES = dict(lowest=LOWEST, second_lowest=SECOND_LOWEST, median=MEDIAN)


def invalid_value(min_disparity: int) -> int:
    return 16 * (min_disparity - 1)


def candidates_walk(d, min_disparity: int = 0, paths: int = 8, max_distance: int = 0, wrap_x: int = 0):
    """-> (value int16 [paths, h, w], distance int16 [paths, h, w]); invalid and 0 without a candidate."""
    d = np.asarray(d)
    h, w = d.shape
    invalid = invalid_value(min_disparity)
    v = [[int(d[y, x]) for x in range(w)] for y in range(h)]
    value = np.full((paths, h, w), invalid, dtype=np.int16)
    distance = np.zeros((paths, h, w), dtype=np.int16)
    for r, (dx, dy) in enumerate(DIRECTIONS[:paths]):
        for y in range(h):
            for x in range(w):
                t = 0
                while True:
                    t += 1
                    yy, xx = y + t * dy, x + t * dx
                    if yy < 0 or yy >= h:
                        break
                    if max_distance > 0 and t > max_distance:
                        break
                    if wrap_x:
                        if dy == 0 and t > w - 1:
                            break
                        xx %= w
                    elif xx < 0 or xx >= w:
                        break
                    if v[yy][xx] != invalid:
                        value[r, y, x], distance[r, y, x] = v[yy][xx], t
                        break
    return value, distance


def _nearest_above(ok: np.ndarray):
    """ok bool [n, m] -> for each element the largest row index i' < i with ok[i', j], -1 if none."""
    n, m = ok.shape
    pos = np.where(ok, np.arange(n)[:, None], -1)
    incl = np.maximum.accumulate(pos, axis=0) if n else pos
    return np.concatenate([np.full((1, m), -1, dtype=incl.dtype), incl[:-1]], axis=0) if n else incl


def candidates_scan(d, min_disparity: int = 0, paths: int = 8, max_distance: int = 0, wrap_x: int = 0):
    """The same two arrays, vectorised."""
    d = np.asarray(d)
    h, w = d.shape
    invalid = invalid_value(min_disparity)
    v = d.astype(np.int32)
    value = np.full((paths, h, w), invalid, dtype=np.int16)
    distance = np.zeros((paths, h, w), dtype=np.int16)
    if h == 0 or w == 0:
        return value, distance
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    for r, (dx, dy) in enumerate(DIRECTIONS[:paths]):
        if dy == 0:
            # the row twice, as columns of a [2w, h] array ordered so that the walk goes to smaller indices
            line = v.T if dx < 0 else v.T[::-1]
            two = np.concatenate([line, line], axis=0)
            src = _nearest_above(two != invalid)[w:]                          # for the second copy: positions w .. 2w - 1
            t = np.arange(w, 2 * w)[:, None] - src
            ok = (src >= 0) & (t <= w - 1)
            val = np.take_along_axis(two, np.maximum(src, 0), axis=0)
            if dx > 0:
                t, ok, val = t[::-1], ok[::-1], val[::-1]
            t, ok, val = t.T, ok.T, val.T
        else:
            cols = (xs + dx * dy * ys) % w                                    # sheared[y, c] = v[y, cols[y, c]]: the walk stays in column c
            sheared = v[ys, cols]
            if dy > 0:
                sheared = sheared[::-1]
            src = _nearest_above(sheared != invalid)
            t = np.arange(h)[:, None] - src
            ok = src >= 0
            val = np.take_along_axis(sheared, np.maximum(src, 0), axis=0)
            if dy > 0:
                t, ok, val = t[::-1], ok[::-1], val[::-1]
            back = (xs - dx * dy * ys) % w                                    # the column of pixel (x, y) in the sheared array
            t, ok, val = t[ys, back], ok[ys, back], val[ys, back]
        if not wrap_x:
            end = xs + t * dx
            ok = ok & (end >= 0) & (end < w)
        if max_distance > 0:
            ok = ok & (t <= max_distance)
        value[r] = np.where(ok, val, invalid)
        distance[r] = np.where(ok, t, 0)
    return value, distance


def select(d, value, distance, min_disparity: int = 0, rule: int = MEDIAN, min_directions: int = 1):
    """-> (out int16 [h, w], mask uint8 [h, w]) from the candidates."""
    d = np.asarray(d)
    invalid = invalid_value(min_disparity)
    above = 1 << 16                                                           # sorts behind every int16
    have = distance > 0
    key = np.sort(np.where(have, value.astype(np.int32), above), axis=0)
    n = have.sum(axis=0)
    n1 = np.maximum(n, 1)
    pick = {LOWEST: np.zeros_like(n1), SECOND_LOWEST: np.minimum(1, n1 - 1), MEDIAN: (n1 - 1) >> 1}[rule]
    chosen = np.take_along_axis(key, pick[None], axis=0)[0] if key.shape[0] else np.zeros(d.shape, np.int32)
    hole = d.astype(np.int32) != invalid
    hole = ~hole
    filled = hole & (n >= min_directions)
    out = np.where(filled, chosen, d).astype(np.int16)
    mask = np.where(hole, np.where(filled, 1, 2), 0).astype(np.uint8)
    return out, mask


def stages(d, walk: bool = False, **params) -> dict:
    p = dict(DEFAULTS, **params)
    if isinstance(p["rule"], str):
        p["rule"] = RULES[p["rule"]]
    d = np.asarray(d)
    cand = candidates_walk if walk else candidates_scan
    value, distance = cand(d, p["min_disparity"], p["paths"], p["max_distance"], p["wrap_x"])
    out, mask = select(d, value, distance, p["min_disparity"], p["rule"], p["min_directions"])
    return dict(value=value, distance=distance, out=out, mask=mask, params=p)


def fill(d, **params):
    """-> (out, mask)"""
    s = stages(d, **params)
    return s["out"], s["mask"]
