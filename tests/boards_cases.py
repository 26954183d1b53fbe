"""Candidate sets for the tests of the batched chessboard structure recovery (tscm_chessboards_from_corners_batch): the random
generator of tests/test_boards.py (copied, so that no test file is imported), its clutter-heavy variant, the edge inputs, and
what the stage properties need in numpy -- the energy of a board from its cells and the cols >= rows turn.  No GPU."""
import functools

import numpy as np

SEEDS = list(range(60)) + list(range(100, 130))          # the seeds tests/test_boards.py uses
HEAVY_SEEDS = list(range(200, 230))                      # 30 sets with 60-120 clutter points


def random_candidates(seed, clutter=(0, 15)):
    """A jittered, rotated, mildly warped grid of 3-11 x 3-8 integer points plus clutter, shuffled: x, y, v1, v2, (gh, gw).
    clutter = (low, high): the number of clutter points is drawn from [low, high)."""
    rng = np.random.default_rng(seed)
    gw, gh = int(rng.integers(3, 12)), int(rng.integers(3, 9))
    ang, step = rng.uniform(0, 2 * np.pi), rng.uniform(18, 60)
    c, r = np.meshgrid(np.arange(gw), np.arange(gh))
    gx, gy = step * (c * np.cos(ang) - r * np.sin(ang)), step * (c * np.sin(ang) + r * np.cos(ang))
    k = rng.uniform(0, 4e-4)                                           # mild barrel-like warp
    rr = gx * gx + gy * gy
    gx, gy = gx * (1 - k * np.sqrt(rr)), gy * (1 - k * np.sqrt(rr))
    pts = np.stack([gx.ravel() + 400, gy.ravel() + 400], axis=1) + rng.uniform(-0.8, 0.8, size=(gw * gh, 2))
    pts = np.rint(pts)                                                 # the candidates are integer maxima
    v1 = np.tile([np.cos(ang), np.sin(ang)], (gw * gh, 1))
    v2 = np.tile([-np.sin(ang), np.cos(ang)], (gw * gh, 1))
    nc = int(rng.integers(*clutter))
    cl = np.rint(rng.uniform(0, 900, size=(nc, 2)))
    a = rng.uniform(0, 2 * np.pi, size=nc)
    pts, v1, v2 = np.concatenate([pts, cl]), np.concatenate([v1, np.stack([np.cos(a), np.sin(a)], 1)]), np.concatenate([v2, np.stack([-np.sin(a), np.cos(a)], 1)])
    perm = rng.permutation(pts.shape[0])
    return pts[perm, 0].copy(), pts[perm, 1].copy(), v1[perm].copy(), v2[perm].copy(), (gh, gw)


def heavy_candidates(seed):
    return random_candidates(seed, clutter=(60, 121))


def grid(gw, gh, step=40.0, x0=100.0, y0=120.0, clutter=0, seed=0, shuffle=True):
    """An exact axis-parallel gw x gh grid (row-major, candidate 0 = its first corner unless shuffled) plus clutter points."""
    rng = np.random.default_rng(seed)
    c, r = np.meshgrid(np.arange(gw), np.arange(gh))
    pts = np.stack([x0 + step * c.ravel(), y0 + step * r.ravel()], axis=1).astype(np.float64)
    pts = np.concatenate([pts, np.rint(rng.uniform(0, 900, size=(clutter, 2)))])
    n = pts.shape[0]
    v1, v2 = np.tile([1.0, 0.0], (n, 1)), np.tile([0.0, 1.0], (n, 1))
    perm = rng.permutation(n) if shuffle else np.arange(n)
    return pts[perm, 0].copy(), pts[perm, 1].copy(), v1[perm].copy(), v2[perm].copy()


def _sized(n, seed):
    """Exactly n candidates: a 9 x 6 grid and n - 54 clutter points (n >= 54), or the first n points of a 4 x 3 grid."""
    if n >= 54:
        return grid(9, 6, clutter=n - 54, seed=seed)
    x, y, v1, v2 = grid(4, 3, shuffle=False)
    return x[:n].copy(), y[:n].copy(), v1[:n].copy(), v2[:n].copy()


@functools.lru_cache(maxsize=None)
def edge_sets():
    """name -> (x, y, v1, v2): the edge inputs of the issue, each one image.  Never written to."""
    out = {}
    e = np.zeros(0)
    out["n0"] = (e, e, np.zeros((0, 2)), np.zeros((0, 2)))
    out["n8"] = _sized(8, 0)
    x = np.full(9, 7.0)
    out["n9_one_point"] = (x, x.copy(), np.tile([1.0, 0.0], (9, 1)), np.tile([0.0, 1.0], (9, 1)))
    out["n12"] = _sized(12, 0)
    out["n70"] = _sized(70, 3)
    # duplicated candidates inside a grid: two grid points come twice
    x, y, v1, v2 = grid(7, 5, clutter=4, seed=5)
    rng = np.random.default_rng(11)
    dup = rng.choice(35, size=2, replace=False)
    inside = np.flatnonzero((x >= 100) & (x <= 100 + 6 * 40) & (y >= 120) & (y <= 120 + 4 * 40))[dup]
    out["duplicates"] = (np.concatenate([x, x[inside]]), np.concatenate([y, y[inside]]), np.concatenate([v1, v1[inside]]), np.concatenate([v2, v2[inside]]))
    # a grid that contains candidate 0 (the empty marker): unshuffled, candidate 0 is its first corner
    out["grid_with_candidate_0"] = grid(6, 5, clutter=3, seed=7, shuffle=False)
    # rows without directions
    x, y, v1, v2 = grid(8, 5, clutter=6, seed=9)
    v1, v2 = v1.copy(), v2.copy()
    v1[::3] = 0.0
    v2[::3] = 0.0
    out["zero_directions"] = (x, y, v1, v2)
    return out


MIXED = ("n0", "n8", "n12", "n70")                       # one call whose images hold 0, 8, 12 and 70 candidates


def energy_of(x, y, cells):
    """The energy of a board (rows x cols matrix of candidate indices) as tscm_boards_core.h states it, in numpy fp64: every
    operation below is one IEEE operation, so the value is the library's bit for bit."""
    b = np.asarray(cells)
    R, Cn = b.shape
    with np.errstate(all="ignore"):
        def q(i0, i1, i2, column):
            ux, uy = x[i0] + x[i2] - 2 * x[i1], y[i0] + y[i2] - 2 * y[i1]
            wx, wy = x[i0] - x[i2], y[i0] - y[i2]
            if column:
                ux, uy, wx, wy = np.rint(ux), np.rint(uy), np.rint(wx), np.rint(wy)
            return (np.sqrt(ux * ux + uy * uy) / np.sqrt(wx * wx + wy * wy)).ravel()
        terms = np.concatenate([q(b[:, :-2], b[:, 1:-1], b[:, 2:], False), q(b[:-2], b[1:-1], b[2:], True)])
    worst = 0.0
    for t in terms:                                        # `worst < q` from 0: a NaN is never taken
        if worst < t:
            worst = float(t)
    return R * Cn * (worst - 1)


def turned(b):
    """cols >= rows: t[j, k] = b[rows - k - 1, j]."""
    return b if b.shape[1] >= b.shape[0] else b[::-1].T


def check_stages(x, y, st, boards, where=""):
    """The stage properties of one image: st = its dict of chessboards_batch_stages, boards = its final boards."""
    n = st["n"]
    assert n == len(x), where
    for k in ("status", "rows", "cols", "steps", "energy"):
        assert st[k].shape == (n,), (where, k)
    assert st["offset"].shape == (n + 1,) and st["offset"][0] == 0 and st["offset"][-1] == st["cells"].shape[0], where
    counts = [int(np.sum(st["status"] == s)) for s in range(4)]
    assert sum(counts) == n, (where, counts)                                       # the statuses partition the seeds
    assert np.array_equal(np.diff(st["offset"]), st["rows"] * st["cols"]), where
    blank = st["status"] == 0
    assert not st["rows"][blank].any() and not st["cols"][blank].any() and not st["energy"][blank].any(), where
    seed = st["status"] == 1
    assert np.all(st["rows"][seed] == 3) and np.all(st["cols"][seed] == 3) and np.all(st["steps"][seed] == 0) and np.all(st["energy"][seed] > 0), where
    grown = st["status"] >= 2
    assert np.array_equal(st["steps"][grown], st["rows"][grown] + st["cols"][grown] - 6), where
    assert not np.any(st["energy"][st["status"] == 2] < -10), where
    offered = []
    for i in np.flatnonzero(st["status"] == 3):
        cells = st["cells"][st["offset"][i]:st["offset"][i + 1]].reshape(st["rows"][i], st["cols"][i])
        assert cells.min() >= 0 and cells.max() < n, (where, i)
        assert st["energy"][i] < -10, (where, i)
        assert st["energy"][i] == energy_of(x, y, cells), (where, i, st["energy"][i], energy_of(x, y, cells))
        offered.append(turned(cells))
    for b in boards:                                                               # every final board is an offered record, turned
        assert any(b.shape == o.shape and np.array_equal(b, o) for o in offered), where
    return counts
