"""Negative control of the Gram kernels' tolerances (CPU: oracle and numpy only).

tests/test_gpu_gram_kernels.py holds the fp64 kernels to 1e-11 of each block's largest entry and the fp32-Jacobian tier
to TOL_F32 of each entry's Cauchy-Schwarz bound.  Here the reference is formed a second time with the mistakes a Gram
kernel could plausibly make at a pass or view boundary, and both comparisons must see every one of them: the fp32 one
by at least 20 x its tolerance, so that the tier's rounding can never hide one wrong row.
"""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import synth
from tests import helpers as H
from tests.test_gpu_gram_kernels import f32_excess, g4_plan, ragged

MARGIN = 20.0


def _passes(cnt, per):
    """(first row, rows) of every pass of a view of cnt corners."""
    return [(c0, min(per, cnt - c0)) for c0 in range(0, cnt, per)]


def dropped_last_row_of_each_pass(p, per):
    start = np.cumsum(p.view_count) - p.view_count
    ex = [(v, start[v] + c0 + nv - 1, -1.0) for v in range(p.n_views) for c0, nv in _passes(int(p.view_count[v]), per)]
    return tuple(np.array(a) for a in zip(*ex))


def doubled_first_row_of_second_pass(p, per):
    start = np.cumsum(p.view_count) - p.view_count
    ex = [(v, start[v] + per, 1.0) for v in range(p.n_views) if p.view_count[v] > per]
    return tuple(np.array(a) for a in zip(*ex))


def stale_row_of_previous_view(p, per):
    """A view whose first pass has fewer rows than the last pass of the view before it also contracts the first row
    the earlier view left behind (lane nv of the tile: the rows it did not overwrite are not zeroed)."""
    start = np.cumsum(p.view_count) - p.view_count
    ex, prev = [], None
    for v in range(p.n_views):
        cnt = int(p.view_count[v])
        if cnt == 0:
            continue
        if prev is not None:
            c0, last = _passes(int(p.view_count[prev]), per)[-1]
            nv = min(per, cnt)
            if nv < last:
                ex.append((v, start[prev] + c0 + nv, 1.0))
        prev = v
    return tuple(np.array(a) for a in zip(*ex))


MISTAKES = {"drop": dropped_last_row_of_each_pass, "double": doubled_first_row_of_second_pass, "stale": stale_row_of_previous_view}


@pytest.mark.parametrize("cols,rows,mono", [(9, 6, False), (19, 3, False), (11, 8, False), (14, 10, False), (17, 12, False), (11, 8, True), (2, 2, False)])
def test_tolerances_see_a_wrong_row(cols, rows, mono):
    n = cols * rows
    passes, per, ks = g4_plan(n)
    C = 1 if mono else 4
    p = ragged(synth.make_problem(C, 80 if mono else 40, 900 + n + mono, cols=cols, rows=rows, pitch=360.0 / max(cols, rows)), n, per)
    cost, res, Jc, Jb, Ji = orc.evaluate(p, jets=True)
    o = H.normal_equations_from(p, res, Jc, Jb, Ji)
    # the reference against itself: no error (the measures are sound where nothing is wrong)
    assert max(H.gram_errors(o, o, p).values()) == 0.0 and max(H.block_errors(o, o, mono).values()) == 0.0
    ran = []
    for name, mistake in MISTAKES.items():
        extra = mistake(p, per)
        if not len(extra) or not len(extra[0]):
            assert name == "double" and passes == 1           # single-pass boards have no second pass
            continue
        # the faintest form: the mistake in long views only (n - 1 or n corners; a stale row in views of 3 or more), where
        # one row is the smallest share of the view's products (views of one or two corners move by O(1))
        long = p.view_count[extra[0]] >= (min(3, n - 1) if name == "stale" else n - 1)
        extra = tuple(a[long] for a in extra)
        assert len(extra[0]), name
        bad = H.normal_equations_from(p, res, Jc, Jb, Ji, extra=extra)
        e32, e64 = H.gram_errors(bad, o, p), H.block_errors(bad, o, mono)
        assert f32_excess(e32) >= MARGIN, (name, e32)
        assert max(e64.values()) > 1e-11, (name, e64)
        # ... and seen in the per-view blocks, which locate the view
        assert f32_excess({k: e32[k] for k in ("view_cross", "view_cross_short")}) >= MARGIN, (name, e32)
        ran.append(name)
    assert ran == (["drop", "double", "stale"] if passes > 1 else ["drop", "stale"])
