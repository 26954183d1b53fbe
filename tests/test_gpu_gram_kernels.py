"""The normal equations of every Gram kernel against the oracle, entry by entry.

tscm_eval_normal_equations_ex runs the Gram kernel a solve with the same options runs: k_eval_gram4<KS, MULTI> (default),
k_eval_gram<58> / k_eval_gram<0> (TSCM_EXEC_GRAM_16X16) and k_eval_gram_f32<KS, MULTI> (jacobian_fp32).  The board shapes
below reach every (KS, MULTI) of the pass plan g4_plan, one to four passes per view; every problem mixes full views with
ragged ones (1..3 corners, around the pass boundary, n - 1, an empty view) and puts short views behind long ones inside
a wave's chunk of views.  Two problems of 280,000 views take every wave's chunk past its first block of 64 views.

Reference: the oracle's dual-number Jacobian with numpy products (tests/helpers.py: normal_equations_from).
  fp64 (gram4): every block within 1e-11 of its largest entry, the cost within 1e-12 (as test_normal_equations)
  16x16 tile:   the same bits as gram4 in every output
  fp32 tier:    every entry within TOL_F32 of its Cauchy-Schwarz bound (helpers.gram_errors), the cost (fp64 in
                this tier too) within 1e-12 of gram4's
tests/test_gram_tolerance.py shows, without a GPU, that these tolerances see a dropped, doubled or stale row.
"""
import functools
import time

import numpy as np
import pytest

from oracle import pyoracle as orc
from tscm_calib_amd import api, lib, synth
from tscm_calib_amd.problem import shard_frames
from tests import helpers as H
from tests import native_check as N

# fp32 tier: largest entrywise error in units of sqrt(G_ii G_jj) (sqrt(G_ii r^T r) for gradients).  fp32 rounding of the
# derivatives and <= 56 rows of fp32 accumulation per pass: measured <= 3.3e-6 on an MI355X, every board shape, views and
# boards of 4 corners or more.  The products of a view or board of one to three corners (*_short) are one or a few row
# pairs with nothing to average over: where the fp32 derivative formula cancels at that corner (a small entry of a large
# sum) its own relative error shows undiluted -- measured up to 3e-5 on 8,192 views, 5e-5 on 280,000, and only in views
# of 1..3 corners (not at pass boundaries, not in the second block of 64 views).
# test_gram_tolerance.py holds the signal of one wrong row at >= 20 x these (measured: >= 9e-3)
TAU_F32, TAU_F32_SHORT = 1e-5, 1e-4
TOL_F32 = dict(board_gram=TAU_F32, board_grad=TAU_F32, view_cross=TAU_F32, cam_gram=TAU_F32, cam_grad=TAU_F32,
               board_gram_short=TAU_F32_SHORT, board_grad_short=TAU_F32_SHORT, view_cross_short=TAU_F32_SHORT)


def f32_excess(e: dict) -> float:
    """Largest normalised error of helpers.gram_errors in units of its tolerance (<= 1: within TOL_F32)."""
    return max(v / TOL_F32[k] for k, v in e.items())


@functools.lru_cache(maxsize=None)
def _g4():
    """kG4MaxKS and g4_plan(n) of tscm_exec_plan.h for every board the library takes (up to about 2,000 corners), as one
    run of tests/native/exec_plan_check.cpp prints them."""
    r = N.run(N.built("exec_plan_check.cpp", "exec_plan_check"), "g4", *range(1, 2049))
    return r["max_ks"], {int(n): tuple(plan) for n, plan in r["plans"].items()}


def g4_plan(n):
    """(passes, per, ks): ceil(n / 56) passes of `per` = 4 KS corners, the last pass takes what is left."""
    return _g4()[1][n]


SINGLE = [(2, 2), (3, 2), (3, 3), (4, 4), (5, 4), (6, 4), (7, 4), (6, 5), (7, 5), (8, 5), (7, 6), (8, 6), (7, 7), (9, 6)]
MULTI = [(19, 3), (10, 7), (11, 7), (11, 8), (12, 8), (13, 8), (12, 9), (14, 10), (17, 12)]
SHAPES = [(c, r, False) for c, r in SINGLE + MULTI] + [(11, 8, True)]        # (cols, rows, mono)


def test_shapes_reach_every_instantiation_of_the_pass_plan():
    """Every k_eval_gram4 / k_eval_gram_f32 instantiation (KS = 1..14 single-pass, 8..14 multi-pass) is run by the
    parametrisations below, and three- and four-pass views are among them."""
    plans = {(c, r): g4_plan(c * r) for c, r, _ in SHAPES}
    MAX_KS = _g4()[0]
    assert MAX_KS == 14
    reached = {(ks, passes > 1) for passes, _, ks in plans.values()}
    assert reached == {(k, False) for k in range(1, MAX_KS + 1)} | {(k, True) for k in range(8, MAX_KS + 1)}
    assert {passes for passes, _, _ in plans.values()} == {1, 2, 3, 4}
    assert g4_plan(57) == (2, 32, 8) and g4_plan(88) == (2, 44, 11) and g4_plan(204) == (4, 52, 13)
    assert any(mono and g4_plan(c * r)[0] > 1 for c, r, mono in SHAPES)


def ragged(p, n, per):
    """Corner counts by board: frame f has pattern[(f // C) % len] corners in each of its views (a prefix of the corner
    list).  A camera's views run over frames of one residue class mod C in device order, so consecutive views of a
    chunk step through the pattern: short views behind long ones, pass boundaries, n - 1, an empty view."""
    pattern = [n, 1, n, 2, n, 3, n, per - 1, n, per, per + 1, n - 1, 0, n, per + 1, 1, n - 1, 2, per, 3]
    q = p.copy()
    k = (q.view_board // max(1, q.n_cameras)) % len(pattern)
    q.view_count = np.clip(np.asarray(pattern)[k], 0, n).astype(np.int32)
    return q.normalised()


def reference(p, world=1):
    """Normal equations from the oracle's Jacobian; large problems in frame slices (42 doubles of Jacobian per corner)."""
    if world == 1:
        cost, res, Jc, Jb, Ji = orc.evaluate(p, jets=True)
        return H.normal_equations_from(p, res, Jc, Jb, Ji)
    out, rr = None, 0.0
    for r in range(world):
        q = shard_frames(p, r, world)
        sel = np.isin(p.view_board, q.meta["owned_boards"])
        cost, res, Jc, Jb, Ji = orc.evaluate(q, jets=True)
        o = H.normal_equations_from(q, res, Jc, Jb, Ji)
        del res, Jc, Jb, Ji
        if out is None:
            out = {k: np.zeros((p.n_views,) + v.shape[1:]) if k in ("view_cross", "view_ediag", "view_fdiag") else np.zeros_like(v)
                   for k, v in o.items() if k != "cost"}
        for k, v in o.items():
            if k in ("view_cross", "view_ediag", "view_fdiag"):
                out[k][sel] = v
            elif k != "cost":
                out[k] += v
        rr += 2.0 * o["cost"]
    out["cost"] = 0.5 * rr
    return out


def check_all_kernels(p, o, tag):
    """The three Gram kernels on problem p against the reference o; returns the fp32 tier's normalised errors."""
    mono = bool(p.mono)
    g = api.normal_equations(p)
    g16 = api.normal_equations(p, exec_flags=lib.EXEC_GRAM_16X16)
    g32 = api.normal_equations(p, jacobian_fp32=1)
    # fp64, k_eval_gram4: the bounds of test_normal_equations
    assert abs(g["cost"] - o["cost"]) <= 1e-12 * o["cost"], tag
    e64 = H.block_errors(g, o, mono)
    assert max(e64.values()) <= 1e-11, (tag, e64)
    # the 16x16 tile contracts the same groups of four rows in the same order: the same bits
    for key in ("board_gram", "board_grad", "view_cross", "cam_gram", "cam_grad", "cost"):
        assert np.array_equal(g16[key], g[key]), (tag, key)
    # fp32-Jacobian tier
    assert abs(g32["cost"] - g["cost"]) <= 1e-12 * g["cost"], tag
    e32 = H.gram_errors(g32, o, p)
    print(f"\n[gram] {tag}: fp64 max error {max(e64.values()):.2e}; fp32 max normalised error "
          f"{', '.join(f'{k} {v:.2e}' for k, v in e32.items())}; {1.0 / max(f32_excess(e32), 1e-300):.1f} x below TOL_F32")
    assert f32_excess(e32) <= 1.0, (tag, e32)
    return e32


@pytest.fixture(scope="module")
def n_cus(hip_device):
    """Compute units of the device, from the HIP runtime the library runs on (hipDeviceAttributeMultiprocessorCount = 63
    in the HIP 6 / 7 ABI)."""
    import ctypes as C
    hip, n = C.CDLL("libamdhip64.so"), C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(n), 63, hip_device) == 0
    assert 1 <= n.value <= 1024, n.value
    return n.value


@pytest.mark.gpu
@pytest.mark.parametrize("cols,rows,mono", SHAPES, ids=[f"{c}x{r}{'-mono' if m else ''}" for c, r, m in SHAPES])
def test_gram_kernels_against_the_oracle(hip_device, n_cus, cols, rows, mono):
    """Every (KS, MULTI) instantiation of k_eval_gram4 and k_eval_gram_f32, and k_eval_gram, on full and ragged views.
    2 x 16 views per CU: at least 16 x CUs chunks would be needed to give every view a chunk of its own, so chunks hold
    two views or more and a chunk's short view follows a long one (the zeroing of the rows the last pass left)."""
    n = cols * rows
    passes, per, ks = g4_plan(n)
    n_views = 32 * n_cus
    C = 1 if mono else 4
    p = synth.make_problem(C, n_views // C, 900 + n + mono, cols=cols, rows=rows, pitch=360.0 / max(cols, rows))
    p = ragged(p, n, per)
    assert p.n_views >= 32 * n_cus and (p.view_count == 0).any() and (p.view_count < 4).any()
    check_all_kernels(p, reference(p), f"{cols}x{rows}{' mono' if mono else ''} (KS {ks}, {passes} pass{'es' if passes > 1 else ''})")


@pytest.mark.gpu
@pytest.mark.parametrize("cols,rows", [(2, 2), (19, 3)])
def test_gram_kernels_on_chunks_of_more_than_64_views(hip_device, n_cus, cols, rows):
    """4 cameras x 70,000 views: more than 64 x 16 views per CU, so every wave's chunk holds more than 64 views however
    many workgroups a CU keeps resident (the host plans at most 16 waves per CU), and its later blocks of 64 views reload
    their corner counts, record slots and first observations.  Ragged views sit next to every block boundary."""
    n = cols * rows
    passes, per, ks = g4_plan(n)
    t0 = time.time()
    p = ragged(synth.make_problem(4, 70_000, 77 + n, cols=cols, rows=rows, pitch=360.0 / max(cols, rows)), n, per)
    assert p.n_views > 64 * 16 * n_cus, (p.n_views, n_cus)
    o = reference(p, world=max(1, p.n_corners // 1_000_000))
    t1 = time.time()
    check_all_kernels(p, o, f"{cols}x{rows} x {p.n_views} views ({p.n_corners} corners)")
    print(f"[gram] {cols}x{rows} large: problem + oracle {t1 - t0:.1f} s, three kernels + checks {time.time() - t1:.1f} s")
