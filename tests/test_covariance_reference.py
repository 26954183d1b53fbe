"""The covariance reference (tests/cov_ref.py) itself, without a GPU: against a dense inverse of the full J^T J in 50
digits, the free-column rules against helpers.step_columns, the singular exits, and the negative control -- every
`mistake` of cov_ref is rejected by the tolerance rule of the GPU tests on at least one of their cases."""
import numpy as np
import pytest

from tests import cov_ref as CR
from tests import helpers as H
from tscm_calib_amd import lib, synth


def _small():
    """2 cameras, 3 boards, 12 corners per view; board 2 seen by one camera.  Large boards (pitch 300) at the ground truth:
    the best-conditioned of the 4 x 3 problems the generator makes (36 were compared by their e64)."""
    p = synth.make_problem(2, 3, 6, cols=4, rows=3, pitch=300.0, perturb=False)
    keep = np.ones(p.n_views, bool)
    keep[np.nonzero(p.view_board == 2)[0][1:]] = False
    q = CR.Problem(p.n_cameras, p.n_boards, p.board_xy, p.view_camera[keep], p.view_board[keep], p.view_offset[keep], p.view_count[keep],
                   p.obs_u, p.obs_v, p.cam_rt, p.intr, p.board_rt, p.cam_pose_constant, False, meta={})
    return q.normalised()


def _dense_inverse(p, fixed):
    """(J^T J)^-1 over the free columns by mpmath LU on the full matrix: cam_cov [C,15,C,15], board_cov [B,6,6]."""
    import mpmath as mp
    mp.mp.dps = 50
    cost, res, Jc, Jb, Ji = H.orc.evaluate(p, jets=True)
    cam_free, board_free = CR.free_columns(p, fixed)
    C, B = p.n_cameras, p.n_boards
    col_c = -np.ones((C, 15), int); col_c[cam_free] = np.arange(cam_free.sum())
    nc = int(cam_free.sum())
    col_b = -np.ones(B, int); col_b[board_free] = nc + 6 * np.arange(board_free.sum())
    n = nc + 6 * int(board_free.sum())
    rows = []
    k = 0
    for v in range(p.n_views):
        m, b = int(p.view_camera[v]), int(p.view_board[v])
        for j in range(int(p.view_count[v])):
            for e in range(2):
                row = [mp.mpf(0)] * n
                F = np.concatenate([Jc[k].reshape(2, 6)[e], Ji[k].reshape(2, 9)[e]])
                for a in range(15):
                    if col_c[m, a] >= 0:
                        row[col_c[m, a]] = mp.mpf(float(F[a]))
                if col_b[b] >= 0:
                    for a in range(6):
                        row[col_b[b] + a] = mp.mpf(float(Jb[k].reshape(2, 6)[e, a]))
                rows.append(row)
            k += 1
    J = mp.matrix(rows)
    inv = (J.T * J) ** -1
    full = np.array([[inv[i, j] for j in range(n)] for i in range(n)], dtype=object)
    cam = np.zeros((C * 15, C * 15), np.longdouble)
    idx = np.nonzero(cam_free.ravel())[0]
    cam[np.ix_(idx, idx)] = np.array([[np.longdouble(mp.nstr(full[i, j], 30)) for j in range(nc)] for i in range(nc)], np.longdouble)
    board = np.zeros((B, 6, 6), np.longdouble)
    for b in np.nonzero(board_free)[0]:
        o = col_b[b]
        board[b] = np.array([[np.longdouble(mp.nstr(full[o + i, o + j], 30)) for j in range(6)] for i in range(6)], np.longdouble)
    return dict(cam_cov=cam.reshape(C, 15, C, 15), board_cov=board, cam_free=cam_free, board_free=board_free)


@pytest.mark.parametrize("fixed", [None, ("xi", "lambda"), np.array([lib.MODEL_UCM, lib.FIX_INTRINSICS])], ids=["free", "ucm", "ucm_all7"])
def test_reference_against_dense_inverse_in_50_digits(fixed):
    """Agreement to 1e-15 in cov_errors' measure, of the reference with its exact-residual refinement
    (cov_ref.refine_full_inverse).  The plain longdouble run cannot reach that without held columns: the scaled reduced
    system of this problem has a smallest pivot of 1.0e-8 when xi, lambda and alpha are all free, and a Schur inverse in
    longdouble (u = 5.4e-20) is off by condition * u.  Its bound here is n_free * u / min_pivot_ratio (2.0e-10 free; measured
    1.7e-11 free, 4.3e-17 ucm, 1.8e-17 ucm_all7).  Refinement starts from that run -- all of the inverse in Schur form, the
    cross blocks included -- and needs a start that is only rounding away: its first residual |I - J^T J X| is asserted
    small (a structural mistake gives O(1) and is not improved).  Refined, the blocks equal the 50-digit inverse rounded to
    longdouble."""
    p = _small()
    assert p.n_cameras == 2 and p.n_boards == 3 and p.n_points == 12
    plain = CR.cov_ref(p, fixed=fixed)
    ref = CR.cov_ref(p, fixed=fixed, refine=True)
    dense = _dense_inverse(p, fixed)
    assert ref["status"] == 0 and ref["n_free"] == int(dense["cam_free"].sum()) + 18
    e0, e = CR.cov_errors(plain, dense), CR.cov_errors(ref, dense)
    u = float(np.finfo(np.longdouble).eps) / 2
    print(f"longdouble reference against 50 digits: plain {e0}, bound {ref['n_free'] * u / ref['min_pivot_ratio']:.2e}; first residual "
          f"{ref['first_residual']:.2e}, {ref['refine_steps']} steps, refined {e}")
    assert max(e0.values()) <= ref["n_free"] * u / ref["min_pivot_ratio"], e0
    assert ref["first_residual"] < 2.0 ** -10
    assert e["cam"] <= 1e-15 and e["board"] <= 1e-15, e
    # not-free rows, columns and blocks are exactly 0
    nf = ~dense["cam_free"].ravel()
    for r in (plain, ref):
        cc = np.asarray(r["cam_cov"]).reshape(30, 30)
        assert not cc[nf].any() and not cc[:, nf].any()


@pytest.mark.parametrize("mistake", ["marginal_term_dropped", "pair_tile_missing_board", "scale_not_undone"])
def test_refinement_does_not_repair_a_mistake(mistake):
    """A start with a structural mistake has |I - J^T J X| >= 1: refine_full_inverse leaves its blocks as they are, so the
    refined reference cannot hide a wrong Schur restatement."""
    p = _small()
    jets = H.orc.evaluate(p, jets=True)
    blk = CR.blocks_from_terms(p, H.step_terms(p, jets=jets))
    bad = CR.cov_from_blocks(p.view_camera, p.view_board, blk["board_gram"], blk["view_cross"], blk["cam_gram"], *CR.free_columns(p), mistake=mistake)
    assert bad["status"] == 0
    out = CR.refine_full_inverse(p, bad, jets)
    assert out["first_residual"] >= 1 and out["refine_steps"] == 1
    assert np.array_equal(out["cam_cov"], bad["cam_cov"]) and np.array_equal(out["board_cov"], bad["board_cov"])


def test_free_columns_are_the_oracles_without_masks():
    for make in (lambda: H.small_rig(4, 4), lambda: H.mixed_visibility_rig(n_frames=13), lambda: synth.make_problem(1, 5, 3),
                 lambda: H.rig_with_unseen_boards(H.small_rig(3, 4), 2), CR._camera_without_views, CR._const_boards):
        p = make()
        cam_free, board_free = CR.free_columns(p)
        cols = H.step_columns(p)
        assert np.array_equal(cam_free[:, :13], cols["cam_free"]) and not cam_free[:, 13:].any()
        assert np.array_equal(board_free, cols["board_free"])


def test_sigma2_dof_and_stds():
    p, kw, ref, e64, tol = CR.case("mixed65-cx_cy")
    assert ref["dof"] == 2 * p.n_corners - ref["n_free"] and ref["n_free"] == 6 * 3 + 5 * 4 + 6 * 65
    assert ref["sigma2"] == 2 * ref["cost"] / ref["dof"]
    assert not ref["intr_std"][:, 2:4].any() and not ref["intr_std"][:, 7:].any() and not ref["cam_rt_std"][0].any()
    assert np.all(ref["intr_std"][:, [0, 1, 4, 5, 6]] > 0) and np.all(ref["board_rt_std"] > 0)
    # fewer residuals than free columns: no sigma2
    q = _small()
    q = CR._with(q, view_count=np.minimum(q.view_count, 1))
    r = CR.cov_ref(q)
    assert r["dof"] <= 0 and r["sigma2"] != r["sigma2"]


def test_singular_blocks_are_reported():
    vc, vb = np.array([0, 1]), np.array([0, 0])
    cg = np.zeros((2, 15, 15)); cg[:, np.arange(13), np.arange(13)] = 4.0
    cf = np.zeros((2, 15), bool); cf[:, 6:8] = True
    bg = np.zeros((2, 6, 6)); bg[:] = 2 * np.eye(6)
    vx = np.zeros((2, 6, 15))
    ok = CR.cov_from_blocks(vc, vb, bg, vx, cg, cf, [True, False])
    assert ok["status"] == 0 and ok["min_pivot_ratio"] == 1.0 and ok["cam_cov"][0, 6, 0, 6] == 0.25 and ok["board_cov"][0, 0, 0] == 0.5
    bad = bg.copy(); bad[0, 5, 5] = 0.0
    r = CR.cov_from_blocks(vc, vb, bad, vx, cg, cf, [True, False])
    assert (r["status"], r["where"]) == (1, 0) and np.isnan(r["cam_cov"]).all()
    cg2 = cg.copy(); cg2[1, 6, 7] = cg2[1, 7, 6] = 4.0
    r = CR.cov_from_blocks(vc, vb, bg, vx, cg2, cf, [True, False])
    assert (r["status"], r["where"], r["min_pivot_ratio"]) == (2, 15 + 7, 0.0)


# mistake -> the cases it changes something on
WHERE = {"marginal_term_dropped": ["rig4"], "pair_tile_transposed": ["rig4", "mixed65"], "pair_tile_missing_board": ["rig4", "ring5"],
         "held_column_kept": ["mixed65-cx_cy", "mixed65-ds1"], "sigma2_forgotten": ["rig4"], "scale_not_undone": ["rig4", "mono7"]}


@pytest.mark.parametrize("mistake", CR.MISTAKES)
def test_tolerance_rejects_every_mistake(mistake):
    seen = []
    for name in WHERE[mistake]:
        p, kw, ref, e64, tol = CR.case(name)
        bad = CR.cov_ref(p, mistake=mistake, **kw)
        e = CR.worst(CR.cov_errors(bad, ref))
        print(f"{mistake} on {name}: error {e:.3e}, tolerance {tol:.3e}, e64 {CR.worst(e64):.3e}")
        seen.append(e > tol)
    assert any(seen), mistake


@pytest.mark.parametrize("name", list(CR.CASES))
def test_cases_are_regular_and_fp64_loses_little(name):
    """Every shared case: a regular reference, and e64 -- what a correct fp64 implementation loses -- far below 1."""
    p, kw, ref, e64, tol = CR.case(name)
    print(f"{name}: n_free {ref['n_free']}, min_pivot_ratio {ref['min_pivot_ratio']:.3e}, e64 {e64}, tolerance {tol:.3e}")
    assert ref["status"] == 0 and 0 < ref["min_pivot_ratio"] <= 1
    assert CR.worst(e64) < 1e-3
