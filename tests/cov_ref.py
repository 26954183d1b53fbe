"""Reference of the covariance stage (tscm.h: tscm_covariance; test infrastructure, may call the oracle): the
definition restated on the oracle's dual-number Jacobians (helpers.step_terms) with the helpers' _chol and
_batched_spd_inv, in np.longdouble or np.float64, with `mistake=` switches that alter the computation the way a kernel
could get it wrong, the error measure, the tolerance rule, and the cases the CPU and the GPU tests share."""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

from tests import helpers as H
from tests import robust_ref as R
from tscm_calib_amd import lib, synth
from tscm_calib_amd.problem import Problem

MISTAKES = ("marginal_term_dropped", "pair_tile_transposed", "pair_tile_missing_board", "held_column_kept", "sigma2_forgotten",
            "scale_not_undone")
EPS = 2.0 ** -52


# ----------------------------------------------------------------------------- the rules of the free columns
def free_columns(p: Problem, fixed=None):
    """cam_free [C,15], board_free [B] (bool) by tscm.h's rules, stated on the problem itself."""
    C, B = p.n_cameras, p.n_boards
    words = lib.fixed_masks(fixed, C)
    cam_seen, board_seen = np.zeros(C, bool), np.zeros(B, bool)
    for v in range(p.n_views):
        if p.view_count[v] > 0:
            cam_seen[p.view_camera[v]] = True
            board_seen[p.view_board[v]] = True
    cam_free = np.zeros((C, 15), bool)
    for m in range(C):
        pose_held = bool(p.mono) or bool(p.cam_pose_constant[m])
        for a in range(13):
            held = pose_held if a < 6 else bool((int(words[m]) >> (a - 6)) & 1)
            cam_free[m, a] = cam_seen[m] and not held
    bconst = np.zeros(B, bool) if p.board_pose_constant is None else np.asarray(p.board_pose_constant, dtype=bool)
    return cam_free, board_seen & ~bconst


# ----------------------------------------------------------------------------- the blocks
def blocks_from_terms(p: Problem, t: dict) -> dict:
    """The host layout of tscm_eval_normal_equations from helpers.step_terms, in the terms' dtype: board_gram [B,6,6],
    view_cross [V,6,15], cam_gram [C,15,15] (b, c columns zero), summed in view order."""
    dt = t["EE"].dtype
    C, B, V = p.n_cameras, p.n_boards, p.n_views
    bg, vx, cg = np.zeros((B, 6, 6), dt), np.zeros((V, 6, 15), dt), np.zeros((C, 15, 15), dt)
    vx[:, :, :13] = t["EF"]
    np.add.at(bg, np.asarray(p.view_board, dtype=np.int64), t["EE"])
    np.add.at(cg[:, :13, :13], np.asarray(p.view_camera, dtype=np.int64), t["FF"])
    return dict(board_gram=bg, view_cross=vx, cam_gram=cg, cost=t["cost"])


def _chol_fail(A):
    """(column, pivot) of the first pivot of A's Cholesky factorisation that is not > 0."""
    Rm = A.copy()
    for k in range(A.shape[0]):
        d = Rm[k, k]
        if not d > 0:
            return k, d
        l = Rm[k + 1:, k] / np.sqrt(d)
        Rm[k + 1:, k + 1:] -= np.outer(l, l)
    raise AssertionError("positive definite")


def _lower_inverse(L):
    """L^-1 of a lower triangular matrix, row by row, in L's dtype."""
    n = L.shape[0]
    X = np.zeros_like(L)
    for r in range(n):
        e = np.zeros(n, L.dtype); e[r] = 1
        X[r] = (e - L[r, :r] @ X[:r]) / L[r, r]
    return X


def cov_from_blocks(view_camera, view_board, board_gram, view_cross, cam_gram, cam_free, board_free, dtype=np.longdouble, mistake=None) -> dict:
    """The definition on given blocks: status / where / min_pivot_ratio / n_free as tscm_covariance_info, cam_cov [C,15,C,15],
    board_cov [B,6,6] in `dtype` (NaN behind a singular block)."""
    dt = np.dtype(dtype).type
    vc, vb = np.asarray(view_camera, dtype=np.int64), np.asarray(view_board, dtype=np.int64)
    bg, vx, cg = (np.asarray(x, dtype=dtype) for x in (board_gram, view_cross, cam_gram))
    cf, bf = np.asarray(cam_free, dtype=bool).reshape(-1, 15), np.asarray(board_free, dtype=bool)
    C, B = cg.shape[0], bg.shape[0]
    fb = np.nonzero(bf)[0]
    out = dict(status=0, where=-1, n_free=int(cf.sum()) + 6 * fb.size, min_pivot_ratio=float("nan"),
               cam_cov=np.full((C, 15, C, 15), np.nan, dtype), board_cov=np.full((B, 6, 6), np.nan, dtype), cam_free=cf, board_free=bf)
    Binv = np.zeros((B, 6, 6), dtype)
    for i in fb:                                        # one at a time: the lowest singular board is reported
        inv = None if H._chol(bg[i]) is None else H._batched_spd_inv(bg[i:i + 1])
        if inv is None:
            out.update(status=1, where=int(i))
            return out
        Binv[i] = inv[0]
    cfk = cf.copy()
    if mistake == "held_column_kept":
        keep = (cg[:, np.arange(15), np.arange(15)] > 0) & ~cf
        keep[:, :6] = False                                 # (an intrinsic: a constant pose kept would be the free gauge)
        held = np.nonzero(keep)
        if held[0].size:
            cfk[held[0][0], held[1][0]] = True              # a held column (its Gram diagonal is there) not removed
    W = vx * cfk[vc][:, None, :]
    Z = np.einsum("vij,vjk->vik", Binv[vb], W)
    views_of = [np.nonzero(vb == i)[0] for i in range(B)]
    S = np.zeros((C, 15, C, 15), dtype)
    S[np.arange(C), :, np.arange(C), :] = cg
    first_pair = None
    for i in fb:
        for v in views_of[i]:
            for w in views_of[i]:
                blk = W[v].T @ Z[w]
                a, b = int(vc[v]), int(vc[w])
                if a != b and first_pair is None:
                    first_pair = (min(a, b), max(a, b), int(i))
                if first_pair is not None and (min(a, b), max(a, b)) == first_pair[:2]:
                    if mistake == "pair_tile_missing_board" and int(i) == first_pair[2]:
                        continue                            # one board left out of one off-diagonal tile (both orientations)
                    if mistake == "pair_tile_transposed":
                        blk = blk.T                         # one off-diagonal tile (both orientations) used transposed
                S[a, :, b, :] -= blk
    fm = cfk.ravel()
    n = int(fm.sum())
    Sf = S.reshape(C * 15, C * 15)[np.ix_(fm, fm)]
    cam_cov = np.zeros((C * 15, C * 15), dtype)
    if n:
        diag = np.diagonal(Sf).copy()
        d = np.where(diag > 0, dt(1) / np.sqrt(np.where(diag > 0, diag, dt(1))), dt(np.nan))
        A = Sf * d[:, None] * d[None, :]
        A[np.arange(n), np.arange(n)] = np.where(diag > 0, dt(1), dt(np.nan))
        L = H._chol(A)
        if L is None:
            k, piv = _chol_fail(A)
            out.update(status=2, where=int(np.nonzero(fm)[0][k]), min_pivot_ratio=float(piv))
            return out
        out["min_pivot_ratio"] = float(np.min(np.diagonal(L) ** 2))
        X = _lower_inverse(L)
        und = d.copy()
        if mistake == "scale_not_undone":
            und[n // 2] = 1                                 # the scaling of one column not undone
        cam_cov[np.ix_(fm, fm)] = (X.T @ X) * und[:, None] * und[None, :]
    else:
        out["min_pivot_ratio"] = 1.0
    out["cam_cov"] = cam_cov.reshape(C, 15, C, 15)
    board_cov = np.zeros((B, 6, 6), dtype)
    for i in fb:
        acc = np.zeros((6, 6), dtype)
        if mistake != "marginal_term_dropped":
            for v in views_of[i]:
                for w in views_of[i]:
                    acc += Z[v] @ out["cam_cov"][vc[v], :, vc[w], :] @ Z[w].T
        board_cov[i] = Binv[i] + (acc + acc.T) / 2
    out["board_cov"] = board_cov
    out["_Z"] = Z                                           # for refine_full_inverse: the cross blocks are products of these
    return out


def _to_fraction(x) -> Fraction:
    """A longdouble as an exact rational: its rounding to a double, and what that left (which a double holds exactly)."""
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - np.longdouble(hi)))


def _from_fraction(r: Fraction):
    hi = float(r)
    return np.longdouble(hi) + np.longdouble(float(r - Fraction(hi)))


def refine_full_inverse(p: Problem, out: dict, jets, max_steps: int = 8) -> dict:
    """Iterative refinement of cov_from_blocks' result as the inverse of the full J^T J over the free columns, with the
    residual in exact rational arithmetic (every entry of the oracle's Jacobian and every longdouble is a dyadic rational):
    X <- X + X (I - M X).  A longdouble Schur inverse is off by condition * u; with an exact residual each step squares
    |I - M X|, and the result is the inverse rounded to longdouble whatever the condition, as long as the start is closer
    than |I - M X| < 1 -- a start with a structural mistake is not (the caller checks `first_residual`).  The start is all
    of the inverse in Schur form: cam_cov, board_cov, and the cross blocks, which the stage itself does not form,
    Sigma_c,b(i) = -sum_v Sigma_cc[:, m_v] Z_v^T and Sigma_b(i),b(j) = sum_{v of i, w of j} Z_v Sigma_cc[m_v, m_w] Z_w^T.
    O(n_free^3) rational operations: for small problems.  Returns a copy of `out` with cam_cov and board_cov refined,
    first_residual = max |I - M X| of the start and refine_steps."""
    ld = np.longdouble
    cf, bf, Z = out["cam_free"], out["board_free"], out["_Z"]
    C, B, V = p.n_cameras, p.n_boards, p.n_views
    vc, vb = np.asarray(p.view_camera, dtype=np.int64), np.asarray(p.view_board, dtype=np.int64)
    col_c = -np.ones((C, 15), int); col_c[cf] = np.arange(int(cf.sum()))
    nc = int(cf.sum())
    col_b = -np.ones(B, int); col_b[bf] = nc + 6 * np.arange(int(bf.sum()))
    n = nc + 6 * int(bf.sum())
    # M = J^T J exactly, row by row of J (a corner's two rows touch one camera and one board)
    _, _, Jc, Jb, Ji = jets
    M = [[Fraction(0)] * n for _ in range(n)]
    k = 0
    for v in range(V):
        m, b = int(vc[v]), int(vb[v])
        for _ in range(int(p.view_count[v])):
            for e in range(2):
                F = np.concatenate([np.asarray(Jc[k]).reshape(2, 6)[e], np.asarray(Ji[k]).reshape(2, 9)[e]])
                row = [(int(col_c[m, a]), Fraction(float(F[a]))) for a in range(15) if col_c[m, a] >= 0]
                if col_b[b] >= 0:
                    row += [(int(col_b[b]) + a, Fraction(float(np.asarray(Jb[k]).reshape(2, 6)[e, a]))) for a in range(6)]
                for i, x in row:
                    Mi = M[i]
                    for j, y in row:
                        Mi[j] += x * y
            k += 1
    # the start, all blocks
    X = np.zeros((n, n), ld)
    cam = np.asarray(out["cam_cov"], dtype=ld).reshape(C * 15, C * 15)
    ci = np.nonzero(cf.ravel())[0]
    X[:nc, :nc] = cam[np.ix_(ci, ci)]
    cc = out["cam_cov"]
    views_of = {int(i): np.nonzero(vb == i)[0] for i in np.nonzero(bf)[0]}
    for i, vi in views_of.items():
        oi = col_b[i]
        cb = np.zeros((C * 15, 6), ld)
        for v in vi:
            cb -= np.asarray(cc[:, :, vc[v], :], dtype=ld).reshape(C * 15, 15) @ Z[v].T
        X[:nc, oi:oi + 6] = cb[ci]
        X[oi:oi + 6, :nc] = cb[ci].T
        for j, vj in views_of.items():
            if j == i:
                X[oi:oi + 6, oi:oi + 6] = out["board_cov"][i]
                continue
            acc = np.zeros((6, 6), ld)
            for v in vi:
                for w in vj:
                    acc += Z[v] @ cc[vc[v], :, vc[w], :] @ Z[w].T
            X[oi:oi + 6, col_b[j]:col_b[j] + 6] = acc
    first, last, steps = None, None, 0
    for steps in range(1, max_steps + 1):
        XF = [[_to_fraction(X[i, j]) for j in range(n)] for i in range(n)]
        XT = list(zip(*XF))
        Rm = np.zeros((n, n), ld)
        for i in range(n):
            Mi = [(j, y) for j, y in enumerate(M[i]) if y]
            for j in range(n):
                col = XT[j]
                Rm[i, j] = _from_fraction((1 if i == j else 0) - sum(y * col[q] for q, y in Mi))
        rmax = float(np.max(np.abs(Rm)))
        first = rmax if first is None else first
        if not rmax < 1 or (last is not None and rmax > last / 4):
            break                                           # no start this iteration improves / the floor condition * u of
        X = X + X @ Rm                                      # a residual of X rounded to longdouble is reached
        last = rmax
    res = dict(out, first_residual=first, refine_steps=steps)
    if last is None:
        return res                                          # no step taken: the blocks as they came
    X = (X + X.T) / 2
    cam2 = np.zeros((C * 15, C * 15), ld); cam2[np.ix_(ci, ci)] = X[:nc, :nc]
    board2 = np.zeros((B, 6, 6), ld)
    for i in views_of:
        board2[i] = X[col_b[i]:col_b[i] + 6, col_b[i]:col_b[i] + 6]
    res.update(cam_cov=cam2.reshape(C, 15, C, 15), board_cov=board2)
    return res


def cov_ref(p: Problem, *, fixed=None, loss=None, dtype=np.longdouble, mistake=None, jets=None, refine=False) -> dict:
    """tscm_covariance on the oracle's Jacobians: cov_from_blocks plus n_residuals, cost, dof, sigma2 and the standard
    deviations.  loss: (kind, scale) as for api.calibrate -- the rows corrected as tests/robust_ref.py corrects them.
    refine (longdouble, no mistake, small problems): the blocks refined as refine_full_inverse does, accurate to the rounding
    of longdouble whatever the condition of the problem; the plain run keeps condition * u, which is what e64 measures."""
    if jets is None:
        jets = H.orc.evaluate(p, jets=True)
    if loss is not None:
        jets = R.robust_jets(p, loss[0], float(loss[1]), jets)
    t = H.step_terms(p, jets=jets, dtype=dtype)
    blk = blocks_from_terms(p, t)
    cam_free, board_free = free_columns(p, fixed)
    out = cov_from_blocks(p.view_camera, p.view_board, blk["board_gram"], blk["view_cross"], blk["cam_gram"], cam_free, board_free, dtype, mistake)
    if refine:
        assert np.dtype(dtype) == np.longdouble and mistake is None and out["status"] == 0
        out = refine_full_inverse(p, out, jets)
    n_res = 2 * int(np.sum(p.view_count))
    dof = n_res - out["n_free"]
    sigma2 = 2.0 * blk["cost"] / dof if dof > 0 else float("nan")
    C, B = p.n_cameras, p.n_boards
    s2 = 1.0 if mistake == "sigma2_forgotten" else sigma2
    cd = np.asarray(np.diagonal(out["cam_cov"].reshape(C * 15, C * 15)), dtype=np.float64).reshape(C, 15)
    bd = np.asarray(np.diagonal(out["board_cov"], axis1=1, axis2=2), dtype=np.float64)
    nan_if = np.nan if out["status"] else 0.0
    cam_std = np.where(cam_free, np.sqrt(s2 * cd), nan_if)
    out.update(n_residuals=n_res, cost=blk["cost"], dof=dof, sigma2=sigma2, cam_rt_std=cam_std[:, :6], intr_std=cam_std[:, 6:],
               board_rt_std=np.where(board_free[:, None], np.sqrt(s2 * bd), nan_if))
    return out


# ----------------------------------------------------------------------------- error measure and tolerance
def cov_errors(got: dict, ref: dict) -> dict:
    """max over the free (i, j) of |got_ij - ref_ij| / sqrt(ref_ii ref_jj) for cam_cov and inside each board_cov block;
    relative errors of the standard deviations and of sigma2 (where both dicts carry them)."""
    cf, bf = ref["cam_free"].ravel(), ref["board_free"]
    n15 = cf.size
    ld = np.longdouble
    a, b = np.asarray(got["cam_cov"], dtype=ld).reshape(n15, n15)[np.ix_(cf, cf)], np.asarray(ref["cam_cov"], dtype=ld).reshape(n15, n15)[np.ix_(cf, cf)]
    d = np.sqrt(np.diagonal(b))
    err = dict(cam=float(np.max(np.abs(a - b) / (d[:, None] * d[None, :]))) if a.size else 0.0)
    ga, gb = np.asarray(got["board_cov"], dtype=ld)[bf], np.asarray(ref["board_cov"], dtype=ld)[bf]
    db = np.sqrt(np.diagonal(gb, axis1=1, axis2=2))
    err["board"] = float(np.max(np.abs(ga - gb) / (db[:, :, None] * db[:, None, :]))) if ga.size else 0.0
    if "intr_std" in got and "intr_std" in ref:
        e = 0.0
        for key, mask in (("cam_rt_std", ref["cam_free"][:, :6]), ("intr_std", ref["cam_free"][:, 6:]), ("board_rt_std", np.repeat(bf[:, None], 6, axis=1))):
            g, r = np.asarray(got[key], dtype=np.float64)[mask], np.asarray(ref[key], dtype=np.float64)[mask]
            if g.size:
                e = max(e, float(np.max(np.abs(g - r) / r)))
        err["std"] = e
        err["sigma2"] = abs(got["sigma2"] - ref["sigma2"]) / ref["sigma2"] if ref["dof"] > 0 else 0.0
    return err


def worst(err: dict) -> float:
    v = list(err.values())
    return float("inf") if any(x != x for x in v) else max(v)


def tolerance(e64: float, n_free: int) -> float:
    """What a device result may differ from the longdouble reference: 8 max(e64, n_free 2^-52), e64 the error of this
    reference run in float64 on the same inputs.  The 8 covers another summation and elimination order, nothing else."""
    return 8.0 * max(e64, n_free * EPS)


# ----------------------------------------------------------------------------- the shared cases
def _with(p: Problem, **kw) -> Problem:
    q = p.copy()
    for k, v in kw.items():
        setattr(q, k, v)
    return q.normalised()


def _mixed65():
    return H.mixed_visibility_rig(n_frames=65)


def _const_boards():
    p = _mixed65()
    c = np.zeros(p.n_boards, np.uint8)
    c[[0, 7, 33, 64]] = 1
    return _with(p, board_pose_constant=c)


def _camera_without_views():
    """mixed65 with a fifth camera that no view uses."""
    p = _mixed65()
    g = synth.make_problem(5, 4, 5, noise_px=0.0)
    q = Problem(5, p.n_boards, p.board_xy, p.view_camera, p.view_board, p.view_offset, p.view_count, p.obs_u, p.obs_v,
                np.concatenate([p.cam_rt, g.cam_rt[4:5]]), np.concatenate([p.intr, g.intr[4:5]]), p.board_rt,
                np.concatenate([p.cam_pose_constant, np.zeros(1, np.uint8)]), False, meta={})
    return q.normalised()


def _outliers():
    p = _mixed65()
    rng = np.random.default_rng(99)
    k = rng.choice(p.obs_u.size, size=p.obs_u.size // 20, replace=False)
    u, v = p.obs_u.copy(), p.obs_v.copy()
    u[k] += rng.normal(scale=8.0, size=k.size)
    v[k] += rng.normal(scale=8.0, size=k.size)
    return _with(p, obs_u=u, obs_v=v)


_DS1 = np.array([0, lib.MODEL_DS, 0, 0], dtype=np.int64)
_ALL2 = np.array([0, 0, lib.FIX_INTRINSICS, 0], dtype=np.int64)
RING5 = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)]

# name -> (problem, keyword arguments of api.covariance / cov_ref)
CASES = {
    "rig4": (lambda: H.small_rig(4, 12), {}),
    "mixed65": (_mixed65, {}),
    "ring5": (lambda: H.rig_with_pairs(5, RING5), {}),
    "ring8": (lambda: synth.make_problem(8, 6, 23), {}),
    "chain12": (lambda: H.rig_with_pairs(12, [(i, i + 1) for i in range(11)], frames_per_pair=2), {}),
    "mono7": (lambda: synth.make_problem(1, 7, 20241), {}),
    "mixed65-cx_cy": (_mixed65, dict(fixed=("cx", "cy"))),
    "mixed65-ds1": (_mixed65, dict(fixed=_DS1)),
    "mixed65-all7_2": (_mixed65, dict(fixed=_ALL2)),
    "mixed65-const_boards": (_const_boards, {}),
    "mixed65-unseen": (lambda: H.rig_with_unseen_boards(_mixed65(), 3), {}),
    "mixed65-idle_camera": (_camera_without_views, {}),
    "mixed65-huber": (_outliers, dict(loss=("huber", 1.0))),
}


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(problem, kwargs, longdouble reference, e64 errors, tolerance) of a case, computed once per process."""
    make, kw = CASES[name]
    p = make()
    jets = H.orc.evaluate(p, jets=True)
    ref = cov_ref(p, jets=jets, **kw)
    assert ref["status"] == 0, (name, ref["status"], ref["where"])
    e64 = cov_errors(cov_ref(p, jets=jets, dtype=np.float64, **kw), ref)
    return p, kw, ref, e64, tolerance(worst(e64), ref["n_free"])
