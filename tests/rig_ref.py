"""Extended-precision reference for the rig initialisation (multi_calib.cpp:25-151) with an a-priori
bound on the difference of the HIP kernels from it.

Hypothesis errors (k_rig_points -> k_rig_hyp_errors<SKEW> -> k_rig_hyp_reduce)
-------------------------------------------------------------------------------
The reference starts from the hypotheses (Rs, ts) tscm_rig_stage_errors returns and from the board
poses Rt_to_R_t makes on the host (float32 r1, r2 and their float32 cross product, pinned bit for bit
by tests/test_rig_oracle.py); those are exact inputs.  Every quantity the kernel forms is carried as a
pair (value, e): the value in np.longdouble (64-bit significand, so its own rounding is ~2^11 times
below fp64's), e an fp64 bound on |kernel's fp64 value - value|.  With u = 2^-53:

  a*b      e = |a| e_b + |b| e_a + e_a e_b + u |ab|
  a+b      e = e_a + e_b + u |a+b|                      (a*b + c: both rules, so an fma or the
                                                          compiler's contraction only does better)
  x*rsq(x) e = e_x / sqrt(x) + 5u (sqrt(x) + e_x / sqrt(x))
             the seed-plus-one-correction reciprocal square root is within 2 ulp (4u relative, the
             claim of tscm_fastmath.h) and the product x * r adds one rounding
  rcp(x)   e = e_x / (|x| (|x| - e_x)) + 4u (|1/x| + that)     (2 ulp)

The kernel's chain per lane (hypothesis j), direction and corner:
  q = R_k w + t_k                 k_rig_points, 3 products and 3 sums per coordinate
  A = Rp Rs_j^T, a = tp - A ts_j  (direction 0), A = Rs_j Rp^T, a = ts_j - A tp (direction 1)
  P = A q + a                     three fused dot products
  rho2, s1, d1, z1, s2, d2, z2, s3, d3, ksai = beta d3 + z2 with beta = alpha / (1 - alpha)
                                  (two IEEE roundings: e_beta = 2u |beta|), ik = rcp(ksai)
  mx = X ik, my = Y ik, u = fx mx + b my + cx, v = c mx + fy my + cy   (skew terms only under SKEW)
  du = pu - u, dv = pv - v
  term = sqrt(max(du^2 + dv^2, 1e-300))
The last step is bounded in absolute terms, because zero-noise terms have du, dv ~ 0 and any
relative bound through sqrt would blow up there: by the triangle inequality for the 2-norm,
| ||(du, dv)||_computed - ||(du, dv)||_reference | <= hypot(e_du, e_dv), the sum of squares adds
gamma_2 / 2 ~ u relative, the rsq-based square root 5u, and the floor max(., 1e-300) at most
sqrt(1e-300) = 1e-150 absolute per term:
  e_term = hypot(e_du, e_dv) + 6u (|term| + hypot(e_du, e_dv)) + 1e-150.
Summation: a lane sums n corner terms into one board-direction sum, adds 2 such sums per board of
its slice (per = ceil(K / ksplit) boards at most), and k_rig_hyp_reduce adds the ksplit partial sums
one after the other, so each term goes through at most D = n + 2 per + ksplit additions of
non-negative numbers: |error| <= sum(e_term) + gamma_D sum(|term| + e_term), gamma_D = D u / (1 - D u).
Over every partition 1 <= ksplit <= K, D <= n + 2K + 1 (ksplit = 1), the partition-free bound.

Board choice (k_rig_boards)
---------------------------
Rs_q = cR_m^T chR, ts_q = cR_m^T (cht - ct_m) for each camera m seeing the board, then per camera k
R = cR_k Rs_q, t = cR_k ts_q + ct_k, P = R w + t and the IEEE project_point (sqrt and divisions
correctly rounded: 1u each), term = sqrt(du^2 + dv^2) without a floor, summed over n corners then
over the nc cameras: D = n + nc.

Everything is first order in u except where written out; the neglected terms are O(u^2) relative.
"""
from __future__ import annotations

import numpy as np

from tests.helpers import np_Rt_to_R_t

LD = np.longdouble
U = 2.0 ** -53
FLOOR_TERM = 1e-150               # sqrt(1e-300): the kernel's floor under e^2 (rsq(0) = inf)


class EV:
    """A value in long double and an fp64 bound on the kernel's deviation from it."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=LD)
        self.e = np.zeros(self.v.shape) if e is None else np.asarray(e, dtype=np.float64)

    @property
    def a(self):
        return np.abs(self.v).astype(np.float64)


def mul(x: EV, y: EV) -> EV:
    v = x.v * y.v
    return EV(v, x.a * y.e + y.a * x.e + x.e * y.e + U * np.abs(v).astype(np.float64))


def add(x: EV, y: EV) -> EV:
    v = x.v + y.v
    return EV(v, x.e + y.e + U * np.abs(v).astype(np.float64))


def sub(x: EV, y: EV) -> EV:
    return add(x, EV(-y.v, y.e))


def fsqrt(x: EV, rel: float = 5 * U) -> EV:
    """sqrt; rel = relative error of the computation from its rounded input (5u: x * fast_rsqrt(x), u: IEEE)."""
    v = np.sqrt(x.v)
    s = v.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        prop = np.where(x.e > 0, x.e / s, 0.0)
    return EV(v, prop + rel * (s + prop))


def frcp(x: EV, rel: float = 4 * U) -> EV:
    """1/x; rel = relative error from the rounded input (4u: fast_rcp's 2 ulp)."""
    v = LD(1) / x.v
    ax = x.a
    with np.errstate(divide="ignore", invalid="ignore"):
        prop = np.where(x.e < ax, x.e / (ax * (ax - x.e)), np.inf)
    return EV(v, prop + rel * (np.abs(v).astype(np.float64) + prop))


def fdiv(x: EV, y: EV) -> EV:
    """IEEE x / y: one rounding."""
    v = x.v / y.v
    ay = y.a
    with np.errstate(divide="ignore", invalid="ignore"):
        prop = np.where(y.e < ay, (x.e + np.abs(v).astype(np.float64) * y.e) / (ay - y.e), np.inf)
    return EV(v, prop + U * np.abs(v).astype(np.float64))


def gamma(d) -> np.ndarray:
    d = np.asarray(d, dtype=np.float64)
    return d * U / (1.0 - d * U)


def matvec(A, Ae, x, xe, c=None, ce=None):
    """y = A x (+ c) with A [..., 3, 3], x [..., 3]: value and bound of the plain (or contracted) dot products."""
    v = np.einsum("...ij,...j->...i", A, x)
    mag = np.einsum("...ij,...j->...i", np.abs(A).astype(np.float64), np.abs(x).astype(np.float64))
    prop = np.einsum("...ij,...j->...i", np.abs(A).astype(np.float64), xe) + np.einsum("...ij,...j->...i", Ae, np.abs(x).astype(np.float64) + xe)
    k = 3
    if c is not None:
        v = v + c
        mag = mag + np.abs(c).astype(np.float64)
        prop = prop + (0.0 if ce is None else ce)
        k = 4
    return v, prop + gamma(k) * mag


def beta_of(alpha) -> EV:
    al = LD(alpha)
    b = al / (LD(1) - al)
    return EV(b, 2.0 * U * abs(float(b)) * (1 + 4 * U))


# ------------------------------------------------------------------------------------------------ stage
def stage_points(inp, i):
    """The prepared points of stage i (k_rig_points) in long double with their fp64 bounds, and the pixels:
    direction 0 = camera i's board points scored in camera i-1, direction 1 = the reverse."""
    common = np.nonzero(inp.has[i - 1].astype(bool) & inp.has[i].astype(bool))[0]
    W = inp.worlds.astype(LD)
    q, qe, pu, pv = [], [], [], []
    for cam, other in ((i, i - 1), (i - 1, i)):
        R, t = np_Rt_to_R_t(inp.Rt[cam, common])
        R, t = R.astype(LD), t.astype(LD)
        v = np.einsum("kij,nj->kni", R, W) + t[:, None, :]
        mag = np.einsum("kij,nj->kni", np.abs(R), np.abs(W)) + np.abs(t)[:, None, :]
        q.append(v); qe.append(gamma(4) * mag.astype(np.float64))
        pu.append(inp.pix_u[other, common].astype(LD)); pv.append(inp.pix_v[other, common].astype(LD))
    return common, np.stack(q), np.stack(qe), np.stack(pu), np.stack(pv)


def host_hypotheses(inp, i, Rp, tp):
    """multi_calib.cpp:29-48 in fp64 numpy (the host's formula; not necessarily its rounding order)."""
    common = np.nonzero(inp.has[i - 1].astype(bool) & inp.has[i].astype(bool))[0]
    Ri, ti = np_Rt_to_R_t(inp.Rt[i, common])
    Rk, tk = np_Rt_to_R_t(inp.Rt[i - 1, common])
    Rik = Ri @ np.swapaxes(Rk, 1, 2)
    tik = ti - np.einsum("kij,kj->ki", Rik, tk)
    return Rik @ np.asarray(Rp), np.einsum("kij,j->ki", Rik, np.asarray(tp)) + tik


def pixel_terms(I, beta: EV, P: EV, pu, pv, skew: bool) -> EV:
    """pixel_error<SKEW> (tscm_rig.hip) as value + bound, elementwise over P [..., 3]."""
    X, Y, Z = EV(P.v[..., 0], P.e[..., 0]), EV(P.v[..., 1], P.e[..., 1]), EV(P.v[..., 2], P.e[..., 2])
    c = [EV(LD(x)) for x in I]
    rho2 = add(mul(Y, Y), mul(X, X))
    d1 = fsqrt(add(mul(Z, Z), rho2))
    z1 = add(mul(c[4], d1), Z)
    d2 = fsqrt(add(mul(z1, z1), rho2))
    z2 = add(mul(c[5], d2), z1)
    d3 = fsqrt(add(mul(z2, z2), rho2))
    ik = frcp(add(mul(beta, d3), z2))
    mx, my = mul(X, ik), mul(Y, ik)
    if skew:
        u = add(mul(c[0], mx), add(mul(c[7], my), c[2]))
        v = add(mul(c[8], mx), add(mul(c[1], my), c[3]))
    else:
        u = add(mul(c[0], mx), c[2])
        v = add(mul(c[1], my), c[3])
    du, dv = sub(EV(pu), u), sub(EV(pv), v)
    term = np.sqrt(du.v * du.v + dv.v * dv.v)
    h = np.hypot(du.e, dv.e)
    return EV(term, h + 6 * U * (np.abs(term).astype(np.float64) + h) + FLOOR_TERM)


def stage_reference(inp, i, Rp, tp, Rs, ts, js=None, depth=None, chunk_elems=1 << 21):
    """Long-double errors of hypotheses js (default: all) of stage i and their fp64 bounds.
    depth = additions each term goes through (n + 2 per + ksplit); default: the partition-free n + 2K + 1.
    Returns (ref [nj] longdouble, bound [nj] float64)."""
    common, q, qe, pu, pv = stage_points(inp, i)
    K, n = common.size, inp.n_points
    js = np.arange(len(Rs)) if js is None else np.asarray(js)
    D = n + 2 * K + 1 if depth is None else depth
    skew = bool(np.any(inp.intr[[i - 1, i], 7:9] != 0.0))
    Rp, tp = np.asarray(Rp, dtype=LD), np.asarray(tp, dtype=LD)
    betas = [beta_of(inp.intr[i - 1, 6]), beta_of(inp.intr[i, 6])]
    ref = np.zeros(js.size, dtype=LD)
    bound = np.zeros(js.size)
    step = max(1, chunk_elems // (2 * K * n))
    for s0 in range(0, js.size, step):
        jj = js[s0:s0 + step]
        Rsj, tsj = np.asarray(Rs, dtype=LD)[jj], np.asarray(ts, dtype=LD)[jj]
        tot = np.zeros(jj.size, dtype=LD)
        terr = np.zeros(jj.size)
        for d in range(2):
            if d == 0:      # A = Rp Rs^T, a = tp - A ts
                A, Ae = matvec_mm(Rp[None], Rsj.transpose(0, 2, 1))
                a, ae = matvec(A, Ae, tsj, np.zeros(tsj.shape))
                a, ae = tp[None] - a, ae + U * np.abs(tp[None] - a).astype(np.float64)
            else:           # A = Rs Rp^T, a = ts - A tp
                A, Ae = matvec_mm(Rsj, Rp.T[None])
                a, ae = matvec(A, Ae, np.broadcast_to(tp, tsj.shape), np.zeros(tsj.shape))
                a, ae = tsj - a, ae + U * np.abs(tsj - a).astype(np.float64)
            # P = A q + a over [jj, K, n]
            Pv, Pe = matvec(A[:, None, None], Ae[:, None, None], q[d][None], qe[d][None], a[:, None, None], ae[:, None, None])
            I = inp.intr[i - 1] if d == 0 else inp.intr[i]
            t = pixel_terms(I, betas[d], EV(Pv, Pe), pu[d][None], pv[d][None], skew)
            tot += t.v.reshape(jj.size, -1).sum(axis=1)
            terr += t.e.reshape(jj.size, -1).sum(axis=1)
        ref[s0:s0 + step] = tot
        bound[s0:s0 + step] = terr + gamma(D) * (np.abs(tot).astype(np.float64) + terr)
    return ref, bound


def matvec_mm(A, B):
    """C = A B for exact inputs (rows of 3-term dot products): value and bound."""
    v = np.einsum("...ik,...kj->...ij", A, B)
    mag = np.einsum("...ik,...kj->...ij", np.abs(A), np.abs(B)).astype(np.float64)
    return v, gamma(3) * mag


def stage_depth(n, K, ksplit):
    """Additions a term goes through in the kernel for a partition into ksplit slices."""
    per = -(-K // ksplit)
    return n + 2 * per + ksplit


def host_partition(K, ksplit_req=0, resident=None):
    """The host's partition rule of rig_stage (tscm_rig.hip): jgroups and ksplit, and the slices [k0, k1)."""
    jgroups = (K + 63) // 64
    if ksplit_req:
        ksplit = ksplit_req
    else:
        ksplit = max(1, min(K, resident // jgroups))
    per = -(-K // ksplit)
    slices = [(b * per, min(K, b * per + per)) for b in range(ksplit)]
    return jgroups, ksplit, slices


def skew_instantiation(intr, i) -> bool:
    """SKEW of k_rig_hyp_errors as the host picks it: b or c != 0 in camera i or i-1."""
    return bool(intr[i, 7] != 0.0 or intr[i, 8] != 0.0 or intr[i - 1, 7] != 0.0 or intr[i - 1, 8] != 0.0)


def first_min(err, limit=1e10) -> int:
    """The strict-< first-minimum scan (multi_calib.cpp:79-83); -1 when nothing is < limit (NaN never is)."""
    best, idx = limit, -1
    for j, e in enumerate(err):
        if e < best:
            best, idx = e, j
    return idx


# ------------------------------------------------------------------------------------------------ boards
def board_hypotheses(inp, cam_R, cam_t, b):
    """multi_calib.cpp:104-118 for board b in fp64 numpy: the cameras seeing it and their (Rs, ts)."""
    ids = np.nonzero(inp.has[:, b])[0]
    R, t = np_Rt_to_R_t(inp.Rt[ids, b])
    cRt = np.swapaxes(cam_R[ids], 1, 2)
    return ids, cRt @ R, np.einsum("kij,kj->ki", cRt, t - cam_t[ids])


def board_reference(inp, cam_R, cam_t, b):
    """multi_calib.cpp:119-151 for board b: long-double error of every camera's hypothesis and its bound for
    k_rig_boards (device-side hypotheses, plain dot products, IEEE project_point, no floor).
    Returns ids, ref [nc], bound [nc]."""
    ids = np.nonzero(inp.has[:, b])[0]
    nc, n = ids.size, inp.n_points
    cR, ct = np.asarray(cam_R, dtype=LD)[ids], np.asarray(cam_t, dtype=LD)[ids]
    R, t = np_Rt_to_R_t(inp.Rt[ids, b])
    R, t = R.astype(LD), t.astype(LD)
    cRt = cR.transpose(0, 2, 1)
    Rs, Rse = matvec_mm(cRt, R)                                       # [nc(q)]
    dt = t - ct
    dte = U * np.abs(dt).astype(np.float64)
    ts, tse = matvec(cRt, np.zeros(cRt.shape), dt, dte)
    # camera k scoring hypothesis q: Rkq = cR_k Rs_q, tkq = cR_k ts_q + ct_k    -> [k, q]
    Rkq = np.einsum("kab,qbc->kqac", cR, Rs)
    Rkqe = np.einsum("kab,qbc->kqac", np.abs(cR).astype(np.float64), Rse) + gamma(3) * np.einsum(
        "kab,qbc->kqac", np.abs(cR), np.abs(Rs)).astype(np.float64)
    tkq, tkqe = matvec(np.broadcast_to(cR[:, None], (nc, nc, 3, 3)), np.zeros((nc, nc, 3, 3)),
                       np.broadcast_to(ts[None], (nc, nc, 3)), np.broadcast_to(tse[None], (nc, nc, 3)),
                       np.broadcast_to(ct[:, None], (nc, nc, 3)), None)
    W = inp.worlds.astype(LD)
    Pv = np.einsum("kqij,nj->kqni", Rkq, W) + tkq[:, :, None, :]
    Pe = (np.einsum("kqij,nj->kqni", Rkqe, np.abs(W).astype(np.float64)) + tkqe[:, :, None, :]
          + gamma(4) * (np.einsum("kqij,nj->kqni", np.abs(Rkq), np.abs(W)) + np.abs(tkq)[:, :, None, :]).astype(np.float64))
    terms = np.zeros((nc, nc, n), dtype=LD)
    terr = np.zeros((nc, nc, n))
    for kk in range(nc):
        I = inp.intr[ids[kk]]
        P = EV(Pv[kk], Pe[kk])
        X, Y, Z = EV(P.v[..., 0], P.e[..., 0]), EV(P.v[..., 1], P.e[..., 1]), EV(P.v[..., 2], P.e[..., 2])
        c = [EV(LD(x)) for x in I]
        r2 = add(mul(X, X), mul(Y, Y))
        d1 = fsqrt(add(r2, mul(Z, Z)), U)
        z1 = add(Z, mul(c[4], d1))
        d2 = fsqrt(add(r2, mul(z1, z1)), U)
        z2 = add(z1, mul(c[5], d2))
        d3 = fsqrt(add(r2, mul(z2, z2)), U)
        ksai = add(z2, mul(beta_of(I[6]), d3))
        u = add(add(fdiv(mul(c[0], X), ksai), fdiv(mul(c[7], Y), ksai)), c[2])
        v = add(add(fdiv(mul(c[8], X), ksai), fdiv(mul(c[1], Y), ksai)), c[3])
        du = sub(EV(inp.pix_u[ids[kk], b].astype(LD)), u)
        dv = sub(EV(inp.pix_v[ids[kk], b].astype(LD)), v)
        tv = np.sqrt(du.v * du.v + dv.v * dv.v)
        h = np.hypot(du.e, dv.e)
        terms[kk], terr[kk] = tv, h + 2 * U * (np.abs(tv).astype(np.float64) + h)
    ref = terms.sum(axis=(0, 2))
    te = terr.sum(axis=(0, 2))
    return ids, ref, te + gamma(n + nc) * (np.abs(ref).astype(np.float64) + te)


# ------------------------------------------------------------------------------------------------ rigs
def _grid(n):
    shape = {1: (1, 1), 4: (2, 2), 54: (9, 6), 88: (11, 8)}[n]
    pitch = 45.0 if n != 88 else 30.0
    x, y = np.meshgrid(np.arange(shape[0]) * pitch, np.arange(shape[1]) * pitch)
    w = np.stack([x.ravel(), y.ravel(), np.zeros(n)], axis=1)
    return w - np.array([w[:, 0].mean(), w[:, 1].mean(), 0.0]) * (n > 1)


def _project(I, P):
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    fx, fy, cx, cy, xi, lam, al, b, c = I
    d1 = np.sqrt(X * X + Y * Y + Z * Z)
    z1 = Z + xi * d1
    z2 = z1 + lam * np.sqrt(X * X + Y * Y + z1 * z1)
    ks = z2 + al / (1 - al) * np.sqrt(X * X + Y * Y + z2 * z2)
    return fx * X / ks + b * Y / ks + cx, c * X / ks + fy * Y / ks + cy


SKEWS = {"none": (), "cur": (1,), "prev": (0,), "both": (0, 1)}


def stage_rig(K, n, skew="none", seed=0, noise_px=0.1, only=3, rt_noise_cams=(0, 1)):
    """Two cameras with K boards in common, interleaved (mixed visibility) with `only` boards seen by camera 0
    only, `only` by camera 1 only and one by neither.  Rt = ground truth perturbed by 0.01 rad / 3 mm, pixels =
    projections with skew where asked plus noise; rt_noise_cams = the cameras whose Rt is perturbed.  Stage i = 1."""
    from tscm_calib_amd import synth
    from tscm_calib_amd.rig import RigInput
    rng = np.random.default_rng(seed)
    intr = synth.CALIB_INTR[:2].copy()
    for m, (b, c) in zip(SKEWS[skew], ((0.8, -0.6), (-0.5, 0.7))[:len(SKEWS[skew])]):
        intr[m, 7], intr[m, 8] = b, c
    camR = np.stack([np.eye(3), synth.rodrigues(np.array([0.02, 0.25, -0.03]))])
    camt = np.array([[0.0, 0.0, 0.0], [-150.0, 4.0, 20.0]])
    vis = ["c"] * K + ["a"] * only + ["b"] * only + ["none"]
    order = rng.permutation(len(vis))
    vis = [vis[o] for o in order]
    B = len(vis)
    W = _grid(n)
    has = np.zeros((2, B), dtype=np.uint8)
    Rt = np.zeros((2, B, 3, 3))
    pu, pv = np.zeros((2, B, n)), np.zeros((2, B, n))
    for j, s in enumerate(vis):
        Rb = synth.rodrigues(rng.normal(scale=0.3, size=3))
        tb = np.array([rng.uniform(-250, 250), rng.uniform(-200, 200), rng.uniform(700, 1400)])
        for m in range(2):
            if not (s == "c" or (s == "a" and m == 0) or (s == "b" and m == 1)):
                continue
            R, t = camR[m] @ Rb, camR[m] @ tb + camt[m]
            u, v = _project(intr[m], W @ R.T + t)
            has[m, j] = 1
            pu[m, j] = u + noise_px * rng.normal(size=n)
            pv[m, j] = v + noise_px * rng.normal(size=n)
            sr, st = (0.01, 3.0) if m in rt_noise_cams else (0.0, 0.0)
            Rn = synth.rodrigues(sr * rng.normal(size=3)) @ R
            Rt[m, j] = np.stack([Rn[:, 0], Rn[:, 1], t + st * rng.normal(size=3)], axis=1)
    return RigInput(W, intr, has, Rt, pu, pv, meta=dict(camR=camR, camt=camt)).normalised()


def stage_tie_rig():
    """Board 5 duplicated as board 6, exact in Rt and pixels; every other board's Rt is perturbed in camera 1 only,
    so their hypotheses carry that error: the pair's hypotheses are bit-identical and the best."""
    inp = stage_rig(12, 54, "none", seed=41, only=0, rt_noise_cams=(1,))
    common = np.nonzero(inp.has[0] & inp.has[1])[0]
    a, b = common[5], common[6]
    camR, camt = inp.meta["camR"], inp.meta["camt"]
    for arr in (inp.Rt, inp.pix_u, inp.pix_v):
        arr[:, b] = arr[:, a]
    # exact pose of board a in both cameras: R_1 = camR_1 R_0, t_1 = camR_1 t_0 + camt_1 (consistent with the rig)
    R0 = inp.Rt[0, a].copy()
    Rf, tf = np_Rt_to_R_t(R0)
    R1 = camR[1] @ Rf
    t1 = camR[1] @ tf + camt[1]
    inp.Rt[1, a] = inp.Rt[1, b] = np.stack([R1[:, 0], R1[:, 1], t1], axis=1)
    # pixels of both cameras: exact projections of that pose (no noise), so the pair is the best hypothesis
    for m, (Rm, tm) in enumerate(((Rf, tf), (R1, t1))):
        u, v = _project(inp.intr[m], inp.worlds @ Rm.T + tm)
        inp.pix_u[m, a] = inp.pix_u[m, b] = u
        inp.pix_v[m, a] = inp.pix_v[m, b] = v
    return dict(inp=inp, first=5, second=6)


def stage_nan_rig():
    """Hypothesis 3's board has r1 = r2 = 0 in camera 1: Rs = 0, ts = t, and with camera 0 at the origin direction 0
    puts every point at the camera centre (P = 0: sqrt(0) * rsq(0) = NaN in the kernel, 0/0 in the oracle)."""
    inp = stage_rig(8, 54, "none", seed=43, only=0)
    common = np.nonzero(inp.has[0] & inp.has[1])[0]
    inp.Rt[1, common[3], :, :2] = 0.0
    return dict(inp=inp, hyp=3)


def stage_refused_rig():
    """Every pixel of both cameras far out: every hypothesis scores >= 1e10."""
    inp = stage_rig(5, 4, "none", seed=47, only=0)
    inp.pix_u += 1e12
    return inp


# The GPU case table: (name, K, n, skew, forced ksplits).  The default partition (ksplit = 0) runs for every row.
STAGE_CASES = [
    ("K1_n54", 1, 54, "none", [1]),
    ("K2_n4", 2, 4, "cur", [1, 2]),
    ("K9_n88", 9, 88, "none", [1, 2, 3, 4, 8, 9]),
    ("K63_n54", 63, 54, "prev", [1, 2, 3, 62, 63]),
    ("K64_n1", 64, 1, "both", [1, 2, 3, 63, 64]),
    ("K65_n54", 65, 54, "none", [1, 2, 3, 64, 65]),
    ("K127_n4", 127, 4, "both", [1, 2, 3, 126, 127]),
    ("K128_n88", 128, 88, "cur", [1, 2, 3, 127, 128]),
    ("K129_n54", 129, 54, "prev", [1, 2, 3, 128, 129]),
    ("K300_n54", 300, 54, "both", [1, 2, 3, 299, 300]),
]

STAGE_POSE_SEED = 1234


def stage_pose(seed=STAGE_POSE_SEED):
    """A pose of camera i-1 away from the identity, so that A = Rp Rs^T mixes every entry."""
    from tscm_calib_amd import synth
    rng = np.random.default_rng(seed)
    return synth.rodrigues(np.array([0.1, -0.2, 0.05])), rng.normal(scale=50.0, size=3)
