// tscm_geometry.h -- stage 1, shared by the Gram kernels: a corner's projection, residual and Jacobian entries, the robust
// loss, and the epilogue that turns a view's accumulator tiles into its record.
#pragma once
// (included inside namespace tscm: from tscm_kernels.h, and from tscm_mono_batch.hip)

// tile column -> (parity mask) bookkeeping shared by the hot kernel's epilogue and k_finalize_eval.
//   f*   = -X/k on u-rows, -Y/k on v-rows : fx is its u-half, fy its v-half
//   one* = -1 on every row                 : cx is its u-half, cy its v-half
// so with separate Gram tiles for the u-rows (GU) and the v-rows (GV) the true products are
//   <a, b> = sum over parities in mask(a) & mask(b) of G_par[tile(a)][tile(b)].
// F index (record / H layout): 0-2 w_c, 3-5 t_c, 6 fx, 7 fy, 8 cx, 9 cy, 10 xi, 11 lambda, 12 alpha, 13 r.
__host__ __device__ __forceinline__ constexpr int f_tile(int f)
{
    return f < 3 ? kTcWc + f : f < 6 ? tc_tc(f - 3) : f < 8 ? kTcF : f < 10 ? kTcOne : f == 10 ? kTcXi : f == 11 ? kTcLam : f == 12 ? kTcAl : kTcR;
}
__device__ __forceinline__ int f_mask(int f) { return (f >= 6 && f < 10) ? (1 << ((f - 6) & 1)) : 3; }

// ---------------------------------------------------------------------------------------------
// Epilogue of the Gram kernels (fp64 and fp32-Jacobian variant): one view's two accumulator tiles (u-rows, v-rows)
// -> its record, entirely in the lane's own registers.
// D layout: lane (col, kq) holds rows kq + 4*reg of tile column col (see the tile-column table above):
//   lanes kq < 3   register 0 = w_b row kq of their column              -> record row kq
//   lanes kq == 3  registers 0, 1, 2 = the t_c rows of their column     -> t_b row l = sum_j R_c[j][l] * (t_c row j),
//                  record rows 3, 4, 5 (row 3 leaves with the w_b rows in one store, rows 4 | 5 as one 16-byte store)
// The columns f* and one* store their u-row part (fx, cx) and next to it the v-row part = total - u-part (fy, cy).
// The record is column-major, so a lane's entries are adjacent: FOUR stores per view (13 in round 2, with 20
// ds_bpermute, three vector loads of R_c and ~90 integer instructions of offset arithmetic around them); lanes without
// an entry store past the end of the buffer, which the bounds check drops.  Neither the t_b x t_b block of E^T E
// (consumers derive it: tb_tb) nor its never-read upper triangle nor copies of E^T r / the diagonal are written.
// ---------------------------------------------------------------------------------------------
typedef const double __attribute__((address_space(4))) *cptr4;

// lane-constant part of the record addressing, computed once per kernel: byte offset of the lane's row-kq entry inside
// the allocation for slot 0 (region base included) and the byte stride per slot of its region
struct RecLane { unsigned off, stride, goff, gstride; };
__device__ __forceinline__ RecLane rec_lane(int lane, unsigned V)
{
    const int col = lane & 15, kq = lane >> 4;
    RecLane r;
    // the gradient column once more in the compact G region: row kq (kq < 3) / rows 3 | 4 5 (kq == 3) of the view's six
    r.goff = col == kTcR ? 8u * ((unsigned)(kRecW + kRecE) * V + (unsigned)kq) : 0xffffe000u; r.gstride = col == kTcR ? 8u * kRecG : 0u;
    if (col < 3) { r.off = 8u * ((unsigned)kRecW * V + 6u * (unsigned)col + (unsigned)kq); r.stride = 8u * kRecE; }
    else if (col == 15) { r.off = 0xffffe000u; r.stride = 0u; }
    else {
        // tile column -> F index (W column); f* and one* are the first of a (u-part, v-part) column pair
        const int f = (col & 3) == 3 ? kWcolTc + (col >> 2) : col < 8 ? col - kTcWc : col == kTcF ? 6 : col == kTcOne ? 8 : col == kTcXi ? 10 : col - 1;
        r.off = 8u * (6u * (unsigned)f + (unsigned)kq); r.stride = 8u * kRecW;
    }
    return r;
}

// t_b x t_b entry (l, lp) of one view's E^T E from the t_c columns of its W record (column-major) and the rotation of
// the camera it was evaluated with -- the SAME three operations, in the same order, the Gram kernel's epilogue used
// when it still stored the block: the values are bit-identical.
template <typename PW, typename PR>
__host__ __device__ __forceinline__ double tb_tb(PW W, PR Rc, int l, int lp)
{
    double t = Rc[3 + lp] * W[6 * (kWcolTc + 1) + 3 + l];
    t = fma(Rc[lp], W[6 * kWcolTc + 3 + l], t);
    return fma(Rc[6 + lp], W[6 * (kWcolTc + 2) + 3 + l], t);
}

__device__ __forceinline__ void store_view_record(__amdgpu_buffer_rsrc_t r_rec, int lane, const d4 &accU, const d4 &accV, cptr4 cc, unsigned slot, RecLane rl)
{
    int le = lane;
    asm volatile("" : "+v"(le));             // the lane predicates are rebuilt per view (a compare each) instead of living in SGPR pairs
    const int col = le & 15;
    const bool k3 = le >= 48, split = col == kTcF || col == kTcOne;
    constexpr unsigned BAD = 0xffffe000u;
    const unsigned off = rl.off + __umul24(slot, rl.stride);
    const double t0 = accU[0] + accV[0], t1 = accU[1] + accV[1], t2 = accU[2] + accV[2];
    // t_b rows l = 0, 1, 2 (of use in the lanes kq == 3): u+v and the u-row part
    double tbT[3], tbU[3];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        tbT[l] = fma(cc[6 + l], t2, fma(cc[l], t0, cc[3 + l] * t1));
        tbU[l] = fma(cc[6 + l], accU[2], fma(cc[l], accU[0], cc[3 + l] * accU[1]));
    }
    const double selT = k3 ? tbT[0] : t0, selU = k3 ? tbU[0] : accU[0];      // record row kq (kq < 3) / row 3 (kq == 3)
    buf_store_f64(r_rec, off, 0u, split ? selU : selT);
    buf_store_2f64(r_rec, (k3 ? off : BAD) + 8u, split ? tbU[1] : tbT[1], split ? tbU[2] : tbT[2]);
    // ... and the v-row parts of f* / one* in the next record column
    buf_store_f64(r_rec, (split ? off : BAD) + 48u, 0u, selT - selU);
    buf_store_2f64(r_rec, (split && k3 ? off : BAD) + 56u, tbT[1] - tbU[1], tbT[2] - tbU[2]);
    const unsigned og = rl.goff + __umul24(slot, rl.gstride);
    buf_store_f64(r_rec, og, 0u, selT);
    buf_store_2f64(r_rec, (k3 ? og : BAD) + 8u, tbT[1], tbT[2]);
}

// ---------------------------------------------------------------------------------------------
// Geometry of one corner for the Gram kernels: board point (x, y, 0) -> camera frame -> Triple Sphere projection,
// residual, and the 15 Jacobian entries of the u-row and of the v-row (multi_calib.h:146-195, hand-derived: tscm_math.h).
// VC(k): the view's constants (kVConst), CC(k): the camera's (kCConst), both wave-uniform (scalar operands);
// PUT(column, u, v) receives the entries by SEMANTIC column (GCol) -- each kernel has its own tile column order.
//   * P_c = x m1 + y m2 + t as two FMAs per component (round 3; rounds 1-2: board -> world -> camera, 21 operations);
//   * camera-rotation columns: n . (a_k x Q') = a_k . (Q' x n) with Q' = P_c - t_c (camera_rotation_constants):
//     one cross product per row and three dot products (33 operations; 45 with three matrix-vector products).
// ---------------------------------------------------------------------------------------------
enum GCol { gcWb0 = 0, gcWb1, gcWb2, gcTc0, gcTc1, gcTc2, gcWc0, gcWc1, gcWc2, gcF, gcOne, gcXi, gcLam, gcAl, gcR };

// WC = false (k_eval_gram4's path for a camera whose pose is held constant): the camera-rotation columns gcWc0..2 are neither
// computed nor handed out; every other entry comes from the same operations in the same order.
// PIN_WB (k_eval_gram4's WEIGHTED instantiation): the w_b entries with their FMAs written out, in the pairing the compiler
// gives the expressions below in the plain instantiation of k_eval_gram4 on both of its paths (read from its gfx950 code:
// h = fma(x, a, y b); u-row fma(n02, h2, fma(n01, h1, n00 h0)); v-row fma(n12, h2, fma(n10, h0, n11 h1))) -- left to itself the
// compiler pairs them differently next to corner_residual, and all-ones weights would miss the plain solve's last bits.
// This is a hand copy of one compiler version's choice: tests/test_gpu_weights.py::test_unit_weights_are_the_plain_gram is its
// guard.  When it trips after a compiler change, read the plain k_eval_gram4<14, false, false>'s pairing again (DESIGN 27 says how)
// and restate it here -- or write the unpinned branch with the same explicit fma and refresh tools/regress_bits.expected.
template <bool WC = true, bool PIN_WB = false, typename FV, typename FC, typename FP>
__device__ __forceinline__ void corner_geometry(double x, double y, double ou, double ov, FV VC, FC CC, FP PUT)
{
    const double X = fma(x, VC(0), fma(y, VC(3), VC(6)));
    const double Y = fma(x, VC(1), fma(y, VC(4), VC(7)));
    const double Z = fma(x, VC(2), fma(y, VC(5), VC(8)));
    const double fx = CC(39), fy = CC(40), xi = CC(43), lam = CC(44), beta = CC(45);
    // triple sphere (multi_calib.h:170-178)
    const double rho2 = X * X + Y * Y;
    double d1, id1, d2, id2, d3, id3;
    sqrt_and_inverse(rho2 + Z * Z, d1, id1);
    const double z1 = Z + xi * d1;
    sqrt_and_inverse(rho2 + z1 * z1, d2, id2);
    const double z2 = z1 + lam * d2;
    sqrt_and_inverse(rho2 + z2 * z2, d3, id3);
    const double k = z2 + beta * d3;
    const double ik = fast_rcp(k);
    const double mx = X * ik, my = Y * ik;
    const double c1 = 1.0 + xi * Z * id1;
    const double c2 = 1.0 + lam * z1 * id2;
    const double c3 = 1.0 + beta * z2 * id3;
    const double q = beta * id3 + c3 * (lam * id2 + c2 * xi * id1);
    const double kz = c1 * c2 * c3;
    const double fxk = fx * ik, fyk = fy * ik;
    // -A = -d(u,v)/dPc  (the t_c columns)
    const double n00 = -fxk * (1.0 - X * mx * q), n01 = fxk * mx * Y * q, n02 = fxk * mx * kz;
    const double n10 = fyk * my * X * q, n11 = -fyk * (1.0 - Y * my * q), n12 = fyk * my * kz;
    PUT(gcTc0, n00, n10);
    PUT(gcTc1, n01, n11);
    PUT(gcTc2, n02, n12);
    // w_b: -A (x e_k0 + y e_k1),  e = R_c dR_b/dw_k columns
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) {
        if constexpr (PIN_WB) {
            const double h0 = fma(x, VC(9 + 6 * kk), y * VC(12 + 6 * kk));
            const double h1 = fma(x, VC(10 + 6 * kk), y * VC(13 + 6 * kk));
            const double h2 = fma(x, VC(11 + 6 * kk), y * VC(14 + 6 * kk));
            PUT(gcWb0 + kk, fma(n02, h2, fma(n01, h1, n00 * h0)), fma(n12, h2, fma(n10, h0, n11 * h1)));
        } else {
            const double h0 = x * VC(9 + 6 * kk) + y * VC(12 + 6 * kk);
            const double h1 = x * VC(10 + 6 * kk) + y * VC(13 + 6 * kk);
            const double h2 = x * VC(11 + 6 * kk) + y * VC(14 + 6 * kk);
            PUT(gcWb0 + kk, n00 * h0 + n01 * h1 + n02 * h2, n10 * h0 + n11 * h1 + n12 * h2);
        }
    }
    // w_c: -A (dR_c/dw_k P_w) = a_k . (Q' x n)
    if constexpr (WC) {
        double Q0 = X - CC(9), Q1 = Y - CC(10), Q2 = Z - CC(11);
        if (CC(24) != 0.0) {                  // small-angle branch of the camera rotation (wave-uniform): Q' = Q - w x Q
            const double w0 = CC(21), w1 = CC(22), w2 = CC(23);
            const double s0 = w1 * Q2 - w2 * Q1, s1 = w2 * Q0 - w0 * Q2, s2 = w0 * Q1 - w1 * Q0;
            Q0 -= s0; Q1 -= s1; Q2 -= s2;
        }
        const double cu0 = Q1 * n02 - Q2 * n01, cu1 = Q2 * n00 - Q0 * n02, cu2 = Q0 * n01 - Q1 * n00;
        const double cv0 = Q1 * n12 - Q2 * n11, cv1 = Q2 * n10 - Q0 * n12, cv2 = Q0 * n11 - Q1 * n10;
#pragma unroll
        for (int kk = 0; kk < 3; ++kk)
            PUT(gcWc0 + kk, CC(12 + 3 * kk) * cu0 + CC(13 + 3 * kk) * cu1 + CC(14 + 3 * kk) * cu2,
                            CC(12 + 3 * kk) * cv0 + CC(13 + 3 * kk) * cv1 + CC(14 + 3 * kk) * cv2);
    }
    // f* and one*
    PUT(gcF, -mx, -my);
    PUT(gcOne, -1.0, -1.0);
    // xi, lambda, alpha: -du/dk * dk/dparam
    const double hu = fxk * mx, hv = fyk * my;
    const double kxi = c3 * c2 * d1, klam = c3 * d2, kal = d3 * CC(46);
    PUT(gcXi, hu * kxi, hv * kxi);
    PUT(gcLam, hu * klam, hv * klam);
    PUT(gcAl, hu * kal, hv * kal);
    // residual = observed - projected (multi_calib.h:192-193)
    PUT(gcR, ou - (fx * mx + CC(41)), ov - (fy * my + CC(42)));
}

// the residual of corner_geometry alone, in its operation order (the robust Gram kernels weight a corner's entries by
// sqrt(rho'(|r|^2)) as corner_geometry hands them out, instead of holding all 30 until the residual, its last output, is
// known: that held 60 registers more and spilled)
template <typename FV, typename FC>
__device__ __forceinline__ void corner_residual(double x, double y, double ou, double ov, FV VC, FC CC, double &ru, double &rv)
{
    const double X = fma(x, VC(0), fma(y, VC(3), VC(6)));
    const double Y = fma(x, VC(1), fma(y, VC(4), VC(7)));
    const double Z = fma(x, VC(2), fma(y, VC(5), VC(8)));
    const double xi = CC(43), lam = CC(44), beta = CC(45);
    const double rho2 = X * X + Y * Y;
    double d1, id1, d2, id2, d3, id3;
    sqrt_and_inverse(rho2 + Z * Z, d1, id1);
    const double z1 = Z + xi * d1;
    sqrt_and_inverse(rho2 + z1 * z1, d2, id2);
    const double z2 = z1 + lam * d2;
    sqrt_and_inverse(rho2 + z2 * z2, d3, id3);
    const double k = z2 + beta * d3;
    const double ik = fast_rcp(k);
    const double mx = X * ik, my = Y * ik;
    ru = ou - (CC(39) * mx + CC(41));
    rv = ov - (CC(40) * my + CC(42));
}

// Robust loss of a residual block (one corner, s = r_u^2 + r_v^2): Ceres' HuberLoss, SoftLOneLoss, CauchyLoss
// (loss_function.cc), same operations.  a: scale in pixels, b = a^2, c = 1 / b (all three computed on the host, as Ceres'
// constructors do).  Every one of them has rho'' <= 0, so Ceres' Corrector takes its alpha = 0 branch: the residuals and the
// Jacobian rows of the block are both scaled by sqrt(rho'), and no rank-one term appears.  The robust Gram-kernel
// instantiations get these values as a kernel argument (wave-uniform: scalar registers).
enum { kLossNone = 0, kLossHuber = 1, kLossSoftL1 = 2, kLossCauchy = 3 };
// (struct LossArg { a, b, c, kind }: tscm_spec.h, with the host code that fills it)
// rho(s) and w = sqrt(rho'(s)), rho' clamped from below as Ceres clamps it (std::numeric_limits<double>::min()).
// WEIGHTED (corner weights, DESIGN 27: Ceres' ScaledLoss): the corner's weight omega >= 0 scales both, rho = omega rho(s) and
// w = sqrt(omega rho'(s)) -- the product formed behind the clamp and before the one sqrt, so omega = 0 gives w = 0 exactly --
// and kind kLossNone is rho(s) = s, rho' = 1 (weights without a loss).  The instantiations without weights never see that kind.
template <bool WEIGHTED = false>
__device__ __forceinline__ void robust_rho(const LossArg &L, double s, double &rho, double &w, double omega = 1.0)
{
    constexpr double kMin = 2.2250738585072014e-308;
    double r1;
    if (WEIGHTED && L.kind == kLossNone) {
        rho = s; r1 = 1.0;
    } else if (L.kind == kLossHuber) {
        if (s > L.b) { const double r = sqrt(s); rho = 2.0 * L.a * r - L.b; r1 = fmax(kMin, L.a / r); }
        else { rho = s; r1 = 1.0; }
    } else if (L.kind == kLossSoftL1) {
        const double sum = 1.0 + s * L.c, tmp = sqrt(sum);
        rho = 2.0 * L.b * (tmp - 1.0); r1 = fmax(kMin, 1.0 / tmp);
    } else {
        const double sum = 1.0 + s * L.c, inv = 1.0 / sum;
        rho = L.b * log(sum); r1 = fmax(kMin, inv);
    }
    if constexpr (WEIGHTED) { rho *= omega; r1 *= omega; }
    w = sqrt(r1);
}
