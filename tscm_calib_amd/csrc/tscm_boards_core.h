// tscm_boards_core.h -- chessboard structure recovery as ONE definition for host and device: the per-seed job
// (3x3 seed -> energy test -> growth loop), the ordered overlap resolution and the cols >= rows turn.  It follows
// tscm_boards.cpp (chessboardsFromCorners, DetectCorner/chessboard.cpp) operation by operation -- neighbour_towards,
// spread, the energy with its integer-rounded column terms and the `worst < q` update that skips a NaN, the m < np return,
// candidate 0 as the empty marker, the > 0, be < e and < -10 tests, first-wins on every tie -- with ONE documented
// deviation: the extrapolation of three corners is stated without atan2 / cos / sin (extrapolate() below), so that host
// and device take the same decision on every input, exact ties of two distances included.
// The callers differ in how the work of a job is spread (a lane policy); nothing here branches on the caller.  Plain C++17
// on the host (tests/native/boards_core_check.cpp runs it there), __host__ __device__ under hipcc.
#ifndef TSCM_BOARDS_CORE_H
#define TSCM_BOARDS_CORE_H

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define TSCM_BD __host__ __device__ __forceinline__
#define TSCM_BD_UNROLL _Pragma("unroll")      // the seed's nine cells stay in registers only if their loops are unrolled
#else
#define TSCM_BD inline
#define TSCM_BD_UNROLL
#endif
#include <math.h>

// No product is fused with a sum, on either side: a prediction's last bit decides a tie.  (g++ has no such pragma; it fuses
// only where the target has the instruction, which the baseline x86-64 of the host checks has not.)
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace tscm {
namespace boards {

enum { kBlankSeed = 0, kSeedRejected = 1, kGrownRejected = 2, kOffered = 3 };

// Sizes of a job's workspace for an image of n candidates.  A board never holds more than cell_cap(n) cells: its non-zero
// cells are distinct candidates (< n of them), candidate 0 -- never marked as used -- comes at most once per accepted line
// and nine times in the seed, and an accepted line brings at least two new candidates, so there are fewer than n / 2 lines.
// A line longer than line_cap(n), or a board beyond cell_cap(n), is a proposal that "does not suffice" like m < np; neither
// is reachable, the two caps only say how much memory a job may touch.
TSCM_BD int cell_cap(int n) { return 2 * n + 16; }
TSCM_BD int line_cap(int n) { return n / 3 + 8; }

// The workspace of one job.  The device keeps it in LDS, the host in vectors.
struct Work {
    int n;
    const double *xy;            // [2n] x, y of candidate j at 2j, 2j + 1
    unsigned short *board;       // [2][cell_cap] the board and the buffer the next one is written to
    unsigned char *used;         // [n] candidate is a non-zero cell of the board
    unsigned char *taken;        // [4][n] candidate is on the line of proposal s
    int *line;                   // [4][line_cap] the candidates of proposal s's new line, -1 = not assigned yet
    double *pred;                // [4][2 line_cap] where proposal s expects them
    double *energy;              // [4] the proposals' energies
};

struct Record {
    int status, rows, cols, steps;
    double energy;
};

// One thread does everything: side after side, candidate after candidate.
struct SerialLanes {
    static TSCM_BD int lane() { return 0; }
    static TSCM_BD int lanes() { return 1; }
    static TSCM_BD int side() { return 0; }
    static TSCM_BD int sides() { return 1; }
    static TSCM_BD int thread() { return 0; }
    static TSCM_BD int threads() { return 1; }
    static TSCM_BD void sync() {}
    static TSCM_BD void min_pair(double &, unsigned &) {}
    static TSCM_BD double max_of(double q) { return q; }
};
#ifdef __HIPCC__
// A workgroup of four waves: wave s evaluates side s, lanes over candidates and triples.  The reductions run in a fixed
// butterfly, every lane receives the same bits.
struct WaveLanes {
    static __device__ __forceinline__ int lane() { return threadIdx.x & 63; }
    static __device__ __forceinline__ int lanes() { return 64; }
    static __device__ __forceinline__ int side() { return threadIdx.x >> 6; }
    static __device__ __forceinline__ int sides() { return 4; }
    static __device__ __forceinline__ int thread() { return threadIdx.x; }
    static __device__ __forceinline__ int threads() { return 256; }
    static __device__ __forceinline__ void sync() { __syncthreads(); }
    // lexicographic minimum of (d, k): the sequential first minimum in the order of k
    static __device__ __forceinline__ void min_pair(double &d, unsigned &k)
    {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double od = __shfl_xor(d, off);
            const unsigned ok = __shfl_xor(k, off);
            if (od < d || (od == d && ok < k)) { d = od; k = ok; }
        }
    }
    static __device__ __forceinline__ double max_of(double q)
    {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_xor(q, off);
            q = q < o ? o : q;
        }
        return q;
    }
};
#endif

constexpr unsigned kNoKey = 0xffffffffu;
#define TSCM_BOARDS_NEVER __builtin_huge_val()

// distance of candidate j from (x0, y0) in direction v: along v (1e10 when behind) + 5 x across
TSCM_BD double towards(const Work &w, int j, double x0, double y0, double vx, double vy)
{
    const double dx = w.xy[2 * j] - x0, dy = w.xy[2 * j + 1] - y0;
    double along = dx * vx + dy * vy;
    const double ex = dx - along * vx, ey = dy - along * vy;
    const double across = sqrt(ex * ex + ey * ey);
    if (along < 0) along = 1e10;
    return along + 5 * across;
}

// nearest free candidate in direction v from candidate idx: distance along v + 5 x distance across.  Free = not a non-zero
// cell among c[0 .. 9) (the seed under construction), so candidate 0 is always free and always the first.  The sequential
// rule -- the first free candidate opens, a later one wins by d < cost -- as a reduction: the lexicographic minimum of
// (d, j) over the free j, in which a NaN never wins; a NaN of candidate 0 itself stays, as nothing is below it.
template <class P>
TSCM_BD void neighbour_towards(const Work &w, const int c[9], int idx, double vx, double vy, int &who, double &cost)
{
    const double x0 = w.xy[2 * idx], y0 = w.xy[2 * idx + 1];
    double bd = TSCM_BOARDS_NEVER;
    unsigned bk = kNoKey;
    for (int j = P::lane(); j < w.n; j += P::lanes()) {
        bool on = false;
        TSCM_BD_UNROLL
        for (int q = 0; q < 9; ++q) on = on || (j > 0 && c[q] == j);
        if (on) continue;
        const double d = towards(w, j, x0, y0, vx, vy);
        if (d < bd || (d == bd && (unsigned)j < bk)) { bd = d; bk = (unsigned)j; }
    }
    P::min_pair(bd, bk);
    const double d0 = towards(w, 0, x0, y0, vx, vy);
    if (d0 != d0 || bk == kNoKey) { who = 0; cost = d0; return; }
    who = (int)bk; cost = bd;
}

template <int n>
TSCM_BD double spread(const double *a)         // sample standard deviation / mean
{
    double mean = 0;
    TSCM_BD_UNROLL
    for (int i = 0; i < n; ++i) mean += a[i];
    mean /= n;
    double s = 0;
    TSCM_BD_UNROLL
    for (int i = 0; i < n; ++i) s += (a[i] - mean) * (a[i] - mean);
    return sqrt(s / (n - 1)) / mean;
}

// one term of the energy: |p0 + p2 - 2 p1| / |p0 - p2|, on integer-rounded differences for a column triple
TSCM_BD double triple(const Work &w, int i0, int i1, int i2, bool column)
{
    const double x0 = w.xy[2 * i0], y0 = w.xy[2 * i0 + 1], x1 = w.xy[2 * i1], y1 = w.xy[2 * i1 + 1], x2 = w.xy[2 * i2], y2 = w.xy[2 * i2 + 1];
    double ux = x0 + x2 - 2 * x1, uy = y0 + y2 - 2 * y1, wx = x0 - x2, wy = y0 - y2;
    if (column) { ux = rint(ux); uy = rint(uy); wx = rint(wx); wy = rint(wy); }     // lrint and int products: exact in fp64 below 2^53
    return sqrt(ux * ux + uy * uy) / sqrt(wx * wx + wy * wy);
}

// A board of R x Cn cells with one more line on `side` (0 right, 1 bottom, 2 left, 3 top), without copying it; side -1: the
// board itself.
struct View {
    const unsigned short *b;
    const int *line;
    int R, Cn, side;
    TSCM_BD int rows() const { return (side == 1 || side == 3) ? R + 1 : R; }
    TSCM_BD int cols() const { return (side == 0 || side == 2) ? Cn + 1 : Cn; }
    TSCM_BD int at(int r, int k) const
    {
        switch (side) {
        case 0: return k == Cn ? line[r] : b[r * Cn + k];
        case 1: return r == R ? line[k] : b[r * Cn + k];
        case 2: return k == 0 ? line[r] : b[r * Cn + k - 1];
        case 3: return r == 0 ? line[k] : b[(r - 1) * Cn + k];
        default: return b[r * Cn + k];
        }
    }
};

// rows * cols * (max over the triples, from 0 by `worst < q`, - 1); lanes over triples
template <class P>
TSCM_BD double energy(const Work &w, const View &v)
{
    const int R = v.rows(), Cn = v.cols();
    double worst = 0;
    const int nr = R * (Cn - 2), nc = Cn * (R - 2);
    for (int t = P::lane(); t < nr + nc; t += P::lanes()) {
        double q;
        if (t < nr) {
            const int r = t / (Cn - 2), k = t % (Cn - 2);
            q = triple(w, v.at(r, k), v.at(r, k + 1), v.at(r, k + 2), false);
        } else {
            const int u = t - nr, k = u / (R - 2), r = u % (R - 2);
            q = triple(w, v.at(r, k), v.at(r + 1, k), v.at(r + 2, k), true);
        }
        if (worst < q) worst = q;
    }
    worst = P::max_of(worst);
    return R * Cn * (worst - 1);
}

// The documented deviation.  With a = p2 - p1, b = p3 - p2: the direction of b turned once more by the angle between a
// and b, the step 2 |b| - |a|, three quarters of it -- the reference's atan2 / cos / sin geometry without a transcendental.
TSCM_BD void extrapolate(const Work &w, int i1, int i2, int i3, double &px, double &py)
{
    const double ax = w.xy[2 * i2] - w.xy[2 * i1], ay = w.xy[2 * i2 + 1] - w.xy[2 * i1 + 1];
    const double bx = w.xy[2 * i3] - w.xy[2 * i2], by = w.xy[2 * i3 + 1] - w.xy[2 * i2 + 1];
    const double la = sqrt(ax * ax + ay * ay), lb = sqrt(bx * bx + by * by);
    double c1 = 1, s1 = 0, c2 = 1, s2 = 0;                   // a zero vector points along x, as atan2(0, 0) = 0 has it
    if (la != 0) { c1 = ax / la; s1 = ay / la; }
    if (lb != 0) { c2 = bx / lb; s2 = by / lb; }
    const double cc = c2 * c2 - s2 * s2, ss = 2 * c2 * s2;
    const double c3 = cc * c1 + ss * s1, s3 = ss * c1 - cc * s1;
    const double step = 2 * lb - la;
    px = w.xy[2 * i3] + 0.75 * step * c3;
    py = w.xy[2 * i3 + 1] + 0.75 * step * s3;
}

// The job of seed `idx`: fills rec, leaves the board in w.board + return value * cell_cap(n) (rec.rows x rec.cols, row-major; nothing
// for a blank seed).  v1, v2: the seed's two directions.  Every thread of the caller's group runs it with the same arguments;
// every branch that holds a sync() is taken by all of them alike.
template <class P>
TSCM_BD int seed_job(const Work &w, int idx, const double v1[2], const double v2[2], Record &rec)
{
    rec.status = kBlankSeed; rec.rows = rec.cols = rec.steps = 0; rec.energy = 0;
    const int n = w.n, ncap = cell_cap(n), lcap = line_cap(n);
    if (n < 9) return 0;
    // ---- the 3 x 3 seed, in every wave alike (registers only)
    int c[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    double d1[2], d2[6];
    const double ax = v1[0], ay = v1[1], bx = v2[0], by = v2[1];
    c[4] = idx;
    int who;
    neighbour_towards<P>(w, c, idx, ax, ay, who, d1[0]); c[5] = who;
    neighbour_towards<P>(w, c, idx, -ax, -ay, who, d1[1]); c[3] = who;
    neighbour_towards<P>(w, c, idx, bx, by, who, d2[0]); c[7] = who;
    neighbour_towards<P>(w, c, idx, -bx, -by, who, d2[1]); c[1] = who;
    neighbour_towards<P>(w, c, c[3], -bx, -by, who, d2[2]); c[0] = who;
    neighbour_towards<P>(w, c, c[3], bx, by, who, d2[3]); c[6] = who;
    neighbour_towards<P>(w, c, c[5], -bx, -by, who, d2[4]); c[2] = who;
    neighbour_towards<P>(w, c, c[5], bx, by, who, d2[5]); c[8] = who;
    if (spread<2>(d1) > 0.3 || spread<6>(d2) > 0.3) return 0;
    if (c[0] == 0 && c[1] == 0) return 0;                                   // the reference's "zero board" test
    double e;
    {
        double worst = 0;
        TSCM_BD_UNROLL
        for (int r = 0; r < 3; ++r) { const double q = triple(w, c[3 * r], c[3 * r + 1], c[3 * r + 2], false); if (worst < q) worst = q; }
        TSCM_BD_UNROLL
        for (int k = 0; k < 3; ++k) { const double q = triple(w, c[k], c[3 + k], c[6 + k], true); if (worst < q) worst = q; }
        e = 9 * (worst - 1);
    }
    int cur = 0, R = 3, Cn = 3;
    TSCM_BD_UNROLL
    for (int t = 0; t < 9; ++t) w.board[t] = (unsigned short)c[t];                // the same cells from every thread
    rec.rows = rec.cols = 3; rec.energy = e;
    if (e > 0) { rec.status = kSeedRejected; return 0; }
    for (int j = P::thread(); j < n; j += P::threads()) {
        w.used[j] = 0;
        for (int s = 0; s < 4; ++s) w.taken[s * n + j] = 0;
    }
    P::sync();
    int m = n;                                                               // free candidates; candidate 0 stays free
    TSCM_BD_UNROLL
    for (int q = 0; q < 9; ++q) {
        bool fresh = c[q] > 0;
        TSCM_BD_UNROLL
        for (int p = 0; p < q; ++p) fresh = fresh && c[p] != c[q];
        if (fresh) { --m; w.used[c[q]] = 1; }                                // the same byte from every thread
    }
    P::sync();
    // ---- growth: the side that lowers the energy most, while one does.  At most n steps, never reached (see cell_cap).
    int steps = 0;
    for (; steps < n; ++steps) {
        const unsigned short *b = w.board + cur * ncap;
        const bool blank = b[0] == 0 && b[1] == 0;
        // A: where each side expects its line
        for (int s = P::side(); s < 4; s += P::sides()) {
            const int np = (s == 0 || s == 2) ? R : Cn;
            const bool can = !blank && m >= np && np <= lcap && (R * Cn + np) <= ncap;
            if (!can) continue;
            int *line = w.line + s * lcap;
            double *pred = w.pred + 2 * s * lcap;
            for (int i = P::lane(); i < np; i += P::lanes()) {
                line[i] = -1;
                switch (s) {
                case 0: extrapolate(w, b[i * Cn + Cn - 3], b[i * Cn + Cn - 2], b[i * Cn + Cn - 1], pred[2 * i], pred[2 * i + 1]); break;
                case 1: extrapolate(w, b[(R - 3) * Cn + i], b[(R - 2) * Cn + i], b[(R - 1) * Cn + i], pred[2 * i], pred[2 * i + 1]); break;
                case 2: extrapolate(w, b[i * Cn + 2], b[i * Cn + 1], b[i * Cn], pred[2 * i], pred[2 * i + 1]); break;
                default: extrapolate(w, b[2 * Cn + i], b[Cn + i], b[i], pred[2 * i], pred[2 * i + 1]); break;
                }
            }
        }
        P::sync();
        // B: greedy assignment -- np times the closest (free candidate, open prediction) pair, the first one in candidate-major
        // order -- and the energy of the proposal.  A lane reads only what it wrote itself (every lane of the wave writes the
        // same pick) or what stood before the sync.
        for (int s = P::side(); s < 4; s += P::sides()) {
            const int np = (s == 0 || s == 2) ? R : Cn;
            bool can = !blank && m >= np && np <= lcap && (R * Cn + np) <= ncap;
            int *line = w.line + s * lcap;
            const double *pred = w.pred + 2 * s * lcap;
            unsigned char *taken = w.taken + s * n;
            double ge = e;
            if (can) {
                for (int it = 0; it < np; ++it) {
                    double bd = TSCM_BOARDS_NEVER;
                    unsigned bk = kNoKey;
                    for (int j = P::lane(); j < n; j += P::lanes()) {
                        if (w.used[j] || taken[j]) continue;
                        const double xj = w.xy[2 * j], yj = w.xy[2 * j + 1];
                        for (int i = 0; i < np; ++i) {
                            if (line[i] >= 0) continue;
                            const double dx = xj - pred[2 * i], dy = yj - pred[2 * i + 1];
                            const double d = sqrt(dx * dx + dy * dy);
                            if (d < bd) { bd = d; bk = (unsigned)j * (unsigned)np + (unsigned)i; }
                        }
                    }
                    P::min_pair(bd, bk);
                    if (bk == kNoKey) { can = false; break; }                // no finite distance left: not with checked input
                    const int bj = (int)(bk / (unsigned)np), bi = (int)(bk % (unsigned)np);
                    line[bi] = bj;
                    taken[bj] = 1;
                }
                if (can) {
                    const View v = { b, line, R, Cn, s };
                    ge = energy<P>(w, v);
                }
                for (int i = 0; i < np; ++i) if (line[i] >= 0) taken[line[i]] = 0;
            }
            w.energy[s] = ge;
        }
        P::sync();
        // C: one comparison, sides in the order 0..3 with strict <
        double be = w.energy[0];
        int best = 0;
        for (int s = 1; s < 4; ++s) if (w.energy[s] < be) { be = w.energy[s]; best = s; }
        if (!(be < e)) break;
        const int *line = w.line + best * lcap;
        const View v = { b, line, R, Cn, best };
        const int nR = v.rows(), nC = v.cols(), np = (best == 0 || best == 2) ? R : Cn;
        unsigned short *nb = w.board + (cur ^ 1) * ncap;
        for (int t = P::thread(); t < nR * nC; t += P::threads()) nb[t] = (unsigned short)v.at(t / nC, t % nC);
        for (int i = 0; i < np; ++i) if (line[i] > 0) --m;
        for (int i = P::thread(); i < np; i += P::threads()) if (line[i] > 0) w.used[line[i]] = 1;
        R = nR; Cn = nC; e = be; cur ^= 1;
        P::sync();
    }
    rec.rows = R; rec.cols = Cn; rec.steps = steps; rec.energy = e;
    rec.status = e < -10 ? kOffered : kGrownRejected;
    return cur;
}

// ---- what follows the jobs, on one thread, over the records of an image in seed order

// Overlap resolution: an offered board that shares a cell value (candidate 0 included) with a kept one replaces every
// such board of higher energy and is kept if it replaced one or overlapped none.  keep[0 .. return) = the kept seeds,
// ascending; mark: n zeroed bytes of scratch, zero again on return.
inline int resolve_overlaps(int n, const Record *rec, const int *offset, const int *cells, unsigned char *mark, int *keep)
{
    int nk = 0;
    for (int i = 0; i < n; ++i) {
        if (rec[i].status != kOffered) continue;
        const int len = rec[i].rows * rec[i].cols;
        for (int q = 0; q < len; ++q) mark[cells[offset[i] + q]] = 1;
        bool overlapped = false, replaced = false;
        int out = 0;
        for (int k = 0; k < nk; ++k) {
            const int o = keep[k], olen = rec[o].rows * rec[o].cols;
            bool shared = false;
            for (int q = 0; q < olen && !shared; ++q) shared = mark[cells[offset[o] + q]] != 0;
            bool drop = false;
            if (shared) {
                overlapped = true;
                if (rec[o].energy > rec[i].energy) { drop = true; replaced = true; }
            }
            if (!drop) keep[out++] = o;
        }
        nk = out;
        if (!overlapped || replaced) keep[nk++] = i;
        for (int q = 0; q < len; ++q) mark[cells[offset[i] + q]] = 0;
    }
    return nk;
}

// at least as many columns as rows: out (rows_out x cols_out) from b (rows x cols)
inline void turned(int rows, int cols, const int *b, int &rows_out, int &cols_out, int *out)
{
    if (cols >= rows) {
        rows_out = rows; cols_out = cols;
        for (int q = 0; q < rows * cols; ++q) out[q] = b[q];
        return;
    }
    rows_out = cols; cols_out = rows;
    for (int j = 0; j < rows_out; ++j)
        for (int k = 0; k < cols_out; ++k) out[j * cols_out + k] = b[(rows - k - 1) * cols + j];
}

}  // namespace boards
}  // namespace tscm

#endif
