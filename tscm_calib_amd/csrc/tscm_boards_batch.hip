// tscm_boards_batch.hip -- chessboard structure recovery for a batch of images, one job per (image, seed candidate), on the
// device (k_board_seeds) or on the host, from the one definition of tscm_boards_core.h.  The jobs of a batch are
// independent; the overlap resolution that walks an image's seeds in order runs on the host over the jobs' records, after one
// copy back.  tscm_chessboards_from_corners (tscm_boards.cpp) is a different function with its own bits and stays as it is.
#include "tscm_boards_core.h"
#include "tscm_host.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

using namespace tscm;
namespace bd = tscm::boards;

struct BoardImage {
    long long cand;         // first candidate of the image in the flat lists
    long long cells;        // first cell of the image's jobs in the cell output, cell_cap(n) per job
    int n, first_job;
};

// Bytes of a job's workspace for n candidates, in the order k_board_seeds carves it: doubles, ints, shorts, bytes.
size_t work_bytes(int n)
{
    const size_t lc = (size_t)bd::line_cap(n), cc = (size_t)bd::cell_cap(n);
    return sizeof(double) * (2 * (size_t)n + 8 * lc + 4) + sizeof(int) * 4 * lc + sizeof(unsigned short) * 2 * cc + 5 * (size_t)n;
}

// One workgroup of four waves per job; wave s evaluates side s of a growth step (bd::WaveLanes).  No atomics, no
// floating-point sum: two launches write the same bytes.
__global__ __launch_bounds__(256) void k_board_seeds(const BoardImage *__restrict__ images, const int *__restrict__ job_image, const double *__restrict__ xy,
                                                     const double *__restrict__ v1, const double *__restrict__ v2, int *__restrict__ rec4,
                                                     double *__restrict__ energy, unsigned short *__restrict__ cells)
{
    extern __shared__ double smem[];
    const int job = blockIdx.x;
    const BoardImage im = images[job_image[job]];
    const int n = im.n, seed = job - im.first_job, lc = bd::line_cap(n), cc = bd::cell_cap(n);
    double *s_xy = smem, *s_pred = s_xy + 2 * n, *s_energy = s_pred + 8 * lc;
    int *s_line = reinterpret_cast<int *>(s_energy + 4);
    unsigned short *s_board = reinterpret_cast<unsigned short *>(s_line + 4 * lc);
    unsigned char *s_used = reinterpret_cast<unsigned char *>(s_board + 2 * cc);
    for (int t = threadIdx.x; t < 2 * n; t += 256) s_xy[t] = xy[2 * im.cand + t];
    __syncthreads();
    const bd::Work w = { n, s_xy, s_board, s_used, s_used + n, s_line, s_pred, s_energy };
    bd::Record rec;
    const int cur = bd::seed_job<bd::WaveLanes>(w, seed, v1 + 2 * (im.cand + seed), v2 + 2 * (im.cand + seed), rec);
    __syncthreads();
    if (threadIdx.x == 0) {
        rec4[4 * job] = rec.status; rec4[4 * job + 1] = rec.rows; rec4[4 * job + 2] = rec.cols; rec4[4 * job + 3] = rec.steps;
        energy[job] = rec.energy;
    }
    unsigned short *out = cells + im.cells + (long long)seed * cc;
    for (int t = threadIdx.x; t < rec.rows * rec.cols; t += 256) out[t] = s_board[cur * cc + t];
}

// the jobs of one image, in seed order
struct ImageJobs {
    std::vector<bd::Record> rec;
    std::vector<int> offset, cells;
    bool on_device = false;
};

thread_local double g_kernel_seconds = 0.0;

int invalid(const std::string &msg) { return tscm_set_error(TSCM_E_INVALID, msg); }

int check_args(int n_images, const tscm_corner_candidates *cands, int where, const void *out)
{
    if (!out) return invalid("out is NULL");
    if (n_images < 0) return invalid("n_images " + std::to_string(n_images) + " is negative");
    if (n_images > 0 && !cands) return invalid("cands is NULL");
    if (where != TSCM_BOARDS_HOST && where != TSCM_BOARDS_DEVICE) return invalid("where " + std::to_string(where) + " is neither TSCM_BOARDS_HOST nor TSCM_BOARDS_DEVICE");
    for (int k = 0; k < n_images; ++k) {
        const tscm_corner_candidates &c = cands[k];
        const std::string at = "cands[" + std::to_string(k) + "]: ";
        if (c.n < 0) return invalid(at + "n " + std::to_string(c.n) + " is negative");
        if (c.n > 0 && (!c.x || !c.y || !c.v1 || !c.v2)) return invalid(at + "x, y, v1 or v2 is NULL");
        if (c.n > 65535) return tscm_set_error(TSCM_E_UNSUPPORTED, at + "more than 65535 candidates (the reference stores the indices as uint16)");
        for (int j = 0; j < c.n; ++j)
            if (!(std::fabs(c.x[j]) <= 32767.0) || !(std::fabs(c.y[j]) <= 32767.0))
                return invalid(at + "coordinate " + std::to_string(j) + " is not finite or beyond 32767 in magnitude");
    }
    return 0;
}

void run_host(const tscm_corner_candidates &c, ImageJobs &jobs)
{
    const int n = c.n, lc = bd::line_cap(n), cc = bd::cell_cap(n);
    jobs.rec.assign((size_t)n, bd::Record{ 0, 0, 0, 0, 0.0 });
    jobs.offset.assign((size_t)n + 1, 0);
    jobs.cells.clear();
    if (n < 9) return;
    std::vector<double> xy(2 * (size_t)n), pred(8 * (size_t)lc), energy(4);
    std::vector<int> line(4 * (size_t)lc);
    std::vector<unsigned short> board(2 * (size_t)cc);
    std::vector<unsigned char> flags(5 * (size_t)n);
    for (int j = 0; j < n; ++j) { xy[2 * (size_t)j] = c.x[j]; xy[2 * (size_t)j + 1] = c.y[j]; }
    const bd::Work w = { n, xy.data(), board.data(), flags.data(), flags.data() + n, line.data(), pred.data(), energy.data() };
    for (int i = 0; i < n; ++i) {
        const int cur = bd::seed_job<bd::SerialLanes>(w, i, c.v1 + 2 * (size_t)i, c.v2 + 2 * (size_t)i, jobs.rec[i]);
        const int len = jobs.rec[i].rows * jobs.rec[i].cols;
        for (int q = 0; q < len; ++q) jobs.cells.push_back(board[(size_t)cur * cc + q]);
        jobs.offset[(size_t)i + 1] = (int)jobs.cells.size();
    }
}

// the images `which` of the batch (9 <= n <= TSCM_BOARDS_MAX_DEVICE_CANDIDATES each) in one launch
int run_device(const tscm_corner_candidates *cands, const std::vector<int> &which, std::vector<ImageJobs> &jobs)
{
    g_kernel_seconds = 0.0;
    if (which.empty()) return 0;
    std::vector<BoardImage> images;
    std::vector<int> job_image;
    std::vector<double> xy, v1, v2;
    long long cand = 0, cells = 0;
    int n_max = 0;
    for (int k : which) {
        const tscm_corner_candidates &c = cands[k];
        images.push_back(BoardImage{ cand, cells, c.n, (int)job_image.size() });
        job_image.insert(job_image.end(), (size_t)c.n, (int)images.size() - 1);
        for (int j = 0; j < c.n; ++j) { xy.push_back(c.x[j]); xy.push_back(c.y[j]); }
        v1.insert(v1.end(), c.v1, c.v1 + 2 * (size_t)c.n);
        v2.insert(v2.end(), c.v2, c.v2 + 2 * (size_t)c.n);
        cand += c.n;
        cells += (long long)c.n * bd::cell_cap(c.n);
        n_max = std::max(n_max, c.n);
    }
    const size_t S = job_image.size();
    DeviceMem mem;
    EventSpan span;
    const BoardImage *d_images = nullptr;
    const int *d_job_image = nullptr;
    const double *d_xy = nullptr, *d_v1 = nullptr, *d_v2 = nullptr;
    int *d_rec = nullptr;
    double *d_energy = nullptr;
    unsigned short *d_cells = nullptr;
    HIP_TRY(mem.upload(&d_images, images));
    HIP_TRY(mem.upload(&d_job_image, job_image));
    HIP_TRY(mem.upload(&d_xy, xy));
    HIP_TRY(mem.upload(&d_v1, v1));
    HIP_TRY(mem.upload(&d_v2, v2));
    HIP_TRY(mem.alloc(&d_rec, 4 * S));
    HIP_TRY(mem.alloc(&d_energy, S));
    HIP_TRY(mem.alloc(&d_cells, (size_t)cells));
    HIP_TRY(span.create(2));
    HIP_TRY(span.mark(0));
    hipLaunchKernelGGL(k_board_seeds, dim3((unsigned)S), dim3(256), work_bytes(n_max), 0, d_images, d_job_image, d_xy, d_v1, d_v2, d_rec, d_energy, d_cells);
    HIP_TRY(span.finish(1, nullptr, &g_kernel_seconds));
    std::vector<int> rec(4 * S);
    std::vector<double> energy(S);
    std::vector<unsigned short> cell((size_t)cells);
    HIP_TRY(hipMemcpy(rec.data(), d_rec, sizeof(int) * rec.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(energy.data(), d_energy, sizeof(double) * S, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cell.data(), d_cells, sizeof(unsigned short) * cell.size(), hipMemcpyDeviceToHost));
    for (size_t q = 0; q < which.size(); ++q) {
        const BoardImage &im = images[q];
        ImageJobs &J = jobs[(size_t)which[q]];
        J.on_device = true;
        J.rec.resize((size_t)im.n);
        J.offset.assign((size_t)im.n + 1, 0);
        J.cells.clear();
        for (int i = 0; i < im.n; ++i) {
            const size_t job = (size_t)im.first_job + i;
            J.rec[i] = bd::Record{ rec[4 * job], rec[4 * job + 1], rec[4 * job + 2], rec[4 * job + 3], energy[job] };
            const unsigned short *src = cell.data() + im.cells + (long long)i * bd::cell_cap(im.n);
            const int len = J.rec[i].rows * J.rec[i].cols;
            if (len < 0 || len > bd::cell_cap(im.n)) return tscm_set_error(TSCM_E_HIP, "k_board_seeds returned a board beyond its workspace");
            J.cells.insert(J.cells.end(), src, src + len);
            J.offset[(size_t)i + 1] = (int)J.cells.size();
        }
    }
    return 0;
}

// every image's jobs; an image beyond the kernel's limit takes the host instantiation inside a device call
int run_jobs(int n_images, const tscm_corner_candidates *cands, int where, int device, const char *who, std::vector<ImageJobs> &jobs)
{
    jobs.assign((size_t)n_images, ImageJobs());
    std::vector<int> on_device;
    for (int k = 0; k < n_images; ++k)
        if (where == TSCM_BOARDS_DEVICE && cands[k].n >= 9 && cands[k].n <= TSCM_BOARDS_MAX_DEVICE_CANDIDATES) on_device.push_back(k);
    if (where == TSCM_BOARDS_DEVICE && n_images > 0) {
        if (int rc = select_device(device, who)) return rc;
        if (int rc = run_device(cands, on_device, jobs)) return rc;
    }
    for (int k = 0; k < n_images; ++k)
        if (!jobs[(size_t)k].on_device) run_host(cands[k], jobs[(size_t)k]);
    return 0;
}

template <typename T>
bool grab(T **p, size_t n)
{
    *p = static_cast<T *>(std::calloc(n ? n : 1, sizeof(T)));
    return *p != nullptr;
}

// overlap resolution and turn of one image's records
int finish(int n, const ImageJobs &J, tscm_chessboards *out)
{
    std::vector<unsigned char> mark((size_t)std::max(n, 1), 0);
    std::vector<int> keep((size_t)std::max(n, 1));
    const int nb = bd::resolve_overlaps(n, J.rec.data(), J.offset.data(), J.cells.data(), mark.data(), keep.data());
    size_t total = 0;
    for (int q = 0; q < nb; ++q) total += (size_t)J.rec[keep[q]].rows * J.rec[keep[q]].cols;
    if (!grab(&out->rows, (size_t)nb) || !grab(&out->cols, (size_t)nb) || !grab(&out->offset, (size_t)nb + 1) || !grab(&out->cells, total)) return TSCM_E_NOMEM;
    size_t o = 0;
    for (int q = 0; q < nb; ++q) {
        const bd::Record &r = J.rec[keep[q]];
        out->offset[q] = (int)o;
        bd::turned(r.rows, r.cols, J.cells.data() + J.offset[keep[q]], out->rows[q], out->cols[q], out->cells + o);
        o += (size_t)r.rows * r.cols;
    }
    out->offset[nb] = (int)o;
    out->n_boards = nb;
    return 0;
}

}  // namespace

extern "C" int tscm_chessboards_from_corners_batch(int n_images, const tscm_corner_candidates *cands, int where, int device_index, tscm_chessboards *out)
{
    if (int rc = check_args(n_images, cands, where, out)) return rc;
    if (n_images > 0) std::memset(out, 0, sizeof(*out) * (size_t)n_images);
    std::vector<ImageJobs> jobs;
    if (int rc = run_jobs(n_images, cands, where, device_index, "tscm_chessboards_from_corners_batch", jobs)) return rc;
    for (int k = 0; k < n_images; ++k)
        if (finish(cands[k].n, jobs[(size_t)k], out + k) != 0) {
            for (int q = 0; q <= k; ++q) tscm_chessboards_free(out + q);
            return tscm_set_error(TSCM_E_NOMEM, "out of memory");
        }
    return 0;
}

extern "C" void tscm_board_seed_stages_free(tscm_board_seed_stages *s)
{
    if (!s) return;
    std::free(s->status); std::free(s->rows); std::free(s->cols); std::free(s->steps); std::free(s->energy); std::free(s->offset); std::free(s->cells);
    std::memset(s, 0, sizeof(*s));
}

extern "C" int tscm_chessboards_batch_stages(int n_images, const tscm_corner_candidates *cands, int where, int device_index, tscm_board_seed_stages *out)
{
    if (int rc = check_args(n_images, cands, where, out)) return rc;
    if (n_images > 0) std::memset(out, 0, sizeof(*out) * (size_t)n_images);
    std::vector<ImageJobs> jobs;
    if (int rc = run_jobs(n_images, cands, where, device_index, "tscm_chessboards_batch_stages", jobs)) return rc;
    for (int k = 0; k < n_images; ++k) {
        const ImageJobs &J = jobs[(size_t)k];
        tscm_board_seed_stages *s = out + k;
        const size_t n = (size_t)cands[k].n;
        if (!grab(&s->status, n) || !grab(&s->rows, n) || !grab(&s->cols, n) || !grab(&s->steps, n) || !grab(&s->energy, n) || !grab(&s->offset, n + 1) ||
            !grab(&s->cells, J.cells.size())) {
            for (int q = 0; q <= k; ++q) tscm_board_seed_stages_free(out + q);
            return tscm_set_error(TSCM_E_NOMEM, "out of memory");
        }
        s->n = (int)n;
        s->on_device = J.on_device ? 1 : 0;
        for (size_t i = 0; i < n; ++i) {
            s->status[i] = J.rec[i].status; s->rows[i] = J.rec[i].rows; s->cols[i] = J.rec[i].cols; s->steps[i] = J.rec[i].steps; s->energy[i] = J.rec[i].energy;
        }
        std::memcpy(s->offset, J.offset.data(), sizeof(int) * (n + 1));
        if (!J.cells.empty()) std::memcpy(s->cells, J.cells.data(), sizeof(int) * J.cells.size());
    }
    return 0;
}

extern "C" double tscm_chessboards_batch_seconds(void) { return g_kernel_seconds; }
