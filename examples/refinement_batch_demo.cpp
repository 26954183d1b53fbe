// TripleSphereCamera::refinement_batch through the mirror header (include/tscm/tscm_calib.hpp): the refinements of several
// cameras in one batch, then the same cameras refined one by one with refinement(), and a batch with mixed losses (refused).
//   refinement_batch_demo <in.bin> <out.bin>
// in.bin:  int C, V, n; double worlds[n][3]; per camera: double intr[9], unsigned char has[V], double rt[V][6],
//          double pix[V][n][2]
// out.bin: per camera, batch then solo: double intr[9], double rt[V][6], int converged, int num_iterations
// Build: g++ -std=c++11 -I include examples/refinement_batch_demo.cpp -L tscm_calib_amd/csrc -ltscm_hip
#include <tscm/tscm_calib.hpp>

#include <cstdio>
#include <vector>

using namespace tscm;

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: refinement_batch_demo <in.bin> <out.bin>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[3];
    if (std::fread(hdr, sizeof(int), 3, f) != 3) return 2;
    const int C = hdr[0], V = hdr[1], n = hdr[2];
    std::vector<double> w(3 * (size_t)n);
    if (std::fread(w.data(), sizeof(double), w.size(), f) != w.size()) return 2;
    std::vector<Point3d> worlds(n);
    for (int j = 0; j < n; ++j) worlds[j] = Point3d{ w[3 * j], w[3 * j + 1], w[3 * j + 2] };
    std::vector<TripleSphereCamera> batch(C), solo(C);
    std::vector<std::vector<std::vector<Point2d> > > pixels(C);
    for (int m = 0; m < C; ++m) {
        std::vector<double> intr(9), rt(6 * (size_t)V), pix(2 * (size_t)V * n);
        std::vector<unsigned char> has(V);
        if (std::fread(intr.data(), sizeof(double), 9, f) != 9 || std::fread(has.data(), 1, V, f) != (size_t)V ||
            std::fread(rt.data(), sizeof(double), rt.size(), f) != rt.size() || std::fread(pix.data(), sizeof(double), pix.size(), f) != pix.size())
            return 2;
        TripleSphereCamera &c = batch[m];
        c.intrinsic_ = intr;
        c.has_chessboard_.assign(V, false);
        c.rt_.assign(V, std::vector<double>(6, 0.0));
        pixels[m].assign(V, std::vector<Point2d>());
        for (int i = 0; i < V; ++i) {
            c.has_chessboard_[i] = has[i] != 0;
            c.rt_[i].assign(&rt[6 * (size_t)i], &rt[6 * (size_t)i] + 6);
            if (has[i]) for (int j = 0; j < n; ++j) pixels[m][i].push_back(Point2d{ pix[2 * ((size_t)i * n + j)], pix[2 * ((size_t)i * n + j) + 1] });
        }
        if (m == 1) c.set_fixed_intrinsics(TSCM_MODEL_DS);      // a mask per camera
        solo[m] = c;
    }
    std::fclose(f);
    std::vector<TripleSphereCamera *> ptr(C);
    for (int m = 0; m < C; ++m) ptr[m] = &batch[m];
    const std::vector<bool> conv = TripleSphereCamera::refinement_batch(ptr, pixels, worlds);
    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (int pass = 0; pass < 2; ++pass)
        for (int m = 0; m < C; ++m) {
            TripleSphereCamera &c = pass ? solo[m] : batch[m];
            const int ok = pass ? (c.refinement(pixels[m], worlds) ? 1 : 0) : (conv[m] ? 1 : 0);
            std::fwrite(c.intrinsic_.data(), sizeof(double), 9, o);
            for (int i = 0; i < V; ++i) std::fwrite(c.rt_[i].data(), sizeof(double), 6, o);
            const int it[2] = { ok, c.summary.num_iterations };
            std::fwrite(it, sizeof(int), 2, o);
        }
    std::fclose(o);
    // the loss is shared by a batch: a camera with another loss is refused before anything runs
    batch[1].set_loss(TSCM_LOSS_HUBER, 1.0);
    try {
        TripleSphereCamera::refinement_batch(ptr, pixels, worlds);
        std::printf("mixed losses accepted\n");
        return 1;
    } catch (const std::invalid_argument &e) {
        std::printf("mixed losses refused: %s\n", e.what());
    }
    std::printf("refinement_batch: %d cameras\n", C);
    return 0;
}
