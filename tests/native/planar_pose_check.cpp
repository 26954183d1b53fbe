// CPU run of the planar pose fit (tscm_calib_amd/csrc/tscm_planar_pose.h), the one copy behind k_estimate_extrinsic and the
// refit of k_estimate_extrinsic_ransac: the serial lane policy, per view, as k_estimate_extrinsic<true> drives it -- over
// all corners, or over the corners of a mask as the refit does.  Reads one case from stdin (numbers as strtod takes them):
//   V n board_w has_masks | intr[9] | worlds[3n] | count[V] | pu[V n] | pv[V n] | masks[V n] if has_masks
// and prints one JSON line with, per view, T, H, rv0, t0, rv, t, steps, code, Rt (a stage not reached is NaN, steps -1).
#include "../../tscm_calib_amd/csrc/tscm_planar_pose.h"

#include <cmath>
#include <cstdio>
#include <vector>

namespace {

bool read(std::vector<double> &v, size_t n)
{
    v.resize(n);
    for (double &x : v)
        if (std::scanf("%lf", &x) != 1) return false;
    return true;
}

void print(const char *name, const double *v, int n, const char *tail = ", ")
{
    std::printf("\"%s\": [", name);
    for (int i = 0; i < n; ++i) {
        if (std::isnan(v[i])) std::printf("NaN");
        else if (std::isinf(v[i])) std::printf(v[i] < 0 ? "-Infinity" : "Infinity");
        else std::printf("%.17g", v[i]);
        std::printf(i + 1 < n ? ", " : "");
    }
    std::printf("]%s", tail);
}

}  // namespace

int main()
{
    int V, n, board_w, has_masks;
    if (std::scanf("%d %d %d %d", &V, &n, &board_w, &has_masks) != 4 || V < 0 || n < 4 || board_w < 1 || n / 2 - board_w / 2 - 1 < 0) return 2;
    std::vector<double> intr, worlds, count, pu, pv, masks;
    const size_t npix = (size_t)V * n;
    if (!read(intr, 9) || !read(worlds, 3 * (size_t)n) || !read(count, V) || !read(pu, npix) || !read(pv, npix) || (has_masks && !read(masks, npix))) return 2;
    const int ref = n / 2 - board_w / 2 - 1;
    std::printf("{\"views\": [");
    for (int k = 0; k < V; ++k) {
        const double *u = pu.data() + (size_t)k * n, *v = pv.data() + (size_t)k * n, *mask = has_masks ? masks.data() + (size_t)k * n : nullptr;
        double T[9], Rt[9], stage[tscm::kStageSteps + 1];
        for (double &x : T) x = NAN;
        for (double &x : Rt) x = NAN;
        for (double &x : stage) x = NAN;
        int code = TSCM_EXTRINSIC_NO_BOARD;
        if (count[k] != 0) {
            tscm::look_at_turn(intr.data(), u[ref], v[ref], T);
            int m = 0;
            for (int i = 0; i < n; ++i) m += !mask || mask[i] != 0;
            auto corner = [&](int i, double &x, double &y) {
                if (mask && mask[i] == 0) return false;
                double Z;
                tscm::turned_corner(intr.data(), T, u[i], v[i], x, y, Z);
                return true;
            };
            double rv[3], t[3], R[9], dR[27];
            code = tscm::fit_planar_pose(tscm::SerialLanes{}, corner, m, worlds.data(), n, stage, rv, t);
            if (code >= TSCM_EXTRINSIC_CONVERGED) {
                tscm::rotation_and_derivatives(rv, R, dR);
                tscm::compose_rt(T, R, t, Rt);
            }
        }
        std::printf("%s{", k ? ", " : "");
        print("T", T, 9);
        print("H", stage + tscm::kStageH, 9);
        print("rv0", stage + tscm::kStagePose0, 3);
        print("t0", stage + tscm::kStagePose0 + 3, 3);
        print("rv", stage + tscm::kStagePose, 3);
        print("t", stage + tscm::kStagePose + 3, 3);
        print("Rt", Rt, 9);
        std::printf("\"steps\": %d, \"code\": %d}", std::isnan(stage[tscm::kStageSteps]) ? -1 : (int)stage[tscm::kStageSteps], code);
    }
    std::printf("]}\n");
    return 0;
}
