// tscm_calib.hpp -- C++11 mirror of the reference's class interface for the accelerated path, on
// top of the C ABI (tscm.h).  Same class and member names, argument meaning and post-conditions as
// imuncle/TSCM_Calib's TripleSphereCamera (TS.h) / MultiCalib (multi_calib.h), with plain structs
// where the reference uses cv::Point / cv::Mat, so that a maintainer can move a call site over by
// changing types only.  Everything heavy runs on the MI355X through libtscm_hip.so; what stays on
// the host are the 3x3 conversions the reference also does on the host (update_param:
// multi_calib.h:42-57,104-108).  Failures throw std::runtime_error(tscm_last_error()).
//
//   reference                                              here
//   TripleSphereCamera::refinement       TS.cpp:247-282    TripleSphereCamera::refinement      -> tscm_solve_mono
//                                                           TripleSphereCamera::refinement_batch (several cameras) -> tscm_solve_mono_batch
//   TripleSphereCamera::estimate_focal   TS.cpp:110-168    TripleSphereCamera::estimate_focal  -> tscm_estimate_focal
//   TripleSphereCamera::estimate_extrinsic TS.cpp:170-203  TripleSphereCamera::estimate_extrinsic -> tscm_estimate_extrinsic (*)
//   loop Rt_ -> rt_                      TS.cpp:62-74      TripleSphereCamera::poses_from_Rt   -> tscm_poses_from_r1r2t
//   TripleSphereCamera::calibrate        TS.cpp:30-105     TripleSphereCamera::calibrate       (the four calls above + refinement)
//   TripleSphereCamera::project          TS.cpp:332-344    TripleSphereCamera::project (batch) -> tscm_project_points
//   get_unit_sphere_coordinate           TS.h:39-57        get_unit_sphere_coordinate (batch)  -> tscm_unproject_pixels
//   TripleSphereCamera::undistort        TS.cpp:284-306    TripleSphereCamera::undistort       -> tscm_build_maps
//   undistort_chessboard (table)         TS.cpp:308-330    undistort_chessboard_maps           -> tscm_build_maps
//   (none: pinhole tables only)                            undistort(..., projection), rectify_pair_maps -> tscm_build_maps_ex
//   (none)                                                 TripleSphereCamera::rectify_point   -> tscm_rectify_points
//   (none: the rectified pair is its last product)         stereo_match, stereo_points         -> tscm_stereo_match, tscm_stereo_points
//   (none: cv::filterSpeckles / medianBlur downstream)     stereo_filter                       -> tscm_stereo_filter
//   (none: hole filling is left to the caller)             stereo_fill, parse_fill_option      -> tscm_stereo_fill
//   (none: cv::ximgproc::weightedMedianFilter downstream)  stereo_refine, range_weights, parse_refine_option -> tscm_stereo_refine
//   (none: occlusion is not handled)                       Sweep::visibility, parse_visibility_option -> tscm_sweep_visibility
//   MultiCalib::MultiCalib               multi_calib.cpp:6-153    MultiCalib::MultiCalib       -> tscm_rig_init
//   MultiCalib::calibrate                multi_calib.cpp:155-283  MultiCalib::calibrate        -> tscm_solve_multi, tscm_reprojection_error
//   YAML output                          main.cpp:305-319         MultiCalib::write_yaml       -> tscm_yaml_write
//   (the error report of multi_calib.cpp:233-283 only)     residual_report on both classes, view_outliers,
//                                                          MultiCalib::prune_views             -> tscm_residual_report
//   AddResidualBlock(new NormalPrior(A, mean), NULL, x)    CameraPriors, set_camera_priors on both classes, set_prior_sigmas,
//                                                          parse_prior_option                  -> tscm_solve_prior, tscm_covariance_prior
//   (cv::solvePnPRansac inside estimate_extrinsic)         TripleSphereCamera::estimate_extrinsic_ransac, set_ransac,
//                                                          parse_ransac_option                 -> tscm_estimate_extrinsic_ransac
// (*) deterministic planar PnP in place of cv::solvePnPRansac (see tscm.h)
#ifndef TSCM_CALIB_HPP
#define TSCM_CALIB_HPP

#include <tscm/tscm.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace tscm {

struct Point2d { double x, y; };
struct Point3d { double x, y, z; };
struct Size { int width, height; };
struct Mat33 { double a[9]; };       // row-major, cv::Mat_<double>(3,3) order

inline void check(int rc) { if (rc != 0) throw std::runtime_error(std::string("tscm: ") + tscm_last_error()); }

// The calibration demos' --ransac THRESHOLD[,HYPOTHESES[,MIN_INLIERS]] -> threshold_px, n_hypotheses and min_inliers of p;
// false when the text is none of that, the threshold is not > 0 or HYPOTHESES lies outside 1..4096 (min_inliers depends on the
// board and is left to tscm_estimate_extrinsic_ransac).
inline bool parse_ransac_option(const char *text, tscm_ransac_params *p)
{
    const char *q = text;
    double thr = 0.0;
    long field[3] = { 0, p->n_hypotheses, p->min_inliers };
    for (int k = 0; k < 3; ++k) {                               // numbers, nothing before, between or after them
        char *end = NULL;
        if (*q != '.' && (*q < '0' || *q > '9')) return false;
        if (k == 0) thr = std::strtod(q, &end);
        else field[k] = std::strtol(q, &end, 10);
        if (end == q) return false;
        if (!*end) break;
        if (*end != ',' || k == 2) return false;
        q = end + 1;
    }
    if (!(thr > 0.0) || field[1] < 1 || field[1] > 4096 || field[2] < 0 || field[2] > 1024) return false;
    p->threshold_px = thr;
    p->n_hypotheses = (int)field[1];
    p->min_inliers = (int)field[2];
    return true;
}

// Command-line forms of the held-intrinsics masks (tscm.h, TSCM_FIX_*), for the example programs.
// model_mask: "ts" -> 0, "ds" -> TSCM_MODEL_DS, "ucm" -> TSCM_MODEL_UCM; false for another name.
inline bool model_mask(const char *name, unsigned short &word)
{
    const std::string n(name);
    if (n == "ts") word = 0;
    else if (n == "ds") word = TSCM_MODEL_DS;
    else if (n == "ucm") word = TSCM_MODEL_UCM;
    else return false;
    return true;
}
// fixed_list_mask: "fx,cx,lambda" -> the OR of those bits (names of fx fy cx cy xi lambda alpha); false for an unknown or empty name.
inline bool fixed_list_mask(const char *list, unsigned short &word)
{
    static const char *const names[7] = { "fx", "fy", "cx", "cy", "xi", "lambda", "alpha" };
    const std::string l(list);
    word = 0;
    for (size_t b = 0; b <= l.size();) {
        size_t e = l.find(',', b);
        if (e == std::string::npos) e = l.size();
        const std::string name = l.substr(b, e - b);
        int k = 0;
        while (k < 7 && name != names[k]) ++k;
        if (k == 7) return false;
        word = (unsigned short)(word | (1u << k));
        b = e + 1;
    }
    return true;
}

// Gaussian priors on camera parameters (tscm.h, "Gaussian priors": Ceres' NormalPrior on single coordinates) in the mirror's
// shape: mean and weight per coordinate, cam_rt_* [C*6] on the raw pose vectors, intr_* [C*9] on fx fy cx cy xi lambda alpha b c;
// a pair may be empty.  Weight = (pixel sigma / sigma)^2, 0 = no prior; a weight on a coordinate that is not free counts as 0.
struct CameraPriors {
    std::vector<double> cam_rt_mean, cam_rt_weight, intr_mean, intr_weight;
    // the C struct over these vectors (valid while they are)
    tscm_camera_priors c_struct() const
    {
        tscm_camera_priors p = tscm_camera_priors();
        p.struct_size = sizeof(tscm_camera_priors);
        p.cam_rt_mean = cam_rt_mean.empty() ? NULL : cam_rt_mean.data(); p.cam_rt_weight = cam_rt_weight.empty() ? NULL : cam_rt_weight.data();
        p.intr_mean = intr_mean.empty() ? NULL : intr_mean.data(); p.intr_weight = intr_weight.empty() ? NULL : intr_weight.data();
        return p;
    }
};
// Command-line form of intrinsic priors, for the example programs: "xi:0.1,lambda:0.05" -> sigma[7] by the names of
// fixed_list_mask (0 where none is given); false for an unknown name, a missing or malformed sigma, or one that is not finite and > 0.
inline bool parse_prior_option(const char *list, double sigma[7])
{
    static const char *const names[7] = { "fx", "fy", "cx", "cy", "xi", "lambda", "alpha" };
    const std::string l(list);
    for (int k = 0; k < 7; ++k) sigma[k] = 0.0;
    for (size_t b = 0; b <= l.size();) {
        size_t e = l.find(',', b);
        if (e == std::string::npos) e = l.size();
        const std::string item = l.substr(b, e - b);
        const size_t colon = item.find(':');
        if (colon == std::string::npos || colon + 1 >= item.size()) return false;
        int k = 0;
        while (k < 7 && item.substr(0, colon) != names[k]) ++k;
        if (k == 7) return false;
        const std::string num = item.substr(colon + 1);
        if (num[0] != '.' && (num[0] < '0' || num[0] > '9')) return false;
        char *end = NULL;
        const double v = std::strtod(num.c_str(), &end);
        if (*end != '\0' || !(v > 0.0) || !std::isfinite(v)) return false;
        sigma[k] = v;
        b = e + 1;
    }
    return true;
}
// priors on the intrinsics of n cameras about the values intr [n*9] holds now: weight 1 / sigma[k]^2 where sigma[k] > 0
inline CameraPriors intrinsic_priors_about(const std::vector<double> &intr, const double sigma[7])
{
    CameraPriors p;
    p.intr_mean = intr;
    p.intr_weight.assign(intr.size(), 0.0);
    for (size_t i = 0; i < intr.size(); ++i) if (i % 9 < 7 && sigma[i % 9] > 0.0) p.intr_weight[i] = 1.0 / (sigma[i % 9] * sigma[i % 9]);
    return p;
}
// what the example programs print: camera m's priors that count under its held intrinsics `fixed`, one line each
inline void print_effective_priors(const CameraPriors &p, size_t cam, int m, unsigned short fixed, const char *stage)
{
    static const char *const names[7] = { "fx", "fy", "cx", "cy", "xi", "lambda", "alpha" };
    for (int k = 0; k < 7; ++k) {
        const size_t i = 9 * cam + (size_t)k;
        if (i >= p.intr_weight.size() || !(p.intr_weight[i] > 0.0) || ((fixed >> k) & 1)) continue;
        std::printf("camera_%d %s prior %s %.17g +- %.17g\n", m, stage, names[k], p.intr_mean[i], 1.0 / std::sqrt(p.intr_weight[i]));
    }
}

// cv::Rodrigues(r -> R), the conversion update_param() does on the host (multi_calib.h:43-45,105-106)
// ---- residual report (tscm.h: tscm_residual_report) of a problem as the classes below build it
struct ResidualReport {
    tscm_residual_info info;
    int n_cameras, grid_w, grid_h, n_angle_bins;
    std::vector<int> view_camera, view_board, view_count;      // the views of the problem that was reported on
    std::vector<double> corner;            // [N][6]  r_u r_v r_rad r_tan angle rho1
    std::vector<double> view;              // [V][8]  n_used sum_w rms mean_err max_err bias_u bias_v mean_rad
    std::vector<int> view_worst;           // [V]
    std::vector<double> camera;            // [C][8]  n_used sum_w rms mean_err max_err worst_view n_views_used 0
    std::vector<long long> grid_count, angle_count;     // [C][gh][gw][2], [C][K][2]: count, n_clamped
    std::vector<double> grid, angle;       // [C][gh][gw][3] mean_u mean_v rms, [C][K][4] mean_rad mean_tan rms mean_angle
};

// params: NULL = the defaults (no loss, no field); weights: [N] in corner order or NULL
inline ResidualReport residual_report_of(const tscm_problem &P, int device, const double *weights, const tscm_residual_params *params)
{
    tscm_residual_params prm;
    if (params) prm = *params; else tscm_residual_default_params(&prm);
    ResidualReport r;
    const size_t C = (size_t)P.n_cameras, V = (size_t)P.n_views;
    size_t N = 0;
    for (size_t v = 0; v < V; ++v) N += (size_t)P.view_count[v];
    r.n_cameras = P.n_cameras; r.grid_w = prm.grid_w; r.grid_h = prm.grid_h; r.n_angle_bins = prm.n_angle_bins;
    r.view_camera.assign(P.view_camera, P.view_camera + V); r.view_board.assign(P.view_board, P.view_board + V); r.view_count.assign(P.view_count, P.view_count + V);
    const size_t cells = (size_t)prm.grid_w * prm.grid_h, K = (size_t)prm.n_angle_bins;
    r.corner.assign(6 * N + 1, 0.0); r.view.assign(8 * V + 1, 0.0); r.view_worst.assign(V + 1, -1); r.camera.assign(8 * C, 0.0);
    r.grid_count.assign(2 * C * cells + 1, 0); r.grid.assign(3 * C * cells + 1, 0.0); r.angle_count.assign(2 * C * K + 1, 0); r.angle.assign(4 * C * K + 1, 0.0);
    r.info = tscm_residual_info();
    r.info.struct_size = (int)sizeof(tscm_residual_info);
    check(tscm_residual_report(&P, device, weights, &prm, r.corner.data(), r.view.data(), r.view_worst.data(), r.camera.data(), r.grid_count.data(), r.grid.data(),
                               r.angle_count.data(), r.angle.data(), &r.info));
    r.corner.resize(6 * N); r.view.resize(8 * V); r.view_worst.resize(V); r.grid_count.resize(2 * C * cells); r.grid.resize(3 * C * cells);
    r.angle_count.resize(2 * C * K); r.angle.resize(4 * C * K);
    return r;
}

// The views of a report whose rms stands out in their camera (api.view_outliers, the same rule and the same arithmetic): per
// camera, over its views with n_used > 0, view v is flagged when rms_v > median + k * 1.4826 * MAD of those rms values and
// rms_v > floor; at most floor(max_fraction * those views) per camera, the worst first, ties to the lower view.
inline std::vector<bool> view_outliers(const ResidualReport &r, double k = 3.0, double floor = 0.0, double max_fraction = 0.2)
{
    const size_t V = r.view_camera.size();
    std::vector<bool> out(V, false);
    auto median = [](std::vector<double> x) {
        std::sort(x.begin(), x.end());
        const size_t n = x.size();
        return n % 2 ? x[n / 2] : (x[n / 2 - 1] + x[n / 2]) / 2.0;
    };
    for (int m = 0; m < r.n_cameras; ++m) {
        std::vector<size_t> views;
        std::vector<double> x;
        for (size_t v = 0; v < V; ++v)
            if (r.view_camera[v] == m && r.view[8 * v] > 0.0) { views.push_back(v); x.push_back(r.view[8 * v + 2]); }
        if (views.empty()) continue;
        const double med = median(x);
        std::vector<double> dev(x.size());
        for (size_t i = 0; i < x.size(); ++i) dev[i] = std::fabs(x[i] - med);
        const double limit = med + k * 1.4826 * median(dev);
        std::vector<size_t> hit;
        for (size_t i = 0; i < x.size(); ++i)
            if (x[i] > limit && x[i] > floor) hit.push_back(views[i]);
        std::stable_sort(hit.begin(), hit.end(), [&r](size_t a, size_t b) { return r.view[8 * a + 2] > r.view[8 * b + 2]; });   // hit ascends: ties keep the lower view first
        const size_t cap = (size_t)std::floor(max_fraction * (double)views.size());
        for (size_t i = 0; i < hit.size() && i < cap; ++i) out[hit[i]] = true;
    }
    return out;
}

// the residual options of the calibrate_from_* programs: --residuals[=FILE], --residual-bins K, --prune K[,ROUNDS[,MAX_FRACTION]]
struct ResidualOptions {
    bool report = false;
    std::string file;                      // empty: standard output
    int bins = 0;
    bool prune = false;
    double k = 3.0, max_fraction = 0.2;
    int rounds = 1;
};
// argv[i] as one of those options (argv[i + 1] consumed where the option takes a value): 1 taken, 0 not one of them, -1 malformed
inline int parse_residual_option(int argc, char **argv, int &i, ResidualOptions &o)
{
    const char *a = argv[i];
    if (!std::strcmp(a, "--residuals")) { o.report = true; return 1; }
    if (!std::strncmp(a, "--residuals=", 12)) { o.report = true; o.file = a + 12; return o.file.empty() ? -1 : 1; }
    if (!std::strcmp(a, "--residual-bins")) {
        if (i + 1 >= argc) return -1;
        char *end = nullptr;
        const long n = std::strtol(argv[++i], &end, 10);
        if (end == argv[i] || *end != '\0' || n < 1 || n > 64) return -1;
        o.bins = (int)n; o.report = true;
        return 1;
    }
    if (!std::strcmp(a, "--prune")) {
        if (i + 1 >= argc) return -1;
        char *end = nullptr;
        const char *at = argv[++i];
        o.k = std::strtod(at, &end);
        if (end == at || !(o.k >= 0.0) || !std::isfinite(o.k)) return -1;
        if (*end == ',') {
            at = end + 1;
            const long r = std::strtol(at, &end, 10);
            if (end == at || r < 1 || r > 100) return -1;
            o.rounds = (int)r;
            if (*end == ',') {
                at = end + 1;
                o.max_fraction = std::strtod(at, &end);
                if (end == at || !(o.max_fraction >= 0.0) || !(o.max_fraction <= 1.0)) return -1;
            }
        }
        if (*end != '\0') return -1;
        o.prune = true;
        return 1;
    }
    return 0;
}

// the per-view table -- `view camera board corners_used rms max worst_corner` -- and, with angle bins, per camera the profile
// `camera_m angle lo hi count clamped mean_rad mean_tan rms` (radians; pixels)
inline void print_residual_report(std::FILE *f, const ResidualReport &r, double max_angle)
{
    std::fprintf(f, "residuals: %lld corners in %d views, rmse %.6f px\n", r.info.n_used, r.info.n_views_used, r.info.rmse);
    for (size_t v = 0; v < r.view_camera.size(); ++v)
        std::fprintf(f, "view %zu camera %d board %d corners %d rms %.6f max %.6f worst %d\n", v, r.view_camera[v], r.view_board[v], (int)r.view[8 * v],
                     r.view[8 * v + 2], r.view[8 * v + 4], r.view_worst[v]);
    for (int m = 0; m < r.n_cameras; ++m)
        for (int k = 0; k < r.n_angle_bins; ++k) {
            const size_t o = (size_t)m * r.n_angle_bins + k;
            std::fprintf(f, "camera_%d angle %.4f %.4f count %lld clamped %lld mean_rad %.6f mean_tan %.6f rms %.6f\n", m, max_angle * k / r.n_angle_bins,
                         max_angle * (k + 1) / r.n_angle_bins, r.angle_count[2 * o], r.angle_count[2 * o + 1], r.angle[4 * o], r.angle[4 * o + 1], r.angle[4 * o + 2]);
        }
}

inline Mat33 rodrigues(const double r[3])
{
    const double th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2], th = std::sqrt(th2);
    Mat33 R = { { 1, 0, 0, 0, 1, 0, 0, 0, 1 } };
    if (th < 2.220446049250313e-16) return R;
    const double c = std::cos(th), s = std::sin(th), c1 = 1.0 - c, k[3] = { r[0] / th, r[1] / th, r[2] / th };
    const double K[9] = { 0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0 };
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R.a[3 * i + j] = (i == j ? c : 0.0) + c1 * k[i] * k[j] + s * K[3 * i + j];
    return R;
}

class TripleSphereCamera {
public:
    explicit TripleSphereCamera(int device = 0) : intrinsic_(9, 0.0), device_(device) {}

    // ---- state with the reference's names (TS.h:78-92) ----
    std::vector<double> intrinsic_;                       // fx fy cx cy xi lambda alpha b c
    std::vector<std::vector<double> > rt_;                // per image: angle-axis + t
    std::vector<Mat33> Rt_;                               // per image: [r1 r2 t]
    std::vector<bool> has_chessboard_;
    std::vector<std::vector<Point2d> > pixels_;

    const std::vector<double> &intrinsic() const { return intrinsic_; }
    bool has_chessboard(int j) const { return has_chessboard_[j]; }
    std::vector<bool> has_chessboard() const { return has_chessboard_; }
    const Mat33 &Rt(int j) const { return Rt_[j]; }
    const std::vector<std::vector<Point2d> > &pixels() const { return pixels_; }
    tscm_summary summary;                                 // of the last refinement()

    // the loss of every residual block of refinement(): TSCM_LOSS_HUBER / _SOFT_L1 / _CAUCHY with its scale in pixels
    // (Ceres' HuberLoss(scale) etc.), TSCM_LOSS_NONE = the reference's NULL (the default).  Checked by the next refinement().
    void set_loss(int kind, double scale) { loss_kind_ = kind; loss_scale_ = scale; }
    // intrinsics refinement() holds at their current values: TSCM_FIX_* bits (TSCM_MODEL_DS, TSCM_MODEL_UCM,
    // TSCM_FIX_INTRINSICS, ...) -- SetManifold(intrinsic_.data(), new SubsetManifold(9, {...})).  0 = none (the default).
    void set_fixed_intrinsics(unsigned short fixed) { fixed_ = fixed; }
    // corner weights of refinement() (tscm.h, "corner weights": Ceres' ScaledLoss per residual block, weight 0 takes the corner
    // out and its pixel may hold anything): weights[i][j] for corner j of view i, shaped like `pixels`; NULL = none (the
    // default).  A view whose weights are all 0 is left out of the refinement like a view without a chessboard.  After a
    // calibrate() with set_ransac(params, true) the RANSAC inlier masks take their place.
    void set_corner_weights(const std::vector<std::vector<double> > *weights)
    {
        use_weights_ = weights != NULL;
        corner_weights_ = weights ? *weights : std::vector<std::vector<double> >();
    }
    // Gaussian priors of refinement() (tscm.h, "Gaussian priors"): a CameraPriors of ONE camera -- intr_* [9]; the pose of a mono
    // problem is not free, so cam_rt_* counts for nothing -- or NULL for none (the default).  Copied.
    void set_camera_priors(const CameraPriors *priors)
    {
        use_priors_ = priors != NULL;
        priors_ = priors ? *priors : CameraPriors();
    }
    // ... or priors about the values each refinement() STARTS from -- calibrate() estimates them first -- with these standard
    // deviations in the unit of a pixel's (sigma[k] of fx fy cx cy xi lambda alpha, 0 = none); NULL = none.  Explicit priors
    // (set_camera_priors) come first.  last_priors_: what the last refinement() took.
    void set_prior_sigmas(const double *sigma7)
    {
        use_sigmas_ = sigma7 != NULL;
        for (int k = 0; k < 7; ++k) prior_sigma_[k] = sigma7 ? sigma7[k] : 0.0;
    }
    CameraPriors last_priors_;
    // weight of corner j of view i in the next refinement(); *weighted: whether there are weights at all
    double corner_weight(size_t i, size_t j, bool *weighted) const
    {
        const bool mask = use_ransac_ && mask_outliers_ && ransac_inliers_.size() == has_chessboard_.size();
        *weighted = mask || use_weights_;
        if (mask) return i < ransac_inliers_.size() && j < ransac_inliers_[i].size() && ransac_inliers_[i][j] ? 1.0 : 0.0;
        if (use_weights_) return i < corner_weights_.size() && j < corner_weights_[i].size() ? corner_weights_[i][j] : 0.0;
        return 1.0;
    }

    // TS.cpp:247-282: joint refinement of intrinsic_ and rt_[i]; returns termination_type == CONVERGENCE
    bool refinement(const std::vector<std::vector<Point2d> > &pixels, const std::vector<Point3d> &worlds,
                    const tscm_options *options = nullptr)
    {
        const int V = (int)pixels.size(), n = (int)worlds.size();
        std::vector<double> bxy(2 * (size_t)n), u, v, w, rt(6 * (size_t)V, 0.0);
        std::vector<int> vc, vb, vo, vn;
        bool weighted = false;
        for (int j = 0; j < n; ++j) { bxy[2 * j] = worlds[j].x; bxy[2 * j + 1] = worlds[j].y; }
        for (int i = 0; i < V; ++i) {
            if (!has_chessboard_[i]) continue;                           // TS.cpp:253
            std::memcpy(&rt[6 * (size_t)i], rt_[i].data(), 6 * sizeof(double));
            bool any = false;
            for (size_t j = 0; j < pixels[i].size(); ++j) any = corner_weight((size_t)i, j, &weighted) != 0.0 || any;
            if (weighted && !any) continue;                              // every weight 0: no residual block of this view
            for (size_t j = 0; j < pixels[i].size(); ++j) w.push_back(corner_weight((size_t)i, j, &weighted));
            vc.push_back(0); vb.push_back(i); vo.push_back((int)u.size()); vn.push_back((int)pixels[i].size());
            for (const Point2d &p : pixels[i]) { u.push_back(p.x); v.push_back(p.y); }
        }
        tscm_problem P = tscm_problem();
        P.n_cameras = 1; P.n_boards = V; P.n_points = n; P.n_views = (int)vc.size();
        P.board_xy = bxy.data(); P.view_camera = vc.data(); P.view_board = vb.data(); P.view_offset = vo.data(); P.view_count = vn.data();
        P.obs_u = u.data(); P.obs_v = v.data(); P.intr = intrinsic_.data(); P.board_rt = rt.data(); P.mono = 1;
        tscm_options o;
        if (options) o = *options; else tscm_default_options(&o, 1);
        last_priors_ = use_priors_ ? priors_ : use_sigmas_ ? intrinsic_priors_about(intrinsic_, prior_sigma_) : CameraPriors();
        const tscm_camera_priors cp = last_priors_.c_struct();
        check(tscm_solve_prior(&P, &o, weighted ? w.data() : NULL, fixed_ ? &fixed_ : NULL, loss_kind_, loss_scale_, use_priors_ || use_sigmas_ ? &cp : NULL, &summary));
        for (int i = 0; i < V; ++i) if (has_chessboard_[i]) rt_[i].assign(&rt[6 * (size_t)i], &rt[6 * (size_t)i] + 6);
        return summary.termination_type == TSCM_CONVERGENCE;             // TS.cpp:281
    }

    // Residual report (tscm_residual_report) of the problem refinement() solves, at the object's current intrinsic_ and rt_:
    // every view with a chessboard, in order; with corner weights (or RANSAC masks) a view whose weights are all 0 stays in as an
    // unused view.  The loss is the one set on this object unless params carries one.  params: NULL = defaults.
    ResidualReport residual_report(const std::vector<std::vector<Point2d> > &pixels, const std::vector<Point3d> &worlds,
                                   const tscm_residual_params *params = nullptr) const
    {
        const int V = (int)pixels.size(), n = (int)worlds.size();
        std::vector<double> bxy(2 * (size_t)n), u, v, w, rt(6 * (size_t)V, 0.0), I(intrinsic_);
        std::vector<int> vc, vb, vo, vn;
        bool weighted = false;
        for (int j = 0; j < n; ++j) { bxy[2 * j] = worlds[j].x; bxy[2 * j + 1] = worlds[j].y; }
        for (int i = 0; i < V; ++i) {
            if (!has_chessboard_[i]) continue;
            std::memcpy(&rt[6 * (size_t)i], rt_[i].data(), 6 * sizeof(double));
            for (size_t j = 0; j < pixels[i].size(); ++j) w.push_back(corner_weight((size_t)i, j, &weighted));
            vc.push_back(0); vb.push_back(i); vo.push_back((int)u.size()); vn.push_back((int)pixels[i].size());
            for (const Point2d &p : pixels[i]) { u.push_back(p.x); v.push_back(p.y); }
        }
        tscm_problem P = tscm_problem();
        P.n_cameras = 1; P.n_boards = V; P.n_points = n; P.n_views = (int)vc.size();
        P.board_xy = bxy.data(); P.view_camera = vc.data(); P.view_board = vb.data(); P.view_offset = vo.data(); P.view_count = vn.data();
        P.obs_u = u.data(); P.obs_v = v.data(); P.intr = I.data(); P.board_rt = rt.data(); P.mono = 1;
        tscm_residual_params prm;
        if (params) prm = *params; else { tscm_residual_default_params(&prm); prm.loss_kind = loss_kind_; prm.loss_scale = loss_scale_; }
        return residual_report_of(P, device_, weighted ? w.data() : nullptr, &prm);
    }

    // refinement() of several cameras in ONE batch (tscm_solve_mono_batch): cams[k] is refined on pixels[k], all against the
    // same worlds, each with the post-conditions of cams[k]->refinement(pixels[k], worlds, options) -- intrinsic_, rt_ and
    // summary updated, its own fixed mask honoured -- and returns, per camera, termination_type == CONVERGENCE.  The loss is
    // shared by a batch: cameras with different losses (set_loss) are refused with std::invalid_argument before anything runs.
    static std::vector<bool> refinement_batch(const std::vector<TripleSphereCamera *> &cams,
                                              const std::vector<std::vector<std::vector<Point2d> > > &pixels,
                                              const std::vector<Point3d> &worlds, const tscm_options *options = nullptr)
    {
        const size_t K = cams.size();
        if (K == 0 || pixels.size() != K) throw std::invalid_argument("tscm: refinement_batch needs one pixel set per camera");
        for (size_t k = 1; k < K; ++k)
            if (cams[k]->loss_kind_ != cams[0]->loss_kind_ || (cams[0]->loss_kind_ != TSCM_LOSS_NONE && cams[k]->loss_scale_ != cams[0]->loss_scale_))
                throw std::invalid_argument("tscm: refinement_batch: the cameras of a batch must share one loss (set_loss)");
        const int n = (int)worlds.size();
        std::vector<double> bxy(2 * (size_t)n);
        for (int j = 0; j < n; ++j) { bxy[2 * j] = worlds[j].x; bxy[2 * j + 1] = worlds[j].y; }
        std::vector<std::vector<double> > u(K), v(K), rt(K);
        std::vector<std::vector<int> > vc(K), vb(K), vo(K), vn(K);
        std::vector<tscm_problem> P(K);
        std::vector<unsigned short> fixed(K);
        for (size_t k = 0; k < K; ++k) {
            const TripleSphereCamera &c = *cams[k];
            const int V = (int)pixels[k].size();
            rt[k].assign(6 * (size_t)V, 0.0);
            for (int i = 0; i < V; ++i) {
                if (!c.has_chessboard_[i]) continue;                         // TS.cpp:253
                vc[k].push_back(0); vb[k].push_back(i); vo[k].push_back((int)u[k].size()); vn[k].push_back((int)pixels[k][i].size());
                for (const Point2d &p : pixels[k][i]) { u[k].push_back(p.x); v[k].push_back(p.y); }
                std::memcpy(&rt[k][6 * (size_t)i], c.rt_[i].data(), 6 * sizeof(double));
            }
            tscm_problem &q = P[k];
            q = tscm_problem();
            q.n_cameras = 1; q.n_boards = V; q.n_points = n; q.n_views = (int)vc[k].size();
            q.board_xy = bxy.data(); q.view_camera = vc[k].data(); q.view_board = vb[k].data(); q.view_offset = vo[k].data();
            q.view_count = vn[k].data(); q.obs_u = u[k].data(); q.obs_v = v[k].data(); q.intr = cams[k]->intrinsic_.data();
            q.board_rt = rt[k].data(); q.mono = 1;
            fixed[k] = c.fixed_;
        }
        tscm_options o;
        if (options) o = *options; else tscm_default_options(&o, 1);
        std::vector<tscm_summary> sums(K);
        check(tscm_solve_mono_batch(P.data(), (int)K, cams[0]->device_, &o, fixed.data(), cams[0]->loss_kind_, cams[0]->loss_scale_, sums.data()));
        std::vector<bool> converged(K);
        for (size_t k = 0; k < K; ++k) {
            TripleSphereCamera &c = *cams[k];
            for (size_t i = 0; i < pixels[k].size(); ++i) if (c.has_chessboard_[i]) c.rt_[i].assign(&rt[k][6 * i], &rt[k][6 * i] + 6);
            c.summary = sums[k];
            converged[k] = sums[k].termination_type == TSCM_CONVERGENCE;    // TS.cpp:281
        }
        return converged;
    }

    // TS.cpp:110-168: fx = fy = mean circle-fit focal length; 0 when no row is usable
    double estimate_focal(const std::vector<std::vector<Point2d> > &pixels, Size chessboard_num)
    {
        const int V = (int)pixels.size(), n = chessboard_num.width * chessboard_num.height;
        std::vector<double> u((size_t)V * n, 0.0), v((size_t)V * n, 0.0);
        std::vector<int> cnt(V);
        for (int k = 0; k < V; ++k) {
            cnt[k] = (int)pixels[k].size();
            for (size_t j = 0; j < pixels[k].size() && j < (size_t)n; ++j) { u[(size_t)k * n + j] = pixels[k][j].x; v[(size_t)k * n + j] = pixels[k][j].y; }
        }
        double focal = 0.0; int used = 0;
        check(tscm_estimate_focal(u.data(), v.data(), cnt.data(), V, chessboard_num.width, chessboard_num.height,
                                  intrinsic_[2], intrinsic_[3], device_, &focal, &used));
        intrinsic_[0] = intrinsic_[1] = focal;
        return focal;
    }

    // TS.cpp:170-203 (planar PnP per image with a board; fills Rt_)
    int estimate_extrinsic(const std::vector<std::vector<Point2d> > &pixels, const std::vector<Point3d> &worlds, Size chessboard_num)
    {
        const int V = (int)pixels.size(), n = (int)worlds.size();
        std::vector<double> u((size_t)V * n, 0.0), v((size_t)V * n, 0.0), W(3 * (size_t)n), M(9 * (size_t)V, 0.0);
        std::vector<int> cnt(V);
        for (int c = 0; c < n; ++c) { W[3 * c] = worlds[c].x; W[3 * c + 1] = worlds[c].y; W[3 * c + 2] = worlds[c].z; }
        for (int k = 0; k < V; ++k) {
            cnt[k] = has_chessboard_[k] ? (int)pixels[k].size() : 0;                // TS.cpp:174
            for (size_t j = 0; j < pixels[k].size() && j < (size_t)n; ++j) { u[(size_t)k * n + j] = pixels[k][j].x; v[(size_t)k * n + j] = pixels[k][j].y; }
        }
        int done = 0;
        check(tscm_estimate_extrinsic(intrinsic_.data(), u.data(), v.data(), cnt.data(), V, W.data(), n, chessboard_num.width, device_, M.data(), &done));
        Rt_.resize(V);
        for (int k = 0; k < V; ++k) if (cnt[k]) std::memcpy(Rt_[k].a, &M[9 * (size_t)k], sizeof(Rt_[k].a));
        return done;
    }

    // The same step with tscm_estimate_extrinsic_ransac (a consensus search over 4-corner homographies and a refit on the
    // winner's inliers, see tscm.h): fills Rt_ for the views with exit code 5..7, ransac_code_ for every view, and *inliers
    // (may be NULL) with one 0/1 flag per corner and view.  params NULL: the library's defaults.  Returns the poses written.
    int estimate_extrinsic_ransac(const std::vector<std::vector<Point2d> > &pixels, const std::vector<Point3d> &worlds, Size chessboard_num,
                                  const tscm_ransac_params *params = NULL, std::vector<std::vector<unsigned char> > *inliers = NULL)
    {
        const int V = (int)pixels.size(), n = (int)worlds.size();
        std::vector<double> u((size_t)V * n, 0.0), v((size_t)V * n, 0.0), W(3 * (size_t)n), M(9 * (size_t)V, 0.0);
        std::vector<int> cnt(V), n_in(V);
        std::vector<unsigned char> mask((size_t)V * n, 0);
        for (int c = 0; c < n; ++c) { W[3 * c] = worlds[c].x; W[3 * c + 1] = worlds[c].y; W[3 * c + 2] = worlds[c].z; }
        for (int k = 0; k < V; ++k) {
            cnt[k] = has_chessboard_[k] ? (int)pixels[k].size() : 0;
            for (size_t j = 0; j < pixels[k].size() && j < (size_t)n; ++j) { u[(size_t)k * n + j] = pixels[k][j].x; v[(size_t)k * n + j] = pixels[k][j].y; }
        }
        tscm_ransac_params def;
        tscm_ransac_default_params(&def);
        int done = 0;
        ransac_code_.assign(V, 0);
        check(tscm_estimate_extrinsic_ransac(intrinsic_.data(), u.data(), v.data(), cnt.data(), V, W.data(), n, chessboard_num.width, params ? params : &def,
                                             device_, M.data(), mask.data(), n_in.data(), ransac_code_.data(), &done, NULL));
        Rt_.resize(V);
        for (int k = 0; k < V; ++k)
            if (ransac_code_[k] >= TSCM_EXTRINSIC_CONVERGED && ransac_code_[k] <= TSCM_EXTRINSIC_GN_CHOLESKY) std::memcpy(Rt_[k].a, &M[9 * (size_t)k], sizeof(Rt_[k].a));
        if (inliers) {
            inliers->assign(V, std::vector<unsigned char>());
            for (int k = 0; k < V; ++k) (*inliers)[k].assign(mask.begin() + (size_t)k * n, mask.begin() + (size_t)(k + 1) * n);
        }
        return done;
    }
    // calibrate() takes its start poses from estimate_extrinsic_ransac with *params (NULL: from estimate_extrinsic again, the
    // default), clears has_chessboard_ for the views without a pose there, and keeps the masks in ransac_inliers_.
    // mask_outliers: calibrate() and every refinement() behind it pass ransac_inliers_ as the corner mask (set_corner_weights):
    // a corner outside the consensus set is taken out of the refinement.
    void set_ransac(const tscm_ransac_params *params, bool mask_outliers = false)
    {
        use_ransac_ = params != NULL;
        mask_outliers_ = use_ransac_ && mask_outliers;
        if (params) ransac_ = *params;
    }
    std::vector<int> ransac_code_;                                    // TSCM_EXTRINSIC_* per view of the last estimate_extrinsic_ransac
    std::vector<std::vector<unsigned char> > ransac_inliers_;         // per view and corner, of the last calibrate() with set_ransac

    // TS.cpp:30-105: initial guess (unless a previous calibration succeeded), poses, refinement
    bool calibrate(const std::vector<std::vector<Point2d> > &pixels, const std::vector<bool> &has_chessboard,
                   const std::vector<Point3d> &worlds, Size img_size, Size chessboard_num)
    {
        pixels_ = pixels;
        has_chessboard_ = has_chessboard;
        Rt_.assign(pixels.size(), Mat33());
        rt_.assign(pixels.size(), std::vector<double>());
        if (!has_init_guess_) {
            intrinsic_.assign(9, 0.0);
            intrinsic_[2] = img_size.width / 2 - 0.5;                                // :43-47
            intrinsic_[3] = img_size.height / 2 - 0.5;
            intrinsic_[6] = 0.5;
            if (estimate_focal(pixels, chessboard_num) == 0.0) return false;          // :48-50
        }
        if (use_ransac_) {
            estimate_extrinsic_ransac(pixels, worlds, chessboard_num, &ransac_, &ransac_inliers_);
            for (size_t i = 0; i < has_chessboard_.size(); ++i)
                if (ransac_code_[i] < TSCM_EXTRINSIC_CONVERGED || ransac_code_[i] > TSCM_EXTRINSIC_GN_CHOLESKY) has_chessboard_[i] = false;
        } else {
            estimate_extrinsic(pixels, worlds, chessboard_num);                       // :52
        }
        poses_from_Rt();                                                              // :62-74
        const bool status = refinement(pixels, worlds);                               // :76-78
        if (status) has_init_guess_ = true;
        for (size_t i = 0; i < Rt_.size(); ++i) {                                     // :88-102: Rt_ from the refined rt_
            if (!has_chessboard_[i]) continue;
            const Mat33 R = rodrigues(rt_[i].data());
            for (int r = 0; r < 3; ++r) { Rt_[i].a[3 * r] = R.a[3 * r]; Rt_[i].a[3 * r + 1] = R.a[3 * r + 1]; Rt_[i].a[3 * r + 2] = rt_[i][3 + r]; }
        }
        return status;
    }
    bool has_init_guess_ = false;
    int loss_kind_ = TSCM_LOSS_NONE;
    double loss_scale_ = 0.0;
    unsigned short fixed_ = 0;
    bool use_ransac_ = false;                 // set_ransac()
    bool mask_outliers_ = false;
    tscm_ransac_params ransac_;
    bool use_weights_ = false;                // set_corner_weights()
    std::vector<std::vector<double> > corner_weights_;
    bool use_priors_ = false, use_sigmas_ = false;      // set_camera_priors(), set_prior_sigmas()
    CameraPriors priors_;
    double prior_sigma_[7] = { 0, 0, 0, 0, 0, 0, 0 };

    // TS.cpp:62-74
    void poses_from_Rt()
    {
        const int V = (int)Rt_.size();
        std::vector<double> M(9 * (size_t)V), rt(6 * (size_t)V, 0.0);
        std::vector<unsigned char> has(V);
        for (int i = 0; i < V; ++i) { std::memcpy(&M[9 * (size_t)i], Rt_[i].a, sizeof(Rt_[i].a)); has[i] = has_chessboard_[i] ? 1 : 0; }
        check(tscm_poses_from_r1r2t(M.data(), has.data(), V, rt.data()));
        rt_.resize(V);
        for (int i = 0; i < V; ++i) if (has[i]) rt_[i].assign(&rt[6 * (size_t)i], &rt[6 * (size_t)i] + 6);
    }

    // TS.cpp:332-344 for a batch of points
    std::vector<Point2d> project(const std::vector<Point3d> &P) const
    {
        std::vector<Point2d> out(P.size());
        if (!P.empty()) check(tscm_project_points(intrinsic_.data(), &P[0].x, (int)P.size(), device_, &out[0].x));
        return out;
    }
    Point2d project(const Point3d &P) const { return project(std::vector<Point3d>(1, P))[0]; }

    // TS.h:39-57 for a batch of pixels (transform == nullptr: identity)
    std::vector<Point3d> get_unit_sphere_coordinate(const std::vector<Point2d> &pixels, const Mat33 *transform = nullptr) const
    {
        std::vector<Point3d> out(pixels.size());
        if (pixels.empty()) return out;
        check(tscm_unproject_pixels(intrinsic_.data(), &pixels[0].x, (int)pixels.size(), device_, &out[0].x));
        if (transform)
            for (Point3d &p : out) {                                     // TS.h:54-55
                const double *T = transform->a, x = p.x, y = p.y, z = p.z;
                p.x = T[0] * x + T[1] * y + T[2] * z; p.y = T[3] * x + T[4] * y + T[5] * z; p.z = T[6] * x + T[7] * y + T[8] * z;
            }
        return out;
    }

    // TS.cpp:284-306; mapx / mapy: img_size.height x img_size.width floats (CV_32FC1 layout)
    void undistort(double fx, double fy, double cx, double cy, Size img_size, std::vector<float> &mapx, std::vector<float> &mapy, bool exact = true) const
    {
        tscm_map_desc d = tscm_map_desc();
        std::memcpy(d.intr, intrinsic_.data(), sizeof(d.intr));
        d.R[0] = d.R[4] = d.R[8] = 1.0;
        d.fx = fx; d.fy = fy; d.cx = cx; d.cy = cy;
        d.width = img_size.width; d.height = img_size.height; d.out_stride = img_size.width;
        const size_t n = (size_t)img_size.width * img_size.height;
        mapx.assign(n, 0.f); mapy.assign(n, 0.f);
        check(tscm_build_maps(&d, 1, device_, exact ? 1 : 0, mapx.data(), mapy.data(), n, nullptr));
    }

    // undistort with an output image of kind `projection` (TSCM_PROJ_*: fx, fy are pixels per radian for the angle kinds)
    void undistort(double fx, double fy, double cx, double cy, Size img_size, std::vector<float> &mapx, std::vector<float> &mapy, bool exact, int projection) const
    {
        tscm_map_desc d = tscm_map_desc();
        std::memcpy(d.intr, intrinsic_.data(), sizeof(d.intr));
        d.R[0] = d.R[4] = d.R[8] = 1.0;
        d.fx = fx; d.fy = fy; d.cx = cx; d.cy = cy;
        d.width = img_size.width; d.height = img_size.height; d.out_stride = img_size.width;
        const size_t n = (size_t)img_size.width * img_size.height;
        mapx.assign(n, 0.f); mapy.assign(n, 0.f);
        check(tscm_build_maps_ex(&d, &projection, 1, device_, exact ? 1 : 0, mapx.data(), mapy.data(), n, nullptr));
    }

    // where a pixel of this camera lands in the output image (fx, fy, cx, cy, R, projection) of undistort / a rectification
    // table (R == nullptr: identity); false when it has no place there (tscm.h: tscm_rectify_points)
    bool rectify_point(const Point2d &pixel, double fx, double fy, double cx, double cy, const Mat33 *R, int projection, Point2d &out) const
    {
        tscm_map_desc d = tscm_map_desc();
        std::memcpy(d.intr, intrinsic_.data(), sizeof(d.intr));
        if (R) std::memcpy(d.R, R->a, sizeof(d.R));
        else d.R[0] = d.R[4] = d.R[8] = 1.0;
        d.fx = fx; d.fy = fy; d.cx = cx; d.cy = cy;
        unsigned char valid = 0;
        check(tscm_rectify_points(&d, projection, &pixel.x, 1, device_, &out.x, &valid));
        return valid != 0;
    }

    // the table of undistort_chessboard(src, index, chessboard, chessboard_size), TS.cpp:308-328
    Size undistort_chessboard_maps(int index, Size chessboard, double chessboard_size, std::vector<float> &mapx, std::vector<float> &mapy,
                                   bool exact = true) const
    {
        Size img = { (int)((chessboard.width + 1) * chessboard_size), (int)((chessboard.height + 1) * chessboard_size) };
        mapx.clear(); mapy.clear();
        if (!has_chessboard_[index]) { img.width = img.height = 0; return img; }       // TS.cpp:311-312
        tscm_map_desc d = tscm_map_desc();
        std::memcpy(d.intr, intrinsic_.data(), sizeof(d.intr));
        std::memcpy(d.R, Rt_[index].a, sizeof(d.R));
        d.fx = d.fy = 1.0; d.cx = d.cy = chessboard_size;
        d.width = img.width; d.height = img.height; d.out_stride = img.width;
        const size_t n = (size_t)img.width * img.height;
        mapx.assign(n, 0.f); mapy.assign(n, 0.f);
        check(tscm_build_maps(&d, 1, device_, exact ? 1 : 0, mapx.data(), mapy.data(), n, nullptr));
        return img;
    }

    // undistort_chessboard(src, index, chessboard, chessboard_size) (TS.cpp:308-330): table + cv::remap(INTER_LINEAR) of an
    // 8-bit image with `channels` interleaved channels (1 or 3); dst gets img.height rows of img.width * channels bytes
    // (empty when the view has no board).  to_gray: BGR input, grey output (what findCorner does next, findCorner.cpp:9-10).
    Size undistort_chessboard(const unsigned char *src, int width, int height, int stride, int channels, int index, Size chessboard, double chessboard_size,
                              std::vector<unsigned char> &dst, bool to_gray = false) const
    {
        std::vector<float> mapx, mapy;
        const Size img = undistort_chessboard_maps(index, chessboard, chessboard_size, mapx, mapy);
        dst.clear();
        if (img.width == 0) return img;
        const int out_ch = (to_gray || channels == 1) ? 1 : channels;
        dst.assign((size_t)img.width * img.height * out_ch, 0);
        check(tscm_remap(src, width, height, stride, channels, mapx.data(), mapy.data(), img.width, img.height, img.width, to_gray ? 1 : 0, device_, dst.data(),
                         img.width * out_ch));
        return img;
    }

    int device() const { return device_; }

private:
    int device_;
};

// What the calibration demos print behind a calibrate() with set_ransac: of the views offered (has), those that kept a pose,
// and the share of inlier corners in them.  camera < 0: no "camera N:" in front.
inline void print_ransac_summary(const TripleSphereCamera &cam, const std::vector<bool> &has, int camera)
{
    size_t offered = 0, kept = 0, corners = 0, inliers = 0;
    for (size_t i = 0; i < has.size(); ++i) {
        offered += has[i] ? 1 : 0;
        if (!has[i] || i >= cam.has_chessboard_.size() || !cam.has_chessboard_[i]) continue;
        ++kept;
        for (size_t j = 0; j < cam.ransac_inliers_[i].size(); ++j) { ++corners; inliers += cam.ransac_inliers_[i][j] ? 1 : 0; }
    }
    if (camera >= 0) std::printf("camera %d: ", camera);
    std::printf("ransac kept %zu of %zu views, %.1f %% of their corners are inliers\n", kept, offered, corners ? 100.0 * inliers / corners : 0.0);
}

// Behind calibrate() calls with set_ransac(params, true): the cameras' inlier masks as the weights of
// MultiCalib::set_corner_weights (weights[m][i][j] = 1 for an inlier, 0 otherwise; a view without a mask gets none)
inline std::vector<std::vector<std::vector<double> > > ransac_corner_masks(const std::vector<TripleSphereCamera> &cameras)
{
    std::vector<std::vector<std::vector<double> > > w(cameras.size());
    for (size_t m = 0; m < cameras.size(); ++m) {
        w[m].resize(cameras[m].ransac_inliers_.size());
        for (size_t i = 0; i < w[m].size(); ++i) w[m][i].assign(cameras[m].ransac_inliers_[i].begin(), cameras[m].ransac_inliers_[i].end());
    }
    return w;
}
// ... and what the demos print with --ransac-mask: the corners of the kept views that the mask takes out of the refinements
inline void print_ransac_masked(const TripleSphereCamera &cam, int camera)
{
    size_t corners = 0, masked = 0;
    for (size_t i = 0; i < cam.ransac_inliers_.size(); ++i) {
        if (i >= cam.has_chessboard_.size() || !cam.has_chessboard_[i]) continue;
        for (size_t j = 0; j < cam.ransac_inliers_[i].size(); ++j) { ++corners; masked += cam.ransac_inliers_[i][j] ? 0 : 1; }
    }
    if (camera >= 0) std::printf("camera %d: ", camera);
    std::printf("ransac mask takes out %zu of %zu corners\n", masked, corners);
}

// multi_calib.h:8-83
class MultiCalib_camera {
public:
    MultiCalib_camera() : intrinsic_(9, 0.0), rt_(6, 0.0), is_initial_(false) {}
    std::vector<double> intrinsic_, rt_;
    bool is_initial() const { return is_initial_; }
    const Mat33 &R() const { return R_; }
    const double *t() const { return t_; }
    double fx() const { return intrinsic_[0]; }
    double fy() const { return intrinsic_[1]; }
    double cx() const { return intrinsic_[2]; }
    double cy() const { return intrinsic_[3]; }
    double xi() const { return intrinsic_[4]; }
    double lamda() const { return intrinsic_[5]; }
    double alpha() const { return intrinsic_[6]; }
    double b() const { return intrinsic_[7]; }
    double c() const { return intrinsic_[8]; }
    const std::vector<std::vector<Point2d> > &pixels() const { return pixel_coordinates_; }
    bool has_chessboard(int j) const { return has_chessboard_[j]; }
    void update_param() { R_ = rodrigues(rt_.data()); std::memcpy(t_, &rt_[3], sizeof(t_)); }       // multi_calib.h:42-57
private:
    friend class MultiCalib;
    std::vector<bool> has_chessboard_;
    std::vector<std::vector<Point2d> > pixel_coordinates_;
    Mat33 R_;
    double t_[3];
    bool is_initial_;
};

// multi_calib.h:85-117
class MultiCalib_chessboard {
public:
    MultiCalib_chessboard() : rt_(6, 0.0), is_initial_(false) {}
    std::vector<double> rt_;
    bool is_initial() const { return is_initial_; }
    const Mat33 &R() const { return R_; }
    const double *t() const { return t_; }
    void update_param() { R_ = rodrigues(rt_.data()); std::memcpy(t_, &rt_[3], sizeof(t_)); }       // multi_calib.h:104-108
private:
    friend class MultiCalib;
    Mat33 R_;
    double t_[3];
    bool is_initial_;
};

// multi_calib.h:119-129
class MultiCalib {
public:
    // multi_calib.cpp:6-153: rig chaining and board-pose selection on the device
    MultiCalib(const std::vector<TripleSphereCamera> &cameras, const std::vector<Point3d> &worlds, int device = 0)
        : worlds_(worlds), mean_error(0.0), device_(device)
    {
        const int C = (int)cameras.size(), B = C ? (int)cameras[0].has_chessboard_.size() : 0, n = (int)worlds.size();
        std::vector<double> W(3 * (size_t)n), I(9 * (size_t)C), Rt(9 * (size_t)C * B, 0.0), pu((size_t)C * B * n, 0.0), pv((size_t)C * B * n, 0.0);
        std::vector<unsigned char> has((size_t)C * B, 0);
        for (int c = 0; c < n; ++c) { W[3 * c] = worlds[c].x; W[3 * c + 1] = worlds[c].y; W[3 * c + 2] = worlds[c].z; }
        for (int m = 0; m < C; ++m) {
            std::memcpy(&I[9 * (size_t)m], cameras[m].intrinsic_.data(), 9 * sizeof(double));
            for (int j = 0; j < B; ++j) {
                if (!cameras[m].has_chessboard_[j]) continue;
                has[(size_t)m * B + j] = 1;
                std::memcpy(&Rt[9 * ((size_t)m * B + j)], cameras[m].Rt_[j].a, 9 * sizeof(double));
                for (int c = 0; c < n; ++c) { pu[((size_t)m * B + j) * n + c] = cameras[m].pixels_[j][c].x; pv[((size_t)m * B + j) * n + c] = cameras[m].pixels_[j][c].y; }
            }
        }
        std::vector<double> cR(9 * (size_t)C), ct(3 * (size_t)C), crt(6 * (size_t)C), bR(9 * (size_t)B), bt(3 * (size_t)B), brt(6 * (size_t)B);
        std::vector<unsigned char> init(B);
        tscm_rig_input in = { C, B, n, W.data(), I.data(), has.data(), Rt.data(), pu.data(), pv.data() };
        tscm_rig_result out = tscm_rig_result();
        out.cam_R = cR.data(); out.cam_t = ct.data(); out.cam_rt = crt.data();
        out.board_R = bR.data(); out.board_t = bt.data(); out.board_rt = brt.data(); out.board_initial = init.data();
        check(tscm_rig_init(&in, device_, &out));
        cameras_.resize(C); chessboards_.resize(B);
        for (int m = 0; m < C; ++m) {                                    // MultiCalib_camera(camera, R, t), multi_calib.h:10-37
            MultiCalib_camera &cam = cameras_[m];
            cam.intrinsic_ = cameras[m].intrinsic_;
            cam.has_chessboard_ = cameras[m].has_chessboard_;
            cam.pixel_coordinates_ = cameras[m].pixels_;
            std::memcpy(cam.R_.a, &cR[9 * (size_t)m], sizeof(cam.R_.a)); std::memcpy(cam.t_, &ct[3 * (size_t)m], sizeof(cam.t_));
            cam.rt_.assign(&crt[6 * (size_t)m], &crt[6 * (size_t)m] + 6);
            cam.is_initial_ = true;
        }
        for (int j = 0; j < B; ++j) {                                    // multi_calib.h:88-97
            MultiCalib_chessboard &cb = chessboards_[j];
            cb.is_initial_ = init[j] != 0;
            if (!cb.is_initial_) continue;
            std::memcpy(cb.R_.a, &bR[9 * (size_t)j], sizeof(cb.R_.a)); std::memcpy(cb.t_, &bt[3 * (size_t)j], sizeof(cb.t_));
            cb.rt_.assign(&brt[6 * (size_t)j], &brt[6 * (size_t)j] + 6);
        }
    }

    // Several GPUs, one process per GPU (no counterpart in the reference): rank / world of this process and the
    // communicator made from rank 0's tscm_comm_unique_id (tscm_comm_create).  calibrate() then shards the frames.
    void set_sharding(int rank, int world, tscm_comm *comm) { rank_ = rank; world_ = world; comm_ = comm; }
    // the loss of every residual block of calibrate() (see TripleSphereCamera::set_loss); with sharding every rank must set the same
    void set_loss(int kind, double scale) { loss_kind_ = kind; loss_scale_ = scale; }
    // intrinsics of camera m that calibrate() holds (TripleSphereCamera::set_fixed_intrinsics); with sharding every rank must set the same
    void set_fixed_intrinsics(int m, unsigned short fixed)
    {
        if (fixed_.size() < (size_t)m + 1) fixed_.resize((size_t)m + 1, 0);
        fixed_[(size_t)m] = fixed;
    }

    // corner weights of calibrate() and covariance() (TripleSphereCamera::set_corner_weights): weights[m][i][j] for corner j of
    // board i in camera m, shaped like the cameras' pixel_coordinates_; NULL = none.  A view whose weights are all 0 is left out.
    // With sharding every rank must set the same.
    void set_corner_weights(const std::vector<std::vector<std::vector<double> > > *weights)
    {
        use_weights_ = weights != NULL;
        corner_weights_ = weights ? *weights : std::vector<std::vector<std::vector<double> > >();
    }
    // Gaussian priors of calibrate() and covariance() (tscm.h, "Gaussian priors"): cam_rt_* [C*6] on the cameras' rt_, intr_*
    // [C*9] on their intrinsic_; NULL = none.  Copied.  Camera 0's pose is constant and held intrinsics are not free: their
    // weights count for nothing.  Not with sharding (set_sharding with more than one rank): calibrate() then throws.
    void set_camera_priors(const CameraPriors *priors)
    {
        use_priors_ = priors != NULL;
        priors_ = priors ? *priors : CameraPriors();
    }
    double corner_weight(size_t m, size_t i, size_t j) const
    {
        return m < corner_weights_.size() && i < corner_weights_[m].size() && j < corner_weights_[m][i].size() ? corner_weights_[m][i][j] : 0.0;
    }

    // the problem of multi_calib.cpp:157-207 at the objects' current parameters (the arrays P points into live in here)
    struct JointProblem {
        std::vector<double> bxy, u, v, w, crt, I, brt;
        std::vector<int> vc, vb, vo, vn;
        std::vector<unsigned char> cc;
        std::vector<unsigned short> fixed;
        bool any_fixed;
        tscm_problem P;
    };
    void joint_problem(JointProblem &q) const
    {
        const int C = (int)cameras_.size(), B = (int)chessboards_.size(), n = (int)worlds_.size();
        q.bxy.assign(2 * (size_t)n, 0.0); q.crt.assign(6 * (size_t)C, 0.0); q.I.assign(9 * (size_t)C, 0.0); q.brt.assign(6 * (size_t)B, 0.0);
        q.cc.assign(C, 0);
        for (int j = 0; j < n; ++j) { q.bxy[2 * j] = worlds_[j].x; q.bxy[2 * j + 1] = worlds_[j].y; }
        for (int m = 0; m < C; ++m)                                      // :162-207: camera m, board i, corner j
            for (int i = 0; i < B; ++i) {
                if (!chessboards_[i].is_initial() || cameras_[m].pixel_coordinates_[i].empty()) continue;
                if (use_weights_) {
                    const size_t nj = cameras_[m].pixel_coordinates_[i].size();
                    bool any = false;
                    for (size_t j = 0; j < nj; ++j) any = any || corner_weight((size_t)m, (size_t)i, j) != 0.0;
                    if (!any) continue;                                  // every weight 0: no residual block of this view
                    for (size_t j = 0; j < nj; ++j) q.w.push_back(corner_weight((size_t)m, (size_t)i, j));
                }
                q.vc.push_back(m); q.vb.push_back(i); q.vo.push_back((int)q.u.size()); q.vn.push_back((int)cameras_[m].pixel_coordinates_[i].size());
                for (const Point2d &p : cameras_[m].pixel_coordinates_[i]) { q.u.push_back(p.x); q.v.push_back(p.y); }
            }
        for (int m = 0; m < C; ++m) { std::memcpy(&q.crt[6 * (size_t)m], cameras_[m].rt_.data(), 6 * sizeof(double)); std::memcpy(&q.I[9 * (size_t)m], cameras_[m].intrinsic_.data(), 9 * sizeof(double)); }
        for (int i = 0; i < B; ++i) if (chessboards_[i].is_initial()) std::memcpy(&q.brt[6 * (size_t)i], chessboards_[i].rt_.data(), 6 * sizeof(double));
        if (C) q.cc[0] = 1;                                              // SetParameterBlockConstant(cameras_[0].rt_), :186
        tscm_problem &P = q.P;
        P = tscm_problem();
        P.n_cameras = C; P.n_boards = B; P.n_points = n; P.n_views = (int)q.vc.size();
        P.board_xy = q.bxy.data(); P.view_camera = q.vc.data(); P.view_board = q.vb.data(); P.view_offset = q.vo.data(); P.view_count = q.vn.data();
        P.obs_u = q.u.data(); P.obs_v = q.v.data(); P.cam_rt = q.crt.data(); P.intr = q.I.data(); P.board_rt = q.brt.data();
        P.cam_pose_constant = q.cc.data(); P.mono = 0;
        q.fixed.assign(C, 0);
        q.any_fixed = false;
        for (int m = 0; m < C && m < (int)fixed_.size(); ++m) { q.fixed[m] = fixed_[m]; q.any_fixed = q.any_fixed || fixed_[m] != 0; }
    }

    // multi_calib.cpp:155-283: joint LM, write-back (update_param), reprojection-error report
    void calibrate(const tscm_options *options = nullptr)
    {
        const int C = (int)cameras_.size(), B = (int)chessboards_.size();
        JointProblem q;
        joint_problem(q);
        tscm_problem &P = q.P;
        std::vector<double> &crt = q.crt, &I = q.I, &brt = q.brt;
        std::vector<unsigned short> &fixed = q.fixed;
        const bool any_fixed = q.any_fixed;
        tscm_options o;
        if (options) o = *options; else tscm_default_options(&o, 0);
        const tscm_camera_priors cp = priors_.c_struct();
        if (comm_) {
            // frame-sharded over the ranks of set_sharding(): every rank builds this same problem, keeps the boards it owns
            // and ends with ALL parameters updated (tscm.h, "multi-GPU").  (A one-rank communicator is legal: the library
            // then solves as if there were none, unless the options carry TSCM_EXEC_KEEP_SINGLE_RANK_COMM.)
            tscm_solver *s = nullptr;
            check(tscm_solver_create_sharded(&P, device_, rank_, world_, &s));
            int rc = tscm_solver_set_comm(s, comm_);
            if (rc == 0) rc = tscm_solver_set_loss(s, loss_kind_, loss_scale_);
            if (rc == 0 && any_fixed) rc = tscm_solver_set_fixed_intrinsics(s, fixed.data());
            if (rc == 0 && use_weights_) rc = tscm_solver_set_corner_weights(s, q.w.data());
            if (rc == 0 && use_priors_) rc = tscm_solver_set_camera_priors(s, &cp);
            if (rc == 0) rc = tscm_solver_solve(s, &o, &summary);
            tscm_solver_destroy(s);
            check(rc);
        } else {
            check(tscm_solve_prior(&P, &o, use_weights_ ? q.w.data() : nullptr, any_fixed ? fixed.data() : nullptr, loss_kind_, loss_scale_,
                                   use_priors_ ? &cp : nullptr, &summary));
        }
        for (int m = 0; m < C; ++m) {                                    // :221-226
            cameras_[m].rt_.assign(&crt[6 * (size_t)m], &crt[6 * (size_t)m] + 6);
            cameras_[m].intrinsic_.assign(&I[9 * (size_t)m], &I[9 * (size_t)m] + 9);
            if (cameras_[m].is_initial()) cameras_[m].update_param();
        }
        for (int i = 0; i < B; ++i) {                                    // :227-232
            if (!chessboards_[i].is_initial()) continue;
            chessboards_[i].rt_.assign(&brt[6 * (size_t)i], &brt[6 * (size_t)i] + 6);
            chessboards_[i].update_param();
        }
        camera_error.assign(C, 0.0);                                     // :233-283
        double rmse = 0.0;
        check(tscm_reprojection_error(&P, device_, camera_error.data(), &mean_error, &rmse));
    }

    // What ceres::Covariance would give for the joint problem at the objects' current parameters (tscm_covariance), with the
    // loss and held intrinsics set on this object: call it after calibrate().  Ceres' convention: the blocks are (J^T J)^-1,
    // not multiplied by sigma2; the standard deviations are.  status != 0: a singular block, every vector NaN (tscm.h).
    struct Covariance {
        tscm_covariance_info info;
        double sigma2;
        std::vector<double> cam_cov;           // [C*15][C*15], a camera's columns: rt (6), intrinsic (9)
        std::vector<double> board_cov;         // [B][6][6]
        std::vector<double> cam_rt_std, intr_std, board_rt_std;      // [C*6], [C*9], [B*6]; 0 where the column is not free
    };
    Covariance covariance() const
    {
        const size_t C = cameras_.size(), B = chessboards_.size();
        JointProblem q;
        joint_problem(q);
        Covariance out;
        out.cam_cov.assign(15 * C * 15 * C, 0.0); out.board_cov.assign(36 * B, 0.0);
        out.cam_rt_std.assign(6 * C, 0.0); out.intr_std.assign(9 * C, 0.0); out.board_rt_std.assign(6 * B, 0.0);
        out.info = tscm_covariance_info();
        out.info.struct_size = (int)sizeof(tscm_covariance_info);
        const tscm_camera_priors cp = priors_.c_struct();
        check(tscm_covariance_prior(&q.P, device_, q.any_fixed ? q.fixed.data() : nullptr, use_weights_ ? q.w.data() : nullptr, loss_kind_, loss_scale_,
                                    use_priors_ ? &cp : nullptr, out.cam_cov.data(), out.board_cov.data(), out.cam_rt_std.data(), out.intr_std.data(), out.board_rt_std.data(), &out.info));
        out.sigma2 = out.info.sigma2;
        return out;
    }

    // Residual report (tscm_residual_report) of the joint problem at the objects' current parameters, with the weights set on
    // this object (a view whose weights are all 0 is not part of the joint problem) and, unless params carries one, its loss:
    // call it after calibrate().  The report's view_camera / view_board name each view.  params: NULL = defaults.
    ResidualReport residual_report(const tscm_residual_params *params = nullptr) const
    {
        JointProblem q;
        joint_problem(q);
        tscm_residual_params prm;
        if (params) prm = *params; else { tscm_residual_default_params(&prm); prm.loss_kind = loss_kind_; prm.loss_scale = loss_scale_; }
        return residual_report_of(q.P, device_, use_weights_ ? q.w.data() : nullptr, &prm);
    }
    // Outlier-view pruning (pipeline.prune_solve's flagging step): residual_report(), view_outliers(k, floor, max_fraction), and
    // every corner weight of the flagged views set to 0 (weights of 1 are created if none were set), so that the next calibrate()
    // and covariance() leave those views out.  Returns the flagged (camera, board) pairs, in view order.  No rig-connectivity
    // logic: a pruned rig that falls apart shows in covariance().info.min_pivot_ratio.
    std::vector<std::pair<int, int> > prune_views(double k = 3.0, double floor = 0.0, double max_fraction = 0.2)
    {
        const ResidualReport rep = residual_report();
        const std::vector<bool> flags = view_outliers(rep, k, floor, max_fraction);
        std::vector<std::pair<int, int> > out;
        for (size_t v = 0; v < flags.size(); ++v)
            if (flags[v]) out.push_back(std::make_pair(rep.view_camera[v], rep.view_board[v]));
        if (out.empty()) return out;
        if (!use_weights_) {
            corner_weights_.assign(cameras_.size(), std::vector<std::vector<double> >());
            for (size_t m = 0; m < cameras_.size(); ++m) {
                corner_weights_[m].resize(cameras_[m].pixel_coordinates_.size());
                for (size_t i = 0; i < corner_weights_[m].size(); ++i) corner_weights_[m][i].assign(cameras_[m].pixel_coordinates_[i].size(), 1.0);
            }
            use_weights_ = true;
        }
        for (const std::pair<int, int> &mb : out) {
            std::vector<std::vector<double> > &cam = corner_weights_[(size_t)mb.first];
            if (cam.size() <= (size_t)mb.second) cam.resize((size_t)mb.second + 1);
            cam[(size_t)mb.second].assign(cameras_[(size_t)mb.first].pixel_coordinates_[(size_t)mb.second].size(), 0.0);
        }
        return out;
    }

    // Projection uncertainty maps (tscm_projection_uncertainty) at the objects' current parameters under the covariance that
    // covariance() returned: per request (camera_a, camera_b, inv_distance) the covariance of a grid pixel of camera a
    // transferred to camera b (a == b: of a fixed rig-frame point in its own camera), in pixels.
    struct Uncertainty {
        int nx, ny, n_requests;
        std::vector<double> planes;            // [n_requests][7][ny][nx]: u_b v_b c_uu c_uv c_vv sd_worst sd_across
        std::vector<unsigned char> flags;      // [n_requests][ny][nx]: bit 0 unprojects, 1 projects, 2 inside camera b's image
        std::vector<double> max_sd;            // [n_requests]: the largest sd_worst of the valid pixels
        std::vector<long long> n_valid;        // [n_requests]
        const double *plane(int request, int k) const { return planes.data() + ((size_t)request * 7 + k) * (size_t)nx * ny; }
    };
    Uncertainty projection_uncertainty(const Covariance &cov, tscm_uncertainty_grid grid, const std::vector<tscm_uncertainty_request> &requests) const
    {
        const size_t C = cameras_.size(), R = requests.size();
        std::vector<double> crt(6 * C), I(9 * C);
        for (size_t m = 0; m < C; ++m) { std::memcpy(&crt[6 * m], cameras_[m].rt_.data(), 6 * sizeof(double)); std::memcpy(&I[9 * m], cameras_[m].intrinsic_.data(), 9 * sizeof(double)); }
        grid.struct_size = (int)sizeof(tscm_uncertainty_grid);
        Uncertainty out;
        out.nx = grid.nx; out.ny = grid.ny; out.n_requests = (int)R;
        const size_t npix = (size_t)(grid.nx > 0 ? grid.nx : 0) * (size_t)(grid.ny > 0 ? grid.ny : 0);
        out.planes.assign(R * 7 * npix + 1, 0.0); out.flags.assign(R * npix + 1, 0);
        out.max_sd.assign(R + 1, 0.0); out.n_valid.assign(R + 1, 0);
        check(tscm_projection_uncertainty((int)C, crt.data(), I.data(), cov.cam_cov.data(), cov.sigma2, &grid, requests.data(), (int)R, device_, out.planes.data(),
                                          out.flags.data(), out.max_sd.data(), out.n_valid.data()));
        out.planes.resize(R * 7 * npix); out.flags.resize(R * npix); out.max_sd.resize(R); out.n_valid.resize(R);
        return out;
    }
    // the grid of the CLI and of pipeline.calibrate_rig: x, y = 0, step, 2 step, ... inside a width x height image
    static tscm_uncertainty_grid image_grid(int width, int height, double step)
    {
        tscm_uncertainty_grid g = tscm_uncertainty_grid();
        g.struct_size = (int)sizeof(tscm_uncertainty_grid);
        g.nx = (int)std::floor((width - 1) / step) + 1; g.ny = (int)std::floor((height - 1) / step) + 1;
        g.width_b = width; g.height_b = height;
        g.x0 = 0.0; g.y0 = 0.0; g.dx = step; g.dy = step;
        return g;
    }
    // the requests of the CLI and of pipeline.calibrate_rig: an observe request per camera (at the first inverse distance), then
    // per inverse distance a transfer request per ordered pair of adjacent cameras (m, m + 1; with three and more also last, first)
    std::vector<tscm_uncertainty_request> uncertainty_requests(const std::vector<double> &inv_distances) const
    {
        const int C = (int)cameras_.size();
        std::vector<tscm_uncertainty_request> req;
        for (int m = 0; m < C; ++m) req.push_back(tscm_uncertainty_request{ m, m, inv_distances.empty() ? 0.0 : inv_distances[0] });
        for (double i : inv_distances)
            for (int m = 0; m < (C > 2 ? C : C - 1); ++m) {
                const int b = (m + 1) % C;
                req.push_back(tscm_uncertainty_request{ m, b, i });
                req.push_back(tscm_uncertainty_request{ b, m, i });
            }
        return req;
    }

    // Next-best view (tscm_view_gain) at the objects' current parameters under the covariance that covariance() returned:
    // what a view of the board at each candidate pose (rig frame) would remove from the camera covariance.  image: every
    // camera's image size; weights: [C*15] of gain_trace, empty for 1 / variance.
    struct ViewGain {
        std::vector<double> gain_logdet, gain_trace;   // [n_candidates]
        std::vector<int> n_visible;                    // [n_candidates][2]
        std::vector<int> flags;                        // [n_candidates]: bit 0 / 1 camera a / b contributes, 2 numbers, 3 a pivot failed
        std::vector<double> cam_cov;                   // view_gain_apply only: [C*15][C*15], the covariance after the view
    };
    ViewGain view_gain(const Covariance &cov, const std::vector<tscm_view_candidate> &candidates, Size image, double border = 0.0, int min_corners = 8,
                       const std::vector<double> &weights = std::vector<double>()) const
    {
        return view_gain_on(cov.cam_cov, candidates.data(), (int)candidates.size(), false, image, border, min_corners, weights);
    }
    // one candidate applied (tscm_view_gain_apply) to cam_cov [C*15][C*15] -- covariance().cam_cov or an earlier call's
    // cam_cov: its outputs and the covariance after the view, for greedy planning without a re-solve
    ViewGain view_gain_apply(const std::vector<double> &cam_cov, const tscm_view_candidate &candidate, Size image, double border = 0.0, int min_corners = 8,
                             const std::vector<double> &weights = std::vector<double>()) const
    {
        return view_gain_on(cam_cov, &candidate, 1, true, image, border, min_corners, weights);
    }
    // Greedy next-best views (pipeline.suggest_views): the candidates are, for every camera alone and (pairs) together with the
    // next one, the board centred on the ray of each pixel of a grid_x x grid_y grid of the image at each distance, facing the
    // camera, then tilted by +-tilt_deg about its x and about its y axis; n_views times: score all (view_gain), take the first
    // arg-max of gain_logdet, apply it (view_gain_apply).  Stops early when no candidate has a positive, finite gain.
    struct SuggestedView {
        tscm_view_candidate candidate;
        double pixel[2], distance, tilt_x, tilt_y;   // of the board centre in camera_a, degrees
        double gain_logdet, gain_trace;
        int n_visible[2], flags;
    };
    std::vector<SuggestedView> suggest_views(const Covariance &cov, Size image, int n_views, const std::vector<double> &distances, int grid_x = 6, int grid_y = 4,
                                             double tilt_deg = 25.0, bool pairs = true, double border = 0.0, int min_corners = 8) const
    {
        const int C = (int)cameras_.size();
        double centre[3] = { 0.0, 0.0, 0.0 };
        for (size_t j = 0; j < worlds_.size(); ++j) { centre[0] += worlds_[j].x / (double)worlds_.size(); centre[1] += worlds_[j].y / (double)worlds_.size(); }
        const double tilts[5][2] = { { 0, 0 }, { tilt_deg, 0 }, { -tilt_deg, 0 }, { 0, tilt_deg }, { 0, -tilt_deg } };
        std::vector<double> px;
        for (int j = 0; j < grid_y; ++j)
            for (int i = 0; i < grid_x; ++i) { px.push_back((i + 0.5) * image.width / grid_x - 0.5); px.push_back((j + 0.5) * image.height / grid_y - 0.5); }
        std::vector<SuggestedView> all;
        std::vector<tscm_view_candidate> cands;
        for (int m = 0; m < C; ++m) {
            std::vector<double> rays(3 * px.size() / 2 + 3);
            check(tscm_unproject_pixels(cameras_[m].intrinsic_.data(), px.data(), (int)(px.size() / 2), device_, rays.data()));
            double Rm[9];
            view_rotation(cameras_[m].rt_.data(), Rm);
            for (int second = 0; second < (pairs && C > 1 && (m + 1 < C || C > 2) ? 2 : 1); ++second)
                for (size_t q = 0; q < px.size() / 2; ++q) {
                    const double *z = &rays[3 * q];
                    if (!(z[0] == z[0] && z[1] == z[1] && z[2] == z[2])) continue;
                    for (size_t d = 0; d < distances.size(); ++d)
                        for (int t = 0; t < (tilt_deg != 0.0 ? 5 : 1); ++t) {
                            // the board's frame in the camera: z the ray, x the camera's x (or y) made orthogonal to it, then the tilts
                            const double zn = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
                            const double zz[3] = { z[0] / zn, z[1] / zn, z[2] / zn };
                            const int ax = std::fabs(zz[0]) < 0.9 ? 0 : 1;
                            double x[3] = { -zz[ax] * zz[0], -zz[ax] * zz[1], -zz[ax] * zz[2] };
                            x[ax] += 1.0;
                            const double xn = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
                            for (int k = 0; k < 3; ++k) x[k] /= xn;
                            const double y[3] = { zz[1] * x[2] - zz[2] * x[1], zz[2] * x[0] - zz[0] * x[2], zz[0] * x[1] - zz[1] * x[0] };
                            double Rcb[9] = { x[0], y[0], zz[0], x[1], y[1], zz[1], x[2], y[2], zz[2] }, T[9], tmp[9];
                            const double wx[3] = { tilts[t][0] * 3.14159265358979323846 / 180.0, 0.0, 0.0 }, wy[3] = { 0.0, tilts[t][1] * 3.14159265358979323846 / 180.0, 0.0 };
                            view_rotation(wx, T); view_mul(Rcb, T, tmp); view_rotation(wy, T); view_mul(tmp, T, Rcb);
                            // t_cb = distance * ray - R_cb centre; rig frame: R = R_m^T R_cb, t = R_m^T (t_cb - t_m)
                            double tcb[3], Rrb[9];
                            for (int k = 0; k < 3; ++k) tcb[k] = distances[d] * zz[k] - (Rcb[3 * k] * centre[0] + Rcb[3 * k + 1] * centre[1]) - cameras_[m].rt_[3 + k];
                            for (int r = 0; r < 3; ++r)
                                for (int c = 0; c < 3; ++c) Rrb[3 * r + c] = Rm[r] * Rcb[c] + Rm[3 + r] * Rcb[3 + c] + Rm[6 + r] * Rcb[6 + c];
                            SuggestedView v = SuggestedView();
                            v.candidate.camera_a = m;
                            v.candidate.camera_b = second ? (m + 1) % C : m;
                            view_angle_axis(Rrb, v.candidate.board_rt);
                            for (int k = 0; k < 3; ++k) v.candidate.board_rt[3 + k] = Rm[k] * tcb[0] + Rm[3 + k] * tcb[1] + Rm[6 + k] * tcb[2];
                            v.pixel[0] = px[2 * q]; v.pixel[1] = px[2 * q + 1]; v.distance = distances[d]; v.tilt_x = tilts[t][0]; v.tilt_y = tilts[t][1];
                            all.push_back(v);
                            cands.push_back(v.candidate);
                        }
                }
        }
        std::vector<SuggestedView> chosen;
        std::vector<double> cc = cov.cam_cov;
        for (int step = 0; step < n_views && !cands.empty(); ++step) {
            const ViewGain g = view_gain_on(cc, cands.data(), (int)cands.size(), false, image, border, min_corners, std::vector<double>());
            int best = -1;
            for (size_t i = 0; i < cands.size(); ++i)
                if ((g.flags[i] & 4) && g.gain_logdet[i] > 0.0 && (best < 0 || g.gain_logdet[i] > g.gain_logdet[(size_t)best])) best = (int)i;
            if (best < 0) break;
            const ViewGain one = view_gain_on(cc, &cands[(size_t)best], 1, true, image, border, min_corners, std::vector<double>());
            SuggestedView v = all[(size_t)best];
            v.gain_logdet = one.gain_logdet[0]; v.gain_trace = one.gain_trace[0]; v.n_visible[0] = one.n_visible[0]; v.n_visible[1] = one.n_visible[1]; v.flags = one.flags[0];
            chosen.push_back(v);
            cc = one.cam_cov;
        }
        return chosen;
    }

    // main.cpp:305-319
    void write_yaml(const std::string &path) const
    {
        const int C = (int)cameras_.size();
        std::vector<double> I(9 * (size_t)C), R(9 * (size_t)C), t(3 * (size_t)C);
        for (int m = 0; m < C; ++m) {
            std::memcpy(&I[9 * (size_t)m], cameras_[m].intrinsic_.data(), 9 * sizeof(double));
            std::memcpy(&R[9 * (size_t)m], cameras_[m].R().a, 9 * sizeof(double));
            std::memcpy(&t[3 * (size_t)m], cameras_[m].t(), 3 * sizeof(double));
        }
        check(tscm_yaml_write(path.c_str(), C, I.data(), R.data(), t.data()));
    }

    std::vector<MultiCalib_camera> cameras_;
    std::vector<MultiCalib_chessboard> chessboards_;
    std::vector<Point3d> worlds_;
    int rank_ = 0, world_ = 1;                // set_sharding()
    int loss_kind_ = TSCM_LOSS_NONE;          // set_loss()
    double loss_scale_ = 0.0;
    std::vector<unsigned short> fixed_;       // set_fixed_intrinsics(), by camera (missing entries: 0)
    bool use_weights_ = false;                // set_corner_weights()
    std::vector<std::vector<std::vector<double> > > corner_weights_;
    bool use_priors_ = false;                 // set_camera_priors()
    CameraPriors priors_;
    tscm_comm *comm_ = nullptr;
    tscm_summary summary;                     // BriefReport data of the solve (:218)
    std::vector<double> camera_error;         // per-camera mean pixel error (:281)
    double mean_error;                        // "average reproject error" (:283)

private:
    // R (row-major) of an angle-axis vector, both branches of ceres::AngleAxisRotatePoint
    static void view_rotation(const double *w, double *R)
    {
        const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
        if (t2 > 2.220446049250313e-16) {
            const double th = std::sqrt(t2), c = std::cos(th), s = std::sin(th), k[3] = { w[0] / th, w[1] / th, w[2] / th };
            for (int r = 0; r < 3; ++r)
                for (int q = 0; q < 3; ++q) R[3 * r + q] = (r == q ? c : 0.0) + (1.0 - c) * k[r] * k[q];
            R[1] -= s * k[2]; R[2] += s * k[1]; R[3] += s * k[2]; R[5] -= s * k[0]; R[6] -= s * k[1]; R[7] += s * k[0];
        } else {
            const double I[9] = { 1.0, -w[2], w[1], w[2], 1.0, -w[0], -w[1], w[0], 1.0 };
            std::memcpy(R, I, sizeof(I));
        }
    }
    static void view_mul(const double *A, const double *B, double *out)
    {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) out[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
    }
    // the angle-axis vector of a rotation matrix, angle in [0, pi]
    static void view_angle_axis(const double *R, double *w)
    {
        const double v[3] = { R[7] - R[5], R[2] - R[6], R[3] - R[1] };
        const double s = 0.5 * std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), c = 0.5 * (R[0] + R[4] + R[8] - 1.0), th = std::atan2(s, c);
        if (s > 1e-8) { for (int k = 0; k < 3; ++k) w[k] = v[k] * (th / (2.0 * s)); return; }
        if (c > 0.0) { for (int k = 0; k < 3; ++k) w[k] = 0.5 * v[k]; return; }
        double k[3], n = 0.0;                                    // angle pi: R = 2 k k^T - I
        int big = 0;
        for (int i = 0; i < 3; ++i) { const double h = 0.5 * (R[4 * i] + 1.0); k[i] = std::sqrt(h > 0.0 ? h : 0.0); if (k[i] > k[big]) big = i; }
        for (int i = 0; i < 3; ++i) { if (i != big && R[3 * big + i] + R[3 * i + big] < 0.0) k[i] = -k[i]; n += k[i] * k[i]; }
        for (int i = 0; i < 3; ++i) w[i] = th * k[i] / std::sqrt(n);
    }

    ViewGain view_gain_on(const std::vector<double> &cam_cov, const tscm_view_candidate *candidates, int n, bool apply, Size image, double border,
                          int min_corners, const std::vector<double> &weights) const
    {
        const size_t C = cameras_.size(), R = (size_t)(n > 0 ? n : 0);
        std::vector<double> crt(6 * C), I(9 * C), xy(2 * worlds_.size());
        std::vector<int> size(2 * C);
        for (size_t m = 0; m < C; ++m) {
            std::memcpy(&crt[6 * m], cameras_[m].rt_.data(), 6 * sizeof(double));
            std::memcpy(&I[9 * m], cameras_[m].intrinsic_.data(), 9 * sizeof(double));
            size[2 * m] = image.width; size[2 * m + 1] = image.height;
        }
        for (size_t j = 0; j < worlds_.size(); ++j) { xy[2 * j] = worlds_[j].x; xy[2 * j + 1] = worlds_[j].y; }
        if (cam_cov.size() != 15 * C * 15 * C) throw std::invalid_argument("view_gain: cam_cov is not [C*15][C*15]");
        if (!weights.empty() && weights.size() != 15 * C) throw std::invalid_argument("view_gain: weights is not [C*15]");
        tscm_view_gain_params prm = tscm_view_gain_params();
        prm.struct_size = (int)sizeof(tscm_view_gain_params);
        prm.min_corners = min_corners;
        prm.border = border;
        ViewGain out;
        out.gain_logdet.assign(R + 1, 0.0); out.gain_trace.assign(R + 1, 0.0); out.n_visible.assign(2 * R + 2, 0); out.flags.assign(R + 1, 0);
        const double *w = weights.empty() ? nullptr : weights.data();
        if (apply) {
            out.cam_cov.assign(cam_cov.size(), 0.0);
            check(tscm_view_gain_apply((int)C, crt.data(), I.data(), cam_cov.data(), w, (int)worlds_.size(), xy.data(), size.data(), &prm, candidates, device_,
                                       out.gain_logdet.data(), out.gain_trace.data(), out.n_visible.data(), out.flags.data(), out.cam_cov.data()));
        } else {
            check(tscm_view_gain((int)C, crt.data(), I.data(), cam_cov.data(), w, (int)worlds_.size(), xy.data(), size.data(), &prm, candidates, n, device_,
                                 out.gain_logdet.data(), out.gain_trace.data(), out.n_visible.data(), out.flags.data()));
        }
        out.gain_logdet.resize(R); out.gain_trace.resize(R); out.n_visible.resize(2 * R); out.flags.resize(R);
        return out;
    }

    int device_;
};

// ---- corner detection: findCorner(img, sigma) (DetectCorner/findCorner.cpp:7-101) -------------------------------------
// Same result structure as the reference (Corner_t / Chessboarder_t, chessboard = matrices of indices into corners.p),
// grey 8-bit image instead of cv::Mat.  Board members carry their sub-pixel position (findCorner.cpp:84-97).
// What the calibrate_from_* programs do with ResidualOptions behind MultiCalib::calibrate(): --prune: `rounds` times
// prune_views(k, 0, max_fraction), one line per flagged view, and calibrate() again (a round that flags nothing ends the loop);
// --residuals / --residual-bins: the report of the final state, over [0, pi] with bins, to the file or standard output.
inline void run_residual_options(MultiCalib &mul, const ResidualOptions &o)
{
    for (int round = 0; o.prune && round < o.rounds; ++round) {
        const std::vector<std::pair<int, int> > out = mul.prune_views(o.k, 0.0, o.max_fraction);
        if (out.empty()) break;
        for (const std::pair<int, int> &mb : out) std::printf("prune round %d: camera %d board %d\n", round + 1, mb.first, mb.second);
        mul.calibrate();
        std::printf("pruned solve %d: %s  iterations %d  rmse %.4f px\n", round + 1, mul.summary.message, mul.summary.num_iterations - 1, mul.summary.rmse);
    }
    if (!o.report) return;
    tscm_residual_params prm;
    tscm_residual_default_params(&prm);
    prm.loss_kind = mul.loss_kind_; prm.loss_scale = mul.loss_scale_;
    prm.n_angle_bins = o.bins; prm.max_angle = 3.14159265358979323846;
    const ResidualReport rep = mul.residual_report(&prm);
    std::FILE *f = o.file.empty() ? stdout : std::fopen(o.file.c_str(), "w");
    if (!f) throw std::runtime_error("tscm: cannot write " + o.file);
    print_residual_report(f, rep, prm.max_angle);
    if (f != stdout) std::fclose(f);
}

struct Corner_t {
    std::vector<Point2d> p, v1, v2;
    std::vector<double> score;
};
struct IndexMat {
    int rows, cols;
    std::vector<unsigned short> data;                 // row-major, CV_16U like the reference
    unsigned short at(int r, int c) const { return data[(size_t)r * cols + c]; }
};
struct Chessboarder_t {
    Corner_t corners;
    std::vector<IndexMat> chessboard;
};

// candidates and boards of one image as the reference's Chessboarder_t: a board member's point is its sub-pixel position
inline Chessboarder_t chessboarder_of(const tscm_corner_candidates &c, const tscm_chessboards &b)
{
    Chessboarder_t out;
    for (int i = 0; i < c.n; ++i) {
        out.corners.p.push_back(Point2d{ c.x[i], c.y[i] });
        out.corners.v1.push_back(Point2d{ c.v1[2 * i], c.v1[2 * i + 1] });
        out.corners.v2.push_back(Point2d{ c.v2[2 * i], c.v2[2 * i + 1] });
        out.corners.score.push_back(c.score[i]);
    }
    for (int q = 0; q < b.n_boards; ++q) {
        IndexMat m;
        m.rows = b.rows[q]; m.cols = b.cols[q];
        for (int k = b.offset[q]; k < b.offset[q + 1]; ++k) {
            const int idx = b.cells[k];
            m.data.push_back((unsigned short)idx);
            out.corners.p[(size_t)idx] = Point2d{ c.sub[2 * idx], c.sub[2 * idx + 1] };
        }
        out.chessboard.push_back(m);
    }
    return out;
}

inline Chessboarder_t findCorner(const unsigned char *gray, int width, int height, int stride, int sigma, int device = 0)
{
    tscm_corner_candidates c;
    check(tscm_detect_corners(gray, width, height, stride, sigma, 0.01, device, &c));
    tscm_chessboards b;
    const int rc = tscm_chessboards_from_corners(c.n, c.x, c.y, c.v1, c.v2, &b);
    if (rc != 0) { tscm_corner_candidates_free(&c); check(rc); }
    const Chessboarder_t out = chessboarder_of(c, b);
    tscm_chessboards_free(&b);
    tscm_corner_candidates_free(&c);
    return out;
}

// findCorner for a batch of images of one size in two calls: tscm_detect_corners_batch, then the structure recovery of all
// of them as independent (image, seed) jobs -- where = TSCM_BOARDS_DEVICE on the device, TSCM_BOARDS_HOST the same
// definition on the host.  That definition differs from findCorner's recovery in one documented step (tscm.h); the boards
// agree unless a winning proposal holds an exact tie of two distances.
inline std::vector<Chessboarder_t> findCorners(const std::vector<const unsigned char *> &images, int width, int height, int stride, int sigma, int device = 0,
                                               int where = TSCM_BOARDS_DEVICE)
{
    const int n = (int)images.size();
    std::vector<Chessboarder_t> out;
    if (n == 0) return out;
    std::vector<tscm_corner_candidates> c((size_t)n);
    check(tscm_detect_corners_batch(images.data(), n, width, height, stride, sigma, 0.01, device, c.data()));
    std::vector<tscm_chessboards> b((size_t)n);
    const int rc = tscm_chessboards_from_corners_batch(n, c.data(), where, device, b.data());
    if (rc == 0)
        for (int k = 0; k < n; ++k) {
            out.push_back(chessboarder_of(c[(size_t)k], b[(size_t)k]));
            tscm_chessboards_free(&b[(size_t)k]);
        }
    for (int k = 0; k < n; ++k) tscm_corner_candidates_free(&c[(size_t)k]);
    check(rc);
    return out;
}

// Remap::calc_R (rectify.cpp:234-248): x along the baseline t2 - t1, z horizontal, y = z x x
inline Mat33 rectify_pair_rotation(const double t1[3], const double t2[3])
{
    double x[3] = { t2[0] - t1[0], t2[1] - t1[1], t2[2] - t1[2] };
    double n = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    if (n != 0) for (int k = 0; k < 3; ++k) x[k] /= n;
    double z[3] = { -x[2], 0.0, x[0] };
    n = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
    if (n != 0) for (int k = 0; k < 3; ++k) z[k] /= n;
    double y[3] = { -z[2] * x[1] + z[1] * x[2], z[2] * x[0] - z[0] * x[2], -z[1] * x[0] + z[0] * x[1] };
    n = std::sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
    if (n != 0) for (int k = 0; k < 3; ++k) y[k] /= n;
    Mat33 R;
    for (int k = 0; k < 3; ++k) { R.a[3 * k] = x[k]; R.a[3 * k + 1] = y[k]; R.a[3 * k + 2] = z[k]; }
    return R;
}

// The two tables that rectify a camera pair in an output image of kind `projection` spanning fov_x by fov_y radians:
// intr [9] and Twc (row-major 3x4 [R | t], camera to rig, as tscm_yaml_read returns them) of both cameras; R of table k
// is R_cam^T * rectify_pair_rotation(t_a, t_b), check_w2 = 1, offsets 0.  With TSCM_PROJ_LONGLAT a scene point lies on
// the same row of both images over the whole hemisphere (fov_x up to pi).  Fills desc[2]; maps are size.height x size.width.
inline void rectify_pair_maps(const double *intr_a, const double *Twc_a, const double *intr_b, const double *Twc_b, int projection, Size size,
                              double fov_x, double fov_y, tscm_map_desc desc[2], std::vector<float> mapx[2], std::vector<float> mapy[2],
                              bool exact = true, int device = 0)
{
    const double pi = 3.14159265358979323846;
    const bool tan_x = projection == TSCM_PROJ_PERSPECTIVE, tan_y = tan_x || projection == TSCM_PROJ_CYLINDRICAL;
    if ((tan_x && !(fov_x < pi)) || (tan_y && !(fov_y < pi))) throw std::runtime_error("tscm: a tangent axis cannot span 180 degrees or more");
    double fx = size.width / fov_x, fy = size.height / fov_y;                      // pixels per radian
    if (tan_x) fx = 0.5 * size.width / std::tan(0.5 * fov_x);
    if (tan_y) fy = 0.5 * size.height / std::tan(0.5 * fov_y);
    if (projection == TSCM_PROJ_STEREOGRAPHIC) { fx = 0.25 * size.width / std::tan(0.25 * fov_x); fy = 0.25 * size.height / std::tan(0.25 * fov_y); }
    const double ta[3] = { Twc_a[3], Twc_a[7], Twc_a[11] }, tb[3] = { Twc_b[3], Twc_b[7], Twc_b[11] };
    const Mat33 Rp = rectify_pair_rotation(ta, tb);
    const size_t n = (size_t)size.width * size.height;
    const int kinds[2] = { projection, projection };
    for (int k = 0; k < 2; ++k) {
        const double *T = k ? Twc_b : Twc_a;
        tscm_map_desc &d = desc[k];
        d = tscm_map_desc();
        std::memcpy(d.intr, k ? intr_b : intr_a, sizeof(d.intr));
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) d.R[3 * r + c] = T[r] * Rp.a[c] + T[4 + r] * Rp.a[3 + c] + T[8 + r] * Rp.a[6 + c];      // R_cam^T * Rp
        d.fx = fx; d.fy = fy; d.cx = 0.5 * size.width; d.cy = 0.5 * size.height;
        d.width = size.width; d.height = size.height; d.out_stride = size.width;
        d.check_w2 = 1; d.w2 = 0.42399;                                            // rectify.cpp:7
        mapx[k].assign(n, 0.f); mapy[k].assign(n, 0.f);
    }
    // two launches: each table has its own host arrays
    for (int k = 0; k < 2; ++k) check(tscm_build_maps_ex(&desc[k], &kinds[k], 1, device, exact ? 1 : 0, mapx[k].data(), mapy[k].data(), n, nullptr));
}

// What the rectified pair is for.  stereo_match: census + semi-global matching of two rectified 8-bit images of `size`
// (rows of size.width bytes) -> 16 * disparity per pixel of the left image, invalid pixels 16 * (min_disparity - 1);
// params == NULL: tscm_stereo_default_params.
inline std::vector<short> stereo_match(const unsigned char *left, const unsigned char *right, Size size, const tscm_stereo_params *params = NULL, int device = 0)
{
    tscm_stereo_params p;
    if (params) p = *params;
    else tscm_stereo_default_params(&p);
    std::vector<short> disparity((size_t)size.width * size.height);
    check(tscm_stereo_match(left, right, size.width, size.height, size.width, &p, device, disparity.data(), size.width, NULL));
    return disparity;
}

// stereo_filter: speckle removal and masked median of a disparity map of `size` (rows of size.width elements) -> the
// filtered map; params == NULL: tscm_stereo_filter_default_params (set min_disparity to the matcher's).
inline std::vector<short> stereo_filter(const std::vector<short> &disparity, Size size, const tscm_stereo_filter_params *params = NULL, int device = 0)
{
    if (disparity.size() != (size_t)size.width * size.height) throw std::runtime_error("tscm: the disparity map does not have the given size");
    tscm_stereo_filter_params p;
    if (params) p = *params;
    else tscm_stereo_filter_default_params(&p);
    std::vector<short> out(disparity.size());
    if (out.empty()) return out;
    check(tscm_stereo_filter(disparity.data(), size.width, size.height, size.width, &p, device, out.data(), size.width, NULL));
    return out;
}

// stereo_fill: every invalid pixel of a disparity or sweep index map of `size` gets the lowest, second-lowest or median of
// the nearest valid values along the path directions -> the filled map; params == NULL: tscm_stereo_fill_default_params
// (set min_disparity to the matcher's, wrap_x = 1 for a 360 degree map).  mask: NULL, or receives 0 valid on input / 1 filled /
// 2 left invalid per pixel.
inline std::vector<short> stereo_fill(const std::vector<short> &disparity, Size size, const tscm_stereo_fill_params *params = NULL, int device = 0,
                                      std::vector<unsigned char> *mask = NULL)
{
    if (disparity.size() != (size_t)size.width * size.height) throw std::runtime_error("tscm: the disparity map does not have the given size");
    tscm_stereo_fill_params p;
    if (params) p = *params;
    else tscm_stereo_fill_default_params(&p);
    std::vector<short> out(disparity.size());
    if (mask) mask->assign(disparity.size(), 0);
    if (out.empty()) return out;
    check(tscm_stereo_fill(disparity.data(), size.width, size.height, size.width, &p, device, out.data(), size.width, mask ? mask->data() : NULL, NULL));
    return out;
}

// The demos' --fill RULE[,MAX_DISTANCE[,MIN_DIRECTIONS]] with RULE lowest | second_lowest | median -> the three fields of p;
// false when the text is none of that (the ranges are the library's to refuse).
inline bool parse_fill_option(const char *text, tscm_stereo_fill_params *p)
{
    const std::string s(text);
    const size_t comma = s.find(',');
    const std::string rule = s.substr(0, comma);
    if (rule == "lowest") p->rule = TSCM_FILL_LOWEST;
    else if (rule == "second_lowest") p->rule = TSCM_FILL_SECOND_LOWEST;
    else if (rule == "median") p->rule = TSCM_FILL_MEDIAN;
    else return false;
    if (comma == std::string::npos) return true;
    int *const field[2] = { &p->max_distance, &p->min_directions };
    const char *q = s.c_str() + comma + 1;
    for (int k = 0; k < 2; ++k) {                               // whole decimal numbers, nothing before, between or after them
        char *end = NULL;
        const long v = std::strtol(q, &end, 10);
        if (end == q || (*q != '-' && (*q < '0' || *q > '9')) || v < -1000000 || v > 1000000) return false;
        *field[k] = (int)v;
        if (!*end) return true;
        if (*end != ',' || k == 1) return false;
        q = end + 1;
    }
    return false;
}

// range_weights: the table of tscm_stereo_refine_weights, floor(255 exp(-k / sigma) + 0.5) for k = 0..255.
inline std::vector<unsigned char> range_weights(double sigma)
{
    std::vector<unsigned char> table(256);
    tscm_stereo_refine_weights(sigma, table.data());
    return table;
}

// stereo_refine: every pixel of a disparity or sweep index map of `size` takes the lower weighted median of the valid pixels
// of its window, a neighbour weighted by weights[|guide(p) - guide(q)|] -> the refined map.  guide: one grey byte per pixel
// of the map; weights: NULL (every weight 255) or 256 entries, e.g. range_weights(sigma); params == NULL:
// tscm_stereo_refine_default_params (set min_disparity to the matcher's, wrap_x = 1 for a 360 degree map).
inline std::vector<short> stereo_refine(const std::vector<short> &disparity, const std::vector<unsigned char> &guide, Size size,
                                        const std::vector<unsigned char> *weights = NULL, const tscm_stereo_refine_params *params = NULL, int device = 0)
{
    if (disparity.size() != (size_t)size.width * size.height) throw std::runtime_error("tscm: the disparity map does not have the given size");
    if (guide.size() != disparity.size()) throw std::runtime_error("tscm: the guide does not have the map's size");
    if (weights && weights->size() != 256) throw std::runtime_error("tscm: the weight table does not have 256 entries");
    tscm_stereo_refine_params p;
    if (params) p = *params;
    else tscm_stereo_refine_default_params(&p);
    std::vector<short> out(disparity.size());
    if (out.empty()) return out;
    check(tscm_stereo_refine(disparity.data(), size.width, size.height, size.width, guide.data(), size.width, weights ? weights->data() : NULL, &p, device, out.data(),
                             size.width, NULL));
    return out;
}

// The demos' --refine RADIUS,SIGMA[,ITERATIONS[,FILL]] -> radius, iterations and fill_invalid of p, and sigma; false when the
// text is none of that or a number lies outside what tscm_stereo_refine takes (radius 1..7, iterations 1..8, FILL 0 or 1).
inline bool parse_refine_option(const char *text, tscm_stereo_refine_params *p, double *sigma)
{
    int field[4] = { 0, 0, p->iterations, p->fill_invalid };
    const char *q = text;
    int k = 0;
    for (; k < 4; ++k) {                                        // whole numbers, nothing before, between or after them
        char *end = NULL;
        if (*q != '-' && *q != '.' && (*q < '0' || *q > '9')) return false;
        if (k == 1) {
            *sigma = std::strtod(q, &end);
        } else {
            const long v = std::strtol(q, &end, 10);
            if (v < -1000 || v > 1000) return false;
            field[k] = (int)v;
        }
        if (end == q) return false;
        if (!*end) break;
        if (*end != ',' || k == 3) return false;
        q = end + 1;
    }
    if (k < 1 || field[0] < 1 || field[0] > 7 || field[2] < 1 || field[2] > 8 || (field[3] != 0 && field[3] != 1)) return false;
    p->radius = field[0];
    p->iterations = field[2];
    p->fill_invalid = field[3];
    return true;
}

// The sweep demo's --visibility SHIFT,TOLERANCE[,DILATE] -> cell_shift, tolerance and dilate of p; false when the text is none
// of that or a number lies outside what tscm_sweep_visibility takes (SHIFT 0..8, TOLERANCE 0..255, DILATE 0..2).
inline bool parse_visibility_option(const char *text, tscm_sweep_visibility_params *p)
{
    int field[3] = { 0, 0, p->dilate };
    const char *q = text;
    int k = 0;
    for (; k < 3; ++k) {                                        // whole numbers, nothing before, between or after them
        char *end = NULL;
        if (*q != '-' && (*q < '0' || *q > '9')) return false;
        const long v = std::strtol(q, &end, 10);
        if (end == q || v < -1000 || v > 1000) return false;
        field[k] = (int)v;
        if (!*end) break;
        if (*end != ',' || k == 2) return false;
        q = end + 1;
    }
    if (k < 1 || field[0] < 0 || field[0] > 8 || field[1] < 0 || field[1] > 255 || field[2] < 0 || field[2] > 2) return false;
    p->cell_shift = field[0];
    p->tolerance = field[1];
    p->dilate = field[2];
    return true;
}

// stereo_points: the disparities of stereo_match on the pair of rectify_pair_maps (left_map = desc[0], projection
// TSCM_PROJ_PERSPECTIVE or TSCM_PROJ_LONGLAT, baseline = |t_b - t_a|) -> points in the pair frame of camera a
// (P_rig = rectify_pair_rotation(t_a, t_b) * P + t_a); points of invalid pixels are NaN, valid[k] = 0.
inline std::vector<Point3d> stereo_points(const std::vector<short> &disparity, Size size, int min_disparity, const tscm_map_desc &left_map, int projection,
                                          double baseline, std::vector<unsigned char> &valid, int device = 0)
{
    if (disparity.size() != (size_t)size.width * size.height) throw std::runtime_error("tscm: the disparity map does not have the given size");
    std::vector<Point3d> points(disparity.size());
    valid.assign(disparity.size(), 0);
    if (points.empty()) return points;
    check(tscm_stereo_points(disparity.data(), size.width, size.height, size.width, min_disparity, &left_map, projection, baseline, device,
                             &points[0].x, valid.data()));
    return points;
}

// The panorama of a calibrated rig: one equirect (or cylindrical) table per camera in the rig frame (R = R_cam^T,
// check_w2 = 1, as maps.panorama_descs builds them), kept on the device with the alphas, seam labels and mask pyramids by a
// tscm_panorama handle; compose() blends one frame.  intr [9 n], Twc [12 n] (row-major 3x4 [R | t]) as tscm_yaml_read
// returns them; weights: NULL (all 255) or n images of image_size (entries may be NULL); params == NULL:
// tscm_panorama_default_params (multi-band, 4 levels).  tests/test_gpu_cpp_mirror.py runs the class through
// tests/native/mirror_perception.cpp and holds overlap, gains and the composed bytes to panorama.Composer.
class Panorama {
public:
    Panorama(int n_cameras, const double *intr, const double *Twc, Size image_size, int channels, Size pano_size, const tscm_panorama_params *params = NULL,
             const unsigned char *const *weights = NULL, int projection = TSCM_PROJ_EQUIRECT, int device = 0)
        : n_(n_cameras), channels_(channels), image_(image_size), pano_(pano_size), handle_(NULL)
    {
        if (projection != TSCM_PROJ_EQUIRECT && projection != TSCM_PROJ_CYLINDRICAL) throw std::runtime_error("tscm: a panorama is equirect or cylindrical");
        if (n_cameras < 1 || pano_size.width < 1 || pano_size.height < 1) throw std::runtime_error("tscm: a panorama needs cameras and a size");
        const double pi = 3.14159265358979323846;
        const size_t npix = (size_t)pano_.width * pano_.height;
        std::vector<tscm_map_desc> desc((size_t)n_);
        std::vector<int> kinds((size_t)n_, projection);
        for (int k = 0; k < n_; ++k) {
            tscm_map_desc &d = desc[(size_t)k];
            d = tscm_map_desc();
            std::memcpy(d.intr, intr + 9 * k, sizeof(d.intr));
            const double *T = Twc + 12 * k;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) d.R[3 * r + c] = T[4 * c + r];           // R_cam^T
            d.fx = pano_.width / (2.0 * pi);
            d.fy = projection == TSCM_PROJ_EQUIRECT ? pano_.height / pi : d.fx;
            d.cx = 0.5 * pano_.width; d.cy = 0.5 * pano_.height;
            d.width = pano_.width; d.height = pano_.height; d.out_stride = pano_.width;
            d.out_offset = (long long)k * (long long)npix;
            d.check_w2 = 1; d.w2 = 0.42399;
        }
        std::vector<float> mapx(npix * n_), mapy(npix * n_);
        check(tscm_build_maps_ex(desc.data(), kinds.data(), n_, device, 1, mapx.data(), mapy.data(), mapx.size(), NULL));
        tscm_panorama_params p;
        if (params) p = *params;
        else tscm_panorama_default_params(&p);
        check(tscm_panorama_create(n_, image_.width, image_.height, channels_, weights, mapx.data(), mapy.data(), pano_.width, pano_.height, &p, device, &handle_));
    }
    ~Panorama() { tscm_panorama_destroy(handle_); }

    // images: n rows-of-`stride`-bytes images (stride 0: image width * channels); gain_q8: NULL or n Q8 gains (exposure_gains)
    // -> pano_size.height rows of pano_size.width * channels bytes
    std::vector<unsigned char> compose(const unsigned char *const *images, int stride = 0, const unsigned short *gain_q8 = NULL, double *seconds_kernel = NULL)
    {
        const int row = pano_.width * channels_;
        std::vector<unsigned char> out((size_t)row * pano_.height);
        check(tscm_panorama_compose(handle_, images, stride ? stride : image_.width * channels_, gain_q8, out.data(), row, NULL, seconds_kernel));
        return out;
    }
    // count, sum [n * n]: pixels that cameras a and b both cover, and camera a's luminance summed over them
    void overlap(const unsigned char *const *images, int stride, std::vector<long long> &count, std::vector<long long> &sum)
    {
        count.assign((size_t)n_ * n_, 0); sum.assign((size_t)n_ * n_, 0);
        check(tscm_panorama_overlap(handle_, images, stride ? stride : image_.width * channels_, count.data(), sum.data()));
    }
    int cameras() const { return n_; }
    Size size() const { return pano_; }

private:
    Panorama(const Panorama &);
    Panorama &operator=(const Panorama &);
    int n_, channels_;
    Size image_, pano_;
    tscm_panorama *handle_;
};

// Gain compensation of Brown & Lowe (OpenCV's GainCompensator) from Panorama::overlap: minimises
// sum_ij N_ij [(g_i I_ij - g_j I_ji)^2 / sigma_n^2 + (1 - g_i)^2 / sigma_g^2], N = count, I = sum / count; the n x n system
// is solved in fp64 by Gaussian elimination with partial pivoting.  Returns round(256 g) clipped to 64..1024.
inline std::vector<unsigned short> exposure_gains(int n, const std::vector<long long> &count, const std::vector<long long> &sum, double sigma_n = 10.0,
                                                  double sigma_g = 0.1)
{
    if (n < 1 || count.size() != (size_t)n * n || sum.size() != (size_t)n * n) throw std::runtime_error("tscm: count and sum are n x n");
    std::vector<unsigned short> out((size_t)n, 256);
    if (n == 1) return out;
    const double alpha = 1.0 / (sigma_n * sigma_n), beta = 1.0 / (sigma_g * sigma_g);
    std::vector<double> A((size_t)n * n, 0.0), b((size_t)n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double N = (double)count[(size_t)i * n + j], Nji = (double)count[(size_t)j * n + i];
            const double Iij = N > 0 ? (double)sum[(size_t)i * n + j] / N : 0.0, Iji = Nji > 0 ? (double)sum[(size_t)j * n + i] / Nji : 0.0;
            b[(size_t)i] += beta * N;
            A[(size_t)i * n + i] += beta * N;
            if (j == i) continue;
            A[(size_t)i * n + i] += 2.0 * alpha * Iij * Iij * N;
            A[(size_t)i * n + j] -= 2.0 * alpha * Iij * Iji * N;
        }
    for (int i = 0; i < n; ++i)
        if (A[(size_t)i * n + i] == 0.0) { A[(size_t)i * n + i] = 1.0; b[(size_t)i] = 1.0; }       // a camera that covers nothing keeps gain 1
    for (int c = 0; c < n; ++c) {
        int piv = c;
        for (int r = c + 1; r < n; ++r)
            if (std::fabs(A[(size_t)r * n + c]) > std::fabs(A[(size_t)piv * n + c])) piv = r;
        if (A[(size_t)piv * n + c] == 0.0) throw std::runtime_error("tscm: singular gain system");
        if (piv != c) {
            for (int k = 0; k < n; ++k) std::swap(A[(size_t)c * n + k], A[(size_t)piv * n + k]);
            std::swap(b[(size_t)c], b[(size_t)piv]);
        }
        for (int r = c + 1; r < n; ++r) {
            const double f = A[(size_t)r * n + c] / A[(size_t)c * n + c];
            for (int k = c; k < n; ++k) A[(size_t)r * n + k] -= f * A[(size_t)c * n + k];
            b[(size_t)r] -= f * b[(size_t)c];
        }
    }
    for (int r = n - 1; r >= 0; --r) {
        double v = b[(size_t)r];
        for (int k = r + 1; k < n; ++k) v -= A[(size_t)r * n + k] * b[(size_t)k];
        b[(size_t)r] = v / A[(size_t)r * n + r];
    }
    for (int i = 0; i < n; ++i) {
        const double q = std::floor(256.0 * b[(size_t)i] + 0.5);
        out[(size_t)i] = (unsigned short)(q < 64.0 ? 64.0 : (q > 1024.0 ? 1024.0 : q));
    }
    return out;
}

// Sphere-sweep depth of a calibrated rig: for every pixel of the rig-frame panorama the inverse-distance hypothesis at which
// the cameras that see the point agree best (tscm.h: tscm_sweep_*).  The tables come from tscm_build_sweep_maps on the
// descriptors a Panorama uses, with the camera centres Twc[:, 3]; inv_distance: D = params.num_hypotheses values, not
// negative and strictly increasing (0 = infinity).  intr [9 n], Twc [12 n] as tscm_yaml_read returns them; grey images;
// weights: NULL (all 255) or n images of image_size (entries may be NULL); params == NULL: tscm_sweep_default_params with
// num_hypotheses = inv_distance.size().  tests/test_gpu_cpp_mirror.py runs depth, compose and points through
// tests/native/mirror_perception.cpp and holds them to sweep.Sweeper, and the all-invalid compose to Panorama::compose.
class Sweep {
public:
    Sweep(int n_cameras, const double *intr, const double *Twc, Size image_size, Size pano_size, const std::vector<double> &inv_distance,
          const tscm_sweep_params *params = NULL, const unsigned char *const *weights = NULL, int projection = TSCM_PROJ_EQUIRECT, int device = 0)
        : n_(n_cameras), image_(image_size), pano_(pano_size), projection_(projection), device_(device), inv_(inv_distance), handle_(NULL)
    {
        if (projection != TSCM_PROJ_EQUIRECT && projection != TSCM_PROJ_CYLINDRICAL) throw std::runtime_error("tscm: a panorama is equirect or cylindrical");
        if (n_cameras < 1 || pano_size.width < 1 || pano_size.height < 1 || inv_.empty()) throw std::runtime_error("tscm: a sweep needs cameras, a size and hypotheses");
        const double pi = 3.14159265358979323846;
        const int D = (int)inv_.size();
        std::vector<tscm_map_desc> desc((size_t)n_);
        std::vector<int> kinds((size_t)n_, projection);
        std::vector<double> centers(3 * (size_t)n_);
        for (int k = 0; k < n_; ++k) {
            tscm_map_desc &d = desc[(size_t)k];
            d = tscm_map_desc();
            std::memcpy(d.intr, intr + 9 * k, sizeof(d.intr));
            const double *T = Twc + 12 * k;
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) d.R[3 * r + c] = T[4 * c + r];           // R_cam^T
                centers[3 * (size_t)k + r] = T[4 * r + 3];
            }
            d.fx = pano_.width / (2.0 * pi);
            d.fy = projection == TSCM_PROJ_EQUIRECT ? pano_.height / pi : d.fx;
            d.cx = 0.5 * pano_.width; d.cy = 0.5 * pano_.height;
            d.width = pano_.width; d.height = pano_.height; d.out_stride = pano_.width;
            d.check_w2 = 1; d.w2 = 0.42399;
        }
        pano_map_ = desc[0];
        const size_t n_elems = (size_t)n_ * D * pano_.width * pano_.height;
        std::vector<float> mapx(n_elems), mapy(n_elems);
        check(tscm_build_sweep_maps(desc.data(), kinds.data(), n_, centers.data(), inv_.data(), D, device, 1, mapx.data(), mapy.data(), n_elems, NULL));
        tscm_sweep_params p;
        if (params) p = *params;
        else { tscm_sweep_default_params(&p); p.num_hypotheses = D; }
        if (p.num_hypotheses != D) throw std::runtime_error("tscm: params.num_hypotheses is not the number of inverse distances");
        check(tscm_sweep_create(n_, image_.width, image_.height, weights, mapx.data(), mapy.data(), pano_.width, pano_.height, &p, device, &handle_));
    }
    ~Sweep() { tscm_sweep_destroy(handle_); }

    // images: n rows-of-`stride`-bytes grey images (stride 0: the image width) -> pano_size.height rows of pano_size.width
    // values 16 k* + sub-index term, -16 where invalid
    std::vector<short> depth(const unsigned char *const *images, int stride = 0, double *seconds_kernel = NULL)
    {
        std::vector<short> out((size_t)pano_.width * pano_.height);
        check(tscm_sweep_depth(handle_, images, stride ? stride : image_.width, out.data(), pano_.width, seconds_kernel));
        return out;
    }
    // The frame blended at the hypothesis the index map names per pixel (tscm_sweep_compose): the panorama without the parallax
    // of a composition at infinity.  images: n rows-of-`stride`-bytes images of `channels` (1 or 3) bytes per pixel (stride 0:
    // image width * channels); index16: a map of depth(), raw or filtered, or NULL for the one the last depth() left on the
    // device; params == NULL: tscm_sweep_compose_default_params; gain_q8: NULL or n Q8 gains
    // -> pano_size.height rows of pano_size.width * channels bytes
    std::vector<unsigned char> compose(const unsigned char *const *images, int channels, const std::vector<short> *index16 = NULL,
                                       const tscm_sweep_compose_params *params = NULL, const unsigned short *gain_q8 = NULL, int stride = 0,
                                       std::vector<unsigned char> *coverage = NULL, double *seconds_kernel = NULL)
    {
        if (index16 && index16->size() != (size_t)pano_.width * pano_.height) throw std::runtime_error("tscm: the index map does not have the panorama's size");
        tscm_sweep_compose_params p;
        if (params) p = *params;
        else tscm_sweep_compose_default_params(&p);
        const int row = pano_.width * channels;
        std::vector<unsigned char> out((size_t)(row > 0 ? row : 0) * pano_.height);
        if (coverage) coverage->assign((size_t)pano_.width * pano_.height, 0);
        check(tscm_sweep_compose(handle_, images, stride ? stride : image_.width * channels, channels, index16 ? index16->data() : NULL, pano_.width, &p, gain_q8,
                                 out.data(), row, coverage ? coverage->data() : NULL, seconds_kernel));
        return out;
    }
    // compose under per-camera visibility (tscm_sweep_compose_visible): a camera that looks at a pixel's point through
    // something nearer is left out of that pixel.  visibility: as for visibility() below, not NULL
    std::vector<unsigned char> compose(const unsigned char *const *images, int channels, const std::vector<short> *index16, const tscm_sweep_compose_params *params,
                                       const tscm_sweep_visibility_params &visibility, const unsigned short *gain_q8 = NULL, int stride = 0,
                                       std::vector<unsigned char> *coverage = NULL, double *seconds_kernel = NULL)
    {
        if (index16 && index16->size() != (size_t)pano_.width * pano_.height) throw std::runtime_error("tscm: the index map does not have the panorama's size");
        tscm_sweep_compose_params p;
        if (params) p = *params;
        else tscm_sweep_compose_default_params(&p);
        const int row = pano_.width * channels;
        std::vector<unsigned char> out((size_t)(row > 0 ? row : 0) * pano_.height);
        if (coverage) coverage->assign((size_t)pano_.width * pano_.height, 0);
        check(tscm_sweep_compose_visible(handle_, images, stride ? stride : image_.width * channels, channels, index16 ? index16->data() : NULL, pano_.width, &p,
                                         &visibility, gain_q8, out.data(), row, coverage ? coverage->data() : NULL, seconds_kernel));
        return out;
    }
    // Which cameras the composer takes at every pixel (tscm_sweep_visibility): use[k * pixels + p] = 1 or 0, cameras() planes of
    // the panorama's size; state (may be NULL): 0 no depth, 1 seen by nobody, 2 all visible, 3 some occluded, 4 all occluded
    // and all kept.  index16: NULL for the map the last depth() left on the device; params == NULL: the defaults
    std::vector<unsigned char> visibility(const std::vector<short> *index16 = NULL, const tscm_sweep_visibility_params *params = NULL,
                                          std::vector<unsigned char> *state = NULL, double *seconds_kernel = NULL)
    {
        if (index16 && index16->size() != (size_t)pano_.width * pano_.height) throw std::runtime_error("tscm: the index map does not have the panorama's size");
        tscm_sweep_visibility_params p;
        if (params) p = *params;
        else tscm_sweep_visibility_default_params(&p);
        std::vector<unsigned char> use((size_t)n_ * pano_.width * pano_.height);
        if (state) state->assign((size_t)pano_.width * pano_.height, 0);
        check(tscm_sweep_visibility(handle_, index16 ? index16->data() : NULL, pano_.width, &p, use.data(), state ? state->data() : NULL, seconds_kernel));
        return use;
    }
    // the points of an index map of depth() in the rig frame; NaN and valid[k] = 0 where invalid or at infinity
    std::vector<Point3d> points(const std::vector<short> &index16, std::vector<unsigned char> &valid) const;
    int cameras() const { return n_; }
    Size size() const { return pano_; }

private:
    Sweep(const Sweep &);
    Sweep &operator=(const Sweep &);
    int n_;
    Size image_, pano_;
    int projection_, device_;
    std::vector<double> inv_;
    tscm_map_desc pano_map_;
    tscm_sweep *handle_;
};

// sweep_points: an index map of a sweep over the panorama `pano_map` (fx fy cx cy of the output grid; kind `projection`) ->
// points dir(i, j) / inv in the rig frame, inv interpolated between the hypotheses; NaN and valid[k] = 0 where invalid.
inline std::vector<Point3d> sweep_points(const std::vector<short> &index16, Size size, const tscm_map_desc &pano_map, int projection,
                                         const std::vector<double> &inv_distance, std::vector<unsigned char> &valid, int device = 0)
{
    if (index16.size() != (size_t)size.width * size.height) throw std::runtime_error("tscm: the index map does not have the given size");
    std::vector<Point3d> points(index16.size());
    valid.assign(index16.size(), 0);
    if (points.empty()) return points;
    check(tscm_sweep_points(index16.data(), size.width, size.height, size.width, &pano_map, projection, inv_distance.data(), (int)inv_distance.size(), device,
                            &points[0].x, valid.data()));
    return points;
}

inline std::vector<Point3d> Sweep::points(const std::vector<short> &index16, std::vector<unsigned char> &valid) const
{
    return sweep_points(index16, pano_, pano_map_, projection_, inv_, valid, device_);
}

}  // namespace tscm
#endif
