// calibrate_from_images.cpp -- the reference's main.cpp from the image files on, through the C++ mirror (no OpenCV):
//   image list  ->  monocular_calib per camera (main.cpp:8-130: findCorner, calibrate, refinement pass on the remapped
//   chessboards with the flip rule, calibrate)  ->  MultiCalib(cameras, worlds) + calibrate (main.cpp:233-234)  ->  calib.yaml
// Images are 8-bit binary PGM files (P5); the list file holds one line per camera: "<n_frames> path_0 path_1 ..." with "-"
// for a frame the camera has no image of.  The viewer and the drawing calls of main.cpp are left out.
//   usage: calibrate_from_images list.txt calib.yaml [cols rows pitch] [--model ts|ds|ucm] [--fix fx,fy,cx,cy,xi,lambda,alpha]
//                                [--prior name:sigma[,name:sigma...]] [--ransac THRESHOLD[,HYPOTHESES[,MIN_INLIERS]] [--ransac-mask]]
//                                [--residuals[=FILE]] [--residual-bins K] [--prune K[,ROUNDS[,MAX_FRACTION]]] [--device-boards]
//   (--device-boards: tscm::findCorners instead of findCorner per image -- a camera's images are detected and their boards
//    recovered in two calls, the structure recovery as one batch on the device, and the remapped boards of the refinement pass
//    likewise.
//    --model ds | ucm: Double Sphere (lambda held at 0) / Unified Camera Model (xi and lambda held at 0) in every solve; the
//    YAML keeps the 9-vector with those entries 0.  --fix: further intrinsics held at their start values in every solve.
//    --prior: Gaussian priors (Ceres' NormalPrior, tscm.h) on the named intrinsics of every camera, in every solve, about the
//    values that solve starts from; sigma in the parameter's unit against a corner sigma of one pixel; names as for --fix.
//    Each camera prints the priors that count: `camera_m mono|rig prior name mean +- sigma` (mono: of its last refinement).
//    --ransac-mask (with --ransac): the inlier masks are the corner masks of every refinement and of the joint solve; prints the
//                  number of corners masked per camera
//    --ransac: the start poses of both calibrate() calls come from tscm_estimate_extrinsic_ransac at THRESHOLD pixels; a view
//    without consensus leaves the calibration, and per camera the views kept and the share of inlier corners are printed
//    --residuals, --residual-bins, --prune (rigs): the residual report and outlier-view pruning behind the joint solve, as
//    calibrate_from_corners has them)
#include <tscm/tscm_calib.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

struct Image { int w = 0, h = 0; std::vector<unsigned char> pix; bool ok() const { return w > 0; } };

Image read_pgm(const std::string &path)
{
    Image im;
    std::ifstream f(path.c_str(), std::ios::binary);
    std::string magic;
    int maxval = 0, w = 0, h = 0;
    if (!(f >> magic >> w >> h >> maxval) || magic != "P5" || maxval != 255 || w < 1 || h < 1) return im;
    f.get();
    im.pix.resize((size_t)w * h);
    f.read(reinterpret_cast<char *>(im.pix.data()), (std::streamsize)im.pix.size());
    if ((size_t)f.gcount() == im.pix.size()) { im.w = w; im.h = h; }
    return im;
}

// the board of the expected size, if findCorner found exactly that (main.cpp:33)
bool board_corners(const tscm::Chessboarder_t &found, tscm::Size board, std::vector<tscm::Point2d> &out)
{
    if (found.chessboard.size() != 1 || found.chessboard[0].rows != board.height || found.chessboard[0].cols != board.width) return false;
    out.clear();
    const tscm::IndexMat &m = found.chessboard[0];
    for (int u = 0; u < m.rows; ++u)
        for (int v = 0; v < m.cols; ++v) out.push_back(found.corners.p[m.at(u, v)]);
    return true;
}

// main.cpp:8-130
void monocular_calib(const std::vector<Image> &images, double size, tscm::Size board, const std::vector<tscm::Point3d> &worlds, tscm::TripleSphereCamera &cam,
                     bool device_boards)
{
    const int V = (int)images.size();
    std::vector<std::vector<tscm::Point2d> > pixels(V);
    std::vector<bool> has(V, false);
    tscm::Size img_size = { 0, 0 };
    std::vector<int> which;                                                    // --device-boards: the images of one batch
    std::vector<const unsigned char *> batch;
    for (int i = 0; i < V; ++i) {                                              // :24-50
        if (!images[i].ok()) continue;
        img_size.width = images[i].w; img_size.height = images[i].h;
        if (device_boards) { which.push_back(i); batch.push_back(images[i].pix.data()); continue; }
        has[i] = board_corners(tscm::findCorner(images[i].pix.data(), images[i].w, images[i].h, images[i].w, 4, cam.device()), board, pixels[i]);
    }
    if (device_boards && !batch.empty()) {
        for (int i : which)
            if (images[i].w != img_size.width || images[i].h != img_size.height) throw std::runtime_error("--device-boards: a camera's images must have one size");
        const std::vector<tscm::Chessboarder_t> found = tscm::findCorners(batch, img_size.width, img_size.height, img_size.width, 4, cam.device());
        for (size_t k = 0; k < which.size(); ++k) has[which[k]] = board_corners(found[k], board, pixels[which[k]]);
    }
    cam.calibrate(pixels, has, worlds, img_size, board);                       // :57
    std::vector<std::vector<unsigned char> > chesses(V);                       // :59-126 refinement pass: the remapped boards
    std::vector<tscm::Size> sizes(V, tscm::Size{ 0, 0 });
    std::vector<tscm::Chessboarder_t> remapped(V);
    which.clear(); batch.clear();
    for (int i = 0; i < V; ++i) {
        if (!has[i]) continue;
        sizes[i] = cam.undistort_chessboard(images[i].pix.data(), images[i].w, images[i].h, images[i].w, 1, i, board, size, chesses[i]);
        if (sizes[i].width == 0) continue;
        if (device_boards) { which.push_back(i); batch.push_back(chesses[i].data()); }
        else remapped[i] = tscm::findCorner(chesses[i].data(), sizes[i].width, sizes[i].height, sizes[i].width, 4, cam.device());
    }
    if (device_boards && !batch.empty()) {                                     // (the remapped boards of one board size have one size)
        const tscm::Size cs = sizes[which[0]];
        const std::vector<tscm::Chessboarder_t> found = tscm::findCorners(batch, cs.width, cs.height, cs.width, 4, cam.device());
        for (size_t k = 0; k < which.size(); ++k) remapped[which[k]] = found[k];
    }
    for (int i = 0; i < V; ++i) {
        if (!has[i]) continue;
        const std::vector<unsigned char> &chess = chesses[i];
        const tscm::Size cs = sizes[i];
        if (cs.width == 0) continue;
        std::vector<tscm::Point2d> refined;
        if (board_corners(remapped[i], board, refined)) {
            const tscm::Mat33 &Rt = cam.Rt(i);                                 // :92-105: back through [r1 r2 t] and project()
            std::vector<tscm::Point3d> P(refined.size());
            for (size_t k = 0; k < refined.size(); ++k) {
                const double x = refined[k].x - size, y = refined[k].y - size;
                P[k] = tscm::Point3d{ Rt.a[0] * x + Rt.a[1] * y + Rt.a[2], Rt.a[3] * x + Rt.a[4] * y + Rt.a[5], Rt.a[6] * x + Rt.a[7] * y + Rt.a[8] };
            }
            pixels[i] = cam.project(P);
        }
        auto grey = [&](double x, double y) { return (int)chess[(size_t)(int)y * cs.width + (int)x]; };          // :72-89 / :107-121 flip rule
        if (grey(size / 2, size / 2) + grey(size * 3 / 2, size * 3 / 2) > grey(size * 3 / 2, size / 2) + grey(size / 2, size * 3 / 2)) {
            const std::vector<tscm::Point2d> tmp = pixels[i];
            for (size_t k = 0; k < tmp.size(); ++k) pixels[i][k] = tmp[tmp.size() - 1 - k];
        }
    }
    const bool ok = cam.calibrate(pixels, has, worlds, img_size, board);       // :127
    if (cam.use_ransac_) tscm::print_ransac_summary(cam, has, -1);
    int n_has = 0;
    for (int i = 0; i < V; ++i) n_has += has[i] ? 1 : 0;
    std::printf("%s, boards %d of %d, rmse %.4f px, fx %.3f fy %.3f cx %.3f cy %.3f xi %.4f lambda %.4f alpha %.4f\n", ok ? "converged" : "NOT converged", n_has, V,
                cam.summary.rmse, cam.intrinsic_[0], cam.intrinsic_[1], cam.intrinsic_[2], cam.intrinsic_[3], cam.intrinsic_[4], cam.intrinsic_[5], cam.intrinsic_[6]);
}

}  // namespace

int main(int argc, char **argv)
{
    std::vector<const char *> pos;                  // positional arguments: list, yaml, then cols rows pitch
    unsigned short model = 0, fix = 0;              // --model (the last one counts), --fix (accumulates)
    bool use_prior = false;                         // --prior (the last one counts)
    double prior_sigma[7] = { 0, 0, 0, 0, 0, 0, 0 };
    bool bad_args = false, use_ransac = false, ransac_mask = false, device_boards = false;
    tscm_ransac_params ransac;
    tscm_ransac_default_params(&ransac);
    tscm::ResidualOptions residual;
    for (int i = 1; i < argc && !bad_args; ++i) {
        const int taken = tscm::parse_residual_option(argc, argv, i, residual);
        if (taken != 0) { bad_args = taken < 0; continue; }
        if (!std::strcmp(argv[i], "--model") && i + 1 < argc) {
            bad_args = !tscm::model_mask(argv[++i], model);
        } else if (!std::strcmp(argv[i], "--fix") && i + 1 < argc) {
            unsigned short w = 0;
            bad_args = !tscm::fixed_list_mask(argv[++i], w);
            fix = (unsigned short)(fix | w);
        } else if (!std::strcmp(argv[i], "--prior") && i + 1 < argc) {
            use_prior = true;
            bad_args = !tscm::parse_prior_option(argv[++i], prior_sigma);
        } else if (!std::strcmp(argv[i], "--ransac") && i + 1 < argc) {
            use_ransac = true;
            bad_args = !tscm::parse_ransac_option(argv[++i], &ransac);
        } else if (!std::strcmp(argv[i], "--ransac")) {
            bad_args = true;
        } else if (!std::strcmp(argv[i], "--ransac-mask")) {
            ransac_mask = true;
        } else if (!std::strcmp(argv[i], "--device-boards")) {
            device_boards = true;
        } else {
            pos.push_back(argv[i]);
        }
    }
    if (bad_args || pos.size() < 2 || (ransac_mask && !use_ransac)) {
        std::fprintf(stderr, "usage: %s list.txt calib.yaml [cols rows pitch] [--model ts|ds|ucm] [--fix fx,fy,cx,cy,xi,lambda,alpha] [--prior name:sigma[,name:sigma...]] "
                     "[--ransac THRESHOLD[,HYPOTHESES[,MIN_INLIERS]] [--ransac-mask]] [--residuals[=FILE]] [--residual-bins K] [--prune K[,ROUNDS[,MAX_FRACTION]]] [--device-boards]\n", argv[0]);
        return 2;
    }
    const unsigned short fixed = (unsigned short)(model | fix);
    const bool dims = pos.size() >= 5;
    const tscm::Size board = { dims ? std::atoi(pos[2]) : 9, dims ? std::atoi(pos[3]) : 6 };
    const double size = dims ? std::atof(pos[4]) : 45.0;
    std::ifstream list(pos[0]);
    if (!list) { std::fprintf(stderr, "cannot open %s\n", pos[0]); return 2; }
    std::vector<std::vector<Image> > images;
    std::string line;
    while (std::getline(list, line)) {
        std::istringstream is(line);
        int n = 0;
        if (!(is >> n)) continue;
        std::vector<Image> cam(n);
        for (int i = 0; i < n; ++i) { std::string path; is >> path; if (path != "-") cam[i] = read_pgm(path); }
        images.push_back(cam);
    }
    try {
        std::vector<tscm::Point3d> worlds;                                     // main.cpp:12-18
        for (int u = 0; u < board.height; ++u)
            for (int v = 0; v < board.width; ++v) worlds.push_back(tscm::Point3d{ v * size, u * size, 0.0 });
        std::vector<tscm::TripleSphereCamera> cameras(images.size());
        for (size_t m = 0; m < images.size(); ++m) {
            std::printf("camera %zu: ", m);
            cameras[m].set_fixed_intrinsics(fixed);                            // (the first calibrate starts at xi = lambda = 0)
            if (use_prior) cameras[m].set_prior_sigmas(prior_sigma);
            if (use_ransac) cameras[m].set_ransac(&ransac, ransac_mask);
            monocular_calib(images[m], size, board, worlds, cameras[m], device_boards);
            if (use_prior) tscm::print_effective_priors(cameras[m].last_priors_, 0, (int)m, fixed, "mono");
            if (ransac_mask) tscm::print_ransac_masked(cameras[m], (int)m);
        }
        if (cameras.size() > 1) {
            tscm::MultiCalib mul_calib(cameras, worlds);                       // main.cpp:233
            for (size_t m = 0; m < cameras.size(); ++m) mul_calib.set_fixed_intrinsics((int)m, fixed);
            const std::vector<std::vector<std::vector<double> > > masks = tscm::ransac_corner_masks(cameras);
            if (ransac_mask) mul_calib.set_corner_weights(&masks);              // the joint solve takes the masks too
            tscm::CameraPriors priors;                                         // about the values the joint solve starts from
            if (use_prior) {
                std::vector<double> start;
                for (size_t m = 0; m < cameras.size(); ++m) start.insert(start.end(), mul_calib.cameras_[m].intrinsic_.begin(), mul_calib.cameras_[m].intrinsic_.end());
                priors = tscm::intrinsic_priors_about(start, prior_sigma);
                mul_calib.set_camera_priors(&priors);
                for (size_t m = 0; m < cameras.size(); ++m) tscm::print_effective_priors(priors, m, (int)m, fixed, "rig");
            }
            mul_calib.calibrate();                                             // main.cpp:234
            std::printf("%s  iterations %d  rmse %.4f px\n", mul_calib.summary.message, mul_calib.summary.num_iterations - 1, mul_calib.summary.rmse);
            std::printf("average reproject error: %.6f\n", mul_calib.mean_error);
            tscm::run_residual_options(mul_calib, residual);
            mul_calib.write_yaml(pos[1]);                                     // main.cpp:305-319
        } else if (cameras.size() == 1) {
            const double I3[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, t0[3] = { 0, 0, 0 };
            tscm::check(tscm_yaml_write(pos[1], 1, cameras[0].intrinsic_.data(), I3, t0));
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
