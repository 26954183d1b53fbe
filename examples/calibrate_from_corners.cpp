// calibrate_from_corners.cpp -- the reference's main.cpp from the corner lists on (main.cpp:196-319), on the GPU:
//   corners.txt (TSCM-CORNERS 1, see tscm.h)  ->  per-camera calibration  ->  MultiCalib  ->  calib.yaml
//
//   g++ -std=c++11 -I include examples/calibrate_from_corners.cpp -L tscm_calib_amd/csrc -ltscm_hip
//       -Wl,-rpath,$PWD/tscm_calib_amd/csrc -o examples/calibrate_from_corners        (one command line)
//   examples/calibrate_from_corners corners.txt calib.yaml [--loss huber|soft_l1|cauchy --loss-scale <px>]
//                                   [--model ts|ds|ucm] [--fix fx,fy,cx,cy,xi,lambda,alpha] [--prior name:sigma[,name:sigma...]]
//                                   [--ransac THRESHOLD[,HYPOTHESES[,MIN_INLIERS]] [--ransac-mask]] [--covariance]
//                                   [--uncertainty STEP[,INV_DISTANCE]] [--suggest N[,DISTANCE...]]
//                                   [--residuals[=FILE]] [--residual-bins K] [--prune K[,ROUNDS[,MAX_FRACTION]]]
//   (--loss: Ceres' HuberLoss / SoftLOneLoss / CauchyLoss(px) on every corner of every solve; the reference passes NULL.
//    --model ds | ucm: Double Sphere (lambda held at 0) / Unified Camera Model (xi and lambda held at 0) in every solve; the
//    YAML keeps the 9-vector with those entries 0.  --fix: further intrinsics held at their start values in every solve.
//    --prior: Gaussian priors (Ceres' NormalPrior, tscm.h) on the named intrinsics of every camera, in every solve, about the
//    values that solve starts from; sigma in the parameter's unit against a corner sigma of one pixel; names as for --fix.
//    Each camera prints the priors that count (a held intrinsic has none): `camera_m mono|rig prior name mean +- sigma`; the
//    covariance includes the joint solve's.
//    --ransac-mask (with --ransac): the inlier masks are the corner masks of every refinement, the joint solve and the covariance
//                  included; prints the number of corners masked per camera
//    --ransac: the start poses come from tscm_estimate_extrinsic_ransac at THRESHOLD pixels; a view without consensus leaves
//    the calibration, and per camera the views kept and the share of inlier corners are printed.
//    --covariance (rigs): after the joint solve, one line per camera parameter, `name value +- standard deviation`
//    (MultiCalib::covariance; 0 for a held parameter), then sigma and min_pivot_ratio -- near 0 when the views do not
//    determine some parameter.
//    --uncertainty (rigs; implies --covariance): projection uncertainty maps (MultiCalib::projection_uncertainty) on the grid
//    x, y = 0, STEP, 2 STEP, ... of the corner file's image size at INV_DISTANCE (1 / distance in 1 / the pitch's unit; default
//    0, infinity): per camera the largest and the median sd_worst of a fixed point seen in that camera, per pair of adjacent
//    cameras the largest and the median sd_across of a pixel transferred from the first to the second -- the pixels by which
//    rectified rows stop being rows
//    --suggest (rigs; implies --covariance): where to hold the board next -- N poses chosen greedily by the covariance each
//    would remove (MultiCalib::suggest_views; default distances: 5 and 10 board diagonals), printed behind the covariance
//    report: `suggest k camera_a[+camera_b] pixel u v distance d tilt x y gain_logdet g gain_trace t visible n[,n]`
//    --residuals (rigs): after the joint solve, the residual report (MultiCalib::residual_report) to FILE or standard output:
//    one line per view, `view v camera m board b corners n rms r max x worst j`; --residual-bins K adds per camera the mean radial
//    and tangential residual over K bins of the incidence angle, 0 .. pi -- what tells a wrong model from a noisy one
//    --prune (rigs): ROUNDS times (default 1): the views whose rms exceeds their camera's median + K * 1.4826 * MAD leave the
//    problem (MultiCalib::prune_views, at most MAX_FRACTION of a camera's views, default 0.2) and the joint solve runs again;
//    the YAML, the covariance and the report are those of the last solve)
#include <tscm/tscm_calib.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv)
{
    int loss = TSCM_LOSS_NONE;
    double loss_scale = 1.0;
    unsigned short model = 0, fix = 0;              // --model (the last one counts), --fix (accumulates)
    bool use_prior = false;                         // --prior (the last one counts)
    double prior_sigma[7] = { 0, 0, 0, 0, 0, 0, 0 };
    bool bad_args = argc < 3, use_ransac = false, ransac_mask = false, covariance = false, uncertainty = false;
    double unc_step = 0.0, unc_inv_distance = 0.0;
    int suggest = 0;
    std::vector<double> suggest_distances;
    tscm::ResidualOptions residual;
    tscm_ransac_params ransac;
    tscm_ransac_default_params(&ransac);
    for (int i = 3; i < argc && !bad_args; ++i) {
        if (!std::strcmp(argv[i], "--loss") && i + 1 < argc) {
            const char *k = argv[++i];
            loss = !std::strcmp(k, "huber") ? TSCM_LOSS_HUBER : !std::strcmp(k, "soft_l1") ? TSCM_LOSS_SOFT_L1 : !std::strcmp(k, "cauchy") ? TSCM_LOSS_CAUCHY : -1;
            bad_args = loss < 0;
        } else if (!std::strcmp(argv[i], "--loss-scale") && i + 1 < argc) {
            loss_scale = std::strtod(argv[++i], nullptr);
        } else if (!std::strcmp(argv[i], "--model") && i + 1 < argc) {
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
        } else if (!std::strcmp(argv[i], "--ransac-mask")) {
            ransac_mask = true;
        } else if (!std::strcmp(argv[i], "--covariance")) {
            covariance = true;
        } else if (!std::strcmp(argv[i], "--uncertainty") && i + 1 < argc) {
            char *end = nullptr;
            unc_step = std::strtod(argv[++i], &end);
            bad_args = end == argv[i] || !(unc_step > 0.0) || !std::isfinite(unc_step);
            if (!bad_args && *end == ',') {
                const char *second = end + 1;
                unc_inv_distance = std::strtod(second, &end);
                bad_args = end == second || !(unc_inv_distance >= 0.0) || !std::isfinite(unc_inv_distance);
            }
            bad_args = bad_args || *end != '\0';
            uncertainty = covariance = true;
        } else if (!std::strcmp(argv[i], "--suggest") && i + 1 < argc) {
            char *end = nullptr;
            const char *at = argv[++i];
            suggest = (int)std::strtol(at, &end, 10);
            bad_args = end == at || suggest < 1;
            while (!bad_args && *end == ',') {
                at = end + 1;
                const double d = std::strtod(at, &end);
                bad_args = end == at || !(d > 0.0) || !std::isfinite(d);
                suggest_distances.push_back(d);
            }
            bad_args = bad_args || *end != '\0';
            covariance = true;
        } else {
            bad_args = tscm::parse_residual_option(argc, argv, i, residual) != 1;
        }
    }
    bad_args = bad_args || (ransac_mask && !use_ransac);
    if (bad_args) {
        std::fprintf(stderr, "usage: %s corners.txt calib.yaml [--loss huber|soft_l1|cauchy --loss-scale <px>] [--model ts|ds|ucm] "
                     "[--fix fx,fy,cx,cy,xi,lambda,alpha] [--prior name:sigma[,name:sigma...]] [--ransac THRESHOLD[,HYPOTHESES[,MIN_INLIERS]] [--ransac-mask]] [--covariance] [--uncertainty STEP[,INV_DISTANCE]] [--suggest N[,DISTANCE...]] "
                     "[--residuals[=FILE]] [--residual-bins K] [--prune K[,ROUNDS[,MAX_FRACTION]]]\n", argv[0]);
        return 2;
    }
    const unsigned short fixed = (unsigned short)(model | fix);
    tscm_corner_set cs;
    if (tscm_corners_read(argv[1], &cs) != 0) { std::fprintf(stderr, "%s\n", tscm_last_error()); return 1; }
    int rc = 0;
    try {
        const int C = cs.n_cameras, B = cs.n_boards, n = cs.board_cols * cs.board_rows;
        const tscm::Size board = { cs.board_cols, cs.board_rows }, image = { cs.image_width, cs.image_height };
        std::vector<tscm::Point3d> worlds;                                   // main.cpp:12-18
        for (int u = 0; u < board.height; ++u)
            for (int v = 0; v < board.width; ++v) worlds.push_back(tscm::Point3d{ v * cs.pitch, u * cs.pitch, 0.0 });
        std::vector<tscm::TripleSphereCamera> cameras(C);
        for (int m = 0; m < C; ++m) {                                        // main.cpp:196-222
            std::vector<std::vector<tscm::Point2d> > pixels(B);
            std::vector<bool> has(B);
            for (int b = 0; b < B; ++b) {
                has[b] = cs.has[(size_t)m * B + b] != 0;
                if (!has[b]) continue;
                pixels[b].resize(n);
                for (int j = 0; j < n; ++j) pixels[b][j] = tscm::Point2d{ cs.pix_u[((size_t)m * B + b) * n + j], cs.pix_v[((size_t)m * B + b) * n + j] };
            }
            cameras[m].set_loss(loss, loss_scale);
            cameras[m].set_fixed_intrinsics(fixed);                          // (a fresh calibrate starts at xi = lambda = 0)
            if (use_prior) cameras[m].set_prior_sigmas(prior_sigma);
            if (use_ransac) cameras[m].set_ransac(&ransac, ransac_mask);
            const bool ok = cameras[m].calibrate(pixels, has, worlds, image, board);
            if (use_prior) tscm::print_effective_priors(cameras[m].last_priors_, 0, m, fixed, "mono");
            if (use_ransac) tscm::print_ransac_summary(cameras[m], has, m);
            if (ransac_mask) tscm::print_ransac_masked(cameras[m], m);
            std::printf("camera %d: %s, rmse %.4f px, fx %.3f fy %.3f cx %.3f cy %.3f xi %.4f lambda %.4f alpha %.4f\n", m, ok ? "converged" : "NOT converged",
                        cameras[m].summary.rmse, cameras[m].intrinsic_[0], cameras[m].intrinsic_[1], cameras[m].intrinsic_[2], cameras[m].intrinsic_[3],
                        cameras[m].intrinsic_[4], cameras[m].intrinsic_[5], cameras[m].intrinsic_[6]);
            if (!ok) rc = 3;
        }
        if (C > 1) {
            tscm::MultiCalib mul_calib(cameras, worlds);                     // main.cpp:233
            mul_calib.set_loss(loss, loss_scale);
            for (int m = 0; m < C; ++m) mul_calib.set_fixed_intrinsics(m, fixed);
            const std::vector<std::vector<std::vector<double> > > masks = tscm::ransac_corner_masks(cameras);
            if (ransac_mask) mul_calib.set_corner_weights(&masks);            // the joint solve and the covariance take the masks too
            tscm::CameraPriors priors;                                       // about the values the joint solve starts from
            if (use_prior) {
                std::vector<double> start;
                for (int m = 0; m < C; ++m) start.insert(start.end(), mul_calib.cameras_[m].intrinsic_.begin(), mul_calib.cameras_[m].intrinsic_.end());
                priors = tscm::intrinsic_priors_about(start, prior_sigma);
                mul_calib.set_camera_priors(&priors);
                for (int m = 0; m < C; ++m) tscm::print_effective_priors(priors, (size_t)m, m, fixed, "rig");
            }
            mul_calib.calibrate();                                           // main.cpp:234
            std::printf("%s  iterations %d  rmse %.4f px\n", mul_calib.summary.message, mul_calib.summary.num_iterations - 1, mul_calib.summary.rmse);
            for (int m = 0; m < C; ++m) std::printf("camera_%d reprojection error: %.6f\n", m, mul_calib.camera_error[m]);
            std::printf("average reproject error: %.6f\n", mul_calib.mean_error);
            tscm::run_residual_options(mul_calib, residual);
            mul_calib.write_yaml(argv[2]);                                   // main.cpp:305-319
            if (covariance) {
                const tscm::MultiCalib::Covariance cov = mul_calib.covariance();
                static const char *const names[15] = { "r0", "r1", "r2", "t0", "t1", "t2", "fx", "fy", "cx", "cy", "xi", "lambda", "alpha", "b", "c" };
                if (cov.info.status != 0) std::printf("covariance: singular %s (%d)\n", cov.info.status == 1 ? "board block" : "reduced system", cov.info.where);
                for (int m = 0; m < C; ++m)
                    for (int a = 0; a < 13; ++a) {
                        const double value = a < 6 ? mul_calib.cameras_[m].rt_[a] : mul_calib.cameras_[m].intrinsic_[a - 6];
                        const double sd = a < 6 ? cov.cam_rt_std[6 * (size_t)m + a] : cov.intr_std[9 * (size_t)m + a - 6];
                        std::printf("camera_%d %s %.17g +- %.17g\n", m, names[a], value, sd);
                    }
                std::printf("sigma %.17g  min_pivot_ratio %.17g  free columns %d\n", std::sqrt(cov.sigma2), cov.info.min_pivot_ratio, cov.info.n_free);
                if (uncertainty) {
                    const std::vector<tscm_uncertainty_request> req = mul_calib.uncertainty_requests(std::vector<double>(1, unc_inv_distance));
                    const tscm::MultiCalib::Uncertainty unc = mul_calib.projection_uncertainty(cov, tscm::MultiCalib::image_grid(image.width, image.height, unc_step), req);
                    const size_t npix = (size_t)unc.nx * unc.ny;
                    for (size_t r = 0; r < req.size(); ++r) {
                        const bool observe = req[r].camera_a == req[r].camera_b;
                        const double *sd = unc.plane((int)r, observe ? 5 : 6);
                        std::vector<double> v;                               // the numbers among the plane's values, sorted
                        for (size_t p = 0; p < npix; ++p) if (sd[p] == sd[p]) v.push_back(sd[p]);
                        std::sort(v.begin(), v.end());
                        const double nan = std::nan(""), vmax = v.empty() ? nan : v.back(), vmed = v.empty() ? nan : v[v.size() / 2];
                        if (observe) std::printf("uncertainty camera_%d sd_worst max %.17g median %.17g valid %lld\n", req[r].camera_a, vmax, vmed, unc.n_valid[r]);
                        else std::printf("uncertainty camera_%d->camera_%d sd_across max %.17g median %.17g valid %lld\n", req[r].camera_a, req[r].camera_b, vmax, vmed, unc.n_valid[r]);
                    }
                }
                if (suggest > 0 && cov.info.status == 0) {
                    if (suggest_distances.empty()) {
                        const double diag = cs.pitch * std::sqrt((double)((board.width - 1) * (board.width - 1) + (board.height - 1) * (board.height - 1)));
                        suggest_distances.push_back(5.0 * diag);
                        suggest_distances.push_back(10.0 * diag);
                    }
                    const std::vector<tscm::MultiCalib::SuggestedView> views = mul_calib.suggest_views(cov, image, suggest, suggest_distances);
                    for (size_t k = 0; k < views.size(); ++k) {
                        const tscm::MultiCalib::SuggestedView &v = views[k];
                        const bool pair = v.candidate.camera_a != v.candidate.camera_b;
                        std::printf("suggest %d camera_%d", (int)k, v.candidate.camera_a);
                        if (pair) std::printf("+camera_%d", v.candidate.camera_b);
                        std::printf(" pixel %.1f %.1f distance %.17g tilt %g %g gain_logdet %.17g gain_trace %.17g visible %d", v.pixel[0], v.pixel[1], v.distance, v.tilt_x,
                                    v.tilt_y, v.gain_logdet, v.gain_trace, v.n_visible[0]);
                        if (pair) std::printf(",%d", v.n_visible[1]);
                        std::printf("\n");
                    }
                }
            }
        } else if (C == 1) {
            const double I3[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, t0[3] = { 0, 0, 0 };
            tscm::check(tscm_yaml_write(argv[2], 1, cameras[0].intrinsic_.data(), I3, t0));
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    tscm_corners_free(&cs);
    return rc;
}
