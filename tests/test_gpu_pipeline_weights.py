"""pipeline.calibrate_camera(..., ransac=params, mask_outliers=True): the RANSAC inlier mask is the corner mask of the
refinement -- the bytes of api.refinement called by hand with the returned mask -- and without it the result is today's."""
import numpy as np
import pytest

from tscm_calib_amd import api, pipeline, rig
from tests.test_gpu_pipeline_ransac import COLS, PITCH, ROWS, SIZE, _views

pytestmark = pytest.mark.gpu


def test_mask_outliers_is_the_refinement_with_the_inlier_mask(hip_device):
    truth, clean, bad, moved = _views()
    has = np.ones(12, dtype=np.uint8)
    prm = rig.ransac_params(seed=0)
    intr, Rt, s = pipeline.calibrate_camera(*bad, has, COLS, ROWS, PITCH, SIZE, hip_device, ransac=prm, mask_outliers=True)
    f = s["ransac"]
    kept = f["has"].astype(bool)
    mask = np.asarray(f["inlier"], dtype=bool)[kept]
    assert not kept.all() and not mask.all()                   # a view was dropped and corners of kept views are masked
    assert s["n_residual_blocks"] == int(mask.sum())
    # by hand: the same start (the pipeline's own preparation), then the refinement with the returned mask
    q, count, sel, found = pipeline._prepare_camera(*bad, has, COLS, ROWS, PITCH, SIZE, hip_device, None, "ts", prm)
    assert np.array_equal(found["inlier"], f["inlier"]) and np.array_equal(np.flatnonzero(kept), sel)
    _, r = api.refinement(q, hip_device, weights=mask.ravel())
    hi, hRt = pipeline._finish_camera(q, count, sel)
    assert np.array_equal(hi, intr) and np.array_equal(hRt, Rt)
    assert r["iterations"] == s["iterations"] and r["rmse"] == s["rmse"] and r["final_cost"] == s["final_cost"]
    # the mask takes out what the plain refinement keeps: the masked solve fits its corners better
    _, _, s0 = pipeline.calibrate_camera(*bad, has, COLS, ROWS, PITCH, SIZE, hip_device, ransac=prm)
    assert s0["n_residual_blocks"] == int(kept.sum()) * COLS * ROWS and s["rmse"] < s0["rmse"]


def test_without_mask_outliers_the_result_is_todays(hip_device):
    truth, clean, bad, moved = _views()
    has = np.ones(12, dtype=np.uint8)
    prm = rig.ransac_params(seed=0)
    a = pipeline.calibrate_camera(*bad, has, COLS, ROWS, PITCH, SIZE, hip_device, ransac=prm)
    b = pipeline.calibrate_camera(*bad, has, COLS, ROWS, PITCH, SIZE, hip_device, ransac=prm, mask_outliers=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2]["iterations"] == b[2]["iterations"]
    # without ransac parameters the switch changes nothing either
    c = pipeline.calibrate_camera(*clean, has, COLS, ROWS, PITCH, SIZE, hip_device)
    d = pipeline.calibrate_camera(*clean, has, COLS, ROWS, PITCH, SIZE, hip_device, mask_outliers=True)
    assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1]) and "ransac" not in d[2]


_rig_cache = {}


def _rig_images():
    """The rendered two-camera rig of test_gpu_pipeline.py and RANSAC parameters tight enough (0.3 px on detected corners: 65-95 % of the corners of the kept views are inliers)
    that the consensus sets leave corners out, so the masks below are not all-ones."""
    if not _rig_cache:
        from tests.test_gpu_pipeline import _render_rig
        _rig_cache["images"] = _render_rig(31, 10)[2]
        _rig_cache["prm"] = rig.ransac_params(threshold_px=0.3, seed=0)
    return _rig_cache["images"], _rig_cache["prm"]


def _same_summary(a, b):
    return all(a[k] == b[k] for k in ("iterations", "final_cost", "rmse", "n_residual_blocks", "termination_type"))


def test_monocular_calib_masks_both_refinements(hip_device):
    images, prm = _rig_images()
    out = pipeline.monocular_calib(images[0], 9, 6, 45.0, device=hip_device, ransac=prm, mask_outliers=True)
    # by hand: detection, then calibrate_camera with the mask on the detected and on the refined corners
    size, has, pu, pv = pipeline._detect(images[0], 9, 6, 4, hip_device)
    i1, Rt1, first = pipeline.calibrate_camera(pu, pv, has, 9, 6, 45.0, size, hip_device, ransac=prm, mask_outliers=True)
    assert _same_summary(first, out["first"])
    has1 = first["ransac"]["has"]
    warm = i1 if first["termination_type"] == 0 else None
    i2, Rt2, second = pipeline.calibrate_camera(out["pix_u"], out["pix_v"], has1, 9, 6, 45.0, size, hip_device, init_intr=warm, ransac=prm,
                                                mask_outliers=True)
    assert _same_summary(second, out["second"]) and np.array_equal(i2, out["intr"]) and np.array_equal(Rt2, out["Rt"])
    kept = out["ransac"]["has"].astype(bool)
    mask = np.asarray(out["ransac"]["inlier"], dtype=bool)[kept]
    assert not mask.all() and out["second"]["n_residual_blocks"] == int(mask.sum())
    # without the switch: today's calls
    a = pipeline.monocular_calib(images[0], 9, 6, 45.0, device=hip_device, ransac=prm)
    b = pipeline.monocular_calib(images[0], 9, 6, 45.0, device=hip_device, ransac=prm, mask_outliers=False)
    assert np.array_equal(a["intr"], b["intr"]) and _same_summary(a["second"], b["second"])
    assert a["second"]["n_residual_blocks"] == int(a["ransac"]["has"].sum()) * 54 and not np.array_equal(a["intr"], out["intr"])


def test_monocular_calib_batch_masks_like_the_solo_calls(hip_device):
    images, prm = _rig_images()
    # one batched calibrate of both cameras against calibrate_camera alone, on the same detections: the RANSAC stage sees the same
    # input, so the masks are equal, and the batched refinement meets the solo one at the bounds of tests/test_gpu_mono_batch_rig.py
    det = [pipeline._detect(imgs, 9, 6, 4, hip_device) for imgs in images]
    args = ([d[2] for d in det], [d[3] for d in det], [d[1] for d in det], 9, 6, 45.0, [d[0] for d in det], hip_device, [None, None], None, "ts",
            np.zeros(2, dtype=np.uint16), prm)
    bat = pipeline._calibrate_cameras_batched(*args, True)
    for m, (bi, bRt, bs) in enumerate(bat):
        si, sRt, ss = pipeline.calibrate_camera(det[m][2], det[m][3], det[m][1], 9, 6, 45.0, det[m][0], hip_device, ransac=prm, mask_outliers=True)
        assert np.array_equal(ss["ransac"]["inlier"], bs["ransac"]["inlier"]) and np.array_equal(ss["ransac"]["has"], bs["ransac"]["has"])
        mask = np.asarray(bs["ransac"]["inlier"], dtype=bool)[bs["ransac"]["has"].astype(bool)]
        assert not mask.all() and bs["n_residual_blocks"] == ss["n_residual_blocks"] == int(mask.sum())
        assert bs["num_iterations"] == ss["num_iterations"] and bs["termination_type"] == ss["termination_type"]
        assert np.max(np.abs(bi[:7] - si[:7]) / np.abs(si[:7]).clip(1e-3)) < 1e-6
    # the whole batched flow carries the switch into both passes
    out = pipeline.monocular_calib_batch(images, 9, 6, 45.0, device=hip_device, ransac=prm, mask_outliers=True)
    for o in out:
        assert o["second"]["n_residual_blocks"] == int(np.asarray(o["ransac"]["inlier"], dtype=bool)[o["has"].astype(bool)].sum())
    plain = pipeline.monocular_calib_batch(images, 9, 6, 45.0, device=hip_device, ransac=prm)
    off = pipeline.monocular_calib_batch(images, 9, 6, 45.0, device=hip_device, ransac=prm, mask_outliers=False)
    for a, b in zip(plain, off):
        assert np.array_equal(a["intr"], b["intr"]) and _same_summary(a["second"], b["second"])
        assert a["second"]["n_residual_blocks"] == int(a["has"].sum()) * 54


def test_calibrate_rig_masks_the_joint_solve_and_the_covariance(hip_device):
    images, prm = _rig_images()
    out = pipeline.calibrate_rig(images, 9, 6, 45.0, device=hip_device, ransac=prm, mask_outliers=True, covariance=True)
    mono, cw = out["mono"], out["corner_mask"]
    # by hand: the rig initialisation's problem, then the joint solve and the covariance with the masks of the mono stage
    W = pipeline.board_points(9, 6, 45.0)
    inp = rig.RigInput(W, np.stack([m["intr"] for m in mono]), np.stack([m["has"] for m in mono]), np.stack([m["Rt"] for m in mono]),
                       np.stack([m["pix_u"] for m in mono]), np.stack([m["pix_v"] for m in mono])).normalised()
    p = rig.problem_from_rig(inp, out["rig_init"])
    want = np.concatenate([np.asarray(mono[m]["ransac"]["inlier"], dtype=bool)[i] for m, i in zip(p.view_camera, p.view_board)])
    assert np.array_equal(cw, want) and not cw.all()
    s = api.calibrate(p, hip_device, weights=cw)
    assert _same_summary(s, out["summary"]) and s["n_residual_blocks"] == int(cw.sum())
    assert all(np.array_equal(getattr(p, k), getattr(out["problem"], k)) for k in ("cam_rt", "intr", "board_rt"))
    c = api.covariance(p, hip_device, weights=cw)
    assert np.array_equal(c["cam_cov"], out["covariance"]["cam_cov"]) and c["dof"] == out["covariance"]["dof"] == 2 * int(cw.sum()) - c["n_free"]
    # without the switch: today's calls
    a = pipeline.calibrate_rig(images, 9, 6, 45.0, device=hip_device, ransac=prm, covariance=True)
    b = pipeline.calibrate_rig(images, 9, 6, 45.0, device=hip_device, ransac=prm, covariance=True, mask_outliers=False)
    assert "corner_mask" not in a and _same_summary(a["summary"], b["summary"]) and np.array_equal(a["problem"].intr, b["problem"].intr)
    assert a["summary"]["n_residual_blocks"] == a["problem"].n_corners and a["covariance"]["dof"] == b["covariance"]["dof"]


CPP = r"""
#include <cstdio>
#include <vector>
#include "tscm/tscm_calib.hpp"
// a mono problem and its corner weights from a binary file, refined through the mirror header
int main(int argc, char **argv)
{
    FILE *f = std::fopen(argv[1], "rb");
    int hdr[2];
    if (!f || std::fread(hdr, sizeof(int), 2, f) != 2) return 2;
    const int n = hdr[0], V = hdr[1];
    std::vector<double> xy(2 * n), u((size_t)n * V), v((size_t)n * V), w((size_t)n * V), intr(9), rt(6 * (size_t)V);
    if (std::fread(xy.data(), 8, xy.size(), f) != xy.size() || std::fread(u.data(), 8, u.size(), f) != u.size() ||
        std::fread(v.data(), 8, v.size(), f) != v.size() || std::fread(w.data(), 8, w.size(), f) != w.size() ||
        std::fread(intr.data(), 8, 9, f) != 9 || std::fread(rt.data(), 8, rt.size(), f) != rt.size()) return 2;
    std::fclose(f);
    tscm::TripleSphereCamera cam;
    cam.intrinsic_ = intr;
    std::vector<tscm::Point3d> worlds(n);
    for (int j = 0; j < n; ++j) { worlds[j].x = xy[2 * j]; worlds[j].y = xy[2 * j + 1]; worlds[j].z = 0.0; }
    std::vector<std::vector<tscm::Point2d> > pixels(V, std::vector<tscm::Point2d>(n));
    std::vector<std::vector<double> > weights(V, std::vector<double>(n));
    for (int i = 0; i < V; ++i) {
        cam.rt_.push_back(std::vector<double>(&rt[6 * (size_t)i], &rt[6 * (size_t)i] + 6));
        cam.has_chessboard_.push_back(true);
        for (int j = 0; j < n; ++j) { pixels[i][j].x = u[(size_t)n * i + j]; pixels[i][j].y = v[(size_t)n * i + j]; weights[i][j] = w[(size_t)n * i + j]; }
    }
    cam.set_corner_weights(&weights);
    const bool ok = cam.refinement(pixels, worlds);
    std::printf("%d %.17g %.17g %.17g %.17g %.17g %d %.17g\n", ok ? 1 : 0, cam.intrinsic_[0], cam.intrinsic_[1], cam.intrinsic_[2],
                cam.intrinsic_[3], cam.summary.final_cost, cam.summary.n_residual_blocks, cam.summary.rmse);
    cam.set_corner_weights(NULL);
    cam.intrinsic_ = intr;
    for (int i = 0; i < V; ++i) cam.rt_[i].assign(&rt[6 * (size_t)i], &rt[6 * (size_t)i] + 6);
    cam.refinement(pixels, worlds);
    std::printf("%.17g %d\n", cam.summary.final_cost, cam.summary.n_residual_blocks);
    return 0;
}
"""


def test_cpp_host_program_sets_corner_weights(hip_device, tmp_path):
    """A C++11 host program built against include/tscm/tscm_calib.hpp: TripleSphereCamera::set_corner_weights + refinement() is
    api.refinement(weights=...) on the same problem -- general weights and a view whose weights are all 0 -- and
    set_corner_weights(NULL) is the plain refinement again."""
    import os
    import subprocess
    from tscm_calib_amd import synth
    from tests import weights_ref as W
    from tests.test_gpu_robust import _corrupt
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "tscm_calib_amd", "csrc")
    src, exe = tmp_path / "weights_host.cpp", str(tmp_path / "weights_host")
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(root, "include"), str(src), "-L", csrc, "-ltscm_hip",
                           "-Wl,-rpath," + csrc, "-o", exe])
    p = _corrupt(synth.make_problem(1, 12, 808).normalised())
    n, V = p.n_points, p.n_views
    assert (p.view_count == n).all() and (p.view_board == np.arange(V)).all()
    w = W.scattered_weights(p, 12)
    w[3 * n:4 * n] = 0.0                                        # view 3: every weight 0
    with open(tmp_path / "problem.bin", "wb") as f:
        f.write(np.array([n, V], dtype=np.int32).tobytes())
        for a in (p.board_xy, p.obs_u, p.obs_v, w, p.intr, p.board_rt):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    lines = subprocess.check_output([exe, str(tmp_path / "problem.bin")], timeout=120).decode().splitlines()
    out = lines[0].split()
    q = p.copy().normalised()
    _, r = api.refinement(q, hip_device, weights=w)
    assert int(out[0]) == (r["termination_type"] == 0)
    assert np.array_equal(np.array([float(x) for x in out[1:5]]), q.intr[0, :4])
    assert float(out[5]) == r["final_cost"] and int(out[6]) == r["n_residual_blocks"] == int(np.sum(w > 0)) and float(out[7]) == r["rmse"]
    # weights cleared: the plain refinement of all corners, which is another solve
    plain = p.copy().normalised()
    _, r0 = api.refinement(plain, hip_device)
    assert float(lines[1].split()[0]) == r0["final_cost"] and int(lines[1].split()[1]) == r0["n_residual_blocks"] == p.n_corners
    assert not np.array_equal(plain.intr[0, :4], q.intr[0, :4])
