#!/usr/bin/env python3
"""Measurement of the projection uncertainty stage (tscm_projection_uncertainty) on one MI355X.

Workload: a 4-camera rig at 1280 x 1080 with step 1 -- 4 observe requests and the 12 ordered camera pairs, 16 requests of
1,382,400 pixels in one launch -- at the generator's parameters with the covariance of api.covariance.  Prints ONE JSON
line and writes it to profiles/bench_uncertainty.json: device milliseconds of the kernel (HIP events around the launch,
median of --repeats warm calls, min and max beside it), pixels per second, the counted fp64 flops per pixel and their share
of the device's vector fp64 peak, the wall time of the whole call (uploads and the read-back of the 1.2 GB of planes
included), and -- for orientation only -- the wall time of the float64 numpy restatement (tests/uncert_ref.py) of the same
requests on a grid of step --numpy-step, scaled to pixels per second.  None of these is a pass/fail bound: the stage has no
earlier code path to compare with.  Not measured: hardware counters, achieved occupancy, LDS bank conflicts."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscm_calib_amd import api, lib, synth  # noqa: E402

# fp64 operations of one valid pixel as the kernel's source states them (a multiply-add counts 2, a division, a square
# root 1 each): the quadratic form is n (n - 1) / 2 off-diagonal entries of 4 and n rows of 13
FLOPS_QUAD = lambda n: 4 * n * (n - 1) // 2 + 13 * n
# ahead of it (unprojection and its three checks 65, s / D / p_b 42, projection with A and G 86, camera b's columns 81, the
# standard deviations 16; a transfer adds AR and M 60, camera a's columns 81, the second projection 86, the 2 x 2 solve and
# the I_a columns 79, e and sd_across 34)
FLOPS_CHAIN = dict(observe=65 + 42 + 86 + 81 + 16, transfer=65 + 42 + 86 + 81 + 16 + 60 + 81 + 86 + 79 + 34)


def flops_per_pixel(transfer: bool) -> int:
    return FLOPS_QUAD(26 if transfer else 13) + FLOPS_CHAIN["transfer" if transfer else "observe"]


def spread(values):
    values = sorted(values)
    return dict(ms=1e3 * values[len(values) // 2], ms_min=1e3 * values[0], ms_max=1e3 * values[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--step", type=float, default=1.0)
    ap.add_argument("--inv-distance", type=float, default=1.0 / 300)
    ap.add_argument("--numpy-step", type=float, default=40.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_uncertainty.json"))
    a = ap.parse_args()
    p = synth.make_problem(4, 30, 99, noise_px=0.1)
    w, h = int(synth.IMG_W), int(synth.IMG_H)
    cov = api.covariance(p, a.device)
    Cn = p.n_cameras
    requests = [(m, m, a.inv_distance) for m in range(Cn)] + [(i, j, a.inv_distance) for i in range(Cn) for j in range(Cn) if i != j]
    grid = api.uncertainty_grid(int((w - 1) // a.step) + 1, int((h - 1) // a.step) + 1, 0.0, 0.0, a.step, a.step, w, h)
    for _ in range(a.warmup):
        api.projection_uncertainty(p.cam_rt, p.intr, cov, requests, grid, a.device)
    kernel, wall = [], []
    for _ in range(a.repeats):
        t = time.perf_counter()
        r = api.projection_uncertainty(p.cam_rt, p.intr, cov, requests, grid, a.device)
        wall.append(time.perf_counter() - t)
        kernel.append(r["seconds_kernel"])
    npix = grid["nx"] * grid["ny"]
    valid = r["n_valid"]
    flops = float(sum(int(valid[k]) * flops_per_pixel(q[0] != q[1]) for k, q in enumerate(requests)))
    mfma, valu = C.c_double(0.0), C.c_double(0.0)              # measured ceilings, TFLOP/s: the stage is v_fma_f64 work
    vector_peak = float("nan")
    if lib.lib().tscm_device_peak_fp64(a.device, C.byref(mfma), C.byref(valu)) == 0:
        vector_peak = valu.value * 1e12
    k = spread(kernel)
    sec = k["ms"] * 1e-3
    # the float64 numpy restatement on a coarser grid
    sys.path.insert(0, ROOT)
    from tests import uncert_ref as U
    g2 = api.uncertainty_grid(int((w - 1) // a.numpy_step) + 1, int((h - 1) // a.numpy_step) + 1, 0.0, 0.0, a.numpy_step, a.numpy_step, w, h)
    t = time.perf_counter()
    ref = U.uncertainty_ref(p.cam_rt, p.intr, cov["cam_cov"], cov["sigma2"], requests, g2, dtype=np.float64)
    t_numpy = time.perf_counter() - t
    dev2 = api.projection_uncertainty(p.cam_rt, p.intr, cov, requests, g2, a.device)
    both = ((ref["flags"] & 3) == 3) & ((dev2["flags"] & 3) == 3)
    diff = float(np.max(np.abs(dev2["sd_worst"][both] - np.asarray(ref["planes"][:, 5], dtype=np.float64)[both]) / np.asarray(ref["planes"][:, 5], dtype=np.float64)[both]))
    row = dict(tool="bench_uncertainty", repeats=a.repeats, cameras=Cn, image=[w, h], step=a.step, inv_distance=a.inv_distance, requests=len(requests),
               pixels_per_request=npix, pixels=npix * len(requests), valid_pixels=int(valid.sum()), sigma2=cov["sigma2"], kernel=k,
               pixels_per_s=npix * len(requests) / sec, counted_flops=flops, gflops=flops / sec * 1e-9, vector_peak_gflops=vector_peak * 1e-9 if vector_peak == vector_peak else None,
               share_of_vector_peak=(flops / sec / vector_peak) if vector_peak == vector_peak and vector_peak > 0 else None,
               flops_per_pixel=dict(observe=flops_per_pixel(False), transfer=flops_per_pixel(True)), call_wall=spread(wall),
               numpy_restatement=dict(step=a.numpy_step, pixels=g2["nx"] * g2["ny"] * len(requests), s=t_numpy, pixels_per_s=g2["nx"] * g2["ny"] * len(requests) / t_numpy,
                                      max_rel_diff_sd_worst=diff),
               not_measured=["hardware counters", "achieved occupancy", "LDS bank conflicts"])
    line = json.dumps(row)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
