#!/usr/bin/env python3
"""Measurement of the RANSAC pose initialisation (tscm_estimate_extrinsic_ransac) on one MI355X.

Workload: 10,000 views of an 11 x 8 and of a 9 x 6 board (camera 0 of the synthetic rig, 0.1 px noise, 5 % of the corners of
every fourth view displaced by 30-200 px), one launch at 64, 256 and 1024 hypotheses.  Prints ONE JSON line: device
milliseconds of the kernel (HIP events around the launch, median of --repeats warm launches, min and max beside it), the
(hypothesis, corner) tests per second that makes, the share of views with a pose, and in the same run on the same data the
wall-clock milliseconds of the whole call beside those of tscm_estimate_extrinsic (uploads and read-back included in both:
the plain entry has no timer of its own).  None of these is a pass/fail bound.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscm_calib_amd import rig, synth  # noqa: E402

BOARDS = [(11, 8, 30.0), (9, 6, 45.0)]
HYPOTHESES = [64, 256, 1024]


def views(cols: int, rows: int, pitch: float, n_views: int):
    p = synth.make_problem(1, n_views, 17, noise_px=0.1, perturb=False, cols=cols, rows=rows, pitch=pitch)
    n = cols * rows
    pu, pv = p.obs_u.reshape(n_views, n).copy(), p.obs_v.reshape(n_views, n).copy()
    rng = np.random.default_rng(3)
    hit = np.zeros((n_views, n), dtype=bool)
    hit[::4] = rng.random((len(range(0, n_views, 4)), n)) < 0.05
    ang, r = rng.uniform(0, 2 * np.pi, (n_views, n)), rng.uniform(30, 200, (n_views, n))
    pu[hit] += (r * np.cos(ang))[hit]
    pv[hit] += (r * np.sin(ang))[hit]
    W = np.concatenate([p.board_xy, np.zeros((n, 1))], axis=1)
    return p.meta["gt_intr"][0].copy(), pu, pv, np.full(n_views, n, dtype=np.int32), W


def median3(values):
    values = sorted(values)
    return dict(ms=1e3 * values[len(values) // 2], ms_min=1e3 * values[0], ms_max=1e3 * values[-1])


def wall(f, warmup: int, repeats: int):
    for _ in range(warmup):
        f()
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        f()
        out.append(time.perf_counter() - t)
    return median3(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    rows = []
    for cols, brows, pitch in BOARDS:
        intr, pu, pv, count, W = views(cols, brows, pitch, a.views)
        n = cols * brows
        plain = wall(lambda: rig.estimate_extrinsic(intr, pu, pv, count, W, cols, a.device), a.warmup, a.repeats)
        for H in HYPOTHESES:
            prm = rig.ransac_params(threshold_px=2.0, n_hypotheses=H, seed=1)
            call = lambda: rig._ransac_call(False, intr, pu, pv, count, W, cols, prm, a.device, None)      # noqa: E731
            for _ in range(a.warmup):
                call()
            kernel = median3([call()["seconds_kernel"] for _ in range(a.repeats)])
            r = call()
            rows.append(dict(board=f"{cols}x{brows}", corners=n, hypotheses=H, kernel=kernel,
                             tests_per_s=a.views * H * n / (1e-3 * kernel["ms"]), share_with_pose=r["n_estimated"] / a.views,
                             mean_inliers=float(r["n_inliers"].mean()), call_wall=wall(call, 0, a.repeats), plain_call_wall=plain))
    print(json.dumps(dict(tool="bench_init_ransac", views=a.views, repeats=a.repeats, rows=rows)))


if __name__ == "__main__":
    main()
