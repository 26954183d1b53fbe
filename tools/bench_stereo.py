#!/usr/bin/env python3
"""Measurement of the stereo matcher (tscm_stereo_match) on one MI355X.

Workload: one rectified pair of 1280 x 640 pixels, 128 disparities, with 4 and with 8 paths.  Prints ONE JSON line: device
milliseconds per pair (HIP events around the kernels, median of --repeats warm calls), each stage's share of it, the bytes
the design moves through device memory (counted from the shapes, below) and the fraction of the streaming rate of HBM that
this traffic over the measured time amounts to.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscm_calib_amd import stereo  # noqa: E402

HBM_MEASURED_BS = 6.29e12        # float4 copy on the MI355X (8.0e12 by specification)
HBM_SPEC_BS = 8.0e12
SEGMENT = 256                    # kCostSegment of tscm_stereo.hip


def design_bytes(w: int, h: int, D: int, paths: int, left_right: bool) -> dict:
    """Bytes each stage reads and writes in device memory: census uint64, C uint8 [h][w][D], S uint16 [h][w][D]."""
    px, vol = w * h, w * h * D
    agg = paths * vol + 2 * vol + (paths - 1) * 4 * vol           # C read per direction; S written once, then read + written
    b = dict(census=2 * (px + 8 * px), cost=2 * 8 * px + vol, aggregate=agg,
             right_winner=(2 * vol * (SEGMENT + D - 1) // SEGMENT + 2 * px) if left_right else 0,
             winner=2 * vol + 2 * px + (2 * px if left_right else 0))
    b["total"] = sum(b.values())
    return b


def make_pair(w: int, h: int, seed: int = 7):
    """Noise with a disparity that grows down the image from 4 to 100 pixels: every row has its match inside the range."""
    src = np.random.default_rng(seed).integers(0, 256, (h, w + 128)).astype(np.uint8)
    d = 4 + (96 * np.arange(h)) // h
    left = np.stack([src[y, 128 - d[y]:128 - d[y] + w] for y in range(h)])
    return left, src[:, 128:128 + w].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--disparities", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    left, right = make_pair(a.width, a.height)
    out = dict(metric="stereo_match_kernel_ms_per_pair", unit="ms", n_gpus=1, higher_is_better=False, data="synthetic",
               config=dict(width=a.width, height=a.height, num_disparities=a.disparities, repeats=a.repeats,
                           hbm_rate_bytes_per_s=HBM_MEASURED_BS, hbm_spec_bytes_per_s=HBM_SPEC_BS))
    for paths in (4, 8):
        p = dict(num_disparities=a.disparities, paths=paths)
        for _ in range(a.warmup):
            stereo.match(left, right, **p)
        runs = []
        for _ in range(a.repeats):
            disp, sec = stereo.match(left, right, with_seconds=True, **p)
            runs.append((sec, stereo.stage_times()))
        runs.sort(key=lambda r: r[0])
        sec, stages = runs[len(runs) // 2]
        b = design_bytes(a.width, a.height, a.disparities, paths, True)
        floor_ms = 1e3 * b["total"] / HBM_MEASURED_BS
        out[f"paths_{paths}"] = dict(
            ms=1e3 * sec, ms_min=1e3 * runs[0][0], ms_max=1e3 * runs[-1][0],
            stage_ms={k: 1e3 * v for k, v in stages.items()}, stage_share={k: v / sec for k, v in stages.items()},
            bytes=b, traffic_floor_ms=floor_ms, achieved_bytes_per_s=b["total"] / sec, frac_of_hbm_rate=b["total"] / sec / HBM_MEASURED_BS,
            aggregate_frac_of_hbm_rate=b["aggregate"] / stages["aggregate"] / HBM_MEASURED_BS,
            valid_share=float(np.mean(disp != -16)))
    out["value"] = out["paths_8"]["ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
