#!/usr/bin/env python3
"""Measurement of the disparity post-filter (tscm_stereo_filter) on one MI355X.

Workload: one 1280 x 640 disparity map, speckle rule only (window 100, range 2) and speckle rule + 5 x 5 masked median,
on two inputs: the output of tscm_stereo_match on the synthetic pair of tools/bench_stereo.py, and the worst case for
union-find, one serpentine component (every second row valid, joined alternately at the right and left ends).  Prints ONE
JSON line: device milliseconds per map (HIP events around the kernels, median of --repeats warm calls), the bytes the design
moves through device memory (counted from the shapes, below), their fraction of the streaming rate of HBM over the
measured time, and the ratio to the numpy restatement tests/stereo_filter_ref.py on the host (and to a scipy.ndimage
labelling of the valid mask where scipy is importable).  None of these is a pass/fail bound.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscm_calib_amd import stereo  # noqa: E402
from tests import stereo_filter_ref as F  # noqa: E402

HBM_MEASURED_BS = 6.29e12        # float4 copy on the MI355X, the rate DESIGN section 17 uses
TILE_W, TILE_H = 64, 16          # kTileW, kTileH of tscm_stereo_filter.hip


def design_bytes(w: int, h: int, median: int) -> dict:
    """Bytes each kernel reads and writes in device memory: d int16, parent / cnt / label / rootsize int32, all [h][w].
    Pointer chases and atomics are counted once per element they touch at least."""
    n, r = w * h, median // 2
    pairs = ((w - 1) // TILE_W) * h + ((h - 1) // TILE_H) * w
    halo = (TILE_W + 2 * r) * (TILE_H + 2 * r) / (TILE_W * TILE_H)
    b = dict(ccl_tile=2 * n + 4 * n + 4 * n,                       # d in; parent, cnt out
             ccl_seams=pairs * (2 * 2 + 2 * 4 + 4),                # two d, two parents, one atomic
             ccl_flatten=4 * n + 4 * n + 4 * n,                    # parent in; label, rootsize out
             ccl_count=4 * n + 4 * n,                              # cnt in; label in and one atomic at tile roots (upper bound)
             speckle_median=int(halo * n * (2 + 4 + 4)) + 2 * n)   # d, label, rootsize[label] with the halo; out
    b["total"] = sum(b.values())
    return b


def make_pair(w: int, h: int, seed: int = 7):
    """tools/bench_stereo.py's pair: noise with a disparity that grows down the image from 4 to 100 pixels."""
    src = np.random.default_rng(seed).integers(0, 256, (h, w + 128)).astype(np.uint8)
    d = 4 + (96 * np.arange(h)) // h
    left = np.stack([src[y, 128 - d[y]:128 - d[y] + w] for y in range(h)])
    return left, src[:, 128:128 + w].copy()


def serpentine(w: int, h: int) -> np.ndarray:
    d = np.full((h, w), -16, dtype=np.int16)
    d[0::2] = 320
    for j, y in enumerate(range(1, h - 1, 2)):
        d[y, w - 1 if j % 2 == 0 else 0] = 320
    return d


def median_seconds(f, repeats: int) -> float:
    runs = []
    for _ in range(repeats):
        t = time.perf_counter()
        f()
        runs.append(time.perf_counter() - t)
    return sorted(runs)[len(runs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-repeats", type=int, default=3)
    a = ap.parse_args()
    w, h = a.width, a.height
    left, right = make_pair(w, h)
    inputs = dict(matcher=stereo.match(left, right, num_disparities=128, paths=8), serpentine=serpentine(w, h))
    out = dict(metric="stereo_filter_kernel_ms_per_map", unit="ms", n_gpus=1, higher_is_better=False, data="synthetic",
               config=dict(width=w, height=h, speckle_window_size=100, speckle_range=2, repeats=a.repeats, hbm_rate_bytes_per_s=HBM_MEASURED_BS))
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for name, disp in inputs.items():
        res = dict(valid_share=float(np.mean(disp != -16)))
        for tag, median in (("speckle", 0), ("speckle_median5", 5)):
            p = dict(speckle_window_size=100, speckle_range=2, median=median)
            for _ in range(a.warmup):
                stereo.filter(disp, **p)
            runs = sorted(stereo.filter(disp, with_seconds=True, **p)[1] for _ in range(a.repeats))
            sec = runs[len(runs) // 2]
            got = stereo.filter(disp, **p)
            host = median_seconds(lambda: F.filter(disp, **p), a.host_repeats)
            b = design_bytes(w, h, median)
            res[tag] = dict(ms=1e3 * sec, ms_min=1e3 * runs[0], ms_max=1e3 * runs[-1], bytes=b, traffic_floor_ms=1e3 * b["total"] / HBM_MEASURED_BS,
                            frac_of_hbm_rate=b["total"] / sec / HBM_MEASURED_BS, numpy_ms=1e3 * host, numpy_over_device=host / sec,
                            equal_to_numpy=bool(np.array_equal(got, F.filter(disp, **p))), removed_share=float(np.mean((disp != -16) & (got == -16))))
        if ndimage is not None:
            def scipy_label():
                lab, _ = ndimage.label(disp != -16)          # the valid mask only: no range test, so a lower bound of the work
                return np.bincount(lab.ravel())[lab]
            t = median_seconds(scipy_label, a.host_repeats)
            res["scipy_label_ms"] = 1e3 * t
            res["scipy_label_over_device"] = t / (1e-3 * res["speckle"]["ms"])
        out[name] = res
    out["value"] = out["matcher"]["speckle"]["ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
