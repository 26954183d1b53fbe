#!/usr/bin/env python3
"""Measurement of the edge-aware weighted median (tscm_stereo_refine) on one MI355X.

Workload: int16 maps of 1024 x 512 and 640 x 320 with a hashed-noise guide, refined with wrap_x = 1 and the table of
sigma = 10 at radius 1, 3, 5 and 7, in one pass and in three, on a map without holes and on one with 90 % of its pixels
invalid (the ratio of the two shows whether the time depends on the map).  Prints ONE JSON line: device milliseconds per
call (HIP events around the launches, median of --repeats warm calls, min and max beside it), the compare-adds of the
bisection counted from the shapes and their rate, and in the same run on the same device what the stage stands beside in
the chain it joins: tscm_stereo_fill on the same map and one tscm_sweep_depth frame of the same panorama size.  One
configuration is compared with the numpy restatement tests/stereo_refine_ref.py.  None of these is a pass/fail bound.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscm_calib_amd import stereo, sweep, synth  # noqa: E402
from tests import stereo_refine_ref as R  # noqa: E402

SIGMA = 10.0


def compare_adds(w: int, h: int, radius: int, iterations: int) -> int:
    """What the bisection does whatever the map holds: 16 steps over the whole window per pixel and pass."""
    return w * h * (2 * radius + 1) ** 2 * 16 * iterations


def hash_noise(k: int, w: int, h: int) -> np.ndarray:
    idx = np.arange(w * h, dtype=np.uint64) + np.uint64(k) * np.uint64(w * h)
    return (synth.splitmix64(idx) >> np.uint64(56)).astype(np.uint8).reshape(h, w)


def smooth_map(w: int, h: int, share: float) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    d = (16 * (4 + (96 * yy) // h) + (xx & 15)).astype(np.int16)
    if share > 0:
        d[np.random.default_rng(7).random((h, w)) < share] = -16
    return d


def guide_image(w: int, h: int) -> np.ndarray:
    """Blocks of 16 x 16 pixels of one hashed grey level, +-4 of hashed noise on top: edges for the table to see"""
    blocks = hash_noise(9, (w + 15) // 16, (h + 15) // 16)
    g = np.kron(blocks, np.ones((16, 16), np.uint8))[:h, :w].astype(np.int64)
    return np.clip(g + (hash_noise(10, w, h).astype(np.int64) & 7) - 4, 0, 255).astype(np.uint8)


def device_ms(f, warmup: int, repeats: int) -> dict:
    for _ in range(warmup):
        f()
    runs = sorted(f()[-1] for _ in range(repeats))
    return dict(ms=1e3 * runs[len(runs) // 2], ms_min=1e3 * runs[0], ms_max=1e3 * runs[-1])


def sweep_frame_ms(w: int, h: int, device: int, warmup: int, repeats: int) -> dict:
    images = [hash_noise(k, int(synth.IMG_W), int(synth.IMG_H)) for k in range(4)]
    inv = sweep.inverse_distances(500.0, D=64)
    with sweep.Sweeper.from_rig(synth.CALIB_INTR, synth.CALIB_TWC, (int(synth.IMG_W), int(synth.IMG_H)), w, h, inv, device=device, paths=8) as s:
        return device_ms(lambda: s.depth(images, with_seconds=True), warmup, repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    table = stereo.range_weights(SIGMA)
    out = dict(metric="stereo_refine_kernel_ms_per_map", unit="ms", n_gpus=1, higher_is_better=False, data="synthetic",
               config=dict(sigma=SIGMA, wrap_x=1, fill_invalid=0, repeats=a.repeats, warmup=a.warmup, tile=[32, 8]))
    for w, h in ((1024, 512), (640, 320)):
        g = guide_image(w, h)
        maps = dict(all_valid=smooth_map(w, h, 0.0), invalid_90=smooth_map(w, h, 0.9))
        size = dict(fill=device_ms(lambda: stereo.fill(maps["invalid_90"], device=a.device, with_seconds=True, wrap_x=1), a.warmup, a.repeats),
                    sweep_frame=sweep_frame_ms(w, h, a.device, a.warmup, a.repeats))
        for radius in (1, 3, 5, 7):
            row = {}
            for iterations in (1, 3):
                res = {}
                for name, d in maps.items():
                    res[name] = device_ms(lambda: stereo.refine(d, g, device=a.device, weights=table, with_seconds=True, radius=radius, iterations=iterations, wrap_x=1),
                                          a.warmup, a.repeats)
                n = compare_adds(w, h, radius, iterations)
                res.update(compare_adds=n, compare_adds_per_s=n / (1e-3 * res["all_valid"]["ms"]),
                           invalid_90_over_all_valid=res["invalid_90"]["ms"] / res["all_valid"]["ms"],
                           over_fill=res["all_valid"]["ms"] / size["fill"]["ms"], share_of_a_sweep_frame=res["all_valid"]["ms"] / size["sweep_frame"]["ms"])
                row[f"iterations_{iterations}"] = res
            size[f"radius_{radius}"] = row
        out[f"{w}x{h}"] = size
    w, h = 640, 320                                             # the bits, once: the restatement is 49 x 49 numpy passes over the map
    d, g = smooth_map(w, h, 0.3), guide_image(w, h)
    out["equal_to_numpy"] = bool(np.array_equal(stereo.refine(d, g, device=a.device, weights=table, radius=3, wrap_x=1), R.refine(d, g, table, radius=3, wrap_x=1)))
    out["value"] = out["1024x512"]["radius_3"]["iterations_1"]["all_valid"]["ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
