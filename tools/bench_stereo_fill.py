#!/usr/bin/env python3
"""Measurement of the hole filling (tscm_stereo_fill) on one MI355X.

Workload: int16 maps of 1024 x 512 and 640 x 320, filled with the defaults plus wrap_x = 1 (MEDIAN, 8 paths), on three
inputs: a smooth map with 30 % of its pixels knocked out at random, the index map that tscm_sweep_depth gives on the hashed
noise frame of tools/bench_sweep.py at that panorama size, and a map with a single valid pixel (the case in which a walk
per invalid pixel would do npix * (w + h) loads).  Prints ONE JSON line: device milliseconds per map (HIP events around the
kernels, median of --repeats warm calls), the bytes the design moves through device memory (counted from the shapes,
below) and their fraction of the streaming rate of HBM over the measured time, and in the same run on the same device
tscm_stereo_filter (speckle rule + 3 x 3 median) on the same map and the numpy restatement tests/stereo_fill_ref.py on the
host.  None of these is a pass/fail bound.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscm_calib_amd import stereo, sweep, synth  # noqa: E402
from tests import stereo_fill_ref as F  # noqa: E402

HBM_MEASURED_BS = 6.29e12        # float4 copy on the MI355X, the rate DESIGN section 17 uses
SWEEP_FRAME_MS = 3.49            # tscm_sweep_depth at 1024 x 512, 64 hypotheses, 8 paths


def design_bytes(w: int, h: int, paths: int = 8, wrap_x: int = 1) -> dict:
    """Bytes each kernel reads and writes in device memory: d int16 [h][w], one packed uint32 candidate plane [h][w] per
    direction, out int16, mask uint8.  The candidate planes, written once and read once, are 8 * paths of the bytes per pixel."""
    n = w * h
    b = dict(rows=2 * ((2 * n if wrap_x else 0) + 2 * n + 4 * n),     # per direction: the first pass with wrap_x, d in, plane out
             lines=(paths - 2) * (2 * n + 4 * n),                     # per direction: d in, plane out
             select=2 * n + 4 * paths * n + 2 * n + n)                # d and the planes in; out and mask
    b["total"] = sum(b.values())
    b["candidate_planes"] = 8 * paths * n
    return b


def hash_noise(k: int, w: int, h: int) -> np.ndarray:
    idx = np.arange(w * h, dtype=np.uint64) + np.uint64(k) * np.uint64(w * h)
    return (synth.splitmix64(idx) >> np.uint64(56)).astype(np.uint8).reshape(h, w)


def scattered(w: int, h: int, share: float = 0.3) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    d = (16 * (4 + (96 * yy) // h) + (xx & 15)).astype(np.int16)
    d[np.random.default_rng(7).random((h, w)) < share] = -16
    return d


def swept(w: int, h: int, device: int) -> np.ndarray:
    images = [hash_noise(k, int(synth.IMG_W), int(synth.IMG_H)) for k in range(4)]
    inv = sweep.inverse_distances(500.0, D=64)
    with sweep.Sweeper.from_rig(synth.CALIB_INTR, synth.CALIB_TWC, (int(synth.IMG_W), int(synth.IMG_H)), w, h, inv, device=device, paths=8) as s:
        return s.depth(images)


def single(w: int, h: int) -> np.ndarray:
    d = np.full((h, w), -16, dtype=np.int16)
    d[h // 3, w // 3] = 320
    return d


def device_ms(f, warmup: int, repeats: int) -> dict:
    for _ in range(warmup):
        f()
    runs = sorted(f()[-1] for _ in range(repeats))
    return dict(ms=1e3 * runs[len(runs) // 2], ms_min=1e3 * runs[0], ms_max=1e3 * runs[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    fill = dict(wrap_x=1)
    post = dict(speckle_window_size=100, speckle_range=2, median=3)
    out = dict(metric="stereo_fill_kernel_ms_per_map", unit="ms", n_gpus=1, higher_is_better=False, data="synthetic",
               config=dict(rule="median", paths=8, wrap_x=1, repeats=a.repeats, filter=post, hbm_rate_bytes_per_s=HBM_MEASURED_BS, sweep_frame_ms=SWEEP_FRAME_MS))
    for w, h in ((1024, 512), (640, 320)):
        b = design_bytes(w, h)
        size = dict(bytes=b, traffic_floor_ms=1e3 * b["total"] / HBM_MEASURED_BS)
        for name, d in (("scattered", scattered(w, h)), ("swept", swept(w, h, a.device)), ("single", single(w, h))):
            res = device_ms(lambda: stereo.fill(d, device=a.device, with_seconds=True, **fill), a.warmup, a.repeats)
            res["filter"] = device_ms(lambda: stereo.filter(d, device=a.device, with_seconds=True, **post), a.warmup, a.repeats)
            got, mask = stereo.fill(d, device=a.device, with_mask=True, **fill)
            runs = []
            for _ in range(a.host_repeats):
                t = time.perf_counter()
                ref = F.fill(d, **fill)
                runs.append(time.perf_counter() - t)
            host = sorted(runs)[len(runs) // 2]
            res.update(invalid_share=float(np.mean(d == -16)), left_invalid=int((mask == 2).sum()), frac_of_hbm_rate=b["total"] / (1e-3 * res["ms"]) / HBM_MEASURED_BS,
                       fill_over_filter=res["ms"] / res["filter"]["ms"], numpy_ms=1e3 * host, numpy_over_device=host / (1e-3 * res["ms"]),
                       equal_to_numpy=bool(np.array_equal(got, ref[0]) and np.array_equal(mask, ref[1])))
            size[name] = res
        size["single_over_scattered"] = size["single"]["ms"] / size["scattered"]["ms"]
        out[f"{w}x{h}"] = size
    out["share_of_a_sweep_frame"] = out["1024x512"]["swept"]["ms"] / SWEEP_FRAME_MS
    out["value"] = out["1024x512"]["swept"]["ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
