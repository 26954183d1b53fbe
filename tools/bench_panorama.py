#!/usr/bin/env python3
"""Measurement of the panorama composer (tscm_panorama_*) on one MI355X.

Workload: the four cameras of the golden calibration, 1280 x 1080 x 3 hash-noise images, into a 2048 x 1024 equirect
panorama with radial weights.  Per mode (seam, feather, multiband with 4 levels): kernel seconds (HIP events, the
seconds_kernel of tscm_panorama_compose) and wall seconds per frame (upload, kernels, download) over --frames frames after
--warmup.  The baseline, measured in the same run, is the route without the composer: one maps.remap call per camera, each
of which uploads the image and both tables again, and a feather blend in numpy.  Prints ONE JSON line and writes it to
profiles/panorama_bench.json; the bytes per frame that each mode has to move are counted from the shapes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscm_calib_amd import calib_io, lib, maps, panorama, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0


def frame_bytes(mode, n, ch, npix, levels, covered):
    """Device bytes one frame has to move at the least (every buffer read or written once; the bilinear taps of a covered
    pixel counted as 4 source pixels).  covered = sum over the cameras of their covered pixels."""
    out = npix * ch
    if mode == "seam":
        return npix * (1 + 8) + npix * 4 * ch + out                       # label, one packed sample, its taps, the output
    if mode == "feather":
        return npix * 2 + covered * (8 + 4 * ch) + out                    # mask, the packed samples and taps of the covering cameras
    pyr = sum(npix >> (2 * l) for l in range(levels + 1))
    sample = n * npix * (8 + 4 * ch + 2 * ch)                             # every camera is sampled everywhere into int16 planes
    reduce_ = n * ch * 2 * (pyr + pyr - npix)                             # each level read once, each coarser level written once
    blend = n * pyr * (1 + 2 * ch) + pyr * (2 + 2 * ch)                   # masks and G of every camera, W, B written
    collapse = 2 * ch * 2 * (pyr - npix) + ch * 2 * npix + npix + out     # B^l read and written, level 0 read, coverage, the output
    return sample + reduce_ + blend + collapse


def hash_noise(k, w, h, ch):
    idx = np.arange(w * h * ch, dtype=np.uint64) + np.uint64(k) * np.uint64(w * h * ch)
    return (synth.splitmix64(idx) >> np.uint64(56)).astype(np.uint8).reshape(h, w, ch)


def numpy_feather(images, mapx, mapy, alphas):
    num = np.zeros(mapx.shape[1:] + (3,), np.int64)
    A = alphas.astype(np.int64).sum(axis=0)
    for k, img in enumerate(images):
        num += alphas[k].astype(np.int64)[..., None] * maps.remap(img, mapx[k], mapy[k]).astype(np.int64)
    return np.where(A[..., None] > 0, (num + (A >> 1)[..., None]) // np.maximum(A, 1)[..., None], 0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pano", type=int, nargs=2, default=[2048, 1024])
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panorama_bench.json"))
    a = ap.parse_args()
    if lib.lib().tscm_device_count() < 1:
        raise SystemExit("no HIP device: the composer has no CPU fallback and nothing is measured without one")
    intr, Twc = calib_io.read_calib_yaml(os.path.join(ROOT, "tests", "golden", "reference_calib.yaml"))
    n, w, h, ch = 4, 1280, 1080, 3
    pw, ph = a.pano
    images = [hash_noise(k, w, h, ch) for k in range(n)]
    out = dict(metric="panorama_frame_seconds", unit="s", n_gpus=1, higher_is_better=False, frames=a.frames, warmup=a.warmup,
               config=dict(workload=f"{n} cameras {w}x{h}x{ch} -> {pw}x{ph}, golden calibration, radial weights", levels=a.levels))
    feather_out = alphas = tables = None
    for mode in ("seam", "feather", "multiband"):
        with panorama.Composer(intr, Twc, (w, h), (pw, ph), channels=ch, mode=mode, levels=a.levels) as c:
            for _ in range(a.warmup):
                c.compose(images)
            kern, t0 = [], time.perf_counter()
            for _ in range(a.frames):
                res, sec = c.compose(images, with_seconds=True)
                kern.append(sec)
            wall = (time.perf_counter() - t0) / a.frames
            if mode == "feather":
                feather_out, alphas, tables = res, c.stages(images)["alpha"], (c.mapx, c.mapy)
            covered = int((alphas > 0).sum()) if alphas is not None else int((c.stages(images)["alpha"] > 0).sum())
        kern.sort()
        nbytes = frame_bytes(mode, n, ch, pw * ph, a.levels, covered)
        out[mode] = dict(seconds_kernel_median=kern[len(kern) // 2], seconds_kernel_min=kern[0], seconds_wall_per_frame=wall, bytes_per_frame=nbytes,
                         hbm_fraction=nbytes / kern[len(kern) // 2] / 1e9 / HBM_PEAK_GBS)
    # the route without the composer: n remap calls (image and tables uploaded every time) and a numpy feather
    for _ in range(2):
        base = numpy_feather(images, tables[0], tables[1], alphas)
    t0 = time.perf_counter()
    reps = max(2, a.frames // 5)
    for _ in range(reps):
        base = numpy_feather(images, tables[0], tables[1], alphas)
    base_wall = (time.perf_counter() - t0) / reps
    out["baseline_remap_numpy_feather"] = dict(seconds_wall_per_frame=base_wall, frames=reps, same_bytes_as_feather=bool(np.array_equal(base, feather_out)))
    out["speedup_wall_vs_baseline"] = {m: base_wall / out[m]["seconds_wall_per_frame"] for m in ("seam", "feather", "multiband")}
    out["value"] = out["multiband"]["seconds_wall_per_frame"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
