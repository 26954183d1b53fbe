#!/usr/bin/env python3
"""Measurement of the composer at the swept depth (tscm_sweep_compose) on one MI355X.

Workload: the four cameras of the golden calibration (1280 x 1080, 3 channels of hashed noise), a 1024 x 512 panorama, 64
inverse-distance hypotheses.  Prints ONE JSON line and writes it to profiles/bench_sweep_compose.json: device milliseconds per
frame (HIP events around the kernels, median of --repeats warm calls) of SEAM, FEATHER and MULTIBAND at the index map the
depth pass gives for the frame and at a constant map, next to tscm_panorama_compose on the z = 0 tables in the same run on the
same device -- the yardstick: the static composer keeps its labels and mask pyramids per rig, this one builds them per frame --
and the bytes the design moves through device memory (counted from the shapes, below) with the time they take at the
streaming rate of HBM.  Nothing is asserted.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscm_calib_amd import panorama, sweep, synth  # noqa: E402

HBM_MEASURED_BS = 6.29e12        # float4 copy on the MI355X (8.0e12 by specification)
MODES = ("seam", "feather", "multiband")


def design_bytes(n: int, pw: int, ph: int, ch: int, mode: str, levels: int, static: bool = False) -> dict:
    """Bytes each step reads and writes in device memory.  Records are 8 bytes per camera and pixel, G and B int16, masks,
    labels, coverage and the output uint8, W uint16, the index map int16.  The source images (gathered, and mostly resident in
    the caches) are not counted, nor is the halo a tile reads beyond its own pixels.  static: tscm_panorama_compose, which
    reads its label or coverage mask per pixel and keeps the mask pyramids and W per rig."""
    px = pw * ph
    if mode != "multiband":
        head = (1 if mode == "seam" else 2) * px if static else 2 * px + px      # label / mask, or index in and coverage out
        b = dict(compose=head + n * px * 8 + ch * px)
        b["total"] = b["compose"]
        return b
    lv = [(pw >> l) * (ph >> l) for l in range(levels + 1)]
    b = dict(gather=n * px * 8 + n * ch * px * 2 + (0 if static else 2 * px + 2 * px + n * px))
    b["reduce"] = sum((lv[l] + lv[l + 1]) * (n * ch * 2 + (0 if static else n)) for l in range(levels))
    b["wsum"] = 0 if static else sum(lv) * (n + 2)
    b["lapblend"] = sum(lv[l] * (n * ch * 2 + n + 2 + ch * 2) + (lv[l + 1] * n * ch * 2 if l < levels else 0) for l in range(levels + 1))
    b["collapse"] = sum(lv[l] * ch * 2 * 2 + lv[l + 1] * ch * 2 for l in range(1, levels)) + lv[0] * (ch * 2 + 1 + ch) + lv[1] * ch * 2
    b["total"] = sum(b.values())
    return b


def hash_noise(k: int, w: int, h: int, ch: int) -> np.ndarray:
    idx = np.arange(w * h * ch, dtype=np.uint64) + np.uint64(k) * np.uint64(w * h * ch)
    return (synth.splitmix64(idx) >> np.uint64(56)).astype(np.uint8).reshape((h, w, ch) if ch > 1 else (h, w))


def median_run(call, warmup: int, repeats: int) -> dict:
    for _ in range(warmup):
        call()
    runs = sorted(call() for _ in range(repeats))
    return dict(ms=1e3 * runs[len(runs) // 2], ms_min=1e3 * runs[0], ms_max=1e3 * runs[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pano-width", type=int, default=1024)
    ap.add_argument("--pano-height", type=int, default=512)
    ap.add_argument("--hypotheses", type=int, default=64)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--near", type=float, default=500.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_sweep_compose.json"))
    a = ap.parse_args()
    n, w, h, ch, pw, ph, D = 4, int(synth.IMG_W), int(synth.IMG_H), a.channels, a.pano_width, a.pano_height, a.hypotheses
    images = [hash_noise(k, w, h, ch) for k in range(n)]
    inv = sweep.inverse_distances(a.near, D=D)
    out = dict(metric="sweep_compose_kernel_ms_per_frame", unit="ms", n_gpus=1, higher_is_better=False, data="synthetic",
               config=dict(n_cameras=n, width=w, height=h, channels=ch, pano_width=pw, pano_height=ph, num_hypotheses=D, levels=a.levels, repeats=a.repeats,
                           hbm_rate_bytes_per_s=HBM_MEASURED_BS))
    with sweep.Sweeper.from_rig(synth.CALIB_INTR, synth.CALIB_TWC, (w, h), pw, ph, inv, device=a.device, keep_tables=True) as s:
        swept = s.depth([sweep.bgr_to_gray(x) for x in images])
        maps = dict(swept=swept, constant=np.full((ph, pw), 16 * (D // 2), np.int16))
        out["config"]["swept_valid_share"] = float(np.mean(swept >= 0))
        out["config"]["swept_distinct_hypotheses"] = int(np.unique((swept.astype(np.int32) + 8) >> 4).size)
        for mode in MODES:
            b = design_bytes(n, pw, ph, ch, mode, a.levels)
            res = dict(bytes=b, traffic_floor_ms=1e3 * b["total"] / HBM_MEASURED_BS)
            for name, idx in maps.items():
                res[name] = median_run(lambda: s.compose(images, idx, with_seconds=True, mode=mode, levels=a.levels)[1], a.warmup, a.repeats)
            out[mode] = res
        mx0, my0 = np.ascontiguousarray(s.mapx[:, 0]), np.ascontiguousarray(s.mapy[:, 0])
        weights = s.weights
    for mode in MODES:
        with panorama.Composer.from_tables(mx0, my0, (w, h), channels=ch, mode=mode, levels=a.levels, wrap_x=True, weights=weights, device=a.device) as c:
            res = median_run(lambda: c.compose(images, with_seconds=True)[1], a.warmup, a.repeats)
        b = design_bytes(n, pw, ph, ch, mode, a.levels, static=True)
        res.update(bytes=b, traffic_floor_ms=1e3 * b["total"] / HBM_MEASURED_BS)
        out[mode]["static"] = res
        out[mode]["ratio_to_static"] = {name: out[mode][name]["ms"] / res["ms"] for name in ("swept", "constant")}
    out["value"] = out["multiband"]["swept"]["ms"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
