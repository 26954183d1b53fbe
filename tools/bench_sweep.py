#!/usr/bin/env python3
"""Measurement of the sphere sweep (tscm_sweep_depth) on one MI355X.

Workload: the four cameras of the golden calibration (1280 x 1080, hashed noise), a 1024 x 512 panorama, 64 inverse-distance
hypotheses, with 4 and with 8 paths.  Prints ONE JSON line: device milliseconds per frame (HIP events around the kernels,
median of --repeats warm calls), each stage's share of it, the bytes the design moves through device memory (counted from
the shapes, below), the fraction of the streaming rate of HBM that this traffic over the measured time amounts to, and the
ratio to the numpy restatement (tests/sweep_ref.py) at a size the restatement finishes in seconds.  Nothing is asserted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscm_calib_amd import sweep, synth  # noqa: E402

HBM_MEASURED_BS = 6.29e12        # float4 copy on the MI355X (8.0e12 by specification)
HBM_SPEC_BS = 8.0e12
HALO = (64 + 8) * (16 + 6) / (64 * 16)      # k_sweep_cost reads a 72 x 22 halo of records per 64 x 16 tile: 1584 / 1024


def design_bytes(n: int, pw: int, ph: int, D: int, paths: int) -> dict:
    """Bytes each stage reads and writes in device memory: packed records uint2 [n][D][ph][pw] (read with the tile's halo),
    C uint8 [ph][pw][D], S uint16 [ph][pw][D], index int16.  The source images (n small planes that stay in the caches) are
    not counted.  Aggregation and winner as tools/bench_stereo.py counts them, the winner with its read of C(k*)."""
    px, vol = pw * ph, pw * ph * D
    b = dict(cost=int(n * D * px * 8 * HALO) + vol,
             aggregate=paths * vol + 2 * vol + (paths - 1) * 4 * vol,
             winner=2 * vol + px + 2 * px)
    b["total"] = sum(b.values())
    return b


def hash_noise(k: int, w: int, h: int) -> np.ndarray:
    idx = np.arange(w * h, dtype=np.uint64) + np.uint64(k) * np.uint64(w * h)
    return (synth.splitmix64(idx) >> np.uint64(56)).astype(np.uint8).reshape(h, w)


def restatement_ratio(device: int) -> dict:
    """The same frame through the device and through tests/sweep_ref.py at 160 x 80, D = 16, a quarter of the resolution."""
    from tests import sweep_ref
    intr = synth.CALIB_INTR.copy()
    intr[:, :4] *= 0.25
    w, h, pw, ph, D = 320, 270, 160, 80, 16
    images = [hash_noise(k, w, h) for k in range(4)]
    inv = sweep.inverse_distances(800.0, D=D)
    with sweep.Sweeper.from_rig(intr, synth.CALIB_TWC, (w, h), pw, ph, inv, device=device, keep_tables=True) as s:
        s.depth(images)
        idx, sec = s.depth(images, with_seconds=True)
        t0 = time.perf_counter()
        ref = sweep_ref.stages(images, None, s.mapx, s.mapy)["index16"]
        host = time.perf_counter() - t0
    return dict(pano=[pw, ph], D=D, device_ms=1e3 * sec, numpy_ms=1e3 * host, ratio=host / sec, equal=bool(np.array_equal(idx, ref)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pano-width", type=int, default=1024)
    ap.add_argument("--pano-height", type=int, default=512)
    ap.add_argument("--hypotheses", type=int, default=64)
    ap.add_argument("--near", type=float, default=500.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-restatement", action="store_true")
    a = ap.parse_args()
    n, w, h = 4, int(synth.IMG_W), int(synth.IMG_H)
    images = [hash_noise(k, w, h) for k in range(n)]
    inv = sweep.inverse_distances(a.near, D=a.hypotheses)
    out = dict(metric="sweep_depth_kernel_ms_per_frame", unit="ms", n_gpus=1, higher_is_better=False, data="synthetic",
               config=dict(n_cameras=n, width=w, height=h, pano_width=a.pano_width, pano_height=a.pano_height, num_hypotheses=a.hypotheses,
                           repeats=a.repeats, hbm_rate_bytes_per_s=HBM_MEASURED_BS, hbm_spec_bytes_per_s=HBM_SPEC_BS,
                           handle_bytes=n * a.hypotheses * a.pano_width * a.pano_height * 8))
    names = ("cost", "aggregate", "winner")
    for paths in (4, 8):
        with sweep.Sweeper.from_rig(synth.CALIB_INTR, synth.CALIB_TWC, (w, h), a.pano_width, a.pano_height, inv, device=a.device, paths=paths) as s:
            for _ in range(a.warmup):
                s.depth(images)
            runs = []
            for _ in range(a.repeats):
                idx, sec = s.depth(images, with_seconds=True)
                runs.append((sec, dict(zip(names, s.stage_times()))))
        runs.sort(key=lambda r: r[0])
        sec, stages = runs[len(runs) // 2]
        b = design_bytes(n, a.pano_width, a.pano_height, a.hypotheses, paths)
        out[f"paths_{paths}"] = dict(
            ms=1e3 * sec, ms_min=1e3 * runs[0][0], ms_max=1e3 * runs[-1][0],
            stage_ms={k: 1e3 * v for k, v in stages.items()}, stage_share={k: v / sec for k, v in stages.items()},
            bytes=b, traffic_floor_ms=1e3 * b["total"] / HBM_MEASURED_BS, achieved_bytes_per_s=b["total"] / sec,
            frac_of_hbm_rate=b["total"] / sec / HBM_MEASURED_BS, cost_frac_of_hbm_rate=b["cost"] / stages["cost"] / HBM_MEASURED_BS,
            valid_share=float(np.mean(idx != sweep.INVALID)))
    if not a.no_restatement:
        out["restatement"] = restatement_ratio(a.device)
    out["value"] = out["paths_8"]["ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
