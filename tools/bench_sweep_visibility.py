#!/usr/bin/env python3
"""Measurement of the per-camera visibility at the swept depth (tscm_sweep_visibility, tscm_sweep_compose_visible) on one
MI355X.

Workload: that of tools/bench_sweep_compose.py -- the four cameras of the golden calibration (1280 x 1080, 3 channels of hashed
noise), a 1024 x 512 panorama, 64 inverse-distance hypotheses, the index map the depth pass gives for the frame.  Prints ONE
JSON line and writes it to profiles/bench_sweep_visibility.json: device milliseconds per frame (HIP events around the kernels,
median of --repeats warm calls), in one run on one device, of tscm_sweep_compose in the three modes -- the yardstick --, of
tscm_sweep_visibility alone and of tscm_sweep_compose_visible in the three modes, with the ratios to the yardstick, the bytes
the pass moves through device memory (counted from the shapes, below) with the time they take at the streaming rate of HBM, and
the share of the pixels in state 3 and state 4.  Nothing is asserted.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_sweep_compose import HBM_MEASURED_BS, MODES, hash_noise, median_run  # noqa: E402
from tools.bench_sweep_compose import design_bytes as compose_bytes  # noqa: E402
from tscm_calib_amd import sweep, synth  # noqa: E402


def design_bytes(n: int, w: int, h: int, pw: int, ph: int, cell_shift: int, dilate: int) -> dict:
    """Bytes the pass reads and writes in device memory.  The clear writes the n depth buffers (4 bytes per cell); the splat
    reads the index map and the n records of every pixel (8 bytes) and sends at most one 4-byte atomic per record; the test
    reads the same and writes n use bytes and one state byte per pixel.  The (2 dilate + 1)^2 cell reads of the test are
    gathers into a buffer of a few hundred kilobytes and are not counted, as the composer's image gathers are not.  The
    composer under visibility reads n use bytes per pixel more than the plain one."""
    px = pw * ph
    cells = n * (((w - 1) >> cell_shift) + 1) * (((h - 1) >> cell_shift) + 1)
    b = dict(clear=4 * cells, splat=2 * px + n * px * 8 + n * px * 4, test=2 * px + n * px * 8 + n * px + px, compose_extra=n * px)
    b["total"] = b["clear"] + b["splat"] + b["test"]
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pano-width", type=int, default=1024)
    ap.add_argument("--pano-height", type=int, default=512)
    ap.add_argument("--hypotheses", type=int, default=64)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--near", type=float, default=500.0)
    ap.add_argument("--cell-shift", type=int, default=2)
    ap.add_argument("--tolerance", type=int, default=2)
    ap.add_argument("--dilate", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_sweep_visibility.json"))
    a = ap.parse_args()
    n, w, h, ch, pw, ph, D = 4, int(synth.IMG_W), int(synth.IMG_H), a.channels, a.pano_width, a.pano_height, a.hypotheses
    vp = dict(cell_shift=a.cell_shift, tolerance=a.tolerance, dilate=a.dilate, near_is_high=1)
    images = [hash_noise(k, w, h, ch) for k in range(n)]
    inv = sweep.inverse_distances(a.near, D=D)
    b = design_bytes(n, w, h, pw, ph, a.cell_shift, a.dilate)
    out = dict(metric="sweep_visibility_kernel_ms_per_frame", unit="ms", n_gpus=1, higher_is_better=False, data="synthetic",
               config=dict(n_cameras=n, width=w, height=h, channels=ch, pano_width=pw, pano_height=ph, num_hypotheses=D, levels=a.levels, repeats=a.repeats,
                           hbm_rate_bytes_per_s=HBM_MEASURED_BS, **vp),
               design_bytes=b, traffic_floor_ms=1e3 * b["total"] / HBM_MEASURED_BS)
    with sweep.Sweeper.from_rig(synth.CALIB_INTR, synth.CALIB_TWC, (w, h), pw, ph, inv, device=a.device) as s:
        swept = s.depth([sweep.bgr_to_gray(x) for x in images])
        state = s.visibility(swept, with_state=True, **vp)[1]
        count = np.bincount(state.ravel(), minlength=5)
        out["config"]["swept_valid_share"] = float(np.mean(swept >= 0))
        out["state_share"] = {str(k): float(count[k]) / state.size for k in range(5)}
        out["state3_share"], out["state4_share"] = out["state_share"]["3"], out["state_share"]["4"]
        out["visibility"] = median_run(lambda: s.visibility(swept, with_seconds=True, **vp)[1], a.warmup, a.repeats)
        for mode in MODES:
            kw = dict(mode=mode, levels=a.levels)
            plain = median_run(lambda: s.compose(images, swept, with_seconds=True, **kw)[1], a.warmup, a.repeats)
            vis = median_run(lambda: s.compose(images, swept, with_seconds=True, visibility=vp, **kw)[1], a.warmup, a.repeats)
            out[mode] = dict(compose=plain, compose_visible=vis, ratio=vis["ms"] / plain["ms"], compose_bytes=compose_bytes(n, pw, ph, ch, mode, a.levels)["total"])
    out["value"] = out["visibility"]["ms"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
