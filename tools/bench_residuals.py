#!/usr/bin/env python3
"""Measurement of the residual report (tscm_residual_report) on one MI355X.

Workload: BASELINE config 4 (4 cameras x 10,000 views, 2.16 M corners) at the generator's start parameters, without a field
and with a 32 x 32 grid plus 32 angle bins.  Prints ONE JSON line and writes it to profiles/bench_residuals.json: per variant
the device seconds of the four launches (HIP events around each: views, cameras, field accumulation, field means; median of
--repeats warm calls, min and max beside it), the bytes the two large kernels move by construction -- k_residual_views reads
16 B of observations per corner (24 with weights) and writes 48 B of rows (52 with a field: the cell / bin word),
k_residual_field reads those 52 B -- as a fraction of --hbm-tbs (8 TB/s), and the wall time of the whole call (uploads and the
read-back of the 6 N doubles included).  For orientation the wall time of api.reprojection_error on the same problem, whose
kernel k_reproj_error reads the same inputs and writes nothing per corner; its device time is not visible from here and comes
from a kernel trace of this tool (tools/prof_tool.sh).  None of these is a pass/fail bound: nothing before did this work."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscm_calib_amd import api, synth  # noqa: E402

STAGES = ("views", "cameras", "field", "field_means")


def spread(values):
    values = sorted(values)
    return dict(s=values[len(values) // 2], s_min=values[0], s_max=values[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--config", type=int, default=4)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--no-cpu", action="store_true", help="accepted for tools/prof_tool.sh; there is no CPU part")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_residuals.json"))
    a = ap.parse_args()
    p = synth.make_config(a.config)
    N = p.n_corners
    size = (int(synth.IMG_W), int(synth.IMG_H))
    variants = [("plain", {}), ("grid32x32_bins32", dict(grid=(32, 32), image_size=size, angle_bins=32, max_angle=np.pi))]
    rows = []
    for name, kw in variants:
        stage, wall = {k: [] for k in STAGES}, []
        for i in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            r = api.residual_report(p, a.device, **kw)
            t1 = time.perf_counter()
            if i < a.warmup:
                continue
            wall.append(t1 - t0)
            for k, s in zip(STAGES, r["seconds_kernel"]):
                stage[k].append(s)
        field = bool(kw)
        views_bytes = N * (16 + 48 + (4 if field else 0))
        field_bytes = N * 52 if field else 0
        med = {k: spread(v) for k, v in stage.items()}
        row = dict(variant=name, corners=N, views=p.n_views, cameras=p.n_cameras, rmse=r["rmse"], stages=med,
                   kernels_total=spread([sum(x) for x in zip(*(stage[k] for k in STAGES))]), call_wall=spread(wall),
                   views_bytes=views_bytes, views_hbm_fraction=views_bytes / med["views"]["s"] / (a.hbm_tbs * 1e12))
        if field:
            row.update(field_bytes=field_bytes, field_hbm_fraction=field_bytes / med["field"]["s"] / (a.hbm_tbs * 1e12),
                       grid_outside=[int(x) for x in r["grid_outside"]], angle_outside=[int(x) for x in r["angle_outside"]],
                       n_clamped=int(r["grid_count"][..., 1].sum()))
        rows.append(row)
    wall = []
    for i in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        api.reprojection_error(p, a.device)
        if i >= a.warmup:
            wall.append(time.perf_counter() - t0)
    out = dict(tool="bench_residuals", config=a.config, repeats=a.repeats, hbm_tbs=a.hbm_tbs, rows=rows, reprojection_error_call_wall=spread(wall))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
