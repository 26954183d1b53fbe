#!/usr/bin/env python3
"""Measurement of the next-best-view stage (tscm_view_gain) on one MI355X.

Workload: a 4-camera rig at 1280 x 1080 with the covariance of api.covariance at the generator's parameters; the candidate
set is api.view_candidates of every camera alone and with the next camera, on a --grid pixel grid, --distances, five tilts
and --rolls rolls (order 10^4 - 10^5 candidates), scored for a 9 x 6 (54 corners: one pass of 64 lanes) and an 11 x 8 board
(88 corners: two passes).  Prints ONE JSON line and writes it to profiles/bench_view_gain.json: per board the number of
candidates of each kind, device milliseconds of the launches (HIP events around them, median of --repeats warm calls, min
and max beside it), candidates per second, the wall time of the whole call, the share of candidates with a contributing
camera, and the comparison with the float64 numpy restatement (tests/view_gain_ref.py) on the CPU on every --numpy-every-th
candidate: its wall time scaled to candidates per second, and the largest difference of the gains in the reference's
measure.  None of these is a pass/fail bound: the stage has no earlier code path to compare with.  Not measured: hardware
counters, achieved occupancy, LDS bank conflicts."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscm_calib_amd import api, pipeline, synth  # noqa: E402


def spread(values):
    values = sorted(values)
    return dict(ms=1e3 * values[len(values) // 2], ms_min=1e3 * values[0], ms_max=1e3 * values[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--grid", default="24,16")
    ap.add_argument("--distances", default="300,500,800")
    ap.add_argument("--rolls", default="0,30")
    ap.add_argument("--numpy-every", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_view_gain.json"))
    a = ap.parse_args()
    from tests import view_gain_ref as V

    p = synth.make_problem(4, 30, 99, noise_px=0.1)
    size = (int(synth.IMG_W), int(synth.IMG_H))
    cov = api.covariance(p, a.device)
    assert cov["status"] == 0
    grid = tuple(int(x) for x in a.grid.split(","))
    distances = tuple(float(x) for x in a.distances.split(","))
    rolls = tuple(float(x) for x in a.rolls.split(","))
    result = dict(tool="bench_view_gain", cameras=p.n_cameras, image=size, grid=grid, distances=distances, rolls=rolls, boards={})
    for cols, rows in ((9, 6), (11, 8)):
        xy = pipeline.board_points(cols, rows, 45.0)[:, :2]
        cands = []
        for m in range(p.n_cameras):
            for b in (None, (m + 1) % p.n_cameras):
                cands += api.view_candidates(p.cam_rt, p.intr, m, size, xy, grid, distances, (0.0, 25.0, -25.0), rolls, pair=b)[0]
        args = (p.cam_rt, p.intr, cov, xy, size, cands)
        for _ in range(a.warmup):
            api.view_gain(*args, device=a.device)
        kernel, wall = [], []
        for _ in range(a.repeats):
            t = time.perf_counter()
            got = api.view_gain(*args, device=a.device)
            wall.append(time.perf_counter() - t)
            kernel.append(got["seconds_kernel"])
        again = api.view_gain(*args, device=a.device)
        same = all(got[k].tobytes() == again[k].tobytes() for k in ("gain_logdet", "gain_trace", "n_visible", "flags"))
        sub = list(range(0, len(cands), max(a.numpy_every, 1)))
        t = time.perf_counter()
        r64 = V.view_gain_ref(p.cam_rt, p.intr, cov["cam_cov"], xy, np.tile(np.array([size], np.int32), (p.n_cameras, 1)), [cands[i] for i in sub], dtype=np.float64)
        numpy_s = time.perf_counter() - t
        dev = {k: got[k][sub] for k in ("gain_logdet", "gain_trace", "n_visible", "flags")}
        diff = V.gain_errors(dev, dict(r64, near=np.zeros(len(sub), bool)))
        k = spread(kernel)
        pair = np.array([c[0] != c[1] for c in cands])
        result["boards"][f"{cols}x{rows}"] = dict(
            corners=cols * rows, candidates=len(cands), one_camera=int((~pair).sum()), pairs=int(pair.sum()), kernel=k,
            candidates_per_second=len(cands) / (1e-3 * k["ms"]), wall=spread(wall), contributing=float(((got["flags"] & 3) != 0).mean()),
            both_contribute=float(((got["flags"] & 3) == 3).mean()), pivot_failures=int(((got["flags"] & 8) != 0).sum()), same_bytes_twice=bool(same),
            best=dict(index=int(np.argmax(got["gain_logdet"])), gain_logdet=float(np.max(got["gain_logdet"]))),
            numpy_float64=dict(candidates=len(sub), seconds=numpy_s, candidates_per_second=len(sub) / numpy_s, flags_equal=bool(np.array_equal(dev["flags"], r64["flags"])),
                               counts_equal=bool(np.array_equal(dev["n_visible"], r64["n_visible"])), difference=diff))
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
