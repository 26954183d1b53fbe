#!/usr/bin/env python3
"""Milliseconds per LM iteration with and without held intrinsics, one JSON line.

Configs 4 and 5 of BASELINE.json, fp64 tier, masks: none, Double Sphere (lambda held) and extrinsics only (all seven
intrinsics held); timed as tools/bench_robust.py times (resident solves of a fixed number of iterations, tolerances off).
Each mask is measured `--rounds` times in alternation and the median is reported.

    python tools/bench_fixed.py [--iters N] [--configs 4,5] [--rounds R]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tscm_calib_amd import api, lib, synth                   # noqa: E402

ITERS_PER_SOLVE = 10
OPTS = dict(function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0, min_trust_region_radius=0.0,
            check_every=ITERS_PER_SOLVE, max_num_iterations=ITERS_PER_SOLVE)
MASKS = {"none": None, "ds": lib.MODEL_DS, "extrinsics_only": lib.FIX_INTRINSICS}


def ms_per_iteration(solver, n_iter):
    solver.solve_resident(reset=True, **OPTS)          # warm-up
    t0 = time.perf_counter()
    for _ in range(n_iter // ITERS_PER_SOLVE):
        s = solver.solve_resident(reset=True, **OPTS)
        if s["lm_iterations"] != ITERS_PER_SOLVE:
            raise RuntimeError(f"expected {ITERS_PER_SOLVE} LM iterations, device ran {s['lm_iterations']} ({s['message']})")
    return 1e3 * (time.perf_counter() - t0) / ((n_iter // ITERS_PER_SOLVE) * ITERS_PER_SOLVE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--configs", default="4,5")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    res = {}
    for cfg in [int(c) for c in a.configs.split(",")]:
        p = synth.make_config(cfg).normalised()
        with api.Solver(p, 0) as s:
            s.upload_params()
            runs = {name: [] for name in MASKS}
            for _ in range(a.rounds):
                for name, mask in MASKS.items():
                    s.set_fixed_intrinsics(mask)
                    runs[name].append(ms_per_iteration(s, a.iters))
            s.set_fixed_intrinsics(None)
        for name, v in runs.items():
            res[f"config{cfg}_{name}"] = round(statistics.median(v), 4)
    line = {"metric": "ms_per_lm_iteration", "iters": a.iters, "rounds": a.rounds, "results": res}
    for key, v in res.items():
        base = res.get(key.split("_")[0] + "_none")
        if base and not key.endswith("_none"):
            line.setdefault("vs_none", {})[key] = round(v / base - 1.0, 4)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
