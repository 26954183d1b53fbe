#!/usr/bin/env python3
"""LM iterations per second with and without a robust loss, one JSON line.

Configs 4 and 5 of BASELINE.json, the fp64 (k_eval_gram4) and fp32-Jacobian (k_eval_gram_f32) tiers, no loss / Huber(1 px)
/ Cauchy(1 px); timed as bench.py times (resident solves of a fixed number of iterations, tolerances off).  With
--kernel-medians-from DIR the line also carries the median duration of the default and the robust k_eval_gram4 launches
of a `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_robust.py --profile-run` run.

--weights adds, for no loss and Huber, the same solves with corner weights (20 % of the corners masked, the rest uniform in
[0.25, 4]: the WEIGHTED instantiations), as <key>_weights, and their cost against the unweighted solve with the same loss.

    python tools/bench_robust.py [--iters N] [--configs 4,5] [--weights] [--kernel-medians-from DIR]"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tscm_calib_amd import api, synth                        # noqa: E402

ITERS_PER_SOLVE = 10
OPTS = dict(function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0, min_trust_region_radius=0.0,
            check_every=ITERS_PER_SOLVE, max_num_iterations=ITERS_PER_SOLVE)
LOSSES = {"none": None, "huber": "huber", "cauchy": "cauchy"}


def iterations_per_s(solver, n_iter, fp32):
    solver.solve_resident(reset=True, jacobian_fp32=fp32, **OPTS)          # warm-up
    t0 = time.perf_counter()
    for _ in range(n_iter // ITERS_PER_SOLVE):
        s = solver.solve_resident(reset=True, jacobian_fp32=fp32, **OPTS)
        if s["lm_iterations"] != ITERS_PER_SOLVE:
            raise RuntimeError(f"expected {ITERS_PER_SOLVE} LM iterations, device ran {s['lm_iterations']} ({s['message']})")
    return (n_iter // ITERS_PER_SOLVE) * ITERS_PER_SOLVE / (time.perf_counter() - t0)


def kernel_medians(d):
    """Median ns of the k_eval_gram4 launches of a kernel trace, default and robust instantiations apart (launches that
    exit early on ctrl->done, a few microseconds, are left out)."""
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[-1]
    dur = {"default": [], "robust": [], "weighted": []}
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        if "k_eval_gram4" not in name:
            continue
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if "k_eval_gram4_weighted" in name:
            dur["weighted"].append(ns)
            continue
        m = re.search(r"k_eval_gram4<\s*\d+\s*,\s*(?:true|false)\s*,\s*(true|false)\s*>", name)
        dur["robust" if m and m.group(1) == "true" else "default"].append(ns)
    out = {}
    for k, v in dur.items():
        big = [x for x in v if x > 0.5 * max(v)] if v else []
        out[k] = {"median_ns": int(statistics.median(big)) if big else None, "launches": len(big)}
    if out["default"]["median_ns"] and out["robust"]["median_ns"]:
        out["robust_over_default"] = round(out["robust"]["median_ns"] / out["default"]["median_ns"], 4)
    if out["robust"]["median_ns"] and out["weighted"]["median_ns"]:
        out["weighted_over_robust"] = round(out["weighted"]["median_ns"] / out["robust"]["median_ns"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--configs", default="4,5")
    ap.add_argument("--weights", action="store_true", help="also with corner weights, for no loss and Huber")
    ap.add_argument("--kernel-medians-from", metavar="DIR")
    ap.add_argument("--profile-run", action="store_true", help="config 4, fp64, none and Huber, 60 iterations each (under rocprofv3)")
    a = ap.parse_args()
    res = {}
    configs = [4] if a.profile_run else [int(c) for c in a.configs.split(",")]
    for cfg in configs:
        p = synth.make_config(cfg).normalised()
        with api.Solver(p, 0) as s:
            s.upload_params()
            for fp32 in ((0,) if a.profile_run else (0, 1)):
                for name, kind in LOSSES.items():
                    if a.profile_run and name == "cauchy":
                        continue
                    s.set_loss(kind, 1.0)
                    key = f"config{cfg}_{'fp32' if fp32 else 'fp64'}_{name}"
                    res[key] = round(iterations_per_s(s, 60 if a.profile_run else a.iters, fp32), 2)
                    if a.weights and name in ("none", "huber"):
                        rng = np.random.default_rng(cfg)
                        w = rng.uniform(0.25, 4.0, p.n_corners)
                        w[rng.random(p.n_corners) < 0.2] = 0.0
                        s.set_corner_weights(w)
                        res[key + "_weights"] = round(iterations_per_s(s, 60 if a.profile_run else a.iters, fp32), 2)
                        s.set_corner_weights(None)
            s.set_loss(None)
    line = {"metric": "lm_iterations_per_s", "iters": a.iters, "results": res}
    for cfg in configs:
        for tier in ("fp64", "fp32"):
            base = res.get(f"config{cfg}_{tier}_none")
            for name in ("huber", "cauchy"):
                v = res.get(f"config{cfg}_{tier}_{name}")
                if base and v:
                    line.setdefault("cost_vs_none", {})[f"config{cfg}_{tier}_{name}"] = round(base / v - 1.0, 4)
    for key, v in list(res.items()):
        if key.endswith("_weights") and res.get(key[:-len("_weights")]):
            line.setdefault("weights_cost_vs_unweighted", {})[key] = round(res[key[:-len("_weights")]] / v - 1.0, 4)
    if a.kernel_medians_from:
        line["k_eval_gram4"] = kernel_medians(a.kernel_medians_from)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
