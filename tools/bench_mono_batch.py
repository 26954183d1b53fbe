#!/usr/bin/env python3
"""Batched mono refinement against sequential solo solves: K reference-shaped problems (185 views of an 11x8
board, each with its own start intrinsics and noise) solved by K sequential tscm_solve_mono calls and by one
tscm_solve_mono_batch call.  Prints one JSON line: per K the wall and device time of both (minima over the repetitions),
the LM iterations (the batch runs as many as its longest problem) and the microseconds per batched iteration: the batch's
device time less that of the same batch with no LM iteration (its start and end), over its iterations.

    python tools/bench_mono_batch.py [--ks 1,4,8,32,128] [--reps 3]      (GPU box)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tscm_calib_amd import api, synth                        # noqa: E402


def problems(k):
    return [synth.make_problem(1, 185, 7000 + i, noise_px=0.1 + 0.05 * (i % 5), cols=11, rows=8) for i in range(k)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,4,8,32,128")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ks = [int(x) for x in a.ks.split(",")]
    pool = problems(max(ks))
    api.refinement_batch([pool[0].copy().normalised()])          # code objects loaded before anything is timed
    api.refinement(pool[0].copy().normalised())
    rows = []
    for k in ks:
        ps = pool[:k]
        seq, seq_dev, bat, dev, fixed = [], [], [], [], []
        for _ in range(a.reps):
            qs = [p.copy().normalised() for p in ps]
            t0 = time.perf_counter()
            solo = [api.refinement(q)[1] for q in qs]
            seq.append(time.perf_counter() - t0)
            seq_dev.append(sum(s["seconds_solve"] for s in solo))
            qs = [p.copy().normalised() for p in ps]
            t0 = time.perf_counter()
            out = api.refinement_batch(qs)
            bat.append(time.perf_counter() - t0)
            dev.append(out[0][1]["seconds_solve"])
            # the same batch without an LM iteration: the start (control blocks, initial evaluation and control step) and
            # the end (k_mb_finish), subtracted before the per-iteration figure
            fixed.append(api.refinement_batch([p.copy().normalised() for p in ps], max_num_iterations=0)[0][1]["seconds_solve"])
        its = max(s["lm_iterations"] for _, s in out)
        rows.append(dict(K=k, sequential_wall_ms=1e3 * min(seq), batch_wall_ms=1e3 * min(bat), sequential_device_ms=1e3 * min(seq_dev),
                         batch_device_ms=1e3 * min(dev), batch_start_end_device_ms=1e3 * min(fixed),
                         lm_iterations_sum=int(sum(s["lm_iterations"] for s in solo)), batch_iterations=int(its),
                         us_per_batch_iteration=1e6 * (min(dev) - min(fixed)) / max(1, its)))
    print(json.dumps(dict(bench="mono_batch", shape="185 views x 11x8", rows=rows)))


if __name__ == "__main__":
    main()
