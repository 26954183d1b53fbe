#!/usr/bin/env python3
"""bench_priors.py -- the price of camera priors at BASELINE config 4: forced LM iterations of one solver with and
without priors, alternating, device time per iteration -> one JSON line (profiles/bench_priors.json).  Needs the MI355X."""
import json, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tscm_calib_amd import api, lib, synth

OPTS = dict(function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0, min_trust_region_radius=0.0, check_every=50)
p = synth.make_config(4).normalised()
pr = api.camera_priors(p, intr_sigma={"xi": 0.05, "lambda": 0.05, "alpha": 0.05}, cam_rt_sigma=[0.01, 0.01, 0.01, 5.0, 5.0, 5.0])
res = {}
with api.Solver(p, 0) as s:
    s.upload_params()
    # default launches: the plain solve's reductions ride in k_schur_gram (priors: k_reduce_stats_prior, one launch more);
    # TSCM_EXEC_SEPARATE_CONTROL: the plain solve runs k_reduce_control (priors: k_reduce_stats_prior, k_finalize_eval, k_control,
    # two launches more) -- the route of boards seen by more than three cameras and of more than one view class
    for shape, flags in (("default", 0), ("separate_control", lib.EXEC_SEPARATE_CONTROL)):
        out = {"plain": [], "priors": []}
        for rep in range(5):
            for name, q in (("plain", None), ("priors", pr)):
                s.set_camera_priors(q)
                for _ in range(2 if rep == 0 else 1):       # (the first pair warms up)
                    r = s.solve_resident(reset=True, max_num_iterations=50, exec_flags=flags, **OPTS)
                assert r["lm_iterations"] == 50, r["message"]
                out[name].append(1e6 * r["seconds_solve"] / 50)
        res[shape] = {k: dict(us_per_iteration=[round(x, 3) for x in v[1:]], median=round(float(np.median(v[1:])), 3)) for k, v in out.items()}
        res[shape]["extra_us_per_iteration"] = round(res[shape]["priors"]["median"] - res[shape]["plain"]["median"], 3)
res["workload"] = "BASELINE config 4, 50 forced LM iterations per solve, device time first to last kernel, 4 alternating pairs after a warm-up pair"
print(json.dumps(res))
