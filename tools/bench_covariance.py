#!/usr/bin/env python3
"""Measurement of the covariance stage (tscm_covariance) on one MI355X.

Workloads: BASELINE configs 3, 4 and 5 (4 cameras x 500 and x 10,000 views, 8 cameras x 20,000 views) and a 32-camera rig, at
the generator's start parameters.  Prints ONE JSON line and writes it to profiles/bench_covariance.json: per workload the
device seconds of the four stages (HIP events around each stage's launches: board factor, Schur complement, reduced inverse,
board marginals; median of --repeats warm calls, min and max beside it), the wall time of the whole call (normal equations,
uploads and read-back included), and -- for orientation only -- the wall time of a float64 numpy restatement of the same
stages on the same blocks with its largest difference from the device result.  None of these is a pass/fail bound: the
stage has no earlier code path to compare with."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscm_calib_amd import api, synth  # noqa: E402

STAGES = ("board_factor", "schur", "reduced_inverse", "board_marginals")


def free_columns(p):
    """No held intrinsics: the rules of tscm.h on the problem."""
    cam_seen = np.zeros(p.n_cameras, bool); cam_seen[p.view_camera[p.view_count > 0]] = True
    board_seen = np.zeros(p.n_boards, bool); board_seen[p.view_board[p.view_count > 0]] = True
    cf = np.zeros((p.n_cameras, 15), bool)
    cf[:, 6:13] = cam_seen[:, None]
    cf[:, :6] = (cam_seen & ~p.cam_pose_constant.astype(bool) & (not p.mono))[:, None]
    return cf, board_seen


def numpy_covariance(p, ne):
    """The four stages in float64 numpy on the device's blocks (boards grouped by their number of views)."""
    C, B = p.n_cameras, p.n_boards
    cf, bf = free_columns(p)
    vc, vb = p.view_camera.astype(np.int64), p.view_board.astype(np.int64)
    Binv = np.zeros((B, 6, 6)); Binv[bf] = np.linalg.inv(ne["board_gram"][bf])
    W = ne["view_cross"] * cf[vc][:, None, :] * bf[vb][:, None, None]
    Z = Binv[vb] @ W
    order = np.argsort(vb, kind="stable")
    nv = np.bincount(vb, minlength=B)
    first = np.cumsum(nv) - nv
    S = np.zeros((C, 15, C, 15)); S[np.arange(C), :, np.arange(C), :] = ne["cam_gram"]
    groups = []
    for k in np.unique(nv[bf & (nv > 0)]):
        grp = order[first[bf & (nv == k)][:, None] + np.arange(k)]
        v1, v2 = np.repeat(grp, k, axis=1).ravel(), np.tile(grp, (1, k)).ravel()
        groups.append((v1, v2))
        np.add.at(S, (vc[v1], slice(None), vc[v2], slice(None)), -np.swapaxes(W[v1], 1, 2) @ Z[v2])
    fm = cf.ravel()
    Sf = S.reshape(C * 15, C * 15)[np.ix_(fm, fm)]
    d = 1.0 / np.sqrt(np.diagonal(Sf))
    cam = np.zeros((C * 15, C * 15)); cam[np.ix_(fm, fm)] = np.linalg.inv(Sf * d[:, None] * d[None, :]) * d[:, None] * d[None, :]
    cam = cam.reshape(C, 15, C, 15)
    board = Binv.copy()
    for v1, v2 in groups:
        np.add.at(board, vb[v1], Z[v1] @ cam[vc[v1], :, vc[v2], :] @ np.swapaxes(Z[v2], 1, 2))
    return cam, board * bf[:, None, None]


def spread(values):
    values = sorted(values)
    return dict(s=values[len(values) // 2], s_min=values[0], s_max=values[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--configs", type=int, nargs="*", default=[3, 4, 5])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_covariance.json"))
    a = ap.parse_args()
    work = [(f"config{k}", lambda k=k: synth.make_config(k)) for k in a.configs] + [("rig32", lambda: synth.make_problem(32, 6, 632))]
    rows = []
    for name, make in work:
        p = make()
        for _ in range(a.warmup):
            api.covariance(p, a.device)
        runs, wall = [], []
        for _ in range(a.repeats):
            t = time.perf_counter()
            runs.append(api.covariance(p, a.device))
            wall.append(time.perf_counter() - t)
        r = runs[-1]
        ne = api.normal_equations(p, a.device)
        t = time.perf_counter()
        cam, board = numpy_covariance(p, ne)
        t_numpy = time.perf_counter() - t
        dc = np.sqrt(np.abs(np.diagonal(cam.reshape(p.n_cameras * 15, -1))))
        scale = np.where(dc > 0, dc, 1.0)
        diff_cam = float(np.max(np.abs(r["cam_cov"].reshape(dc.size, dc.size) - cam.reshape(dc.size, dc.size)) / (scale[:, None] * scale[None, :])))
        db = np.sqrt(np.abs(np.diagonal(board, axis1=1, axis2=2)))
        sb = np.where(db > 0, db, 1.0)
        diff_board = float(np.max(np.abs(r["board_cov"] - board) / (sb[:, :, None] * sb[:, None, :])))
        rows.append(dict(workload=name, cameras=p.n_cameras, boards=p.n_boards, views=p.n_views, corners=p.n_corners, n_free=r["n_free"],
                         status=r["status"], min_pivot_ratio=r["min_pivot_ratio"], sigma2=r["sigma2"],
                         stages={s: spread([x["seconds_kernel"][i] for x in runs]) for i, s in enumerate(STAGES)},
                         kernels_total=spread([sum(x["seconds_kernel"]) for x in runs]), call_wall=spread(wall),
                         numpy_restatement=dict(s=t_numpy, max_diff_cam=diff_cam, max_diff_board=diff_board)))
    line = json.dumps(dict(tool="bench_covariance", repeats=a.repeats, rows=rows))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
