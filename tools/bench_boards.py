#!/usr/bin/env python3
"""Measurement of the chessboard structure recovery on one MI355X and its host: the sequential host function
(tscm_chessboards_from_corners, one call per image) against the batched definition (tscm_chessboards_from_corners_batch) on the
host and on the device (k_board_seeds), at batch 1 and batch 32.

Workload: 32 rendered 1280 x 1080 images of a 9 x 6 board (synth.render_chessboard, distinct poses), half of them with 10-40
added clutter blobs (small 2 x 2 checker patches away from the board, each an X-junction the detector keeps), and the
candidates tscm_detect_corners_batch finds in them.  Every path is timed at the C ABI (ctypes calls on prepared arrays, the
result freed inside the timed window, no numpy conversion), --warmup calls first, then --repeats rounds that run the paths one
after the other, so that each round's figures share the machine's state; the median per path is reported, minimum and
maximum beside it.  Wall times are host clocks around calls that return after the copy back and the overlap resolution;
kernel times are the HIP events around k_board_seeds (tscm_chessboards_batch_seconds).  Prints ONE JSON line and writes it to
profiles/bench_boards.json: per path the milliseconds per image, ratio = sequential host function / device call at batch 32
(wall, per image; above 1 the device call is faster), the share of seeds per status and the mean number of growth steps of
the grown seeds (the load-imbalance picture), and whether all paths gave the same boards.  Not measured: hardware counters,
achieved occupancy, the spread of a workgroup's run time."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tscm_calib_amd import corners, lib, synth  # noqa: E402

N_IMAGES = 32


def images(seed=5):
    """The 32 images and the number of blobs added to each."""
    p = synth.make_problem(1, N_IMAGES, seed, noise_px=0.0, perturb=False)
    rng = np.random.default_rng(seed)
    out, blobs = [], []
    for v in range(N_IMAGES):
        img = synth.render_chessboard(p.meta["gt_intr"][0], p.meta["gt_board_rt"][v], 9, 6, 45.0, 1280, 1080, supersample=2)
        o = p.view_offset[v]
        u, w = p.obs_u[o:o + 54], p.obs_v[o:o + 54]
        box = (u.min() - 90, u.max() + 90, w.min() - 90, w.max() + 90)
        n_blobs = int(rng.integers(10, 41)) if v % 2 else 0
        placed = 0
        for _ in range(50 * n_blobs):
            if placed == n_blobs:
                break
            s = int(rng.integers(10, 19))                                           # side of one square of the patch
            x, y = int(rng.integers(4, 1280 - 2 * s - 4)), int(rng.integers(4, 1080 - 2 * s - 4))
            if box[0] < x + s < box[1] and box[2] < y + s < box[3]:
                continue
            img[y:y + s, x:x + s] = img[y + s:y + 2 * s, x + s:x + 2 * s] = 25
            img[y:y + s, x + s:x + 2 * s] = img[y + s:y + 2 * s, x:x + s] = 230
            placed += 1
        out.append(img)
        blobs.append(placed)
    return out, blobs


def spread(values, per):
    values = sorted(values)
    return dict(ms_per_image=1e3 * values[len(values) // 2] / per, ms_min=1e3 * values[0] / per, ms_max=1e3 * values[-1] / per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_boards.json"))
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("--repeats: the median of at least 7")
    L = lib.lib()
    assert L.tscm_device_count() > 0, "no HIP device: this is a measurement on the GPU"
    imgs, blobs = images()
    cands = corners.detect_corners_batch(imgs, device=a.device)
    keep, recs = corners._candidate_records(cands)
    one = [corners._candidate_records([c]) for c in cands]
    f_old, f_new, f_free, f_sec = L.tscm_chessboards_from_corners, L.tscm_chessboards_from_corners_batch, L.tscm_chessboards_free, L.tscm_chessboards_batch_seconds
    f_old.restype = f_new.restype = C.c_int
    f_old.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_void_p]
    f_new.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    f_free.restype, f_free.argtypes = None, [C.c_void_p]
    f_sec.restype, f_sec.argtypes = C.c_double, []
    outs = (lib.CChessboards * N_IMAGES)()

    def sequential():
        t = time.perf_counter()
        for k, arrs in enumerate(keep):
            lib.check(f_old(arrs[0].shape[0], arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, arrs[3].ctypes.data, C.byref(outs[k])))
            f_free(C.byref(outs[k]))
        return time.perf_counter() - t, 0.0

    def batch(where):
        def run():
            t = time.perf_counter()
            lib.check(f_new(N_IMAGES, recs, where, a.device, outs))
            kernel = f_sec()
            for k in range(N_IMAGES):
                f_free(C.byref(outs[k]))
            return time.perf_counter() - t, kernel
        return run

    def device_one_by_one():
        t, kernel = time.perf_counter(), 0.0
        for k in range(N_IMAGES):
            lib.check(f_new(1, one[k][1], lib.BOARDS_DEVICE, a.device, outs))
            kernel += f_sec()
            f_free(C.byref(outs[0]))
        return time.perf_counter() - t, kernel

    paths = dict(host_sequential=sequential, host_batch=batch(lib.BOARDS_HOST), device_batch_1=device_one_by_one, device_batch_32=batch(lib.BOARDS_DEVICE))
    wall, kernel = {k: [] for k in paths}, {k: [] for k in paths}
    for r in range(a.warmup + a.repeats):
        for name, fn in paths.items():                                              # the paths alternate inside every round
            w, kt = fn()
            if r >= a.warmup:
                wall[name].append(w)
                kernel[name].append(kt)
    # what was computed: the same boards on every path, and the jobs' statuses
    old = [corners.chessboards_from_corners(c["x"], c["y"], c["v1"], c["v2"]) for c in cands]
    same = True
    for where in ("host", "device"):
        new = corners.chessboards_from_corners_batch(cands, where=where, device=a.device)
        same = same and all(len(u) == len(v) and all(np.array_equal(p, q) for p, q in zip(u, v)) for u, v in zip(old, new))
    st = corners.chessboards_batch_stages(cands, where="device", device=a.device)
    status = np.concatenate([s["status"] for s in st])
    steps = np.concatenate([s["steps"] for s in st])
    n = np.array([c["n"] for c in cands])
    res = dict(tool="bench_boards", images=N_IMAGES, image=[1280, 1080], board=[9, 6], images_with_blobs=int(np.sum(np.array(blobs) > 0)),
               candidates=dict(min=int(n.min()), median=float(np.median(n)), max=int(n.max()), total=int(n.sum())), repeats=a.repeats, warmup=a.warmup,
               accepted=int(sum(len(b) == 1 and b[0].shape == (6, 9) for b in old)), same_boards_on_every_path=bool(same))
    for name in paths:
        res[name] = dict(wall=spread(wall[name], N_IMAGES))
        if name.startswith("device"):
            res[name]["kernel"] = spread(kernel[name], N_IMAGES)
    res["ratio_host_sequential_over_device_batch_32"] = res["host_sequential"]["wall"]["ms_per_image"] / res["device_batch_32"]["wall"]["ms_per_image"]
    res["ratio_host_sequential_over_host_batch"] = res["host_sequential"]["wall"]["ms_per_image"] / res["host_batch"]["wall"]["ms_per_image"]
    res["seeds"] = dict(total=int(status.shape[0]), share_by_status=[float(np.mean(status == s)) for s in range(4)],
                        mean_steps_of_grown=float(steps[status >= 2].mean()) if np.any(status >= 2) else 0.0,
                        max_steps=int(steps.max()) if steps.size else 0)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
