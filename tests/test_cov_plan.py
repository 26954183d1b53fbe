"""Host plan of the covariance stage (tscm_calib_amd/csrc/tscm_cov_plan.h: cov_masks, plan_covariance), run by
tests/native/cov_plan_check.cpp and compared here with a Python statement of the same rules: the free columns (and
helpers.step_columns where no intrinsic is held), the compact numbering with holes, the views of the free boards, the
camera-pair tiles with their (view, view') lists and chunks.  Built twice: plain, and under AddressSanitizer + UBSan.  No GPU."""
import numpy as np
import pytest

from tests import cov_ref as CR
from tests import helpers as H
from tests import native_check as N
from tscm_calib_amd import lib, synth

pytestmark = N.NEEDS_GXX
checker = N.checker_fixture("cov_plan_check.cpp", "cov_plan_check")
CHUNK = 64


def _zero_corner_views():
    """mixed visibility with views that have no corners: camera 3 only has such views, board 2 too."""
    p = H.mixed_visibility_rig(n_frames=13)
    cnt = p.view_count.copy()
    cnt[(p.view_camera == 3) | (p.view_board == 2)] = 0
    off = (np.cumsum(cnt) - cnt).astype(np.int32)
    keep = np.concatenate([np.arange(o, o + c) for o, c in zip(p.view_offset, cnt)]).astype(np.int64)
    return CR._with(p, view_count=cnt, view_offset=off, obs_u=p.obs_u[keep], obs_v=p.obs_v[keep])


PROBLEMS = {
    "rig4": lambda: H.small_rig(4, 12),
    "rig4_two_chunks": lambda: synth.make_problem(4, 80, 3),          # 80 boards per camera: diagonal tiles of two chunks
    "mixed65": lambda: H.mixed_visibility_rig(n_frames=65),
    "ring8": lambda: synth.make_problem(8, 6, 23),
    "idle_camera": CR._camera_without_views,
    "unseen_boards": lambda: H.rig_with_unseen_boards(H.mixed_visibility_rig(n_frames=13), 3),
    "const_boards": CR._const_boards,
    "mono": lambda: synth.make_problem(1, 7, 20241),
    "zero_corner_views": _zero_corner_views,
}
MASKS = {
    "none": lambda C: None,
    "cx_cy": lambda C: ("cx", "cy"),
    "ds_on_1": lambda C: np.array([lib.MODEL_DS if m == min(1, C - 1) else 0 for m in range(C)]),
    "all7_on_last": lambda C: np.array([lib.FIX_INTRINSICS if m == C - 1 else 0 for m in range(C)]),
    "b_c_too": lambda C: np.full(C, lib.FIX["b"] | lib.FIX["c"] | lib.FIX["alpha"]),
}


def _expected(p, fixed):
    """The plan by the rules of tscm.h / DESIGN 25, stated in Python."""
    cam_free, board_free = CR.free_columns(p, fixed)
    C, V = p.n_cameras, p.n_views
    wide_of = [i for i in range(C * 15) if cam_free.ravel()[i]]
    compact_of = [-1] * (C * 15)
    for k, i in enumerate(wide_of):
        compact_of[i] = k
    free_boards = [i for i in range(p.n_boards) if board_free[i]]
    views = {i: [v for v in range(V) if p.view_board[v] == i] for i in free_boards}
    board_start, board_views, view_slot = [0], [], []
    for s, i in enumerate(free_boards):
        board_views += views[i]
        view_slot += [s] * len(views[i])
        board_start.append(len(board_views))
    tiles = {}
    for i in free_boards:
        for v in views[i]:
            for w in views[i]:
                a, b = int(p.view_camera[v]), int(p.view_camera[w])
                if a <= b:
                    tiles.setdefault((a, b), []).append((v, w))
    keys = sorted(tiles)
    tile_of = [-1] * (C * C)
    tile_start, pair_v, pair_w, tile_chunk, chunk_begin, chunk_end = [0], [], [], [0], [], []
    for t, (a, b) in enumerate(keys):
        tile_of[a * C + b] = t
        for k in range(0, len(tiles[a, b]), CHUNK):
            chunk_begin.append(len(pair_v) + k)
            chunk_end.append(len(pair_v) + min(k + CHUNK, len(tiles[a, b])))
        pair_v += [v for v, _ in tiles[a, b]]
        pair_w += [w for _, w in tiles[a, b]]
        tile_start.append(len(pair_v))
        tile_chunk.append(len(chunk_begin))
    return dict(rc=0, n_cam_free=len(wide_of), n_free=len(wide_of) + 6 * len(free_boards), cam_free=cam_free.ravel().astype(int).tolist(),
                board_free=board_free.astype(int).tolist(), compact_of=compact_of, wide_of=wide_of, free_boards=free_boards,
                board_start=board_start, board_views=board_views, view_slot=view_slot, tile_a=[a for a, _ in keys], tile_b=[b for _, b in keys],
                tile_of=tile_of, tile_start=tile_start, pair_v=pair_v, pair_w=pair_w, tile_chunk=tile_chunk, chunk_begin=chunk_begin,
                chunk_end=chunk_end)


def _describe(p, fixed):
    words = None if fixed is None else lib.fixed_masks(fixed, p.n_cameras)
    bc = p.board_pose_constant
    out = [p.n_cameras, p.n_boards, p.n_views, int(p.mono), 1, int(bc is not None), int(words is not None)]
    for v in range(p.n_views):
        out += [p.view_camera[v], p.view_board[v], p.view_count[v]]
    out += list(p.cam_pose_constant) + ([] if bc is None else list(bc)) + ([] if words is None else list(words))
    return " ".join(str(int(x)) for x in out)


def test_header_is_plain_cpp17():
    N.assert_plain_cpp17("tscm_cov_plan.h")


def test_plans_follow_the_rules(checker):
    jobs = [(name, mask, make(), ) for name, make in PROBLEMS.items() for mask in MASKS]
    jobs = [(name, mask, p, MASKS[mask](p.n_cameras)) for name, mask, p in jobs]
    text = f"{len(jobs)}\n" + "\n".join(_describe(p, fixed) for _, _, p, fixed in jobs) + "\n"
    got = N.run(checker, "plan", stdin=text)
    assert len(got) == len(jobs)
    seen = dict(holes=0, two_chunks=0, idle=0, unfree_boards=0, absent_tiles=0, no_pose=0)
    for (name, mask, p, fixed), g in zip(jobs, got):
        want = _expected(p, fixed)
        for key, val in want.items():
            assert g[key] == val, (name, mask, key)
        cf = np.array(g["cam_free"]).reshape(-1, 15)
        if fixed is None:                                   # no held intrinsic: the oracle's columns (helpers.step_columns)
            cols = H.step_columns(p)
            assert np.array_equal(cf[:, :13].astype(bool), cols["cam_free"]) and np.array_equal(np.array(g["board_free"], bool), cols["board_free"]), name
        assert not cf[:, 13:].any()
        seen["holes"] += any(np.any(np.diff(np.nonzero(r)[0]) > 1) for r in cf)
        seen["two_chunks"] += any(b - a > 1 for a, b in zip(g["tile_chunk"], g["tile_chunk"][1:]))
        seen["idle"] += any(not r.any() for r in cf)
        seen["unfree_boards"] += len(g["free_boards"]) < p.n_boards
        seen["absent_tiles"] += len(g["tile_a"]) < p.n_cameras * (p.n_cameras + 1) // 2
        seen["no_pose"] += bool(p.mono)
        # every chunk is a non-empty range of one tile of at most 64 pairs, and the chunks of a tile tile its list
        for t in range(len(g["tile_a"])):
            cs = range(g["tile_chunk"][t], g["tile_chunk"][t + 1])
            assert g["chunk_begin"][cs[0]] == g["tile_start"][t] and g["chunk_end"][cs[-1]] == g["tile_start"][t + 1]
            assert all(0 < g["chunk_end"][c] - g["chunk_begin"][c] <= CHUNK for c in cs)
            assert all(g["chunk_end"][c] == g["chunk_begin"][c + 1] for c in cs[:-1])
    assert all(seen.values()), seen


def test_refusals(checker):
    r = N.run(checker, "refuse")
    assert r["ok"], r
