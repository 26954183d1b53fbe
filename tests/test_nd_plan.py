"""Host logic of the reduced camera system's solver (tscm_calib_amd/csrc/tscm_nd_plan.h): the elimination plan along the
camera-pair graph -- levels of non-adjacent cameras, panels, steps, the structurally non-zero tiles -- and the tile
algorithm k_solve_nd runs over it, emulated on the CPU by tests/native/nd_plan_check.cpp (same schedule, same masks, same
double buffering between the same barriers) against a dense Cholesky solve of the same system.  No GPU."""
import pytest

from tests import native_check as N


@pytest.fixture(scope="module")
def checker():
    return N.built("nd_plan_check.cpp", "nd_plan_check")


def run(exe, C, graph, const_mask=1, inactive=0, dense=0, seed=1):
    return N.run(exe, C, graph, const_mask, inactive, dense, seed)


CASES = [(C, g) for C in range(1, 9) for g in ("ring", "chain", "complete", "star")] + [
    (8, "pairs:0-1,1-2,2-3,3-0,4-5,5-6,6-7,7-4,0-4"), (8, "pairs:0-1,2-3"), (6, "pairs:0-1,1-2,2-0,3-4,4-5,5-3,0-3"), (7, "pairs:0-3,3-6,6-2,2-5,5-1,1-4")]


@pytest.mark.parametrize("C,graph", CASES)
def test_plan_solves_the_system(checker, C, graph):
    for dense in (0, 1):
        for seed in (1, 2):
            r = run(checker, C, graph, dense=dense, seed=seed)
            assert r["ok"], r
            assert r["covered"] == r["free_cols"]
            assert r["rel_err"] < 1e-12, r
            assert r["NP"] <= 32 and r["tiles"] <= 384 and r["lds_bytes"] <= 72 * 1024, r


def test_constant_and_inactive_cameras(checker):
    for const_mask, inactive in ((0, 0), (0b101, 0), (1, 0b100), (0b11, 0b1000), (0xff, 0)):
        for graph in ("ring", "chain", "complete"):
            r = run(checker, 6, graph, const_mask=const_mask, inactive=inactive)
            assert r["ok"] and r["rel_err"] < 1e-12, (const_mask, inactive, graph, r)


def test_ring_schedules(checker):
    """BASELINE configs 3-5 are rings (frame f is seen by cameras f and f + 1): 9 phases instead of 12 at
    four cameras, 13 instead of 25 at eight, the last level being the dense block of the two cameras that are left; the
    solver workgroup's LDS stays under a third of a CU's (three workgroups of the fused launch per CU)."""
    r4, r8 = run(checker, 4, "ring"), run(checker, 8, "ring")
    assert (r4["phases"], r4["levels"], r4["tpt"]) == (9, "1,3|0,2", 1)
    assert (r8["phases"], r8["levels"], r8["tpt"]) == (13, "1,3,5,7|2,6|0,4", 2)
    assert r8["lds_bytes"] <= 160 * 1024 // 3 - 2560 and r4["lds_bytes"] <= 32 * 1024
    d4, d8 = run(checker, 4, "ring", dense=1), run(checker, 8, "ring", dense=1)
    assert (d4["phases"], d8["phases"]) == (12, 25) and d4["dense"] and d8["dense"]
    assert run(checker, 4, "complete")["dense"]                       # a complete pair graph IS the dense block


def test_graph_plan_that_does_not_fit_falls_back_to_the_dense_plan(checker):
    """8 free cameras (no constant pose: `cam_pose_constant` NULL is legal API) on a dense but incomplete pair graph: the
    graph plan's per-camera panel padding exceeds the tile budget, the dense packing of the same system (377 tiles) does
    not -- tscm_solver_create must take the dense plan instead of refusing the rig (round-4 advisor finding).  Random
    connected 8-camera graphs: every one of them gets a plan that solves the system."""
    import itertools
    import random
    r = run(checker, 8, "pairs:" + ",".join(f"{a}-{b}" for a, b in itertools.combinations(range(8), 2) if (a, b) != (0, 1)), const_mask=0)
    assert r["ok"] and r["fell_back"] and r["dense"] and r["tiles"] <= 384 and r["rel_err"] < 1e-12, r
    rng = random.Random(5)
    fell = 0
    for _ in range(60):
        edges = {(i, rng.randrange(i)) for i in range(1, 8)}          # a random spanning tree ...
        edges |= {e for e in itertools.combinations(range(8), 2) if rng.random() < 0.6}      # ... plus a dense random graph
        g = "pairs:" + ",".join(f"{min(a, b)}-{max(a, b)}" for a, b in sorted(edges))
        r = run(checker, 8, g, const_mask=0)
        assert r["ok"] and r["rel_err"] < 1e-12 and r["tiles"] <= 384, (g, r)
        fell += bool(r["fell_back"])
    assert fell > 0          # the sample does contain graphs that need the fall-back
