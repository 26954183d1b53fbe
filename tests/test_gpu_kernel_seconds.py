"""GPU tests of the device seconds that the perception entry points report.  They come from one pair (or chain) of events
around the launches of a call, so: the total of the matcher and of the sweep is the sum of their stage times, the same
doubles added in the same order; every value is above zero and below the wall time of the call that contains it; and an
entry point or a handle that is used again reports the time of that call, not a running sum.

Fresh or accumulated is decided between the calls (_fresh_values): CALLS = 21 warm calls of the same work.  Fresh values
scatter around one kernel time m, so the median of the last three is about the median of the first three; of a running
sum they are 20 m and 2 m, a ratio of 10.  The bound 3 leaves a factor of 3 for noise (a median of three also forgives one
outlier each side) and 10 / 3 on the other.  The law is tried on the running sum of the measured values too and must fail
there.  It needs warm kernels: the first launch of a kernel loads its code between the events, a time that in a running
sum would drown the later terms, so a handle of the same kind (for the one-shot entry points: the same call) runs WARM = 3
times first.

Shapes are the smallest of the stages' own tests: a map of 130 x 35 (more than one tile each way, remainders in both), a
2-camera 64 x 32 panorama."""
import statistics
import time

import numpy as np
import pytest

from tests import test_gpu_panorama as gp
from tests import test_gpu_stereo_filter as gf
from tests import test_gpu_sweep as gs
from tests.test_corners_oracle import _scene
from tscm_calib_amd import corners, maps, rig, stereo, sweep, synth

pytestmark = pytest.mark.gpu

CALLS, WARM = 21, 3


def _timed(call):
    """-> (what call() returned, wall seconds of the call)"""
    t0 = time.perf_counter()
    res = call()
    return res, time.perf_counter() - t0


def _inside(seconds, wall):
    assert 0.0 < seconds < wall, (seconds, wall)


def _sum_in_order(times):
    total = 0.0
    for t in times:
        total += t
    return total


def _is_fresh(values):
    return statistics.median(values[-3:]) < 3.0 * statistics.median(values[:3])


def _fresh_values(call, seconds=lambda res: res[-1], warm=False):
    """CALLS calls of call() -> their reported seconds, each inside its wall time and none of them a running sum; warm: the
    calls that load the kernels come first"""
    for _ in range(WARM if warm else 0):
        call()
    values = []
    for _ in range(CALLS):
        res, wall = _timed(call)
        _inside(seconds(res), wall)
        values.append(seconds(res))
    assert _is_fresh(values), values
    assert not _is_fresh(np.cumsum(values).tolist()), values          # what the law is for: it refuses the running sum of these values
    return values


# ------------------------------------------------------------------------------------------------ totals and stage times
def _matcher_law(sec, st):
    times = [st[k] for k in stereo.STAGE_NAMES]
    assert all(t >= 0.0 for t in times) and st["aggregate"] > 0.0, st
    assert abs(sec - _sum_in_order(times)) <= 1e-12 * sec, (sec, times)


def test_matcher_total_is_the_sum_of_its_stage_times(hip_device):
    left, right = gf._board_pair(96, 48)
    match = lambda: stereo.match(left, right, device=hip_device, with_seconds=True, num_disparities=32)
    stages = []

    def call():
        res = match()
        stages.append(stereo.stage_times())
        _matcher_law(res[1], stages[-1])
        return res

    _fresh_values(call, warm=True)
    assert _is_fresh([st["aggregate"] for st in stages[WARM:]]), stages      # a stage time is fresh as well


def test_sweep_total_is_the_sum_of_its_stage_times(hip_device):
    n, D, pw, ph = 2, 16, 64, 32
    mx, my = gs._tables(n, D, pw, ph)
    images = gs._images(n)
    for warm in (True, False):                                              # the first handle loads the kernels
        with sweep.Sweeper.from_tables(mx, my, (gs.SRC_W, gs.SRC_H), device=hip_device) as s:
            def call():
                res = s.depth(images, with_seconds=True)
                times = s.stage_times().tolist()                            # cost volume, aggregation, winner
                assert all(t >= 0.0 for t in times) and times[1] > 0.0, times
                assert abs(res[1] - _sum_in_order(times)) <= 1e-12 * res[1], (res[1], times)
                return res
            if warm:
                _ = [call() for _ in range(WARM)]
            else:
                _fresh_values(call)


# ------------------------------------------------------------------------------------------------ one-shot entry points
def test_map_stages_report_their_device_time(hip_device):
    d = gf._random_map(130, 35)
    guide = np.random.default_rng(5).integers(0, 256, d.shape).astype(np.uint8)
    for call in (lambda: stereo.filter(d, device=hip_device, with_seconds=True, median=3),
                 lambda: stereo.fill(d, device=hip_device, with_seconds=True, max_distance=40),
                 lambda: stereo.refine(d, guide, device=hip_device, with_seconds=True, sigma=8.0, iterations=2)):
        _fresh_values(call, warm=True)


def test_map_builders_report_their_device_time(hip_device):
    descs, centers = gs._rig_descs(gs.mref.EQUIRECT)
    pinhole = maps.undistort_desc(synth.CALIB_INTR[2], 250.0, 250.0, 100.0, 80.0, 203, 77, out_stride=205)      # ragged rows
    inv = sweep.inverse_distances(500.0, D=16)
    for call in (lambda: maps.build_maps([pinhole], device=hip_device),     # tscm_build_maps
                 lambda: maps.build_maps([descs[0]], device=hip_device),    # tscm_build_maps_ex
                 lambda: maps.build_sweep_maps(descs, centers, inv, device=hip_device)):
        _fresh_values(call, warm=True)


def test_corner_detector_and_rig_init_report_their_device_time(hip_device):
    img, _ = _scene(3, 0)
    detect = lambda: corners.detect_corners(img, device=hip_device)
    _fresh_values(detect, seconds=lambda g: g["seconds"], warm=True)                 # the arena of the first call is kept: still fresh values
    inp = synth.make_rig_input(synth.make_problem(4, 12, 7))
    init = lambda: rig.rig_init(inp, hip_device)
    _fresh_values(init, seconds=lambda g: g["seconds_hypotheses"], warm=True)


# ------------------------------------------------------------------------------------------------ handles
@pytest.mark.parametrize("mode,levels", [("seam", 0), ("feather", 0), ("multiband", 2)])
def test_panorama_composer_reports_each_call(hip_device, mode, levels):
    n, ch, pw, ph = 2, 1, 64, 32
    images = list(gp._images(n, ch))
    for warm in (True, False):                                              # the first handle loads the kernels
        with gp._composer(n, ch, pw, ph, mode, levels, True, False, hip_device) as c:
            call = lambda: c.compose(images, with_seconds=True)
            if warm:
                _ = [call() for _ in range(WARM)]
            else:
                _fresh_values(call)


@pytest.mark.parametrize("visibility", [None, dict(cell_shift=1)], ids=["plain", "visible"])
@pytest.mark.parametrize("mode,levels", [("seam", 0), ("feather", 0), ("multiband", 2)])
def test_sweep_composer_and_visibility_report_each_call(hip_device, mode, levels, visibility):
    n, D, pw, ph = 2, 16, 64, 32
    mx, my = gs._tables(n, D, pw, ph)
    images = gs._images(n)
    for warm in (True, False):                                              # the first handle loads the kernels
        with sweep.Sweeper.from_tables(mx, my, (gs.SRC_W, gs.SRC_H), device=hip_device) as s:
            s.depth(images)
            compose = lambda: s.compose(images, with_seconds=True, visibility=visibility, mode=mode, levels=max(levels, 1))
            passes = lambda: s.visibility(with_seconds=True)
            if warm:
                _ = [(compose(), passes()) for _ in range(WARM)]
            else:
                _fresh_values(compose)
                _fresh_values(passes)
