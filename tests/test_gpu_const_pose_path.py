"""k_eval_gram4's constant-pose path: the waves of a camera whose pose block is held constant form no camera-rotation
columns w_c (the reduced system has no column for them: plan_columns), two 4x4x4 MFMAs per four rows instead of three.

(a) api.normal_equations(as_solved=True) -- the evaluation launch as a solve makes it -- against the same entry without
    it, which forms every column: every entry outside the dropped rows and columns has the same bits, the dropped ones
    are exactly 0 on a fresh solver, the cost is equal.  Every kind of instantiation: KS 1, KS 14, MULTI (KS 11), ROBUST;
    ragged views (lost corners, pass boundaries, empty views) and chunks of more than 64 views.
(b) solves against TSCM_EXEC_GRAM_16X16, whose kernel forms every column whatever the plan says: rigs of 2, 3 and 4
    cameras, the constant camera not always camera 0, 12 forced iterations with rejected steps among them -- iteration
    logs and final parameters byte-equal.
(c) the same for a solo mono solve (every chunk takes the path)."""
import numpy as np
import pytest

from tscm_calib_amd import api, lib, synth
from tests.test_gpu_gram_kernels import g4_plan, n_cus, ragged      # noqa: F401  (n_cus: fixture)

pytestmark = pytest.mark.gpu

KEYS = ("board_gram", "board_grad", "view_cross", "cam_gram", "cam_grad")
BOARDS = [(2, 2), (9, 6), (11, 8)]                  # KS 1 | KS 14 | two passes of KS 11
CONST = {"cam0": [1, 0, 0, 0], "cam0+2": [1, 0, 1, 0], "mono": None}


def _problem(cols, rows, const, n_views, seed):
    n = cols * rows
    C = 1 if const is None else len(const)
    p = synth.make_problem(C, n_views // C, seed, cols=cols, rows=rows, pitch=360.0 / max(cols, rows))
    if const is not None:
        p.cam_pose_constant = np.asarray(const, dtype=np.uint8)
    return ragged(p, n, g4_plan(n)[1])


def _dropped(p):
    """Boolean masks of the entries the constant-pose path leaves out: rows and columns 0-2 (w_c) of a constant camera's
    tile and gradient, columns 0-2 of the W block of its views."""
    const = np.ones(p.n_cameras, bool) if p.mono else p.cam_pose_constant.astype(bool)
    assert const.any()
    m = {k: None for k in KEYS}
    cg = np.zeros((p.n_cameras, 15, 15), bool)
    cg[const, 0:3, :] = True
    cg[const, :, 0:3] = True
    m["cam_gram"] = cg
    m["cam_grad"] = np.zeros((p.n_cameras, 15), bool)
    m["cam_grad"][const, 0:3] = True
    m["view_cross"] = np.zeros((p.n_views, 6, 15), bool)
    m["view_cross"][const[p.view_camera] & (p.view_count > 0), :, 0:3] = True
    return m


def _check_as_solved(p, tag, **kw):
    full = api.normal_equations(p, **kw)
    part = api.normal_equations(p, as_solved=True, **kw)
    masks = _dropped(p)
    assert part["cost"] == full["cost"], tag
    for k in KEYS:
        m = masks[k] if masks[k] is not None else np.zeros(full[k].shape, bool)
        assert np.array_equal(part[k][~m], full[k][~m]), (tag, k)
        assert np.all(part[k][m] == 0.0), (tag, k)
        # the full path does form these entries: the comparison above is one of two different code paths
        if m.any():
            assert np.count_nonzero(full[k][m]) > 0.5 * m.sum(), (tag, k)


@pytest.mark.parametrize("const", list(CONST), ids=list(CONST))
@pytest.mark.parametrize("cols,rows", BOARDS, ids=[f"{c}x{r}" for c, r in BOARDS])
def test_as_solved_drops_only_the_rotation_columns_of_constant_cameras(hip_device, n_cus, cols, rows, const):
    """32 ragged views per CU: chunks of two views or more, a short view behind a long one."""
    p = _problem(cols, rows, CONST[const], 32 * n_cus, 500 + cols * rows)
    assert p.n_views >= 32 * n_cus and (p.view_count == 0).any()
    _check_as_solved(p, f"{cols}x{rows} {const}")


def test_as_solved_on_chunks_of_more_than_64_views(hip_device, n_cus):
    """4 x 70,000 views of a 2 x 2 board: every chunk passes 64 views and reloads its view metadata."""
    p = _problem(2, 2, CONST["cam0+2"], 4 * 70_000, 81)
    assert p.n_views > 64 * 16 * n_cus
    _check_as_solved(p, "2x2 x 280,000 views")


@pytest.mark.parametrize("cols,rows", [(9, 6), (11, 8)], ids=["9x6", "11x8"])
def test_as_solved_with_a_huber_loss(hip_device, n_cus, cols, rows):
    """The ROBUST instantiations (single pass and MULTI)."""
    p = _problem(cols, rows, CONST["cam0+2"], 8 * n_cus, 91)
    _check_as_solved(p, f"{cols}x{rows} huber", loss=("huber", 0.1))


FORCED = dict(max_num_iterations=12, function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0,
              min_trust_region_radius=0.0, initial_trust_region_radius=1e8)


def _pattern(s):
    return "".join("A" if it["step_is_successful"] else ("r" if it["step_is_valid"] else "x") for it in s["iterations"][1:])


def _solve_both(p):
    """The default solve (k_eval_gram4, constant-pose path) and the 16x16 kernel's: logs and parameters byte-equal."""
    a, b = p.copy().normalised(), p.copy().normalised()
    run = (lambda q, **o: api.refinement(q, **o)[1]) if p.mono else api.calibrate
    sa, sb = run(a, **FORCED), run(b, exec_flags=lib.EXEC_GRAM_16X16, **FORCED)
    assert sa["lm_iterations"] == 12 and "r" in _pattern(sa), _pattern(sa)
    assert sa["iterations"] == sb["iterations"] and sa["final_cost"] == sb["final_cost"] and sa["message"] == sb["message"]
    for x, y in ((a.cam_rt, b.cam_rt), (a.intr, b.intr), (a.board_rt, b.board_rt)):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("C,const,seed", [(2, 1, 41), (3, 2, 42), (4, 0, 43), (4, 3, 44)], ids=["2cam-c1", "3cam-c2", "4cam-c0", "4cam-c3"])
def test_solves_equal_the_16x16_kernel_s_byte_for_byte(hip_device, C, const, seed):
    """A nearly undamped first step (radius 1e8) overshoots: rejected steps among the twelve."""
    p = synth.make_problem(C, 24, seed)
    k = np.zeros(C, dtype=np.uint8)
    k[const] = 1
    p.cam_pose_constant = k
    _solve_both(p.normalised())


def test_mono_solve_equals_the_16x16_kernel_s_byte_for_byte(hip_device):
    _solve_both(synth.make_problem(1, 60, 45).normalised())
