"""k_solve_reduced with the solution carried through the factorisation (e-row and solution tiles, plan_solve_ext) against
the back-substitution it replaces, on the GPU.

Rigs (synth.make_problem, 6-8 views per camera), by the reduced system's free columns:
  c1     one camera (7 columns, 2 panels)
  c2     two cameras, camera 0 constant (20 columns, 5 full panels)
  c4     a ring of four, camera 0 constant (46 columns: 12 panels, the last one partial)
  c4-41  the same with five held intrinsics (41 columns: 11 panels, the last one partial)
  c4-52  a ring of four with no constant camera pose (52 columns, 13 panels: the plan's fallback, which back-substitutes);
         every third board is constant instead, which holds the gauge: with a free gauge the system at radius 1e12 is
         singular up to the damping (kappa 2e12) and the forward error of the back-substitution path itself -- the code
         as it was -- measured 110 kappa eps on the boards, past C_KAPPA = 100, so that rig says nothing about either path
For each rig one LM step at radius 1e-2 and one at 1e12, on the default path and with
tscm_solver_debug_reduced_backsub on the old one: both candidates within the backward / forward tolerances of
tests/test_gpu_step.py (TAU_B, TAU_F: test_gpu_step.tolerances) of the extended-precision step of tests/helpers.py.  On
the fallback rig the setter changes no bit (both runs back-substitute); on c4 it must change some, or the new path was
not taken.  With the setter left alone, the candidate's bits
do not depend on the TSCM_EXEC_* fusion flags (the property of test_fusion_flags_keep_the_candidate_bits on these rigs).
"""
import functools

import numpy as np
import pytest

from tscm_calib_amd import api, lib, synth
from tests import helpers as H
from tests import test_gpu_step as ST
from tests.test_fixed_reference import masked_columns

pytestmark = pytest.mark.gpu

F = lib.FIX
# (problem, held-intrinsics words or None, free columns of the reduced system)
RIGS = {
    "c1": (lambda: synth.make_problem(1, 8, 4301), None, 7),
    "c2": (lambda: synth.make_problem(2, 7, 4302), None, 20),
    "c4": (lambda: synth.make_problem(4, 6, 4304), None, 46),
    "c4-41": (lambda: synth.make_problem(4, 6, 4304), [F["cx"] | F["cy"], F["cx"] | F["cy"], F["cx"], 0], 41),
    "c4-52": (lambda: ST.with_const_boards(ST.with_const_cams(synth.make_problem(4, 6, 4305), [])), None, 52),
}
RADII = (1e-2, 1e12)


@functools.lru_cache(maxsize=None)
def rig(name):
    build, fixed, n_cols = RIGS[name]
    p = build().normalised()
    cols = masked_columns(p, np.asarray(fixed)) if fixed is not None else H.step_columns(p)
    assert int(cols["cam_free"].sum()) == n_cols, (name, int(cols["cam_free"].sum()))
    return p, fixed, cols, H.step_terms(p)


@functools.lru_cache(maxsize=None)
def reference(name, radius):
    p, _, cols, terms = rig(name)
    ref = H.reference_step(p, terms=terms, cols=cols, initial_trust_region_radius=radius)
    assert ref["ok"]
    return ref


def step(name, device, **opt):
    p, fixed, _, _ = rig(name)
    return api.step(p, device, fixed=fixed, **opt)


def step_on_old_path(name, device, **opt):
    api.debug_reduced_backsub_default(True)
    try:
        return step(name, device, **opt)
    finally:
        api.debug_reduced_backsub_default(False)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", sorted(RIGS))
def test_both_paths_against_extended_precision(hip_device, name, radius):
    p = rig(name)[0]
    ref = reference(name, radius)
    opt = dict(initial_trust_region_radius=radius)
    tau_b, tau_f, _ = ST.tolerances((name, name, opt), ref["kappa"], ref["cost"], ref["model_cost_change"])
    cand = {"new": step(name, hip_device, **opt), "old": step_on_old_path(name, hip_device, **opt)}
    for path, g in cand.items():
        assert g["valid"], path
        e = H.step_errors(p, ref, g)
        print(f"{name} radius {radius:g} {path}: backward {e['backward']:.3g} forward pose {e['forward_cam_pose']:.3g} "
              f"intr {e['forward_intr']:.3g} board {e['forward_board']:.3g}  (tau_b {tau_b:g}, tau_f {tau_f:.3g}, kappa {ref['kappa']:.3g})")
        assert e["backward"] <= tau_b, (path, e["backward"])
        for k in ("forward_cam_pose", "forward_intr", "forward_board"):
            assert not e[k] > tau_f, (path, k, e[k], tau_f)
    if name == "c4-52":
        # the plan's fallback: the setter has nothing to switch
        for k in ("cam_rt", "intr", "board_rt"):
            assert np.array_equal(cand["new"][k], cand["old"][k]), k
    if name == "c4":
        # the two paths round differently over 46 columns: equal bits would mean that the new path was never taken (a plan or a
        # switch that silently stayed off) and that both candidates above are the back-substitution's
        assert any(not np.array_equal(cand["new"][k], cand["old"][k]) for k in ("cam_rt", "intr", "board_rt"))


@pytest.mark.parametrize("name", sorted(RIGS))
def test_fusion_flags_keep_the_candidate_bits(hip_device, name):
    base = step(name, hip_device)
    assert base["valid"]
    for f in ST.FUSION_FLAGS:
        g = step(name, hip_device, exec_flags=f)
        for k in ("cam_rt", "intr", "board_rt"):
            assert np.array_equal(g[k], base[k]), (f, k)


def test_setter_on_a_solver_switches_that_solver_only(hip_device):
    """Solver.debug_reduced_backsub: the same one-iteration solve on both paths of one solver accepts its step, the
    setter moves the bits, and switching back gives the first run's bits again."""
    p = rig("c4")[0]
    opt = dict(max_num_iterations=1, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    runs = []
    q = p.copy().normalised()
    with api.Solver(q, hip_device) as s:
        for on in (False, True, False):
            s.debug_reduced_backsub(on)
            s.upload_params(p.cam_rt, p.intr, p.board_rt)
            r = s.solve_resident(**opt)
            assert r["iterations"][1]["step_is_successful"]
            runs.append(s.download_params())
    for a, c in zip(runs[0], runs[2]):
        assert np.array_equal(a, c)
    assert any(not np.array_equal(a, b) for a, b in zip(runs[0], runs[1])), "the setter switched nothing"
