"""Every C-ABI entry point that takes a device index answers an index outside [0, tscm_device_count()) with
TSCM_E_NO_DEVICE, and checks its required pointers before it looks at the device: a NULL one together with the bad
index is TSCM_E_INVALID.  The index used is tscm_device_count() itself, which is out of range on every machine, so no
call here reaches a GPU (no `gpu` marker: the test runs with and without one)."""
import ctypes as C

import numpy as np
import pytest

from tscm_calib_amd import lib, synth

E_INVALID, E_NO_DEVICE = -1, -2
dbl, i32, u8 = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)


def _cases():
    """(name, call(device) with valid tiny arguments, call(device) with one required pointer NULL or None)"""
    L = lib.lib()
    p = synth.make_problem(2, 4, 5).normalised()
    cp, o, s = lib.c_problem(p), lib.default_options(False), lib.CSummary()
    h = C.c_void_p()
    buf = np.zeros(65536)
    d = lib.dptr(buf)                                       # any output array: nothing is written before the device check
    valid = C.c_int(0)
    masks = lib.ushort_ptr(np.zeros(p.n_cameras, np.uint16))
    P, O, S, V = C.byref(cp), C.byref(o), C.byref(s), C.byref(valid)
    HUBER = lib.LOSS_HUBER
    out = [
        ("tscm_device_synchronize", lambda dv: L.tscm_device_synchronize(dv), None),
        ("tscm_solver_create", lambda dv: L.tscm_solver_create(P, dv, C.byref(h)), lambda dv: L.tscm_solver_create(P, dv, None)),
        ("tscm_solver_create_sharded", lambda dv: L.tscm_solver_create_sharded(P, dv, 0, 1, C.byref(h)),
         lambda dv: L.tscm_solver_create_sharded(None, dv, 0, 1, C.byref(h))),
        ("tscm_eval_functor", lambda dv: L.tscm_eval_functor(P, dv, d, d, d, d, d), lambda dv: L.tscm_eval_functor(None, dv, d, d, d, d, d)),
        ("tscm_eval_normal_equations", lambda dv: L.tscm_eval_normal_equations(P, dv, d, d, d, d, d, d),
         lambda dv: L.tscm_eval_normal_equations(None, dv, d, d, d, d, d, d)),
        ("tscm_eval_normal_equations_ex", lambda dv: L.tscm_eval_normal_equations_ex(P, dv, O, d, d, d, d, d, d),
         lambda dv: L.tscm_eval_normal_equations_ex(None, dv, O, d, d, d, d, d, d)),
        ("tscm_eval_normal_equations_robust", lambda dv: L.tscm_eval_normal_equations_robust(P, dv, O, HUBER, 1.0, d, d, d, d, d, d),
         lambda dv: L.tscm_eval_normal_equations_robust(None, dv, O, HUBER, 1.0, d, d, d, d, d, d)),
        ("tscm_eval_step_ex", lambda dv: L.tscm_eval_step_ex(P, dv, O, d, d, d, V, S), lambda dv: L.tscm_eval_step_ex(P, dv, O, d, None, d, V, S)),
        ("tscm_eval_step_robust", lambda dv: L.tscm_eval_step_robust(P, dv, O, HUBER, 1.0, d, d, d, V, S),
         lambda dv: L.tscm_eval_step_robust(P, dv, O, HUBER, 1.0, d, d, d, None, S)),
        ("tscm_eval_step_fixed", lambda dv: L.tscm_eval_step_fixed(P, dv, O, masks, 0, 0.0, d, d, d, V, S),
         lambda dv: L.tscm_eval_step_fixed(None, dv, O, masks, 0, 0.0, d, d, d, V, S)),
        ("tscm_project_points", lambda dv: L.tscm_project_points(d, d, 4, dv, d), lambda dv: L.tscm_project_points(None, d, 4, dv, d)),
        ("tscm_unproject_pixels", lambda dv: L.tscm_unproject_pixels(d, d, 4, dv, d), lambda dv: L.tscm_unproject_pixels(d, d, 4, dv, None)),
        ("tscm_reprojection_error", lambda dv: L.tscm_reprojection_error(P, dv, d, d, d), lambda dv: L.tscm_reprojection_error(None, dv, d, d, d)),
    ]
    # batched mono refinement
    m = synth.make_problem(1, 3, 7).normalised()
    cps, sums = (lib.CProblem * 1)(lib.c_problem(m)), (lib.CSummary * 1)()
    om = lib.default_options(True)
    out.append(("tscm_solve_mono_batch", lambda dv: L.tscm_solve_mono_batch(cps, 1, dv, C.byref(om), None, 0, 0.0, sums),
                lambda dv: L.tscm_solve_mono_batch(cps, 1, dv, C.byref(om), None, 0, 0.0, None)))
    # mono initialisation: two images of one 4 x 3 board
    cnt = np.full(2, 12, np.int32).ctypes.data_as(i32)
    used, ivec = C.c_int(0), np.zeros(16, np.int32).ctypes.data_as(i32)
    out += [
        ("tscm_estimate_focal", lambda dv: L.tscm_estimate_focal(d, d, cnt, 2, 4, 3, 8.0, 8.0, dv, d, C.byref(used)),
         lambda dv: L.tscm_estimate_focal(d, d, cnt, 2, 4, 3, 8.0, 8.0, dv, None, C.byref(used))),
        ("tscm_estimate_focal_rows", lambda dv: L.tscm_estimate_focal_rows(d, d, cnt, 2, 4, 3, 8.0, 8.0, dv, d),
         lambda dv: L.tscm_estimate_focal_rows(d, d, cnt, 2, 4, 3, 8.0, 8.0, dv, None)),
        ("tscm_estimate_extrinsic", lambda dv: L.tscm_estimate_extrinsic(d, d, d, cnt, 2, d, 12, 4, dv, d, C.byref(used)),
         lambda dv: L.tscm_estimate_extrinsic(None, d, d, cnt, 2, d, 12, 4, dv, d, C.byref(used))),
        ("tscm_estimate_extrinsic_stages", lambda dv: L.tscm_estimate_extrinsic_stages(d, d, d, cnt, 2, d, 12, 4, dv, d, C.byref(used), d, d, d, d, ivec, ivec),
         lambda dv: L.tscm_estimate_extrinsic_stages(d, d, d, cnt, 2, d, 12, 4, dv, d, C.byref(used), d, d, d, d, ivec, None)),
    ]
    # remap tables and their application: one 16 x 16 map, one 16 x 16 image
    md = lib.CMapDesc()
    md.width = md.height = md.out_stride = 16
    md.fx = md.fy = 8.0
    fl = np.zeros(256, np.float32)
    fp = fl.ctypes.data_as(C.POINTER(C.c_float))
    kinds = np.zeros(1, np.int32).ctypes.data_as(i32)
    img = np.zeros((16, 16), np.uint8)
    img2 = np.zeros((16, 16), np.uint8)
    flag = np.zeros(16, np.uint8).ctypes.data_as(u8)
    remap = L.tscm_remap
    remap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    out += [
        ("tscm_build_maps", lambda dv: L.tscm_build_maps(C.byref(md), 1, dv, 0, fp, fp, 256, None), lambda dv: L.tscm_build_maps(None, 1, dv, 0, fp, fp, 256, None)),
        ("tscm_build_maps_ex", lambda dv: L.tscm_build_maps_ex(C.byref(md), kinds, 1, dv, 0, fp, fp, 256, None),
         lambda dv: L.tscm_build_maps_ex(C.byref(md), kinds, 1, dv, 0, None, fp, 256, None)),
        ("tscm_rectify_points", lambda dv: L.tscm_rectify_points(C.byref(md), 0, d, 4, dv, d, flag), lambda dv: L.tscm_rectify_points(None, 0, d, 4, dv, d, flag)),
        ("tscm_remap", lambda dv: remap(img.ctypes.data, 16, 16, 16, 1, fl.ctypes.data, fl.ctypes.data, 16, 16, 16, 0, dv, img2.ctypes.data, 16),
         lambda dv: remap(None, 16, 16, 16, 1, fl.ctypes.data, fl.ctypes.data, 16, 16, 16, 0, dv, img2.ctypes.data, 16)),
    ]
    # rig initialisation
    rin = synth.make_rig_input(synth.make_problem(2, 4, 5)).normalised()
    q, r = lib.CRigInput(), lib.CRigResult()
    q.n_cameras, q.n_boards, q.n_points = rin.n_cameras, rin.n_boards, rin.n_points
    for name in ("worlds", "intr", "has", "Rt", "pix_u", "pix_v"):
        setattr(q, name, getattr(rin, name).ctypes.data)
    for name in ("cam_R", "cam_t", "cam_rt", "board_R", "board_t", "board_rt", "board_initial"):
        setattr(r, name, buf.ctypes.data)
    eye = lib.dptr(np.eye(3).reshape(9).copy())
    out += [
        ("tscm_rig_init", lambda dv: L.tscm_rig_init(C.byref(q), dv, C.byref(r)), lambda dv: L.tscm_rig_init(C.byref(q), dv, None)),
        ("tscm_rig_stage_errors", lambda dv: L.tscm_rig_stage_errors(C.byref(q), 1, eye, d, 0, dv, d, d, d, None),
         lambda dv: L.tscm_rig_stage_errors(C.byref(q), 1, None, d, 0, dv, d, d, d, None)),
    ]
    # corner detector: one 16 x 16 image, sigma 4 (the reference's)
    imgs = (C.c_void_p * 1)(img.ctypes.data)
    cand = lib.CCornerCandidates()
    det, det_b, planes = L.tscm_detect_corners, L.tscm_detect_corners_batch, L.tscm_corner_planes_batch
    det.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]
    det_b.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]
    planes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
    out += [
        ("tscm_detect_corners", lambda dv: det(img.ctypes.data, 16, 16, 16, 4, 0.01, dv, C.addressof(cand)),
         lambda dv: det(None, 16, 16, 16, 4, 0.01, dv, C.addressof(cand))),
        ("tscm_detect_corners_batch", lambda dv: det_b(C.addressof(imgs), 1, 16, 16, 16, 4, 0.01, dv, C.addressof(cand)),
         lambda dv: det_b(C.addressof(imgs), 1, 16, 16, 16, 4, 0.01, dv, None)),
        ("tscm_corner_planes_batch", lambda dv: planes(C.addressof(imgs), 1, 16, 16, 16, 4, dv, None, None, None),
         lambda dv: planes(None, 1, 16, 16, 16, 4, dv, None, None, None)),
    ]
    # communicators and the micro-benchmarks
    comm = (C.c_void_p * 2)()
    handle = (C.c_ubyte * lib.IPC_HANDLE_BYTES)()
    uid = (C.c_ubyte * lib.UNIQUE_ID_BYTES)()
    out += [
        ("tscm_comm_create", lambda dv: L.tscm_comm_create(uid, 0, 1, dv, comm), lambda dv: L.tscm_comm_create(None, 0, 1, dv, comm)),
        ("tscm_comm_create_local", lambda dv: L.tscm_comm_create_local(2, dv, comm), lambda dv: L.tscm_comm_create_local(2, dv, None)),
        ("tscm_comm_ipc_open", lambda dv: L.tscm_comm_ipc_open(0, 1, dv, 64, comm, handle), lambda dv: L.tscm_comm_ipc_open(0, 1, dv, 64, comm, None)),
        ("tscm_device_peak_fp64", lambda dv: L.tscm_device_peak_fp64(dv, d, d), None),      # (both outputs are optional)
        ("tscm_device_peak_fp64_ex", lambda dv: L.tscm_device_peak_fp64_ex(dv, d), lambda dv: L.tscm_device_peak_fp64_ex(dv, None)),
        ("tscm_device_peak_fp32_mfma", lambda dv: L.tscm_device_peak_fp32_mfma(dv, d), lambda dv: L.tscm_device_peak_fp32_mfma(dv, None)),
    ]
    keep = (p, cp, o, s, buf, m, cps, sums, om, md, fl, img, img2, rin, q, r, imgs, cand, comm, handle, uid)
    return [(name, good, null, keep) for name, good, null in out]


CASES = _cases()


@pytest.mark.parametrize("name,good,null,keep", CASES, ids=[c[0] for c in CASES])
def test_out_of_range_device_is_no_device_and_arguments_come_first(name, good, null, keep):
    L = lib.lib()
    n = L.tscm_device_count()
    for dv in (n, -1):
        assert good(dv) == E_NO_DEVICE, (name, dv)
        assert L.tscm_last_error(), name
    if null is not None:
        assert null(n) == E_INVALID, name


def test_every_export_with_a_device_argument_is_covered():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tscm", "tscm.h")).read()
    decls = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S).split(";")
    with_device = {m.group(1) for m in (re.search(r"\b(tscm_[a-z_0-9]+)\s*\(.*\bint device\b", x, re.S) for x in decls) if m}
    assert with_device == {c[0] for c in CASES}, with_device ^ {c[0] for c in CASES}
