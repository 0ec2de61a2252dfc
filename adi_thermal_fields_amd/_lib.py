"""ctypes binding of libadi_hip.so (include/adi_hip.h).

The product path has NO CPU fallback: if the HIP library is missing this module raises at import
time with the command that builds it.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('ADI_HIP_LIB') or os.path.join(_HERE, 'csrc', 'libadi_hip.so')   # env: A/B builds of the kernels

ADI_OK, ADI_ERR_ARG, ADI_ERR_HIP, ADI_ERR_UNSUPPORTED, ADI_ERR_STATE = 0, 1, 2, 3, 4
FACE_NONE, FACE_SCALAR, FACE_FIELD = 0, 1, 2
ZBC_KINDS = {'neumann0': 0, 'dirichlet': 1, 'robin': 2}
SWEEP_GENERAL, SWEEP_NO_DIR, SWEEP_NO_Q, SWEEP_LEAN = 0, 1, 2, 3
# bytes per cell each sweep variant moves (its input arrays + the output), SURVEY.md 8(d) variant rule
SWEEP_BYTES_PER_CELL = {SWEEP_GENERAL: 42, SWEEP_NO_DIR: 33, SWEEP_NO_Q: 34, SWEEP_LEAN: 25}
EXPLICIT_BYTES_PER_CELL = 17
FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "adi_thermal_fields_amd: %s not found. Build the HIP library first:\n"
        "    python -m adi_thermal_fields_amd.build\n"
        "(there is no CPU fallback; the MI355X kernels are the product)" % LIB_PATH)

lib = ctypes.CDLL(LIB_PATH)

c_int, c_double, c_void_p, c_size_t = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
c_long = ctypes.c_long
c_int_p = ctypes.POINTER(c_int)
c_double_p = ctypes.POINTER(c_double)
c_void_pp = ctypes.POINTER(c_void_p)

# every exported symbol of include/adi_hip.h: name -> (restype, argtypes)
SIGNATURES = {
    'adi_abi_version': (c_int, []),
    'adi_build_stamp': (ctypes.c_char_p, []),
    'adi_last_error': (ctypes.c_char_p, []),
    'adi_device_count': (c_int, [c_int_p]),
    'adi_device_info': (c_int, [c_int, ctypes.c_char_p, c_int_p, ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]),
    'adi_recommended_plane_stride': (ctypes.c_long, [c_int, c_int]),
    'adi_recommended_dims': (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'adi_exposed_mask': (c_int, [c_void_p, c_int, c_int, c_int, c_long, c_int, c_void_p, c_void_p]),
    'adi_build_coeffs': (c_int, [c_void_p, c_int, c_int, c_int, c_long, c_double, c_double, c_double,
                                 c_int_p, c_double_p, c_void_pp, c_int_p, c_double_p, c_void_pp,
                                 c_void_pp, c_void_pp, c_void_p]),
    'adi_build_nbr_flags': (c_int, [c_void_p, c_int, c_int, c_int, c_long, c_void_p, c_void_p]),
    'adi_build_nbr_flags_planes': (c_int, [c_void_p, c_int, c_int, c_int, c_long, c_void_p, c_int, c_int, c_void_p]),
    'adi_flag_bricks_words': (ctypes.c_long, [c_int, c_int, c_int]),
    'adi_build_flag_bricks': (c_int, [c_void_p, c_int, c_int, c_int, c_long, c_void_p, c_int, c_int, c_void_p]),
    'adi_build_coeffs_planes': (c_int, [c_void_p, c_int, c_int, c_int, c_long, c_double, c_double, c_double,
                                        c_int_p, c_double_p, c_void_pp, c_int_p, c_double_p, c_void_pp,
                                        c_void_pp, c_void_pp, c_int, c_int, c_void_p]),
    'adi_explicit_rhs': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_double, c_double, c_double,
                                 c_double, c_void_p, c_void_p]),
    'adi_explicit_rhs_planes': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_double, c_double, c_double,
                                        c_double, c_void_p, c_int, c_int, c_void_p]),
    'adi_sweep': (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                          c_int, c_int, c_int, c_long, c_int, c_double, c_double, c_double, c_double,
                          c_void_p, c_void_p, c_void_p, c_double_p, c_void_p, c_size_t, c_void_p]),
    'adi_sweep_bricks': (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int, c_int, c_int, c_long, c_int, c_double, c_double, c_double, c_double,
                                 c_void_p, c_void_p, c_void_p, c_double_p, c_void_p, c_size_t, c_void_p]),
    'adi_face_constants': (c_int, [c_double, c_double, c_double, c_int_p, c_double_p, c_int_p, c_double_p, c_double_p, c_int_p]),
    'adi_sweep_workspace_bytes': (c_int, [c_int, c_int, c_int, c_int, c_long, ctypes.POINTER(c_size_t)]),
    'adi_sweep_condense': (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_int, c_int, c_int, c_long, c_int, c_double, c_double, c_double, c_double,
                                   c_void_p, c_double_p, c_void_p, c_size_t, c_void_p]),
    'adi_explicit_fused_supported': (c_int, [c_int, c_int, c_int, c_long, c_int]),
    'adi_explicit_sweep0': (c_int, [c_int, c_void_p, c_long, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int, c_int, c_int, c_long, c_int, c_double, c_double, c_double, c_double, c_double,
                                    c_void_p, c_void_p, c_void_p, c_double_p, c_void_p, c_size_t, c_void_p]),
    'adi_explicit_sweep0_bricks': (c_int, [c_int, c_void_p, c_long, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_int, c_int, c_int, c_long, c_int, c_double, c_double, c_double, c_double,
                                           c_double, c_void_p, c_void_p, c_void_p, c_double_p, c_void_p, c_size_t, c_void_p]),
    'adi_explicit_condense0': (c_int, [c_int, c_void_p, c_long, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int, c_int, c_int, c_long, c_int, c_double, c_double, c_double, c_double,
                                       c_double, c_void_p, c_void_p, c_double_p, c_void_p, c_size_t, c_void_p]),
    'adi_axis0_dots_supported': (c_int, [c_int, c_int, c_int, c_long]),
    'adi_axis0_dots_workspace': (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]),
    'adi_axis0_dots_setup': (c_int, [c_int, c_double, c_double, c_void_p, c_void_p]),
    'adi_axis0_classify': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_void_p, c_void_p, c_void_p]),
    'adi_axis0_dots_ichunk': (c_int, [c_int]),
    'adi_explicit_rhs_dots': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_double, c_double, c_double,
                                      c_double, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'adi_axis0_dots_finish': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_double, c_double,
                                      c_double, c_double, c_long, c_long, c_void_p, c_void_p]),
    'adi_interface_solve': (c_int, [c_void_p, c_int, c_int, c_long, c_void_p, c_void_p, c_void_p]),
    'adi_interface_pair': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p]),
    'adi_axis0_deferred_setup': (c_int, [c_int, c_double, c_double, c_double, c_void_p, c_double_p, c_int_p, c_void_p]),
    'adi_axis0_weights_host': (c_int, [c_int, c_double, c_double, c_int, c_double, c_void_p, c_int_p]),
    'adi_interface_deferred': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_long, c_void_p, c_void_p, c_void_p]),
    'adi_deferred_exact_setup': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_double, c_double, c_double,
                                         c_long, c_void_p, c_void_p, c_void_p]),
    'adi_interface_solve_uniform': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_long, c_void_p, c_void_p, c_void_p]),
    'adi_deferred_exact_coef': (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p]),
    'adi_sweep_corrected': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int, c_int, c_int, c_long, c_int, c_double, c_double, c_double, c_double,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_double_p, c_void_p, c_size_t,
                                    c_void_p]),
    'adi_interface_deferred_lines': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'adi_deferred_lines_apply': (c_int, [c_void_p, c_int, c_long, c_long, c_void_p, c_long, c_void_p, c_int, c_void_p, c_int,
                                         c_void_p, c_void_p]),
    'adi_step': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_pp, c_void_p, c_void_p,
                         c_void_pp, c_int, c_int, c_int, c_int, c_int, c_long, c_double, c_double, c_double, c_double,
                         c_double, c_double, c_double, c_double_p, c_void_p, c_size_t, c_void_p]),
    'adi_step_queued': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_pp, c_void_p, c_void_p,
                         c_void_pp, c_int, c_int, c_int, c_int, c_int, c_long, c_double, c_double, c_double, c_double,
                         c_double, c_double, c_double, c_double_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    'adi_step_bricks': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_pp, c_void_p, c_void_p,
                                c_void_pp, c_int, c_int, c_int, c_int, c_int, c_long, c_double, c_double, c_double, c_double,
                                c_double, c_double, c_double, c_double_p, c_void_p, c_size_t, c_void_p]),
    'adi_step_queued_bricks': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_pp, c_void_p, c_void_p,
                                       c_void_pp, c_int, c_int, c_int, c_int, c_int, c_long, c_double, c_double, c_double, c_double,
                                       c_double, c_double, c_double, c_double_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    'adi_morph6': (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'adi_flood_outside': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int_p, c_void_p]),
    'adi_pack_frame_f32be': (c_int, [c_void_p, c_int, c_int, c_int, c_long, c_void_p, c_void_p]),
    'adi_stlcorr_count': (c_int, [c_void_p, c_void_p, c_long, c_double, c_int, c_double, c_void_p, c_void_p]),
    'adi_stlcorr_bin': (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_long, c_void_p, c_int, c_int, c_int, c_long, c_long,
                                c_double_p, c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'adi_stlcorr_accumulate': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_double, c_double_p,
                                       c_void_pp, c_void_pp, c_void_pp, c_void_p]),
    'adi_stlcorr_fallback': (c_int, [c_void_p, c_int, c_int, c_int, c_long, c_long, c_int, c_double, c_void_p, c_void_p,
                                     c_void_p]),
    'adi_voxelize_words': (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(c_long)]),
    'adi_voxelize_count': (c_int, [c_void_p, c_long, c_double_p, c_double, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'adi_voxelize_toggle': (c_int, [c_void_p, c_void_p, c_long, c_long, c_double_p, c_double, c_int, c_int, c_int, c_int,
                                    c_void_p, c_void_p]),
    'adi_voxelize_scan': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'adi_voxelize_majority': (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    'adi_count_exposed_faces': (c_int, [c_void_p, c_int, c_int, c_int, c_long, c_int, c_void_p, c_void_p]),
    'adi_birth_planes': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_int, c_int, c_double, c_void_p,
                                 c_void_p]),
    'adi_copy_planes': (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_void_p]),
    'adi_masked_fill': (c_int, [c_void_p, c_void_p, c_size_t, c_double, c_void_p]),
    'adi_mask_or': (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'adi_cyl_plan_create': (c_int, [c_int, c_int, c_int, c_long, c_double, c_double, c_double, c_double, c_double, c_double,
                                    c_double, c_double, c_double, c_int, c_int, c_double, c_double, c_double,
                                    c_double, c_double, c_double, c_void_pp]),
    'adi_cyl_plan_create_annular': (c_int, [c_int, c_int, c_int, c_long, c_double, c_double, c_double, c_double, c_double, c_double,
                                            c_double, c_double, c_double, c_double, c_int, c_int, c_double, c_double, c_double,
                                            c_double, c_double, c_double, c_void_pp]),
    'adi_cyl_plan_tables': (c_int, [c_int, c_int, c_int, c_double, c_double, c_double, c_double, c_double, c_double,
                                    c_double, c_double, c_double, c_double, c_int, c_int, c_double, c_double, c_double,
                                    c_double, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_long]),
    'adi_cyl_plan_destroy': (c_int, [c_void_p]),
    'adi_cyl_step': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_double, c_double, c_void_p]),
    'adi_cyl_sweep': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_void_p]),
    'adi_source_sample': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_double, c_double, c_void_p, c_void_p]),
    'adi_source_set': (c_int, [c_void_p, c_void_p, c_double, c_double, ctypes.c_longlong, c_void_p]),
    'adi_source_tick': (c_int, [c_void_p, c_void_p]),
    'adi_source_lines0': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long,
                                  c_int, c_double, c_double, c_double, c_double, c_double, c_double, c_double_p, c_void_p,
                                  c_size_t, c_void_p]),
    'adi_source_lines0_slab': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                       c_long, c_int, c_int, c_double, c_double, c_double, c_double, c_double, c_double,
                                       c_double_p, c_void_p, c_size_t, c_void_p]),
    'adi_source_add_r0': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_int,
                                  c_int, c_int, c_double, c_double, c_double, c_double, c_void_p]),
    'adi_source_workspace_bytes': (c_int, [c_void_p, c_int, c_int, c_int, c_double, ctypes.POINTER(c_size_t)]),
    'adi_explicit_rhs_src': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_double, c_double, c_double,
                                     c_double, c_double, c_double, c_void_p, c_void_p]),
    'adi_scan_sample_host': (c_int, [c_void_p, c_void_p, c_int, c_double, c_void_p, c_int, c_int, c_int, c_double, c_double,
                                     c_double, c_void_p]),
    'adi_scan_sample': (c_int, [c_void_p, c_void_p, c_int, c_double, c_void_p, c_int, c_int, c_int, c_long, c_double, c_double,
                                c_double, c_void_p, c_void_p]),
    'adi_scan_window_box': (c_int, [c_void_p, c_void_p, c_int, c_double, c_int, c_int, c_int, c_double, c_double, c_double,
                                    c_int_p, c_int_p]),
    'adi_matmap_scan_add_r0': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                       c_int, c_long, c_double, c_double, c_double, c_int, c_double_p, c_int_p, c_void_p]),
    'adi_matmap_scan_add_r0_host': (c_int, [c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                            c_int, c_double, c_double, c_double, c_int, c_double_p, c_int_p]),
    'adi_bead_index_box': (c_int, [c_void_p, c_void_p, c_int, c_double, c_int, c_int, c_int, c_double, c_double, c_double,
                                   c_int_p, c_int_p]),
    'adi_bead_deposit_host': (c_int, [c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p, c_int, c_int, c_int, c_double,
                                      c_double, c_double, c_void_p]),
    'adi_bead_deposit': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                 c_int, c_int, c_int, c_int, c_long, c_double, c_double, c_double, c_double, c_void_p,
                                 c_void_p]),
    'adi_bead_deposit_ids': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_long, c_double, c_double, c_double,
                                     c_double, c_void_p, c_void_p]),
    'adi_surface_loss_update': (c_int, [c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_double,
                                        c_double, c_double, c_void_pp, c_int, c_int, c_int, c_void_p]),
    'adi_phase_summary_words': (ctypes.c_long, [c_int, c_int, c_int]),
    'adi_phase_apply': (c_int, [c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                c_int, c_long, c_void_p]),
    'adi_phase_seed': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                               c_long, c_void_p]),
    'adi_matlaw_theta': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_void_p]),
    'adi_matlaw_recover': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long,
                                   c_void_p]),
    'adi_matlaw_loss_update': (c_int, [c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long,
                                       c_double, c_double, c_double, c_void_pp, c_int, c_int, c_int, c_void_p]),
    'adi_history_record': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_int, c_int, c_int, c_long, c_void_p]),
    'adi_history_set_clock': (c_int, [c_void_p, c_double, c_double, c_void_p]),
    'adi_history_tick': (c_int, [c_void_p, c_void_p]),
    'adi_history_seed': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                 c_long, c_void_p]),
    'adi_history_reset_log': (c_int, [c_void_p, c_void_p, c_long, c_void_p]),
    'adi_solid_record': (c_int, [c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_void_p]),
    'adi_solid_seed': (c_int, [c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                               c_int, c_int, c_long, c_void_p]),
    'adi_monitor_record': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_int,
                                   c_int_p, c_int, c_int_p, c_void_p, c_int, c_double_p, c_void_p, c_long, c_void_p, c_long,
                                   c_void_p]),
    'adi_monitor_reset_log': (c_int, [c_void_p, c_void_p, c_long, c_long, c_void_p]),
    'adi_cyl_source_set': (c_int, [c_void_p, c_void_p, c_double, c_double, ctypes.c_longlong, c_void_p]),
    'adi_cyl_source_sample': (c_int, [c_void_p, c_int, c_int, c_int, c_long, c_double, c_double, c_double, c_double, c_double,
                                      c_void_p, c_void_p, c_void_p]),
    'adi_cyl_step_src': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_void_p]),
    'adi_cyl_sweep_src': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_void_p]),
    'adi_cyl_phase_apply': (c_int, [c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                    c_long, c_void_p]),
    'adi_cyl_phase_apply_host': (c_int, [c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                         c_int, c_long]),
    'adi_cyl_phase_seed': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_void_p]),
    'adi_cyl_history_record': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int, c_int, c_int, c_long, c_void_p]),
    'adi_cyl_history_record_host': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_int, c_int, c_int, c_long]),
    'adi_cyl_history_seed': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long,
                                     c_void_p]),
    'adi_cyl_history_reset_log': (c_int, [c_void_p, c_void_p, c_long, c_void_p]),
    'adi_cyl_monitor_record': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_double, c_double,
                                       c_int, c_int_p, c_int, c_int_p, c_void_p, c_void_p, c_long, c_void_p, c_long, c_void_p]),
    'adi_cyl_monitor_record_host': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_double,
                                            c_double, c_int, c_int_p, c_int, c_int_p, c_void_p, c_long]),
    'adi_cyl_monitor_reset_log': (c_int, [c_void_p, c_void_p, c_long, c_long, c_void_p]),
    'adi_cyl_solid_record': (c_int, [c_double, c_double, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_void_p]),
    'adi_cyl_solid_record_host': (c_int, [c_double, c_double, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                          c_long]),
    'adi_cyl_solid_hot_seed': (c_int, [c_double, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_void_p]),
    'adi_cyl_solid_hot_seed_host': (c_int, [c_double, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long]),
    'adi_matmap_build_coeffs': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_double, c_int, c_double_p,
                                        c_int_p, c_double_p, c_void_pp, c_int_p, c_double_p, c_void_pp, c_void_pp, c_void_pp,
                                        c_void_p]),
    'adi_matmap_build_coeffs_planes': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_double, c_int, c_double_p,
                                               c_int_p, c_double_p, c_void_pp, c_int_p, c_double_p, c_void_pp, c_void_pp,
                                               c_void_pp, c_int, c_int, c_void_p]),
    'adi_matmap_source_add_r0': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_double,
                                         c_double, c_int, c_double_p, c_void_p]),
    'adi_matmap_explicit': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_int, c_double_p,
                                    c_double_p, c_double, c_double, c_void_p, c_void_p]),
    'adi_matmap_workspace_bytes': (c_int, [c_int, c_int, c_int, c_int, c_long, ctypes.POINTER(c_size_t)]),
    'adi_matmap_sweep': (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                 c_int, c_int, c_long, c_int, c_double_p, c_double, c_double, c_double, c_void_p, c_void_p,
                                 c_size_t, c_void_p]),
    'adi_matmap_phase_apply': (c_int, [c_int, c_void_p, c_int_p, c_double_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_void_p]),
    'adi_matmap_phase_seed': (c_int, [c_int, c_void_p, c_int_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_void_p]),
    'adi_matmap_loss_table_bytes': (c_size_t, []),
    'adi_matmap_loss_table': (c_int, [c_int, c_void_p, c_double_p, c_double, c_void_p, c_size_t]),
    'adi_matmap_loss_update': (c_int, [c_void_p, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                       c_long, c_double, c_void_pp, c_int, c_int, c_int, c_void_p]),
    'adi_matmap_transition': (c_int, [c_int, c_int_p, c_double_p, c_void_p, c_int_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long,
                                      c_double, c_double_p, c_int_p, c_double_p, c_void_pp, c_int_p, c_double_p, c_void_pp,
                                      c_void_pp, c_void_pp, c_void_p]),
    'adi_matmap_brick_sets': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_void_p]),
    'adi_ctx_create': (c_int, [c_int, c_int, c_int, c_double, c_int, c_void_pp]),
    'adi_ctx_destroy': (c_int, [c_void_p]),
    'adi_ctx_set_mask': (c_int, [c_void_p, c_void_p]),
    'adi_ctx_build_coeffs': (c_int, [c_void_p, c_double, c_double, c_int_p, c_double_p, c_void_pp,
                                     c_int_p, c_double_p, c_void_pp, c_void_p, c_void_p]),
    'adi_ctx_upload_T': (c_int, [c_void_p, c_void_p]),
    'adi_ctx_download_T': (c_int, [c_void_p, c_void_p]),
    'adi_ctx_download_pack': (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    'adi_ctx_step': (c_int, [c_void_p, c_double, c_double, c_double, c_double, c_double, c_double, c_int]),
    'adi_ctx_last_step_ms': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_float)]),
}

MIXED_MIN_TG = 1e-9           # kMixedMinTg (csrc/adi_core.hpp): below this theta * gamma a sweep runs no FAST kernel
MAX_BOX_CELLS = 1 << 32       # ADI_MAX_BOX_CELLS: nx * plane_stride of a Cartesian box stays below it
SOURCE_BLOCK_BYTES = 128     # ADI_SOURCE_BLOCK_BYTES
SOURCE_E_CUT = 40.0          # ADI_SOURCE_E_CUT
CYL_ZCLOSURE_LEN = 11        # ADI_CYL_ZCLOSURE_LEN: f b0 bN aN c0 add0 addN T0 TN dir0 dirN
CYL_RF_MAXM = 16             # ADI_CYL_RF_MAXM
CYL_RF_STRIDE = 83           # ADI_CYL_RF_STRIDE: doubles per segment of the r FAST tables
SCAN_TABLE_COLS = 8         # ADI_SCAN_TABLE_COLS: { t_begin, p[3], d[2], speed, power }
SURFACE_LOSS_MAX_KNOTS = 16  # ADI_SURFACE_LOSS_MAX_KNOTS
SURFACE_LOSS_SIGMA = 5.670374419e-8   # ADI_SURFACE_LOSS_SIGMA (Stefan-Boltzmann, CODATA 2018)
MATLAW_MAX_KNOTS = 16        # ADI_MATLAW_MAX_KNOTS
MATMAP_MAX = 8               # ADI_MATMAP_MAX: materials per grid
HISTORY_BLOCK_BYTES = 40     # ADI_HISTORY_BLOCK_BYTES: { double t0, dt; int64 n, slot, capacity }
HISTORY_LOG_INTS = 8         # ADI_HISTORY_LOG_INTS: { cells, lo[3], hi[3], pad }
CYL_HISTORY_LOG_INTS = 12    # ADI_CYL_HISTORY_LOG_INTS: { cells, lo[3], hi[3], pad, int64 sum_i, pad, pad }
CYL_SOLID_TILE = 512         # ADI_CYL_SOLID_TILE: cells of a (phi, z) plane per hot word of the cylindrical solidification record
MONITOR_MAX_REGIONS = 8      # ADI_MONITOR_MAX_REGIONS
MONITOR_MAX_PROBES = 256     # ADI_MONITOR_MAX_PROBES
MONITOR_REGION_WORDS = 6     # ADI_MONITOR_REGION_WORDS: { cells, T_min, T_max, sum_T, sum_wT, sum_extra }
MONITOR_PARTIAL_WORDS = 6    # ADI_MONITOR_PARTIAL_WORDS
CYL_MONITOR_REGION_WORDS = 8   # ADI_CYL_MONITOR_REGION_WORDS: { cells, sum_i, T_min, T_max, sum_T, sum_rT, sum_extra, sum_rextra }
CYL_MONITOR_PARTIAL_WORDS = 5  # ADI_CYL_MONITOR_PARTIAL_WORDS
BRICK = 16                # kBrick (csrc/adi_cart_dev.hpp): the edge of a brick of the flags summary
STLCORR_DROPPED = (1 << 63) - 1   # ADI_STLCORR_DROPPED
STLCORR_MAX_SUBDIV = 4096    # ADI_STLCORR_MAX_SUBDIV


class HeatSource(ctypes.Structure):
    """adi_heat_source (include/adi_hip.h)"""
    _fields_ = [('power', c_double), ('eta', c_double), ('a', c_double), ('b', c_double), ('c_f', c_double),
                ('c_r', c_double), ('f_f', c_double), ('origin', c_double * 3), ('velocity', c_double),
                ('travel_axis', c_int), ('travel_sign', c_int), ('depth_axis', c_int), ('reserved', c_int)]


class ScanShape(ctypes.Structure):
    """adi_scan_shape (include/adi_hip.h)"""
    _fields_ = [('eta', c_double), ('a', c_double), ('b', c_double), ('c_f', c_double), ('c_r', c_double), ('f_f', c_double),
                ('depth_axis', c_int), ('reserved', c_int)]


BEAD_PROFILES = {'box': 0, 'parabola': 1}   # adi_bead_shape.profile


class BeadShape(ctypes.Structure):
    """adi_bead_shape (include/adi_hip.h)"""
    _fields_ = [('width', c_double), ('height', c_double), ('profile', c_int), ('depth_axis', c_int)]


class SurfaceLossLaw(ctypes.Structure):
    """adi_surface_loss (include/adi_hip.h)"""
    _fields_ = [('h', c_double * 6), ('emissivity', c_double * 6), ('T_offset', c_double), ('n_knots', c_int),
                ('reserved', c_int), ('knot_T', c_double * 16), ('knot_h', c_double * 16)]


class PhaseChangeLaw(ctypes.Structure):
    """adi_phase_change (include/adi_hip.h)"""
    _fields_ = [('latent_heat', c_double), ('T_solidus', c_double), ('T_liquidus', c_double)]


class MaterialLawC(ctypes.Structure):
    """adi_material_law (include/adi_hip.h)"""
    _fields_ = [('n_knots', c_int), ('reserved', c_int), ('k_ref', c_double), ('cp_ref', c_double), ('c_lo', c_double)] + [
        (name, c_double * 16) for name in ('x', 'kq', 'hks', 'ks2', 'theta', 'c', 'hcs', 'cs2', 'H')]


class HistoryLevelsC(ctypes.Structure):
    """adi_history_levels (include/adi_hip.h)"""
    _fields_ = [('T_hi', c_double), ('T_lo', c_double), ('T_melt', c_double)]


CYL_DEPTHS = {'z': 0, 'r': 1}   # ADI_CYL_DEPTH_Z, ADI_CYL_DEPTH_R


class CylHeatSource(ctypes.Structure):
    """adi_cyl_heat_source (include/adi_hip.h)"""
    _fields_ = [('power', c_double), ('eta', c_double), ('a', c_double), ('b', c_double), ('c_f', c_double),
                ('c_r', c_double), ('f_f', c_double), ('r_c', c_double), ('phi0', c_double), ('omega', c_double),
                ('z0', c_double), ('v_z', c_double), ('depth', c_int), ('reserved', c_int)]


for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)   # AttributeError here = the .so does not export what the header declares
    _fn.restype = _res
    _fn.argtypes = _args


class AdiError(RuntimeError):
    pass


class AdiArgError(AdiError, ValueError):
    """ADI_ERR_ARG: the ValueError the reference would have raised, and -- like every status of the library -- an AdiError"""


def last_error():
    msg = lib.adi_last_error()
    return msg.decode('utf-8', 'replace') if msg else ''


def check(rc):
    """Map a C-ABI status to the exception the reference would have raised."""
    if rc == ADI_OK:
        return
    msg = last_error()
    if rc == ADI_ERR_ARG:
        raise AdiArgError(msg)         # e.g. ValueError("bad face"), adi3d_numba_coeff.py:54
    raise AdiError('libadi_hip error %d: %s' % (rc, msg))


def ptr_array(ptrs):
    arr = (c_void_p * len(ptrs))()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr
