"""ctypes binding of libmundy_hip.so (include/mundy_hip.h).  Plumbing only: torch supplies device memory and the
current HIP stream; every computation happens in the hand-written HIP library.  There is no CPU fallback: if the
library is missing `load()` raises, and on a box without a GPU every compute entry point fails in HIP.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmundy_hip.so")

SUCCESS, ERR_INVALID_ARGUMENT, ERR_LOGIC, ERR_RUNTIME, ERR_HIP, ERR_NO_DEVICE = range(6)
SEARCH_SPHERES, SEARCH_AABB = 0, 1
SEARCH_METHOD_AUTO, SEARCH_METHOD_GRID, SEARCH_METHOD_MORTON_LBVH = 0, 1, 2
SPACE_UNCONSTRAINED, SPACE_LOWER_BOUND, SPACE_UPPER_BOUND, SPACE_BOUNDED = 0, 1, 2, 3
RESIDUAL_PROJECTED_DIFF, RESIDUAL_PROJECTED_GRADIENT = 0, 1
SPRING_HOOKEAN, SPRING_FENE, SPRING_FENEWCA = 0, 1, 2
PERIPHERY_SPHERE, PERIPHERY_ELLIPSOID, PERIPHERY_ELLIPSOID_FAST = 0, 1, 2
HYDRO_STOKES, HYDRO_RPY, HYDRO_RPYC = 0, 1, 2
HYDRO_CHUNK = 1024  # MHIP_HYDRO_CHUNK: the width of the summation order's chunks
HYDRO_PATH_AUTO, HYDRO_PATH_IN_LANE, HYDRO_PATH_PARTIAL = 0, 1, 2


class MhipError(RuntimeError):
    """HIP runtime failure or missing device (MHIP_ERR_HIP / MHIP_ERR_NO_DEVICE)."""


class BroadphaseConfig(C.Structure):
    _fields_ = [("search_kind", C.c_int), ("symmetric", C.c_int), ("buffer", C.c_double), ("periodic", C.c_int),
                ("box", C.c_double * 3), ("method", C.c_int), ("include_self", C.c_int), ("cell", C.c_double * 9)]


class Space(C.Structure):
    _fields_ = [("kind", C.c_int), ("lower_bound", C.c_double), ("upper_bound", C.c_double)]


class PgdConfig(C.Structure):
    _fields_ = [("max_iters", C.c_uint), ("tol", C.c_double), ("residual_kind", C.c_int)]


class SolveResult(C.Structure):
    _fields_ = [("num_iters", C.c_uint), ("residual", C.c_double), ("converged", C.c_int)]


class HertzFrictionParams(C.Structure):
    _fields_ = [("mu", C.c_double), ("normal_damping", C.c_double), ("tangential_damping", C.c_double),
                ("density", C.c_double), ("dt", C.c_double)]


class Periphery(C.Structure):
    _fields_ = [("shape", C.c_int), ("center", C.c_double * 3), ("quat", C.c_double * 4), ("radii", C.c_double * 3),
                ("k", C.c_double)]


class FilamentParams(C.Structure):
    _fields_ = [("youngs_modulus", C.c_double), ("poisson_ratio", C.c_double), ("rest_length", C.c_double),
                ("viscosity", C.c_double), ("wave_amplitude", C.c_double), ("wave_number", C.c_double),
                ("wave_frequency", C.c_double), ("wave", C.c_int), ("disable_twist", C.c_int), ("monolayer", C.c_int)]


FILAMENT_FIELDS = ("center", "twist", "velocity", "twist_velocity", "force", "twist_torque", "radius", "rest_curvature",
                   "arclength", "curvature", "phase", "edge_tangent", "edge_orientation", "edge_length", "edge_binormal",
                   "edge_tangent_old", "edge_orientation_old", "edge_length_old", "edge_binormal_old")


class FilamentFields(C.Structure):
    _fields_ = [("num_nodes", C.c_size_t), ("num_filaments", C.c_size_t)] + [(f, C.c_void_p) for f in FILAMENT_FIELDS]


class FilamentInertialParams(C.Structure):
    """mhip_filament_inertial_params (include/mundy_hip_filament_inertial.h)"""
    _fields_ = [("density", C.c_double), ("damping_kind", C.c_int), ("translational_damping", C.c_double),
                ("twist_damping", C.c_double)]


class FilamentInertialFields(C.Structure):
    _fields_ = [("acceleration", C.c_void_p), ("twist_acceleration", C.c_void_p)]


class FilamentContactParams(C.Structure):
    _fields_ = [("skin", C.c_double), ("youngs_modulus", C.c_double), ("poisson_ratio", C.c_double), ("mu", C.c_double),
                ("normal_damping", C.c_double), ("tangential_damping", C.c_double), ("density", C.c_double),
                ("history_dt", C.c_double), ("bonded_exclusion", C.c_int), ("monolayer", C.c_int)]


# mhip_filament_contact_fields: name -> columns; pairs (int32) .. share have num_pairs rows, the rest num_nodes
FILAMENT_CONTACT_FIELDS = {"pairs": 2, "sep": 1, "tang_disp": 3, "force": 3, "share": 6, "node_force": 3, "seg": 8,
                           "aabb": 6, "velocity_prev": 3}


class FilamentContactFields(C.Structure):
    _fields_ = [("num_nodes", C.c_size_t), ("num_pairs", C.c_size_t)] + [(f, C.c_void_p)
                                                                         for f in FILAMENT_CONTACT_FIELDS]


class SegmentContactParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("skin", C.c_double), ("youngs_modulus", C.c_double), ("poisson_ratio", C.c_double),
                ("epsilon", C.c_double), ("sigma", C.c_double), ("cutoff", C.c_double)]


# mhip_segment_contact_fields: name -> columns; pairs (int32) .. share have num_pairs rows, seg and aabb num_segments
SEGMENT_CONTACT_FIELDS = {"pairs": 2, "sep": 1, "force": 3, "share": 6, "seg": 8, "aabb": 6}


class SegmentContactFields(C.Structure):
    _fields_ = [("num_bodies", C.c_size_t), ("num_segments", C.c_size_t),
                ("num_pairs", C.c_size_t)] + [(f, C.c_void_p) for f in SEGMENT_CONTACT_FIELDS]


class VelocityHalo(C.Structure):
    """mhip_velocity_halo: the per-iteration ghost-velocity exchange of one rank (host lists + one device index list)"""
    _fields_ = [("velocity", C.c_void_p), ("num_send_peers", C.c_int), ("send_peer", C.POINTER(C.c_int)),
                ("send_rows", C.POINTER(C.c_size_t)), ("send_index", C.c_void_p), ("num_recv_peers", C.c_int),
                ("recv_peer", C.POINTER(C.c_int)), ("recv_first_row", C.POINTER(C.c_size_t)),
                ("recv_rows", C.POINTER(C.c_size_t))]


class GhostLayout(C.Structure):
    _fields_ = [("num_ghost_lo", C.c_size_t), ("num_owned", C.c_size_t), ("num_ghost_hi", C.c_size_t),
                ("num_sent", C.c_size_t), ("halo", VelocityHalo)]


class DistProfile(C.Structure):
    _fields_ = [("body_ms", C.c_double), ("constraint_ms", C.c_double), ("halo_wait_ms", C.c_double),
                ("timed_iterations", C.c_size_t), ("halo_post_ms", C.c_double), ("record_ms", C.c_double),
                ("halo_path", C.c_int), ("record_path", C.c_int)]


# host-callback transport (mhip_comm_create_host): device pointers arrive as integers
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                          C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                          C.POINTER(C.c_size_t))
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
COMM_ID_BYTES = 128

_vp, _sz, _d, _i = C.c_void_p, C.c_size_t, C.c_double, C.c_int

# name -> argtypes; every function returns int status.  Must list every symbol include/mundy_hip.h declares
# (tests/test_capi_symbols.py checks the header against this table and against the built library).
SIGNATURES = {
    "mhip_device_info": [C.POINTER(C.c_int), C.c_char_p, _sz],
    "mhip_malloc": [C.POINTER(_vp), _sz],
    "mhip_free": [_vp],
    "mhip_memory_stats": [C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz)],
    "mhip_memcpy_h2d": [_vp, _vp, _sz, _vp],
    "mhip_memcpy_d2h": [_vp, _vp, _sz, _vp],
    "mhip_stream_synchronize": [_vp],
    "mhip_compute_aabb_spheres": [_sz, _vp, _vp, _vp, _vp],
    "mhip_compute_aabb_spherocylinders": [_sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "mhip_compute_aabb_ellipsoids": [_sz, _vp, _vp, _vp, _vp, _vp],
    "mhip_compute_aabb_ellipsoids_conservative": [_sz, _vp, _vp, _vp, _vp, _vp],
    "mhip_compute_aabb_segments": [_sz, _vp, _vp, _vp],
    "mhip_bounding_radius_spherocylinders": [_sz, _vp, _vp, _vp, _vp],
    "mhip_bounding_radius_ellipsoids": [_sz, _vp, _vp, _vp],
    "mhip_spherocylinder_segments": [_sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "mhip_distance_sphere_sphere": [_sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mhip_distance_point_segment": [_sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mhip_distance_point_sphere": [_sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "mhip_distance_segment_sphere": [_sz] + [_vp] * 9,
    "mhip_distance_segment_segment": [_sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mhip_distance_ellipsoid_ellipsoid": [_sz] + [_vp] * 12,
    "mhip_distance_point_ellipsoid": [_sz] + [_vp] * 8,
    "mhip_contact_ellipsoids": [_sz] + [_vp] * 11,
    "mhip_compute_aabb_mixed": [_sz] + [_vp] * 7,
    "mhip_compute_aabb_mixed_conservative": [_sz] + [_vp] * 7,
    "mhip_contact_mixed": [_sz] + [_vp] * 11 + [C.POINTER(_sz), _vp],
    "mhip_contact_mixed_set_contraction": [_i],
    "mhip_contact_mixed_set_sphere_ellipsoid_route": [_i],
    "mhip_contact_mixed_last_evaluations": [C.POINTER(C.c_ulonglong), _vp],
    "mhip_ellipsoid_last_evaluations": [C.POINTER(C.c_ulonglong), _vp],
    "mhip_contact_mixed_periodic": [_sz] + [_vp] * 5 + [C.POINTER(_d)] + [_vp] * 6 + [C.POINTER(_sz), _vp],
    "mhip_contact_spherocylinders_periodic": [_sz, _vp, _vp, _vp, C.POINTER(_d)] + [_vp] * 9,
    "mhip_hertz_contact_force": [_sz, _sz, _vp, _vp, _vp, _vp, _d, _vp, _d, _vp, _vp, _vp],
    "mhip_hertz_friction_force": [_sz, _sz] + [_vp] * 8 + [_d, _vp, _d, _vp, C.POINTER(HertzFrictionParams), _vp, _vp, _vp,
                                  _vp],
    "mhip_contact_history_carry": [_sz, _vp, _vp, _vp, _sz, _sz, _vp, _vp, C.POINTER(_sz), _vp],
    "mhip_select_dividing": [_sz, _vp, _d, _vp, C.POINTER(_sz), _vp],
    "mhip_divide_grow_spherocylinders": [_sz, _sz, _vp, _d, _d, C.POINTER(_d), _vp, _vp, _vp, _vp, _vp],
    "mhip_aabb_moved": [_sz, _vp, _vp, _d, C.POINTER(_i), _vp],
    "mhip_springs_create": [C.POINTER(_vp), _sz, _sz, _vp, _i, _vp, _d, _vp, _d, _vp],
    "mhip_springs_force": [_vp, _vp, _vp, _vp, _vp, _vp],
    "mhip_springs_destroy": [_vp],
    "mhip_crosslinkers_create": [C.POINTER(_vp), _sz, _sz, _vp, _vp, _vp, _i, _d, _d, _d, _d, _d, _d, _vp],
    "mhip_crosslinkers_set_candidates": [_vp, _vp, _vp, _sz, _vp, _vp],
    "mhip_crosslinkers_kmc_step": [_vp, _vp, _d, _vp, _vp, _vp, _vp, _vp],
    "mhip_crosslinkers_force": [_vp, _vp, _vp, _i, _vp, _vp, _vp],
    "mhip_crosslinkers_get_state": [_vp, _vp, _vp, _vp],
    "mhip_crosslinkers_set_state": [_vp, _vp, _vp, _vp],
    "mhip_crosslinkers_renumber": [_vp, _vp, _vp],
    "mhip_crosslinkers_destroy": [_vp],
    "mhip_periphery_force": [C.POINTER(Periphery), _sz, _vp, _vp, _vp, _i, _vp, _vp, _vp],
    "mhip_active_springs_create": [C.POINTER(_vp), _sz, _sz, _vp, _d, _d, _d, _vp, _vp, _vp],
    "mhip_active_springs_sample": [_vp, _vp, _vp],
    "mhip_active_springs_force": [_vp, _vp, _vp, _i, _vp, _vp],
    "mhip_active_springs_advance": [_vp, _d, _vp],
    "mhip_active_springs_get_state": [_vp, _vp, _vp, _vp, _vp, _vp],
    "mhip_active_springs_set_state": [_vp, _vp, _vp, _vp, _vp, _vp],
    "mhip_active_springs_renumber": [_vp, _vp, _vp],
    "mhip_active_springs_destroy": [_vp],
    "mhip_filaments_create": [C.POINTER(_vp), _sz, _vp, _vp, _vp, _vp, _vp, C.POINTER(FilamentParams), _vp],
    "mhip_filaments_set_state": [_vp, _vp, _vp, _vp],
    "mhip_filaments_advance": [_vp, _d],
    "mhip_filaments_force": [_vp, _d, _vp, _vp],
    "mhip_filaments_edge_pass": [_vp],
    "mhip_filaments_node_pass": [_vp, _d, _vp, _vp],
    "mhip_filaments_velocity": [_vp],
    "mhip_filaments_get": [_vp, C.POINTER(FilamentFields)],
    "mhip_filaments_destroy": [_vp],
    "mhip_filament_contacts_create": [C.POINTER(_vp), _vp, _vp, _vp, C.POINTER(FilamentContactParams), _vp],
    "mhip_filament_contacts_save_velocity": [_vp],
    "mhip_filament_contacts_update": [_vp, C.POINTER(_i)],
    "mhip_filament_contacts_force": [_vp, _d, _vp, _vp],
    "mhip_filament_contacts_segment_view": [_vp],
    "mhip_filament_contacts_linker_pass": [_vp, _d, _vp],
    "mhip_filament_contacts_reduce": [_vp, _vp],
    "mhip_filament_contacts_set_history": [_vp, _sz, _vp, _vp],
    "mhip_filament_contacts_get": [_vp, C.POINTER(FilamentContactFields)],
    "mhip_filament_contacts_destroy": [_vp],
    "mhip_philox4x32_10": [_sz, _vp, _vp, C.c_uint32, _vp, _vp],
    "mhip_brownian_velocity": [_sz, _vp, _vp, _d, _d, _vp, _vp, _vp],
    "mhip_drag_velocity": [_sz, _vp, _vp, _vp, _vp],
    "mhip_hydro_create": [C.POINTER(_vp)],
    "mhip_hydro_destroy": [_vp],
    "mhip_hydro_set_path": [_vp, _i],
    "mhip_hydro_last_path": [_vp, C.POINTER(_i)],
    "mhip_hydro_velocity": [_vp, _i, _d, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _i, _i, _vp],
    "mhip_hydro_add_velocity": [_sz, _vp, _vp, _i, _vp],
    "mhip_contact_spheres": [_sz, _vp, _vp, _vp, C.POINTER(_d), _vp, _vp, _vp],
    "mhip_contact_spherocylinders": [_sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mhip_broadphase_create": [C.POINTER(_vp)],
    "mhip_broadphase_destroy": [_vp],
    "mhip_broadphase_build": [_vp, C.POINTER(BroadphaseConfig), _sz, _vp, _vp, _vp, C.POINTER(_sz), _vp],
    "mhip_broadphase_get_pairs": [_vp, _vp, _vp, _vp, _vp],
    "mhip_broadphase_needs_rebuild": [_vp, _sz, _vp, C.POINTER(_i), _vp],
    "mhip_select_contacts": [_sz, _vp, _d, _vp, C.POINTER(_sz), _vp],
    "mhip_curve_keys": [_sz, _vp, C.POINTER(_d), C.POINTER(_d), _i, _vp, _vp, _vp],
    "mhip_sort_by_key_u64": [_sz, _vp, _vp, _vp],
    "mhip_broadphase_set_sets": [_vp, _sz, _vp, _vp, _vp],
    "mhip_broadphase_set_exclusions": [_vp, _sz, _vp, _vp, _sz, _vp],
    "mhip_broadphase_set_identities": [_vp, _sz, _vp, _vp, _vp],
    "mhip_broadphase_get_ident_pairs": [_vp, _vp, _vp, _vp, _vp, _vp],
    "mhip_broadphase_method_used": [_vp, C.POINTER(_i)],
    "mhip_broadphase_minimum_image_complete": [_vp, C.POINTER(_i)],
    "mhip_links_export_coo": [_vp, C.c_uint64, _i, _i, _vp, _vp, _vp, _vp],
    "mhip_links_export_crs": [_vp, C.c_uint64, C.c_uint, _vp, _vp, _vp, _vp, _vp],
    "mhip_deep_copy": [_sz, _vp, _vp, _vp],
    "mhip_fill": [_sz, _vp, _d, _vp],
    "mhip_axpby": [_sz, _d, _vp, _d, _vp, _vp],
    "mhip_wrapped_axpbyz": [_sz, _d, _vp, _d, _vp, _vp, C.POINTER(Space), _vp],
    "mhip_diff_dot2": [_sz, _vp, _vp, C.POINTER(_d), _vp],
    "mhip_diff_dot4": [_sz, _vp, _vp, _vp, _vp, C.POINTER(_d), _vp],
    "mhip_residual": [_sz, _i, _vp, _vp, C.POINTER(Space), C.POINTER(_d), _vp],
    "mhip_bb_step": [_sz, _vp, _vp, _vp, _vp, C.POINTER(_d), _vp],
    "mhip_gemv": [_sz, _vp, _vp, _vp, _vp],
    "mhip_contact_op_create": [C.POINTER(_vp), _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _d, _vp, _vp],
    "mhip_contact_op_create_rods": [C.POINTER(_vp), _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _d, _vp, _vp],
    "mhip_contact_op_refresh": [_vp, _vp, _vp, _vp, _vp],
    "mhip_contact_op_refresh_rods": [_vp, _vp, _vp, _vp, _vp, _vp],
    "mhip_contact_op_destroy": [_vp],
    "mhip_contact_op_apply": [_vp, _vp, _vp, _vp],
    "mhip_contact_op_body_sweep": [_vp, _vp, _vp],
    "mhip_contact_op_body_sweep_vector": [_vp, _vp, _vp],
    "mhip_contact_op_constraint_rate": [_vp, _vp, _vp, _vp],
    "mhip_contact_op_body_velocity": [_vp, C.POINTER(_vp)],
    "mhip_contact_op_set_profiling": [_vp, _i],
    "mhip_contact_op_set_tiering": [_vp, _i],
    "mhip_contact_op_tier_stats": [_vp, C.POINTER(_sz), C.POINTER(_d), C.POINTER(_sz), C.POINTER(_sz)],
    "mhip_contact_op_set_work_mapping": [_vp, _i, _i],
    "mhip_bbpgd_stage_snapshot_active": [_vp, _vp],
    "mhip_contact_op_get_profile": [_vp, C.POINTER(_d), C.POINTER(_d), C.POINTER(_sz)],
    "mhip_bbpgd_solve_dense": [_sz, _vp, _vp, C.POINTER(Space), C.POINTER(PgdConfig), _vp, _vp, _vp, _vp,
                               C.POINTER(SolveResult), _vp],
    "mhip_bbpgd_solve_contact": [_vp, _vp, C.POINTER(Space), C.POINTER(PgdConfig), _vp, _vp, _vp, _vp,
                                 C.POINTER(SolveResult), _vp],
    "mhip_bbpgd_solve_contact_friction": [_vp, _vp, _d, C.POINTER(PgdConfig), _vp, _vp, C.POINTER(SolveResult), _vp],
    "mhip_apgd_solve_contact_friction": [_vp, _vp, _d, C.POINTER(PgdConfig), _vp, _vp, C.POINTER(SolveResult), _vp],
    "mhip_solve_small_cqpp_batch": [_sz, _i, _vp, _vp, C.POINTER(Space), C.POINTER(PgdConfig), _vp, _vp, _vp, _vp,
                                    _vp, _vp],
    "mhip_scrap_bbpgd_solve_contact": [_vp, _vp, _d, C.c_uint, _vp, _vp, _vp, _vp, C.POINTER(SolveResult),
                                       C.POINTER(_d), _vp],
    "mhip_contact_op_set_partition": [_vp, _sz, _sz, _vp, _vp],
    "mhip_bbpgd_stage_begin": [_vp, _vp, C.POINTER(Space), C.POINTER(PgdConfig), _vp, _vp, _vp, _vp, _vp],
    "mhip_bbpgd_stage_body": [_vp, _i, _vp],
    "mhip_bbpgd_stage_constraint": [_vp, _i, _vp, _vp],
    "mhip_bbpgd_stage_constraint_range": [_vp, _i, _sz, _sz, _vp],
    "mhip_bbpgd_stage_reduce": [_vp, _i, _vp, _vp],
    "mhip_bbpgd_stage_finalize": [_vp, _i, _vp, _i, _vp],
    "mhip_bbpgd_stage_poll": [_vp, C.POINTER(SolveResult), C.POINTER(_i), _vp],
    "mhip_bbpgd_stage_end": [_vp, C.POINTER(SolveResult), _vp],
    "mhip_filter_pairs_owned": [_sz, _vp, _sz, _sz, _vp, _vp, C.POINTER(_sz), _vp],
    "mhip_partition_pairs_owned": [_sz, _vp, _sz, _sz, _vp, _vp, C.POINTER(_sz), C.POINTER(_sz), _vp],
    "mhip_select_aabb_overlap": [_sz, _vp, _d, C.POINTER(_d), _vp, C.POINTER(_sz), _vp],
    "mhip_aabb_chunk_bounds": [_sz, _vp, _d, _i, _vp, _vp],
    "mhip_select_aabb_overlap_any": [_sz, _vp, _d, _i, _vp, _vp, C.POINTER(_sz), _vp],
    "mhip_aabb_bounds": [_sz, _vp, _d, C.POINTER(_d), _vp],
    "mhip_bbpgd_solve_contact_unfused": [_vp, _vp, C.POINTER(Space), C.POINTER(PgdConfig), _vp, _vp, _vp, _vp,
                                         C.POINTER(SolveResult), _vp],
    "mhip_periodic_sep": [_sz, C.POINTER(_d), _vp, _vp, _vp, _vp],
    "mhip_wrap_rigid": [_sz, C.POINTER(_d), _vp, _vp],
    "mhip_unit_cell_inverse": [C.POINTER(_d), C.POINTER(_d)],
    "mhip_periodic_sep_triclinic": [_sz, C.POINTER(_d), _vp, _vp, _vp, _vp],
    "mhip_wrap_rigid_triclinic": [_sz, C.POINTER(_d), _vp, _vp],
    "mhip_shift_image_triclinic": [_sz, C.POINTER(_d), _vp, _vp, _vp, _vp],
    "mhip_contact_spheres_triclinic": [_sz, _vp, _vp, _vp, C.POINTER(_d), _vp, _vp, _vp],
    "mhip_integrate_euler": [_sz, _d, _vp, _vp, _vp, _vp],
    "mhip_morton_order": [_sz, _vp, C.POINTER(_d), _d, _vp, _vp],
    "mhip_set_tracing": [_i],
    "mhip_curve_order": [_sz, _vp, C.POINTER(_d), C.POINTER(_d), _i, _vp, _vp, _vp],
    "mhip_gather_rows": [_sz, _sz, _vp, _vp, _vp, _vp],
    "mhip_copy_strided": [_sz, _sz, _vp, _sz, _vp, _sz, _vp],
    "mhip_contact_op_sizes": [_vp, C.POINTER(_sz), C.POINTER(_sz)],
    "mhip_contact_op_set_drift_source": [_vp, _i],
    "mhip_contact_op_get_drift_source": [_vp, C.POINTER(_i)],
    "mhip_comm_unique_id": [C.c_char_p],
    "mhip_comm_create_rccl": [C.POINTER(_vp), C.c_char_p, _i, _i],
    "mhip_comm_create_host": [C.POINTER(_vp), _i, _i, EXCHANGE_FN, ALL_GATHER_FN, _vp],
    "mhip_comm_destroy": [_vp],
    "mhip_comm_info": [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)],
    "mhip_comm_mailbox_open": [_vp, C.POINTER(_i), _vp],
    "mhip_comm_mailbox_close": [_vp],
    "mhip_comm_halo_ipc_enable": [_vp, _i],
    "mhip_comm_set_exchange_timeout": [_vp, C.c_double],
    "mhip_comm_inject_fault": [_vp, C.c_uint],
    "mhip_comm_halo_ipc_active": [_vp, C.POINTER(_i)],
    "mhip_comm_all_gather": [_vp, _vp, _sz, _vp, _vp],
    "mhip_comm_exchange_start": [_vp, _i, C.POINTER(_i), C.POINTER(_vp), C.POINTER(_sz), _i, C.POINTER(_i),
                                 C.POINTER(_vp), C.POINTER(_sz), _vp],
    "mhip_comm_exchange_finish": [_vp, _vp],
    "mhip_ghost_layout_from_counts": [_i, _i, _sz, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_i),
                                      C.POINTER(_i), C.POINTER(_sz), C.POINTER(_i), C.POINTER(_i), C.POINTER(_sz),
                                      C.POINTER(_sz)],
    "mhip_ghost_plan": [_vp, _sz, _vp, _d, C.POINTER(GhostLayout), _vp],
    "mhip_ghost_exchange": [_vp, _sz, _vp, _vp, _vp],
    "mhip_hilbert_key_table": [_i, _vp],
    "mhip_body_work_weights": [_sz, _vp, _sz, _sz, _vp, _vp],
    "mhip_compose_keys_u64": [_sz, _vp, _vp, _i, _vp, _vp],
    "mhip_fill_sequence": [_sz, _d, _vp, _vp],
    "mhip_curve_cut": [_vp, _sz, _vp, _vp, _sz, _vp, _vp],
    "mhip_migrate_plan": [_vp, _sz, _vp, _vp, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz), _vp],
    "mhip_migrate_exchange": [_vp, _sz, _vp, _vp, _vp],
    "mhip_bbpgd_solve_contact_distributed": [_vp, _vp, C.POINTER(VelocityHalo), _sz, _vp, C.POINTER(Space),
                                             C.POINTER(PgdConfig), _vp, _vp, _vp, _vp, C.c_uint,
                                             C.POINTER(SolveResult), C.POINTER(DistProfile), _vp],
}
# include/mundy_hip_hydro_periphery.h, a header of its own (its first comment says why): name -> argtypes, every
# function returns int status.  tests/test_hydro_periphery_host.py checks this table against that header and the library.
HYDRO_PERIPHERY_EMPTY, HYDRO_PERIPHERY_MATRIX, HYDRO_PERIPHERY_INVERSE, HYDRO_PERIPHERY_DOUBLE_LAYER = 0, 1, 2, 3
PERIPHERY_SIGNATURES = {
    "mhip_hydro_periphery_create": [C.POINTER(_vp), _sz, _vp, _vp, _vp, _d, _vp],
    "mhip_hydro_periphery_destroy": [_vp],
    "mhip_hydro_periphery_fill_double_layer": [_vp, _vp],
    "mhip_hydro_periphery_fill_matrix": [_vp, _vp],
    "mhip_hydro_periphery_set_matrix": [_vp, _vp, _vp],
    "mhip_hydro_periphery_invert": [_vp, C.POINTER(_d), _vp],
    "mhip_hydro_periphery_set_inverse": [_vp, _vp, _vp],
    "mhip_hydro_periphery_matrix": [_vp, C.POINTER(_vp), C.POINTER(_i)],
    "mhip_hydro_periphery_surface_forces": [_vp, _vp, _vp, _vp],
    "mhip_hydro_double_layer": [_vp, _d, _sz, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _i, _i, _i, _vp],
    "mhip_hydro_periphery_correct": [_vp, _vp, _i, _sz, _vp, _vp, _vp, _vp, _i, _i, _vp],
}
# include/mundy_hip_contact_force.h, a header of its own for the same reason: name -> argtypes, every function returns int
# status.  tests/test_contact_force_host.py checks this table against that header and the library.
CONTACT_FORCE_SIGNATURES = {
    "mhip_contact_op_body_force": [_vp, _vp, _vp, _i, _i, _vp],
    "mhip_contact_op_body_force_vector": [_vp, _vp, _vp, _i, _i, _vp],
}
# include/mundy_hip_periphery_binding.h, a header of its own for the same reason: name -> argtypes, every function returns
# int status.  tests/test_periphery_binding_host.py checks this table against that header and the library.
PERIPHERY_BINDING_SIGNATURES = {
    "mhip_crosslinkers_set_periphery_sites": [_vp, _sz, _vp, _d, _d, _d, _d, _d, _vp],
    "mhip_crosslinkers_set_periphery_candidates": [_vp, _vp, _vp, _sz, C.c_int32, _vp],
    "mhip_crosslinkers_kmc_step_periphery": [_vp, _vp, _d, _vp, _vp, _vp, _vp, _vp, _vp],
}
# include/mundy_hip_segment_contact.h, a header of its own for the same reason: name -> argtypes, every function returns
# int status.  tests/test_segment_contact_host.py checks this table against that header and the library.
SEGMENT_CONTACT_HERTZ, SEGMENT_CONTACT_WCA = 0, 1
SEGMENT_CONTACT_SIGNATURES = {
    "mhip_segment_contacts_create": [C.POINTER(_vp), _sz, _sz, _vp, _vp, _d, _vp, C.POINTER(SegmentContactParams), _vp],
    "mhip_segment_contacts_destroy": [_vp],
    "mhip_segment_contacts_update": [_vp, _vp, _i, C.POINTER(_i), _vp],
    "mhip_segment_contacts_force": [_vp, _vp, _vp, _i, _vp, _vp],
    "mhip_segment_contacts_linker_pass": [_vp, _vp, _vp],
    "mhip_segment_contacts_reduce": [_vp, _vp, _i, _vp, _vp],
    "mhip_segment_contacts_get": [_vp, C.POINTER(SegmentContactFields)],
}
# include/mundy_hip_hydro_solve.h, a header of its own for the same reason: name -> argtypes, every function returns int
# status.  tests/test_hydro_solve_host.py checks this table against that header and the library.
class HydroMobility(C.Structure):
    """mhip_hydro_mobility: M_h without its dry part (workspace, kind, viscosity, n, center, radius, periphery, skip)"""
    _fields_ = [("workspace", C.c_void_p), ("kind", C.c_int), ("viscosity", C.c_double), ("n", C.c_size_t),
                ("center", C.c_void_p), ("radius", C.c_void_p), ("periphery", C.c_void_p), ("skip_same_index", C.c_int)]


HYDRO_SOLVE_SIGNATURES = {
    "mhip_hydro_set_sparse_sources": [_vp, _i],
    "mhip_contact_op_apply_hydro": [_vp, C.POINTER(HydroMobility), _vp, _vp, _vp],
    "mhip_bbpgd_solve_contact_hydro": [_vp, C.POINTER(HydroMobility), _vp, C.POINTER(Space), C.POINTER(PgdConfig), _vp,
                                       _vp, _vp, _vp, C.POINTER(SolveResult), _vp],
}
# include/mundy_hip_filament_inertial.h, a header of its own for the same reason: name -> argtypes, every function returns
# int status.  tests/test_filament_inertial_host.py checks this table against that header and the library.
FILAMENT_DAMPING_CONSTANT, FILAMENT_DAMPING_CRITICAL = 0, 1
FILAMENT_CONTACT_FRICTIONAL, FILAMENT_CONTACT_HERTZ = 0, 1
FILAMENT_INERTIAL_SIGNATURES = {
    "mhip_filaments_set_inertial": [_vp, C.POINTER(FilamentInertialParams), _vp],
    "mhip_filaments_set_motion": [_vp, _vp, _vp, _vp, _vp],
    "mhip_filaments_predict": [_vp, _d],
    "mhip_filaments_correct": [_vp, _d, _vp],
    "mhip_filaments_kinetic_energy": [_vp, _vp],
    "mhip_filaments_set_youngs_modulus": [_vp, _d],
    "mhip_filaments_get_inertial": [_vp, C.POINTER(FilamentInertialFields)],
    "mhip_filament_contacts_set_law": [_vp, _i],
}
# include/mundy_hip_bending.h, a header of its own for the same reason: name -> argtypes, every function returns int
# status.  tests/test_bending_host.py checks this table against that header and the library.
BENDING_SIGNATURES = {
    "mhip_springs_set_wca": [_vp, _d, _d],
    "mhip_angular_springs_create": [C.POINTER(_vp), _sz, _sz, _vp, _vp, _d, _vp, _d, _vp],
    "mhip_angular_springs_force": [_vp, _vp, _vp, _i, _vp, _vp, _vp],
    "mhip_angular_springs_renumber": [_vp, _vp, _vp],
    "mhip_angular_springs_get": [_vp, _vp, _vp, _vp],
    "mhip_angular_springs_destroy": [_vp],
}
OTHER_SYMBOLS = {"mhip_last_error": ([], C.c_char_p), "mhip_version": ([], C.c_int),
                 "mhip_release_cached_workspaces": ([], C.c_int)}

_lib = None


def load():
    """dlopen the in-tree library; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MhipError("%s is missing: run `python -m mundy_amd.build` (or __graft_entry__.build()); "
                            "mundy_amd has no CPU fallback" % LIB_PATH)
        # torch ships its own libamdhip64; it must be mapped first so that torch's allocator/streams and this
        # library share ONE HIP runtime (loading the system runtime first leaves the process with a runtime that
        # cannot see torch's device context)
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, argtypes in (list(SIGNATURES.items()) + list(PERIPHERY_SIGNATURES.items()) +
                               list(CONTACT_FORCE_SIGNATURES.items()) + list(PERIPHERY_BINDING_SIGNATURES.items()) +
                               list(SEGMENT_CONTACT_SIGNATURES.items()) + list(HYDRO_SOLVE_SIGNATURES.items()) +
                               list(FILAMENT_INERTIAL_SIGNATURES.items()) + list(BENDING_SIGNATURES.items())):
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = C.c_int
        for name, (argtypes, restype) in OTHER_SYMBOLS.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = lib
    return _lib


def check(status):
    """status -> the exception type the reference throws for that class of error (throw_assert.hpp:135-203)."""
    if status == SUCCESS:
        return
    msg = load().mhip_last_error().decode()
    if status == ERR_INVALID_ARGUMENT:
        raise ValueError(msg)  # std::invalid_argument
    if status == ERR_LOGIC:
        raise AssertionError(msg)  # std::logic_error
    if status == ERR_RUNTIME:
        raise RuntimeError(msg)  # std::runtime_error
    raise MhipError(msg)
