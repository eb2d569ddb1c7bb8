"""ctypes binding of libsph_hip.so (C ABI: include/sph_hip.h).

The product path has no fallback: if the shared library is missing (and cannot
be built) or no gfx950 device is visible, this raises.
"""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

_F3 = C.c_float * 3
_I3 = C.c_int32 * 3


class SphParams(C.Structure):
    """Mirror of `struct SphParams` (include/sph_hip.h)."""
    _fields_ = [
        ("n_particles", C.c_int32), ("capacity", C.c_int32), ("grid_num", _I3), ("cell_origin", _I3),
        ("n_objects", C.c_int32), ("cold_capacity", C.c_int32),
        ("grid_size", C.c_float), ("support_radius", C.c_float), ("particle_diameter", C.c_float),
        ("m_V0", C.c_float), ("density_0", C.c_float), ("stiffness", C.c_float), ("exponent", C.c_float),
        ("viscosity", C.c_float), ("surface_tension", C.c_float), ("dt", C.c_float),
        ("g", _F3), ("domain_size", _F3), ("padding", C.c_float), ("wall_hi", _F3),
        ("k_w", C.c_float), ("k_dw", C.c_float), ("visc_d_nu", C.c_float), ("visc_eps", C.c_float),
    ]


class SphTimings(C.Structure):
    _fields_ = [("sort_ms", C.c_double), ("neighbour_ms", C.c_double), ("force_ms", C.c_double),
                ("integrate_ms", C.c_double), ("halo_ms", C.c_double), ("total_ms", C.c_double),
                ("steps", C.c_int64)]


class SphStats(C.Structure):
    _fields_ = [("targets", C.c_int64), ("list_entries", C.c_int64), ("max_list", C.c_int32),
                ("list_overflow_targets", C.c_int32), ("lds_overflow_targets", C.c_int32),
                ("max_cell_occupancy", C.c_int32), ("nonempty_cells", C.c_int32), ("polar_fallbacks", C.c_int32)]


class SphDfsphParams(C.Structure):
    _fields_ = [("enable_divergence_solver", C.c_int32), ("m_max_iterations_v", C.c_int32),
                ("m_max_iterations", C.c_int32), ("fluid_particle_num", C.c_int32), ("m_eps", C.c_float),
                ("reserved_", C.c_float), ("max_error_V", C.c_double), ("max_error", C.c_double)]


class SphDfsphStats(C.Structure):
    _fields_ = [("iterations_v", C.c_int32), ("iterations", C.c_int32), ("avg_density_err_v", C.c_double),
                ("avg_density_err", C.c_double), ("total_iterations_v", C.c_int64), ("total_iterations", C.c_int64),
                ("steps", C.c_int64)]


class SphRenderParams(C.Structure):
    """Mirror of `struct SphRenderParams` (include/sph_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("eye", _F3), ("lookat", _F3), ("up", _F3),
                ("fov_y_deg", C.c_float), ("radius", C.c_float), ("near_plane", C.c_float), ("light", _F3),
                ("ambient", C.c_float), ("background", C.c_uint8 * 3), ("draw_box", C.c_uint8),
                ("box_end", _F3), ("box_color", _F3)]


RENDER_MAX_INVISIBLE = 32
_D3 = C.c_double * 3


class SphKinematicMotion(C.Structure):
    """Mirror of `struct SphKinematicMotion` (include/sph_hip.h)."""
    _fields_ = [("object_id", C.c_int32), ("pivot", _F3), ("lin_vel", _D3), ("ang_vel", _D3), ("osc_amplitude", _D3),
                ("osc_frequency", C.c_double), ("osc_phase", C.c_double), ("start_time", C.c_double), ("end_time", C.c_double)]


class SphBodyPose(C.Structure):
    """Mirror of `struct SphBodyPose` (include/sph_hip.h)."""
    _fields_ = [("object_id", C.c_int32), ("R", C.c_float * 9), ("pivot", _F3), ("origin", _F3), ("lin_vel", _F3),
                ("ang_vel", _F3)]


MAX_KINEMATIC = 8


class SphDiagRow(C.Structure):
    """Mirror of `struct SphDiagRow` (include/sph_hip.h)."""
    _fields_ = [("count", C.c_int64), ("fluid_count", C.c_int64), ("moving_count", C.c_int64), ("mass", C.c_double),
                ("mx", _D3), ("momentum", _D3), ("kinetic", C.c_double), ("v2_max", C.c_double), ("a2_max", C.c_double),
                ("density_min", C.c_float), ("density_max", C.c_float), ("pressure_min", C.c_float),
                ("pressure_max", C.c_float), ("lo", _F3), ("hi", _F3)]


# launch shape of the diagnostics reduction (SPH_DIAG_BLOCKS x SPH_DIAG_THREADS, striding) and its object limit
DIAG_BLOCKS, DIAG_THREADS, DIAG_MAX_OBJECTS = 1024, 256, 96

class SphColumnParams(C.Structure):
    """Mirror of `struct SphColumnParams` (include/sph_hip.h)."""
    _fields_ = [("axis", C.c_int32), ("n", C.c_int32 * 2), ("origin", C.c_float * 2), ("inv_cell", C.c_float * 2),
                ("object_id", C.c_int32)]


class SphColumnTotals(C.Structure):
    """Mirror of `struct SphColumnTotals` (include/sph_hip.h)."""
    _fields_ = [("selected", C.c_int64), ("binned", C.c_int64), ("outside", C.c_int64)]


# limits of the column maps: columns per map, and the fixed-point scale 2^20 of the velocity sums
COLUMNS_MAX, COLUMNS_V_SCALE_LOG2 = 1 << 20, 20

class SphExportParams(C.Structure):
    """Mirror of `struct SphExportParams` (include/sph_hip.h)."""
    _fields_ = [("fields", C.c_int32), ("material", C.c_int32), ("n_objects", C.c_int32), ("object_ids", C.c_int32 * 32),
                ("pid_stride", C.c_int32), ("pid_phase", C.c_int32), ("use_box", C.c_int32), ("box_lo", _F3), ("box_hi", _F3)]


class SphExportInfo(C.Structure):
    """Mirror of `struct SphExportInfo` (include/sph_hip.h)."""
    _fields_ = [("selected", C.c_int64), ("rows", C.c_int64), ("row_bytes", C.c_int32), ("duplicate_ids", C.c_int32)]


# field bits of the particle export (SPH_EXPORT_*) and its object-list limit
EXPORT_X, EXPORT_V, EXPORT_DENSITY, EXPORT_PRESSURE, EXPORT_MASS, EXPORT_ID, EXPORT_OBJECT = 1, 2, 4, 8, 16, 32, 64
EXPORT_MAX_OBJECTS = 32

class SphSurfaceParams(C.Structure):
    """Mirror of `struct SphSurfaceParams` (include/sph_hip.h)."""
    _fields_ = [("iterations", C.c_int32), ("filter_radius", C.c_float), ("depth_range", C.c_float), ("fluid_color", _F3),
                ("absorb", _F3), ("sky", _F3), ("f0", C.c_float), ("specular", C.c_float)]


# limits of the surface frame (SPH_SURFACE_*) and the number of passes sph_surface_frame_timed reports
SURFACE_MAX_FILTER_R, SURFACE_MAX_ITERATIONS, SURFACE_PASSES = 16, 8, 6
SURFACE_PASS_NAMES = ("clear", "opaque_splat", "fluid_splat", "depth_smoothing", "thickness_smoothing", "shade_resolve")

FIELD_MAX_OBJECTS = 32


class SphFieldColour(C.Structure):
    """Mirror of `struct SphFieldColour` (include/sph_hip.h); `field` is an index into render.FIELDS."""
    _fields_ = [("field", C.c_int32), ("material", C.c_int32), ("n_objects", C.c_int32), ("object_ids", C.c_int32 * FIELD_MAX_OBJECTS),
                ("lo", C.c_float), ("hi", C.c_float), ("axis_origin", C.c_float)]


class SphFieldRange(C.Structure):
    """Mirror of `struct SphFieldRange` (include/sph_hip.h)."""
    _fields_ = [("lo", C.c_float), ("hi", C.c_float), ("count", C.c_int64), ("non_finite", C.c_int64)]


class SphSampleSelect(C.Structure):
    """Mirror of `struct SphSampleSelect` (include/sph_hip.h)."""
    _fields_ = [("material", C.c_int32), ("n_objects", C.c_int32), ("object_ids", C.c_int32 * 32)]


class SphSampleGrid(C.Structure):
    """Mirror of `struct SphSampleGrid` (include/sph_hip.h)."""
    _fields_ = [("n", C.c_int32 * 3), ("origin", _F3), ("spacing", _F3), ("inv_h", C.c_float), ("fields", C.c_int32),
                ("select", SphSampleSelect)]


class SphMeshSpec(C.Structure):
    """Mirror of `struct SphMeshSpec` (include/sph_hip.h)."""
    _fields_ = [("iso", C.c_float), ("cap", C.c_int32)]


class SphTracerParams(C.Structure):
    """Mirror of `struct SphTracerParams` (include/sph_hip.h)."""
    _fields_ = [("min_fill", C.c_float), ("record_every", C.c_int32), ("record_capacity", C.c_int32), ("select", SphSampleSelect)]


class SphTracerInfo(C.Structure):
    """Mirror of `struct SphTracerInfo` (include/sph_hip.h)."""
    _fields_ = [("m", C.c_int32), ("reserved_", C.c_int32), ("advances", C.c_int64), ("frames", C.c_int64), ("dropped", C.c_int64)]


STATS_MAX_SAMPLES = 1 << 19


class SphStatsParams(C.Structure):
    """Mirror of `struct SphStatsParams` (include/sph_hip.h)."""
    _fields_ = [("grid", SphSampleGrid), ("every", C.c_int32), ("capacity", C.c_int32), ("wet_min", C.c_int64)]


class SphStatsInfo(C.Structure):
    """Mirror of `struct SphStatsInfo` (include/sph_hip.h)."""
    _fields_ = [("nodes", C.c_int64), ("n", C.c_int32 * 3), ("every", C.c_int32), ("samples", C.c_int64), ("dropped", C.c_int64),
                ("steps_seen", C.c_int64), ("t_first", C.c_double), ("t_last", C.c_double)]


LOADS_MAX_OBJECTS, LOADS_ROW_WORDS, LOADS_SCALE_LOG2 = 32, 9, 24


class SphLoadParams(C.Structure):
    """Mirror of `struct SphLoadParams` (include/sph_hip.h)."""
    _fields_ = [("object_ids", C.c_int32 * LOADS_MAX_OBJECTS), ("n_objects", C.c_int32), ("about", _F3), ("every", C.c_int32),
                ("capacity", C.c_int32)]


class SphLoadInfo(C.Structure):
    """Mirror of `struct SphLoadInfo` (include/sph_hip.h)."""
    _fields_ = [("n_objects", C.c_int32), ("every", C.c_int32), ("samples", C.c_int64), ("dropped", C.c_int64), ("steps_seen", C.c_int64)]


SCALARS_MAX_CHANNELS, SCALARS_MAX_SOURCES, SCALARS_SCALE_LOG2 = 4, 8, 32


class SphScalarParams(C.Structure):
    """Mirror of `struct SphScalarParams` (include/sph_hip.h)."""
    _fields_ = [("K", C.c_int32), ("kappa", C.c_float * SCALARS_MAX_CHANNELS), ("every", C.c_int32), ("select", SphSampleSelect),
                ("n_sources", C.c_int32), ("source_object", C.c_int32 * SCALARS_MAX_SOURCES),
                ("source_value", (C.c_double * SCALARS_MAX_CHANNELS) * SCALARS_MAX_SOURCES)]


class SphScalarInfo(C.Structure):
    """Mirror of `struct SphScalarInfo` (include/sph_hip.h)."""
    _fields_ = [("K", C.c_int32), ("every", C.c_int32), ("ids", C.c_int64), ("samples", C.c_int64), ("steps_seen", C.c_int64),
                ("overshoot", C.c_int64 * SCALARS_MAX_CHANNELS), ("saturated", C.c_int64 * SCALARS_MAX_CHANNELS)]


FEATURES_SCALE_LOG2, FEATURES_FILL_SCALE_LOG2 = 24, 30
FEATURE_VALID, FEATURE_SURFACE, FEATURE_SATURATED = 1, 2, 4
FEATURE_FIELDS = ("vorticity", "divergence", "fill", "neighbours", "surface")      # enum SphFeatureField


class SphFeatureParams(C.Structure):
    """Mirror of `struct SphFeatureParams` (include/sph_hip.h)."""
    _fields_ = [("select", SphSampleSelect), ("every", C.c_int32), ("min_neighbours", C.c_int32), ("normal_min", C.c_float)]


class SphFeatureRow(C.Structure):
    """Mirror of `struct SphFeatureRow` (include/sph_hip.h): 64 bytes."""
    _fields_ = [("x", _F3), ("vorticity", _F3), ("divergence", C.c_float), ("normal", _F3), ("fill", C.c_float),
                ("n_fluid", C.c_int32), ("n_solid", C.c_int32), ("flags", C.c_int32), ("reserved_", C.c_int32 * 2)]


class SphFeatureInfo(C.Structure):
    """Mirror of `struct SphFeatureInfo` (include/sph_hip.h)."""
    _fields_ = [("every", C.c_int32), ("reserved_", C.c_int32), ("rows", C.c_int64), ("samples", C.c_int64), ("steps_seen", C.c_int64),
                ("step", C.c_int64), ("time", C.c_double)]


TRACERS_MAX = 1 << 22

# field bits of the field sampling (SPH_SAMPLE_*), its limits and the fixed-point scale 2^30 of its sums
SAMPLE_VX, SAMPLE_VY, SAMPLE_VZ, SAMPLE_DENSITY, SAMPLE_PRESSURE = 1, 2, 4, 8, 16
SAMPLE_MAX_NODES, SAMPLE_MAX_POINTS, SAMPLE_MAX_OBJECTS, SAMPLE_SCALE_LOG2 = 1 << 24, 1024, 32, 30
SAMPLE_MAX_CHANNELS = 2 + 5 + 3 + 15     # count, weight, five field planes, Gx Gy Gz, three planes per gradient bit

# enum SphField
F_OBJECT_ID, F_X, F_X_0, F_V, F_ACCELERATION, F_M_V, F_M, F_DENSITY, F_PRESSURE, F_MATERIAL, F_COLOR, \
    F_IS_DYNAMIC, F_GRID_IDS, F_GRID_PARTICLES_NUM, F_PID, F_RIGID_REST_CM, F_DFSPH_FACTOR, F_DENSITY_ADV = range(18)
# enum SphOption
OPT_GATHER_IMPL, OPT_TIMING, OPT_FUSED_STEP, OPT_BRICK_SHAPE, OPT_NO_DYNAMIC_SOLIDS, OPT_DEBUG_ABLATE, \
    OPT_SLAB_DROP_OUTSIDE, OPT_UNIFORM_FLUID, OPT_UNIFORM_FLUID_STATE, OPT_SORT_BY_PID, OPT_KERNEL_VARIANT, \
    OPT_RIGID_BATCH, OPT_EXACT_MATH, OPT_DF_RUNAHEAD, OPT_RIGID_SUMS_FROM_X0, OPT_PURE_FLUID_INSTANCE, OPT_BRICK_RECORDS, OPT_DF_FUSE_ERROR, \
    OPT_SORT_FAST, OPT_SORT_FAST_COUNT, OPT_SORT_GENERAL_COUNT, OPT_SORT_LEAN = range(22)
VAR_GROUPS, VAR_GAT_LDS, VAR_GAT_LDS4, VAR_FORCE_BF, VAR_DEEP, VAR_MFMA = 1, 2, 4, 8, 16, 32
VAR_DEFAULT = VAR_GROUPS | VAR_FORCE_BF | VAR_DEEP

ABI_VERSION = 6

# every symbol include/sph_hip.h declares: (name, restype, argtypes)
_ctx = C.c_void_p
SYMBOLS = [
    ("sph_abi_version", C.c_int32, []),
    ("sph_device_count", C.c_int32, []),
    ("sph_create", C.c_int32, [C.POINTER(SphParams), C.c_int32, C.c_void_p, C.POINTER(_ctx)]),
    ("sph_destroy", C.c_int32, [_ctx]),
    ("sph_last_error", C.c_char_p, [_ctx]),
    ("sph_set_option", C.c_int32, [_ctx, C.c_int32, C.c_int32]),
    ("sph_get_option", C.c_int32, [_ctx, C.c_int32, C.POINTER(C.c_int32)]),
    ("sph_set_params", C.c_int32, [_ctx, C.POINTER(SphParams)]),
    ("sph_set_dt", C.c_int32, [_ctx, C.c_float]),
    ("sph_set_particle_count", C.c_int32, [_ctx, C.c_int32]),
    ("sph_upload", C.c_int32, [_ctx, C.c_int32, C.c_void_p, C.c_size_t]),
    ("sph_download", C.c_int32, [_ctx, C.c_int32, C.c_void_p, C.c_size_t]),
    ("sph_update_grid_id", C.c_int32, [_ctx]),
    ("sph_prefix_sum", C.c_int32, [_ctx]),
    ("sph_counting_sort", C.c_int32, [_ctx]),
    ("sph_initialize_particle_system", C.c_int32, [_ctx]),
    ("sph_compute_boundary_volume", C.c_int32, [_ctx, C.c_int32]),
    ("sph_compute_densities", C.c_int32, [_ctx]),
    ("sph_compute_non_pressure_forces", C.c_int32, [_ctx]),
    ("sph_compute_pressure_forces", C.c_int32, [_ctx]),
    ("sph_advect", C.c_int32, [_ctx]),
    ("sph_enforce_boundary_3D", C.c_int32, [_ctx, C.c_int32]),
    ("sph_compute_rigid_rest_cm", C.c_int32, [_ctx, C.c_int32]),
    ("sph_solve_constraints", C.c_int32, [_ctx, C.c_int32, C.POINTER(C.c_float)]),
    ("sph_compute_com", C.c_int32, [_ctx, C.c_int32, C.POINTER(C.c_float)]),
    ("sph_step", C.c_int32, [_ctx, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    ("sph_sync", C.c_int32, [_ctx]),
    ("sph_get_timings", C.c_int32, [_ctx, C.POINTER(SphTimings)]),
    ("sph_reset_timings", C.c_int32, [_ctx]),
    ("sph_get_stats", C.c_int32, [_ctx, C.POINTER(SphStats)]),
    ("sph_get_particle_count", C.c_int32, [_ctx, C.POINTER(C.c_int32)]),
    ("sph_layer_offsets", C.c_int32, [_ctx, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]),
    ("sph_layer_offsets_begin", C.c_int32, [_ctx, C.POINTER(C.c_int32), C.c_int32]),
    ("sph_layer_offsets_end", C.c_int32, [_ctx, C.POINTER(C.c_int32), C.c_int32]),
    ("sph_select_range", C.c_int32, [_ctx, C.c_int32, C.c_int32]),
    ("sph_truncate", C.c_int32, [_ctx, C.c_int32]),
    ("sph_pack_range", C.c_int32, [_ctx, C.c_int32, C.c_int32, C.c_void_p]),
    ("sph_append_records", C.c_int32, [_ctx, C.c_void_p, C.c_int32]),
    ("sph_set_target_layers", C.c_int32, [_ctx, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ("sph_slab_set_window", C.c_int32, [_ctx, C.c_int32, C.c_int32]),
    ("sph_slab_pack", C.c_int32, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    ("sph_slab_advance", C.c_int32, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                     C.POINTER(C.c_int32), C.c_int32, C.c_int32]),
    ("sph_slab_forces", C.c_int32, [_ctx, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_int32, C.c_int32, C.c_void_p]),
    ("sph_slab_wait_pack", C.c_int32, [_ctx]),
    ("sph_slab_density", C.c_int32, [_ctx]),
    ("sph_sort", C.c_int32, [_ctx]),
    ("sph_sweeps", C.c_int32, [_ctx]),
    ("sph_rigid_partial_sums", C.c_int32, [_ctx, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    ("sph_rigid_apply_sums", C.c_int32, [_ctx, C.c_int32, C.c_void_p, C.c_int32]),
    ("sph_upload_rest_positions", C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_int32]),
    ("sph_dfsph_set_params", C.c_int32, [_ctx, C.POINTER(SphDfsphParams)]),
    ("sph_dfsph_get_stats", C.c_int32, [_ctx, C.POINTER(SphDfsphStats)]),
    ("sph_dfsph_compute_densities", C.c_int32, [_ctx]),
    ("sph_dfsph_compute_DFSPH_factor", C.c_int32, [_ctx]),
    ("sph_dfsph_compute_density_change", C.c_int32, [_ctx]),
    ("sph_dfsph_compute_density_adv", C.c_int32, [_ctx]),
    ("sph_dfsph_compute_density_error", C.c_int32, [_ctx, C.c_float, C.POINTER(C.c_float)]),
    ("sph_dfsph_multiply_time_step", C.c_int32, [_ctx, C.c_float]),
    ("sph_dfsph_divergence_solver_iteration_kernel", C.c_int32, [_ctx]),
    ("sph_dfsph_pressure_solve_iteration_kernel", C.c_int32, [_ctx]),
    ("sph_dfsph_divergence_solve", C.c_int32, [_ctx]),
    ("sph_dfsph_pressure_solve", C.c_int32, [_ctx]),
    ("sph_dfsph_compute_non_pressure_forces", C.c_int32, [_ctx]),
    ("sph_dfsph_predict_velocity", C.c_int32, [_ctx]),
    ("sph_dfsph_advect", C.c_int32, [_ctx]),
    ("sph_dfsph_step", C.c_int32, [_ctx, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    ("sph_dfsph_compute_density_error_range", C.c_int32, [_ctx, C.c_float, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    ("sph_copy_velocity_records", C.c_int32, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]),
    ("sph_comm_last_error", C.c_char_p, []),
    ("sph_comm_available", C.c_int32, []),
    ("sph_comm_unique_id", C.c_int32, [C.c_void_p]),
    ("sph_comm_create", C.c_int32, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    ("sph_comm_destroy", C.c_int32, [C.c_void_p]),
    ("sph_slab_announce", C.c_int32, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ("sph_slab_incoming", C.c_int32, [_ctx, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("sph_slab_exchange", C.c_int32, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                      C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]),
    ("sph_comm_swap", C.c_int32, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                  C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    ("sph_comm_all_reduce", C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    ("sph_comm_sync", C.c_int32, [_ctx, C.c_void_p]),
    ("sph_comm_halo_time", C.c_int32, [_ctx, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    ("sph_comm_info", C.c_int32, [_ctx, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("sph_render_set_params", C.c_int32, [_ctx, C.POINTER(SphRenderParams)]),
    ("sph_render_set_invisible", C.c_int32, [_ctx, C.POINTER(C.c_int32), C.c_int32]),
    ("sph_render_frame", C.c_int32, [_ctx]),
    ("sph_render_download", C.c_int32, [_ctx, C.c_void_p, C.c_size_t]),
    ("sph_render_download_depth", C.c_int32, [_ctx, C.c_void_p, C.c_size_t]),
    ("sph_kinematic_set", C.c_int32, [_ctx, C.POINTER(SphKinematicMotion), C.c_int32]),
    ("sph_kinematic_apply", C.c_int32, [_ctx, C.POINTER(SphBodyPose), C.c_int32]),
    ("sph_get_time", C.c_int32, [_ctx, C.POINTER(C.c_double)]),
    ("sph_set_time", C.c_int32, [_ctx, C.c_double]),
    ("sph_diag_reduce", C.c_int32, [_ctx]),
    ("sph_diag_download", C.c_int32, [_ctx, C.POINTER(SphDiagRow), C.c_int32]),
    ("sph_columns_reduce", C.c_int32, [_ctx, C.POINTER(SphColumnParams)]),
    ("sph_columns_download", C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.POINTER(SphColumnTotals)]),
    ("sph_export_select", C.c_int32, [_ctx, C.POINTER(SphExportParams)]),
    ("sph_export_info", C.c_int32, [_ctx, C.POINTER(SphExportInfo)]),
    ("sph_export_download", C.c_int32, [_ctx, C.c_void_p, C.c_size_t]),
    ("sph_surface_set_params", C.c_int32, [_ctx, C.POINTER(SphSurfaceParams)]),
    ("sph_surface_frame", C.c_int32, [_ctx]),
    ("sph_surface_download", C.c_int32, [_ctx, C.c_void_p, C.c_size_t]),
    ("sph_surface_download_depth", C.c_int32, [_ctx, C.c_void_p, C.c_size_t]),
    ("sph_surface_download_thickness", C.c_int32, [_ctx, C.c_void_p, C.c_size_t]),
    ("sph_surface_frame_timed", C.c_int32, [_ctx, C.POINTER(C.c_float), C.c_int32]),
    ("sph_frame_set_colour", C.c_int32, [_ctx, C.POINTER(SphFieldColour), C.c_void_p]),
    ("sph_field_range", C.c_int32, [_ctx, C.POINTER(SphFieldColour), C.POINTER(SphFieldRange)]),
    ("sph_frame_download_field_index", C.c_int32, [_ctx, C.c_void_p, C.c_size_t]),
    ("sph_sample_grid", C.c_int32, [_ctx, C.POINTER(SphSampleGrid)]),
    ("sph_sample_grid_download", C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    ("sph_sample_points", C.c_int32, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SphSampleSelect), C.c_float]),
    ("sph_sample_points_download", C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    ("sph_sample_grid_gradients", C.c_int32, [_ctx, C.POINTER(SphSampleGrid), C.c_int32]),
    ("sph_sample_grid_gradients_download", C.c_int32, [_ctx, C.c_void_p, C.c_int64]),
    ("sph_sample_points_gradients", C.c_int32, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(SphSampleSelect), C.c_float]),
    ("sph_sample_points_gradients_download", C.c_int32, [_ctx, C.c_void_p, C.c_int32]),
    ("sph_mesh_extract", C.c_int32, [_ctx, C.POINTER(SphMeshSpec)]),
    ("sph_mesh_counts", C.c_int32, [_ctx, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("sph_mesh_download", C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    ("sph_tracers_set", C.c_int32, [_ctx, C.c_void_p, C.c_int32, C.POINTER(SphTracerParams)]),
    ("sph_tracers_info", C.c_int32, [_ctx, C.POINTER(SphTracerInfo)]),
    ("sph_tracers_download", C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    ("sph_tracers_history_download", C.c_int32, [_ctx, C.c_void_p, C.c_int64, C.c_int32]),
    ("sph_stats_set", C.c_int32, [_ctx, C.POINTER(SphStatsParams)]),
    ("sph_stats_sample", C.c_int32, [_ctx]),
    ("sph_stats_info", C.c_int32, [_ctx, C.POINTER(SphStatsInfo)]),
    ("sph_stats_download", C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    ("sph_stats_reset", C.c_int32, [_ctx]),
    ("sph_loads_set", C.c_int32, [_ctx, C.POINTER(SphLoadParams)]),
    ("sph_loads_sample", C.c_int32, [_ctx]),
    ("sph_loads_info", C.c_int32, [_ctx, C.POINTER(SphLoadInfo)]),
    ("sph_loads_download", C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    ("sph_loads_reset", C.c_int32, [_ctx]),
    ("sph_scalars_set", C.c_int32, [_ctx, C.c_void_p, C.c_int64, C.POINTER(SphScalarParams)]),
    ("sph_scalars_sample", C.c_int32, [_ctx]),
    ("sph_scalars_info", C.c_int32, [_ctx, C.POINTER(SphScalarInfo)]),
    ("sph_scalars_download", C.c_int32, [_ctx, C.c_void_p, C.c_void_p, C.c_int64]),
    ("sph_scalars_paint", C.c_int32, [_ctx, C.c_int32, C.c_float, C.c_float, C.c_void_p]),
    ("sph_features_set", C.c_int32, [_ctx, C.POINTER(SphFeatureParams)]),
    ("sph_features_sample", C.c_int32, [_ctx]),
    ("sph_features_info", C.c_int32, [_ctx, C.POINTER(SphFeatureInfo)]),
    ("sph_features_download", C.c_int32, [_ctx, C.c_void_p, C.c_int64]),
    ("sph_features_paint", C.c_int32, [_ctx, C.c_int32, C.c_float, C.c_float, C.c_void_p]),
]

_LIB = None


class SphError(RuntimeError):
    pass


def profiling_variant() -> bool:
    """SPH_HIP_LIB_VARIANT=profile: load the profiling build (section ablation compiled in) instead of the product library.
    Set by bench.py --ablate / --ablate-mask before the first load; never by the product."""
    return os.environ.get("SPH_HIP_LIB_VARIANT", "") == "profile"


def experiment_variant() -> str:
    """SPH_HIP_LIB_VARIANT=x-<tag>: load libsph_hip_x-<tag>.so -- the SAME sources built with other compiler flags by
    tools/sched_sweep.py (an A/B aid of the measurement tools, never set by the product; the file must exist, it is never built here)."""
    v = os.environ.get("SPH_HIP_LIB_VARIANT", "")
    return v if v.startswith("x-") else ""


def library_path() -> str:
    if experiment_variant():
        return os.path.join(os.path.dirname(_build.LIB), f"libsph_hip_{experiment_variant()}.so")
    return _build.LIB_PROFILE if profiling_variant() else _build.LIB


def _preload_shared_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME
    as /opt/rocm's); whichever copy is mapped first serves both torch and libsph_hip.so, and torch
    cannot initialise on the system copy.  So when torch is installed, map its copy first -- then the
    import order of torch and this package no longer matters.  Without torch the system runtime is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load(build_if_missing: bool = True):
    """dlopen libsph_hip.so, binding every symbol of the header.  Raises if absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if build_if_missing and not experiment_variant() and _build.stale(profiling_variant()):
        try:
            _build.build(profile=profiling_variant())
        except Exception as e:  # no hipcc on this box: use the prebuilt file if any
            if not os.path.exists(path):
                raise SphError(f"libsph_hip.so is missing and could not be built: {e}") from e
    if not os.path.exists(path):
        raise SphError(f"{path} not found: run `python -m sph_taichi_amd.build` (needs hipcc)")
    _preload_shared_hip_runtime()
    lib = C.CDLL(path)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.sph_abi_version() != ABI_VERSION:
        raise SphError(f"libsph_hip ABI {lib.sph_abi_version()} != binding {ABI_VERSION}")
    _LIB = lib
    return lib


def check(lib, ctx, rc: int, what: str):
    if rc != 0:
        msg = lib.sph_last_error(ctx)
        raise SphError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
