"""ctypes binding of libg4c.so (the C-ABI declared in include/g4c.h).

The product path has no CPU / eager-torch fallback: if the HIP library is missing the import
of any compute entry point raises, and every op rejects non-HIP tensors.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("G4C_LIB_PATH") or os.path.join(_HERE, "lib", "libg4c.so")      # (G4C_LIB_PATH: A/B of two builds)

OK, EINVAL, ELAUNCH, EUNSUPPORTED = 0, -1, -2, -3
ACT_NONE, ACT_SELU, ACT_TANH = 0, 1, 2
MAX_SRC, MAX_LAYERS = 4, 4
MAX_HEADS = 2
NARROW_MAX = 8
KERNEL_MLP_RS = 5
KERNEL_MLP_RS2 = 6
KERNEL_MLP_BX6, KERNEL_MLP_WS = 2, 4
KERNEL_MLP_BX6_CERT, KERNEL_MLP_WS_CERT = 7, 8      # the instantiations without the fp16 range tracker (g4c_mlp_t.range_certified)
KERNEL_MLP_WS_PRE = 9                               # mlp_ws_pre_kernel: the first layer precomputed (g4c_mlp_t.k_pad[0] == 0)
KERNEL_NAMES = {0: "none", 1: "mlp_split_kernel", 2: "mlp_bx6_kernel", 3: "mlp_bx6i_kernel", 4: "mlp_ws_kernel", 5: "mlp_rs1_kernel", 6: "mlp_rs2_kernel",
                7: "mlp_bx6_kernel", 8: "mlp_ws_kernel", 9: "mlp_ws_kernel"}   # g4c_mlp_last_kernel (9: its first-layer-precomputed form, one family for the timer)

TILE_SHAPE_GENERIC, TILE_SHAPE_NODE, TILE_SHAPE_UP, TILE_SHAPE_DOWN = 0, 1, 2, 3      # g4c_mlp_last_shape

_ACT_CODES = {None: ACT_NONE, "none": ACT_NONE, "selu": ACT_SELU, "tanh": ACT_TANH}


def act_code(activation) -> Optional[int]:
    """Map an activation spec to a fused-epilogue code, or None if it cannot be fused
    (an arbitrary callable is then applied by the caller with torch on the HIP tensor)."""
    if activation is None or isinstance(activation, str):
        return _ACT_CODES[activation]
    if activation is torch.tanh or activation is torch.nn.functional.tanh:
        return ACT_TANH
    if activation is torch.nn.functional.selu or activation is torch.selu:
        return ACT_SELU
    return None


class g4c_src_t(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("idx", C.c_void_p), ("width", C.c_int32), ("ld", C.c_int32),
                ("col0", C.c_int32), ("pre_act", C.c_int32), ("additive", C.c_int32), ("seg_mean", C.c_int32),
                ("w", C.c_void_p), ("seg_off", C.c_void_p), ("seg_perm", C.c_void_p), ("dtype", C.c_int32)]


class g4c_mlp_t(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("k_pad", C.c_int32 * MAX_LAYERS), ("n_pad", C.c_int32 * MAX_LAYERS),
                ("w", C.c_void_p * MAX_LAYERS), ("b", C.c_void_p * MAX_LAYERS),
                ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_eps", C.c_float), ("n_out", C.c_int32), ("w_format", C.c_int32),
                ("range_slot", C.c_int32), ("range_certified", C.c_int32)]


WFMT_FP32, WFMT_F16X2, WFMT_BF16X3, WFMT_BF16_RS, WFMT_BF16_RS2, WFMT_BF16_RS2N, WFMT_BF16 = 0, 1, 2, 3, 4, 5, 6
DTYPE_F32, DTYPE_BF16 = 0, 1          # g4c_mlp_io_t.save_dtype / mul_dtype


class g4c_mlp_io_t(C.Structure):
    _fields_ = [("size", C.c_int32), ("act", C.c_int32), ("row_begin", C.c_int64), ("row_count", C.c_int64),
                ("out", C.c_void_p), ("out_ld", C.c_int32), ("out_dtype", C.c_int32), ("out_idx", C.c_void_p),
                ("resid", C.c_void_p), ("resid_ld", C.c_int32), ("resid_col0", C.c_int32),
                ("n_heads", C.c_int32), ("head_ld", C.c_int32), ("head_dtype", C.c_int32), ("head_out", C.c_void_p * MAX_HEADS),
                ("tile_rows", C.c_void_p), ("tile_seg", C.c_void_p), ("seg_off", C.c_void_p), ("n_tiles", C.c_int32),
                ("agg", C.c_void_p), ("agg_ld", C.c_int32), ("agg_mode", C.c_int32),
                ("n_save", C.c_int32), ("save", C.c_void_p * MAX_LAYERS), ("save_ld", C.c_int32),
                ("mul", C.c_void_p * MAX_LAYERS), ("mul_ld", C.c_int32),
                ("upd", C.POINTER(g4c_mlp_t)), ("v", C.c_void_p), ("v_ld", C.c_int32), ("v_act", C.c_int32),
                ("v_out", C.c_void_p), ("v_out_ld", C.c_int32), ("range_flag", C.c_void_p),
                ("save_dtype", C.c_int32), ("mul_dtype", C.c_int32),
                ("wg_rows", C.c_void_p), ("wg_seg", C.c_void_p), ("n_wg", C.c_int32), ("wg_pairs", C.c_int32), ("wg_max_seg", C.c_int32)]

    def __init__(self, **kw):
        super().__init__(size=C.sizeof(g4c_mlp_io_t), **kw)


REC_SQ_ERR, REC_ABS_ERR, REC_MAX_ABS_ERR, REC_TGT_SUM, REC_TGT_SQ_SUM, REC_ABS_ERR_MASK, REC_NSTAT = range(7)     # G4C_REC_*
REC_MAX_NF = 8                                      # widest prediction g4c_rollout_advance_record forms statistics of


class g4c_rollout_rec_t(C.Structure):
    _fields_ = [("max_steps", C.c_int32), ("snap", C.c_void_p), ("every", C.c_int32), ("n_snap", C.c_int32),
                ("probe_rows", C.c_void_p), ("n_probe", C.c_int32), ("probe_out", C.c_void_p),
                ("target", C.c_void_p), ("target_ld", C.c_int32), ("mask", C.c_void_p), ("stats", C.c_void_p),
                ("scratch", C.c_void_p)]


class g4c_rollout_moments_t(C.Structure):
    _fields_ = [("max_steps", C.c_int32), ("stride", C.c_int32), ("window", C.c_void_p), ("sub", C.c_void_p), ("sub_ld", C.c_int32),
                ("plane_ld", C.c_int64), ("pivot", C.c_void_p), ("sum", C.c_void_p), ("sum2", C.c_void_p), ("lo", C.c_void_p),
                ("hi", C.c_void_p)]


SPECTRUM_MAX_BINS = 64                              # most frequencies g4c_rollout_spectrum accumulates


class g4c_rollout_spectrum_t(C.Structure):
    _fields_ = [("max_steps", C.c_int32), ("stride", C.c_int32), ("n_samples", C.c_int32), ("n_bins", C.c_int32), ("window", C.c_void_p),
                ("tw", C.c_void_p), ("x_ld", C.c_int32), ("x_step", C.c_int32), ("plane_ld", C.c_int64), ("pivot", C.c_void_p),
                ("sum", C.c_void_p), ("re", C.c_void_p), ("im", C.c_void_p)]


WELCH_MAX_TRACK = 1024                              # most tracked rows g4c_rollout_welch keeps the per-segment power of


class g4c_rollout_welch_t(C.Structure):
    _fields_ = [("max_steps", C.c_int32), ("stride", C.c_int32), ("seg_len", C.c_int32), ("hop", C.c_int32), ("n_bins", C.c_int32),
                ("x_ld", C.c_int32), ("x_step", C.c_int32), ("ref_row", C.c_int32), ("ref_field", C.c_int32), ("n_track", C.c_int32),
                ("max_segments", C.c_int32), ("window", C.c_void_p), ("tw", C.c_void_p), ("W", C.c_void_p), ("inv_L", C.c_double),
                ("plane_ld", C.c_int64), ("pivot", C.c_void_p), ("sum", C.c_void_p), ("re", C.c_void_p), ("im", C.c_void_p),
                ("pxx", C.c_void_p), ("cxr_re", C.c_void_p), ("cxr_im", C.c_void_p), ("ref_sum", C.c_void_p), ("ref_re", C.c_void_p),
                ("ref_im", C.c_void_p), ("track", C.c_void_p), ("track_host", C.c_void_p), ("seg_power", C.c_void_p)]


DERIVED_MAX_COLS, DERIVED_MAX_TERMS = 8, 3         # G4C_DERIVED_MAX_COLS / _TERMS
JET_MAX_FIELDS = 4                                  # G4C_JET_MAX_FIELDS
DERIVED_SQ, DERIVED_ABS, DERIVED_MAX_ABS, DERIVED_NSTAT = range(4)     # G4C_DERIVED_*


class g4c_derived_program_t(C.Structure):
    _fields_ = [("nd", C.c_int32), ("n_terms", C.c_int32 * DERIVED_MAX_COLS),
                ("field", (C.c_int32 * DERIVED_MAX_TERMS) * DERIVED_MAX_COLS), ("axis", (C.c_int32 * DERIVED_MAX_TERMS) * DERIVED_MAX_COLS),
                ("coef", (C.c_float * DERIVED_MAX_TERMS) * DERIVED_MAX_COLS)]


class g4c_mesh_derived_t(C.Structure):
    _fields_ = [("dim", C.c_int32), ("nf", C.c_int32), ("x_ld", C.c_int32), ("g", C.c_void_p), ("src", C.c_void_p), ("off", C.c_void_p),
                ("cur", C.c_void_p), ("step", C.c_void_p), ("every", C.c_int32), ("n_snap", C.c_int32), ("max_steps", C.c_int32),
                ("snap", C.c_void_p), ("stats", C.c_void_p), ("scratch", C.c_void_p)]


FORCES_FPX, FORCES_FPY, FORCES_FVX, FORCES_FVY, FORCES_MP, FORCES_MV, FORCES_NSUM = range(7)     # G4C_FORCES_*


class g4c_body_forces_t(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_ld", C.c_int32), ("x_step", C.c_int32), ("step", C.c_void_p), ("t0", C.c_int32),
                ("pcol", C.c_int32), ("ucol", C.c_int32), ("vcol", C.c_int32), ("mu", C.c_double), ("p_scale", C.c_double),
                ("p_shift", C.c_double), ("u_scale", C.c_double), ("v_scale", C.c_double), ("g", C.c_void_p), ("src", C.c_void_p),
                ("off", C.c_void_p), ("item", C.c_void_p), ("body_off", C.c_void_p), ("area", C.c_void_p), ("unit", C.c_void_p),
                ("arm", C.c_void_p), ("stats", C.c_void_p), ("cur", C.c_void_p), ("wall", C.c_void_p), ("max_steps", C.c_int32)]


class g4c_body_forces_adjoint_t(C.Structure):
    _fields_ = [("gF", C.c_void_p), ("gwall", C.c_void_p), ("nf", C.c_int32), ("pcol", C.c_int32), ("ucol", C.c_int32), ("vcol", C.c_int32),
                ("mu", C.c_double), ("p_scale", C.c_double), ("u_scale", C.c_double), ("v_scale", C.c_double), ("g", C.c_void_p),
                ("off", C.c_void_p), ("item_body", C.c_void_p), ("area", C.c_void_p), ("unit", C.c_void_p), ("arm", C.c_void_p),
                ("own_off", C.c_void_p), ("own_item", C.c_void_p), ("in_off", C.c_void_p), ("in_item", C.c_void_p), ("in_g", C.c_void_p),
                ("hw", C.c_void_p), ("gx", C.c_void_p)]


SAMPLE_MAX_K = 16                                  # G4C_SAMPLE_MAX_K: most neighbours of a sample point (the grid search's limit)


class g4c_sample_points_t(C.Structure):
    _fields_ = [("idx", C.c_void_p), ("coef", C.c_void_p), ("k", C.c_int32), ("nf", C.c_int32), ("x_ld", C.c_int32), ("cur", C.c_void_p),
                ("step", C.c_void_p), ("every", C.c_int32), ("n_slots", C.c_int32), ("max_steps", C.c_int32), ("series", C.c_void_p)]


# g4c_tracer_advance (csrc/tracer.hip): the integration schemes and a particle's states
TRACER_EULER, TRACER_HEUN = 0, 1
TRACER_WAITING, TRACER_MOVING, TRACER_LEFT, TRACER_FAR, TRACER_NONFINITE = 0, 1, 2, 3, 4


class g4c_tracer_t(C.Structure):
    _fields_ = [("pos_sorted", C.c_void_p), ("order", C.c_void_p), ("cell_start", C.c_void_p), ("n_cells", C.c_int32 * 3),
                ("origin", C.c_float * 3), ("cell_size", C.c_float), ("dim", C.c_int32), ("k", C.c_int32), ("power", C.c_int32),
                ("x0", C.c_void_p), ("x1", C.c_void_p), ("x0_ld", C.c_int32), ("x1_ld", C.c_int32), ("vcol", C.c_int32 * 3),
                ("scale", C.c_float * 3), ("shift", C.c_float * 3), ("dt", C.c_float), ("scheme", C.c_int32), ("box_lo", C.c_float * 3),
                ("box_hi", C.c_float * 3), ("max_distance", C.c_float), ("step", C.c_void_p), ("t_host", C.c_int32),
                ("max_steps", C.c_int32), ("every", C.c_int32), ("n_slots", C.c_int32), ("series", C.c_void_p), ("q", C.c_void_p),
                ("status", C.c_void_p), ("stopped", C.c_void_p), ("release", C.c_void_p), ("vel", C.c_void_p)]


class g4c_periodic_grid_t(C.Structure):             # the cell grid of the periodic searches (csrc/knn_periodic.hip)
    _fields_ = [("n_cells", C.c_int32 * 3), ("origin", C.c_float * 3), ("period", C.c_float * 3), ("cell", C.c_double * 3)]


class g4c_tracer_periodic_t(C.Structure):
    _fields_ = [("base", g4c_tracer_t), ("period", C.c_float * 3), ("cell", C.c_double * 3)]


# g4c_voronoi_cells / g4c_weighted_integrals (csrc/control_volumes.hip)
VORONOI_MAX_VERTS = 32                             # G4C_VORONOI_MAX_VERTS
VORONOI_BOX, VORONOI_WALL, VORONOI_DUPLICATE, VORONOI_OVERFLOW = 1, 2, 4, 8     # G4C_VORONOI_*: bits of `flags`
INTEGRALS_MAX_ENTRIES = 8                          # G4C_INTEGRALS_MAX_ENTRIES


class g4c_voronoi_cells_t(C.Structure):
    _fields_ = [("pos_sorted", C.c_void_p), ("order", C.c_void_p), ("cell_start", C.c_void_p), ("n_cells", C.c_int32 * 3),
                ("origin", C.c_float * 3), ("cell_size", C.c_float), ("box_lo", C.c_double * 2), ("box_hi", C.c_double * 2),
                ("normals", C.c_void_p), ("area", C.c_void_p), ("centroid", C.c_void_p), ("nvert", C.c_void_p), ("flags", C.c_void_p),
                ("rings", C.c_void_p)]


class g4c_integral_program_t(C.Structure):
    _fields_ = [("ne", C.c_int32), ("a", C.c_int32 * INTEGRALS_MAX_ENTRIES), ("b", C.c_int32 * INTEGRALS_MAX_ENTRIES)]


class g4c_weighted_integrals_t(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_ld", C.c_int32), ("x_step", C.c_int32), ("sub", C.c_void_p), ("sub_ld", C.c_int32),
                ("sub_step", C.c_int32), ("nz", C.c_int32), ("w", C.c_void_p), ("step", C.c_void_p), ("t_host", C.c_int32),
                ("max_steps", C.c_int32), ("stats", C.c_void_p), ("scratch", C.c_void_p)]


class g4c_weighted_integrals_adjoint_t(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_ld", C.c_int32), ("x_step", C.c_int32), ("sub", C.c_void_p), ("sub_ld", C.c_int32),
                ("sub_step", C.c_int32), ("nz", C.c_int32), ("w", C.c_void_p), ("g", C.c_void_p), ("n_groups", C.c_int32),
                ("group", C.c_void_p), ("t_host", C.c_int32), ("max_steps", C.c_int32), ("gx", C.c_void_p), ("gx_ld", C.c_int32)]


# g4c_snapshot_* (csrc/snapshot_modes.hip): the envelope and the tile sizes the tests walk
SNAPSHOT_MAX_ROWS = 1024                           # G4C_SNAPSHOT_MAX_ROWS: Ma, Mb, R
SNAPSHOT_MAX_COLUMNS = 2 ** 31 - 1                 # G4C_SNAPSHOT_MAX_COLUMNS: L
SNAPSHOT_GRAM_BLOCK, SNAPSHOT_GRAM_CHUNK, SNAPSHOT_COMBINE_BLOCK = 64, 2048, 8


class g4c_snapshot_sel_t(C.Structure):
    _fields_ = [("rows", C.c_int32), ("first", C.c_int32), ("stride", C.c_int32), ("count", C.c_int32)]


_SIGNATURES = {
    "g4c_version": (C.c_int, []),
    "g4c_device_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "g4c_last_error": (C.c_char_p, []),
    "g4c_plan_csr": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "g4c_plan_pool_edge": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "g4c_plan_pool_edge_ordered": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "g4c_segment_reduce": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "g4c_weighted_segment_mean": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "g4c_mlp_pack_layer": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_int32, C.c_int32, C.c_void_p]),
    "g4c_mlp_run": (C.c_int, [C.POINTER(g4c_mlp_t), C.POINTER(g4c_src_t), C.c_int32, C.c_int64, C.POINTER(g4c_mlp_io_t), C.c_void_p]),
    "g4c_plan_tiles": (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]),
    "g4c_plan_row_ranges": (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "g4c_mlp_ws_grid": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "g4c_mlp_bx6i_enable": (C.c_int, [C.c_int]),
    "g4c_mlp_ws_enable": (C.c_int, [C.c_int]),
    "g4c_mlp_small_launch_tiles": (C.c_int, [C.c_int]),
    "g4c_layer_norm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "g4c_debug_mean_div": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "g4c_mlp_last_kernel": (C.c_int, []),
    "g4c_mlp_last_row_ranges": (C.c_int, []),
    "g4c_mlp_shapes_enable": (C.c_int, [C.c_int]),
    "g4c_mlp_last_shape": (C.c_int, []),
    "g4c_mlp_tile_form": (C.c_int, [C.c_int]),
    "g4c_mlp_last_tile_rows": (C.c_int, []),
    "g4c_project_to_edges": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                       C.c_void_p, C.c_int32, C.c_void_p]),
    "g4c_edge_scalar_to_node_vector": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int32,
                                                 C.c_void_p, C.c_int32, C.c_void_p]),
    "g4c_knn_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                               C.c_void_p, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]),
    "g4c_knn_grid_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "g4c_knn_grid_periodic": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(g4c_periodic_grid_t), C.c_int32,
                                        C.c_void_p, C.c_void_p]),
    "g4c_knn_grid_query_periodic": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(g4c_periodic_grid_t),
                                              C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "g4c_rollout_advance": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                      C.c_void_p, C.c_int64, C.c_void_p]),
    "g4c_rollout_record_scratch_doubles": (C.c_int64, [C.c_int64, C.c_int32]),
    "g4c_rollout_advance_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(g4c_rollout_rec_t),
                                             C.c_void_p, C.c_int64, C.c_void_p]),
    "g4c_rollout_moments": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(g4c_rollout_moments_t), C.c_void_p, C.c_int64, C.c_void_p]),
    "g4c_rollout_spectrum": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(g4c_rollout_spectrum_t), C.c_void_p, C.c_int64, C.c_void_p]),
    "g4c_rollout_welch": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(g4c_rollout_welch_t), C.c_void_p, C.c_int64, C.c_void_p]),
    "g4c_mesh_gradient_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "g4c_mesh_derived_scratch_doubles": (C.c_int64, [C.c_int64, C.c_int32]),
    "g4c_mesh_derived": (C.c_int, [C.c_void_p, C.POINTER(g4c_mesh_derived_t), C.POINTER(g4c_derived_program_t), C.c_int64, C.c_void_p]),
    "g4c_mesh_derived_adjoint": (C.c_int, [C.c_void_p, C.POINTER(g4c_derived_program_t), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "g4c_mesh_jet_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "g4c_mesh_jet": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(g4c_derived_program_t),
                               C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "g4c_mesh_jet_adjoint": (C.c_int, [C.c_void_p, C.POINTER(g4c_derived_program_t), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "g4c_body_forces": (C.c_int, [C.POINTER(g4c_body_forces_t), C.c_int64, C.c_int64, C.c_void_p]),
    "g4c_body_forces_adjoint": (C.c_int, [C.POINTER(g4c_body_forces_adjoint_t), C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "g4c_sample_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "g4c_sample_weights_periodic": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "g4c_sample_points": (C.c_int, [C.c_void_p, C.POINTER(g4c_sample_points_t), C.c_int64, C.c_int64, C.c_void_p]),
    "g4c_sample_points_adjoint": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                            C.c_void_p]),
    "g4c_tracer_advance": (C.c_int, [C.POINTER(g4c_tracer_t), C.c_int64, C.c_int64, C.c_void_p]),
    "g4c_tracer_advance_periodic": (C.c_int, [C.POINTER(g4c_tracer_periodic_t), C.c_int64, C.c_int64, C.c_void_p]),
    "g4c_voronoi_cells": (C.c_int, [C.POINTER(g4c_voronoi_cells_t), C.c_int64, C.c_void_p]),
    "g4c_weighted_integrals_scratch_doubles": (C.c_int64, [C.c_int64, C.c_int32]),
    "g4c_weighted_integrals": (C.c_int, [C.POINTER(g4c_weighted_integrals_t), C.POINTER(g4c_integral_program_t), C.c_int64, C.c_void_p]),
    "g4c_weighted_integrals_adjoint": (C.c_int, [C.POINTER(g4c_weighted_integrals_adjoint_t), C.POINTER(g4c_integral_program_t), C.c_int64,
                                                 C.c_void_p]),
    "g4c_snapshot_mean": (C.c_int, [C.c_void_p, C.POINTER(g4c_snapshot_sel_t), C.c_int64, C.c_void_p, C.c_void_p]),
    "g4c_snapshot_gram_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "g4c_snapshot_gram": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(g4c_snapshot_sel_t), C.c_void_p, C.c_void_p, C.POINTER(g4c_snapshot_sel_t),
                                    C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "g4c_snapshot_combine": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(g4c_snapshot_sel_t), C.c_void_p, C.c_int64, C.c_int32, C.c_int64,
                                       C.c_void_p, C.c_void_p]),
    "g4c_activation_inplace": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "g4c_add_cols": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                               C.c_int32, C.c_int64, C.c_void_p]),
    "g4c_copy_cols": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                C.c_int32, C.c_int64, C.c_void_p]),
    # training path (train_ops.hip)
    "g4c_train_gather": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                   C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_void_p]),
    "g4c_act_grad": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                               C.c_int32, C.c_int64, C.c_void_p]),
    "g4c_act_grad_ref16": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                     C.c_int32, C.c_int64, C.c_void_p]),
    "g4c_layernorm_grad_partials": (C.c_int32, [C.c_int64]),
    "g4c_layernorm_grad": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                     C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_void_p]),
    "g4c_layernorm_grad_z16": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                         C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_void_p]),
    "g4c_colsum_partials": (C.c_int32, [C.c_int64]),
    "g4c_colsum": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "g4c_weight_grad_partials": (C.c_int32, [C.c_int64]),
    "g4c_weight_grad_scratch_floats": (C.c_int64, [C.c_int64]),
    "g4c_weight_grad": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                  C.c_void_p]),
    "g4c_weight_grad_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_void_p]),
    "g4c_weight_grad_bf16_a16": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_void_p]),
    "g4c_segment_broadcast": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_int32, C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def load() -> C.CDLL:
    """Load libg4c.so (built in-tree by `__graft_entry__.build()` / `make -C graphs4cfd_amd/csrc`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"graphs4cfd_amd: HIP library not found at {LIB_PATH}. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)   # AttributeError if the library does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(code: int) -> None:
    if code == OK:
        return
    msg = load().g4c_last_error().decode("utf-8", "replace")
    if code == EINVAL:
        raise ValueError(msg)
    if code == EUNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError(msg)


def require_hip(*tensors: torch.Tensor) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("graphs4cfd_amd kernels run on an MI355X (HIP) device only; got a tensor on "
                               f"'{t.device}'. Move the model and Graph to 'cuda' (there is no CPU fallback).")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} and {t.device}")
    return dev


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def stream_handle(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream
