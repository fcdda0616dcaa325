"""ctypes binding of libdgll_hip.so (the C ABI declared in include/dgll_hip.h).

There is no fallback: if the library is missing and cannot be built, importing dgll_amd raises.  The
in-tree location (dgll_amd/lib/libdgll_hip.so) is deliberate -- the driver records which in-tree .so
files the test processes mapped.
"""
import contextlib
import ctypes as C
import os

# torch bundles its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  It must be mapped BEFORE
# libdgll_hip.so so that the library's NEEDED libamdhip64.so.7 binds to that same runtime; loaded the other way
# round the process ends up with two HIP runtimes and the second one sees no device.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdgll_hip.so")

OK = 0
F32, BF16 = 0, 1
REDUCE_SUM, REDUCE_MEAN = 0, 1
EPI_NONE, EPI_BIAS, EPI_RELU = 0, 1, 2


class BatchLoad(C.Structure):
    """include/dgll_hip.h: struct dgll_batch_load (dgll_hip_load_sampled_batch)."""
    _fields_ = [("staged_host", C.c_void_p), ("staged_entries", C.c_int64), ("staged_dev", C.c_void_p),
                ("pos_host", C.c_void_p), ("n_outer", C.c_int64), ("pos_bytes", C.c_int), ("pos_dev", C.c_void_p),
                ("indptr", C.c_void_p), ("indices", C.c_void_p),
                ("n_hops", C.c_int), ("rows", C.c_int64 * 8), ("seeds_off", C.c_int64), ("src_off", C.c_int64 * 8), ("ptr_off", C.c_int64 * 8),
                ("cache", C.c_void_p), ("ldc", C.c_int64), ("host", C.c_void_p), ("ldh", C.c_int64), ("slot", C.c_void_p),
                ("host_map", C.c_void_p), ("feat", C.c_int), ("dtype", C.c_int), ("miss_count", C.c_void_p),
                ("feat_out", C.c_void_p * 8), ("ld_feat", C.c_int64),
                ("reduced_out", C.c_void_p), ("ld_reduced", C.c_int64), ("reduce", C.c_int),
                ("ids_out", C.c_void_p),
                ("rowptr_out", C.c_void_p * 8), ("rowptr_cap", C.c_int64 * 8),
                ("labels", C.c_void_p), ("labels_out", C.c_void_p), ("labels_cap", C.c_int64), ("label_fill", C.c_int64),
                ("stage_map", C.c_void_p), ("stage_rows", C.c_void_p), ("ld_stage", C.c_int64), ("stage_cap", C.c_int64),
                ("stage_list", C.c_void_p), ("stage_count", C.c_void_p), ("stage_serial", C.c_uint), ("stage_blocks", C.c_int),
                ("upload_blocks", C.c_int)]


class SpmmChoice(C.Structure):
    """include/dgll_hip.h: struct dgll_spmm_choice (dgll_hip_debug_spmm_choice)."""
    _fields_ = [(n, C.c_int) for n in ("kernel", "epv", "lpr", "spr", "unroll", "prefetch", "rows_per_wave", "grid_y")] + \
               [("row_blocks", C.c_int64), ("chunk_blocks", C.c_int64)]


class GatChoice(C.Structure):
    """include/dgll_hip.h: struct dgll_gat_choice (dgll_hip_debug_gat_choice)."""
    _fields_ = [(n, C.c_int) for n in ("generation", "kind", "trow", "drop", "inrow", "epv", "lpr", "nh", "lph", "unroll", "grid_y",
                                       "rows_per_wave", "finalize", "error")] + \
               [("row_blocks", C.c_int64), ("chunk_blocks", C.c_int64), ("message", C.c_char_p)]


class TransformChoice(C.Structure):
    """include/dgll_hip.h: struct dgll_transform_choice (dgll_hip_debug_transform_choice)."""
    _fields_ = [(n, C.c_int) for n in ("kernel", "nt", "ntw", "nc", "cs", "colsplit", "epi", "dual", "rows_per_block", "lds_bytes",
                                       "per_cu", "bits_in_epilogue", "error")] + \
               [("workgroups", C.c_int64), ("row_sequences", C.c_int64), ("n_blocks", C.c_int64), ("message", C.c_char_p)]


class GatDesc(C.Structure):
    """include/dgll_hip.h: struct dgll_gat_desc (dgll_hip_gat_pass)."""
    _fields_ = [("pass_", C.c_int), ("dtype", C.c_int), ("mode", C.c_int), ("apply_elu", C.c_int),
                ("plan", C.c_void_p), ("rowptr", C.c_void_p), ("col", C.c_void_p), ("perm", C.c_void_p), ("n_rows", C.c_int64),
                ("n_cols", C.c_int64), ("heads", C.c_int), ("fo", C.c_int), ("alpha", C.c_float),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("edge_scale", C.c_void_p),
                ("drop_p", C.c_double), ("drop_seed", C.c_void_p),
                ("h", C.c_void_p), ("ld_h", C.c_int64), ("out", C.c_void_p), ("ld_out", C.c_int64),
                ("grad_out", C.c_void_p), ("ld_grad_out", C.c_int64), ("dn", C.c_void_p), ("ld_dn", C.c_int64),
                ("grad_h", C.c_void_p), ("ld_grad_h", C.c_int64),
                ("row_score", C.c_void_p), ("col_score", C.c_void_p), ("col_score_stride", C.c_int), ("col_dd", C.c_void_p),
                ("attn1", C.c_void_p), ("attn2", C.c_void_p), ("grad_s_rows", C.c_void_p), ("rowsum", C.c_void_p), ("rowmax", C.c_void_p),
                ("dd", C.c_void_p), ("sd", C.c_void_p), ("sd_stride", C.c_int), ("grad_score", C.c_void_p), ("partial3", C.c_void_p),
                ("raw", C.c_int), ("accumulate", C.c_int), ("phase", C.c_int)]


GAT_FORWARD, GAT_ROWS, GAT_TRANSPOSED = 0, 1, 2
GAT_ROWS_STORED_FIRST, GAT_ROWS_STORED_FURTHER, GAT_ROWS_EXACT_ONLY = 0, 1, 3       # DGLL_GAT_ROWS_*: the rows pass's `phase`
GAT_ROWS_EXACT_FIRST, GAT_ROWS_EXACT_MIDDLE, GAT_ROWS_EXACT_LAST = 4, 5, 6


class Gatv2Desc(C.Structure):
    """include/dgll_hip.h: struct dgll_gatv2_desc (dgll_hip_gatv2_pass)."""
    _fields_ = [("pass_", C.c_int), ("dtype", C.c_int),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("n_rows", C.c_int64), ("n_cols", C.c_int64),
                ("heads", C.c_int), ("D", C.c_int), ("slope", C.c_float),
                ("xl", C.c_void_p), ("ld_xl", C.c_int64), ("xr", C.c_void_p), ("ld_xr", C.c_int64), ("attn", C.c_void_p),
                ("grad_out", C.c_void_p), ("ld_grad_out", C.c_int64), ("out", C.c_void_p), ("ld_out", C.c_int64),
                ("lse", C.c_void_p), ("lse_delta", C.c_void_p), ("dattn_part", C.c_void_p), ("dattn_blocks", C.c_int64), ("dattn", C.c_void_p)]


GATV2_FORWARD, GATV2_ROWS, GATV2_TRANSPOSED = 0, 1, 2
GATV2_LONG_ROW = 256        # DGLL_GATV2_LONG_ROW of include/dgll_hip.h


class AttnDesc(C.Structure):
    """include/dgll_hip.h: struct dgll_attn_desc (dgll_hip_sparse_attn_pass)."""
    _fields_ = [("pass_", C.c_int), ("dtype", C.c_int),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("n_rows", C.c_int64), ("n_cols", C.c_int64),
                ("heads", C.c_int), ("D", C.c_int), ("scale", C.c_float), ("kv_shared", C.c_int),
                ("q", C.c_void_p), ("ld_q", C.c_int64), ("k", C.c_void_p), ("ld_k", C.c_int64), ("v", C.c_void_p), ("ld_v", C.c_int64),
                ("grad_out", C.c_void_p), ("ld_grad_out", C.c_int64), ("out", C.c_void_p), ("ld_out", C.c_int64),
                ("out2", C.c_void_p), ("ld_out2", C.c_int64), ("lse", C.c_void_p), ("lse_delta", C.c_void_p)]


ATTN_FORWARD, ATTN_ROWS, ATTN_COLS = 0, 1, 2
ATTN_LONG_ROW = 256         # DGLL_ATTN_LONG_ROW of include/dgll_hip.h


class TypedDesc(C.Structure):
    """include/dgll_hip.h: struct dgll_typed_desc (dgll_hip_typed_spmm_pass)."""
    _fields_ = [("pass_", C.c_int), ("dtype", C.c_int),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("etype", C.c_void_p), ("norm", C.c_void_p),
                ("n_rows", C.c_int64), ("n_cols", C.c_int64), ("R", C.c_int), ("B", C.c_int), ("F", C.c_int64),
                ("coeff", C.c_void_p), ("x", C.c_void_p), ("ld_x", C.c_int64), ("dz", C.c_void_p), ("ld_dz", C.c_int64),
                ("out", C.c_void_p), ("ld_out", C.c_int64), ("p", C.c_void_p), ("ld_p", C.c_int64)]


TYPED_EXPAND, TYPED_CONTRACT, TYPED_EDGE_DOTS = 0, 1, 2
TYPED_LONG_ROW = 256        # DGLL_TYPED_LONG_ROW of include/dgll_hip.h
TYPED_COEFF_LDS = 4096      # DGLL_TYPED_COEFF_LDS: the coefficient table is staged in LDS up to this many entries (R * B)
TYPED_BASIS_BLOCK = 8       # DGLL_TYPED_BASIS_BLOCK: bases a launch block accumulates at the most


class MpDesc(C.Structure):
    """include/dgll_hip.h: struct dgll_mp_desc (dgll_hip_mp_pass)."""
    _fields_ = [("pass_", C.c_int), ("dtype", C.c_int),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("perm", C.c_void_p), ("n_rows", C.c_int64), ("n_cols", C.c_int64),
                ("nnz", C.c_int64), ("heads", C.c_int), ("D", C.c_int),
                ("e", C.c_void_p), ("ld_e", C.c_int64), ("e2", C.c_void_p), ("ld_e2", C.c_int64), ("e_out", C.c_void_p), ("ld_e_out", C.c_int64),
                ("x", C.c_void_p), ("ld_x", C.c_int64), ("y", C.c_void_p), ("ld_y", C.c_int64), ("out", C.c_void_p), ("ld_out", C.c_int64)]


MP_EDGE_SOFTMAX, MP_EDGE_SOFTMAX_BWD, MP_E_SUM, MP_U_ADD_V, MP_U_MUL_E_SUM, MP_U_DOT_V = range(6)
MP_LONG_ROW = 256           # DGLL_MP_LONG_ROW of include/dgll_hip.h


class MultiAggDesc(C.Structure):
    """include/dgll_hip.h: struct dgll_multi_agg_desc (dgll_hip_multi_agg_pass)."""
    _fields_ = [("pass_", C.c_int), ("dtype", C.c_int),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("n_rows", C.c_int64), ("n_cols", C.c_int64), ("F", C.c_int64),
                ("n_agg", C.c_int), ("agg", C.c_int * 6), ("n_scaler", C.c_int), ("scaler", C.c_int * 3), ("delta", C.c_float),
                ("x", C.c_void_p), ("ld_x", C.c_int64), ("y", C.c_void_p), ("ld_y", C.c_int64), ("out", C.c_void_p), ("ld_out", C.c_int64),
                ("grad_out", C.c_void_p), ("ld_grad_out", C.c_int64), ("stats", C.c_void_p), ("ld_stats", C.c_int64),
                ("arg", C.c_void_p), ("ld_arg", C.c_int64), ("coef", C.c_void_p), ("ld_coef", C.c_int64),
                ("grad_y", C.c_void_p), ("ld_grad_y", C.c_int64), ("grad_x", C.c_void_p), ("ld_grad_x", C.c_int64)]


MAGG_FORWARD, MAGG_ROWS, MAGG_COLS = 0, 1, 2
MAGG_MEAN, MAGG_SUM, MAGG_MAX, MAGG_MIN, MAGG_VAR, MAGG_STD = range(6)
MAGG_IDENTITY, MAGG_AMPLIFICATION, MAGG_ATTENUATION = 0, 1, 2
MAGG_LONG_ROW = 256         # DGLL_MAGG_LONG_ROW of include/dgll_hip.h


class EdgeFeatDesc(C.Structure):
    """include/dgll_hip.h: struct dgll_edge_feat_desc (dgll_hip_edge_feat_pass)."""
    _fields_ = [("pass_", C.c_int), ("dtype", C.c_int), ("op", C.c_int),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("perm", C.c_void_p), ("n_rows", C.c_int64), ("n_cols", C.c_int64),
                ("nnz", C.c_int64), ("F", C.c_int64), ("scale", C.c_void_p),
                ("x", C.c_void_p), ("ld_x", C.c_int64), ("e", C.c_void_p), ("ld_e", C.c_int64),
                ("grad_out", C.c_void_p), ("ld_grad_out", C.c_int64), ("out", C.c_void_p), ("ld_out", C.c_int64),
                ("grad_x", C.c_void_p), ("ld_grad_x", C.c_int64), ("grad_e", C.c_void_p), ("ld_grad_e", C.c_int64)]


EF_FORWARD, EF_COLS, EF_EDGE = 0, 1, 2
EF_ADD, EF_ADD_RELU, EF_MUL = 0, 1, 2
EF_LONG_ROW = 256           # DGLL_EF_LONG_ROW of include/dgll_hip.h


class GatedDesc(C.Structure):
    """include/dgll_hip.h: struct dgll_gated_desc (dgll_hip_gated_pass)."""
    _fields_ = [("pass_", C.c_int), ("dtype", C.c_int),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("perm", C.c_void_p), ("n_rows", C.c_int64), ("n_cols", C.c_int64),
                ("nnz", C.c_int64), ("F", C.c_int64), ("eps", C.c_float),
                ("a", C.c_void_p), ("ld_a", C.c_int64), ("b", C.c_void_p), ("ld_b", C.c_int64),
                ("c", C.c_void_p), ("ld_c", C.c_int64), ("v", C.c_void_p), ("ld_v", C.c_int64),
                ("out", C.c_void_p), ("ld_out", C.c_int64), ("ehat", C.c_void_p), ("ld_ehat", C.c_int64),
                ("inv_s", C.c_void_p), ("ld_inv_s", C.c_int64), ("out32", C.c_void_p), ("ld_out32", C.c_int64),
                ("grad_out", C.c_void_p), ("ld_grad_out", C.c_int64), ("grad_ehat", C.c_void_p), ("ld_grad_ehat", C.c_int64),
                ("grad_c", C.c_void_p), ("ld_grad_c", C.c_int64), ("grad_a", C.c_void_p), ("ld_grad_a", C.c_int64),
                ("w", C.c_void_p), ("ld_w", C.c_int64), ("grad_b", C.c_void_p), ("ld_grad_b", C.c_int64),
                ("grad_v", C.c_void_p), ("ld_grad_v", C.c_int64)]


GATED_FORWARD, GATED_ROWS, GATED_COLS = 0, 1, 2
GATED_LONG_ROW = 256        # DGLL_GATED_LONG_ROW of include/dgll_hip.h


class ResGatedDesc(C.Structure):
    """include/dgll_hip.h: struct dgll_res_gated_desc (dgll_hip_res_gated_pass)."""
    _fields_ = [("pass_", C.c_int), ("dtype", C.c_int),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("n_rows", C.c_int64), ("n_cols", C.c_int64),
                ("F", C.c_int64), ("mean", C.c_int),
                ("k", C.c_void_p), ("ld_k", C.c_int64), ("q", C.c_void_p), ("ld_q", C.c_int64),
                ("v", C.c_void_p), ("ld_v", C.c_int64), ("grad_out", C.c_void_p), ("ld_grad_out", C.c_int64),
                ("out", C.c_void_p), ("ld_out", C.c_int64), ("grad_k", C.c_void_p), ("ld_grad_k", C.c_int64),
                ("grad_q", C.c_void_p), ("ld_grad_q", C.c_int64), ("grad_v", C.c_void_p), ("ld_grad_v", C.c_int64)]


RES_GATED_FORWARD, RES_GATED_ROWS, RES_GATED_COLS = 0, 1, 2
RES_GATED_LONG_ROW = 256    # DGLL_RES_GATED_LONG_ROW of include/dgll_hip.h


class EdgeProjDesc(C.Structure):
    """include/dgll_hip.h: struct dgll_edge_proj_desc (dgll_hip_edge_proj_pass)."""
    _fields_ = [("pass_", C.c_int), ("dtype", C.c_int), ("op", C.c_int), ("De", C.c_int),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("perm", C.c_void_p), ("n_rows", C.c_int64), ("n_cols", C.c_int64),
                ("nnz", C.c_int64), ("F", C.c_int64), ("scale", C.c_void_p),
                ("x", C.c_void_p), ("ld_x", C.c_int64), ("a", C.c_void_p), ("ld_a", C.c_int64),
                ("weight", C.c_void_p), ("bias", C.c_void_p),
                ("grad_out", C.c_void_p), ("ld_grad_out", C.c_int64), ("out", C.c_void_p), ("ld_out", C.c_int64),
                ("grad_x", C.c_void_p), ("ld_grad_x", C.c_int64), ("grad_a", C.c_void_p), ("ld_grad_a", C.c_int64),
                ("dots_part", C.c_void_p), ("slabs", C.c_void_p), ("partials", C.c_int64)]


EFP_FORWARD, EFP_COLS, EFP_PARAM, EFP_DOTS = 0, 1, 2, 3
EFP_LONG_ROW = 256          # DGLL_EFP_LONG_ROW of include/dgll_hip.h
EFP_MAX_DE = 16             # DGLL_EFP_MAX_DE: the widest edge attribute row
EFP_MAX_PARTIALS = 512      # DGLL_EFP_MAX_PARTIALS: workgroups (and slabs) of the PARAM pass at the most


class GmmDesc(C.Structure):
    """include/dgll_hip.h: struct dgll_gmm_desc (dgll_hip_gmm_pass)."""
    _fields_ = [("pass_", C.c_int), ("dtype", C.c_int), ("K", C.c_int), ("dim", C.c_int),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("perm", C.c_void_p), ("n_rows", C.c_int64), ("n_cols", C.c_int64),
                ("nnz", C.c_int64), ("F", C.c_int64), ("scale", C.c_void_p),
                ("pseudo", C.c_void_p), ("ld_pseudo", C.c_int64), ("mu", C.c_void_p), ("inv_sigma", C.c_void_p),
                ("x", C.c_void_p), ("ld_x", C.c_int64), ("dz", C.c_void_p), ("ld_dz", C.c_int64),
                ("out", C.c_void_p), ("ld_out", C.c_int64), ("p", C.c_void_p), ("ld_p", C.c_int64),
                ("grad_pseudo", C.c_void_p), ("ld_grad_pseudo", C.c_int64), ("slabs", C.c_void_p), ("partials", C.c_int64)]


GMM_EXPAND, GMM_CONTRACT, GMM_PARAM = 0, 1, 2
GMM_LONG_ROW = 256          # DGLL_GMM_LONG_ROW of include/dgll_hip.h
GMM_MAX_DIM = 8             # DGLL_GMM_MAX_DIM: pseudo-coordinates of an entry at the most
GMM_MAX_KERNELS = 64        # DGLL_GMM_MAX_KERNELS: Gaussian kernels at the most
GMM_KERNEL_BLOCK = 8        # DGLL_GMM_KERNEL_BLOCK: kernels a launch block of EXPAND accumulates at the most
GMM_MAX_PARTIALS = 2048     # DGLL_GMM_MAX_PARTIALS: workgroups (and slabs) of the PARAM pass at the most


class SoftAggDesc(C.Structure):
    """include/dgll_hip.h: struct dgll_soft_agg_desc (dgll_hip_soft_agg_pass)."""
    _fields_ = [("pass_", C.c_int), ("dtype", C.c_int), ("mode", C.c_int), ("semi_grad", C.c_int),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("perm", C.c_void_p), ("n_rows", C.c_int64), ("n_cols", C.c_int64),
                ("nnz", C.c_int64), ("F", C.c_int64), ("eps", C.c_float), ("theta", C.c_void_p),
                ("x", C.c_void_p), ("ld_x", C.c_int64), ("e", C.c_void_p), ("ld_e", C.c_int64),
                ("grad_out", C.c_void_p), ("ld_grad_out", C.c_int64), ("out", C.c_void_p), ("ld_out", C.c_int64),
                ("stats", C.c_void_p), ("ld_stats", C.c_int64),
                ("grad_x", C.c_void_p), ("ld_grad_x", C.c_int64), ("grad_e", C.c_void_p), ("ld_grad_e", C.c_int64),
                ("partials", C.c_void_p), ("n_partials", C.c_int64), ("grad_theta", C.c_void_p)]


SOFT_AGG_FORWARD, SOFT_AGG_ROWS, SOFT_AGG_COLS = 0, 1, 2
SOFT_AGG_SOFTMAX, SOFT_AGG_POWER = 0, 1
SOFT_AGG_LONG_ROW = 256         # DGLL_SOFT_AGG_LONG_ROW of include/dgll_hip.h
SOFT_AGG_MAX_PARTIALS = 1024    # DGLL_SOFT_AGG_MAX_PARTIALS: workgroups per column block (and partials) of the ROWS pass at the most
KNN_MAX_K, KNN_MAX_D = 64, 256              # DGLL_KNN_MAX_K, DGLL_KNN_MAX_D: the limits of dgll_hip_knn
KNN_QUERY_TILE, KNN_CAND_TILE = 256, 32     # DGLL_KNN_QUERY_TILE, DGLL_KNN_CAND_TILE: its tile geometry


class DgllHipError(RuntimeError):
    pass


def _load():
    # Build when the library is missing or was built from different sources (content hash, not mtimes); hipcc
    # cross-compiles without a GPU.  A failed build raises: there is nothing to fall back to.
    from . import build as _build

    if not _build.is_current():
        _build.build()      # serialised across processes by a file lock; the library is linked to a temporary name and renamed
    if not os.path.exists(LIB_PATH):
        raise ImportError("libdgll_hip.so is missing (expected at %s); run `python -m dgll_amd.build`" % LIB_PATH)
    return C.CDLL(LIB_PATH)


lib = _load()

_vp, _i32, _i64, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t

# name -> (restype, argtypes); mirrors include/dgll_hip.h one to one (tests/test_abi.py checks the header)
SIGNATURES = {
    "dgll_hip_abi_version": (_i32, []),
    "dgll_hip_last_error": (C.c_char_p, []),
    "dgll_hip_device_info": (_i32, [_i32, C.c_char_p, _i32, C.POINTER(_i32), C.POINTER(_i64)]),
    "dgll_hip_debug_tune": (_i32, [_i32, _i32]),
    "dgll_hip_debug_spmm_choice": (_i32, [_i32, _i32, _i32, _i64, _i32, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dgll_hip_debug_gat_choice": (_i32, [_i32] * 17 + [_i64, _i32, _i64, _i64, _i64, _i64, _i32, _vp]),
    "dgll_hip_debug_transform_choice": (_i32, [_i32] * 12 + [_i64, _i32, _vp]),
    "dgll_hip_csr_plan_create": (_i32, [_vp, _vp, _i64, _i64, _i32, C.POINTER(_vp)]),
    "dgll_hip_csr_plan_destroy": (None, [_vp]),
    "dgll_hip_csr_plan_workspace_bytes": (_sz, [_vp, _i32]),
    "dgll_hip_csr_plan_num_long_rows": (_i64, [_vp]),
    "dgll_hip_csr_plan_num_chunks": (_i64, [_vp]),
    "dgll_hip_spmm_csr": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i32, _i32,
                                 _i32, _vp, _vp, _sz]),
    "dgll_hip_spmm_csr_ex": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i32, _i32,
                                    _i32, _vp, _vp, _sz, _vp, _i32]),
    "dgll_hip_spmm_csr_gated": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i32, _i32,
                                       _i32, _vp, _vp, _sz, _vp, _i32, _vp, _i64]),
    "dgll_hip_sage_fused_forward": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _i32,
                                           _vp, _i32, _vp, _i64, _i32, _vp, _i64, _i64, _i64, _vp, _sz]),
    "dgll_hip_sddmm_csr": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _i32]),
    "dgll_host_sampler_pool_create": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i32, C.c_uint64, C.c_uint64, _i32, _i32, _vp, _i64,
                                             _i64, _vp, _vp, _vp, _i32]),
    "dgll_host_sampler_pool_next": (_i32, [_vp, _vp, _vp]),
    "dgll_host_sampler_pool_release": (_i32, [_vp, _i32]),
    "dgll_host_sampler_pool_destroy": (_i32, [_vp]),
    "dgll_hip_gat_workspace_bytes": (_sz, [_vp, _i32, _i32]),
    "dgll_hip_gather_rows": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp]),
    "dgll_hip_pack_weight_bf16": (_i32, [_vp, _vp, _i32, _i64, _i64, _i32, _i32, _vp, _i64, _i32]),
    "dgll_hip_gather_rows_mapped": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp]),
    "dgll_hip_aggregate_rows_mapped": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "dgll_hip_translate_positions": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i32, _vp]),
    "dgll_hip_load_sampled_batch": (_i32, [_vp, _vp]),
    "dgll_hip_expand_rows": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _i32]),
    "dgll_host_sample_neighbors": (_i32, [_vp, C.POINTER(_i32), _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64,
                                          C.POINTER(_i64)]),
    "dgll_host_translate_neighbors": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "dgll_host_mt_seed": (_i32, [_vp, _i64, _vp, C.POINTER(_i32)]),
    "dgll_host_sample_batch_seeded": (_i32, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32]),
    "dgll_hip_adam_flat": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _i64,
                                  C.c_float, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dgll_hip_gemm_f32": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _i32]),
    "dgll_hip_mm_f32": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _i32, _vp, _i64]),
    "dgll_hip_mm2_f32": (_i32, [_vp, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _i32, _vp, _i64,
                                _vp, _i64]),
    "dgll_hip_grad_weight_f32_workspace": (_i64, [_i32, _i32, _i32]),
    "dgll_hip_grad_weight_f32": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _i64, _i32]),
    "dgll_hip_transform_bf16": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64, _vp,
                                       _i64, _i32, _i64, _i32, _i32, _vp]),
    "dgll_hip_transform_bf16_gated": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64,
                                             _vp, _i64, _i32, _i64, _i32, _i32, _vp, _vp, _i64, _vp]),
    "dgll_hip_transform_bf16_add": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64,
                                           _vp, _i64, _i32, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _i64]),
    "dgll_hip_transform_bf16_bits": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64, _i64, _i32,
                                            _i32, _vp, _vp, _i64, _vp, _i64, _vp, _i64]),
    "dgll_hip_transform_bf16_dual": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _i64, _i32]),
    "dgll_hip_grad_weight_workspace": (_i64, [_i32, _i32, _i32]),
    "dgll_hip_grad_weight_bf16": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64, _i32, _i64, _vp, _i64, _i32, _vp, _i64,
                                         _vp, _i64]),
    "dgll_hip_grad_weight_bf16_tr": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64, _i32, _i64, _vp, _i64, _i32, _vp, _i64,
                                            _vp, _i64]),
    "dgll_hip_softmax_xent": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _i32]),
    "dgll_hip_softmax_xent_soft": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i32]),
    "dgll_hip_softmax_xent_ex": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i32, _i32]),
    "dgll_hip_xent_reduce": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "launch_gcn_fused_kernel": (None, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32]),
    "launch_gcn_fused_kernel_backward_optimized": (None, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                                                          _i32, _i32]),
    "dgll_hip_gcn_fused_forward": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _sz]),
    "dgll_hip_gcn_fused_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "dgll_hip_segment_max": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i64, _i32]),
    "dgll_hip_segment_max_bwd": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i64, _i32]),
    "dgll_hip_lw_column_mass": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, C.c_uint32, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "dgll_hip_lw_column_p": (_i32, [_vp, _vp, _vp, _i64, _vp, _i32, _i32, _vp, _vp]),
    "dgll_hip_lw_ctrl_words": (_i64, []),
    "dgll_hip_lw_select": (_i32, [_vp, _vp, _vp, _i64, _vp, _i32, _i32, C.c_uint64, _i32, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "dgll_hip_lw_union_sorted": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, C.c_uint32, _vp, _vp, _vp, _vp]),
    "dgll_hip_lw_weights": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp]),
    "dgll_hip_lw_block_count": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, C.c_uint32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "dgll_hip_lw_block_fill": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, C.c_uint32, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp]),
    "dgll_host_philox4x32_10": (_i32, [_vp, _vp, _vp]),
    "dgll_hip_nb_sample": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _i32, C.c_uint64, _i32, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _i64, _vp, _vp]),
    "dgll_hip_nb_block": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp,
                                 _vp]),
    "dgll_hip_nb_max_fanout": (_i32, []),
    "dgll_hip_nb_sample_weighted": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i32, C.c_uint64, _i32, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _i64,
                                           _vp, _vp]),
    "dgll_hip_nb_long_row": (_i32, []),
    "dgll_hip_ep_draw": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _i32, _i32, _i32, C.c_uint64, _vp, C.c_uint32, _vp, _vp, _vp, _i64, _vp]),
    "dgll_hip_ep_compact": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    "dgll_hip_ep_exclude_count": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _vp]),
    "dgll_hip_ep_exclude_fill": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    "dgll_hip_pair_dot": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _vp, _i64, _vp]),
    "dgll_hip_pair_dot_bwd": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _i64]),
    "dgll_hip_sg_count": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, C.c_uint32, _vp, _vp]),
    "dgll_hip_sg_fill": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, C.c_uint32, _vp, _i64, _vp, _vp, _vp, _vp]),
    "dgll_hip_sg_long_row": (_i32, []),
    "dgll_hip_sg_draw": (_i32, [_vp, _vp, _vp, _i64, _i64, _i32, _i64, C.c_uint64, _vp, _vp, _vp, _vp]),
    "dgll_hip_sg_walk_nodes": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    "dgll_hip_sg_compact": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp]),
    "dgll_hip_random_walk": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _i32, C.c_uint64, C.c_uint64, C.c_double, C.c_double, _i32, _vp, _vp]),
    "dgll_host_node2vec_thresholds": (_i32, [C.c_double, C.c_double, _vp]),
    "dgll_hip_alias_build": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _sz, _vp, _vp]),
    "dgll_hip_random_walk_weighted": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i32, C.c_uint64, C.c_uint64, C.c_double, C.c_double, _i32,
                                             _vp, _vp]),
    "dgll_hip_struc_dtw": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _vp]),
    "dgll_hip_struc_dtw_max_rows": (_i32, []),
    "dgll_hip_struc_walk": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _i32, C.c_uint64, C.c_uint64, C.c_double, _i32, _vp, _vp,
                                   _vp]),
    "dgll_hip_sgns_negatives": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _i64, C.c_uint64, C.c_uint64, _vp]),
    "dgll_hip_sgns_step": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _i32, _i32, _vp, C.c_uint64, C.c_uint64, C.c_float,
                                  _vp, _vp, _vp, _vp]),
    "dgll_hip_louvain_move": (_i32, [_vp] * 10 + [_i64, _i64, _i64, C.c_double, _i64, C.c_uint64, C.c_uint32, C.c_uint32, _i32, _i32, _i32,
                                     _vp, _sz, _vp, _vp]),
    "dgll_hip_louvain_scratch_bytes": (_sz, [_i64, _i64]),
    "dgll_hip_leiden_refine": (_i32, [_vp] * 12 + [_i64, _i64, _i64, C.c_double, _i64, _i32, _i32, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "dgll_hip_gat_dropout_mask": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp, C.c_double, _vp]),
    "dgll_host_gat_dropout_mask": (_i32, [_vp, _vp, _i64, _i32, _vp, C.c_double, _vp]),
    "dgll_hip_gat_pass": (_i32, [_vp, C.POINTER(GatDesc)]),
    "dgll_hip_gatv2_pass": (_i32, [_vp, C.POINTER(Gatv2Desc)]),
    "dgll_hip_sparse_attn_pass": (_i32, [_vp, C.POINTER(AttnDesc)]),
    "dgll_hip_typed_spmm_pass": (_i32, [_vp, C.POINTER(TypedDesc)]),
    "dgll_hip_mp_pass": (_i32, [_vp, C.POINTER(MpDesc)]),
    "dgll_hip_multi_agg_pass": (_i32, [_vp, C.POINTER(MultiAggDesc)]),
    "dgll_hip_edge_feat_pass": (_i32, [_vp, C.POINTER(EdgeFeatDesc)]),
    "dgll_hip_gated_pass": (_i32, [_vp, C.POINTER(GatedDesc)]),
    "dgll_hip_res_gated_pass": (_i32, [_vp, C.POINTER(ResGatedDesc)]),
    "dgll_hip_edge_proj_pass": (_i32, [_vp, C.POINTER(EdgeProjDesc)]),
    "dgll_hip_gmm_pass": (_i32, [_vp, C.POINTER(GmmDesc)]),
    "dgll_hip_soft_agg_pass": (_i32, [_vp, C.POINTER(SoftAggDesc)]),
    "dgll_hip_knn": (_i32, [_vp, _vp, _i64, _i32, _i64, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64]),
}

for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == the library does not export a declared symbol
    _fn.restype = _res
    _fn.argtypes = _args


# ---- launch plumbing shared by the Python wrappers ---------------------------------------------------------------------------
# Every stream-taking entry point is called through `launch`: device current, raw stream, optional LaunchTimer bracket, the call,
# the error check under the name of the entry that ran.  From torch a launch needs the raw stream the caller is on and the guarantee
# that the tensor's device is current.  torch.cuda.current_stream() builds a Stream object (2-4 us) and `with torch.cuda.device(d)` a
# context object (3-4 us): of the ~25 us a launch costs through Python that is a third, and the consumer thread of the mini-batch
# pipeline issues ~80 launches per 2 ms batch.  `launch` uses their cheap cores (`raw_stream`, `on_device`) and builds a Stream
# object only for the events of an active timer.
_NULL_CTX = contextlib.nullcontext()


def raw_stream(device):
    """hipStream_t (an int) of torch's current stream on `device`."""
    idx = device.index
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if idx is None else idx)


def on_device(device):
    """Context that makes `device` current for the launch: a shared no-op object when it already is."""
    idx = device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NULL_CTX
    return torch.cuda.device(idx)


def ptr(t):
    """t.data_ptr(), None (a NULL argument) for None."""
    return None if t is None else t.data_ptr()


def pitch(t):
    """t.stride(0), the row pitch in elements; 0 for None."""
    return 0 if t is None else t.stride(0)


class LaunchTimer:
    """HIP-event timing of individual kernel launches on the stream they are issued on (bench.py's roofline leg).
    Usage: `with LaunchTimer() as t: ...steps...` then t.summary() -> {tag: (count, avg_ms)}."""
    active = None

    def __init__(self):
        self.records = []

    def __enter__(self):
        LaunchTimer.active = self
        return self

    def __exit__(self, *exc):
        LaunchTimer.active = None

    def start(self, tag, stream):
        """Record the opening event on `stream`; the caller records the returned closing event there after the launch."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        self.records.append((tag, a, b))
        return b

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for tag, a, b in self.records:
            n, tot = out.get(tag, (0, 0.0))
            out[tag] = (n + 1, tot + a.elapsed_time(b))
        return {k: (n, tot / n) for k, (n, tot) in out.items()}


def launch(name, device, *args, tag=None, stream=None):
    """lib.<name>(stream, *args) on `device`, checked.  stream: a torch stream, None = the current one of `device`.  tag: the launch's
    LaunchTimer key, or a zero-argument callable that builds it (called only while a timer is active)."""
    timer = LaunchTimer.active if tag is not None else None
    with on_device(device):
        raw = raw_stream(device) if stream is None else stream.cuda_stream
        if timer is None:
            code = getattr(lib, name)(raw, *args)
        else:
            on = torch.cuda.current_stream(device) if stream is None else stream
            end = timer.start(tag() if callable(tag) else tag, on)
            code = getattr(lib, name)(raw, *args)
            end.record(on)
    check(code, name)


def last_error():
    msg = lib.dgll_hip_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(code, what):
    if code != OK:
        raise DgllHipError("%s failed (code %d): %s" % (what, code, last_error()))


def device_info(device=0):
    name = C.create_string_buffer(64)
    cus, mem = _i32(0), _i64(0)
    check(lib.dgll_hip_device_info(device, name, 64, C.byref(cus), C.byref(mem)), "dgll_hip_device_info")
    return {"arch": name.value.decode(), "compute_units": cus.value, "global_mem_bytes": mem.value}
