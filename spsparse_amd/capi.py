"""ctypes binding of libspsparse_amd.so -- the C ABI in include/spsparse_amd.h.

Thin marshalling only: numpy arrays (host operands) or raw device pointers
(e.g. torch tensors' data_ptr()) go in, the library's result struct comes out.
There is no CPU fallback: if the shared library is missing or no MI355X is
visible this module raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPSAMD_LIB") or os.path.join(_HERE, "lib", "libspsparse_amd.so")    # SPSAMD_LIB: a developer variant build

LEAVE_ALONE, ADD, REPLACE = 0, 1, 2
MEM_HOST, MEM_DEVICE, MEM_PREPARED = 0, 1, 2
AS_A, AS_B = 1, 2
SINK_COO, SINK_DIGEST = 1, 2
SINK_ROWSTATS = 1
SINK_ORDERED = 2
SINK_PERMUTE = 4
SINK_EXACT_PATTERN = 8
SELECT_TRIL, SELECT_TRIU, SELECT_DIAG, SELECT_OFFDIAG, SELECT_ABS_GE, SELECT_ROW_REL, SELECT_ROW_TOPK = 1, 2, 3, 4, 5, 6, 7
SELECT_COMPLEMENT = 1
# ROW_TOPK: the longest row of the light (a wave per row) and of the mid (a workgroup per row, keys in LDS) kernel class
select_light_max, select_mid_max = 64, 4096
# extract: the longest output row of the light and of the mid ordering kernel class
extract_light_max, extract_mid_max = 64, 4096
REDUCE_SUM, REDUCE_SUM_ABS, REDUCE_SUM_SQ, REDUCE_MAX_ABS, REDUCE_COUNT, REDUCE_DIAG = 1, 2, 3, 4, 5, 6
POST_NONE, POST_RECIP, POST_SQRT, POST_RSQRT = 0, 1, 2, 3
# reduce: the longest row of the short rows' kernel class, and the values per row and step of the long rows' LDS tile
reduce_light_max, reduce_chunk = 64, 32
EMULT_TIMES, EMULT_FIRST = 1, 2
EMULT_COMPLEMENT = 1
# emult: the merged items per tile of the merge path, and the tuples per wave of the probe and compact kernels
emult_tile, emult_unit = 2048, 512
TRI_LOWER, TRI_UPPER = 0, 1
DIAG_NONUNIT, DIAG_UNIT = 0, 1
# solve_tri: the default of the solve_fuse_rows knob, the (row, rhs) pairs that also bound a thin level under that default,
# and the threads of a fused run's one workgroup; the analysis: the widest frontier the one-workgroup peel takes, and the
# launches of the wide peel between two looks at the frontier size
solve_fuse_rows, solve_fuse_work, solve_fused_threads = 256, 2048, 1024
peel_thin_max, peel_batch = 2048, 16
# factor_ilu0: the defaults of the factor_fuse_rows, factor_serial_work and factor_lds_row knobs, and the most the last
# may ask for
factor_fuse_rows, factor_serial_work, factor_lds_row, factor_lds_row_max = 256, 64, 256, 4096
# color: the orders, the flag, and the defaults of the color_fuse_rows and color_wave_deg knobs
COLOR_ORDER_HASH, COLOR_ORDER_DEGREE = 0, 1
COLOR_SYMMETRIC = 1
color_fuse_rows, color_wave_deg, color_fused_threads = 1024, 16, 1024
# aggregate: the orders, the flag, and the defaults of the agg_fuse_rows and agg_wave_deg knobs
AGG_ORDER_HASH, AGG_ORDER_DEGREE = 0, 1
AGG_SYMMETRIC = 1
agg_fuse_rows, agg_wave_deg = 1024, 32
# solve_pcg: the preconditioners, the stop reasons, the default of the pcg_check_every knob and the elements of one chunk of
# the dot products' fold
PRECOND_NONE, PRECOND_JACOBI, PRECOND_LU = 0, 1, 2
PCG_CONVERGED, PCG_MAXITER, PCG_BREAKDOWN = 0, 1, 2
pcg_check_every, pcg_chunk = 8, 1024
# solve_gmres: the largest restart length
GMRES_MAX_RESTART = 256
# amg_apply, solve_pcg_amg: the default of the amg_fuse_rows knob and the most levels of a hierarchy
amg_fuse_rows, amg_max_levels = 1024, 32

ERRORS = {-1: "EDIM", -2: "EINVAL", -3: "EHIP", -4: "ENOMEM", -5: "ECAPACITY", -6: "ENODEVICE", -7: "EPEER"}


class SpsamdError(RuntimeError):
    """A negative return code of the C ABI (the shim's (*spsparse_error)(-1, msg))."""

    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "?"), code, msg))
        self.code = code
        self.msg = msg


class Coo(C.Structure):
    _fields_ = [("idx0", C.c_void_p), ("idx1", C.c_void_p), ("val", C.c_void_p), ("nnz", C.c_size_t),
                ("shape0", C.c_size_t), ("shape1", C.c_size_t), ("sort0", C.c_int), ("mem", C.c_int)]


class Vec(C.Structure):
    _fields_ = [("idx", C.c_void_p), ("val", C.c_void_p), ("nnz", C.c_size_t), ("shape0", C.c_size_t),
                ("sort0", C.c_int), ("mem", C.c_int)]


class Result(C.Structure):
    _fields_ = [("shape0", C.c_uint64), ("shape1", C.c_uint64), ("nnz", C.c_uint64), ("products", C.c_uint64),
                ("nnz_a", C.c_uint64), ("nnz_b", C.c_uint64), ("sum", C.c_double), ("hash", C.c_uint64),
                ("idx0", C.c_void_p), ("idx1", C.c_void_p), ("val", C.c_void_p),
                ("row_nnz", C.c_void_p), ("row_sum", C.c_void_p),
                ("ms_consolidate", C.c_float), ("ms_symbolic", C.c_float), ("ms_numeric", C.c_float),
                ("ms_total", C.c_float), ("ms_light", C.c_float), ("ms_mid", C.c_float), ("ms_heavy", C.c_float),
                ("ms_dense", C.c_float), ("window", C.c_uint32), ("cells_hash", C.c_uint64), ("cells_dense", C.c_uint64), ("products_dense", C.c_uint64), ("workspace_bytes", C.c_uint64),
                ("rows_light", C.c_uint64), ("rows_mid", C.c_uint64), ("rows_heavy", C.c_uint64),
                ("products_light", C.c_uint64), ("products_mid", C.c_uint64), ("products_heavy", C.c_uint64),
                ("tuples_light", C.c_uint64), ("tuples_mid", C.c_uint64), ("tuples_heavy", C.c_uint64),
                ("ms_tiles", C.c_float), ("ms_direct", C.c_float), ("products_tiles", C.c_uint64), ("products_direct", C.c_uint64),
                ("row_hash", C.c_void_p)]


class StreamStats(C.Structure):
    _fields_ = [("blocks", C.c_uint64), ("block_tuples", C.c_uint64), ("max_block_nnz", C.c_uint64),
                ("device_output_bytes", C.c_uint64), ("ms_device", C.c_float), ("ms_callback", C.c_float),
                ("ms_wall", C.c_float)]


class SolveStats(C.Structure):
    _fields_ = [("levels", C.c_uint64), ("max_level_rows", C.c_uint64), ("launches", C.c_uint64),
                ("fused_levels", C.c_uint64), ("tuples_used", C.c_uint64), ("zero_pivot", C.c_int64),
                ("analysis_reused", C.c_uint32), ("ms_analysis", C.c_float), ("ms_solve", C.c_float),
                ("peel_thin_launches", C.c_uint64), ("peel_wide_launches", C.c_uint64)]


class FactorStats(C.Structure):
    _fields_ = [("levels", C.c_uint64), ("max_level_rows", C.c_uint64), ("launches", C.c_uint64),
                ("fused_levels", C.c_uint64), ("lookups", C.c_uint64), ("updates", C.c_uint64),
                ("zero_pivot", C.c_int64), ("missing_diag", C.c_int64),
                ("rows_serial", C.c_uint64), ("rows_wave", C.c_uint64), ("rows_block", C.c_uint64),
                ("analysis_reused", C.c_uint32), ("ms_analysis", C.c_float), ("ms_factor", C.c_float)]


class ColorStats(C.Structure):
    _fields_ = [("ncolors", C.c_uint64), ("rounds", C.c_uint64), ("adjacency", C.c_uint64), ("max_degree", C.c_uint64),
                ("conflicts", C.c_uint64), ("launches", C.c_uint64), ("fused_rounds", C.c_uint64),
                ("rows_thread", C.c_uint64), ("rows_wave", C.c_uint64), ("ms_adjacency", C.c_float), ("ms_color", C.c_float)]


class AggregateStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("naggregates", "rounds", "ring1", "ring2", "max_size", "min_size", "adjacency", "max_degree",
                                          "asymmetric", "launches", "fused_rounds", "rows_thread", "rows_wave")] + \
               [("ms_adjacency", C.c_float), ("ms_sweep", C.c_float), ("ms_assign", C.c_float)]


class PcgStats(C.Structure):
    _fields_ = [("iterations", C.c_uint64), ("reason", C.c_int32), ("bb", C.c_double), ("rr0", C.c_double), ("rr", C.c_double),
                ("launches", C.c_uint64), ("readbacks", C.c_uint64), ("analyses", C.c_uint32),
                ("ms_setup", C.c_float), ("ms_iterate", C.c_float)]


class AmgLevel(C.Structure):
    """spsamd_amg_level: op(A_l), and below the last level op(P_l) and op(R_l) (pointers to Coo structs the caller keeps alive)."""
    _fields_ = [("A", C.POINTER(Coo)), ("transpose_A", C.c_char), ("P", C.POINTER(Coo)), ("transpose_P", C.c_char),
                ("R", C.POINTER(Coo)), ("transpose_R", C.c_char)]


class AmgParams(C.Structure):
    _fields_ = [("pre", C.c_uint32), ("post", C.c_uint32), ("coarse", C.c_uint32), ("omega", C.c_double)]


class AmgStats(C.Structure):
    _fields_ = [("levels", C.c_uint32), ("fused_levels", C.c_uint32), ("launches_per_cycle", C.c_uint64),
                ("rows", C.c_uint64 * 32), ("nnz", C.c_uint64 * 32), ("operator_complexity", C.c_double),
                ("long_rows", C.c_uint64), ("ms_setup", C.c_float), ("ms_cycle", C.c_float)]


class DistStats(C.Structure):
    _fields_ = [("block_nnz_a", C.c_uint64), ("panel_tuples", C.c_uint64), ("remote_tuples", C.c_uint64),
                ("sent_tuples", C.c_uint64), ("ms_exchange", C.c_float), ("pad_", C.c_float)]


# spsamd_alltoallv_fn: (user, send**, sendbytes*, recv**, recvbytes*, world, stream)
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                           C.POINTER(C.c_size_t), C.c_int, C.c_void_p)

CHUNK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_size_t)

# every symbol include/spsparse_amd.h declares
SYMBOLS = ["spsamd_ctx_create", "spsamd_ctx_destroy", "spsamd_last_error", "spsamd_ctx_reserve", "spsamd_version", "spsamd_ctx_set_tuning",
           "spsamd_multiply", "spsamd_multiply_mv", "spsamd_result_fetch", "spsamd_result_scatter_dense", "spsamd_memcpy", "spsamd_consolidate", "spsamd_sorted_permutation",
           "spsamd_dim_beginnings", "spsamd_gen_rmat",
           "spsamd_gen_random_rows", "spsamd_gen_poisson2d", "spsamd_gen_laplace3d", "spsamd_gen_aggregation3d",
           "spsamd_dist_unique_id", "spsamd_dist_create", "spsamd_dist_destroy", "spsamd_dist_multiply",
           "spsamd_operand_prepare", "spsamd_operand_as_coo", "spsamd_operand_bytes", "spsamd_operand_destroy",
           "spsamd_multiply_dense", "spsamd_add", "spsamd_multiply_stream", "spsamd_multiply_masked",
           "spsamd_multiply_sampled", "spsamd_select", "spsamd_extract", "spsamd_reduce", "spsamd_emult", "spsamd_solve_tri",
           "spsamd_factor_ilu0", "spsamd_color", "spsamd_solve_pcg", "spsamd_aggregate",
           "spsamd_amg_apply", "spsamd_solve_pcg_amg", "spsamd_solve_bicgstab", "spsamd_solve_gmres"]

_lib = None


def load():
    """dlopen the library and declare prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libspsparse_amd.so is not built: run `python -m spsparse_amd.build` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    if os.environ.get("SPSAMD_NO_TORCH") != "1":
        # PyTorch wheels bundle their own HIP runtime under the same SONAME
        # (libamdhip64.so.7).  Two runtimes in one process cannot both own the
        # GPU, so when torch is installed it is imported FIRST: the loader then
        # binds this library to the runtime torch already brought in.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    L.spsamd_ctx_create.argtypes = [P(C.c_void_p), C.c_int, C.c_void_p]
    L.spsamd_ctx_destroy.argtypes = [C.c_void_p]
    L.spsamd_ctx_destroy.restype = None
    L.spsamd_last_error.argtypes = [C.c_void_p]
    L.spsamd_last_error.restype = C.c_char_p
    L.spsamd_ctx_reserve.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t]
    L.spsamd_version.restype = C.c_char_p
    L.spsamd_ctx_set_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    L.spsamd_multiply.argtypes = [C.c_void_p, C.c_double, P(Vec), P(Coo), C.c_char, P(Vec), P(Coo), C.c_char, P(Vec),
                                  C.c_int, C.c_int, C.c_int, C.c_int, P(Result)]
    L.spsamd_multiply_mv.argtypes = [C.c_void_p, C.c_double, P(Vec), P(Coo), C.c_char, P(Vec), P(Vec),
                                     C.c_int, C.c_int, C.c_int, C.c_int, P(Result)]
    L.spsamd_result_fetch.argtypes = [C.c_void_p, P(Result), CHUNK_FN, C.c_void_p]
    L.spsamd_result_scatter_dense.argtypes = [C.c_void_p, P(Result), C.c_void_p, C.c_size_t, C.c_int]
    L.spsamd_multiply_dense.argtypes = [C.c_void_p, P(Coo), C.c_char, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                        C.c_size_t, C.c_int, C.c_int, C.c_int]
    L.spsamd_add.argtypes = [C.c_void_p, C.c_double, P(Coo), C.c_char, C.c_double, P(Coo), C.c_char,
                             C.c_int, C.c_int, C.c_int, C.c_int, P(Result)]
    L.spsamd_multiply_stream.argtypes = [C.c_void_p, C.c_double, P(Vec), P(Coo), C.c_char, P(Vec), P(Coo), C.c_char, P(Vec),
                                         C.c_int, C.c_int, C.c_int, C.c_size_t, CHUNK_FN, C.c_void_p, P(Result),
                                         P(StreamStats)]
    L.spsamd_multiply_masked.argtypes = [C.c_void_p, C.c_double, P(Vec), P(Coo), C.c_char, P(Vec), P(Coo), C.c_char, P(Vec),
                                         P(Coo), C.c_int, C.c_int, C.c_int, C.c_int, P(Result)]
    L.spsamd_multiply_sampled.argtypes = [C.c_void_p, P(Coo), C.c_char, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                          C.c_size_t, C.c_double, C.c_double, C.c_void_p, C.c_int]
    L.spsamd_select.argtypes = [C.c_void_p, P(Coo), C.c_char, C.c_int, C.c_int64, C.c_double, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_int, P(Result)]
    L.spsamd_extract.argtypes = [C.c_void_p, P(Coo), C.c_char, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int,
                                 C.c_int, C.c_int, C.c_int, C.c_int, P(Result)]
    L.spsamd_reduce.argtypes = [C.c_void_p, P(Coo), C.c_char, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_size_t, C.c_int, P(C.c_size_t), P(Result)]
    L.spsamd_emult.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, P(Coo), C.c_char, P(Coo), C.c_char,
                               C.c_int, C.c_int, C.c_int, C.c_int, P(Result)]
    L.spsamd_solve_tri.argtypes = [C.c_void_p, P(Coo), C.c_char, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                   C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, P(SolveStats), P(Result)]
    L.spsamd_factor_ilu0.argtypes = [C.c_void_p, P(Coo), C.c_char, C.c_int, C.c_int, C.c_int, C.c_int, P(FactorStats), P(Result)]
    L.spsamd_color.argtypes = [C.c_void_p, P(Coo), C.c_char, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_size_t, C.c_int, P(C.c_size_t), P(ColorStats), P(Result)]
    L.spsamd_aggregate.argtypes = [C.c_void_p, P(Coo), C.c_char, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_size_t, C.c_int, P(C.c_size_t), P(AggregateStats), P(Result)]
    L.spsamd_solve_pcg.argtypes = [C.c_void_p, P(Coo), C.c_char, C.c_int, P(Coo), C.c_char, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_double, C.c_uint64, C.c_void_p, C.c_size_t, C.c_int, C.c_int, P(PcgStats), P(Result)]
    L.spsamd_solve_bicgstab.argtypes = L.spsamd_solve_pcg.argtypes
    L.spsamd_solve_gmres.argtypes = L.spsamd_solve_pcg.argtypes[:11] + [C.c_uint32] + L.spsamd_solve_pcg.argtypes[11:]
    L.spsamd_amg_apply.argtypes = [C.c_void_p, P(AmgLevel), C.c_size_t, P(AmgParams), C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_int, C.c_int, P(AmgStats), P(Result)]
    L.spsamd_solve_pcg_amg.argtypes = [C.c_void_p, P(AmgLevel), C.c_size_t, P(AmgParams), C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_double, C.c_uint64, C.c_void_p, C.c_size_t, C.c_int, C.c_int, P(PcgStats),
                                       P(AmgStats), P(Result)]
    L.spsamd_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.spsamd_consolidate.argtypes = [C.c_void_p, P(Coo), C.c_int, C.c_int, C.c_int, P(Result)]
    L.spsamd_sorted_permutation.argtypes = [C.c_void_p, P(Coo), C.c_int, C.c_void_p]
    L.spsamd_dim_beginnings.argtypes = [C.c_void_p, P(Coo), C.c_int, C.c_void_p, P(C.c_size_t)]
    L.spsamd_gen_rmat.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                  C.c_void_p, C.c_void_p, C.c_void_p]
    L.spsamd_gen_random_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    for name in ("spsamd_gen_poisson2d", "spsamd_gen_laplace3d", "spsamd_gen_aggregation3d"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.spsamd_dist_unique_id.argtypes = [C.c_char_p]
    L.spsamd_dist_create.argtypes = [P(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_void_p, ALLTOALLV_FN, C.c_void_p]
    L.spsamd_dist_destroy.argtypes = [C.c_void_p]
    L.spsamd_dist_destroy.restype = None
    L.spsamd_dist_multiply.argtypes = [C.c_void_p, C.c_double, P(Vec), P(Coo), C.c_char, P(Vec), P(Coo), C.c_char, P(Vec), C.c_void_p,
                                       C.c_int, C.c_int, C.c_int, C.c_int, P(Result), P(DistStats)]
    L.spsamd_operand_prepare.argtypes = [C.c_void_p, P(Coo), C.c_char, C.c_int, C.c_int, C.c_int, P(C.c_void_p)]
    L.spsamd_operand_as_coo.argtypes = [C.c_void_p, P(Coo)]
    L.spsamd_operand_bytes.argtypes = [C.c_void_p]
    L.spsamd_operand_bytes.restype = C.c_uint64
    L.spsamd_operand_destroy.argtypes = [C.c_void_p]
    L.spsamd_operand_destroy.restype = None
    _lib = L
    return L


def host_coo(idx0, idx1, val, shape, sort0=-1):
    """Coo struct over numpy arrays; returns (struct, keepalive)."""
    a0 = np.ascontiguousarray(idx0, dtype=np.int32)
    a1 = np.ascontiguousarray(idx1, dtype=np.int32)
    av = np.ascontiguousarray(val, dtype=np.float64)
    assert a0.shape == a1.shape == av.shape
    return Coo(a0.ctypes.data, a1.ctypes.data, av.ctypes.data, av.size, int(shape[0]), int(shape[1]), sort0, MEM_HOST), (a0, a1, av)


def device_coo(ptr0, ptr1, ptrv, nnz, shape, sort0=-1):
    return Coo(ptr0, ptr1, ptrv, nnz, int(shape[0]), int(shape[1]), sort0, MEM_DEVICE)


def result_operand(res):
    """A SINK_COO result as the device operand of the NEXT call on the same context (read in place:
    sorted row-major, each index once -- sort0 = 0, so it is trusted like Consolidate<> does)."""
    return Coo(res.idx0, res.idx1, res.val, int(res.nnz), int(res.shape0), int(res.shape1), 0, MEM_DEVICE)


def prolongator(agg, naggregates, device=False):
    """The tentative prolongator P (n x naggregates) of Context.aggregate's agg: (Coo, keepalive) with idx0 = 0 .. n - 1,
    idx1 = agg, val = 1.0 and sort0 = 0 -- sorted, one tuple per row, trusted as it stands.  agg: a numpy array, or an
    int32 torch tensor (kept where it is if on the device).  device: build the arrays with torch on cuda, else numpy."""
    n = int(agg.shape[0])
    if device or not isinstance(agg, np.ndarray):
        import torch
        a1 = torch.as_tensor(agg, dtype=torch.int32).to("cuda").contiguous()
        a0 = torch.arange(n, dtype=torch.int32, device=a1.device)
        av = torch.ones(n, dtype=torch.float64, device=a1.device)
        return device_coo(a0.data_ptr(), a1.data_ptr(), av.data_ptr(), n, (n, int(naggregates)), 0), (a0, a1, av)
    return host_coo(np.arange(n, dtype=np.int32), agg, np.ones(n), (n, int(naggregates)), 0)


def host_vec(idx, val, shape0, sort0=-1):
    a = np.ascontiguousarray(idx, dtype=np.int32)
    v = np.ascontiguousarray(val, dtype=np.float64)
    return Vec(a.ctypes.data, v.ctypes.data, v.size, int(shape0), sort0, MEM_HOST), (a, v)


def device_vec(ptr_idx, ptr_val, nnz, shape0, sort0=-1):
    """Vec struct over device memory (e.g. the sparse form of Context.reduce written into torch tensors): a scale vector
    or MV right-hand side that never leaves the device."""
    return Vec(ptr_idx, ptr_val, int(nnz), int(shape0), sort0, MEM_DEVICE)


class Context:
    """One device + stream + workspace (spsamd_ctx)."""

    def __init__(self, device=-1, stream=None):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.spsamd_ctx_create(C.byref(h), device, stream)
        if rc != 0:
            raise SpsamdError(rc, "spsamd_ctx_create failed (no MI355X visible?)")
        self.h = h

    def close(self):
        if self.h:
            self.L.spsamd_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise SpsamdError(rc, self.L.spsamd_last_error(self.h).decode())

    def set_tuning(self, name, value):
        """Developer knob (spsamd_ctx_set_tuning): selects between equivalent kernels, never changes a result."""
        self._check(self.L.spsamd_ctx_set_tuning(self.h, name.encode(), int(value)))

    def reserve(self, workspace_bytes=0, output_tuples=0):
        self._check(self.L.spsamd_ctx_reserve(self.h, workspace_bytes, output_tuples))

    def multiply(self, A, B, C_=1.0, scalei=None, tA='.', scalej=None, tB='.', scalek=None,
                 duplicate_policy=ADD, zero_nan=False, sink=SINK_COO, flags=0):
        """spsamd_multiply.  A, B: Coo structs; scale*: Vec structs or None."""
        res = Result()
        ptr = [None if s is None else C.byref(s) for s in (scalei, scalej, scalek)]
        rc = self.L.spsamd_multiply(self.h, float(C_), ptr[0], C.byref(A), tA.encode(), ptr[1], C.byref(B),
                                    tB.encode(), ptr[2], duplicate_policy, int(zero_nan), sink, flags, C.byref(res))
        self._check(rc)
        return res

    def multiply_masked(self, A, B, M, C_=1.0, scalei=None, tA='.', scalej=None, tB='.', scalek=None,
                        duplicate_policy=ADD, zero_nan=False, sink=SINK_COO, flags=0):
        """spsamd_multiply_masked: the tuples of multiply(A, B, ...) whose key is a key of M, bit for bit.  A, B, M: Coo
        structs (M in the product's orientation, its values never read); scale*: Vec structs or None."""
        res = Result()
        ptr = [None if s is None else C.byref(s) for s in (scalei, scalej, scalek)]
        rc = self.L.spsamd_multiply_masked(self.h, float(C_), ptr[0], C.byref(A), tA.encode(), ptr[1], C.byref(B),
                                           tB.encode(), ptr[2], C.byref(M), duplicate_policy, int(zero_nan), sink, flags,
                                           C.byref(res))
        self._check(rc)
        return res

    def multiply_stream(self, A, B, C_=1.0, scalei=None, tA='.', scalej=None, tB='.', scalek=None,
                        duplicate_policy=ADD, zero_nan=False, flags=0, block_tuples=0, on_chunk=None):
        """spsamd_multiply_stream: the product delivered in row blocks while it is computed.  on_chunk(i, j, v) gets
        numpy views of each chunk (valid during the call only: copy what you keep) and returns None / 0 to go on or a
        non-zero int to stop: the call then returns that value, raised as SpsamdError with that code.  An exception in
        on_chunk stops the delivery and is re-raised.  Returns (Result, StreamStats)."""
        if on_chunk is None:
            raise ValueError("on_chunk is required")
        res, stats = Result(), StreamStats()
        raised = []

        def cb(_user, pi, pj, pv, cnt):
            try:
                r = on_chunk(np.ctypeslib.as_array(pi, shape=(cnt,)), np.ctypeslib.as_array(pj, shape=(cnt,)),
                             np.ctypeslib.as_array(pv, shape=(cnt,)))
                return int(r or 0)
            except BaseException as e:                      # never let an exception cross the C boundary
                raised.append(e)
                return 1

        ptr = [None if s is None else C.byref(s) for s in (scalei, scalej, scalek)]
        fn = CHUNK_FN(cb)
        rc = self.L.spsamd_multiply_stream(self.h, float(C_), ptr[0], C.byref(A), tA.encode(), ptr[1], C.byref(B),
                                           tB.encode(), ptr[2], duplicate_policy, int(zero_nan), flags, int(block_tuples),
                                           fn, None, C.byref(res), C.byref(stats))
        if raised:
            raise raised[0]
        if rc > 0:
            raise SpsamdError(rc, "delivery stopped by on_chunk")
        self._check(rc)
        return res, stats

    def multiply_mv(self, A, V, C_=1.0, scalei=None, tA='.', scalej=None, duplicate_policy=ADD, zero_nan=False,
                    sink=SINK_COO, flags=0):
        """spsamd_multiply_mv.  A: Coo struct; V, scale*: Vec structs."""
        res = Result()
        ptr = [None if s is None else C.byref(s) for s in (scalei, scalej)]
        rc = self.L.spsamd_multiply_mv(self.h, float(C_), ptr[0], C.byref(A), tA.encode(), ptr[1], C.byref(V),
                                       duplicate_policy, int(zero_nan), sink, flags, C.byref(res))
        self._check(rc)
        return res

    def add(self, A, B, alpha=1.0, beta=1.0, tA='.', tB='.', duplicate_policy=ADD, zero_nan=False, sink=SINK_COO, flags=0):
        """spsamd_add: alpha * op(A) + beta * op(B), the reference's consolidate() of the two operands' scaled tuples
        appended (A's first).  A, B: Coo structs."""
        res = Result()
        rc = self.L.spsamd_add(self.h, float(alpha), C.byref(A), tA.encode(), float(beta), C.byref(B), tB.encode(),
                               duplicate_policy, int(zero_nan), sink, flags, C.byref(res))
        self._check(rc)
        return res

    def select(self, A, predicate, iparam=0, dparam=0.0, complement=False, transpose='.', duplicate_policy=ADD,
               zero_nan=False, sink=SINK_COO, flags=0):
        """spsamd_select: the tuples of op(A) that a SELECT_* predicate keeps (its complement: those it drops), in
        op(A)'s order, values untouched.  iparam: the diagonal d of TRIL / TRIU / DIAG / OFFDIAG or the k of ROW_TOPK;
        dparam: the theta of ABS_GE / ROW_REL.  A: a Coo struct."""
        res = Result()
        rc = self.L.spsamd_select(self.h, C.byref(A), transpose.encode(), int(predicate), int(iparam), float(dparam),
                                  SELECT_COMPLEMENT if complement else 0, duplicate_policy, int(zero_nan), sink, flags,
                                  C.byref(res))
        self._check(rc)
        return res

    def emult(self, op, A, B, tA='.', tB='.', alpha=1.0, complement=False, duplicate_policy=ADD, zero_nan=False,
              sink=SINK_COO, flags=0):
        """spsamd_emult: the tuples of op(A) whose key is a key of op(B) (complement: is not), in op(A)'s order.  op:
        EMULT_TIMES -- the value is (alpha * a) * b with b the first tuple of op(B) of that key -- or EMULT_FIRST -- a's own
        bits, B's values never read (B.val may be None).  complement goes with EMULT_FIRST only.  A, B: Coo structs."""
        res = Result()
        rc = self.L.spsamd_emult(self.h, int(op), EMULT_COMPLEMENT if complement else 0, float(alpha), C.byref(A), tA.encode(),
                                 C.byref(B), tB.encode(), duplicate_policy, int(zero_nan), sink, flags, C.byref(res))
        self._check(rc)
        return res

    def extract(self, A, rows=None, cols=None, transpose='.', duplicate_policy=ADD, zero_nan=False, sink=SINK_COO, flags=0):
        """spsamd_extract: the submatrix op(A)(rows, cols), values untouched, in (r, c, storage position) order.  rows, cols:
        None for every index of that dimension, or int32 index lists -- numpy arrays (host lists) or torch CUDA tensors
        (device lists), both of one kind; a list may be unordered and may repeat indices.  A: a Coo struct."""
        args = [_index_list(rows, "rows"), _index_list(cols, "cols")]
        mems = {m for _p, _n, m, _k in args if m is not None}
        if len(mems) > 1:
            raise ValueError("rows and cols must both be host (numpy) or both device (torch) lists")
        res = Result()
        rc = self.L.spsamd_extract(self.h, C.byref(A), transpose.encode(), args[0][0], args[0][1], args[1][0], args[1][1],
                                   mems.pop() if mems else MEM_HOST, duplicate_policy, int(zero_nan), sink, flags, C.byref(res))
        del args
        self._check(rc)
        return res

    def reduce(self, A, op, post=POST_NONE, transpose='.', duplicate_policy=ADD, zero_nan=False, dense=False, out=None,
               result=None):
        """spsamd_reduce: post(fold of every row of op(A)) -- REDUCE_* and POST_* -- bit for bit the serial loop over the
        row's tuples in op(A)'s order.  A: a Coo struct.  Without out: returns numpy arrays, (idx, val) of the rows that
        have a contributing tuple, or with dense=True val alone, one entry per row of op(A) (+0.0 where none contributes).
        With out: torch tensors on this context's device that receive the result -- (idx int32, val float64) for the sparse
        form, the float64 val alone (or (None, val)) for the dense form -- and the count is returned; a sparse out that is
        too small raises SpsamdError with code -5.  result: a capi.Result to fill (timings, rows by kernel class)."""
        nrow = int(A.shape1 if transpose == 'T' else A.shape0)
        cnt = C.c_size_t(0)
        rp = None if result is None else C.byref(result)

        def call(pi, pv, cap, mem):
            return self.L.spsamd_reduce(self.h, C.byref(A), transpose.encode(), int(op), int(post), duplicate_policy,
                                        int(zero_nan), pi, pv, cap, mem, C.byref(cnt), rp)

        if out is not None:
            oi, ov = out if isinstance(out, (tuple, list)) else (None, out)
            if dense and oi is not None:
                raise ValueError("the dense form takes the value tensor alone")
            pv, _ld, _n, mv = _dense_arg(ov, "out val", writable=True)
            if mv != MEM_DEVICE or ov.ndim != 1 or not ov.is_contiguous():
                raise ValueError("out val must be a contiguous 1-D float64 device tensor")
            cap, pi = int(ov.shape[0]), None
            if oi is not None:
                pi, ni, mi, _k = _index_list(oi, "out idx")
                if mi != MEM_DEVICE and ni:
                    raise ValueError("out idx must be a device tensor")
                cap = min(cap, ni)
                pi = oi.data_ptr()
            self._check(call(pi, pv, cap, MEM_DEVICE))
            return int(cnt.value)
        if dense:
            val = np.empty(nrow, np.float64)
            self._check(call(None, val.ctypes.data, nrow, MEM_HOST))
            return val
        cap = min(nrow, int(A.nnz)) if A.mem != MEM_PREPARED else nrow
        idx, val = np.empty(max(cap, 1), np.int32), np.empty(max(cap, 1), np.float64)
        self._check(call(idx.ctypes.data, val.ctypes.data, cap, MEM_HOST))
        return idx[:cnt.value].copy(), val[:cnt.value].copy()

    def consolidate(self, A, so0, duplicate_policy=ADD, zero_nan=False):
        res = Result()
        self._check(self.L.spsamd_consolidate(self.h, C.byref(A), so0, duplicate_policy, int(zero_nan), C.byref(res)))
        return res

    def sorted_permutation(self, A, so0):
        perm = np.zeros(A.nnz, dtype=np.uint64)
        self._check(self.L.spsamd_sorted_permutation(self.h, C.byref(A), so0, perm.ctypes.data))
        return perm

    def dim_beginnings(self, A, so0):
        out = np.zeros(A.nnz + 1, dtype=np.uint64)
        cnt = C.c_size_t(0)
        self._check(self.L.spsamd_dim_beginnings(self.h, C.byref(A), so0, out.ctypes.data, C.byref(cnt)))
        return out[:cnt.value]

    def fetch(self, res):
        """Host copy of a SINK_COO result through spsamd_result_fetch: (i, j, v)."""
        n = int(res.nnz)
        oi, oj, ov = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float64)
        pos = [0]

        def cb(_user, pi, pj, pv, cnt):
            o = pos[0]
            oi[o:o + cnt] = np.ctypeslib.as_array(pi, shape=(cnt,))
            if pj:                                                      # NULL for a rank-1 (MV) result
                oj[o:o + cnt] = np.ctypeslib.as_array(pj, shape=(cnt,))
            else:
                oj[o:o + cnt] = 0
            ov[o:o + cnt] = np.ctypeslib.as_array(pv, shape=(cnt,))
            pos[0] = o + cnt
            return 0

        self._check(self.L.spsamd_result_fetch(self.h, C.byref(res), CHUNK_FN(cb), None))
        assert pos[0] == n
        return oi, oj, ov

    def scatter_dense(self, res, dense_ptr, ld, duplicate_policy=ADD):
        """DenseAccum on the device: dense[i*ld + j] (+)= v for the tuples of a SINK_COO result."""
        self._check(self.L.spsamd_result_scatter_dense(self.h, C.byref(res), dense_ptr, ld, duplicate_policy))

    def multiply_dense(self, M, X, Y, transpose='.', duplicate_policy=ADD, handle_nan=False):
        """spsamd_multiply_dense: Y (op)= op(M) @ X, bit-identical to the reference's loop over M's tuples in storage
        order (multiply_dense.hpp:11-35, Y a DenseAccum).  M: a Coo struct.  X, Y: 2-D float64 numpy arrays (host) or
        float64 torch tensors on this context's device, rows contiguous (stride 1 along the right-hand sides); a 1-D
        X / Y is one right-hand side.  Y is updated in place."""
        (px, ldx, nx, mx), (py, ldy, ny, my) = _dense_arg(X, "X", writable=False), _dense_arg(Y, "Y", writable=True)
        if mx != my:
            raise ValueError("X and Y must both be host (numpy) or both device (torch) arrays")
        if nx != ny:
            raise ValueError("X has %d right-hand sides, Y %d" % (nx, ny))
        nrow, ncol = (M.shape1, M.shape0) if transpose == 'T' else (M.shape0, M.shape1)
        if _rows(X) != ncol or _rows(Y) != nrow:
            raise ValueError("X needs %d rows and Y %d rows for op(M) of shape (%d, %d)" % (ncol, nrow, nrow, ncol))
        self._check(self.L.spsamd_multiply_dense(self.h, C.byref(M), transpose.encode(), px, ldx, py, ldy, nx, mx,
                                                 duplicate_policy, int(handle_nan)))
        return Y

    def solve_tri(self, A, B, uplo=TRI_LOWER, diag=DIAG_NONUNIT, transpose='.', X=None, duplicate_policy=ADD, zero_nan=False,
                  stats=False, result=None):
        """spsamd_solve_tri: X with T @ X = B, T the `uplo` triangle of op(A) (the other triangle is skipped; under
        DIAG_UNIT the diagonal too), bit for bit the serial substitution loop of the header.  A: a Coo struct.  B, X: 2-D
        float64 numpy arrays (host) or float64 torch tensors on this context's device, rows contiguous; a 1-D B / X is one
        right-hand side.  X=None allocates it; X=B solves in place.  Returns X, or (X, SolveStats) with stats=True.
        result: a capi.Result to fill (timings)."""
        pb, ldb, nb, mb = _dense_arg(B, "B", writable=False)
        if X is None:
            if mb == MEM_HOST:
                X = np.empty(B.shape, dtype=np.float64)
            else:
                import torch
                X = torch.empty(tuple(B.shape), dtype=torch.float64, device=B.device)
        px, ldx, nx, mx = _dense_arg(X, "X", writable=True)
        if mx != mb:
            raise ValueError("B and X must both be host (numpy) or both device (torch) arrays")
        if nx != nb:
            raise ValueError("B has %d right-hand sides, X %d" % (nb, nx))
        n = int(A.shape1 if transpose == 'T' else A.shape0)
        if _rows(B) != n or _rows(X) != n:
            raise ValueError("B and X need %d rows" % n)
        st = SolveStats()
        self._check(self.L.spsamd_solve_tri(self.h, C.byref(A), transpose.encode(), int(uplo), int(diag), pb, ldb, px, ldx, nb,
                                            mb, duplicate_policy, int(zero_nan), C.byref(st),
                                            None if result is None else C.byref(result)))
        return (X, st) if stats else X

    def factor_ilu0(self, A, transpose='.', duplicate_policy=ADD, zero_nan=False, sink=SINK_COO, flags=0, stats=False):
        """spsamd_factor_ilu0: F = ILU(0) of op(A) on its own pattern, bit for bit the row-wise loop of the header -- L
        strictly below the diagonal (unit diagonal implied), U on and above it, S's keys in S's order.  A: a Coo struct
        whose op() is square and strictly ascending in (row, col) once taken.  Returns the Result like emult (chain it with
        result_operand, or prepare it and apply solve_tri(LOWER, UNIT) then solve_tri(UPPER, NONUNIT)), or
        (Result, FactorStats) with stats=True."""
        res, st = Result(), FactorStats()
        rc = self.L.spsamd_factor_ilu0(self.h, C.byref(A), transpose.encode(), duplicate_policy, int(zero_nan), sink, flags,
                                       C.byref(st), C.byref(res))
        self._check(rc)
        return (res, st) if stats else res

    def _graph_call(self, fn, stats_cls, names, A, order, seed, flags, transpose, out, stats, result):
        """What color and aggregate share: fn into `out` (device tensors named `names`: per-vertex ids, ordered list, bounds)
        or into host arrays of its own."""
        n = int(A.shape1 if transpose == 'T' else A.shape0)
        cnt, st = C.c_size_t(0), stats_cls()
        rp = None if result is None else C.byref(result)

        def call(pi, pl, pq, cap, mem):
            return fn(self.h, C.byref(A), transpose.encode(), int(order), int(seed) & 0xFFFFFFFF, int(flags),
                      pi, pl, pq, cap, mem, C.byref(cnt), C.byref(st), rp)

        if out is not None:
            oi, ol, oq = out
            if oi is None:
                raise ValueError("out %s is required" % names[0])
            ptrs, sizes = [], []
            for t, name in zip((oi, ol, oq), names):
                if t is None:
                    ptrs.append(None)
                    sizes.append(0)
                    continue
                _p, nt, mt, _k = _index_list(t, "out " + name)
                if mt != MEM_DEVICE and nt:
                    raise ValueError("out %s must be a device tensor" % name)
                ptrs.append(t.data_ptr())
                sizes.append(nt)
            if sizes[0] < n or (ol is not None and sizes[1] < n):
                raise ValueError("out %s and out %s need %d entries" % (names[0], names[1], n))
            self._check(call(ptrs[0], ptrs[1], ptrs[2], sizes[2], MEM_DEVICE))
            return (int(cnt.value), st) if stats else int(cnt.value)
        ids, lst, ptr = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.int32), np.empty(n + 1, np.int32)
        self._check(call(ids.ctypes.data, lst.ctypes.data, ptr.ctypes.data, n + 1, MEM_HOST))
        got = (ids[:n].copy(), lst[:n].copy(), ptr[:cnt.value + 1].copy())
        return got + (st,) if stats else got

    def color(self, A, order=COLOR_ORDER_HASH, seed=0, flags=0, transpose='.', out=None, stats=False, result=None):
        """spsamd_color: the greedy multi-colour ordering of op(A)'s graph, exactly the serial loop of the header.  A: a Coo
        struct whose op() is square (only its keys are read).  Without out: returns numpy int32 arrays (color, perm,
        color_ptr) -- perm the vertices ascending in (colour, index), the list to hand to extract as rows and cols;
        color_ptr the ncolors + 1 bounds of the colours in perm.  With out: contiguous 1-D int32 torch tensors on this
        context's device, (color, perm, color_ptr) with perm and color_ptr possibly None, that receive the result; the
        colour count is returned, and a color_ptr that is too small raises SpsamdError with code -5.  stats=True appends
        a ColorStats to what is returned.  result: a capi.Result to fill (timings)."""
        return self._graph_call(self.L.spsamd_color, ColorStats, ("color", "perm", "color_ptr"), A, order, seed, flags, transpose, out, stats, result)

    def aggregate(self, A, order=AGG_ORDER_HASH, seed=0, flags=0, transpose='.', out=None, stats=False, result=None):
        """spsamd_aggregate: the MIS(2) aggregates of op(A)'s graph, exactly the serial loop of the header.  A: a Coo struct
        whose op() is square (only its keys are read).  Without out: returns numpy int32 arrays (agg, members, agg_ptr) --
        members the vertices ascending in (aggregate, ring, index), agg_ptr the naggregates + 1 bounds of the aggregates in
        members.  With out: contiguous 1-D int32 torch tensors on this context's device, (agg, members, agg_ptr) with
        members and agg_ptr possibly None, that receive the result; the aggregate count is returned, and an agg_ptr that
        is too small raises SpsamdError with code -5.  stats=True appends an AggregateStats to what is returned.  result:
        a capi.Result to fill (timings).  prolongator(agg, naggregates) makes the tentative prolongator of the result."""
        return self._graph_call(self.L.spsamd_aggregate, AggregateStats, ("agg", "members", "agg_ptr"), A, order, seed, flags, transpose, out, stats, result)

    def solve_pcg(self, A, b, x=None, precond=PRECOND_NONE, M=None, transpose='.', transpose_M='.', tol=1e-8, max_iter=1000,
                  hist_capacity=None, duplicate_policy=ADD, zero_nan=False, result=None):
        """spsamd_solve_pcg: op(A) x = b by preconditioned conjugate gradients, bit for bit the loop of the header.  A, M:
        Coo structs (M with PRECOND_LU and only then: the spsamd_factor_ilu0 result, chained or prepared).  b, x: 1-D
        contiguous float64 numpy arrays (host) or float64 torch tensors on this context's device, n values each; x holds
        x0 and receives the iterate at the stop (x=None: a zero start, allocated here).  hist_capacity: the entries of the
        history to bring back (None: max_iter + 1; 0: none).  Returns (x, hist, PcgStats): hist a float64 numpy array of
        min(iterations + 1, hist_capacity) values of dot(r, r).  result: a capi.Result to fill (timings)."""
        return self._krylov(self.L.spsamd_solve_pcg, A, b, x, precond, M, transpose, transpose_M, tol, max_iter, hist_capacity,
                            duplicate_policy, zero_nan, result)

    def solve_bicgstab(self, A, b, x=None, precond=PRECOND_NONE, M=None, transpose='.', transpose_M='.', tol=1e-8,
                       max_iter=1000, hist_capacity=None, duplicate_policy=ADD, zero_nan=False, result=None):
        """spsamd_solve_bicgstab: op(A) x = b for an unsymmetric op(A) by right-preconditioned BiCGStab, bit for bit the loop
        of the header.  The arguments and the returned (x, hist, PcgStats) are solve_pcg's."""
        return self._krylov(self.L.spsamd_solve_bicgstab, A, b, x, precond, M, transpose, transpose_M, tol, max_iter,
                            hist_capacity, duplicate_policy, zero_nan, result)

    def solve_gmres(self, A, b, x=None, precond=PRECOND_NONE, M=None, transpose='.', transpose_M='.', tol=1e-8,
                    max_iter=1000, restart=30, hist_capacity=None, duplicate_policy=ADD, zero_nan=False, result=None):
        """spsamd_solve_gmres: op(A) x = b for an unsymmetric op(A) by right-preconditioned restarted GMRES(restart), bit
        for bit the loop of the header; CONVERGED is decided on the recomputed b - A x alone.  The other arguments and the
        returned (x, hist, PcgStats) are solve_pcg's: iterations counts Arnoldi steps, readbacks - 1 the cycles, and inside
        a cycle hist holds the estimate of dot(r, r), at a cycle's last step the true value."""
        return self._krylov(self.L.spsamd_solve_gmres, A, b, x, precond, M, transpose, transpose_M, tol, max_iter,
                            hist_capacity, duplicate_policy, zero_nan, result, (int(restart),))

    def _krylov(self, call, A, b, x, precond, M, transpose, transpose_M, tol, max_iter, hist_capacity, duplicate_policy,
                zero_nan, result, loop_args=()):
        """The arguments of solve_pcg / solve_bicgstab / solve_gmres as the C ABI takes them (loop_args: those a loop adds
        behind max_iter), the call, and what all return."""
        pb, _ldb, nb, mb = _dense_arg(b, "b", writable=False)
        if x is None:
            if mb == MEM_HOST:
                x = np.zeros(b.shape, dtype=np.float64)
            else:
                import torch
                x = torch.zeros(tuple(b.shape), dtype=torch.float64, device=b.device)
        px, _ldx, nx, mx = _dense_arg(x, "x", writable=True)
        if mx != mb:
            raise ValueError("b and x must both be host (numpy) or both device (torch) arrays")
        n = int(A.shape1 if transpose == 'T' else A.shape0)
        if b.ndim != 1 or x.ndim != 1 or nb != 1 or nx != 1 or _rows(b) != n or _rows(x) != n:
            raise ValueError("b and x must be 1-D arrays of %d values" % n)
        if n > 1 and (_ldb != 1 or _ldx != 1):
            raise ValueError("b and x must be contiguous")
        cap = int(max_iter) + 1 if hist_capacity is None else int(hist_capacity)
        hist = np.empty(max(cap, 1), np.float64)
        st = PcgStats()
        self._check(call(self.h, C.byref(A), transpose.encode(), int(precond), None if M is None else C.byref(M),
                         transpose_M.encode(), pb, px, mb, float(tol), int(max_iter), *loop_args, hist.ctypes.data if cap else None,
                         cap, duplicate_policy, int(zero_nan), C.byref(st), None if result is None else C.byref(result)))
        return x, hist[:min(int(st.iterations) + 1, cap)].copy(), st

    def _amg_args(self, levels, params, b, x, zero_x):
        """The level table, the parameters and the two vectors of amg_apply / solve_pcg_amg as the C ABI takes them."""
        levels = levels.levels if isinstance(levels, Hierarchy) else list(levels)
        arr = (AmgLevel * max(len(levels), 1))()
        for l, lv in enumerate(levels):
            A, tA, Pm, tP, Rm, tR = amg_level(*lv) if isinstance(lv, (tuple, list)) else lv
            arr[l] = AmgLevel(C.pointer(A), tA.encode(), None if Pm is None else C.pointer(Pm), tP.encode(),
                              None if Rm is None else C.pointer(Rm), tR.encode())
        prm = params if isinstance(params, AmgParams) else AmgParams(*params)
        pb, _ldb, nb, mb = _dense_arg(b, "b", writable=False)
        if x is None:
            if mb == MEM_HOST:
                x = np.zeros(b.shape, dtype=np.float64) if zero_x else np.empty(b.shape, dtype=np.float64)
            else:
                import torch
                x = torch.zeros(tuple(b.shape), dtype=torch.float64, device=b.device)
        px, _ldx, nx, mx = _dense_arg(x, "x", writable=True)
        if mx != mb:
            raise ValueError("b and x must both be host (numpy) or both device (torch) arrays")
        if b.ndim != 1 or x.ndim != 1 or nb != 1 or nx != 1 or _rows(b) != _rows(x):
            raise ValueError("b and x must be 1-D arrays of one length")
        if _rows(b) > 1 and (_ldb != 1 or _ldx != 1):
            raise ValueError("b and x must be contiguous")
        return arr, len(levels), prm, pb, px, mb, x, levels

    def amg_apply(self, levels, params, b, x=None, duplicate_policy=ADD, zero_nan=False, result=None):
        """spsamd_amg_apply: x = cycle(0, b), one multigrid cycle over `levels`, bit for bit the loop of the header.
        levels: a Hierarchy, or a list with one entry per level, each (A, P, R) or (A, tA, P, tP, R, tR) of Coo structs and
        transpose flags (P and R None on the last level; (A, P) passes P again as R with 'T').  params: an AmgParams or
        (pre, post, coarse, omega).  b, x: 1-D contiguous float64 numpy arrays or device torch tensors of n_0 values (x
        allocated when None).  Returns (x, AmgStats).  result: a capi.Result to fill (timings)."""
        arr, nl, prm, pb, px, mem, x, _keep = self._amg_args(levels, params, b, x, False)
        st = AmgStats()
        self._check(self.L.spsamd_amg_apply(self.h, arr, nl, C.byref(prm), pb, px, mem, duplicate_policy, int(zero_nan),
                                            C.byref(st), None if result is None else C.byref(result)))
        return x, st

    def solve_pcg_amg(self, levels, params, b, x=None, tol=1e-8, max_iter=1000, hist_capacity=None, duplicate_policy=ADD,
                      zero_nan=False, result=None):
        """spsamd_solve_pcg_amg: levels[0].A x = b by the loop of solve_pcg with z = cycle(0, r).  levels, params, b, x: as
        for amg_apply; x holds x0 and receives the iterate at the stop (None: a zero start).  Returns (x, hist, PcgStats,
        AmgStats) with hist as solve_pcg returns it."""
        arr, nl, prm, pb, px, mem, x, _keep = self._amg_args(levels, params, b, x, True)
        cap = int(max_iter) + 1 if hist_capacity is None else int(hist_capacity)
        hist = np.empty(max(cap, 1), np.float64)
        st, ast = PcgStats(), AmgStats()
        self._check(self.L.spsamd_solve_pcg_amg(self.h, arr, nl, C.byref(prm), pb, px, mem, float(tol), int(max_iter),
                                                hist.ctypes.data if cap else None, cap, duplicate_policy, int(zero_nan),
                                                C.byref(st), C.byref(ast), None if result is None else C.byref(result)))
        return x, hist[:min(int(st.iterations) + 1, cap)].copy(), st, ast

    def multiply_sampled(self, M, P, Q, out=None, transpose='.', alpha=1.0, beta=0.0):
        """spsamd_multiply_sampled: out[t] = alpha * (P[i] . Q[j]) (+ beta * v) for every tuple t = (i, j, v) of op(M) in
        storage order, the k terms of each summed serially in ascending order, bit for bit.  M: a Coo struct.  P, Q: 2-D
        float64 numpy arrays (host) or float64 torch tensors on this context's device, rows contiguous, with rows(op(M)) and
        cols(op(M)) rows of k values; a 1-D P / Q means k = 1.  out: one float64 per tuple of M (1-D, contiguous, the same
        kind as P and Q; it may be M's value array), allocated when None.  Returns out."""
        (pp, ldp, kp, mp), (pq, ldq, kq, mq) = _dense_arg(P, "P", writable=False), _dense_arg(Q, "Q", writable=False)
        if mp != mq:
            raise ValueError("P and Q must both be host (numpy) or both device (torch) arrays")
        if kp != kq:
            raise ValueError("P has rows of %d values, Q of %d" % (kp, kq))
        nrow, ncol = (M.shape1, M.shape0) if transpose == 'T' else (M.shape0, M.shape1)
        if _rows(P) != nrow or _rows(Q) != ncol:
            raise ValueError("P needs %d rows and Q %d rows for op(M) of shape (%d, %d)" % (nrow, ncol, nrow, ncol))
        nnz = int(M.nnz)
        if out is None:
            if mp == MEM_HOST:
                out = np.empty(nnz, dtype=np.float64)
            else:
                import torch
                out = torch.empty(nnz, dtype=torch.float64, device=P.device)
        po, _ldo, _n1, mo = _dense_arg(out, "out", writable=True)
        if mo != mp:
            raise ValueError("out must be the same kind of array as P and Q")
        if out.ndim != 1 or int(out.shape[0]) != nnz or (nnz > 1 and _ldo != 1):
            raise ValueError("out must be a contiguous 1-D array of %d values (one per tuple of M)" % nnz)
        self._check(self.L.spsamd_multiply_sampled(self.h, C.byref(M), transpose.encode(), pp, ldp, pq, ldq, kp,
                                                   float(alpha), float(beta), po, mp))
        return out

    def to_host(self, dev_ptr, count, dtype):
        """numpy copy of `count` elements of device memory (spsamd_memcpy)."""
        out = np.empty(count, dtype=dtype)
        self._check(self.L.spsamd_memcpy(self.h, out.ctypes.data, dev_ptr, out.nbytes))
        return out

    def memcpy(self, dst_ptr, src_ptr, nbytes):
        self._check(self.L.spsamd_memcpy(self.h, dst_ptr, src_ptr, nbytes))

    # ---- device generators (outputs: caller-owned device pointers)
    def gen_rmat(self, scale, seed, first_edge, n_edges, p0, p1, pv, edge_factor=16):
        self._check(self.L.spsamd_gen_rmat(self.h, scale, edge_factor, seed, first_edge, n_edges, p0, p1, pv))

    def gen_random_rows(self, n, per_row, seed, stream_base, p0, p1, pv):
        self._check(self.L.spsamd_gen_random_rows(self.h, n, per_row, seed, stream_base, p0, p1, pv))

    def gen_poisson2d(self, N, p0, p1, pv):
        self._check(self.L.spsamd_gen_poisson2d(self.h, N, p0, p1, pv))

    def gen_laplace3d(self, N, p0, p1, pv):
        self._check(self.L.spsamd_gen_laplace3d(self.h, N, p0, p1, pv))

    def gen_aggregation3d(self, N, p0, p1, pv):
        self._check(self.L.spsamd_gen_aggregation3d(self.h, N, p0, p1, pv))


_EMPTY_LIST = np.zeros(1, np.int32)        # what an empty host list points at (NULL means every index)


def _index_list(L, name):
    """(pointer, count, mem, keepalive) of an index list argument of extract; (None, 0, None, None) for every index."""
    if L is None:
        return None, 0, None, None
    if isinstance(L, np.ndarray) or isinstance(L, (list, tuple, range)):
        a = np.asarray(L)
        if a.size and a.dtype != np.int32:
            if not np.issubdtype(a.dtype, np.integer) or isinstance(L, np.ndarray):
                raise TypeError("%s must be int32" % name)
        a = np.ascontiguousarray(a, dtype=np.int32)
        if a.ndim != 1:
            raise ValueError("%s must be 1-D" % name)
        return (a if a.size else _EMPTY_LIST).ctypes.data, int(a.size), MEM_HOST, a
    import torch
    if not isinstance(L, torch.Tensor):
        raise TypeError("%s must be None, a numpy int32 array or a torch CUDA int32 tensor" % name)
    if L.dtype != torch.int32 or L.ndim != 1 or not L.is_contiguous():
        raise TypeError("%s must be a contiguous 1-D int32 tensor" % name)
    if L.device.type != "cuda":
        raise ValueError("%s must be a device tensor (or a numpy array for a host list)" % name)
    n = int(L.shape[0])
    return (L.data_ptr() if n else _EMPTY_LIST.ctypes.data), n, (MEM_DEVICE if n else None), L


def _rows(A):
    return int(A.shape[0])


def _dense_arg(A, name, writable):
    """(pointer, leading dimension, right-hand sides, mem) of a dense X / Y argument."""
    if isinstance(A, np.ndarray):
        if A.dtype != np.float64:
            raise TypeError("%s must be float64" % name)
        if writable and not A.flags.writeable:
            raise ValueError("%s is read-only" % name)
        mem, item, strides = MEM_HOST, A.itemsize, A.strides
    else:
        import torch
        if not isinstance(A, torch.Tensor):
            raise TypeError("%s must be a numpy array or a torch tensor" % name)
        if A.dtype != torch.float64:
            raise TypeError("%s must be float64" % name)
        if A.device.type != "cuda":
            raise ValueError("%s must be a device tensor (or a numpy array for host memory)" % name)
        mem, item, strides = MEM_DEVICE, 8, tuple(s * 8 for s in A.stride())
    if A.ndim == 1:
        nrhs, ld = 1, strides[0] // item
        if strides[0] % item or (A.shape[0] > 1 and ld < 1):
            raise ValueError("%s: unsupported stride" % name)
        ld = max(ld, 1)
    elif A.ndim == 2:
        nrhs = int(A.shape[1])
        if nrhs > 1 and strides[1] != item:
            raise ValueError("%s must have contiguous rows (stride 1 along the right-hand sides)" % name)
        if strides[0] % item:
            raise ValueError("%s: unsupported row stride" % name)
        ld = strides[0] // item if A.shape[0] > 1 else nrhs
        if ld < nrhs:
            raise ValueError("%s: rows overlap" % name)
    else:
        raise ValueError("%s must be 1-D or 2-D" % name)
    ptr = A.ctypes.data if mem == MEM_HOST else A.data_ptr()
    return ptr, ld, nrhs, mem


class Operand:
    """spsamd_operand: an operand prepared once (consolidated tuples, row structure, and whatever later products build
    from it), accepted by every entry point through `.coo`."""

    def __init__(self, ctx, X, transpose='.', role=AS_A | AS_B, duplicate_policy=ADD, zero_nan=False):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.L.spsamd_operand_prepare(ctx.h, C.byref(X), transpose.encode(), role, duplicate_policy, int(zero_nan), C.byref(h)))
        self.h = h
        self.coo = Coo()
        ctx._check(ctx.L.spsamd_operand_as_coo(self.h, C.byref(self.coo)))

    @property
    def bytes(self):
        return int(self.ctx.L.spsamd_operand_bytes(self.h))

    def close(self):
        if self.h:
            self.ctx.L.spsamd_operand_destroy(self.h)
            self.h = None


def amg_level(A, *rest):
    """One level as (A, tA, P, tP, R, tR) from (A,), (A, P), (A, P, R) or the six values themselves: flags default to '.',
    and a P without R is passed again as R with 'T' (the tentative prolongator's use)."""
    if len(rest) == 5:
        return (A,) + tuple(rest)
    Pm = rest[0] if len(rest) > 0 else None
    Rm = rest[1] if len(rest) > 1 else None
    if Pm is not None and Rm is None:
        return A, '.', Pm, '.', Pm, 'T'
    return A, '.', Pm, '.', Rm, '.'


class Hierarchy:
    """An unsmoothed-aggregation hierarchy built from public calls only, as prepared operands: per level
    Context.aggregate -> prolongator -> the Galerkin operator P^T (A P) by two Context.multiply calls into SINK_COO, each
    product copied out to device tensors; A and P are prepared with '.', P again with 'T' (the restriction).  It stops at
    max_levels or at a level of at most min_coarse rows.  `levels` is what Context.amg_apply / solve_pcg_amg take;
    `seconds` splits the set-up into aggregate, products and prepare (host wall time, each stage synchronised).  A: a Coo
    struct whose tuples are on the device (a device_coo, or a chained result), square.  close() destroys the handles."""

    def __init__(self, ctx, A, order=AGG_ORDER_HASH, seed=0, flags=0, max_levels=amg_max_levels, min_coarse=64):
        import time
        import torch
        self.ctx, self.levels, self.operands, self.keep = ctx, [], [], []
        self.seconds = {"aggregate": 0.0, "products": 0.0, "prepare": 0.0}
        self.rows, self.nnz = [], []

        def timed(key, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            self.seconds[key] += time.perf_counter() - t0
            return out

        def prepared(X, tr):
            op = timed("prepare", lambda: Operand(ctx, X, tr, AS_A | AS_B))
            self.operands.append(op)
            return op.coo

        def copied(res):
            i = torch.empty(max(int(res.nnz), 1), dtype=torch.int32, device="cuda")
            j, v = torch.empty_like(i), torch.empty(max(int(res.nnz), 1), dtype=torch.float64, device="cuda")
            for dst, src, w in ((i, res.idx0, 4), (j, res.idx1, 4), (v, res.val, 8)):
                if res.nnz:
                    ctx.memcpy(dst.data_ptr(), src, int(res.nnz) * w)
            self.keep.append((i, j, v))
            return device_coo(i.data_ptr(), j.data_ptr(), v.data_ptr(), int(res.nnz), (int(res.shape0), int(res.shape1)), 0)

        try:
            cur = A
            while True:
                n = int(cur.shape0)
                Ap = prepared(cur, '.')
                self.rows.append(n)
                self.nnz.append(int(cur.nnz))
                if len(self.levels) + 1 >= max_levels or n <= min_coarse:
                    self.levels.append((Ap, '.', None, '.', None, '.'))
                    break
                agg = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
                nagg = timed("aggregate", lambda: ctx.aggregate(cur, order=order, seed=seed, flags=flags, out=(agg, None, None)))
                if nagg >= n:                                   # no coarsening (no off-diagonal tuple left): this is the last level
                    self.levels.append((Ap, '.', None, '.', None, '.'))
                    break
                Pc, keep = prolongator(agg[:n], nagg, device=True)
                self.keep.append(keep)
                AP = copied(timed("products", lambda: ctx.multiply(cur, Pc)))
                cur = copied(timed("products", lambda: ctx.multiply(Pc, AP, tA='T')))
                self.levels.append((Ap, '.', prepared(Pc, '.'), '.', prepared(Pc, 'T'), 'T'))
        except Exception:
            self.close()
            raise

    def close(self):
        for op in self.operands:
            op.close()
        self.operands, self.levels, self.keep = [], [], []


class Dist:
    """spsamd_dist: this rank's end of the row-block sharded multiply (one rank per GPU).

    transport=None: the built-in RCCL transport; `unique_id` (128 bytes from Dist.unique_id() on one rank,
    handed to every rank) creates its communicator.  transport=callable(send_ptrs, send_bytes, recv_ptrs,
    recv_bytes, stream) replaces it (the tests route it through gloo on host copies)."""

    @staticmethod
    def unique_id():
        L = load()
        buf = C.create_string_buffer(128)
        rc = L.spsamd_dist_unique_id(buf)
        if rc != 0:
            raise SpsamdError(rc, "spsamd_dist_unique_id failed (librccl not loadable?)")
        return buf.raw

    def __init__(self, ctx, rank, world, unique_id=None, transport=None):
        self.ctx, self.rank, self.world = ctx, rank, world
        self._cb = ALLTOALLV_FN()
        if transport is not None:
            def cb(_user, send, sendb, recv, recvb, n, stream):
                try:
                    transport([send[p] for p in range(n)], [sendb[p] for p in range(n)],
                              [recv[p] for p in range(n)], [recvb[p] for p in range(n)], stream)
                    return 0
                except Exception:                      # never let an exception cross the C boundary
                    import traceback
                    traceback.print_exc()
                    return 1
            self._cb = ALLTOALLV_FN(cb)
        h = C.c_void_p()
        rc = ctx.L.spsamd_dist_create(C.byref(h), ctx.h, rank, world, unique_id, None, self._cb, None)
        ctx._check(rc)
        self.h = h

    def multiply(self, A_block, B_block, b_bounds, C_=1.0, scalei=None, tA='.', scalej=None, tB='.', scalek=None,
                 duplicate_policy=ADD, zero_nan=False, sink=SINK_DIGEST, flags=0):
        """spsamd_dist_multiply: spsparse::multiply's arguments, the two matrices block-wise (collective)."""
        res, stats = Result(), DistStats()
        bb = (C.c_uint64 * len(b_bounds))(*[int(x) for x in b_bounds])
        ptr = [None if s is None else C.byref(s) for s in (scalei, scalej, scalek)]
        rc = self.ctx.L.spsamd_dist_multiply(self.h, float(C_), ptr[0], C.byref(A_block), tA.encode(), ptr[1],
                                             None if B_block is None else C.byref(B_block), tB.encode(), ptr[2], bb,
                                             duplicate_policy, int(zero_nan), sink, flags, C.byref(res), C.byref(stats))
        self.ctx._check(rc)
        return res, stats

    def close(self):
        if self.h:
            self.ctx.L.spsamd_dist_destroy(self.h)
            self.h = None
