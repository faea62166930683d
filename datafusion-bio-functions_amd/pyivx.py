"""ctypes binding of libivx_hip.so (include/ivx.h) for tests and bench.py.

Plumbing only: numpy arrays go through the IVX_MEM_HOST entry points, torch CUDA
tensors through IVX_MEM_DEVICE with their data_ptr().  There is no fallback of
any kind: if the HIP library is missing or no gfx950 device is usable this
module raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libivx_hip.so")

MEM_HOST, MEM_DEVICE = 0, 1
KIND_OVERLAP, KIND_COUNT, KIND_COVERAGE, KIND_NEAREST = 0, 1, 2, 3
OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_OOM, ERR_CAPACITY, ERR_UNSUPPORTED = range(7)
NULL_IDX = 0xFFFFFFFF

# every symbol include/ivx.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "ivx_ctx_create", "ivx_ctx_free", "ivx_last_error", "ivx_ctx_set_stream", "ivx_ctx_use_own_stream",
    "ivx_ctx_synchronize",
    "ivx_ctx_last_kernel_ms", "ivx_version", "ivx_index_build", "ivx_index_free", "ivx_index_rows",
    "ivx_index_device_bytes", "ivx_probe_overlap_count", "ivx_probe_overlap_fill", "ivx_probe_exists",
    "ivx_probe_count", "ivx_probe_coverage", "ivx_probe_nearest", "ivx_merge", "ivx_subtract",
    "ivx_cluster", "ivx_complement", "ivx_take_fixed", "ivx_take_utf8", "ivx_take_bits", "ivx_take_view",
    "ivx_ctx_metrics", "ivx_ctx_reset_metrics", "ivx_ctx_set_memory_limit", "ivx_ctx_trim", "ivx_scatter_fixed",
    "ivx_ctx_reserved_bytes", "ivx_ctx_set_build_overlap", "ivx_index_layout",
    "ivx_probe_mark_build", "ivx_bits_mark", "ivx_bits_select", "ivx_depth", "ivx_probe_overlap_agg",
    "ivx_depth_profile_build", "ivx_depth_profile_free", "ivx_depth_profile_steps", "ivx_depth_profile_device_bytes",
    "ivx_depth_profile_read", "ivx_depth_profile_expand", "ivx_depth_profile_merge", "ivx_depth_profile_blocks",
    "ivx_cigar_parse", "ivx_depth_text", "ivx_depth_profile_build_text",
    "ivx_depth_profile_summarize", "ivx_depth_profile_windows",
    "ivx_depth_profile_quantiles", "ivx_depth_profile_window_quantiles",
    "ivx_depth_profile_quantize", "ivx_depth_profile_hist", "ivx_intersect",
]

# every symbol the companion headers declare (include/ivx_select.h; checked by tests/test_select_abi.py): entries that are
# not in include/ivx.h yet, bound beside SYMBOLS the way the test hooks are
EXT_SYMBOLS = ["ivx_probe_overlap_select"]

# every symbol include/ivx_where.h declares (checked by tests/test_where_abi.py): the overlap thresholds' entries, a list of
# their own
WHERE_SYMBOLS = ["ivx_probe_overlap_count_where", "ivx_probe_mark_build_where", "ivx_probe_overlap_agg_where",
                 "ivx_probe_overlap_select_where", "ivx_pairs_where"]
# every symbol include/ivx_nearest.h declares (checked by tests/test_nearest_dir_abi.py): nearest on one side only and / or
# within a distance cap, a list of its own
NEAREST_SYMBOLS = ["ivx_probe_nearest_dir"]
# directions of ivx_probe_nearest_dir, in the order of the IVX_NEAR_* enum (include/ivx_nearest.h), and their aliases
NEAR_DIRECTIONS = ("any", "before", "after")
NEAR_ALIASES = {"upstream": "before", "downstream": "after"}
# pairs per tile of ivx_pairs_where's two passes (csrc/ivx_where.hpp PW_TILE = PW_T * PW_PI; tests/test_gpu_overlap_where.py)
PAIRS_WHERE_TILE = 1024

# outputs one workgroup of the expand kernel makes (csrc/ivx_depth_expand.hip DEPTH_EXPAND_TILE; tests/test_depth_per_base_tile.py)
DEPTH_EXPAND_TILE = 4096
# merged steps one workgroup of the merge kernel makes (csrc/ivx_depth_merge.hip DEPTH_MERGE_TILE; tests/test_depth_merge_cpu.py)
DEPTH_MERGE_TILE = 2048
# steps one tile aggregate of the region summaries covers (csrc/ivx_depth_regions.hip DEPTH_REGION_TILE; tests/test_depth_regions_cpu.py)
DEPTH_REGION_TILE = 1024
# thresholds one summary call takes (include/ivx.h IVX_DEPTH_MAX_THRESHOLDS)
DEPTH_MAX_THRESHOLDS = 8
# the region order statistics (csrc/ivx_depth_rank.hip; tests/test_depth_quantiles_cpu.py): steps per (min, max) tile, segments
# one wavefront ranks in registers (more go to the select kernel), workgroups of the select kernel
DEPTH_RANK_TILE = 1024
DEPTH_RANK_SEGS = 64
DEPTH_RANK_SELECT_GRID = 512
# quantiles one call takes (include/ivx.h IVX_DEPTH_MAX_QUANTILES)
DEPTH_MAX_QUANTILES = 8
# the coverage classes (csrc/ivx_depth_classes.hip; tests/test_gpu_depth_classes.py): steps per tile of both passes, the bins a
# workgroup of the histogram pass keeps in LDS (more go to memory directly), the key ids a tile may span and still use them
DEPTH_CLASS_TILE = 1024
DEPTH_HIST_LDS_BINS = 2048
DEPTH_HIST_TILE_KEYS = 8
# cuts of one quantize call, bins of one hist call (include/ivx.h IVX_DEPTH_MAX_CUTS, IVX_DEPTH_MAX_BINS)
DEPTH_MAX_CUTS = 31
DEPTH_MAX_BINS = 65536
# bytes one thread / one workgroup of the text-CIGAR parser takes (csrc/ivx_cigar.hip CIGAR_B, CIGAR_TILE)
CIGAR_B = 16
CIGAR_TILE = 4096

# outputs of ivx_probe_overlap_agg, in the order of its pointers, and their element types
AGG_OUTPUTS = ("count", "sum", "min", "max", "bases", "wsum")

# criteria of ivx_probe_overlap_select, in the order of the IVX_SEL_* enum (include/ivx_select.h)
SEL_BY = ("min_val", "max_val", "max_overlap", "min_overlap", "first_row", "last_row")

# slots of ivx_index_layout (include/ivx.h IVX_LAYOUT_*), in order
LAYOUT_SLOTS = ["kind", "sh0", "nlev", "levrows", "rcells", "rcs", "nreg", "pk24", "slow", "fg", "fbits", "nroute_nreg", "lbuild"]

# words of the test hook ivx_debug_index_forms (csrc/ivx_internal.hpp IVX_FORMS_*): these scalars, then (shift, cells) per rank grid
FORMS_SLOTS = ["kind", "nroute_nreg", "near_words", "near_order", "near_fallback"]
FORMS_GRIDS = {KIND_COUNT: ("starts", "ends"), KIND_COVERAGE: ("first", "last"), KIND_NEAREST: ("by_start", "by_end", "pmax")}
NEAR_ORDER_PRESORTED, NEAR_ORDER_REPAIR, NEAR_ORDER_FULL = 0, 1, 2      # near_order
NEAR_FB_NOFIT, NEAR_FB_LIN_RUN, NEAR_FB_SE_RUN = 1, 2, 4                # near_fallback bits

# words of the test hook ivx_debug_sweep_form (csrc/ivx_internal.hpp IVX_SWEEP_*), in order
SWEEP_SLOTS = ["sort_words", "nw", "lin", "bits_s", "bits_e", "bits_k", "sorted_in", "two_step", "toolong", "narrow_rows", "k8",
               "packed", "narrow_runs", "ntile"]
SWEEP_ROWS, SWEEP_PACKED, SWEEP_PACKED_BESIDE_ROWS = 0, 1, 2            # packed
# ... and the two words behind them that only an intersect sets (IVX_SWEEP_LEFT_*): nw and sort_words of its LEFT side's sort
SWEEP_LEFT_SLOTS = ["left_nw", "left_sort_words"]

# words per workgroup of the test hook ivx_debug_intersect_paths (csrc/ivx_sweep.hip k_frag_count<IsectOp>), in order: the bracket of the
# workgroup's first searches, the staged window (first run, runs), whether LDS was used, rows planned again from global memory
ISECT_DBG_SLOTS = ["brk_lo", "brk_hi", "win_first", "win_runs", "lds", "escaped"]


def intersect_geometry():
    """the constants of intersect's count pass (test hook ivx_debug_intersect_geometry): left rows per workgroup, the most
    runs a workgroup stages in LDS, the runs staged past its bracket, the words of ISECT_DBG_SLOTS"""
    v = [C.c_uint32(0) for _ in range(4)]
    lib().ivx_debug_intersect_geometry(*[C.byref(x) for x in v])
    return dict(zip(("rows_per_wg", "staged_runs", "margin", "dbg_words"), (x.value for x in v)))


# words of the test hook ivx_debug_ctx_state (csrc/ivx_internal.hpp IVX_STATE_*), in order; the masks have a bit per scratch slot
STATE_SLOTS = ["join_valid", "join_slots", "sub_valid", "sub_slots", "tail_pending", "scratch_held", "pool_free", "join_fills_planned",
               "sub_fills_planned"]
# bits of the test hook ivx_debug_poison's `what` (csrc/ivx_internal.hpp IVX_POISON_*)
POISON_SCRATCH, POISON_DROP_PLANS, POISON_SCALARS, POISON_PINNED, POISON_POOL = 1, 2, 4, 8, 16


class Metrics(C.Structure):
    _fields_ = [("build_time", C.c_double), ("join_time", C.c_double), ("build_input_batches", C.c_uint64),
                ("build_input_rows", C.c_uint64), ("build_mem_used", C.c_uint64), ("input_batches", C.c_uint64),
                ("input_rows", C.c_uint64), ("output_batches", C.c_uint64), ("output_rows", C.c_uint64)]


class OverlapWhereC(C.Structure):
    """ivx_overlap_where of include/ivx_where.h"""
    _fields_ = [("min_bases", C.c_int64), ("probe_num", C.c_uint32), ("probe_den", C.c_uint32),
                ("build_num", C.c_uint32), ("build_den", C.c_uint32), ("either", C.c_uint32)]


def _fraction(f, what):
    """(num, den) of a threshold fraction: None -> not asked; a (num, den) pair is taken as it is (the library checks it); a
    Fraction exactly; a float as Fraction(f).limit_denominator(10**9) -- the nearest fraction with a denominator up to 10^9, so
    0.5 is 1/2 and 0.1 is 1/10, but a pair that sits exactly on a boundary may fall on the other side of it than it does for a
    tool that compares in floating point."""
    from fractions import Fraction
    if f is None:
        return 0, 0
    if isinstance(f, (tuple, list)):
        if len(f) != 2:
            raise ValueError(f"overlap where: {what} is a (num, den) pair")
        return int(f[0]), int(f[1])
    if isinstance(f, float):
        if f != f or f < 0:
            raise ValueError(f"overlap where: {what} is a fraction in [0, 1]")
        f = Fraction(f).limit_denominator(10 ** 9)
    if isinstance(f, (Fraction, int)) and not isinstance(f, bool):
        f = Fraction(f)
        if f < 0:
            raise ValueError(f"overlap where: {what} is a fraction in [0, 1]")
        return f.numerator, f.denominator
    raise TypeError(f"overlap where: {what} is a (num, den) pair, a Fraction or a float")


class OverlapWhere:
    """An overlap threshold (include/ivx_where.h): min_bases shared bases, and / or minimum fractions of the probe row and of
    the build row that the overlap must cover; either=True: one of two fractions suffices.  Fractions: see _fraction."""

    def __init__(self, min_bases=0, probe=None, build=None, either=False):
        self.min_bases, self.probe, self.build, self.either = min_bases, probe, build, either

    def __repr__(self):
        return f"OverlapWhere(min_bases={self.min_bases!r}, probe={self.probe!r}, build={self.build!r}, either={self.either!r})"

    def c_struct(self):
        pn, pd = _fraction(self.probe, "probe")
        bn, bd = _fraction(self.build, "build")
        for v in (pn, pd, bn, bd):
            if not 0 <= v <= 0xFFFFFFFF:
                raise ValueError("overlap where: a fraction's terms are unsigned 32-bit numbers")
        return OverlapWhereC(int(self.min_bases), pn, pd, bn, bd, int(self.either))


def as_where(w):
    """None, an OverlapWhere, or a dict of its keywords -> a byref() argument (None: the NULL pointer) and the struct it
    points to (to be kept alive across the call)"""
    if w is None:
        return None, None
    if isinstance(w, dict):
        w = OverlapWhere(**w)
    if isinstance(w, OverlapWhereC):
        return C.byref(w), w
    if not isinstance(w, OverlapWhere):
        raise TypeError("where is None, an OverlapWhere or a dict of its keywords")
    s = w.c_struct()
    return C.byref(s), s


class IvxError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"ivx status {status}: {msg}")
        self.status = status


_lib = None


def _preload_hip_runtime():
    """PyTorch-ROCm bundles its own libamdhip64.so (same SONAME as /opt/rocm's).  Two HIP
    runtimes in one process do not share device state, so when torch is installed make its
    copy the one that is resident before libivx_hip.so binds to libamdhip64.so.7."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.origin:
        p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IvxError(ERR_NO_DEVICE, f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        _preload_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.ivx_last_error.restype = C.c_char_p
        L.ivx_version.restype = C.c_char_p
        L.ivx_ctx_last_kernel_ms.restype = C.c_double
        L.ivx_index_rows.restype = C.c_uint64
        L.ivx_index_device_bytes.restype = C.c_uint64
        L.ivx_ctx_reserved_bytes.restype = C.c_uint64
        L.ivx_probe_overlap_agg.restype = C.c_int
        L.ivx_probe_overlap_agg.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_uint64, C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        L.ivx_depth.restype = C.c_int
        L.ivx_probe_overlap_select.restype = C.c_int
        L.ivx_probe_overlap_select.argtypes = ([C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_uint64, C.c_void_p, C.c_uint32, C.c_int] +
                                               [C.c_void_p] * 2)
        head = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_uint64]        # ctx, ix, mem, key, start, end, n
        W = C.POINTER(OverlapWhereC)
        for name in WHERE_SYMBOLS:
            getattr(L, name).restype = C.c_int
        L.ivx_probe_overlap_count_where.argtypes = head + [W, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.ivx_probe_mark_build_where.argtypes = head + [W, C.c_void_p]
        L.ivx_probe_overlap_agg_where.argtypes = head + [C.c_void_p, C.c_uint32, W] + [C.c_void_p] * 6
        L.ivx_probe_overlap_select_where.argtypes = head + [C.c_void_p, C.c_uint32, C.c_int, W] + [C.c_void_p] * 2
        L.ivx_pairs_where.argtypes = ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                       C.c_void_p, C.c_void_p, C.c_uint64, W, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)])
        L.ivx_probe_nearest_dir.restype = C.c_int
        L.ivx_probe_nearest_dir.argtypes = head + [C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 3 + [C.c_uint64, C.POINTER(C.c_uint64)]
        L.ivx_depth.argtypes = ([C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_uint64] + [C.c_void_p] * 4 + [C.c_uint64] +
                                [C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 +
                                [C.c_uint64, C.POINTER(C.c_uint64)])
        L.ivx_depth_profile_build.restype = C.c_int
        L.ivx_depth_profile_build.argtypes = L.ivx_depth.argtypes[:18] + [C.POINTER(C.c_void_p)]
        L.ivx_cigar_parse.restype = C.c_int
        L.ivx_cigar_parse.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                      C.c_uint64, C.POINTER(C.c_uint64)]
        # (large, text_offsets, text) in place of (cigar_offsets, cigar_ops)
        L.ivx_depth_text.restype = C.c_int
        L.ivx_depth_text.argtypes = L.ivx_depth.argtypes[:6] + [C.c_int, C.c_void_p, C.c_void_p] + L.ivx_depth.argtypes[8:]
        L.ivx_depth_profile_build_text.restype = C.c_int
        L.ivx_depth_profile_build_text.argtypes = L.ivx_depth_text.argtypes[:19] + [C.POINTER(C.c_void_p)]
        L.ivx_depth_profile_free.restype = None
        L.ivx_depth_profile_free.argtypes = [C.c_void_p]
        L.ivx_depth_profile_steps.restype = C.c_uint64
        L.ivx_depth_profile_steps.argtypes = [C.c_void_p]
        L.ivx_depth_profile_device_bytes.restype = C.c_uint64
        L.ivx_depth_profile_device_bytes.argtypes = [C.c_void_p]
        L.ivx_depth_profile_read.restype = C.c_int
        L.ivx_depth_profile_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_uint64, C.POINTER(C.c_uint64)]
        L.ivx_depth_profile_expand.restype = C.c_int
        L.ivx_depth_profile_expand.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
        L.ivx_depth_profile_merge.restype = C.c_int
        L.ivx_depth_profile_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.ivx_depth_profile_blocks.restype = C.c_int
        L.ivx_depth_profile_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_uint64, C.POINTER(C.c_uint64)]
        L.ivx_depth_profile_summarize.restype = C.c_int
        L.ivx_depth_profile_summarize.argtypes = ([C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_uint64, C.c_uint32, C.c_void_p, C.c_int,
                                                  C.c_void_p, C.c_uint32] + [C.c_void_p] * 3)
        L.ivx_depth_profile_windows.restype = C.c_int
        L.ivx_depth_profile_windows.argtypes = ([C.c_void_p, C.c_void_p, C.c_int] + [C.c_uint32] * 4 + [C.c_uint64, C.c_int, C.c_void_p, C.c_uint32] +
                                                [C.c_void_p] * 3)
        L.ivx_depth_profile_quantiles.restype = C.c_int
        L.ivx_depth_profile_quantiles.argtypes = ([C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_uint64, C.c_uint32, C.c_void_p, C.c_int,
                                                  C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4)
        L.ivx_depth_profile_window_quantiles.restype = C.c_int
        L.ivx_depth_profile_window_quantiles.argtypes = ([C.c_void_p, C.c_void_p, C.c_int] + [C.c_uint32] * 4 + [C.c_uint64, C.c_int, C.c_void_p, C.c_uint32,
                                                         C.c_uint32] + [C.c_void_p] * 4)
        L.ivx_depth_profile_quantize.restype = C.c_int
        L.ivx_depth_profile_quantize.argtypes = ([C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32,
                                                  C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint64, C.POINTER(C.c_uint64)])
        L.ivx_depth_profile_hist.restype = C.c_int
        L.ivx_depth_profile_hist.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_uint32, C.c_void_p]
        # test hook of csrc/ivx_sweep.hip (not in include/ivx.h): what subtract's count pass did (tests/test_gpu_subtract_edges.py)
        L.ivx_debug_subtract_paths.restype = C.c_int
        L.ivx_debug_subtract_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ivx_intersect.restype = C.c_int
        L.ivx_intersect.argtypes = ([C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_uint64] + [C.c_void_p] * 3 + [C.c_uint64, C.c_uint32, C.c_int] +
                                    [C.c_void_p] * 4 + [C.c_uint64, C.POINTER(C.c_uint64)])
        # test hooks of csrc/ivx_capi.hip / ivx_sweep.hip (not in include/ivx.h): the same call up to `strict`, then where to report
        # what its count pass did; the constants of that pass (tests/test_gpu_intersect_edges.py)
        L.ivx_debug_intersect_paths.restype = C.c_int
        L.ivx_debug_intersect_paths.argtypes = (L.ivx_intersect.argtypes[:12] + [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] +
                                                [C.POINTER(C.c_uint64)] * 3)
        L.ivx_debug_intersect_geometry.restype = None
        L.ivx_debug_intersect_geometry.argtypes = [C.POINTER(C.c_uint32)] * 4
        # test hook of csrc/ivx_capi.hip (not in include/ivx.h): the forms a count / coverage / nearest index took (tests/test_gpu_rank_edges.py)
        L.ivx_debug_index_forms.restype = C.c_int
        L.ivx_debug_index_forms.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32]
        # test hook of csrc/ivx_sweep.hip (not in include/ivx.h): the forms the last merge / cluster / complement took (tests/test_gpu_run_edges.py)
        L.ivx_debug_sweep_form.restype = C.c_int
        L.ivx_debug_sweep_form.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32]
        # test hooks of csrc/ivx_capi.hip (not in include/ivx.h): what a context carries between calls, and a fixed word written
        # over all of it that no plan and no outliving scalar word needs (tests/test_gpu_entry_state.py)
        L.ivx_debug_ctx_state.restype = C.c_int
        L.ivx_debug_ctx_state.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]
        L.ivx_debug_poison.restype = C.c_int
        L.ivx_debug_poison.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _ptr(x):
    if x is None:
        return None
    if _is_torch(x):
        return C.c_void_p(x.data_ptr())
    return x.ctypes.data_as(C.c_void_p)


def _mem_of(*arrs):
    kinds = {_is_torch(a) for a in arrs if a is not None}
    if len(kinds) > 1:
        raise ValueError("mix of host and device buffers in one call")
    return MEM_DEVICE if kinds == {True} else MEM_HOST


def _np(a, dt):
    return None if a is None else np.ascontiguousarray(a, dtype=dt)


def _cols(key, s, e, dt):
    """normalise one (key,start,end) side; returns (key,start,end,n,mem)"""
    if _is_torch(s):
        assert s.is_contiguous() and e.is_contiguous() and (key is None or key.is_contiguous())
        return key, s, e, int(s.numel()), MEM_DEVICE
    key, s, e = _np(key, np.uint32), _np(s, dt), _np(e, dt)
    return key, s, e, len(s), MEM_HOST


class Index:
    def __init__(self, ctx, handle, kind):
        self.ctx, self.h, self.kind = ctx, handle, kind

    @property
    def rows(self):
        return lib().ivx_index_rows(self.h)

    @property
    def device_bytes(self):
        return lib().ivx_index_device_bytes(self.h)

    def layout(self):
        """the form the build picked for the binned overlap index (include/ivx.h ivx_index_layout) as a dict"""
        out = (C.c_uint32 * len(LAYOUT_SLOTS))()
        self.ctx._chk(lib().ivx_index_layout(self.ctx.h, self.h, out, C.c_uint32(len(LAYOUT_SLOTS))))
        return dict(zip(LAYOUT_SLOTS, list(out)))

    def forms(self):
        """the forms a count / coverage / nearest index took (test hook ivx_debug_index_forms) as a dict: the scalar
        FORMS_SLOTS, and "grids": {name: (shift, cells)} of the kind's rank grids"""
        n = len(FORMS_SLOTS) + 6
        out = (C.c_uint32 * n)()
        self.ctx._chk0(lib().ivx_debug_index_forms(self.ctx.h, self.h, out, C.c_uint32(n)))
        f = dict(zip(FORMS_SLOTS, list(out)))
        f["grids"] = {g: (out[len(FORMS_SLOTS) + 2 * i], out[len(FORMS_SLOTS) + 2 * i + 1]) for i, g in enumerate(FORMS_GRIDS.get(self.kind, ()))}
        return f

    def free(self):
        if self.h:
            lib().ivx_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DepthProfile:
    """the step function of depth() on the device (include/ivx.h ivx_depth_profile_*).  `ctx` is the context that built it;
    read() and expand() take any other context of the same device as ctx=."""

    def __init__(self, ctx, handle, n_keys, device):
        self.ctx, self.h, self.n_keys, self.device = ctx, handle, n_keys, device

    def steps(self):
        return lib().ivx_depth_profile_steps(self.h)

    @property
    def device_bytes(self):
        return lib().ivx_depth_profile_device_bytes(self.h)

    def read(self, device=False, ctx=None):
        """-> (key u32, pos u32, coverage i32, key_seen u8[n_keys]); numpy arrays, or torch tensors with device=True
        (the unsigned columns as their int32 bits)"""
        ctx = ctx or self.ctx
        n = self.steps()
        if device:
            import torch
            dev = self.device or "cuda:0"
            out = [torch.empty(max(n, 1), dtype=torch.int32, device=dev) for _ in range(3)]
            seen = torch.empty(max(self.n_keys, 1), dtype=torch.uint8, device=dev)
        else:
            out = [np.empty(max(n, 1), dt) for dt in (np.uint32, np.uint32, np.int32)]
            seen = np.empty(max(self.n_keys, 1), np.uint8)
        m = C.c_uint64(0)
        ctx._chk0(lib().ivx_depth_profile_read(ctx.h, self.h, MEM_DEVICE if device else MEM_HOST, *[_ptr(o) for o in out], _ptr(seen),
                                               max(n, 1), C.byref(m)))
        return tuple(o[:m.value] for o in out) + (seen[:self.n_keys],)

    def expand(self, key, first_pos, n, skip_pos0=False, want_pos=True, out_pos=None, out_cov=None, device=None, ctx=None, want_cov=True):
        """positions [first_pos, first_pos + n) of `key` -> (pos int32 or None, coverage int16 or None).  out_pos / out_cov:
        caller's buffers of n elements (numpy, or torch device tensors: then the call may return with the kernel in
        flight); without them numpy arrays are made, or device tensors with device=True."""
        ctx = ctx or self.ctx
        given = [o for o in (out_pos, out_cov) if o is not None]
        if device is None:
            device = bool(given) and _is_torch(given[0])
        if device:
            import torch
            dev = given[0].device if given else (self.device or "cuda:0")
            if want_pos and out_pos is None:
                out_pos = torch.empty(n, dtype=torch.int32, device=dev)
            if want_cov and out_cov is None:
                out_cov = torch.empty(n, dtype=torch.int16, device=dev)
            assert all(o is None or (o.is_contiguous() and o.numel() >= n) for o in (out_pos, out_cov))
        else:
            if want_pos and out_pos is None:
                out_pos = np.empty(n, np.int32)
            if want_cov and out_cov is None:
                out_cov = np.empty(n, np.int16)
        mem = _mem_of(out_pos, out_cov) if (out_pos is not None or out_cov is not None) else (MEM_DEVICE if device else MEM_HOST)
        ctx._chk(lib().ivx_depth_profile_expand(ctx.h, self.h, mem, int(key), int(first_pos), int(n), int(bool(skip_pos0)),
                                                _ptr(out_pos), _ptr(out_cov)))
        return out_pos, out_cov

    def merge(self, other, ctx=None):
        """self + other -> a new DepthProfile: the profile of the union of the inputs that made the two (both stay valid;
        other may be self).  Built by, and reserved against, ctx (default: the context that built self)."""
        ctx = ctx or self.ctx
        h = C.c_void_p()
        ctx._chk(lib().ivx_depth_profile_merge(ctx.h, self.h, other.h if other is not None else None, C.byref(h)))
        return DepthProfile(ctx, h, max(self.n_keys, other.n_keys), self.device or other.device)

    def blocks(self, device=False, ctx=None, cap=None, outputs=(True, True, True, True)):
        """the coverage blocks of the profile, what Ctx.depth() gives for the inputs that made it -> (key, start, end,
        coverage), None where not asked for; numpy arrays, or torch tensors with device=True (the unsigned columns as
        their int32 bits).  cap=None: a sizing call, then the fill call."""
        ctx = ctx or self.ctx
        mem = MEM_DEVICE if device else MEM_HOST
        if cap is None:
            m = C.c_uint64(0)
            ctx._chk(lib().ivx_depth_profile_blocks(ctx.h, self.h, mem, None, None, None, None, 0, C.byref(m)))
            cap = max(m.value, 1)
        if device:
            import torch
            out = [torch.empty(cap, dtype=torch.int32, device=self.device or "cuda:0") if w else None for w in outputs]
        else:
            out = [np.empty(cap, dt) if w else None for w, dt in zip(outputs, (np.uint32, np.uint32, np.uint32, np.int32))]
        m2 = C.c_uint64(0)
        st = lib().ivx_depth_profile_blocks(ctx.h, self.h, mem, *[_ptr(o) for o in out], cap, C.byref(m2))
        if st == ERR_CAPACITY:
            raise IvxError(st, f"{lib().ivx_last_error(ctx.h).decode()} (needed {m2.value})")
        ctx._chk(st)
        return tuple(None if o is None else o[:m2.value] for o in out)

    def _summary_out(self, n, n_thr, device, dev, outputs):
        shapes = ((n,), (n,), (n_thr, n))
        if device:
            import torch
            return [torch.empty(sh, dtype=torch.int64, device=dev) if w else None for w, sh in zip(outputs, shapes)]
        return [np.empty(sh, np.int64) if w else None for w, sh in zip(outputs, shapes)]

    def summarize(self, key, start, end, thresholds=(), pos_lo=0, key_hi=None, skip_pos0=False, ctx=None, outputs=(True, True, True)):
        """per region [start[i], end[i]] (closed, clipped to the key's domain [pos_lo, key_hi[key]]) of key[i] (None: key 0)
        -> (bases int64[n], coverage sum int64[n], bases at or above each threshold int64[n_thr, n]); None where `outputs`
        does not ask.  numpy arrays, or torch device tensors (then the results are device tensors and the call may return
        with kernels in flight); a mix is a ValueError."""
        ctx = ctx or self.ctx
        mem = _mem_of(key, start, end, key_hi)
        thr = np.ascontiguousarray(thresholds, dtype=np.int32).reshape(-1)
        if mem == MEM_DEVICE:
            assert all(a is None or a.is_contiguous() for a in (key, start, end, key_hi))
            n, dev = int(start.numel()), start.device
        else:
            key, start, end, key_hi = (_np(a, np.uint32) for a in (key, start, end, key_hi))
            n, dev = len(start), None
        out = self._summary_out(n, len(thr), mem == MEM_DEVICE, dev, outputs)
        ctx._chk(lib().ivx_depth_profile_summarize(ctx.h, self.h, mem, _ptr(key), _ptr(start), _ptr(end), n, int(pos_lo), _ptr(key_hi),
                                                   int(bool(skip_pos0)), _ptr(thr), len(thr), *[_ptr(o) for o in out]))
        return tuple(out)

    def windows(self, key, first_pos, last_pos, width, n=None, thresholds=(), skip_pos0=False, device=False, ctx=None, outputs=(True, True, True)):
        """the same three outputs for the windows [first_pos + i * width, + width - 1] of `key`, cut at last_pos; n defaults
        to the count that covers [first_pos, last_pos].  numpy arrays, or torch device tensors with device=True."""
        ctx = ctx or self.ctx
        if n is None:
            n = (int(last_pos) - int(first_pos)) // int(width) + 1 if int(last_pos) >= int(first_pos) and int(width) > 0 else 0
        thr = np.ascontiguousarray(thresholds, dtype=np.int32).reshape(-1)
        out = self._summary_out(int(n), len(thr), device, self.device or "cuda:0", outputs)
        ctx._chk(lib().ivx_depth_profile_windows(ctx.h, self.h, MEM_DEVICE if device else MEM_HOST, int(key), int(first_pos), int(last_pos),
                                                 int(width), int(n), int(bool(skip_pos0)), _ptr(thr), len(thr), *[_ptr(o) for o in out]))
        return tuple(out)

    def _rank_out(self, n, n_q, device, dev, outputs):
        shapes, dts = ((n,), (n,), (n,), (n_q, n)), ("int64", "int32", "int32", "int32")
        if device:
            import torch
            return [torch.empty(sh, dtype=getattr(torch, dt), device=dev) if w else None for w, sh, dt in zip(outputs, shapes, dts)]
        return [np.empty(sh, dt) if w else None for w, sh, dt in zip(outputs, shapes, dts)]

    def quantiles(self, key, start, end, q_num=(), q_den=2, pos_lo=0, key_hi=None, skip_pos0=False, ctx=None, outputs=(True,) * 4):
        """per region of summarize() -> (bases int64[n], min int32[n], max int32[n], quantiles int32[n_q, n]) of its per-base
        coverage; quantile j is element floor((bases - 1) * q_num[j] / q_den) of the sorted values (q_num=(1,), q_den=2: the
        lower median), and a region without bases gives 0.  None where `outputs` does not ask.  numpy arrays, or torch
        device tensors (then the results are device tensors and the call may return with kernels in flight)."""
        ctx = ctx or self.ctx
        mem = _mem_of(key, start, end, key_hi)
        qn = np.ascontiguousarray(q_num, dtype=np.uint32).reshape(-1)
        if mem == MEM_DEVICE:
            assert all(a is None or a.is_contiguous() for a in (key, start, end, key_hi))
            n, dev = int(start.numel()), start.device
        else:
            key, start, end, key_hi = (_np(a, np.uint32) for a in (key, start, end, key_hi))
            n, dev = len(start), None
        out = self._rank_out(n, len(qn), mem == MEM_DEVICE, dev, outputs)
        ctx._chk(lib().ivx_depth_profile_quantiles(ctx.h, self.h, mem, _ptr(key), _ptr(start), _ptr(end), n, int(pos_lo), _ptr(key_hi),
                                                   int(bool(skip_pos0)), _ptr(qn), len(qn), int(q_den), *[_ptr(o) for o in out]))
        return tuple(out)

    def window_quantiles(self, key, first_pos, last_pos, width, n=None, q_num=(), q_den=2, skip_pos0=False, device=False, ctx=None,
                         outputs=(True,) * 4):
        """the same four outputs for the windows of windows()"""
        ctx = ctx or self.ctx
        if n is None:
            n = (int(last_pos) - int(first_pos)) // int(width) + 1 if int(last_pos) >= int(first_pos) and int(width) > 0 else 0
        qn = np.ascontiguousarray(q_num, dtype=np.uint32).reshape(-1)
        out = self._rank_out(int(n), len(qn), device, self.device or "cuda:0", outputs)
        ctx._chk(lib().ivx_depth_profile_window_quantiles(ctx.h, self.h, MEM_DEVICE if device else MEM_HOST, int(key), int(first_pos),
                                                          int(last_pos), int(width), int(n), int(bool(skip_pos0)), _ptr(qn), len(qn),
                                                          int(q_den), *[_ptr(o) for o in out]))
        return tuple(out)

    def _key_hi(self, key_hi, device):
        """key_hi where the call's memory mode wants it: a torch device tensor passes through in device mode, anything else is
        made a uint32 numpy array (host mode) or copied to the device as its int32 bits"""
        if key_hi is None:
            return None
        if device:
            if _is_torch(key_hi):
                assert key_hi.is_contiguous()
                return key_hi
            import torch
            return torch.from_numpy(np.ascontiguousarray(key_hi, dtype=np.uint32).view(np.int32)).to(self.device or "cuda:0")
        if _is_torch(key_hi):
            raise ValueError("mix of host and device buffers in one call")
        return _np(key_hi, np.uint32)

    def quantize(self, cuts, emit=None, pos_lo=0, key_hi=None, skip_pos0=False, seen_only=False, device=False, ctx=None, cap=None,
                 outputs=(True, True, True, True)):
        """the maximal runs of positions whose coverage stays in one class -> (key, start, end, cls), closed intervals ordered
        by (key, start); class(v) = the number of cuts <= v.  emit: the classes to emit (None: all; an iterable of class
        numbers, or the bit mask as an int); the runs of the others still separate their neighbours.  numpy arrays, or torch
        tensors with device=True (as their int32 bits).  cap=None: a sizing call, then the fill call."""
        ctx = ctx or self.ctx
        mem = MEM_DEVICE if device else MEM_HOST
        c = np.ascontiguousarray(cuts, dtype=np.int32).reshape(-1)
        if emit is None:
            mask = (1 << (len(c) + 1)) - 1 if len(c) < 32 else 0xFFFFFFFF
        elif isinstance(emit, (int, np.integer)):
            mask = int(emit)
        else:
            mask = 0
            for j in emit:
                mask |= 1 << int(j)
        if mask >> 32:
            raise ValueError("emit names a class above 31")
        hi = self._key_hi(key_hi, device)
        head = (ctx.h, self.h, mem, int(pos_lo), _ptr(hi), int(bool(skip_pos0)), int(bool(seen_only)), _ptr(c), len(c), mask)
        if cap is None:
            m = C.c_uint64(0)
            ctx._chk(lib().ivx_depth_profile_quantize(*head, None, None, None, None, 0, C.byref(m)))
            cap = max(m.value, 1)
        if device:
            import torch
            out = [torch.empty(cap, dtype=torch.int32, device=self.device or "cuda:0") if w else None for w in outputs]
        else:
            out = [np.empty(cap, np.uint32) if w else None for w in outputs]
        m2 = C.c_uint64(0)
        st = lib().ivx_depth_profile_quantize(*head, *[_ptr(o) for o in out], cap, C.byref(m2))
        if st == ERR_CAPACITY:
            raise IvxError(st, f"{lib().ivx_last_error(ctx.h).decode()} (needed {m2.value})")
        ctx._chk(st)
        return tuple(None if o is None else o[:m2.value] for o in out)

    def hist(self, v_lo=0, n_bins=256, pos_lo=0, key_hi=None, skip_pos0=False, seen_only=False, device=False, ctx=None):
        """per key the number of positions of its domain at each coverage value -> int64 [n_keys, n_bins]: bin b counts the
        positions with coverage v_lo + b, the first bin also everything below, the last one everything above.  A numpy array,
        or a torch tensor with device=True (then the call may return with kernels in flight)."""
        ctx = ctx or self.ctx
        hi = self._key_hi(key_hi, device)
        if device:
            import torch
            out = torch.empty((self.n_keys, int(n_bins)), dtype=torch.int64, device=self.device or "cuda:0")
        else:
            out = np.empty((self.n_keys, int(n_bins)), np.int64)
        ctx._chk(lib().ivx_depth_profile_hist(ctx.h, self.h, MEM_DEVICE if device else MEM_HOST, int(pos_lo), _ptr(hi), int(bool(skip_pos0)),
                                              int(bool(seen_only)), int(v_lo), int(n_bins), _ptr(out) if self.n_keys and n_bins else None))
        return out

    def free(self):
        if self.h:
            lib().ivx_depth_profile_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Ctx:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        st = lib().ivx_ctx_create(C.c_int(device), C.byref(self.h))
        if st != OK:
            self.h = None
            raise IvxError(st, "ivx_ctx_create failed (no usable gfx950 device; there is no CPU fallback)")

    def close(self):
        if self.h:
            lib().ivx_ctx_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    acc_ms = None       # set to 0.0 to sum the device time (hipEvents) of every compute call made from here on

    def _chk0(self, st):
        if st != OK:
            raise IvxError(st, lib().ivx_last_error(self.h).decode())

    def _chk(self, st):
        """status check of a COMPUTE call (one that brackets its kernels with the context's events)"""
        self._chk0(st)
        if self.acc_ms is not None:
            self.acc_ms += self.last_kernel_ms()

    def set_stream(self, stream_ptr):
        """use this hipStream_t verbatim (0/None = HIP's default stream)"""
        self._chk0(lib().ivx_ctx_set_stream(self.h, C.c_void_p(stream_ptr or 0)))

    def use_own_stream(self):
        self._chk0(lib().ivx_ctx_use_own_stream(self.h))

    def synchronize(self):
        self._chk0(lib().ivx_ctx_synchronize(self.h))

    def last_kernel_ms(self):
        return lib().ivx_ctx_last_kernel_ms(self.h)

    def metrics(self):
        """BuildProbeJoinMetrics under the reference's names (joins/utils.rs:399-453)."""
        m = Metrics()
        self._chk0(lib().ivx_ctx_metrics(self.h, C.byref(m)))
        return {f: getattr(m, f) for f, _ in Metrics._fields_}

    def reset_metrics(self):
        lib().ivx_ctx_reset_metrics(self.h)

    def set_memory_limit(self, nbytes):
        self._chk0(lib().ivx_ctx_set_memory_limit(self.h, C.c_uint64(int(nbytes))))

    def set_build_overlap(self, on=True):
        """an overlap index build returns once the routing tables are final; its tail runs beside the next probe's routing
        pass (include/ivx.h: the build columns must then outlive the index's first probe call)"""
        self._chk0(lib().ivx_ctx_set_build_overlap(self.h, C.c_int(int(on))))

    def reserved_bytes(self):
        return lib().ivx_ctx_reserved_bytes(self.h)

    def trim(self, keep_bytes=0):
        """scratch (and the pool of recycled index buffers) back to the device"""
        self._chk0(lib().ivx_ctx_trim(self.h, C.c_uint64(int(keep_bytes))))

    # ---- index ----
    def build(self, kind, key, start, end, n_keys=None):
        key, s, e, n, mem = _cols(key, start, end, np.int32)
        if n_keys is None:
            n_keys = 1 if key is None else (int(key.max()) + 1 if n else 1)
        h = C.c_void_p()
        self._chk(lib().ivx_index_build(self.h, C.c_int(kind), C.c_int(mem), _ptr(key), _ptr(s), _ptr(e),
                                         C.c_uint64(n), C.c_uint32(n_keys), C.byref(h)))
        return Index(self, h, kind)

    # ---- a3 ----
    def overlap_count(self, ix, key, start, end, per_row=False):
        key, s, e, n, mem = _cols(key, start, end, np.int32)
        total = C.c_uint64(0)
        pr = None
        if per_row:
            if mem == MEM_DEVICE:
                import torch
                pr = torch.empty(n, dtype=torch.int32, device=s.device)
            else:
                pr = np.empty(n, np.uint32)
        self._chk(lib().ivx_probe_overlap_count(self.h, ix.h, C.c_int(mem), _ptr(key), _ptr(s), _ptr(e),
                                                 C.c_uint64(n), _ptr(pr), C.byref(total)))
        return (total.value, pr) if per_row else total.value

    def overlap_fill(self, ix, key, start, end, cap=None, out=None):
        """-> (build_idx, probe_idx) of length `written`.  Host arrays: cap defaults to a count pass."""
        key, s, e, n, mem = _cols(key, start, end, np.int32)
        if out is not None:
            ob, op = out
            cap = int(ob.numel()) if _is_torch(ob) else len(ob)
        else:
            if cap is None:
                cap = self.overlap_count(ix, key, s, e)
            if mem == MEM_DEVICE:
                import torch
                ob = torch.empty(max(cap, 1), dtype=torch.int32, device=s.device)
                op = torch.empty(max(cap, 1), dtype=torch.int32, device=s.device)
            else:
                ob = np.empty(max(cap, 1), np.uint32); op = np.empty(max(cap, 1), np.uint32)
        written = C.c_uint64(0)
        st = lib().ivx_probe_overlap_fill(self.h, ix.h, C.c_int(mem), _ptr(key), _ptr(s), _ptr(e), C.c_uint64(n),
                                          _ptr(ob), _ptr(op), C.c_uint64(cap), C.byref(written))
        if st == ERR_CAPACITY:
            raise IvxError(st, f"need {written.value} pairs, cap {cap}")
        self._chk(st)
        w = written.value
        return ob[:w], op[:w]

    def exists(self, ix, key, start, end):
        key, s, e, n, mem = _cols(key, start, end, np.int32)
        if mem == MEM_DEVICE:
            import torch
            out = torch.empty(n, dtype=torch.uint8, device=s.device)
        else:
            out = np.empty(n, np.uint8)
        self._chk(lib().ivx_probe_exists(self.h, ix.h, C.c_int(mem), _ptr(key), _ptr(s), _ptr(e), C.c_uint64(n), _ptr(out)))
        return out

    # ---- a3'': build-side match marks ----
    @staticmethod
    def new_marks(n_bits, device=None):
        """a zeroed mark bitmap of n_bits bits: uint32 words on the host, or int32 on `device` (same bytes)"""
        nw = (int(n_bits) + 31) // 32
        if device is None:
            return np.zeros(max(nw, 1), np.uint32)
        import torch
        return torch.zeros(max(nw, 1), dtype=torch.int32, device=device)

    def mark_build(self, ix, key, start, end, marks, where=None):
        """OR the bit of every build row of `ix` that a row of this batch overlaps into `marks` (ix.rows bits); -> marks.
        where (as_where): only overlaps that pass the threshold count"""
        key, s, e, n, mem = _cols(key, start, end, np.int32)
        if _is_torch(marks) != (mem == MEM_DEVICE):
            raise ValueError("mix of host and device buffers in one call")
        if where is not None:
            wp, _keep = as_where(where)
            self._chk(lib().ivx_probe_mark_build_where(self.h, ix.h, mem, _ptr(key), _ptr(s), _ptr(e), n, wp, _ptr(marks)))
            return marks
        self._chk(lib().ivx_probe_mark_build(self.h, ix.h, C.c_int(mem), _ptr(key), _ptr(s), _ptr(e), C.c_uint64(n), _ptr(marks)))
        return marks

    # ---- a3''': overlap aggregates ----
    def overlap_agg(self, ix, key, start, end, val, outputs=AGG_OUTPUTS, where=None):
        """per probe row, over the build rows the join pairs it with: aggregates of `val` (one int32 or int64 per build row
        of `ix`) -> {name: column} for the names in `outputs` (AGG_OUTPUTS): "count" uint32, the others int64 (min / max of
        a row without a match: INT64_MAX / INT64_MIN).  numpy arrays, or device tensors ("count" then as its int32 bits).
        where (as_where): over the build rows whose overlap passes the threshold."""
        key, s, e, n, mem = _cols(key, start, end, np.int32)
        unknown = [o for o in outputs if o not in AGG_OUTPUTS]
        if unknown:
            raise ValueError(f"overlap_agg: unknown outputs {unknown}")
        if val is not None and _is_torch(val) != (mem == MEM_DEVICE):
            raise ValueError("mix of host and device buffers in one call")
        vb = 8
        if val is not None:
            if mem == MEM_DEVICE:
                import torch
                if val.dtype not in (torch.int32, torch.int64) or not val.is_contiguous():
                    raise ValueError("overlap_agg: val is a contiguous int32 or int64 tensor")
                vb = 4 if val.dtype == torch.int32 else 8
            else:
                val = np.asarray(val)
                if val.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
                    raise ValueError("overlap_agg: val is an int32 or int64 array")
                val = np.ascontiguousarray(val)
                vb = val.dtype.itemsize
        out = {}
        for name in AGG_OUTPUTS:
            if name not in outputs:
                out[name] = None
            elif mem == MEM_DEVICE:
                import torch
                out[name] = torch.empty(max(n, 1), dtype=torch.int32 if name == "count" else torch.int64, device=s.device)
            else:
                out[name] = np.empty(max(n, 1), np.uint32 if name == "count" else np.int64)
        if where is not None:
            wp, _keep = as_where(where)
            self._chk(lib().ivx_probe_overlap_agg_where(self.h, ix.h, mem, _ptr(key), _ptr(s), _ptr(e), n, _ptr(val), vb, wp,
                                                        *[_ptr(out[name]) for name in AGG_OUTPUTS]))
        else:
            self._chk(lib().ivx_probe_overlap_agg(self.h, ix.h, mem, _ptr(key), _ptr(s), _ptr(e), n, _ptr(val), vb,
                                                  *[_ptr(out[name]) for name in AGG_OUTPUTS]))
        return {name: out[name][:n] for name in AGG_OUTPUTS if out[name] is not None}

    # ---- a3'''': overlap select ----
    def overlap_select(self, ix, key, start, end, by="max_overlap", val=None, score=True, where=None):
        """per probe row, of the build rows the join pairs it with, the one that is best by `by` (SEL_BY; ties: the smallest
        build row) -> (build_idx, score): build_idx uint32, NULL_IDX without a match; score int64, the criterion's value at
        the winner (0 without a match), or None with score=False.  `val` (one int32 or int64 per build row of `ix`) is read
        by "min_val" / "max_val" only.  numpy arrays, or device tensors (build_idx then as its int32 bits).
        where (as_where): of the build rows whose overlap passes the threshold."""
        key, s, e, n, mem = _cols(key, start, end, np.int32)
        if by not in SEL_BY:
            raise ValueError(f"overlap_select: by is one of {SEL_BY}, got {by!r}")
        if val is not None and _is_torch(val) != (mem == MEM_DEVICE):
            raise ValueError("mix of host and device buffers in one call")
        vb = 8
        if val is not None:
            if mem == MEM_DEVICE:
                import torch
                if val.dtype not in (torch.int32, torch.int64) or not val.is_contiguous():
                    raise ValueError("overlap_select: val is a contiguous int32 or int64 tensor")
                vb = 4 if val.dtype == torch.int32 else 8
            else:
                val = np.asarray(val)
                if val.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
                    raise ValueError("overlap_select: val is an int32 or int64 array")
                val = np.ascontiguousarray(val)
                vb = val.dtype.itemsize
        if mem == MEM_DEVICE:
            import torch
            bi = torch.empty(max(n, 1), dtype=torch.int32, device=s.device)
            sc = torch.empty(max(n, 1), dtype=torch.int64, device=s.device) if score else None
        else:
            bi = np.empty(max(n, 1), np.uint32)
            sc = np.empty(max(n, 1), np.int64) if score else None
        if where is not None:
            wp, _keep = as_where(where)
            self._chk(lib().ivx_probe_overlap_select_where(self.h, ix.h, mem, _ptr(key), _ptr(s), _ptr(e), n, _ptr(val), vb, SEL_BY.index(by),
                                                           wp, _ptr(bi), _ptr(sc)))
        else:
            self._chk(lib().ivx_probe_overlap_select(self.h, ix.h, mem, _ptr(key), _ptr(s), _ptr(e), n, _ptr(val), vb, SEL_BY.index(by),
                                                     _ptr(bi), _ptr(sc)))
        return bi[:n], (sc[:n] if score else None)

    # ---- a3''''': overlap thresholds (include/ivx_where.h) ----
    def overlap_count_where(self, ix, key, start, end, where=None, per_row=True, exists=True, total=True):
        """the matches of every probe row that pass `where` (as_where; None: all of them) -> {"per_row": uint32 column,
        "exists": uint8 column, "total": int}, each only if wanted.  numpy arrays, or device tensors (per_row as int32 bits)."""
        key, s, e, n, mem = _cols(key, start, end, np.int32)
        wp, _keep = as_where(where)
        pr = ex = None
        if mem == MEM_DEVICE:
            import torch
            if per_row:
                pr = torch.empty(max(n, 1), dtype=torch.int32, device=s.device)
            if exists:
                ex = torch.empty(max(n, 1), dtype=torch.uint8, device=s.device)
        else:
            if per_row:
                pr = np.empty(max(n, 1), np.uint32)
            if exists:
                ex = np.empty(max(n, 1), np.uint8)
        tot = C.c_uint64(0)
        self._chk(lib().ivx_probe_overlap_count_where(self.h, ix.h, mem, _ptr(key), _ptr(s), _ptr(e), n, wp, _ptr(pr), _ptr(ex),
                                                      C.byref(tot) if total else None))
        out = {}
        if per_row:
            out["per_row"] = pr[:n]
        if exists:
            out["exists"] = ex[:n]
        if total:
            out["total"] = tot.value
        return out

    def pairs_where(self, build_idx, probe_idx, bstart, bend, pstart, pend, where=None, cap=None, count_only=False, out=None):
        """the pairs (build_idx[j], probe_idx[j]) whose overlap passes `where` (as_where), in input order, from the two sides'
        int32 coordinate columns -> (out_build, out_probe).  cap=None: a counting call sizes the outputs; count_only: -> the
        count; out: the caller's own (out_build, out_probe).  A cap that is too small raises IvxError(ERR_CAPACITY) whose
        .needed is the size."""
        cols = (build_idx, probe_idx, bstart, bend, pstart, pend)
        dev = _is_torch(build_idx)
        if any(_is_torch(c) != dev for c in cols) or (out is not None and any(_is_torch(o) != dev for o in out)):
            raise ValueError("mix of host and device buffers in one call")
        if dev:
            assert all(c.is_contiguous() for c in cols)
            n, nb, npr = int(build_idx.numel()), int(bstart.numel()), int(pstart.numel())
            assert int(probe_idx.numel()) == n and int(bend.numel()) == nb and int(pend.numel()) == npr
        else:
            build_idx, probe_idx = _np(build_idx, np.uint32), _np(probe_idx, np.uint32)
            bstart, bend, pstart, pend = (_np(c, np.int32) for c in (bstart, bend, pstart, pend))
            n, nb, npr = len(build_idx), len(bstart), len(pstart)
            assert len(probe_idx) == n and len(bend) == nb and len(pend) == npr
        wp, _keep = as_where(where)
        mem = MEM_DEVICE if dev else MEM_HOST
        m = C.c_uint64(0)

        def call(ob, op, cap):
            return lib().ivx_pairs_where(self.h, mem, _ptr(build_idx), _ptr(probe_idx), n, _ptr(bstart), _ptr(bend), nb,
                                         _ptr(pstart), _ptr(pend), npr, wp, _ptr(ob), _ptr(op), cap, C.byref(m))

        if out is not None:
            ob, op = out
            cap = int(ob.numel()) if dev else len(ob)
        else:
            if count_only or cap is None:
                self._chk(call(None, None, 0))
                if count_only:
                    return m.value
                cap = m.value
            if dev:
                import torch
                ob = torch.empty(max(cap, 1), dtype=torch.int32, device=build_idx.device)
                op = torch.empty(max(cap, 1), dtype=torch.int32, device=build_idx.device)
            else:
                ob = np.empty(max(cap, 1), np.uint32); op = np.empty(max(cap, 1), np.uint32)
        st = call(ob, op, cap) if cap else call(None, None, 0)
        if st == ERR_CAPACITY:
            err = IvxError(st, f"need {m.value} pairs, cap {cap}")
            err.needed = m.value
            raise err
        self._chk(st)
        return ob[: m.value], op[: m.value]

    def bits_mark(self, idx, bits, n_bits):
        """OR bit idx[i] into `bits` (NULL_IDX skipped, anything else >= n_bits raises ERR_INVALID); -> bits"""
        dev = _is_torch(bits)
        if _is_torch(idx) != dev:
            raise ValueError("mix of host and device buffers in one call")
        if dev:
            assert idx.is_contiguous() and bits.is_contiguous()
            n = int(idx.numel())
        else:
            idx = np.ascontiguousarray(idx, np.uint32)
            n = len(idx)
        self._chk(lib().ivx_bits_mark(self.h, C.c_int(MEM_DEVICE if dev else MEM_HOST), _ptr(idx), C.c_uint64(n), _ptr(bits), C.c_uint64(int(n_bits))))
        return bits

    def bits_select(self, bits, n_bits, want_set=True, cap=None, count_only=False):
        """positions < n_bits whose bit is set (or clear), ascending.  cap=None: a counting call sizes the output.
        count_only: -> the count.  A cap that is too small raises IvxError(ERR_CAPACITY) whose .needed is the size."""
        dev = _is_torch(bits)
        mem, n_bits, want = C.c_int(MEM_DEVICE if dev else MEM_HOST), C.c_uint64(int(n_bits)), C.c_int(int(bool(want_set)))
        m = C.c_uint64(0)
        if count_only or cap is None:
            self._chk(lib().ivx_bits_select(self.h, mem, _ptr(bits), n_bits, want, None, C.c_uint64(0), C.byref(m)))
            if count_only:
                return m.value
            cap = m.value
        if dev:
            import torch
            out = torch.empty(max(cap, 1), dtype=torch.int32, device=bits.device)
        else:
            out = np.empty(max(cap, 1), np.uint32)
        st = lib().ivx_bits_select(self.h, mem, _ptr(bits), n_bits, want, _ptr(out), C.c_uint64(cap), C.byref(m))
        if st == ERR_CAPACITY:
            err = IvxError(st, f"need {m.value} positions, cap {cap}")
            err.needed = m.value
            raise err
        self._chk(st)
        return out[: m.value]

    # ---- a4 / a5 ----
    def _per_row_i64(self, fn, ix, key, start, end, strict, out=None):
        key, s, e, n, mem = _cols(key, start, end, np.int32)
        if out is not None:
            assert len(out) >= n                                    # (a caller's own int64 buffer, e.g. one it has touched before)
        elif mem == MEM_DEVICE:
            import torch
            out = torch.empty(n, dtype=torch.int64, device=s.device)
        else:
            out = np.empty(n, np.int64)
        self._chk(fn(self.h, ix.h, C.c_int(mem), _ptr(key), _ptr(s), _ptr(e), C.c_uint64(n), C.c_int(int(strict)), _ptr(out)))
        return out

    def count_overlaps(self, ix, key, start, end, strict=False, out=None):
        return self._per_row_i64(lib().ivx_probe_count, ix, key, start, end, strict, out)

    def coverage(self, ix, key, start, end, strict=False, out=None):
        return self._per_row_i64(lib().ivx_probe_coverage, ix, key, start, end, strict, out)

    # ---- a6 ----
    def nearest(self, ix, key, start, end, k=1, overlap=True, strict=False, distance=True):
        key, s, e, n, mem = _cols(key, start, end, np.int32)
        cap = n * max(int(k), 1)
        if mem == MEM_DEVICE:
            import torch
            ob = torch.empty(max(cap, 1), dtype=torch.int32, device=s.device)
            op = torch.empty(max(cap, 1), dtype=torch.int32, device=s.device)
            od = torch.empty(max(cap, 1), dtype=torch.int64, device=s.device) if distance else None
        else:
            ob = np.empty(max(cap, 1), np.uint32); op = np.empty(max(cap, 1), np.uint32)
            od = np.empty(max(cap, 1), np.int64) if distance else None
        rows = C.c_uint64(0)
        self._chk(lib().ivx_probe_nearest(self.h, ix.h, C.c_int(mem), _ptr(key), _ptr(s), _ptr(e), C.c_uint64(n),
                                           C.c_int(int(strict)), C.c_uint32(int(k)), C.c_int(int(overlap)),
                                           _ptr(ob), _ptr(op), _ptr(od), C.c_uint64(cap), C.byref(rows)))
        r = rows.value
        return ob[:r], op[:r], (od[:r] if distance else None)

    # ---- a6': one side only and / or within a distance cap (include/ivx_nearest.h) ----
    def nearest_dir(self, ix, key, start, end, k=1, overlap=True, strict=False, distance=True, direction="any", max_distance=None):
        """nearest() restricted to build rows that end before the probe row ("before" / "upstream") or start after it ("after" /
        "downstream"), and / or to build rows no farther than max_distance (None: no cap).  Direction does not touch
        overlapping rows: `overlap` alone decides them.  direction="any" without a cap is nearest()."""
        d = NEAR_ALIASES.get(direction, direction)
        if d not in NEAR_DIRECTIONS:
            raise ValueError(f"direction must be one of {NEAR_DIRECTIONS + tuple(NEAR_ALIASES)}, got {direction!r}")
        if max_distance is not None and int(max_distance) < 0:
            raise ValueError(f"max_distance must be >= 0 or None, got {max_distance!r}")
        key, s, e, n, mem = _cols(key, start, end, np.int32)
        cap = n * max(int(k), 1)
        if mem == MEM_DEVICE:
            import torch
            ob = torch.empty(max(cap, 1), dtype=torch.int32, device=s.device)
            op = torch.empty(max(cap, 1), dtype=torch.int32, device=s.device)
            od = torch.empty(max(cap, 1), dtype=torch.int64, device=s.device) if distance else None
        else:
            ob = np.empty(max(cap, 1), np.uint32); op = np.empty(max(cap, 1), np.uint32)
            od = np.empty(max(cap, 1), np.int64) if distance else None
        rows = C.c_uint64(0)
        self._chk(lib().ivx_probe_nearest_dir(self.h, ix.h, mem, _ptr(key), _ptr(s), _ptr(e), n, int(strict), int(k), int(overlap),
                                               NEAR_DIRECTIONS.index(d), -1 if max_distance is None else int(max_distance),
                                               _ptr(ob), _ptr(op), _ptr(od), cap, C.byref(rows)))
        r = rows.value
        return ob[:r], op[:r], (od[:r] if distance else None)

    # ---- a7..a9 ----
    def merge(self, key, start, end, n_keys=None, min_dist=0, strict=False):
        key, s, e, n, mem = _cols(key, start, end, np.int64)
        if n_keys is None:
            n_keys = 1 if key is None else (int(key.max()) + 1 if n else 1)
        cap = max(n, 1)
        if mem == MEM_DEVICE:
            import torch
            dev = s.device
            ok = torch.empty(cap, dtype=torch.int32, device=dev); os_ = torch.empty(cap, dtype=torch.int64, device=dev)
            oe = torch.empty(cap, dtype=torch.int64, device=dev); on = torch.empty(cap, dtype=torch.int64, device=dev)
        else:
            ok = np.empty(cap, np.uint32); os_ = np.empty(cap, np.int64); oe = np.empty(cap, np.int64); on = np.empty(cap, np.int64)
        m = C.c_uint64(0)
        self._chk(lib().ivx_merge(self.h, C.c_int(mem), _ptr(key), _ptr(s), _ptr(e), C.c_uint64(n), C.c_uint32(n_keys),
                                   C.c_int64(int(min_dist)), C.c_int(int(strict)), _ptr(ok), _ptr(os_), _ptr(oe), _ptr(on),
                                   C.c_uint64(cap), C.byref(m)))
        m = m.value
        return ok[:m], os_[:m], oe[:m], on[:m]

    def subtract(self, lkey, ls, le, rkey, rs, re, n_keys=None, strict=False, cap=None, between=None):
        """cap=None: sizing call, then the fill call (which reuses the sizing call's sorted sides).  cap=N: one call into
        buffers of N rows.  between: callable run between the two calls (tests)."""
        lkey, ls, le, nl, mem = _cols(lkey, ls, le, np.int64)
        rkey, rs, re, nr, mem2 = _cols(rkey, rs, re, np.int64)
        assert mem == mem2
        if n_keys is None:
            mk = 0
            for k_, n_ in ((lkey, nl), (rkey, nr)):
                if k_ is not None and n_:
                    mk = max(mk, int(k_.max()))
            n_keys = mk + 1
        args = (C.c_int(mem), _ptr(lkey), _ptr(ls), _ptr(le), C.c_uint64(nl), _ptr(rkey), _ptr(rs), _ptr(re),
                C.c_uint64(nr), C.c_uint32(n_keys), C.c_int(int(strict)))
        def bufs(cap):
            if mem == MEM_DEVICE:
                import torch
                dev = ls.device
                return (torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int64, device=dev),
                        torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int32, device=dev))
            return np.empty(cap, np.uint32), np.empty(cap, np.int64), np.empty(cap, np.int64), np.empty(cap, np.uint32)
        # sizing call (counting half only), then the fill call: the fragment count has no useful a-priori bound
        if cap is None:
            m = C.c_uint64(0)
            self._chk(lib().ivx_subtract(self.h, *args, None, None, None, None, C.c_uint64(0), C.byref(m)))
            cap = max(m.value, 1)
            if between is not None:
                between()
        ok, os_, oe, orow = bufs(cap)
        m2 = C.c_uint64(0)
        self._chk(lib().ivx_subtract(self.h, *args, _ptr(ok), _ptr(os_), _ptr(oe), _ptr(orow), C.c_uint64(cap), C.byref(m2)))
        m2 = m2.value
        return ok[:m2], os_[:m2], oe[:m2], orow[:m2]

    def intersect_left_form(self):
        """after an intersect: which sort its left side took (the words of SWEEP_LEFT_SLOTS behind those of sweep_form()) as a dict"""
        n = len(SWEEP_SLOTS) + len(SWEEP_LEFT_SLOTS)
        out = (C.c_uint32 * n)()
        self._chk0(lib().ivx_debug_sweep_form(self.h, out, C.c_uint32(n)))
        return dict(zip(SWEEP_LEFT_SLOTS, list(out)[len(SWEEP_SLOTS):]))

    # (Ctx.subtract keeps its own copy of this normalisation inline, as it was before intersect came: the two must stay alike)
    def _two_sides(self, lkey, ls, le, rkey, rs, re, n_keys, strict):
        """both sides of subtract / intersect normalised -> (the C arguments from `mem` to `strict`, mem, nl, device or None)"""
        lkey, ls, le, nl, mem = _cols(lkey, ls, le, np.int64)
        rkey, rs, re, nr, mem2 = _cols(rkey, rs, re, np.int64)
        assert mem == mem2
        if n_keys is None:
            mk = 0
            for k_, n_ in ((lkey, nl), (rkey, nr)):
                if k_ is not None and n_:
                    mk = max(mk, int(k_.max()))
            n_keys = mk + 1
        args = (C.c_int(mem), _ptr(lkey), _ptr(ls), _ptr(le), C.c_uint64(nl), _ptr(rkey), _ptr(rs), _ptr(re),
                C.c_uint64(nr), C.c_uint32(n_keys), C.c_int(int(strict)))
        return args, (lkey, ls, le, rkey, rs, re), mem, nl, (ls.device if mem == MEM_DEVICE else None)

    def intersect(self, lkey, ls, le, rkey, rs, re, n_keys=None, strict=False, cap=None):
        """the pieces of the left rows that the right side covers (include/ivx.h ivx_intersect) -> (key, start, end, left row).
        cap=None: sizing call, then the fill call (which does the work again: no plan is kept).  cap=N: one call into
        buffers of N rows."""
        args, keep, mem, _, dev = self._two_sides(lkey, ls, le, rkey, rs, re, n_keys, strict)
        if cap is None:
            m = C.c_uint64(0)
            self._chk(lib().ivx_intersect(self.h, *args, None, None, None, None, C.c_uint64(0), C.byref(m)))
            cap = max(m.value, 1)
        if mem == MEM_DEVICE:
            import torch
            ok, os_, oe, orow = (torch.empty(cap, dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int64, torch.int32))
        else:
            ok, os_, oe, orow = np.empty(cap, np.uint32), np.empty(cap, np.int64), np.empty(cap, np.int64), np.empty(cap, np.uint32)
        m2 = C.c_uint64(0)
        self._chk(lib().ivx_intersect(self.h, *args, _ptr(ok), _ptr(os_), _ptr(oe), _ptr(orow), C.c_uint64(cap), C.byref(m2)))
        m2 = m2.value
        return ok[:m2], os_[:m2], oe[:m2], orow[:m2]

    def intersect_count(self, lkey, ls, le, rkey, rs, re, n_keys=None, strict=False):
        """the sizing call of intersect alone -> the number of pieces"""
        args, keep, _, _, _ = self._two_sides(lkey, ls, le, rkey, rs, re, n_keys, strict)
        m = C.c_uint64(0)
        self._chk(lib().ivx_intersect(self.h, *args, None, None, None, None, C.c_uint64(0), C.byref(m)))
        return m.value

    def intersect_paths(self, lkey, ls, le, rkey, rs, re, n_keys=None, strict=False):
        """what the count pass of an intersect sizing call for these inputs does (test hook ivx_debug_intersect_paths) ->
        (wg, row_esc, n_out): wg uint32 [workgroups, len(ISECT_DBG_SLOTS)], row_esc uint8 per left row at its input index"""
        args, keep, mem, nl, _ = self._two_sides(lkey, ls, le, rkey, rs, re, n_keys, strict)
        g = intersect_geometry()
        nwg = (nl + 1 + g["rows_per_wg"] - 1) // g["rows_per_wg"]
        wg = np.zeros((nwg, g["dbg_words"]), np.uint32); esc = np.zeros(max(nl, 1), np.uint8)
        n_wg, n_rows, n_out = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().ivx_debug_intersect_paths(self.h, *args, _ptr(wg), C.c_uint64(nwg), _ptr(esc), C.c_uint64(len(esc)),
                                                   C.byref(n_wg), C.byref(n_rows), C.byref(n_out)))
        return wg[:n_wg.value], esc[:n_rows.value], n_out.value

    def sweep_form(self):
        """the forms the last merge / cluster / complement of this context took (test hook ivx_debug_sweep_form) as a dict of
        the SWEEP_SLOTS: what its sort and its packed sweep decided on the host.  After a subtract: its last sort's; after an
        intersect: its right side's."""
        out = (C.c_uint32 * len(SWEEP_SLOTS))()
        self._chk0(lib().ivx_debug_sweep_form(self.h, out, C.c_uint32(len(SWEEP_SLOTS))))
        return dict(zip(SWEEP_SLOTS, list(out)))

    def debug_state(self):
        """what this context carries from one call to the next (test hook ivx_debug_ctx_state) as a dict of the STATE_SLOTS:
        both plans and their scratch-slot masks, the pending build tail, the slots that hold memory, the free buffers of
        the index pool on this device, the fill calls so far that a plan served"""
        out = (C.c_uint64 * len(STATE_SLOTS))()
        self._chk0(lib().ivx_debug_ctx_state(self.h, out, C.c_uint32(len(STATE_SLOTS))))
        return dict(zip(STATE_SLOTS, list(out)))

    def debug_poison(self, word, what):
        """word (0 or 1) into every 32-bit word of what the POISON_* bits of `what` select (test hook ivx_debug_poison);
        refused while a build tail is pending.  -> the mask of scratch slots written"""
        wrote = C.c_uint64(0)
        self._chk0(lib().ivx_debug_poison(self.h, C.c_uint32(int(word)), C.c_int(int(what)), C.byref(wrote)))
        return wrote.value

    # ---- f1, f2 ----
    def cluster(self, key, start, end, n_keys=None, min_dist=0, strict=False, key_base=None, rows=True):
        """-> dict(key, start, end, row, cluster, cluster_start, cluster_end [rows sorted by (key,start,end,row)],
                   key_clusters[n_keys], n_clusters); rows=False only counts the clusters per key."""
        key, s, e, n, mem = _cols(key, start, end, np.int64)
        if n_keys is None:
            n_keys = 1 if key is None else (int(key.max()) + 1 if n else 1)
        cap = max(n, 1)
        if mem == MEM_DEVICE:
            import torch
            dev = s.device
            mk = lambda dt, m=cap: torch.empty(m, dtype=dt, device=dev)
            i32, i64 = torch.int32, torch.int64
            if key_base is not None:
                key_base = torch.as_tensor(key_base, dtype=torch.int64, device=dev).contiguous()
        else:
            mk = lambda dt, m=cap: np.empty(m, dt)
            i32, i64 = np.uint32, np.int64
            if key_base is not None:
                key_base = np.ascontiguousarray(key_base, np.int64)
        out = {}
        if rows:
            out = dict(key=mk(i32), start=mk(i64), end=mk(i64), row=mk(i32), cluster=mk(i64), cluster_start=mk(i64), cluster_end=mk(i64))
        kc = mk(i64, max(n_keys, 1))
        m = C.c_uint64(0)
        g = lambda name: _ptr(out[name]) if rows else None
        self._chk(lib().ivx_cluster(self.h, C.c_int(mem), _ptr(key), _ptr(s), _ptr(e), C.c_uint64(n), C.c_uint32(n_keys),
                                     C.c_int64(int(min_dist)), C.c_int(int(strict)), _ptr(key_base) if key_base is not None else None,
                                     g("key"), g("start"), g("end"), g("row"), g("cluster"), g("cluster_start"), g("cluster_end"),
                                     _ptr(kc), C.byref(m)))
        out = {k_: v[:n] for k_, v in out.items()}
        out["key_clusters"] = kc[:n_keys]
        out["n_clusters"] = m.value
        return out

    def complement(self, key, start, end, vkey=None, vstart=None, vend=None, n_keys=None, strict=False):
        """-> (key, start, end); without view rows every key gets the implicit view [0, i64::MAX)."""
        key, s, e, n, mem = _cols(key, start, end, np.int64)
        if vstart is None:
            nv, vk, vs, ve = 0, None, None, None
        else:
            vk, vs, ve, nv, mem2 = _cols(vkey, vstart, vend, np.int64)
            assert mem == mem2
        if n_keys is None:
            mx = 0
            for k_, n_ in ((key, n), (vk, nv)):
                if k_ is not None and n_:
                    mx = max(mx, int(k_.max()))
            n_keys = mx + 1
        args = (C.c_int(mem), _ptr(key), _ptr(s), _ptr(e), C.c_uint64(n), _ptr(vk), _ptr(vs), _ptr(ve), C.c_uint64(nv),
                C.c_uint32(n_keys), C.c_int(int(strict)))
        def bufs(cap):
            if mem == MEM_DEVICE:
                import torch
                dev = s.device
                return torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
            return np.empty(cap, np.uint32), np.empty(cap, np.int64), np.empty(cap, np.int64)
        cap = max(n + 2 * nv + 2 * n_keys + 16, 1)          # enough unless views overlap each other heavily; else one retry
        m2 = C.c_uint64(0)
        ok, os_, oe = bufs(cap)
        st = lib().ivx_complement(self.h, *args, _ptr(ok), _ptr(os_), _ptr(oe), C.c_uint64(cap), C.byref(m2))
        if st == ERR_CAPACITY:
            cap = m2.value
            ok, os_, oe = bufs(cap)
            st = lib().ivx_complement(self.h, *args, _ptr(ok), _ptr(os_), _ptr(oe), C.c_uint64(cap), C.byref(m2))
        self._chk(st)
        m2 = m2.value
        return ok[:m2], os_[:m2], oe[:m2]

    # ---- g: depth ----
    def cigar_parse(self, text_offsets, text):
        """text CIGARs -> packed ops (include/ivx.h ivx_cigar_parse): text_offsets int32 (Utf8) or int64 (LargeUtf8)
        [n_reads + 1], text uint8; numpy arrays or torch device tensors.  -> (offsets int32 [n_reads + 1], ops uint32)"""
        mem = _mem_of(text_offsets, text)
        if mem == MEM_DEVICE:
            import torch
            assert text_offsets.is_contiguous() and (text is None or text.is_contiguous())
            large = int(text_offsets.dtype == torch.int64)
            assert large or text_offsets.dtype == torch.int32
            n_reads = max(int(text_offsets.numel()) - 1, 0)
        else:
            text_offsets = np.ascontiguousarray(text_offsets)
            large = int(text_offsets.dtype == np.int64)
            if not large:
                text_offsets = np.ascontiguousarray(text_offsets, np.int32)
            text = _np(text, np.uint8)
            n_reads = max(len(text_offsets) - 1, 0)
        head = (self.h, C.c_int(mem), C.c_int(large), _ptr(text_offsets), _ptr(text), C.c_uint64(n_reads))
        m = C.c_uint64(0)
        self._chk0(lib().ivx_cigar_parse(*head, None, None, 0, C.byref(m)))
        cap = m.value
        if mem == MEM_DEVICE:
            import torch
            off = torch.empty(n_reads + 1, dtype=torch.int32, device=text_offsets.device)
            ops = torch.empty(max(cap, 1), dtype=torch.int32, device=text_offsets.device)
        else:
            off = np.empty(n_reads + 1, np.int32)
            ops = np.empty(max(cap, 1), np.uint32)
        if n_reads == 0:
            off[:] = 0
        self._chk0(lib().ivx_cigar_parse(*head, _ptr(off), _ptr(ops), C.c_uint64(max(cap, 1)), C.byref(m)))
        return off, ops[:m.value]

    def depth(self, rkey=None, rpos=None, rflags=None, rmapq=None, cigar_offsets=None, cigar_ops=None,
              skey=None, sstart=None, send=None, sweight=None, n_keys=None, key_len=None, filter_flag=1796, min_mapq=0,
              cap=None, outputs=(True, True, True, True), text_offsets=None, text=None):
        """coverage blocks of reads (rkey/rpos/rflags/rmapq + the Arrow Binary column cigar_offsets [bytes] / cigar_ops
        [packed u32 ops]) and of weighted segments (skey/sstart/send/sweight); numpy arrays or torch device tensors.
        text_offsets (int32: Utf8, int64: LargeUtf8) / text (uint8) in place of cigar_offsets / cigar_ops: the cigar
        column as text (ivx_depth_text).
        cap=None: a sizing call, then the fill call.  outputs: which of (key, start, end, coverage) to ask for.
        -> (key, start, end, coverage), None where not asked for."""
        args, mem, cols, n_keys = self._depth_args(rkey, rpos, rflags, rmapq, cigar_offsets, cigar_ops, skey, sstart, send, sweight,
                                                   n_keys, key_len, filter_flag, min_mapq, text_offsets, text)
        fn = lib().ivx_depth if text_offsets is None else lib().ivx_depth_text

        def bufs(cap):
            if mem == MEM_DEVICE:
                import torch
                dev = next(c for c in cols if c is not None).device
                return [torch.empty(cap, dtype=torch.int32, device=dev) if w else None for w in outputs]
            return [np.empty(cap, dt) if w else None for w, dt in zip(outputs, (np.uint32, np.uint32, np.uint32, np.int32))]
        if cap is None:
            m = C.c_uint64(0)
            self._chk(fn(self.h, *args, None, None, None, None, 0, C.byref(m)))
            cap = max(m.value, 1)
        out = bufs(cap)
        m2 = C.c_uint64(0)
        st = fn(self.h, *args, *[_ptr(o) for o in out], cap, C.byref(m2))
        if st == ERR_CAPACITY:
            raise IvxError(st, f"{lib().ivx_last_error(self.h).decode()} (needed {m2.value})")
        self._chk(st)
        return tuple(None if o is None else o[:m2.value] for o in out)

    def depth_profile(self, rkey=None, rpos=None, rflags=None, rmapq=None, cigar_offsets=None, cigar_ops=None,
                      skey=None, sstart=None, send=None, sweight=None, n_keys=None, key_len=None, filter_flag=1796, min_mapq=0,
                      text_offsets=None, text=None):
        """the depth profile of the same inputs as depth() -> DepthProfile (per-base output: .expand())"""
        args, mem, cols, n_keys = self._depth_args(rkey, rpos, rflags, rmapq, cigar_offsets, cigar_ops, skey, sstart, send, sweight,
                                                   n_keys, key_len, filter_flag, min_mapq, text_offsets, text)
        h = C.c_void_p()
        fn = lib().ivx_depth_profile_build if text_offsets is None else lib().ivx_depth_profile_build_text
        self._chk(fn(self.h, *args, C.byref(h)))
        dev = next(c for c in cols if c is not None).device if mem == MEM_DEVICE else None
        return DepthProfile(self, h, n_keys, dev)

    def _depth_args(self, rkey, rpos, rflags, rmapq, cigar_offsets, cigar_ops, skey, sstart, send, sweight, n_keys, key_len,
                    filter_flag, min_mapq, text_offsets=None, text=None):
        """the 17 input arguments of ivx_depth / ivx_depth_profile_build (18 with text_offsets / text, for the _text calls)
        -> (ctypes args, mem, normalised columns, n_keys)"""
        cols = [rkey, rpos, rflags, rmapq, cigar_offsets, cigar_ops, skey, sstart, send, sweight, key_len]
        if text_offsets is not None and (cigar_offsets is not None or cigar_ops is not None):
            raise ValueError("give the cigar column as packed ops or as text, not both")
        mem = _mem_of(*cols, text_offsets, text)
        large = 0
        if text_offsets is not None:
            if mem == MEM_DEVICE:
                import torch
                assert text_offsets.is_contiguous() and (text is None or text.is_contiguous())
                large = int(text_offsets.dtype == torch.int64)
                assert large or text_offsets.dtype == torch.int32
            else:
                text_offsets = np.ascontiguousarray(text_offsets)
                large = int(text_offsets.dtype == np.int64)
                if not large:
                    text_offsets = np.ascontiguousarray(text_offsets, np.int32)
                text = _np(text, np.uint8)
        n_reads = 0 if rpos is None else (int(rpos.numel()) if _is_torch(rpos) else len(rpos))
        n_seg = 0 if sstart is None else (int(sstart.numel()) if _is_torch(sstart) else len(sstart))
        if mem == MEM_DEVICE:
            assert all(c is None or c.is_contiguous() for c in cols)
        else:
            dts = [np.uint32, np.uint32, np.uint32, np.uint32, np.int32, np.uint32, np.uint32, np.uint32, np.uint32, np.int32, np.uint32]
            cols = [_np(c, dt) for c, dt in zip(cols, dts)]
        rkey, rpos, rflags, rmapq, cigar_offsets, cigar_ops, skey, sstart, send, sweight, key_len = cols
        if n_keys is None:
            if key_len is not None:
                n_keys = int(key_len.numel()) if _is_torch(key_len) else len(key_len)
            else:
                mk = 0
                for k_, n_ in ((rkey, n_reads), (skey, n_seg)):
                    if k_ is not None and n_:
                        kk = k_.to("cpu").numpy().view(np.uint32) if _is_torch(k_) else k_
                        kk = kk[kk != NULL_IDX]
                        if len(kk):
                            mk = max(mk, int(kk.max()))
                n_keys = mk + 1
        cig = (_ptr(cigar_offsets), _ptr(cigar_ops)) if text_offsets is None else (C.c_int(large), _ptr(text_offsets), _ptr(text))
        args = (C.c_int(mem), _ptr(rkey), _ptr(rpos), _ptr(rflags), _ptr(rmapq), *cig, n_reads,
                _ptr(skey), _ptr(sstart), _ptr(send), _ptr(sweight), n_seg, n_keys, _ptr(key_len), int(filter_flag), int(min_mapq))
        return args, mem, cols + [text_offsets, text], n_keys

    # ---- f3: compute::take of payload columns ----
    def take_fixed(self, src, idx, src_valid_bits=None, want_valid=True):
        """src: 1-D array (numpy or torch) of a fixed-width type (1, 2, 4, 8, 16 or 32 bytes per element; wider
        records as a 2-D uint8 array [n_src, width]); idx: uint32 rows, NULL_IDX = null.  -> (out, valid u8 or None)"""
        dev = _is_torch(src)
        if _is_torch(idx) != dev:
            raise ValueError("mix of host and device buffers in one call")
        if dev:
            import torch
            assert src.is_contiguous() and idx.is_contiguous()
            n_src = src.shape[0]
            width = src.element_size() * (src.shape[1] if src.dim() == 2 else 1)
            n = int(idx.numel())
            out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
            valid = torch.empty(max(n, 1), dtype=torch.uint8, device=src.device) if want_valid else None
            svb = src_valid_bits
        else:
            src = np.ascontiguousarray(src); idx = np.ascontiguousarray(idx, np.uint32)
            n_src = src.shape[0]
            width = src.dtype.itemsize * (src.shape[1] if src.ndim == 2 else 1)
            n = len(idx)
            out = np.empty((n,) + src.shape[1:], src.dtype)
            valid = np.empty(max(n, 1), np.uint8) if want_valid else None
            svb = None if src_valid_bits is None else np.ascontiguousarray(src_valid_bits, np.uint8)
        self._chk(lib().ivx_take_fixed(self.h, C.c_int(MEM_DEVICE if dev else MEM_HOST), _ptr(src), C.c_uint32(width), C.c_uint64(n_src),
                                        _ptr(svb), _ptr(idx), C.c_uint64(n), _ptr(out), _ptr(valid)))
        return out, (valid[:n] if valid is not None else None)

    def scatter_fixed(self, src, idx, out):
        """out[idx[i]] = src[i] (idx: uint32 rows of `out`); -> out"""
        dev = _is_torch(src)
        if _is_torch(idx) != dev or _is_torch(out) != dev:
            raise ValueError("mix of host and device buffers in one call")
        if dev:
            assert src.is_contiguous() and idx.is_contiguous() and out.is_contiguous() and src.dtype == out.dtype
            width, n, n_out = src.element_size(), int(idx.numel()), int(out.numel())
        else:
            src = np.ascontiguousarray(src, out.dtype); idx = np.ascontiguousarray(idx, np.uint32)
            assert out.flags.c_contiguous
            width, n, n_out = out.dtype.itemsize, len(idx), len(out)
        assert (int(src.numel()) if dev else len(src)) == n
        self._chk(lib().ivx_scatter_fixed(self.h, C.c_int(MEM_DEVICE if dev else MEM_HOST), _ptr(src), C.c_uint32(width), _ptr(idx),
                                           C.c_uint64(n), _ptr(out), C.c_uint64(n_out)))
        return out

    def take_utf8(self, offsets, data, idx, src_valid_bits=None, want_valid=True):
        """offsets: int32 (Utf8/Binary) or int64 (LargeUtf8/LargeBinary) [n_src+1]; data: uint8 bytes.
        -> (out_offsets, out_data u8, valid u8 or None)"""
        dev = _is_torch(offsets)
        if dev:
            import torch
            large = offsets.dtype == torch.int64
            n_src, nbytes, n = int(offsets.numel()) - 1, int(data.numel()), int(idx.numel())
            mk = lambda m, dt: torch.empty(max(m, 1), dtype=dt, device=offsets.device)
            odt, u8 = offsets.dtype, torch.uint8
            svb = src_valid_bits
        else:
            offsets = np.ascontiguousarray(offsets); data = np.ascontiguousarray(data, np.uint8); idx = np.ascontiguousarray(idx, np.uint32)
            large = offsets.dtype == np.int64
            assert large or offsets.dtype == np.int32
            n_src, nbytes, n = len(offsets) - 1, len(data), len(idx)
            mk = lambda m, dt: np.empty(max(m, 1), dt)
            odt, u8 = offsets.dtype, np.uint8
            svb = None if src_valid_bits is None else np.ascontiguousarray(src_valid_bits, np.uint8)
        mem = C.c_int(MEM_DEVICE if dev else MEM_HOST)
        out_off = mk(n + 1, odt)
        valid = mk(n, u8) if want_valid else None
        need = C.c_uint64(0)
        head = (self.h, mem, C.c_int(int(large)), _ptr(offsets), _ptr(data), C.c_uint64(n_src), C.c_uint64(nbytes), _ptr(svb), _ptr(idx), C.c_uint64(n))
        # optimistic size from the mean source string length; the call reports the exact need if it is short
        cap = int(n * (nbytes / max(n_src, 1)) * 1.5) + 64
        out_data = mk(cap, u8)
        st = lib().ivx_take_utf8(*head, _ptr(out_off), _ptr(out_data), C.c_uint64(cap), C.byref(need), _ptr(valid))
        if st == ERR_CAPACITY:
            cap = max(need.value, 1)
            out_data = mk(cap, u8)
            st = lib().ivx_take_utf8(*head, _ptr(out_off), _ptr(out_data), C.c_uint64(cap), C.byref(need), _ptr(valid))
        self._chk(st)
        return out_off[: n + 1], out_data[: need.value], (valid[:n] if valid is not None else None)

    def take_bits(self, src_bits, n_src, idx, src_valid_bits=None, want_valid=True):
        """src_bits: uint8 bitmap (LSB first, bit offset 0) of a Boolean column of n_src rows.
        -> (out_bits u8 [(n+7)/8], valid u8 or None)"""
        dev = _is_torch(src_bits)
        if _is_torch(idx) != dev:
            raise ValueError("mix of host and device buffers in one call")
        if dev:
            import torch
            assert src_bits.is_contiguous() and idx.is_contiguous()
            n = int(idx.numel())
            mk = lambda m: torch.empty(max(m, 1), dtype=torch.uint8, device=src_bits.device)
            svb = src_valid_bits
        else:
            src_bits = np.ascontiguousarray(src_bits, np.uint8); idx = np.ascontiguousarray(idx, np.uint32)
            n = len(idx)
            mk = lambda m: np.empty(max(m, 1), np.uint8)
            svb = None if src_valid_bits is None else np.ascontiguousarray(src_valid_bits, np.uint8)
        nb = (n + 7) // 8
        out = mk(nb)
        valid = mk(n) if want_valid else None
        self._chk(lib().ivx_take_bits(self.h, C.c_int(MEM_DEVICE if dev else MEM_HOST), _ptr(src_bits), C.c_uint64(int(n_src)), _ptr(svb),
                                       _ptr(idx), C.c_uint64(n), _ptr(out), _ptr(valid)))
        return out[:nb], (valid[:n] if valid is not None else None)

    def take_view(self, views, data_bufs, idx, src_valid_bits=None, want_valid=True):
        """views: uint8 [n_src, 16] (Utf8View / BinaryView); data_bufs: list of the variadic uint8 data buffers.
        Sizes first, then fills.  -> (out_views u8 [n, 16], out_data u8 = the one data buffer of the output, valid u8 or None)"""
        dev = _is_torch(views)
        if _is_torch(idx) != dev or any(_is_torch(b) != dev for b in data_bufs):
            raise ValueError("mix of host and device buffers in one call")
        if dev:
            import torch
            assert views.is_contiguous() and idx.is_contiguous() and all(b.is_contiguous() for b in data_bufs)
            n_src, n = int(views.numel()) // 16, int(idx.numel())
            sizes = [int(b.numel()) for b in data_bufs]
            mk = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=views.device)
            svb = src_valid_bits
        else:
            views = np.ascontiguousarray(views, np.uint8); idx = np.ascontiguousarray(idx, np.uint32)
            data_bufs = [np.ascontiguousarray(b, np.uint8) for b in data_bufs]
            n_src, n = views.size // 16, len(idx)
            sizes = [len(b) for b in data_bufs]
            mk = lambda *shape: np.empty(shape, np.uint8)
            svb = None if src_valid_bits is None else np.ascontiguousarray(src_valid_bits, np.uint8)
        nb = len(data_bufs)
        table = (C.c_void_p * max(nb, 1))(*[_ptr(b).value for b in data_bufs])        # host table of the buffers' pointers, in either mode
        nbytes = (C.c_uint64 * max(nb, 1))(*sizes)
        valid = mk(max(n, 1)) if want_valid else None
        need = C.c_uint64(0)
        head = (self.h, C.c_int(MEM_DEVICE if dev else MEM_HOST), _ptr(views), table, nbytes, C.c_uint32(nb), C.c_uint64(n_src), _ptr(svb),
                _ptr(idx), C.c_uint64(n))
        self._chk(lib().ivx_take_view(*head, None, None, C.c_uint64(0), C.byref(need), _ptr(valid)))
        cap = max(need.value, 1)
        out_views, out_data = mk(max(n, 1), 16), mk(cap)
        self._chk(lib().ivx_take_view(*head, _ptr(out_views), _ptr(out_data), C.c_uint64(cap), C.byref(need), _ptr(valid)))
        return out_views[:n], out_data[: need.value], (valid[:n] if valid is not None else None)
