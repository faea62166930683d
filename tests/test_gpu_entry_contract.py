"""-m gpu: the contract of the C entry layer (csrc/ivx_capi.hip), entry by entry -- what staging, copy-back and the argument
checks do, whatever the kernels compute.

1. Host mode equals device mode: every entry that takes `mem` gets the same small seeded input as numpy arrays and as
   device tensors; all outputs, the scalar ones included, must be bit-identical (1 000 rows over 3 keys, the empty call, the
   one-row call; the sizing / fill pairs at a sizing call, an exact capacity and a capacity one short).
2. Argument errors: (entry, one bad argument) -> (status, exact ivx_last_error text), the texts as literals of the source.
3. A host-mode call that fails its argument check leaves the caller's output buffers untouched.

No bad argument here reaches a kernel: each is one the entry layer rejects on the host.  The entries are called through
pyivx.lib() with ctypes directly: pyivx's wrappers would allocate, retry or reject first.
"""
import ctypes as C

import numpy as np
import pytest

from entry_cases import (CAPACITY, CASES, INVALID, NK, NULL, OK, SIZES, UNSUPPORTED, Buf, Env, Mode, _same, cint, i64, ivals,
                         pyivx, cto, reads, sized, u32, u64, untouched)  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


# ------------------------------------------------------------------ 1. host mode equals device mode (the cases: entry_cases.py)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_mode_equals_device_mode(env, name, n):
    host = CASES[name](env, Mode(False), n)
    dev = CASES[name](env, Mode(True), n)
    dev = {k: (v.cpu().numpy().view(host[k].dtype) if pyivx._is_torch(v) else v) for k, v in dev.items()}
    assert sorted(host) == sorted(dev)
    assert all(host[k] == OK for k in ("st", "st0", "st1", "st2") if k in host), env.err()
    diff = [k for k in host if not _same(host[k], dev[k])]
    assert not diff, {k: (host[k], dev[k]) for k in diff[:3]}


# ------------------------------------------------------------------ 2. / 3. argument errors; outputs left alone

class Args:
    """good host-mode arguments of every entry (8 rows), output buffers filled with the pattern"""

    def __init__(self, E):
        H = Mode(False)
        self.E, self.n = E, 8
        n = self.n
        self.k, self.s, self.e = (H.put(a) for a in ivals(n, 30))
        self.k64, self.s64, self.e64 = (H.put(a) for a in ivals(n, 30, np.int64))
        r = reads(n, 31)
        self.r = {c: H.put(v) for c, v in r.items()}
        toff, ttext = cto.text_column(cto.render_reads(r["off"], r["ops"]))
        self.toff, self.ttext = H.put(toff), H.put(ttext)
        self.thr, self.qn = H.put(np.array([1, 2], np.int32)), H.put(np.array([1], np.uint32))
        self.idx = H.put(np.arange(n, dtype=np.uint32))
        self.src = H.put(np.arange(64, dtype=np.int64))
        self.bits = H.put(np.zeros(8, np.uint8))
        self.views = H.put(np.zeros(32 * 16, np.uint8))            # 32 empty strings
        self.val = H.put(np.arange(E.n_build, dtype=np.int64))     # overlap_agg, overlap_select: one value per build row
        self.w = pyivx.OverlapWhereC(10, 1, 2, 0, 0, 0)             # the *_where entries: min_bases 10, half of the probe row
        self.o = [H.out(64, np.int64) for _ in range(8)]       # outputs: enough bytes for any column of 8 rows
        self.count = u64(0)
        self.handle = C.c_void_p()
        import torch
        self.dev_out = torch.zeros(64, dtype=torch.int64, device="cuda:0")

    def good(self, entry):
        E, n, r, o = self.E, self.n, self.r, [b.p for b in self.o]
        cnt, H = C.byref(self.count), cint(pyivx.MEM_HOST)
        cols = (self.k.p, self.s.p, self.e.p, u64(n))
        cols64 = (self.k64.p, self.s64.p, self.e64.p, u64(n))
        dcols = (r["rkey"].p, r["rpos"].p, r["rflags"].p, r["rmapq"].p)
        dseg = (n, r["skey"].p, r["ss"].p, r["se"].p, r["sw"].p, n // 4, NK, None, 1796, 0)
        prof = E.profile.h
        regions = (r["rkey"].p, r["rpos"].p, r["rpos"].p, n, 0, None, 0)
        table = {
            "ivx_index_build": [cint(0), H, *cols, u32(NK), C.byref(self.handle)],
            "ivx_probe_overlap_count": [E.ix[0].h, H, *cols, o[0], cnt],
            "ivx_probe_overlap_fill": [E.ix[0].h, H, *cols, o[0], o[1], u64(64), cnt],
            "ivx_probe_exists": [E.ix[0].h, H, *cols, o[0]],
            "ivx_probe_mark_build": [E.ix[0].h, H, *cols, o[0]],
            "ivx_probe_overlap_agg": [E.ix[0].h, H, *cols, self.val.p, u32(8), *o[:6]],
            "ivx_probe_overlap_select": [E.ix[0].h, H, *cols, self.val.p, u32(8), cint(1), o[0], o[1]],
            "ivx_probe_overlap_count_where": [E.ix[0].h, H, *cols, C.byref(self.w), o[0], o[1], cnt],
            "ivx_probe_mark_build_where": [E.ix[0].h, H, *cols, C.byref(self.w), o[0]],
            "ivx_probe_overlap_agg_where": [E.ix[0].h, H, *cols, self.val.p, u32(8), C.byref(self.w), *o[:6]],
            "ivx_probe_overlap_select_where": [E.ix[0].h, H, *cols, self.val.p, u32(8), cint(1), C.byref(self.w), o[0], o[1]],
            "ivx_pairs_where": [H, self.idx.p, self.idx.p, u64(n), self.s.p, self.e.p, u64(n), self.s.p, self.e.p, u64(n), C.byref(self.w),
                                o[0], o[1], u64(64), cnt],
            "ivx_probe_nearest_dir": [E.ix[3].h, H, *cols, cint(0), u32(1), cint(1), cint(1), i64(10), o[0], o[1], o[2], u64(n), cnt],
            "ivx_bits_mark": [H, self.idx.p, u64(n), o[0], u64(64)],
            "ivx_bits_select": [H, self.bits.p, u64(64), cint(1), o[0], u64(64), cnt],
            "ivx_probe_count": [E.ix[1].h, H, *cols, cint(0), o[0]],
            "ivx_probe_coverage": [E.ix[2].h, H, *cols, cint(0), o[0]],
            "ivx_probe_nearest": [E.ix[3].h, H, *cols, cint(0), u32(1), cint(1), o[0], o[1], o[2], u64(n), cnt],
            "ivx_merge": [H, *cols64, u32(NK), i64(0), cint(0), o[0], o[1], o[2], o[3], u64(n), cnt],
            "ivx_subtract": [H, *cols64, *cols64, u32(NK), cint(0), o[0], o[1], o[2], o[3], u64(64), cnt],
            "ivx_intersect": [H, *cols64, *cols64, u32(NK), cint(0), o[0], o[1], o[2], o[3], u64(64), cnt],
            "ivx_cluster": [H, *cols64, u32(NK), i64(0), cint(0), None, *o[:7], o[7], cnt],
            "ivx_complement": [H, *cols64, None, None, None, u64(0), u32(NK), cint(0), o[0], o[1], o[2], u64(64), cnt],
            "ivx_depth": [H, *dcols, r["off"].p, r["ops"].p, *dseg, o[0], o[1], o[2], o[3], 64, cnt],
            "ivx_depth_text": [H, *dcols, 0, self.toff.p, self.ttext.p, *dseg, o[0], o[1], o[2], o[3], 64, cnt],
            "ivx_depth_profile_build": [H, *dcols, r["off"].p, r["ops"].p, *dseg, C.byref(self.handle)],
            "ivx_depth_profile_build_text": [H, *dcols, 0, self.toff.p, self.ttext.p, *dseg, C.byref(self.handle)],
            "ivx_cigar_parse": [H, 0, self.toff.p, self.ttext.p, n, o[0], o[1], 64, cnt],
            "ivx_depth_profile_read": [prof, H, None, None, None, o[3], 0, cnt],
            "ivx_depth_profile_expand": [prof, H, 0, 0, n, 0, o[0], o[1]],
            "ivx_depth_profile_merge": [prof, E.profile2.h, C.byref(self.handle)],
            "ivx_depth_profile_blocks": [prof, H, None, None, None, None, 0, cnt],
            "ivx_depth_profile_summarize": [prof, H, *regions, self.thr.p, 2, o[0], o[1], o[2]],
            "ivx_depth_profile_windows": [prof, H, 0, 0, 100, 10, n, 0, self.thr.p, 2, o[0], o[1], o[2]],
            "ivx_depth_profile_quantiles": [prof, H, *regions, self.qn.p, 1, 2, o[0], o[1], o[2], o[3]],
            "ivx_depth_profile_window_quantiles": [prof, H, 0, 0, 100, 10, n, 0, self.qn.p, 1, 2, o[0], o[1], o[2], o[3]],
            "ivx_depth_profile_quantize": [prof, H, 0, None, 0, 0, self.thr.p, 2, 7, None, None, None, None, 0, cnt],
            "ivx_depth_profile_hist": [prof, H, 0, None, 0, 0, 0, 4, o[0]],
            "ivx_take_fixed": [H, self.src.p, u32(8), u64(64), None, self.idx.p, u64(n), o[0], o[1]],
            "ivx_scatter_fixed": [H, self.src.p, u32(8), self.idx.p, u64(n), o[0], u64(64)],
            "ivx_take_utf8": [H, cint(0), self.toff.p, self.ttext.p, u64(n), u64(len(self.ttext.np())), None, self.idx.p, u64(n), o[0], o[1], u64(512), cnt, o[2]],
            "ivx_take_bits": [H, self.bits.p, u64(64), None, self.idx.p, u64(n), o[0], o[1]],
            "ivx_take_view": [H, self.views.p, None, None, u32(0), u64(32), None, self.idx.p, u64(n), o[0], o[1], u64(64), cnt, o[2]],
        }
        return table[entry]


MEM2 = cint(2)
DEVICE = cint(pyivx.MEM_DEVICE)
ODD = "odd"                 # stands for a device pointer that is off its element size by one byte
BAD_MEM = (INVALID, "bad mem")
ALIGN = (INVALID, "depth profile: output pointer not aligned to its element size")
ALIGN_ANY = (INVALID, "depth profile: pointer not aligned to its element size")      # quantize and hist check key_hi as well
DESCENDING = np.array([3, 1], np.int32)                                                # cuts are host memory in both modes
NEGATIVE_W = pyivx.OverlapWhereC(-1, 0, 0, 0, 0, 0)                                    # thresholds (host structs in both modes) that break a rule
ABOVE_ONE_W = pyivx.OverlapWhereC(0, 3, 2, 0, 0, 0)

# (entry, {argument position after ctx: bad value}) -> (status, ivx_last_error), the texts as csrc/ivx_capi.hip has them
ERRORS = [
    # mem = 2
    ("ivx_index_build", {1: MEM2}, BAD_MEM), ("ivx_probe_overlap_count", {1: MEM2}, BAD_MEM), ("ivx_probe_overlap_fill", {1: MEM2}, BAD_MEM),
    ("ivx_probe_exists", {1: MEM2}, BAD_MEM), ("ivx_probe_mark_build", {1: MEM2}, BAD_MEM), ("ivx_bits_mark", {0: MEM2}, BAD_MEM),
    ("ivx_bits_select", {0: MEM2}, BAD_MEM), ("ivx_probe_count", {1: MEM2}, BAD_MEM), ("ivx_probe_coverage", {1: MEM2}, BAD_MEM),
    ("ivx_probe_nearest", {1: MEM2}, BAD_MEM), ("ivx_merge", {0: MEM2}, BAD_MEM), ("ivx_subtract", {0: MEM2}, BAD_MEM),
    ("ivx_cluster", {0: MEM2}, BAD_MEM), ("ivx_complement", {0: MEM2}, BAD_MEM), ("ivx_depth", {0: 2}, BAD_MEM), ("ivx_depth_text", {0: 2}, BAD_MEM),
    ("ivx_depth_profile_build", {0: 2}, BAD_MEM), ("ivx_depth_profile_build_text", {0: 2}, BAD_MEM), ("ivx_cigar_parse", {0: 2}, BAD_MEM),
    ("ivx_depth_profile_read", {1: 2}, BAD_MEM), ("ivx_depth_profile_expand", {1: 2}, BAD_MEM), ("ivx_depth_profile_blocks", {1: 2}, BAD_MEM),
    ("ivx_depth_profile_summarize", {1: 2}, BAD_MEM), ("ivx_depth_profile_windows", {1: 2}, BAD_MEM),
    ("ivx_depth_profile_quantiles", {1: 2}, BAD_MEM), ("ivx_depth_profile_window_quantiles", {1: 2}, BAD_MEM),
    ("ivx_take_fixed", {0: MEM2}, BAD_MEM), ("ivx_scatter_fixed", {0: MEM2}, BAD_MEM), ("ivx_take_utf8", {0: MEM2}, BAD_MEM),
    ("ivx_take_bits", {0: MEM2}, BAD_MEM), ("ivx_take_view", {0: MEM2}, BAD_MEM),
    ("ivx_probe_overlap_agg", {1: MEM2}, BAD_MEM), ("ivx_intersect", {0: MEM2}, BAD_MEM),
    ("ivx_depth_profile_quantize", {1: 2}, BAD_MEM), ("ivx_depth_profile_hist", {1: 2}, BAD_MEM),
    # a null required column with n > 0
    ("ivx_index_build", {3: None}, (INVALID, "null coordinate column")),
    ("ivx_probe_overlap_count", {4: None}, (INVALID, "null coordinate column")),
    ("ivx_probe_overlap_fill", {6: None}, (INVALID, "null pair buffers")),
    ("ivx_probe_exists", {6: None}, (INVALID, "null exists buffer")),
    ("ivx_probe_mark_build", {6: None}, (INVALID, "null mark bitmap")),
    ("ivx_bits_mark", {1: None}, (INVALID, "bits_mark: null idx")),
    ("ivx_bits_mark", {3: None}, (INVALID, "bits_mark: null bitmap")),
    ("ivx_bits_select", {1: None}, (INVALID, "bits_select: null bitmap")),
    ("ivx_bits_select", {4: None}, (INVALID, "bits_select: null out")),
    ("ivx_probe_count", {7: None}, (INVALID, "null output column")),
    ("ivx_probe_coverage", {3: None}, (INVALID, "null coordinate column")),
    ("ivx_probe_nearest", {9: None}, (INVALID, "null output column")),
    ("ivx_merge", {2: None}, (INVALID, "null coordinate column")),
    ("ivx_subtract", {7: None}, (INVALID, "null coordinate column")),
    ("ivx_cluster", {3: None}, (INVALID, "null coordinate column")),
    ("ivx_complement", {2: None}, (INVALID, "null coordinate column")),
    ("ivx_depth", {2: None}, (INVALID, "depth: null read position or CIGAR offset column")),
    ("ivx_depth", {9: None}, (INVALID, "depth: null segment coordinate column")),
    ("ivx_depth_text", {6: None}, (INVALID, "depth: null read position or CIGAR offset column")),
    ("ivx_depth_profile_build", {5: None}, (INVALID, "depth: null read position or CIGAR offset column")),
    ("ivx_depth_profile_build_text", {10: None}, (INVALID, "depth: null segment coordinate column")),
    ("ivx_cigar_parse", {2: None}, (INVALID, "cigar: null text offset column")),
    ("ivx_depth_profile_summarize", {3: None}, (INVALID, "null coordinate column")),
    ("ivx_depth_profile_summarize", {9: None}, (INVALID, "depth profile: null thresholds")),
    ("ivx_depth_profile_quantiles", {4: None}, (INVALID, "null coordinate column")),
    ("ivx_depth_profile_window_quantiles", {8: None}, (INVALID, "depth profile: null q_num")),
    ("ivx_take_fixed", {5: None}, (INVALID, "take: null idx or out")),
    ("ivx_take_fixed", {1: None}, (INVALID, "take: null source column")),
    ("ivx_scatter_fixed", {1: None}, (INVALID, "scatter: null src, idx or out")),
    ("ivx_take_utf8", {7: None}, (INVALID, "take: null idx")),
    ("ivx_take_utf8", {2: None}, (INVALID, "take: null source column")),
    ("ivx_take_bits", {6: None}, (INVALID, "take: null idx or out")),
    ("ivx_take_view", {1: None}, (INVALID, "take: null source column")),
    ("ivx_probe_overlap_agg", {4: None}, (INVALID, "null coordinate column")),
    ("ivx_probe_overlap_agg", {6: None}, (INVALID, "overlap_agg: null value column")),
    ("ivx_probe_overlap_agg", {8: None, 9: None, 10: None, 11: None, 12: None, 13: None}, (INVALID, "overlap_agg: no output wanted")),
    ("ivx_intersect", {7: None}, (INVALID, "null coordinate column")),
    ("ivx_intersect", {5: None}, (INVALID, "intersect: key given for one side only")),
    ("ivx_depth_profile_merge", {0: None}, (INVALID, "null depth profile")),
    ("ivx_depth_profile_merge", {1: None}, (INVALID, "null depth profile")),
    ("ivx_depth_profile_quantize", {6: None}, (INVALID, "depth profile: null cuts")),
    ("ivx_depth_profile_hist", {8: None}, (INVALID, "depth profile: null out_hist")),
    # a null n_out (or the entry's word for it)
    ("ivx_index_build", {7: None}, (INVALID, "null out")), ("ivx_bits_select", {6: None}, (INVALID, "null n_out")),
    ("ivx_probe_nearest", {13: None}, (INVALID, "null rows")), ("ivx_merge", {13: None}, (INVALID, "null n_out")),
    ("ivx_subtract", {16: None}, (INVALID, "null n_out")), ("ivx_cluster", {17: None}, (INVALID, "null n_clusters")),
    ("ivx_complement", {15: None}, (INVALID, "null n_out")), ("ivx_depth", {22: None}, (INVALID, "null n_out")),
    ("ivx_depth_text", {23: None}, (INVALID, "null n_out")), ("ivx_depth_profile_build", {17: None}, (INVALID, "null out")),
    ("ivx_depth_profile_build_text", {18: None}, (INVALID, "null out")), ("ivx_cigar_parse", {8: None}, (INVALID, "null n_ops")),
    ("ivx_depth_profile_read", {7: None}, (INVALID, "null n_out")), ("ivx_depth_profile_blocks", {7: None}, (INVALID, "null n_out")),
    ("ivx_take_utf8", {12: None}, (INVALID, "null data_bytes")), ("ivx_take_view", {12: None}, (INVALID, "null data_bytes")),
    ("ivx_intersect", {16: None}, (INVALID, "null n_out")), ("ivx_depth_profile_merge", {2: None}, (INVALID, "null out")),
    ("ivx_depth_profile_quantize", {14: None}, (INVALID, "null n_out")),
    # a misaligned device output pointer
    ("ivx_depth_profile_expand", {1: DEVICE, 6: ODD}, ALIGN), ("ivx_depth_profile_expand", {1: DEVICE, 7: ODD}, ALIGN),
    ("ivx_depth_profile_summarize", {1: DEVICE, 12: ODD}, ALIGN), ("ivx_depth_profile_windows", {1: DEVICE, 11: ODD}, ALIGN),
    ("ivx_depth_profile_quantiles", {1: DEVICE, 13: ODD}, ALIGN), ("ivx_depth_profile_window_quantiles", {1: DEVICE, 14: ODD}, ALIGN),
    ("ivx_depth_profile_quantize", {1: DEVICE, 9: ODD}, ALIGN_ANY), ("ivx_depth_profile_quantize", {1: DEVICE, 12: ODD}, ALIGN_ANY),
    ("ivx_depth_profile_hist", {1: DEVICE, 8: ODD}, ALIGN_ANY), ("ivx_depth_profile_hist", {1: DEVICE, 3: ODD}, ALIGN_ANY),
    # val_bytes = 3, 32 cuts, descending cuts, an emit bit above the last class, n_bins = 0
    ("ivx_probe_overlap_agg", {7: u32(3)}, (INVALID, "overlap_agg: val_bytes is 4 or 8")),
    ("ivx_depth_profile_quantize", {7: 32}, (INVALID, "depth profile: more than 31 cuts")),
    ("ivx_depth_profile_quantize", {6: pyivx._ptr(DESCENDING)}, (INVALID, "depth profile: cuts not strictly ascending")),
    ("ivx_depth_profile_quantize", {8: 8}, (INVALID, "depth profile: emit_mask names a class above n_cuts")),
    ("ivx_depth_profile_hist", {7: 0}, (INVALID, "depth profile: n_bins outside 1 .. 65536")),
    # width = 0, n_thr = 9, q_den = 0
    ("ivx_depth_profile_windows", {5: 0}, (INVALID, "depth profile: window width 0")),
    ("ivx_depth_profile_window_quantiles", {5: 0}, (INVALID, "depth profile: window width 0")),
    ("ivx_depth_profile_summarize", {10: 9}, (INVALID, "depth profile: more than 8 thresholds")),
    ("ivx_depth_profile_windows", {9: 9}, (INVALID, "depth profile: more than 8 thresholds")),
    ("ivx_depth_profile_quantiles", {11: 0}, (INVALID, "depth profile: q_den outside 1 .. 65536")),
    ("ivx_depth_profile_window_quantiles", {10: 0}, (INVALID, "depth profile: q_den outside 1 .. 65536")),
    # two bad arguments at once: which message wins
    ("ivx_merge", {0: MEM2, 13: None}, (INVALID, "null n_out")),
    ("ivx_depth_profile_windows", {1: 2, 5: 0}, BAD_MEM),
    ("ivx_depth_profile_summarize", {1: DEVICE, 10: 9, 12: ODD}, (INVALID, "depth profile: more than 8 thresholds")),
    ("ivx_take_fixed", {0: MEM2, 2: u32(3)}, BAD_MEM),
    ("ivx_probe_overlap_agg", {1: MEM2, 7: u32(3)}, BAD_MEM),
    ("ivx_depth_profile_quantize", {1: 2, 7: 32}, BAD_MEM),
    ("ivx_depth_profile_hist", {1: DEVICE, 7: 0, 8: ODD}, (INVALID, "depth profile: n_bins outside 1 .. 65536")),
    # ---- the entries of the companion headers (include/ivx_select.h, ivx_where.h, ivx_nearest.h)
    # mem = 2
    ("ivx_probe_overlap_select", {1: MEM2}, BAD_MEM), ("ivx_probe_overlap_count_where", {1: MEM2}, BAD_MEM),
    ("ivx_probe_mark_build_where", {1: MEM2}, BAD_MEM), ("ivx_probe_overlap_agg_where", {1: MEM2}, BAD_MEM),
    ("ivx_probe_overlap_select_where", {1: MEM2}, BAD_MEM), ("ivx_pairs_where", {0: MEM2}, BAD_MEM), ("ivx_probe_nearest_dir", {1: MEM2}, BAD_MEM),
    # a null required column
    ("ivx_probe_overlap_select", {3: None}, (INVALID, "null coordinate column")),
    ("ivx_probe_overlap_select", {9: None}, (INVALID, "overlap_select: null build_idx")),
    ("ivx_probe_overlap_select", {6: None}, (INVALID, "overlap_select: null value column")),
    ("ivx_probe_overlap_count_where", {4: None}, (INVALID, "null coordinate column")),
    ("ivx_probe_mark_build_where", {7: None}, (INVALID, "null mark bitmap")),
    ("ivx_probe_overlap_agg_where", {6: None}, (INVALID, "overlap_agg: null value column")),
    ("ivx_probe_overlap_select_where", {10: None}, (INVALID, "overlap_select: null build_idx")),
    ("ivx_pairs_where", {1: None}, (INVALID, "pairs_where: null pair columns")),
    ("ivx_pairs_where", {8: None}, (INVALID, "pairs_where: null coordinate column")),
    ("ivx_pairs_where", {11: None}, (INVALID, "pairs_where: null output columns")),
    ("ivx_probe_nearest_dir", {3: None}, (INVALID, "null coordinate column")),
    ("ivx_probe_nearest_dir", {11: None}, (INVALID, "null output column")),
    # the null count word
    ("ivx_pairs_where", {14: None}, (INVALID, "pairs_where: null n_out")), ("ivx_probe_nearest_dir", {15: None}, (INVALID, "null rows")),
    # no output wanted; val_bytes = 3, an unknown criterion; a direction of 3; a threshold that breaks a rule
    ("ivx_probe_overlap_count_where", {7: None, 8: None, 9: None}, (INVALID, "overlap_count_where: no output wanted")),
    ("ivx_probe_overlap_agg_where", {9: None, 10: None, 11: None, 12: None, 13: None, 14: None}, (INVALID, "overlap_agg: no output wanted")),
    ("ivx_probe_overlap_select", {7: u32(3)}, (INVALID, "overlap_select: val_bytes is 4 or 8")),
    ("ivx_probe_overlap_select", {8: cint(6)}, (INVALID, "overlap_select: unknown criterion")),
    ("ivx_probe_overlap_select_where", {8: cint(-1)}, (INVALID, "overlap_select: unknown criterion")),
    ("ivx_probe_nearest_dir", {9: cint(3)}, (INVALID, "nearest: direction must be IVX_NEAR_ANY, IVX_NEAR_BEFORE or IVX_NEAR_AFTER")),
    ("ivx_probe_nearest_dir", {9: cint(3), 10: i64(-1)}, (INVALID, "nearest: direction must be IVX_NEAR_ANY, IVX_NEAR_BEFORE or IVX_NEAR_AFTER")),
    ("ivx_probe_mark_build_where", {6: C.byref(NEGATIVE_W)}, (INVALID, "overlap_where: min_bases is negative")),
    ("ivx_pairs_where", {10: C.byref(ABOVE_ONE_W)}, (INVALID, "overlap_where: a fraction is above 1 (num > den)")),
    # two bad arguments at once: which message wins
    ("ivx_probe_overlap_agg_where", {1: MEM2, 7: u32(3)}, BAD_MEM),
    ("ivx_probe_overlap_count_where", {6: C.byref(NEGATIVE_W), 7: None, 8: None, 9: None}, (INVALID, "overlap_where: min_bases is negative")),
    ("ivx_probe_overlap_select_where", {7: u32(3), 9: C.byref(NEGATIVE_W)}, (INVALID, "overlap_where: min_bases is negative")),
    ("ivx_pairs_where", {0: MEM2, 14: None}, (INVALID, "pairs_where: null n_out")),
    ("ivx_probe_nearest_dir", {1: MEM2, 9: cint(3)}, BAD_MEM),
]


@pytest.fixture(scope="module")
def args(env):
    return Args(env)


@pytest.mark.parametrize("entry,bad,want", ERRORS, ids=[f"{e[4:]}-{'-'.join(map(str, b))}" for e, b, _ in ERRORS])
def test_argument_error(env, args, entry, bad, want):
    a = args.good(entry)
    for pos, v in bad.items():
        a[pos] = C.c_void_p(args.dev_out.data_ptr() + 1) if v is ODD else v
    st = getattr(env.L, entry)(env.h, *a)
    assert (st, env.err()) == want
    # the call stopped at its argument check: no output buffer of the caller was written
    assert all(untouched(o) for o in args.o)
    assert args.handle.value is None


def test_good_arguments_pass(env, args):
    """the table's good arguments are good: every error above comes from the one argument it names"""
    for entry in sorted({e for e, _, _ in ERRORS}):
        H = Mode(False)
        args.o = [H.out(64, np.int64) for _ in range(8)]
        st = getattr(env.L, entry)(env.h, *args.good(entry))
        assert st == OK, (entry, st, env.err())
        if args.handle.value:
            (env.L.ivx_depth_profile_free if "profile" in entry else env.L.ivx_index_free)(args.handle)
            args.handle.value = None
    args.o = [H.out(64, np.int64) for _ in range(8)]
