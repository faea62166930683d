//! FFI declarations of the overlap thresholds -- a minimum of shared bases and minimum overlap fractions on every per-row
//! probe, and the stable pair filter -- at both levels: the C entries of `include/ivx_where.h` (libivx_hip.so) and the
//! Arrow-level operators `brh_*_where` of `include/bio_ranges_host.h` (libbio_ranges_hip.so).  They live beside `hip_ffi.rs`,
//! `join_stream_ffi.rs` and `select_ffi.rs` until the entries are folded into `ivx.h`; the opaque types are those files' own.
//! `tests/test_where_abi.py` holds every declaration, and the struct's field order and types, against the headers.
use std::ffi::{c_char, c_int, c_void};

use arrow::ffi::{FFI_ArrowArray, FFI_ArrowSchema};

use crate::hip_ffi::{IvxCtx, IvxIndex};
use crate::join_stream_ffi::{BrhBatch, BrhColumns, BrhSession};

/// `ivx_overlap_where`: a matched pair passes iff its closed overlap length `len` is at least `max(1, min_bases)`,
/// `len * probe_den >= plen * probe_num` and `len * build_den >= blen * build_num` in exact integers (a fraction with
/// `num == 0` is not asked; `either == 1`: one of two asked fractions suffices).  All zero asks nothing.
#[repr(C)] #[derive(Clone, Copy, Default, PartialEq, Eq, Debug)]
pub struct IvxOverlapWhere {
    pub min_bases: i64,
    pub probe_num: u32,
    pub probe_den: u32,
    pub build_num: u32,
    pub build_den: u32,
    pub either: u32,
}

/// `brh_overlap_where`: the same fields in the same order.
pub type BrhOverlapWhere = IvxOverlapWhere;

#[link(name = "ivx_hip")]
extern "C" {
    pub fn ivx_probe_overlap_count_where(ctx: *mut IvxCtx, ix: *const IvxIndex, mem: i32, key: *const u32, start: *const i32,
                                         end: *const i32, n: u64, w: *const IvxOverlapWhere,
                                         per_row: *mut u32, exists: *mut u8, total: *mut u64) -> i32;
    pub fn ivx_probe_mark_build_where(ctx: *mut IvxCtx, ix: *const IvxIndex, mem: i32, key: *const u32, start: *const i32,
                                      end: *const i32, n: u64, w: *const IvxOverlapWhere, marks: *mut u32) -> i32;
    pub fn ivx_probe_overlap_agg_where(ctx: *mut IvxCtx, ix: *const IvxIndex, mem: i32, key: *const u32, start: *const i32,
                                       end: *const i32, n: u64, val: *const c_void, val_bytes: u32, w: *const IvxOverlapWhere,
                                       count: *mut u32, sum: *mut i64, vmin: *mut i64, vmax: *mut i64,
                                       bases: *mut i64, wsum: *mut i64) -> i32;
    pub fn ivx_probe_overlap_select_where(ctx: *mut IvxCtx, ix: *const IvxIndex, mem: i32, key: *const u32, start: *const i32,
                                          end: *const i32, n: u64, val: *const c_void, val_bytes: u32, by: i32,
                                          w: *const IvxOverlapWhere, build_idx: *mut u32, score: *mut i64) -> i32;
    pub fn ivx_pairs_where(ctx: *mut IvxCtx, mem: i32, build_idx: *const u32, probe_idx: *const u32, n_pairs: u64,
                           bstart: *const i32, bend: *const i32, nb: u64, pstart: *const i32, pend: *const i32, np: u64,
                           w: *const IvxOverlapWhere, out_build: *mut u32, out_probe: *mut u32, cap: u64,
                           n_out: *mut u64) -> i32;
}

#[link(name = "bio_ranges_hip")]
extern "C" {
    pub fn brh_interval_join_where(s: *mut BrhSession, build: BrhBatch, bcols: BrhColumns, probe: BrhBatch, pcols: BrhColumns,
                                   join_type: c_int, strict_predicate: c_int, nearest_algorithm: c_int,
                                   where_: *const BrhOverlapWhere,
                                   build_idx: *mut FFI_ArrowArray, build_idx_schema: *mut FFI_ArrowSchema,
                                   probe_idx: *mut FFI_ArrowArray, probe_idx_schema: *mut FFI_ArrowSchema) -> c_int;
    pub fn brh_overlap_aggregate_where(s: *mut BrhSession, build: BrhBatch, bcols: BrhColumns, value_column: *const c_char,
                                       probe: BrhBatch, pcols: BrhColumns, strict_predicate: c_int, ops: u32,
                                       where_: *const BrhOverlapWhere,
                                       out: *mut FFI_ArrowArray, out_schema: *mut FFI_ArrowSchema) -> c_int;
    pub fn brh_overlap_select_where(s: *mut BrhSession, build: BrhBatch, bcols: BrhColumns, value_column: *const c_char,
                                    probe: BrhBatch, pcols: BrhColumns, strict_predicate: c_int, by: c_int,
                                    where_: *const BrhOverlapWhere,
                                    build_idx: *mut FFI_ArrowArray, build_idx_schema: *mut FFI_ArrowSchema,
                                    score: *mut FFI_ArrowArray, score_schema: *mut FFI_ArrowSchema) -> c_int;
}
