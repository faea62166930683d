//! FFI declarations of nearest on one side only and / or within a distance cap, at both levels: the C entry of
//! `include/ivx_nearest.h` (libivx_hip.so) and the Arrow-level operator `brh_nearest_dir` of `include/bio_ranges_host.h`
//! (libbio_ranges_hip.so).  They live beside `hip_ffi.rs` / `join_stream_ffi.rs` until the entry is folded into `ivx.h`;
//! the opaque types are those two files' own.  `tests/test_nearest_dir_abi.py` holds every declaration against its header.
use std::ffi::c_int;

use arrow::ffi::{FFI_ArrowArray, FFI_ArrowSchema};

use crate::hip_ffi::{IvxCtx, IvxIndex};
use crate::join_stream_ffi::{BrhBatch, BrhColumns, BrhSession};

/// `direction` of both entries (the IVX_NEAR_* / BRH_NEAR_* enums): which cursor(s) of the reference's nearest_k feed the
/// answer.  Before = build rows that end before the probe row ("upstream"), After = build rows that start after it
/// ("downstream").  Overlapping rows are not touched by it: `include_overlaps` alone decides them.
#[repr(i32)] #[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum NearDirection { Any = 0, Before = 1, After = 2 }

/// `max_distance` of both entries when there is no cap (any negative value)
pub const NO_MAX_DISTANCE: i64 = -1;

#[link(name = "ivx_hip")]
extern "C" {
    pub fn ivx_probe_nearest_dir(ctx: *mut IvxCtx, ix: *const IvxIndex, mem: i32, key: *const u32, start: *const i32,
                                 end: *const i32, n: u64, strict: i32, k: u32, include_overlaps: i32,
                                 direction: i32, max_distance: i64,
                                 build_idx: *mut u32, probe_idx: *mut u32, distance: *mut i64, cap: u64, rows: *mut u64) -> i32;
}

#[link(name = "bio_ranges_hip")]
extern "C" {
    pub fn brh_nearest_dir(s: *mut BrhSession, left: BrhBatch, lcols: BrhColumns, right: BrhBatch, rcols: BrhColumns,
                           filter_op: c_int, k: u32, include_overlaps: c_int, compute_distance: c_int,
                           direction: c_int, max_distance: i64,
                           left_idx: *mut FFI_ArrowArray, left_idx_schema: *mut FFI_ArrowSchema,
                           right_idx: *mut FFI_ArrowArray, right_idx_schema: *mut FFI_ArrowSchema,
                           distance: *mut FFI_ArrowArray, distance_schema: *mut FFI_ArrowSchema) -> c_int;
}
