//! FFI declarations of overlap select -- the one best build row per probe row -- at both levels: the C entry of
//! `include/ivx_select.h` (libivx_hip.so) and the Arrow-level operator `brh_overlap_select` of `include/bio_ranges_host.h`
//! (libbio_ranges_hip.so).  They live beside `hip_ffi.rs` / `join_stream_ffi.rs` until the entry is folded into `ivx.h`;
//! the opaque types are those two files' own.  `tests/test_select_abi.py` holds every declaration against its header.
use std::ffi::{c_char, c_int, c_void};

use arrow::ffi::{FFI_ArrowArray, FFI_ArrowSchema};

use crate::hip_ffi::{IvxCtx, IvxIndex};
use crate::join_stream_ffi::{BrhBatch, BrhColumns, BrhSession};

/// `by` of both entries (the IVX_SEL_* / BRH_SEL_* enums): the criterion the winner is smallest or largest in; ties go to
/// the smallest build row.
#[repr(i32)] #[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum SelectBy { MinVal = 0, MaxVal = 1, MaxOverlap = 2, MinOverlap = 3, FirstRow = 4, LastRow = 5 }

/// `build_idx` of a probe row without a match (IVX_NULL_IDX)
pub const NULL_IDX: u32 = 0xFFFF_FFFF;

#[link(name = "ivx_hip")]
extern "C" {
    pub fn ivx_probe_overlap_select(ctx: *mut IvxCtx, ix: *const IvxIndex, mem: i32, key: *const u32, start: *const i32,
                                    end: *const i32, n: u64, val: *const c_void, val_bytes: u32, by: i32,
                                    build_idx: *mut u32, score: *mut i64) -> i32;
}

#[link(name = "bio_ranges_hip")]
extern "C" {
    pub fn brh_overlap_select(s: *mut BrhSession, build: BrhBatch, bcols: BrhColumns, value_column: *const c_char,
                              probe: BrhBatch, pcols: BrhColumns, strict_predicate: c_int, by: c_int,
                              build_idx: *mut FFI_ArrowArray, build_idx_schema: *mut FFI_ArrowSchema,
                              score: *mut FFI_ArrowArray, score_schema: *mut FFI_ArrowSchema) -> c_int;
}
