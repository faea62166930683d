//! Rust side of the push-style join stream of `include/bio_ranges_host.h` (`brh_join_stream_*`), the piece of
//! `IntervalJoinStream` (interval_join.rs:934-1140) that coalesces probe RecordBatches before they go to the GPU.
//!
//! NOT compiled in this repository (no Rust toolchain in the build image).  The declarations mirror the header one
//! to one (`tests/test_abi.py` checks names and parameter counts); `poll_next_impl` below shows how the reference's
//! state machine maps onto them.  Arrays cross as Arrow C Data Interface structs (`arrow::ffi`).
#![allow(dead_code)]

use std::ffi::{c_char, c_int, CStr};

use arrow::array::{ArrayRef, Int64Array, RecordBatch, StructArray, UInt32Array};
use arrow::compute::concat_batches;
use arrow::ffi::{from_ffi, to_ffi, FFI_ArrowArray, FFI_ArrowSchema};
use datafusion::common::{DataFusionError, Result};

#[repr(C)] pub struct BrhSession { _p: [u8; 0] }
#[repr(C)] pub struct BrhJoinStream { _p: [u8; 0] }
#[repr(C)] pub struct BrhDepthStream { _p: [u8; 0] }
#[repr(C)] pub struct BrhDepthPush { _p: [u8; 0] }
#[repr(C)] pub struct BrhBatch { pub array: *const FFI_ArrowArray, pub schema: *const FFI_ArrowSchema }
#[repr(C)] pub struct BrhColumns { pub keys: *const *const c_char, pub n_keys: c_int, pub start: *const c_char, pub end: *const c_char }

/// `join_type` of `brh_join_stream_open` (the BRH_JOIN_* enum of the header).  From LEFT_SEMI on: SQL semantics over the
/// build side's match marks -- LeftSemi / LeftAnti groups give no result, and `finish` ends with one result of
/// `n_batches == 0` that carries the build-side rows (probe_idx all NULL, or empty for LeftSemi / LeftAnti): take the
/// build columns with build_idx and extend the probe columns with NULLs, there is no probe batch to concatenate.
pub const BRH_JOIN_INNER: c_int = 0;
pub const BRH_JOIN_RIGHT_SEMI: c_int = 1;
pub const BRH_JOIN_RIGHT_ANTI: c_int = 2;
pub const BRH_JOIN_NEAREST: c_int = 3;
pub const BRH_JOIN_LEFT_SEMI: c_int = 4;
pub const BRH_JOIN_LEFT_ANTI: c_int = 5;
pub const BRH_JOIN_LEFT: c_int = 6;
pub const BRH_JOIN_RIGHT: c_int = 7;
pub const BRH_JOIN_FULL: c_int = 8;

#[link(name = "bio_ranges_hip")]
extern "C" {
    pub fn brh_session_create(device_ordinal: c_int, out: *mut *mut BrhSession) -> c_int;
    pub fn brh_session_free(s: *mut BrhSession);
    pub fn brh_last_error(s: *const BrhSession) -> *const c_char;
    pub fn brh_join_stream_open(s: *mut BrhSession, build: BrhBatch, bcols: BrhColumns, pcols: BrhColumns, strict_predicate: c_int,
                                coalesce_rows: u64, join_type: c_int, max_output_rows: u64, out: *mut *mut BrhJoinStream) -> c_int;
    pub fn brh_join_stream_push(js: *mut BrhJoinStream, probe: BrhBatch, n_ready: *mut c_int) -> c_int;
    pub fn brh_join_stream_finish(js: *mut BrhJoinStream, n_ready: *mut c_int) -> c_int;
    pub fn brh_join_stream_next(js: *mut BrhJoinStream, first_batch: *mut u64, n_batches: *mut u64, group_done: *mut c_int,
                                build_idx: *mut FFI_ArrowArray, build_idx_schema: *mut FFI_ArrowSchema,
                                probe_idx: *mut FFI_ArrowArray, probe_idx_schema: *mut FFI_ArrowSchema,
                                batch_offsets: *mut FFI_ArrowArray, batch_offsets_schema: *mut FFI_ArrowSchema) -> c_int;
    pub fn brh_join_stream_close(js: *mut BrhJoinStream);
    // depth(path, zero_based, per_base = true): PerBaseEmitter as a pull stream over one depth profile kept on the device
    pub fn brh_depth_per_base_open(s: *mut BrhSession, reads: BrhBatch, prior: BrhBatch, lengths: BrhBatch, zero_based: c_int,
                                   filter_flag: u32, min_mapq: u32, out: *mut *mut BrhDepthStream) -> c_int;
    pub fn brh_depth_per_base_next(ds: *mut BrhDepthStream, max_rows: u64, done: *mut c_int,
                                   contig: *mut FFI_ArrowArray, contig_schema: *mut FFI_ArrowSchema,
                                   pos: *mut FFI_ArrowArray, pos_schema: *mut FFI_ArrowSchema,
                                   coverage: *mut FFI_ArrowArray, coverage_schema: *mut FFI_ArrowSchema) -> c_int;
    pub fn brh_depth_per_base_close(ds: *mut BrhDepthStream);
    // depth() over a stream of read batches: accumulate_partition as a push interface; finish = merge_*_results + the blocks,
    // finish_per_base hands the merged profile to the pull stream above
    pub fn brh_depth_push_open(s: *mut BrhSession, lengths: BrhBatch, filter_flag: u32, min_mapq: u32, out: *mut *mut BrhDepthPush) -> c_int;
    pub fn brh_depth_push_batch(dp: *mut BrhDepthPush, reads: BrhBatch) -> c_int;
    pub fn brh_depth_push_finish(dp: *mut BrhDepthPush,
                                 contig: *mut FFI_ArrowArray, contig_schema: *mut FFI_ArrowSchema,
                                 pos_start: *mut FFI_ArrowArray, pos_start_schema: *mut FFI_ArrowSchema,
                                 pos_end: *mut FFI_ArrowArray, pos_end_schema: *mut FFI_ArrowSchema,
                                 coverage: *mut FFI_ArrowArray, coverage_schema: *mut FFI_ArrowSchema) -> c_int;
    pub fn brh_depth_push_finish_per_base(dp: *mut BrhDepthPush, zero_based: c_int, out: *mut *mut BrhDepthStream) -> c_int;
    pub fn brh_depth_push_close(dp: *mut BrhDepthPush);
    // depth region summaries: bases, coverage sum and bases at or above each threshold per row of a regions table (all Int64);
    // ge / ge_schemas point at n_thr structs.  The push form leaves the stream open.
    pub fn brh_depth_regions(s: *mut BrhSession, reads: BrhBatch, prior: BrhBatch, lengths: BrhBatch, regions: BrhBatch, region_cols: BrhColumns,
                             zero_based: c_int, end_exclusive: c_int, filter_flag: u32, min_mapq: u32,
                             thresholds: *const i32, n_thr: u32,
                             bases: *mut FFI_ArrowArray, bases_schema: *mut FFI_ArrowSchema,
                             sum: *mut FFI_ArrowArray, sum_schema: *mut FFI_ArrowSchema,
                             ge: *mut FFI_ArrowArray, ge_schemas: *mut FFI_ArrowSchema) -> c_int;
    pub fn brh_depth_push_regions(dp: *mut BrhDepthPush, regions: BrhBatch, region_cols: BrhColumns, zero_based: c_int, end_exclusive: c_int,
                                  thresholds: *const i32, n_thr: u32,
                                  bases: *mut FFI_ArrowArray, bases_schema: *mut FFI_ArrowSchema,
                                  sum: *mut FFI_ArrowArray, sum_schema: *mut FFI_ArrowSchema,
                                  ge: *mut FFI_ArrowArray, ge_schemas: *mut FFI_ArrowSchema) -> c_int;
    // depth region order statistics: bases (Int64) and min, max and n_q quantiles (Int32, NULL where bases = 0) per row of a
    // regions table; quantile j = element floor((bases - 1) * q_num[j] / q_den) of the sorted per-base values; q / q_schemas point
    // at n_q structs.  The push form leaves the stream open.
    pub fn brh_depth_region_quantiles(s: *mut BrhSession, reads: BrhBatch, prior: BrhBatch, lengths: BrhBatch, regions: BrhBatch,
                                      region_cols: BrhColumns, zero_based: c_int, end_exclusive: c_int, filter_flag: u32, min_mapq: u32,
                                      q_num: *const u32, n_q: u32, q_den: u32,
                                      bases: *mut FFI_ArrowArray, bases_schema: *mut FFI_ArrowSchema,
                                      min: *mut FFI_ArrowArray, min_schema: *mut FFI_ArrowSchema,
                                      max: *mut FFI_ArrowArray, max_schema: *mut FFI_ArrowSchema,
                                      q: *mut FFI_ArrowArray, q_schemas: *mut FFI_ArrowSchema) -> c_int;
    pub fn brh_depth_push_region_quantiles(dp: *mut BrhDepthPush, regions: BrhBatch, region_cols: BrhColumns, zero_based: c_int,
                                           end_exclusive: c_int, q_num: *const u32, n_q: u32, q_den: u32,
                                           bases: *mut FFI_ArrowArray, bases_schema: *mut FFI_ArrowSchema,
                                           min: *mut FFI_ArrowArray, min_schema: *mut FFI_ArrowSchema,
                                           max: *mut FFI_ArrowArray, max_schema: *mut FFI_ArrowSchema,
                                           q: *mut FFI_ArrowArray, q_schemas: *mut FFI_ArrowSchema) -> c_int;
}

/// What `IntervalJoinStream` keeps per partition when `Algorithm::Hip` is selected.
pub struct HipJoinStream {
    session: *mut BrhSession,
    js: *mut BrhJoinStream,
    /// probe batches pushed but not yet returned in a result (the payload `take` needs them)
    pending: Vec<RecordBatch>,
}

impl HipJoinStream {
    fn check(&self, rc: c_int) -> Result<()> {
        if rc == 0 { return Ok(()); }
        let msg = unsafe { CStr::from_ptr(brh_last_error(self.session)) }.to_string_lossy().into_owned();
        Err(DataFusionError::Execution(msg))
    }

    /// FetchProbeBatch + ProcessProbeBatch (interval_join.rs:1107-1140, :1614-1653): hand the batch over; if a
    /// coalesced group became ready, return its pairs together with the concatenated probe batches they refer to.
    pub fn push(&mut self, batch: RecordBatch) -> Result<Option<(UInt32Array, UInt32Array, RecordBatch)>> {
        let (arr, sch) = to_ffi(&StructArray::from(batch.clone()).into_data())?;
        let mut ready: c_int = 0;
        self.pending.push(batch);
        self.check(unsafe { brh_join_stream_push(self.js, BrhBatch { array: &arr, schema: &sch }, &mut ready) })?;
        if ready == 0 { Ok(None) } else { self.next().map(Some) }
    }

    /// ExhaustedProbeSide: flush the last, partial group.
    pub fn finish(&mut self) -> Result<Option<(UInt32Array, UInt32Array, RecordBatch)>> {
        let mut ready: c_int = 0;
        self.check(unsafe { brh_join_stream_finish(self.js, &mut ready) })?;
        if ready == 0 { Ok(None) } else { self.next().map(Some) }
    }

    fn next(&mut self) -> Result<(UInt32Array, UInt32Array, RecordBatch)> {
        let (mut first, mut nb, mut done) = (0u64, 0u64, 0 as c_int);
        let (mut ba, mut bs) = (FFI_ArrowArray::empty(), FFI_ArrowSchema::empty());
        let (mut pa, mut ps) = (FFI_ArrowArray::empty(), FFI_ArrowSchema::empty());
        let (mut oa, mut os) = (FFI_ArrowArray::empty(), FFI_ArrowSchema::empty());
        self.check(unsafe { brh_join_stream_next(self.js, &mut first, &mut nb, &mut done, &mut ba, &mut bs, &mut pa, &mut ps, &mut oa, &mut os) })?;
        let build_idx = UInt32Array::from(unsafe { from_ffi(ba, &bs) }?);
        let probe_idx = UInt32Array::from(unsafe { from_ffi(pa, &ps) }?);
        let _offsets = Int64Array::from(unsafe { from_ffi(oa, &os) }?);   // first row of every batch in the group
        // the group's batches in push order = the rows probe_idx counts over.  A bounded-output stream
        // (max_output_rows > 0, the low-memory mode) returns several results per group: the batches go with the last one
        let group: Vec<RecordBatch> = if done != 0 { self.pending.drain(..nb as usize).collect() } else { self.pending[..nb as usize].to_vec() };
        let probe = concat_batches(&group[0].schema(), &group)?;
        Ok((build_idx, probe_idx, probe))
        // caller: build_batch_from_indices(schema, build_side, &probe, &build_idx, &probe_idx, ..)  (interval_join.rs:1655-1667)
    }
}

impl Drop for HipJoinStream {
    fn drop(&mut self) { unsafe { brh_join_stream_close(self.js) } }
}

#[allow(unused)]
fn _types(_: ArrayRef) {}
