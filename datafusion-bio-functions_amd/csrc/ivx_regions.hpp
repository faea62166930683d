// ivx_regions.hpp -- what the two halves of the region-partitioned probe share: ivx_regions_route.hip routes probe rows to
// index regions and describes where it put them (ivx_routed, ivx_internal.hpp); ivx_regions_probe.hip probes a region's
// rows against its LDS-resident slice of the index.  Private to those two files.
#pragma once
#include <type_traits>
#include <cstdlib>
#include <cstring>
#include "ivx_rowops.hpp"

// PK (8-byte routed rows, hdr[HDR_PK24]): a routed row is ONE word,
//     bits  0..23  start inside its region          bits 24..31  length (end - start), low 8 bits
//     bits 32..    row id (rowbits bits)             bits 32+rowbits..63  length, the bits above the low 8
// so the fewer rows a batch has, the longer a row may be (100 M rows: 27 bits of row id, lengths up to 8190).  A length
// field of all ones marks a row that does not fit -- it starts outside its region's coordinates (before the key's first
// or behind its last start), is too long, or has end < start: the probe reads such a row's coordinates from the input
// columns by its row id.
// the length field's all-ones value: 8 bits plus the row id's spare bits, at most 16 (the host passes rowbits = 32, i.e. no
// spare bits, when the occupancy bitmap is in use: the partition kernel then has no register to carry the upper bits in)
__host__ __device__ __forceinline__ u32 pk_maxlen(u32 rowbits) { const u32 spare = rowbits >= 32 ? 0u : 32u - rowbits; return (1u << (8u + (spare > 8u ? 8u : spare))) - 1u; }
// the reading side of the format (the packing side is k_part_onepass, whose fields are parked across registers): rel = start
// inside the region, len = the length field (pk_maxlen(rowbits): an escape), hi = the word's upper half, from which callers
// that want the row id mask it (hi & rowmask; the lean kernels put that off: see k_fill_fast's copy-out)
struct PkRow { u32 rel, len, hi; };
__device__ __forceinline__ PkRow pk_unpack(u64 w, u32 rowbits)
{
    const u32 lo32 = (u32)w, hi32 = (u32)(w >> 32);
    return PkRow{lo32 & 0xFFFFFFu, (lo32 >> 24) | ((rowbits < 32 ? (hi32 >> rowbits) & 0xFFu : 0u) << 8), hi32};
}

// Where routed row v of region r (v: its number inside the region, "virtual row") sits in the page pool.  A page-table entry
// of 0 means the partition never published the page: that cannot happen once k_part_onepass has completed (it did in a
// profiling build whose switch skipped the publication, and the page "0 - 1" then was a wild address).  The word of page 0
// is returned instead, which is in bounds, and miss() is called: the fill kernels raise the fault word there, the per-row
// value and mark kernels pass a no-op.
template <class W, class Miss>
__device__ __forceinline__ W *routed_word(const PageTab &pt, W *pool, u32 r, u32 v, Miss &&miss)
{
    u32 pg = pt.ptab[(u64)r * pt.pstride + (v >> pt.lgpg)];
    if (pg == 0u) { pg = 1u; miss(); }
    return pool + (((u64)(pg - 1u) << pt.lgpg) + (v & ((1u << pt.lgpg) - 1u)));
}

constexpr int RP_W = RP_T / IVX_WAVE;
// the lean probes deal their work in CHUNKS of 8192 routed rows that never straddle a pool page (k_chunk_bounds, k_fill_fast)
constexpr u32 FP_CHUNK = (u32)RP_W * IVX_WAVE * 8u;

// Rows the lean kernel does not take: region, first virtual row, rows -- ONE row the packed form cannot carry (an escape, or
// a row that reaches past its slice's halo; listed by its lane, the rest of its batch goes the fast way), or a whole batch
// that found more pairs than the ring holds (nothing of it stays staged).  k_fill_fast appends them to a list; k_fill_rest
// walks the listed rows afterwards with the generic gather walk -- the lean kernel holds no generic code (and no scratch).
struct FpRest { u32 r, first, cnt, pad; };
// the two lists live in one scratch buffer: batches first (at most one per wavefront batch), then single rows (at most n)
__host__ __device__ __forceinline__ u64 fp_max_batches(u64 n, u32 nreg) { return ((n >> 13) + nreg + 1) * (u64)(RP_W * 8); }

// ------------------------------------------------------------------ routing (ivx_regions_route.hip)
// Each fills in *R (and R->slots); none waits for an index's `ready` event: all they read of the index is final before a
// build tail starts.
// flat two-pass partition: ndig digits (256: up to IVX_MAXREG regions, 1024: up to IVX_MAXREG_WIDE); ids16: chunk-local u16
// indices (R->cidx) instead of row ids; a workgroup takes 1, 2 or 4 tiles by n, at most max_tiles
ivx_status ivx_route_flat(ivx_ctx *ctx, const JoinIndexView &jv, const u32 *key, const i32 *s, const i32 *e, u64 n, u32 adj,
                          u32 ndig, bool ids16, u32 max_tiles, ivx_routed *R);
// one-pass partition into region pages (nreg <= IVX_MAXREG_WIDE).  rowval (per-row-value consumers; always packed, nreg <=
// IVX_MAXREG): also vtab for the un-permute (no_vtab: a consumer that never un-permutes, the marks: no table, and the
// 16384-row tiles stay open to it).  lean: the consumer may run the lean kernels (rest lists, chunk table)
// zero2 (nullable): two 64-bit words of the caller's that the pass's clearing kernel zeroes on the way (a memset launch less)
// defer_bounds: the regions' first rows and first chunks (R->rfirst, ctl->cfirst: k_chunk_bounds) are not computed and
// R->tables_due says so; a probe that reads them queues ivx_route_paged_bounds behind the pass first (probe_pairs does, on
// every way but the lean pair alone: k_fill_fast scans the regions' row counts itself)
struct ivx_paged_opts { bool filter, packed, rowval, lean; u32 adj; u64 *zero2 = nullptr; bool defer_bounds = false; bool no_vtab = false; };
ivx_status ivx_route_paged(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const u32 *key, const i32 *s, const i32 *e, u64 n,
                           const ivx_paged_opts &o, ivx_routed *R);
ivx_status ivx_route_paged_bounds(ivx_ctx *ctx, const ivx_routed &R, u32 nreg);
// more than IVX_MAXREG_WIDE regions: two partition passes (super-region, then region inside it) and a global region table
ivx_status ivx_route_two_level(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const u32 *key, const i32 *s, const i32 *e, u64 n, ivx_routed *R);
// one u32 value per routed row back into input order, as kind (IVX_RV_*) wants it: FLAT, val[] in routed order; PAGED (rowval),
// the values sit in the low halves of the rows' own words.  *d_total += the values (IVX_RV_PER_ROW)
ivx_status ivx_unroute_values(ivx_ctx *ctx, const ivx_routed &R, u32 nreg, int kind, const u32 *val, u64 n, void *out, u64 *d_total, int sorted_done = 0);
// the overlap aggregates' records back into input order (PAGED, rowval): rec.* are indexed like the page pool, one array per
// wanted output of `out` (null: not wanted); rows that were never routed get the empty result (0, and the min / max identities)
ivx_status ivx_unroute_records(ivx_ctx *ctx, const ivx_routed &R, u32 nreg, u64 n, const AggOut &rec, const AggOut &out);
// the same for overlap select's records: rows that were never routed get (IVX_NULL_IDX, 0)
ivx_status ivx_unroute_sel_records(ivx_ctx *ctx, const ivx_routed &R, u32 nreg, u64 n, const SelOut &rec, const SelOut &out);
