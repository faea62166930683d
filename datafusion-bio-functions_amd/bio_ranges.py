"""Table-level mirror of the reference's range functions, driven through libbio_ranges_hip.so
(Arrow C Data Interface) -- what a DataFusion session would expose as

    count_overlaps('l','r'), coverage('l','r'), nearest('l','r',k,overlap,distance),
    overlap('l','r'[,mode]), merge('t'[,min_dist]), subtract('l','r'), cluster('t'[,min_dist]), complement('t'[,'view']),
    intersect('l','r') -- subtract's dual, which the reference does not have: the parts of the left rows that the right table covers,
    depth('reads') of the pileup crate,
    and the SQL range join handled by IntervalJoinExec

Argument meaning and output schemas follow R/src/table_function.rs and the providers
(`left_`/`right_` prefixes: nearest.rs:57-78, overlap.rs:106-126; appended `count`/`coverage`
column: count_overlaps.rs:60-66; Int64 start/end + n_intervals: merge.rs:43-48).  pyarrow only
plays DataFusion's part (holding the tables, `take` of payload columns); every interval
computation happens in the HIP kernels.  There is no CPU fallback.
"""
import ctypes as C
import os

import pyarrow as pa
import pyarrow.compute as pc

import pyivx

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "lib", "libbio_ranges_hip.so")

DEFAULT_COLS = ("contig", "pos_start", "pos_end")
WEAK, STRICT = 0, 1
JOIN_INNER, JOIN_RIGHT_SEMI, JOIN_RIGHT_ANTI = 0, 1, 2
# (3 = BRH_JOIN_NEAREST, join stream only)  The build-side and outer types: SQL semantics over the build side's match marks
JOIN_LEFT_SEMI, JOIN_LEFT_ANTI, JOIN_LEFT, JOIN_RIGHT, JOIN_FULL = 4, 5, 6, 7, 8
# the outputs of overlap_aggregate, in the order of the BRH_AGG_* bits (include/bio_ranges_host.h)
AGG_OPS = ("count", "sum", "min", "max", "bases", "wsum")
# the criteria of overlap_select, in the order of the BRH_SEL_* enum (include/bio_ranges_host.h)
SEL_BY = pyivx.SEL_BY
# an overlap threshold (`where=` of interval_join, overlap_aggregate and overlap_select): a pyivx.OverlapWhere or a dict of its
# keywords -- min_bases, probe / build (minimum fractions of the probe / build row that the overlap covers: a (num, den) pair, a
# Fraction, or a float, which is taken as Fraction(f).limit_denominator(10**9)) and either.  brh_overlap_where has the layout of
# ivx_overlap_where.
OverlapWhere = pyivx.OverlapWhere


class _ArrowSchema(C.Structure):
    pass


class _ArrowArray(C.Structure):
    pass


_ArrowSchema._fields_ = [("format", C.c_char_p), ("name", C.c_char_p), ("metadata", C.c_char_p), ("flags", C.c_int64),
                         ("n_children", C.c_int64), ("children", C.POINTER(C.POINTER(_ArrowSchema))),
                         ("dictionary", C.POINTER(_ArrowSchema)), ("release", C.c_void_p), ("private_data", C.c_void_p)]
_ArrowArray._fields_ = [("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64), ("n_buffers", C.c_int64),
                        ("n_children", C.c_int64), ("buffers", C.POINTER(C.c_void_p)),
                        ("children", C.POINTER(C.POINTER(_ArrowArray))), ("dictionary", C.POINTER(_ArrowArray)),
                        ("release", C.c_void_p), ("private_data", C.c_void_p)]


class _Batch(C.Structure):
    _fields_ = [("array", C.POINTER(_ArrowArray)), ("schema", C.POINTER(_ArrowSchema))]


class _Columns(C.Structure):
    _fields_ = [("keys", C.POINTER(C.c_char_p)), ("n_keys", C.c_int), ("start", C.c_char_p), ("end", C.c_char_p)]


class BioRangesError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is None:
        pyivx.lib()                                   # loads libivx_hip.so (and the HIP runtime) first
        _lib = C.CDLL(os.environ.get("BRH_LIB") or _LIB_PATH)     # BRH_LIB: another build of the host library (the sanitizer build)
        _lib.brh_last_error.restype = C.c_char_p
    return _lib


class _Exported:
    """A pyarrow Table exported as one struct array (kept alive for the call)."""

    def __init__(self, table):
        self.batch = table.combine_chunks().to_batches()[0] if table.num_rows else pa.RecordBatch.from_pylist([], schema=table.schema)
        self.arr, self.sch = _ArrowArray(), _ArrowSchema()
        self.batch._export_to_c(C.addressof(self.arr), C.addressof(self.sch))
        self.c = _Batch(C.pointer(self.arr), C.pointer(self.sch))

    def close(self):
        for obj in (self.arr, self.sch):
            if obj.release:
                C.CFUNCTYPE(None, C.c_void_p)(obj.release)(C.addressof(obj))


def _cols(cols):
    keys = cols[0] if isinstance(cols[0], (list, tuple)) else [cols[0]]
    arr = (C.c_char_p * len(keys))(*[k.encode() for k in keys])
    c = _Columns(arr, len(keys), cols[1].encode(), cols[2].encode())
    c._keep = arr
    return c


def _out():
    return _ArrowArray(), _ArrowSchema()


def _import(a, s):
    return pa.Array._import_from_c(C.addressof(a), C.addressof(s))


class Session:
    """create_bio_session() counterpart: owns the GPU context."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        rc = lib().brh_session_create(C.c_int(device), C.byref(self.h))
        if rc != 0:
            raise BioRangesError(f"no usable gfx950 device (status {rc}); there is no CPU fallback")

    def close(self):
        if self.h:
            lib().brh_session_free(self.h)
            self.h = None

    def _chk(self, rc):
        if rc != 0:
            raise BioRangesError(lib().brh_last_error(self.h).decode())

    def metrics(self):
        """BuildProbeJoinMetrics of the session (joins/utils.rs:399-453): build_time, join_time [ms], build_input_batches,
        build_input_rows, build_mem_used, input_batches, input_rows, output_batches, output_rows."""
        m = pyivx.Metrics()
        self._chk(lib().brh_session_metrics(self.h, C.byref(m)))
        return {f: getattr(m, f) for f, _ in pyivx.Metrics._fields_}

    def set_strict_null_contigs(self, on=True):
        """refuse batches with NULL contigs instead of treating them as the reference does (bio_ranges_host.h)"""
        self._chk(lib().brh_session_set_strict_null_contigs(self.h, C.c_int(int(on))))

    def set_string_cigars(self, on=True):
        """depth(), depth_per_base() and depth_stream() accept a Utf8 / LargeUtf8 cigar column ("5M3D5M"), parsed on the
        device; off (the default) such a column is refused (bio_ranges_host.h brh_session_set_string_cigars)"""
        self._chk(lib().brh_session_set_string_cigars(self.h, C.c_int(int(on))))

    def set_memory_limit(self, nbytes):
        """device bytes the session may reserve (MemoryReservation, interval_join.rs:614-639); 0 = no limit"""
        self._chk(lib().brh_session_set_memory_limit(self.h, C.c_uint64(int(nbytes))))

    def reserved_bytes(self):
        """device bytes the session holds reserved right now: scratch plus live indexes and depth profiles"""
        n = C.c_uint64(0)
        self._chk(lib().brh_session_reserved_bytes(self.h, C.byref(n)))
        return n.value

    # ---- count_overlaps / coverage: RangeTableFunction (table_function.rs:521-560)
    def _count(self, left, right, cols_left, cols_right, strict, coverage):
        L, R = _Exported(left), _Exported(right)
        a, s = _out()
        try:
            self._chk(lib().brh_count_overlaps(self.h, L.c, _cols(cols_left), R.c, _cols(cols_right),
                                               C.c_int(STRICT if strict else WEAK), C.c_int(int(coverage)), C.byref(a), C.byref(s)))
        finally:
            L.close(); R.close()
        col = _import(a, s)
        return right.append_column("coverage" if coverage else "count", col)

    def count_overlaps(self, left, right, cols_left=DEFAULT_COLS, cols_right=DEFAULT_COLS, strict=False):
        return self._count(left, right, cols_left, cols_right, strict, False)

    def coverage(self, left, right, cols_left=DEFAULT_COLS, cols_right=DEFAULT_COLS, strict=False):
        return self._count(left, right, cols_left, cols_right, strict, True)

    # ---- nearest: NearestTableFunction (table_function.rs:286-367)
    def nearest(self, left, right, k=1, overlap=True, compute_distance=True, cols_left=DEFAULT_COLS, cols_right=DEFAULT_COLS,
                strict=False, direction="any", max_distance=None):
        """direction: "any" | "before" ("upstream": only left rows that end before the right row) | "after" ("downstream": only
        left rows that start after it); max_distance: no left row farther than that is an answer (None: no cap).  Direction
        does not touch overlapping rows: `overlap` alone decides them.  The defaults are the reference's nearest()."""
        d = pyivx.NEAR_ALIASES.get(direction, direction)
        if d not in pyivx.NEAR_DIRECTIONS:
            raise ValueError(f"direction must be one of {pyivx.NEAR_DIRECTIONS + tuple(pyivx.NEAR_ALIASES)}, got {direction!r}")
        if max_distance is not None and int(max_distance) < 0:
            raise ValueError(f"max_distance must be >= 0 or None, got {max_distance!r}")
        L, R = _Exported(left), _Exported(right)
        (la, ls), (ra, rs), (da, ds) = _out(), _out(), _out()
        try:
            head = (self.h, L.c, _cols(cols_left), R.c, _cols(cols_right), C.c_int(STRICT if strict else WEAK),
                    C.c_uint32(int(k)), C.c_int(int(overlap)), C.c_int(int(compute_distance)))
            outs = (C.byref(la), C.byref(ls), C.byref(ra), C.byref(rs), C.byref(da), C.byref(ds))
            if d == "any" and max_distance is None:
                self._chk(lib().brh_nearest(*head, *outs))
            else:
                self._chk(lib().brh_nearest_dir(*head, C.c_int(pyivx.NEAR_DIRECTIONS.index(d)), C.c_int64(int(max_distance if max_distance is not None else -1)),
                                                *outs))
        finally:
            L.close(); R.close()
        li, ri = _import(la, ls), _import(ra, rs)
        out = {}
        for name in left.schema.names:                       # nearest.rs:57-78: left_*, right_*, distance
            out["left_" + name] = pc.take(left.column(name), li)
        for name in right.schema.names:
            out["right_" + name] = pc.take(right.column(name), ri)
        if compute_distance:
            out["distance"] = _import(da, ds)
        return pa.table(out)

    # ---- IntervalJoinExec (the SQL range join), `build` = the SQL join's left table
    def interval_join(self, build, probe, cols_build=DEFAULT_COLS, cols_probe=DEFAULT_COLS, join_type=JOIN_INNER,
                      strict_predicate=False, nearest_algorithm=False, where=None):
        """-> (build_idx, probe_idx) UInt32 arrays.  JOIN_RIGHT_SEMI / _ANTI: probe_idx only; JOIN_LEFT_SEMI / _ANTI: build_idx
        only, ascending; JOIN_LEFT / _RIGHT / _FULL: the Inner pairs, then the unmatched rows with a NULL on the other side.
        where (OverlapWhere): only overlaps that pass the threshold are matches, for every join type alike."""
        wp, _keep = pyivx.as_where(where)
        B, P = _Exported(build), _Exported(probe)
        (ba, bs), (pa_, ps) = _out(), _out()
        try:
            if where is not None:
                self._chk(lib().brh_interval_join_where(self.h, B.c, _cols(cols_build), P.c, _cols(cols_probe), C.c_int(join_type),
                                                        C.c_int(int(strict_predicate)), C.c_int(int(nearest_algorithm)), wp,
                                                        C.byref(ba), C.byref(bs), C.byref(pa_), C.byref(ps)))
            else:
                self._chk(lib().brh_interval_join(self.h, B.c, _cols(cols_build), P.c, _cols(cols_probe), C.c_int(join_type),
                                                  C.c_int(int(strict_predicate)), C.c_int(int(nearest_algorithm)),
                                                  C.byref(ba), C.byref(bs), C.byref(pa_), C.byref(ps)))
        finally:
            B.close(); P.close()
        return _import(ba, bs), _import(pa_, ps)

    # ---- overlap aggregates: the join grouped by probe row, a build-side value aggregated (no pairs are made)
    def overlap_aggregate(self, build, probe, value, ops=AGG_OPS, cols_build=DEFAULT_COLS, cols_probe=DEFAULT_COLS,
                          strict_predicate=False, where=None):
        """per row of `probe`, over the rows of `build` it overlaps (where: with an overlap that passes the threshold): aggregates of build's column `value` (Int8 .. Int64 or
        UInt8 .. UInt32) -> a table of Int64 columns named after `ops` (AGG_OPS), one row per probe row in probe order.
        count and bases are non-null; sum, min, max and wsum are NULL where count is 0."""
        unknown = [o for o in ops if o not in AGG_OPS]
        if unknown or not ops:
            raise BioRangesError(f"overlap_aggregate: ops is a non-empty subset of {AGG_OPS}, got {tuple(ops)}")
        mask = sum(1 << AGG_OPS.index(o) for o in set(ops))
        wp, _keep = pyivx.as_where(where)
        B, P = _Exported(build), _Exported(probe)
        arrs, schs = (_ArrowArray * len(AGG_OPS))(), (_ArrowSchema * len(AGG_OPS))()
        try:
            if where is not None:
                self._chk(lib().brh_overlap_aggregate_where(self.h, B.c, _cols(cols_build), value.encode(), P.c, _cols(cols_probe),
                                                            C.c_int(int(strict_predicate)), C.c_uint32(mask), wp, arrs, schs))
            else:
                self._chk(lib().brh_overlap_aggregate(self.h, B.c, _cols(cols_build), value.encode(), P.c, _cols(cols_probe),
                                                      C.c_int(int(strict_predicate)), C.c_uint32(mask), arrs, schs))
        finally:
            B.close(); P.close()
        got = {o: _import(arrs[i], schs[i]) for i, o in enumerate(AGG_OPS) if mask & (1 << i)}
        return pa.table({o: got[o] for o in ops})

    # ---- overlap select: the join reduced to the one best build row per probe row (no pairs are made)
    def overlap_select(self, build, probe, by, value=None, cols_build=DEFAULT_COLS, cols_probe=DEFAULT_COLS,
                       strict_predicate=False, where=None):
        """per row of `probe`, of the rows of `build` it overlaps (where: with an overlap that passes the threshold), the one that is best by `by` (SEL_BY; ties: the smallest
        build row) -> (build_idx, score), one row per probe row in probe order.  build_idx: UInt32, NULL without a match --
        take_table(build, build_idx) gives the left join to at most one row.  score: Int64, NULL where build_idx is: the
        winner's value, closed overlap length or row.  `value` names build's value column for "min_val" / "max_val" (and for
        them only): Int8 .. Int64, UInt8 .. UInt64, Float32 or Float64 without nulls or NaNs; for UInt64 and float columns
        score is None (take the value with build_idx)."""
        if by not in SEL_BY:
            raise BioRangesError(f"overlap_select: by is one of {SEL_BY}, got {by!r}")
        wp, _keep = pyivx.as_where(where)
        B, P = _Exported(build), _Exported(probe)
        (ia, is_), (sa, ss) = _out(), _out()
        try:
            if where is not None:
                self._chk(lib().brh_overlap_select_where(self.h, B.c, _cols(cols_build), None if value is None else value.encode(), P.c,
                                                         _cols(cols_probe), C.c_int(int(strict_predicate)), C.c_int(SEL_BY.index(by)), wp,
                                                         C.byref(ia), C.byref(is_), C.byref(sa), C.byref(ss)))
            else:
                self._chk(lib().brh_overlap_select(self.h, B.c, _cols(cols_build), None if value is None else value.encode(), P.c,
                                                   _cols(cols_probe), C.c_int(int(strict_predicate)), C.c_int(SEL_BY.index(by)),
                                                   C.byref(ia), C.byref(is_), C.byref(sa), C.byref(ss)))
        finally:
            B.close(); P.close()
        return _import(ia, is_), (_import(sa, ss) if sa.release else None)

    def sql_range_join(self, build, probe, cols_build=DEFAULT_COLS, cols_probe=DEFAULT_COLS, strict_predicate=False,
                       nearest_algorithm=False, device_take=False):
        """SELECT * FROM build JOIN probe ON key = key AND range predicate  (build columns, then probe columns)."""
        bi, pi = self.interval_join(build, probe, cols_build, cols_probe, JOIN_INNER, strict_predicate, nearest_algorithm)
        if device_take:                                      # payload gather on the GPU as well
            cols = list(self.take_table(build, bi).values()) + list(self.take_table(probe, pi).values())
        else:
            cols = [pc.take(build.column(n), bi) for n in build.schema.names] + [pc.take(probe.column(n), pi) for n in probe.schema.names]
        names = [f"l.{n}" for n in build.schema.names] + [f"r.{n}" for n in probe.schema.names]
        return pa.table(cols, names=names)

    def join_stream(self, build, cols_build=DEFAULT_COLS, cols_probe=DEFAULT_COLS, strict_predicate=False, coalesce_rows=0,
                    join_type="inner", max_output_rows=0):
        """IntervalJoinStream as a push interface: index `build` once, then push probe batches; see JoinStream.
        join_type: "inner" | "right_semi" | "right_anti" | "nearest" (Algorithm::CoitreesNearest) | "left_semi" | "left_anti" |
        "left" | "right" | "full" (these five: finish() ends with one result of n_batches = 0 that carries the build-side rows;
        max_output_rows must be 0);
        max_output_rows: 0 = one result per group, N = the low-memory stream's output budget, "env" = the reference's
        default (BIO_MAX_OUTPUT_BATCH_SIZE or 100000)."""
        return JoinStream(self, build, cols_build, cols_probe, strict_predicate, coalesce_rows, join_type, max_output_rows)

    # ---- overlap UDTF (overlap.rs:154-226): FROM right AS b, left AS a  => the user's RIGHT table is the build side
    def overlap(self, left, right, mode="join", cols_left=DEFAULT_COLS, cols_right=DEFAULT_COLS, strict=False):
        if mode == "left":                                   # LeftDistinct: RIGHT SEMI JOIN, left rows that have a match
            _, pi = self.interval_join(right, left, cols_right, cols_left, JOIN_RIGHT_SEMI, strict)
            return left.take(pi)
        bi, pi = self.interval_join(right, left, cols_right, cols_left, JOIN_INNER, strict)
        if mode == "left_all":                               # Inner projecting left only (overlap multiplicity kept)
            return left.take(pi)
        out = {"left_" + n: pc.take(left.column(n), pi) for n in left.schema.names}
        out.update({"right_" + n: pc.take(right.column(n), bi) for n in right.schema.names})
        return pa.table(out)

    # ---- merge (table_function.rs:441-464)
    def merge(self, table, min_dist=0, cols=DEFAULT_COLS, strict=False):
        if min_dist < 0:
            raise BioRangesError(f"merge() min_dist must be >= 0, got {min_dist}")          # table_function.rs:237
        T = _Exported(table)
        outs = [_out() for _ in range(4)]
        try:
            self._chk(lib().brh_merge(self.h, T.c, _cols(cols), C.c_int64(int(min_dist)), C.c_int(STRICT if strict else WEAK),
                                      *[C.byref(x) for pair in outs for x in pair]))
        finally:
            T.close()
        key = cols[0] if isinstance(cols[0], str) else cols[0][0]
        return pa.table([_import(*o) for o in outs], names=[key, cols[1], cols[2], "n_intervals"])

    # ---- subtract (table_function.rs:574-612); extra left columns are carried along (subtract.rs:501-527)
    def subtract(self, left, right, cols_left=DEFAULT_COLS, cols_right=DEFAULT_COLS, strict=False):
        return self._left_pieces(lib().brh_subtract, left, right, cols_left, cols_right, strict)

    # ---- intersect: the pieces of the left rows that the right table's merged intervals cover (include/ivx.h ivx_intersect);
    # schema, order and extra left columns as subtract
    def intersect(self, left, right, cols_left=DEFAULT_COLS, cols_right=DEFAULT_COLS, strict=False):
        return self._left_pieces(lib().brh_intersect, left, right, cols_left, cols_right, strict)

    def _left_pieces(self, fn, left, right, cols_left, cols_right, strict):
        L, R = _Exported(left), _Exported(right)
        outs = [_out() for _ in range(4)]
        try:
            self._chk(fn(self.h, L.c, _cols(cols_left), R.c, _cols(cols_right), C.c_int(STRICT if strict else WEAK),
                         *[C.byref(x) for pair in outs for x in pair]))
        finally:
            L.close(); R.close()
        contig, start, end, row = [_import(*o) for o in outs]
        key = cols_left[0] if isinstance(cols_left[0], str) else cols_left[0][0]
        cols = []
        for n in left.schema.names:
            cols.append(contig if n == key else start if n == cols_left[1] else end if n == cols_left[2] else pc.take(left.column(n), row))
        return pa.table(cols, names=left.schema.names)


    # ---- f3: compute::take of payload columns on the device (interval_join.rs:1655-1667, nearest.rs:469-482)
    def take(self, column, idx):
        """column: pyarrow Array / ChunkedArray of any flat, dictionary-encoded or nested (struct / list / map) type;
        idx: UInt32 array (nulls -> null rows).  Raises for layouts the gather does not cover (unions, run-end encoding)."""
        if isinstance(column, pa.ChunkedArray):
            column = column.combine_chunks() if column.num_chunks != 1 else column.chunk(0)
        if isinstance(idx, pa.ChunkedArray):
            idx = idx.combine_chunks()
        ca, cs, ia, is_ = _ArrowArray(), _ArrowSchema(), _ArrowArray(), _ArrowSchema()
        column._export_to_c(C.addressof(ca), C.addressof(cs))
        idx._export_to_c(C.addressof(ia), C.addressof(is_))
        a, sc = _out()
        try:
            self._chk(lib().brh_take(self.h, C.byref(ca), C.byref(cs), C.byref(ia), C.byref(is_), C.byref(a), C.byref(sc)))
        finally:
            for obj in (ca, cs, ia, is_):
                if obj.release:
                    C.CFUNCTYPE(None, C.c_void_p)(obj.release)(C.addressof(obj))
        return _import(a, sc)

    def take_table(self, table, idx, prefix=""):
        return {prefix + n: self.take(table.column(n), idx) for n in table.schema.names}

    # ---- cluster (table_function.rs:574-612; ClusterProvider cluster.rs:29-82)
    def cluster(self, table, min_dist=0, cols=DEFAULT_COLS, strict=False):
        if min_dist < 0:
            raise BioRangesError(f"cluster() min_dist must be >= 0, got {min_dist}")        # table_function.rs:237
        T = _Exported(table)
        outs = [_out() for _ in range(7)]
        try:
            self._chk(lib().brh_cluster(self.h, T.c, _cols(cols), C.c_int64(int(min_dist)), C.c_int(STRICT if strict else WEAK),
                                        *[C.byref(x) for pair in outs for x in pair]))
        finally:
            T.close()
        contig, start, end, row, cl, cs, ce = [_import(*o) for o in outs]
        key = cols[0] if isinstance(cols[0], str) else cols[0][0]
        if table.num_columns > 3:                            # extra columns: every input field kept as it is (cluster.rs:50-53)
            out_cols = [pc.take(table.column(n), row) for n in table.schema.names]
            names = list(table.schema.names)
        else:
            out_cols, names = [contig, start, end], [key, cols[1], cols[2]]
        return pa.table(out_cols + [cl, cs, ce], names=names + ["cluster", "cluster_start", "cluster_end"])

    # ---- complement (table_function.rs:614-786; ComplementProvider complement.rs:28-75)
    def complement(self, table, view=None, cols=DEFAULT_COLS, view_cols=None, strict=False):
        T = _Exported(table)
        V = _Exported(view) if view is not None else None
        outs = [_out() for _ in range(3)]
        try:
            vb = V.c if V is not None else _Batch(None, None)
            self._chk(lib().brh_complement(self.h, T.c, _cols(cols), vb, _cols(view_cols or cols), C.c_int(STRICT if strict else WEAK),
                                           *[C.byref(x) for pair in outs for x in pair]))
        finally:
            T.close()
            if V is not None:
                V.close()
        key = cols[0] if isinstance(cols[0], str) else cols[0][0]
        return pa.table([_import(*o) for o in outs], names=[key, cols[1], cols[2]])


    # ---- depth (bio-function-pileup: table_function.rs depth(); events.rs + coverage.rs)
    def depth(self, reads, prior=None, lengths=None, filter_flag=1796, min_mapq=0):
        """coverage blocks of a reads table (chrom, start UInt32, flags UInt32, mapping_quality UInt32, cigar Binary -- or
        Utf8 / LargeUtf8 text after set_string_cigars(True)):
        -> contig Utf8, pos_start Int32, pos_end Int32, coverage Int16.  prior: the blocks of an earlier call, added in;
        lengths: a table (name, length) that turns the reference's dense-mode clipping on."""
        tabs = [_Exported(t) if t is not None else None for t in (reads, prior, lengths)]
        outs = [_out() for _ in range(4)]
        try:
            b = [t.c if t is not None else _Batch(None, None) for t in tabs]
            self._chk(lib().brh_depth(self.h, b[0], b[1], b[2], C.c_uint32(int(filter_flag)), C.c_uint32(int(min_mapq)),
                                      *[C.byref(x) for pair in outs for x in pair]))
        finally:
            for t in tabs:
                if t is not None:
                    t.close()
        return pa.table([_import(*o) for o in outs], names=["contig", "pos_start", "pos_end", "coverage"])

    def depth_per_base(self, reads, prior=None, lengths=None, zero_based=False, batch_rows=8192, filter_flag=1796, min_mapq=0):
        """depth(..., per_base = true): a generator of tables (contig Utf8, pos Int32, coverage Int16), one row per position
        of every contig of `lengths` that has reads, contigs in byte order, at most batch_rows rows a table and one contig a
        table.  Positions are [0, len) when zero_based, else [1, len + 1).  The profile is built on the first next(); the
        stream is closed when the generator is exhausted, closed or dropped."""
        tabs = [_Exported(t) if t is not None else None for t in (reads, prior, lengths)]
        h = C.c_void_p()
        try:
            b = [t.c if t is not None else _Batch(None, None) for t in tabs]
            self._chk(lib().brh_depth_per_base_open(self.h, b[0], b[1], b[2], C.c_int(int(bool(zero_based))), C.c_uint32(int(filter_flag)),
                                                    C.c_uint32(int(min_mapq)), C.byref(h)))
        finally:
            for t in tabs:
                if t is not None:
                    t.close()
        try:
            while True:
                outs = [_out() for _ in range(3)]
                done = C.c_int(0)
                self._chk(lib().brh_depth_per_base_next(h, C.c_uint64(int(batch_rows)), C.byref(done), *[C.byref(x) for pair in outs for x in pair]))
                if done.value:
                    return
                yield pa.table([_import(*o) for o in outs], names=["contig", "pos", "coverage"])
        finally:
            lib().brh_depth_per_base_close(h)

    def depth_regions(self, reads, regions, prior=None, lengths=None, zero_based=False, end_exclusive=False, thresholds=(),
                      cols=DEFAULT_COLS, filter_flag=1796, min_mapq=0):
        """depth summarised per row of `regions` (contig, start, end as `cols` names them; ends inclusive, or BED-style
        half-open with end_exclusive): -> the regions table with bases Int64 (positions counted), sum Int64 (coverage summed
        over them: mean depth = sum / bases) and one bases_ge_<t> Int64 per threshold (positions with coverage >= t)
        appended.  reads / prior / lengths as for depth(); with lengths the positions are those depth_per_base() emits."""
        tabs = [_Exported(t) if t is not None else None for t in (reads, prior, lengths, regions)]
        try:
            b = [t.c if t is not None else _Batch(None, None) for t in tabs]
            return _regions_call(self, regions, thresholds, lambda *outs: lib().brh_depth_regions(
                self.h, b[0], b[1], b[2], b[3], _cols(cols), C.c_int(int(bool(zero_based))), C.c_int(int(bool(end_exclusive))),
                C.c_uint32(int(filter_flag)), C.c_uint32(int(min_mapq)), *outs))
        finally:
            for t in tabs:
                if t is not None:
                    t.close()

    def depth_region_quantiles(self, reads, regions, prior=None, lengths=None, zero_based=False, end_exclusive=False, q_num=(1,), q_den=2,
                               cols=DEFAULT_COLS, filter_flag=1796, min_mapq=0):
        """order statistics of the depth per row of `regions` (read as for depth_regions): -> the regions table with bases
        Int64 and min, max and one q_<num>_<den> per quantile appended, Int32 and null where bases is 0.  Quantile num / den
        is element floor((bases - 1) * num / den) of the region's per-base coverage sorted ascending: the default (1,) / 2
        is the lower median."""
        tabs = [_Exported(t) if t is not None else None for t in (reads, prior, lengths, regions)]
        try:
            b = [t.c if t is not None else _Batch(None, None) for t in tabs]
            return _quantiles_call(self, regions, q_num, q_den, lambda *outs: lib().brh_depth_region_quantiles(
                self.h, b[0], b[1], b[2], b[3], _cols(cols), C.c_int(int(bool(zero_based))), C.c_int(int(bool(end_exclusive))),
                C.c_uint32(int(filter_flag)), C.c_uint32(int(min_mapq)), *outs))
        finally:
            for t in tabs:
                if t is not None:
                    t.close()

    def depth_quantize(self, reads, cuts, emit=None, prior=None, lengths=None, zero_based=False, end_exclusive=False, touched_only=False,
                       filter_flag=1796, min_mapq=0):
        """the maximal intervals whose depth stays in one bin (mosdepth --quantize; "the intervals at 10x or more"): bin(v) =
        the number of `cuts` (ascending, at most 31) that are <= v.  emit: the bins to return (None: all); the others still
        separate their neighbours.  -> contig Utf8, start Int64, end Int64 (inclusive; half-open with end_exclusive: mosdepth's
        BED is zero_based + end_exclusive), bin Int32, ordered by (contig, start).  reads / prior / lengths and the domain as for
        depth_regions(); touched_only: only contigs that kept a read."""
        tabs = [_Exported(t) if t is not None else None for t in (reads, prior, lengths)]
        try:
            b = [t.c if t is not None else _Batch(None, None) for t in tabs]
            return _quantize_call(self, cuts, emit, lambda *a: lib().brh_depth_quantize(
                self.h, b[0], b[1], b[2], C.c_int(int(bool(zero_based))), C.c_int(int(bool(end_exclusive))), C.c_int(int(bool(touched_only))),
                C.c_uint32(int(filter_flag)), C.c_uint32(int(min_mapq)), *a))
        finally:
            for t in tabs:
                if t is not None:
                    t.close()

    def depth_dist(self, reads, v_lo=0, n_bins=256, prior=None, lengths=None, zero_based=False, touched_only=False, filter_flag=1796, min_mapq=0):
        """the bases of every contig at each depth (bedtools genomecov, mosdepth's dist): -> contig Utf8, coverage Int32, bases
        Int64, one row per contig and depth with bases > 0, ordered by (contig, coverage).  The depths are v_lo .. v_lo + n_bins
        - 1; the first stands for "v_lo or less", the last for "that or more".  The rest as for depth_quantize()."""
        tabs = [_Exported(t) if t is not None else None for t in (reads, prior, lengths)]
        try:
            b = [t.c if t is not None else _Batch(None, None) for t in tabs]
            return _dist_call(self, lambda *a: lib().brh_depth_dist(
                self.h, b[0], b[1], b[2], C.c_int(int(bool(zero_based))), C.c_int(int(bool(touched_only))),
                C.c_uint32(int(filter_flag)), C.c_uint32(int(min_mapq)), C.c_int32(int(v_lo)), C.c_uint32(int(n_bins)), *a))
        finally:
            for t in tabs:
                if t is not None:
                    t.close()

    def depth_stream(self, lengths=None, filter_flag=1796, min_mapq=0):
        """depth() over a stream of read batches (brh_depth_push): -> DepthStream"""
        return DepthStream(self, lengths, filter_flag, min_mapq)


def _regions_call(session, regions, thresholds, call):
    """the thresholds and the output structs of brh_depth_regions / brh_depth_push_regions -> regions + the summary columns"""
    thr = [int(t) for t in thresholds]
    n = len(thr)
    cthr = (C.c_int32 * max(n, 1))(*thr)
    bases, total = _out(), _out()
    ge, ge_s = (_ArrowArray * max(n, 1))(), (_ArrowSchema * max(n, 1))()
    session._chk(call(cthr, C.c_uint32(n), C.byref(bases[0]), C.byref(bases[1]), C.byref(total[0]), C.byref(total[1]),
                      ge if n else None, ge_s if n else None))
    out = regions.append_column("bases", _import(*bases)).append_column("sum", _import(*total))
    for j, t in enumerate(thr):
        out = out.append_column(f"bases_ge_{t}", _import(ge[j], ge_s[j]))
    return out


def _quantiles_call(session, regions, q_num, q_den, call):
    """the fractions and the output structs of brh_depth_region_quantiles / brh_depth_push_region_quantiles -> regions + the columns"""
    qn = [int(q) for q in q_num]
    n = len(qn)
    cq = (C.c_uint32 * max(n, 1))(*qn)
    bases, mn, mx = _out(), _out(), _out()
    q, q_s = (_ArrowArray * max(n, 1))(), (_ArrowSchema * max(n, 1))()
    session._chk(call(cq, C.c_uint32(n), C.c_uint32(int(q_den)), C.byref(bases[0]), C.byref(bases[1]), C.byref(mn[0]), C.byref(mn[1]),
                      C.byref(mx[0]), C.byref(mx[1]), q if n else None, q_s if n else None))
    out = regions.append_column("bases", _import(*bases)).append_column("min", _import(*mn)).append_column("max", _import(*mx))
    for j, t in enumerate(qn):
        out = out.append_column(f"q_{t}_{int(q_den)}", _import(q[j], q_s[j]))
    return out


def _quantize_call(session, cuts, emit, call):
    """the cuts, the emit mask and the output structs of brh_depth_quantize / brh_depth_push_quantize -> the interval table"""
    c = [int(x) for x in cuts]
    n = len(c)
    if emit is None:
        mask = (1 << (n + 1)) - 1 if n < 32 else 0xFFFFFFFF
    elif isinstance(emit, int):
        mask = emit
    else:
        mask = 0
        for j in emit:
            mask |= 1 << int(j)
    if mask >> 32:
        raise BioRangesError("depth_quantize() emit names a bin above 31")
    ccuts = (C.c_int32 * max(n, 1))(*c)
    outs = [_out() for _ in range(4)]
    session._chk(call(ccuts, C.c_uint32(n), C.c_uint32(mask), *[C.byref(x) for pair in outs for x in pair]))
    return pa.table([_import(*o) for o in outs], names=["contig", "start", "end", "bin"])


def _dist_call(session, call):
    outs = [_out() for _ in range(3)]
    session._chk(call(*[C.byref(x) for pair in outs for x in pair]))
    return pa.table([_import(*o) for o in outs], names=["contig", "coverage", "bases"])


class DepthStream:
    """brh_depth_push: read tables pushed one by one, each accumulated into a depth profile on the device; finish() gives the
    table Session.depth() gives for all of them together, finish_per_base() the tables of Session.depth_per_base().  Also a
    context manager; close() is run when the object is dropped."""

    def __init__(self, session, lengths=None, filter_flag=1796, min_mapq=0):
        self.session = session
        self.h = C.c_void_p()
        L = _Exported(lengths) if lengths is not None else None
        try:
            session._chk(lib().brh_depth_push_open(session.h, L.c if L is not None else _Batch(None, None), C.c_uint32(int(filter_flag)),
                                                   C.c_uint32(int(min_mapq)), C.byref(self.h)))
        finally:
            if L is not None:
                L.close()

    def push(self, table):
        T = _Exported(table)
        try:
            self.session._chk(lib().brh_depth_push_batch(self.h, T.c))
        finally:
            T.close()

    def depth_regions(self, regions, zero_based=False, end_exclusive=False, thresholds=(), cols=DEFAULT_COLS):
        """Session.depth_regions over everything pushed so far; the stream stays open"""
        R = _Exported(regions)
        try:
            return _regions_call(self.session, regions, thresholds, lambda *outs: lib().brh_depth_push_regions(
                self.h, R.c, _cols(cols), C.c_int(int(bool(zero_based))), C.c_int(int(bool(end_exclusive))), *outs))
        finally:
            R.close()

    def depth_region_quantiles(self, regions, zero_based=False, end_exclusive=False, q_num=(1,), q_den=2, cols=DEFAULT_COLS):
        """Session.depth_region_quantiles over everything pushed so far; the stream stays open"""
        R = _Exported(regions)
        try:
            return _quantiles_call(self.session, regions, q_num, q_den, lambda *outs: lib().brh_depth_push_region_quantiles(
                self.h, R.c, _cols(cols), C.c_int(int(bool(zero_based))), C.c_int(int(bool(end_exclusive))), *outs))
        finally:
            R.close()

    def depth_quantize(self, cuts, emit=None, zero_based=False, end_exclusive=False, touched_only=False):
        """Session.depth_quantize over everything pushed so far; the stream stays open"""
        return _quantize_call(self.session, cuts, emit, lambda *a: lib().brh_depth_push_quantize(
            self.h, C.c_int(int(bool(zero_based))), C.c_int(int(bool(end_exclusive))), C.c_int(int(bool(touched_only))), *a))

    def depth_dist(self, v_lo=0, n_bins=256, zero_based=False, touched_only=False):
        """Session.depth_dist over everything pushed so far; the stream stays open"""
        return _dist_call(self.session, lambda *a: lib().brh_depth_push_dist(
            self.h, C.c_int(int(bool(zero_based))), C.c_int(int(bool(touched_only))), C.c_int32(int(v_lo)), C.c_uint32(int(n_bins)), *a))

    def finish(self):
        """-> contig Utf8, pos_start Int32, pos_end Int32, coverage Int16 of everything pushed"""
        outs = [_out() for _ in range(4)]
        self.session._chk(lib().brh_depth_push_finish(self.h, *[C.byref(x) for pair in outs for x in pair]))
        return pa.table([_import(*o) for o in outs], names=["contig", "pos_start", "pos_end", "coverage"])

    def finish_per_base(self, zero_based=False, batch_rows=8192):
        """a generator of tables (contig Utf8, pos Int32, coverage Int16) like Session.depth_per_base; the stream is finished
        on the first next()"""
        h = C.c_void_p()
        self.session._chk(lib().brh_depth_push_finish_per_base(self.h, C.c_int(int(bool(zero_based))), C.byref(h)))
        try:
            while True:
                outs = [_out() for _ in range(3)]
                done = C.c_int(0)
                self.session._chk(lib().brh_depth_per_base_next(h, C.c_uint64(int(batch_rows)), C.byref(done), *[C.byref(x) for pair in outs for x in pair]))
                if done.value:
                    return
                yield pa.table([_import(*o) for o in outs], names=["contig", "pos", "coverage"])
        finally:
            lib().brh_depth_per_base_close(h)

    def close(self):
        if self.h:
            lib().brh_depth_push_close(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class JoinStream:
    """brh_join_stream: the build side indexed once, probe RecordBatches pushed one by one and coalesced into
    groups before they go to the GPU.  push()/finish() return the results that became ready, each a dict
    first_batch, n_batches, group_done, build_idx, probe_idx (rows counted over the group's concatenated batches),
    batch_offsets."""

    JOIN_TYPES = {"inner": 0, "right_semi": 1, "right_anti": 2, "nearest": 3, "left_semi": 4, "left_anti": 5, "left": 6, "right": 7, "full": 8}

    def __init__(self, session, build, cols_build, cols_probe, strict_predicate, coalesce_rows, join_type="inner", max_output_rows=0):
        self.session = session
        budget = (1 << 64) - 1 if max_output_rows == "env" else int(max_output_rows)
        self.h = C.c_void_p()
        B = _Exported(build)
        try:
            session._chk(lib().brh_join_stream_open(session.h, B.c, _cols(cols_build), _cols(cols_probe), C.c_int(int(strict_predicate)),
                                                    C.c_uint64(int(coalesce_rows)), C.c_int(self.JOIN_TYPES[join_type]), C.c_uint64(budget),
                                                    C.byref(self.h)))
        finally:
            B.close()

    def _drain(self, n):
        out = []
        for _ in range(n):
            first, nb, done = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
            (ba, bs), (pa_, ps), (oa, os_) = _out(), _out(), _out()
            self.session._chk(lib().brh_join_stream_next(self.h, C.byref(first), C.byref(nb), C.byref(done), C.byref(ba), C.byref(bs),
                                                         C.byref(pa_), C.byref(ps), C.byref(oa), C.byref(os_)))
            out.append({"first_batch": first.value, "n_batches": nb.value, "group_done": bool(done.value), "build_idx": _import(ba, bs),
                        "probe_idx": _import(pa_, ps), "batch_offsets": _import(oa, os_)})
        return out

    def push(self, batch):
        P = _Exported(batch if isinstance(batch, pa.Table) else pa.Table.from_batches([batch]))
        n = C.c_int(0)
        try:
            self.session._chk(lib().brh_join_stream_push(self.h, P.c, C.byref(n)))
        finally:
            P.close()
        return self._drain(n.value)

    def finish(self):
        n = C.c_int(0)
        self.session._chk(lib().brh_join_stream_finish(self.h, C.byref(n)))
        return self._drain(n.value)

    def close(self):
        if self.h:
            lib().brh_join_stream_close(self.h)
            self.h = C.c_void_p()


def check_position_column(table, column, as_i64=False):
    """PosArray::resolve / resolve_i64 checks alone (no GPU): returns None or the error text."""
    T = _Exported(table)
    buf = C.create_string_buffer(512)
    try:
        rc = lib().brh_check_position_column(None, T.c, column.encode(), C.c_int(int(as_i64)), buf, C.c_int(512))
    finally:
        T.close()
    return None if rc == 0 else buf.value.decode()


def check_contig_column(table, column):
    """ContigArray checks alone (no GPU): Utf8 / LargeUtf8 / Utf8View (NULL contigs only fail under
    BIO_STRICT_NULL_CONTIGS=1 / a strict session); returns None or the error text."""
    T = _Exported(table)
    buf = C.create_string_buffer(512)
    try:
        rc = lib().brh_check_contig_column(None, T.c, column.encode(), buf, C.c_int(512))
    finally:
        T.close()
    return None if rc == 0 else buf.value.decode()
