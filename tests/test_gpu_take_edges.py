"""-m gpu: the payload take kernels (csrc/ivx_take.hip) at the sizes where their loops, buffers and limits change,
exact against pyarrow's take (views: take on the column cast to string / binary, cast back) and numpy's cumsum.

Thresholds, from the launch code in ivx_take.hip:
  k_take_bytes / k_view_copy  one 64-row group per wavefront, grid = min(groups / 4, 4096) blocks of 4 wavefronts:
                              a wavefront makes a second trip (and reuses its LDS rows) only when n > 4 * 4096 * 64 = 1 048 576
  k_take_bits                 one output byte per thread, grid = bytes / 1024 blocks of 256 threads: a second byte per thread
                              from n > 2048, more than one block from n > 8192
  views                       len <= 12 stays inline, len > 12 is gathered into ONE buffer and renamed (buffer 0, new offset)
  Utf8                        2^31 - 1 bytes is the last total that int32 offsets hold; views: the last that one buffer holds
"""
import ctypes as C
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import bio_ranges as br  # noqa: E402
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

NULL = pyivx.NULL_IDX
KINDS = {"utf8": pa.string(), "large": pa.large_string(), "view": pa.string_view()}


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sess():
    s = br.Session(0)
    yield s
    s.close()


# ---- plumbing: Arrow column -> the buffers the C ABI takes, and back

def _ia(idx):
    return pa.array(idx, pa.uint32(), mask=idx == NULL)


def _valid_bits(col):
    """validity bitmap at bit offset 0 (None without nulls)"""
    if col.null_count == 0:
        return None
    return np.packbits(col.is_valid().to_numpy(zero_copy_only=False), bitorder="little")


def _vbuf(valid):
    return pa.py_buffer(np.packbits(np.asarray(valid, np.uint8), bitorder="little"))


def _dev(a):
    import torch
    if a is None:
        return None
    a = np.array(a)                                                  # (a writable copy: Arrow's buffers are read-only)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _host(*ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def _utf8_parts(col):
    odt = np.int64 if col.type in (pa.large_string(), pa.large_binary()) else np.int32
    _, ob, db = col.buffers()
    off = np.frombuffer(ob, odt)[col.offset: col.offset + len(col) + 1]
    data = np.frombuffer(db, np.uint8) if db is not None else np.zeros(0, np.uint8)
    return off, data, _valid_bits(col)


def _view_parts(col):
    bufs = col.buffers()
    views = np.frombuffer(bufs[1], np.uint8).reshape(-1, 16)[col.offset: col.offset + len(col)]
    return views, [np.frombuffer(b, np.uint8) for b in bufs[2:]], _valid_bits(col)


def _take_utf8(ctx, col, idx, mem="host"):
    off, data, bits = _utf8_parts(col)
    if mem == "device":
        out = ctx.take_utf8(_dev(off), _dev(data), _dev(idx), src_valid_bits=_dev(bits))
        ctx.synchronize()                                            # device calls may return with kernels in flight
        return _host(*out)
    return ctx.take_utf8(off, data, idx, src_valid_bits=bits)


def _take_view(ctx, col, idx, mem="host"):
    views, bufs, bits = _view_parts(col)
    if mem == "device":
        out = ctx.take_view(_dev(views), [_dev(b) for b in bufs], _dev(idx), src_valid_bits=_dev(bits))
        ctx.synchronize()
        return _host(*out)
    return ctx.take_view(views, bufs, idx, src_valid_bits=bits)


def _want(col, idx):
    """the reference: pyarrow's take; this pyarrow has no take kernel for views, so those go through string / binary"""
    if col.type in (pa.string_view(), pa.binary_view()):
        flat = pa.binary() if col.type == pa.binary_view() else pa.string()
        return pc.take(col.cast(flat), _ia(idx)).cast(col.type)
    return pc.take(col, _ia(idx))


def _check_utf8(col, idx, got, want=None):
    """offsets, bytes and validity byte-equal to arrow's (the sources here keep null slots empty, as arrow's output does)"""
    out_off, out_data, valid = got
    n = len(idx)
    want = _want(col, idx) if want is None else want
    assert len(out_off) == n + 1 and out_off.dtype == (np.int64 if col.type == pa.large_string() else np.int32)
    assert ((np.asarray(valid) != 0) == want.is_valid().to_numpy(zero_copy_only=False)).all()
    arr =pa.Array.from_buffers(col.type, n, [_vbuf(valid), pa.py_buffer(np.ascontiguousarray(out_off)), pa.py_buffer(np.ascontiguousarray(out_data))])
    arr.validate(full=True)
    assert arr.equals(want)
    w_off, w_data, _ = _utf8_parts(want)
    assert (out_off == w_off - w_off[0]).all()
    assert len(out_data) == int(w_off[-1] - w_off[0]) and (out_data == w_data[int(w_off[0]): int(w_off[-1])]).all()


def _view_contract(col, idx, out_views, data_bytes):
    """include/ivx.h: short views are the source's 16 bytes; long ones keep length and prefix word, name buffer 0 and sit at
    the exclusive sum of the long lengths; data_bytes is that sum"""
    n = len(idx)
    ov = np.ascontiguousarray(out_views, np.uint8).reshape(n, 16).view(np.uint32)
    sv = np.frombuffer(col.buffers()[1], np.uint32).reshape(-1, 4)[col.offset: col.offset + len(col)]
    null = idx == NULL
    taken = sv[np.where(null, 0, idx).astype(np.int64)].copy()
    taken[null] = 0
    long = taken[:, 0] > 12
    lens = np.where(long, taken[:, 0], 0).astype(np.uint64)
    pos = np.cumsum(lens) - lens
    assert (ov[~long] == taken[~long]).all()
    assert (ov[long, 0] == taken[long, 0]).all() and (ov[long, 1] == taken[long, 1]).all()
    assert (ov[long, 2] == 0).all() and (ov[long, 3] == pos[long]).all()
    assert data_bytes == int(lens.sum())


def _check_view(col, idx, got, want=None):
    out_views, out_data, valid = got
    n = len(idx)
    want = _want(col, idx) if want is None else want
    out_views = np.ascontiguousarray(out_views, np.uint8).reshape(n, 16)
    arr = pa.Array.from_buffers(col.type, n, [_vbuf(valid), pa.py_buffer(out_views), pa.py_buffer(np.ascontiguousarray(out_data))])
    arr.validate(full=True)
    assert arr.equals(want)
    assert ((np.asarray(valid) != 0) == want.is_valid().to_numpy(zero_copy_only=False)).all()
    _view_contract(col, idx, out_views, len(out_data))


def _take_and_check(ctx, col, idx, mem="host", want=None):
    if col.type in (pa.string_view(), pa.binary_view()):
        _check_view(col, idx, _take_view(ctx, col, idx, mem), want)
    else:
        _check_utf8(col, idx, _take_utf8(ctx, col, idx, mem), want)


# ---- A. second trip of the wavefront loops: n = 4 * 4096 * 64 + 785 (16 384 groups, then 12 whole groups and 17 rows)

N_TRIP2 = 4 * 4096 * 64 + 785


@pytest.fixture(scope="module")
def trip2():
    rng = np.random.default_rng(11)
    n_src = 5000
    lens = rng.choice([0, 1, 11, 12, 13, 14, 40], n_src)             # both sides of the views' inline limit
    null = rng.random(n_src) < 0.08
    py = [None if null[i] else (("r%04d|" % i) * 8)[: lens[i]] for i in range(n_src)]
    idx = rng.integers(0, n_src, N_TRIP2).astype(np.uint32)
    idx[::29] = NULL
    cols = {k: pa.array(py, t) for k, t in KINDS.items()}
    want = pc.take(cols["utf8"], _ia(idx))                          # computed once, shared by the six cases
    return cols, idx, {k: want.cast(t) for k, t in KINDS.items()}


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_second_loop_trip(ctx, trip2, kind, mem):
    cols, idx, want = trip2
    assert len(idx) > 4 * 4096 * 64                                  # what puts a second group on a wavefront
    _take_and_check(ctx, cols[kind], idx, mem, want[kind])


@pytest.mark.parametrize("mem", ["host", "device"])
def test_bits_second_byte_and_tail(ctx, mem):
    # n = 3 * 8192 + 5: 3073 output bytes = 4 blocks, up to four bytes per thread, and a last byte with 5 live bits
    rng = np.random.default_rng(12)
    n_src, n = 5000, 8 * 1024 * 3 + 5
    vals = rng.random(n_src) < 0.5
    col = pa.array(vals, pa.bool_(), mask=rng.random(n_src) < 0.10)
    idx = rng.integers(0, n_src, n).astype(np.uint32)
    idx[::29] = NULL
    src_bits, bits = np.packbits(vals, bitorder="little"), _valid_bits(col)
    if mem == "device":
        got = ctx.take_bits(_dev(src_bits), n_src, _dev(idx), src_valid_bits=_dev(bits))
        ctx.synchronize()
        out, valid = _host(*got)
    else:
        out, valid = ctx.take_bits(src_bits, n_src, idx, src_valid_bits=bits)
    want = pc.take(col, _ia(idx))
    assert len(out) == (n + 7) // 8
    assert pa.Array.from_buffers(pa.bool_(), n, [_vbuf(valid), pa.py_buffer(np.ascontiguousarray(out))]).equals(want)
    assert ((valid != 0) == want.is_valid().to_numpy(zero_copy_only=False)).all()
    # every bit, those under nulls and past n too: a null index gives 0, the bits past n stay 0
    exp = np.where(idx == NULL, False, vals[np.where(idx == NULL, 0, idx).astype(np.int64)])
    assert (out == np.packbits(exp, bitorder="little")).all()


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("width", [16, 32])
def test_fixed_wide_matches_arrow(ctx, width, mem):
    # 16- and 32-byte elements (uint4 / two uint4 per thread) against arrow's take of fixed_size_binary; n is odd and
    # spans 98 blocks
    rng = np.random.default_rng(13)
    n_src, n = 5000, 100_003
    src = rng.integers(0, 256, (n_src, width)).astype(np.uint8)
    vb = np.packbits(rng.random(n_src) >= 0.10, bitorder="little")
    col = pa.Array.from_buffers(pa.binary(width), n_src, [pa.py_buffer(vb), pa.py_buffer(src)])
    idx = rng.integers(0, n_src, n).astype(np.uint32)
    idx[::29] = NULL
    if mem == "device":
        out, valid = _host(*ctx.take_fixed(_dev(src), _dev(idx), src_valid_bits=_dev(vb)))
    else:
        out, valid = ctx.take_fixed(src, idx, src_valid_bits=vb)
    want = pc.take(col, _ia(idx))
    assert pa.Array.from_buffers(pa.binary(width), n, [_vbuf(valid), pa.py_buffer(np.ascontiguousarray(out))]).equals(want)
    assert ((valid != 0) == want.is_valid().to_numpy(zero_copy_only=False)).all()
    live = idx != NULL
    assert (out[live] == src[idx[live]]).all() and (out[~live] == 0).all()


# ---- B. group shapes of the cooperative byte copy (64 rows per wavefront, bisect over the rows' first-byte positions)

E_, N_, ABC, BIG = 0, NULL, 2, 3                                     # rows of the source below: "", a null index, "abc", 70 000 bytes


def W(length):
    return 3 + length                                                # the source row of that many bytes, 1..40


def _shape_source(typ):
    big = "".join(chr(33 + (k * 7 + k // 90) % 90) for k in range(70_000))
    py = ["", None, "abc", big] + [("w%02d-" % m + "abcdefghijklmnopqrstuvwxyz0123456789" * 2)[:m] for m in range(1, 41)]
    return pa.array(py, typ)


def _mixed(n):
    """n rows of empties, nulls and strings of 1..40 bytes that end in a non-empty string"""
    rows = [(E_, N_, W(1 + i % 40))[i % 3] for i in range(n)]
    if n:
        rows[-1] = W(13)
    return rows


SHAPES = {
    # a group of 0 bytes (total == 0: its t loop makes no trip) between two groups that have bytes
    "bytes_empty_bytes": [W(1 + i % 40) for i in range(64)] + [(E_, N_)[i % 2] for i in range(64)] + [W(40 - i % 40) for i in range(64)],
    # one string of 70 000 bytes alone in its group: 1094 trips of the t loop, all with the same bisect answer
    "big_at_lane0": [W(7)] * 64 + [BIG] + [E_] * 63 + [W(9)] * 64,
    "big_at_lane63": [W(7)] * 64 + [E_] * 63 + [BIG] + [W(9)] * 64,
    # rows that share s_ex with the string after them: the bisect has to take the LAST row whose first byte is <= t
    "tie_rule": [E_, N_, E_, ABC] + [E_] * 5,
    "all_null": [N_] * 200,                                          # total == 0: no copy kernel is launched
    "empty": [],
}
SHAPES.update({"n%d" % n: _mixed(n) for n in (1, 63, 64, 65, 127, 128, 129)})   # the last group has 1, 63 or 64 live lanes


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_group_shapes(ctx, kind, shape):
    col = _shape_source(KINDS[kind])
    _take_and_check(ctx, col, np.array(SHAPES[shape], np.uint32))


# ---- C. views whose bytes live in data buffers 0..5, inline and gathered lengths mixed, source sliced by 3

def _multi_buffer_views(typ):
    def s(i):
        if i % 11 == 0:
            return None
        m = i % 13 if i % 7 == 0 else 40                             # 0..12 inline, 40 gathered
        return (("%05d/" % i) * 7)[:m]
    head = pa.array([s(i) for i in range(5600)], pa.string_view())   # pyarrow opens a new data buffer every 32 760 bytes
    tail = pa.array([None if i % 9 == 0 else ("t%03d" % i) * (1 + i % 6) for i in range(300)], pa.string_view())
    col = pa.concat_arrays([head, tail])                             # keeps both sets of buffers: the tail's is one more
    if typ == pa.binary_view():
        col = pa.Array.from_buffers(typ, len(col), col.buffers())
    return col.slice(3)


def _multi_buffer_idx(col):
    n_src = len(col)
    idx = ((np.arange(3000, dtype=np.uint64) * 37) % n_src).astype(np.uint32)
    idx[::13] = NULL
    sv = np.frombuffer(col.buffers()[1], np.uint32).reshape(-1, 4)[col.offset: col.offset + n_src]
    live = sv[idx[idx != NULL].astype(np.int64)]
    assert len(col.buffers()) - 2 >= 6 and set(live[live[:, 0] > 12, 2].tolist()) >= set(range(6))      # the input, not the output
    assert (live[:, 0] <= 12).any() and (live[:, 0] == 12).any() and (live[:, 0] > 12).any()
    return idx


@pytest.mark.parametrize("path", ["host_api", "pyivx_host", "pyivx_device"])
@pytest.mark.parametrize("typ", [pa.string_view(), pa.binary_view()], ids=str)
def test_views_across_data_buffers(ctx, sess, typ, path):
    col = _multi_buffer_views(typ)
    idx = _multi_buffer_idx(col)
    if path != "host_api":
        _check_view(col, idx, _take_view(ctx, col, idx, "device" if path == "pyivx_device" else "host"))
        return
    got = sess.take(col, _ia(idx))                                   # brh_take: host staging of the six buffers in one area
    got.validate(full=True)
    assert got.type == typ and got.equals(_want(col, idx))
    bufs = got.buffers()
    views = np.frombuffer(bufs[1], np.uint8).reshape(-1, 16)[got.offset: got.offset + len(got)]
    _view_contract(col, idx, views, bufs[2].size if len(bufs) > 2 and bufs[2] is not None else 0)


# ---- D. size limits, with sizing calls only (out_data = NULL, data_cap = 0): n + 1 lengths are scanned, no byte moves

def _raw_utf8(ctx, mem, large, off, data, idx, out_off, out_data, cap, out_valid, svb=None):
    n_src = (int(off.numel()) if pyivx._is_torch(off) else len(off)) - 1
    nbytes = int(data.numel()) if pyivx._is_torch(data) else len(data)
    n = int(idx.numel()) if pyivx._is_torch(idx) else len(idx)
    need = C.c_uint64(0)
    p = pyivx._ptr
    st = pyivx.lib().ivx_take_utf8(ctx.h, C.c_int(mem), C.c_int(int(large)), p(off), p(data), C.c_uint64(n_src), C.c_uint64(nbytes), p(svb),
                                   p(idx), C.c_uint64(n), p(out_off), p(out_data), C.c_uint64(cap), C.byref(need), p(out_valid))
    return st, need.value


def _raw_view_size(ctx, col, idx):
    views, bufs, _ = _view_parts(col)
    views = np.ascontiguousarray(views)
    table = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
    sizes = (C.c_uint64 * len(bufs))(*[len(b) for b in bufs])
    need = C.c_uint64(0)
    st = pyivx.lib().ivx_take_view(ctx.h, C.c_int(pyivx.MEM_HOST), pyivx._ptr(views), table, sizes, C.c_uint32(len(bufs)), C.c_uint64(len(col)), None,
                                   pyivx._ptr(idx), C.c_uint64(len(idx)), None, None, C.c_uint64(0), C.byref(need), None)
    return st, need.value


LIMIT_LENS = [4096, 4095, 5000]


def _limit_source(typ):
    return pa.array([chr(65 + k) * m for k, m in enumerate(LIMIT_LENS)], typ)


def test_limit_two_gib_refused(ctx):
    # 524 288 * 4096 = 2^31 bytes: one more than int32 offsets, or one view data buffer, can hold
    idx = np.zeros(524_288, np.uint32)
    off, data, _ = _utf8_parts(_limit_source(pa.string()))
    out_off = np.empty(len(idx) + 1, np.int32)
    st, need = _raw_utf8(ctx, pyivx.MEM_HOST, False, off, data, idx, out_off, None, 0, None)
    assert st == pyivx.ERR_INVALID and need == 2 ** 31
    assert "overflow" in pyivx.lib().ivx_last_error(ctx.h).decode()
    st, _ = _raw_view_size(ctx, _limit_source(pa.string_view()), idx)
    assert st == pyivx.ERR_UNSUPPORTED


def test_limit_two_gib_minus_one_accepted(ctx):
    # one index moved to the 4095-byte string: 2^31 - 1, the last total both forms accept
    idx = np.zeros(524_288, np.uint32)
    idx[1234] = 1
    off, data, _ = _utf8_parts(_limit_source(pa.string()))
    out_off = np.full(len(idx) + 1, -7, np.int32)
    st, need = _raw_utf8(ctx, pyivx.MEM_HOST, False, off, data, idx, out_off, None, 0, None)
    assert st == pyivx.OK and need == 2 ** 31 - 1
    want = np.concatenate([[0], np.cumsum(np.array(LIMIT_LENS, np.int64)[idx])])
    assert int(out_off[-1]) == 2 ** 31 - 1 and (out_off == want).all()
    st, need = _raw_view_size(ctx, _limit_source(pa.string_view()), idx)
    assert st == pyivx.OK and need == 2 ** 31 - 1


def test_limit_large_offsets_past_32_bits(ctx):
    # LargeUtf8: 900 000 * 5000 = 4.5e9 > 2^32 bytes, every 1000th index null
    idx = np.full(900_000, 2, np.uint32)
    idx[::1000] = NULL
    off, data, _ = _utf8_parts(_limit_source(pa.large_string()))
    out_off = np.full(len(idx) + 1, -7, np.int64)
    valid = np.full(len(idx), 9, np.uint8)
    st, need = _raw_utf8(ctx, pyivx.MEM_HOST, True, off, data, idx, out_off, None, 0, valid)
    want = np.concatenate([[0], np.cumsum(np.where(idx == NULL, 0, 5000).astype(np.int64))])
    assert want[-1] > 2 ** 32
    assert st == pyivx.OK and need == int(want[-1])
    assert (out_off == want).all() and (valid == (idx != NULL)).all()


# ---- E. the capacity protocol of ivx_take_utf8 (include/ivx.h: out_offsets is written whenever given)

@pytest.mark.parametrize("mem", ["host", "device"])
def test_capacity_protocol(ctx, mem):
    col = pa.array([None if i % 7 == 0 else "g%d" % i * (i % 5) for i in range(60)], pa.string())
    idx = np.array([NULL if i % 11 == 0 else (i * 7) % 60 for i in range(300)], np.uint32)
    want = pc.take(col, _ia(idx))
    w_off, w_data, _ = _utf8_parts(want)
    need0 = int(w_off[-1])
    off, data, bits = _utf8_parts(col)
    conv, back, m = (_dev, lambda t: t.cpu().numpy(), pyivx.MEM_DEVICE) if mem == "device" else (np.array, lambda a: a, pyivx.MEM_HOST)
    off, data, bits, didx = conv(off), conv(data), conv(bits), conv(idx)
    out_off, valid = conv(np.full(len(idx) + 1, -7, np.int32)), conv(np.full(len(idx), 9, np.uint8))
    out_data = conv(np.zeros(need0, np.uint8))
    st, need = _raw_utf8(ctx, m, False, off, data, didx, out_off, out_data, need0 - 1, valid, svb=bits)
    ctx.synchronize()
    assert st == pyivx.ERR_CAPACITY and need == need0
    print("offsets after IVX_ERR_CAPACITY (%s):" % mem, back(out_off)[:6].tolist(), "valid:", back(valid)[:6].tolist())
    assert (back(out_off) == w_off).all()                            # one byte short: the offsets are final all the same
    assert ((back(valid) != 0) == want.is_valid().to_numpy(zero_copy_only=False)).all()
    st, need = _raw_utf8(ctx, m, False, off, data, didx, out_off, out_data, need0, valid, svb=bits)
    ctx.synchronize()
    assert st == pyivx.OK and need == need0
    _check_utf8(col, idx, (back(out_off), back(out_data), back(valid)), want)


def test_capacity_retry_of_the_binding(ctx):
    # every index names the longest string, so 1.5 x the mean source length falls short and pyivx.take_utf8 calls again
    col = pa.array(["s%d" % i for i in range(99)] + ["L" * 1000], pa.string())
    idx = np.full(500, 99, np.uint32)
    off, data, _ = _utf8_parts(col)
    assert int(len(idx) * (len(data) / len(col)) * 1.5) + 64 < 500 * 1000          # the binding's first guess
    _check_utf8(col, idx, _take_utf8(ctx, col, idx))
