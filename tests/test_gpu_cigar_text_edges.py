"""-m gpu: ivx_cigar_parse (csrc/ivx_cigar.hip) bit-exact against the byte-loop restatement (tests/cigar_text_oracle.py),
every case with numpy arrays (IVX_MEM_HOST) and with torch device tensors (IVX_MEM_DEVICE).

The kernel's constants: a thread owns B = 16 bytes (one 16-byte load), a wavefront 64 * B = 1024, a workgroup's tile is
T = 4096 bytes; one workgroup scans up to 4096 tile states serially, beyond 4096 tiles they get a scan level of their own.
Threads sit on the 16-byte aligned grid under the text, so with an aligned first byte (offset 0 of a fresh buffer) the
edges below are thread, wavefront and tile edges; the sliced and misaligned cases shift the text against that grid."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cigar_text_oracle as cto  # noqa: E402
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

B, W, T = pyivx.CIGAR_B, 64 * pyivx.CIGAR_B, pyivx.CIGAR_TILE
assert (B, W, T) == (16, 1024, 4096)


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


def dev(a, shift=0):
    """a numpy array on the device; shift: that many bytes off a fresh (aligned) buffer"""
    import torch
    a = np.array(a)                                      # (a writable copy: np.frombuffer gives read-only arrays)
    if a.dtype == np.uint8:
        buf = torch.empty(len(a) + shift, dtype=torch.uint8, device="cuda:0")
        buf[:shift] = ord("M")
        buf[shift:] = torch.from_numpy(a).to("cuda:0")
        out = buf[shift:]
        assert out.data_ptr() % 16 == shift % 16
        return out
    return torch.from_numpy(a).to("cuda:0")


def parse_both(ctx, off, text, shift=0):
    """(offsets, ops) through both memory modes (asserted identical)"""
    ho, hp = ctx.cigar_parse(off, text)
    do, dp = ctx.cigar_parse(dev(off), dev(text, shift))
    do, dp = do.cpu().numpy(), dp.cpu().numpy().view(np.uint32)
    assert ho.dtype == np.int32 and hp.dtype == np.uint32
    assert np.array_equal(ho, do) and np.array_equal(hp, dp)
    return ho, hp


def check(ctx, strings, large=False, first=0, shift=0, want=None):
    off, text = cto.text_column(strings, large=large, first=first, pad=b"M")
    text = np.r_[text, np.frombuffer(b"9M7", np.uint8)]              # bytes after the last offset are not the column's
    wo, wp = cto.parse_reads(strings) if want is None else want
    go, gp = parse_both(ctx, off, text, shift)
    assert np.array_equal(go, wo)
    assert np.array_equal(gp, wp)
    return go, gp


def tokens(rng, n_bytes, other=0.25):
    """n_bytes of tokens: up to 6 digits (always packable), then an op letter or, with probability `other`, any other byte"""
    out = bytearray()
    while len(out) < n_bytes:
        nd = int(rng.integers(0, 7))
        out += b"".join(bytes([48 + int(d)]) for d in rng.integers(0, 10, nd))
        if rng.random() < other:
            c = int(rng.integers(0, 256))
            out.append(c if not 48 <= c <= 57 else 42)
        else:
            out.append(cto.LETTERS[int(rng.integers(0, 9))])
    return bytes(out[:n_bytes])


def cut(raw, cuts):
    cuts = [0] + sorted(cuts) + [len(raw)]
    return [raw[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


# ------------------------------------------------------------------------------------------------ sizes and straddles
@pytest.mark.parametrize("n", [0, 1, B - 1, B, B + 1, W - 1, W, W + 1, T - 1, T, T + 1, 3 * T + 5])
def test_total_text_sizes(ctx, n):
    rng = np.random.default_rng(n)
    raw = tokens(rng, n)
    check(ctx, [raw])                                                            # one read
    k = min(n, 40)
    check(ctx, cut(raw, rng.integers(0, n + 1, k).tolist()))                     # random reads, some empty
    check(ctx, [raw[i:i + 1] for i in range(n)])                                 # one-byte reads


@pytest.mark.parametrize("e", [B, W, T, 2 * T])
def test_digit_run_and_read_boundary_straddle(ctx, e):
    fill = b"1M" * ((e - 2) // 2)
    assert len(fill) == e - 2
    # a digit run over bytes e-1 | e, inside one read
    go, gp = check(ctx, [fill + b"123456M2D"])
    assert gp[-2:].tolist() == [(123456 << 4) | 0, (2 << 4) | 2]
    # a read boundary at e-1 | e inside a digit run: the left digits are dropped, the right read starts over
    go, gp = check(ctx, [fill + b"12", b"3456M"])
    assert gp[-1] == (3456 << 4) and go.tolist() == [0, 4 * (len(gp) - 1), 4 * len(gp)]
    # the same with the boundary one byte to either side, and with the right read starting with a letter
    check(ctx, [fill + b"1", b"23456M"])
    check(ctx, [fill + b"123", b"456M"])
    go, gp = check(ctx, [fill + b"12", b"M3456X"])
    assert gp[-2:].tolist() == [0, (3456 << 4) | 8]


def test_digit_run_longer_than_a_tile(ctx):
    z = b"0" * 5000
    go, gp = check(ctx, [b"3S" + z + b"7M", z + b"12=", b"1" + z[:20] + b"M"])
    assert gp.tolist() == [(3 << 4) | 4, (7 << 4) | 0, (12 << 4) | 7, 0]         # 10^20 >= 2^32 parses to 0
    # ending in a tenth significant digit: 2^32 and above parse to 0, below that the op cannot be packed
    go, gp = check(ctx, [z + b"4294967296M", z + b"9999999999D"])
    assert gp.tolist() == [0, 2]
    off, text = cto.text_column([b"5M", z + b"1000000000M"])
    for a, b in ((off, text), (dev(off), dev(text))):
        with pytest.raises(pyivx.IvxError) as ei:
            ctx.cigar_parse(a, b)
        assert ei.value.status == pyivx.ERR_INVALID and "2^28" in str(ei.value) and "read 1" in str(ei.value)


def test_one_read_over_several_tiles(ctx):
    rng = np.random.default_rng(9)
    n = 20_000
    ops = ((rng.integers(0, 3000, n) << 4) | rng.integers(0, 9, n)).astype(np.uint32)
    s = cto.render_ops(ops)
    assert len(s) > 10 * T
    go, gp = check(ctx, [s])
    assert np.array_equal(gp, ops) and go.tolist() == [0, 4 * n]
    go, gp = check(ctx, [b"", s, b"*", s[:777]])


def test_many_one_byte_reads_in_one_thread(ctx):
    check(ctx, [b"*", b"M"] * 20)
    check(ctx, [b"M"] * 33)
    check(ctx, [b"*"] * 50)
    check(ctx, [b"7"] * 17 + [b"M"] + [b"", b"=", b"", b"", b"X"] * 7)


@pytest.mark.parametrize("where", ["front", "middle", "end", "all"])
def test_runs_of_empty_reads(ctx, where):
    e = [b""] * 5000
    a, b = [b"3M2D", b"10M5"], [b"8M", b"*", b"1S"]
    strings = {"front": e + a + b, "middle": a + e + b, "end": a + b + e, "all": e}[where]
    go, gp = check(ctx, strings)
    if where == "all":
        assert len(gp) == 0 and not go.any()


def test_trailing_digits_do_not_reach_the_next_read(ctx):
    go, gp = check(ctx, [b"10M5", b"3M"])
    assert gp.tolist() == [160, 48] and go.tolist() == [0, 4, 8]
    go, gp = check(ctx, [b"12", b"", b"34", b"M", b"5", b"6I"])
    assert gp.tolist() == [0, (6 << 4) | 1] and go.tolist() == [0, 0, 0, 0, 4, 4, 8]


# ------------------------------------------------------------------------------------------ slices, alignment, offsets
@pytest.mark.parametrize("first", [1, 3, 15, 16, 17])
@pytest.mark.parametrize("large", [False, True])
def test_sliced_columns(ctx, first, large):
    rng = np.random.default_rng(first)
    raw = tokens(rng, 3 * W + 7)
    check(ctx, cut(raw, rng.integers(0, len(raw), 60).tolist()), large=large, first=first)
    check(ctx, [b"", b""] + cut(raw[:40], [13]), large=large, first=first)


@pytest.mark.parametrize("shift", [1, 5, 8, 15])
def test_misaligned_device_text(ctx, shift):
    rng = np.random.default_rng(shift)
    raw = tokens(rng, T + 3 * B + 1)
    check(ctx, cut(raw, rng.integers(0, len(raw), 50).tolist()), shift=shift)
    check(ctx, [raw[:B - 3]], shift=shift)                                      # no aligned body at all
    check(ctx, [raw[:7]], shift=shift, first=3)


def test_large_offsets(ctx):
    rng = np.random.default_rng(4)
    raw = tokens(rng, 2 * T + 100)
    strings = cut(raw, rng.integers(0, len(raw), 300).tolist())
    a = check(ctx, strings, large=True)
    b = check(ctx, strings, large=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_scan_of_the_tile_states_changes_level(ctx):
    """4 * 1024 + 1 tiles: the tile states no longer fit one workgroup's serial scan.  The text repeats one period of 37 bytes
    (two reads), so every phase of the period against thread, wavefront and tile edges occurs"""
    period = [b"12M3I00400D5N", b"6S7H8P90=1X22M77*3M12345"]                     # 13 + 24 bytes; trailing digits dropped
    plen = sum(map(len, period))
    assert plen == 37
    reps = (4 * 1024 * T) // plen + 2
    assert reps * plen > 4 * 1024 * T and (reps * plen + T - 1) // T == 4 * 1024 + 1
    po, pops = cto.parse_reads(period)
    lens = np.tile(np.array([len(s) for s in period], np.int64), reps)
    off = np.r_[0, np.cumsum(lens)].astype(np.int32)
    text = np.tile(np.frombuffer(b"".join(period), np.uint8), reps)
    want_ops = np.tile(pops, reps)
    per_read = np.tile(np.diff(po.astype(np.int64)), reps)
    want_off = np.r_[0, np.cumsum(per_read)].astype(np.int32)
    go, gp = parse_both(ctx, off, text)
    assert np.array_equal(gp, want_ops) and np.array_equal(go, want_off)


# ---------------------------------------------------------------------------------------------------------------- fuzz
def fuzz_bytes(rng, n):
    kind = rng.random(n)
    out = np.where(kind < 0.45, rng.integers(48, 58, n),
                   np.where(kind < 0.85, np.frombuffer(cto.LETTERS, np.uint8)[rng.integers(0, 9, n)], rng.integers(0, 256, n)))
    return out.astype(np.uint8).tobytes()


@pytest.mark.parametrize("seed", range(8))
def test_fuzz_all_byte_values(ctx, seed):
    rng = np.random.default_rng(1000 + seed)
    strings = []
    for _ in range(400):
        r = rng.random()
        strings.append(b"" if r < 0.1 else fuzz_bytes(rng, int(rng.integers(1, 60 if r < 0.9 else 700))))
    off, text = cto.text_column(strings, large=bool(seed & 1), first=seed)
    assert len(np.unique(text)) == 256
    bad = [i for i, s in enumerate(strings) if any(ln > cto.MAX_PACKED_LEN for ln, _ in cto.tokenize(s))]
    if bad:
        # a run of 9 or 10 digits before an op letter: the lowest such read is named, in both modes; then without those reads
        for a, b in ((off, text), (dev(off), dev(text))):
            with pytest.raises(pyivx.IvxError) as ei:
                ctx.cigar_parse(a, b)
            assert ei.value.status == pyivx.ERR_INVALID and f"(read {bad[0]})" in str(ei.value)
        strings = [b"" if i in bad else s for i, s in enumerate(strings)]
        off, text = cto.text_column(strings, large=bool(seed & 1), first=seed)
    assert len(bad) < 40
    want = cto.parse_reads(strings)
    go, gp = parse_both(ctx, off, text)
    assert np.array_equal(go, want[0]) and np.array_equal(gp, want[1])


# -------------------------------------------------------------------------------------------------------------- errors
def raw_parse(ctx, off, text, out_off, out_ops, cap):
    n = C.c_uint64(12345)
    st = pyivx.lib().ivx_cigar_parse(ctx.h, C.c_int(pyivx.MEM_HOST), C.c_int(int(off.dtype == np.int64)), pyivx._ptr(off), pyivx._ptr(text),
                                     C.c_uint64(len(off) - 1), pyivx._ptr(out_off), pyivx._ptr(out_ops), C.c_uint64(cap), C.byref(n))
    return st, n.value


def still_works(ctx):
    go, gp = ctx.cigar_parse(*cto.text_column([b"5M3D5M", b"*"]))
    assert gp.tolist() == [80, 50, 80] and go.tolist() == [0, 12, 12]


@pytest.mark.parametrize("large", [False, True])
def test_bad_offsets_are_refused(ctx, large):
    dt = np.int64 if large else np.int32
    text = np.frombuffer(b"5M3D5M10M", np.uint8)
    for bad in ([0, 6, 3, 9], [-1, 3, 6], [3, 0], [0, 9, -2]):
        off = np.array(bad, dt)
        for a, b in ((off, text), (dev(off), dev(text))):
            with pytest.raises(pyivx.IvxError) as ei:
                ctx.cigar_parse(a, b)
            assert ei.value.status == pyivx.ERR_INVALID and "offsets" in str(ei.value)
        still_works(ctx)


def test_op_length_limits(ctx):
    go, gp = check(ctx, [b"268435455M", b"0268435455N"])
    assert gp.tolist() == [(268435455 << 4), (268435455 << 4) | 3]
    for s in (b"268435456M", b"4294967295M", b"268435456S", b"00004294967295H"):
        off, text = cto.text_column([b"1M", b"", s, b"268435456M"])
        for a, b in ((off, text), (dev(off), dev(text))):
            with pytest.raises(pyivx.IvxError) as ei:
                ctx.cigar_parse(a, b)
            assert ei.value.status == pyivx.ERR_INVALID and "(read 2)" in str(ei.value)
        st, n = raw_parse(ctx, off, text, None, None, 0)                         # a counting call checks too
        assert st == pyivx.ERR_INVALID
        still_works(ctx)
    go, gp = check(ctx, [b"4294967296M", b"99999999999X", b"268435456B1M", b"4294967295*"])   # >= 2^32 is 0; no op, no check
    assert gp.tolist() == [0, 8, 16]


def test_capacity_protocol(ctx):
    off, text = cto.text_column([b"5M3D5M", b"", b"2S8="])
    st, n = raw_parse(ctx, off, text, None, None, 0)
    assert (st, n) == (pyivx.OK, 5)
    out_off = np.full(4, -7, np.int32)
    out_ops = np.full(8, 0xDEADBEEF, np.uint32)
    st, n = raw_parse(ctx, off, text, out_off, out_ops, 4)
    assert (st, n) == (pyivx.ERR_CAPACITY, 5)
    assert (out_ops == 0xDEADBEEF).all()                                         # no op is written
    assert out_off.tolist() == [0, 12, 12, 20]                                   # the offsets are, whenever they are given
    st, n = raw_parse(ctx, off, text, out_off, out_ops, 5)
    assert (st, n) == (pyivx.OK, 5)
    assert out_ops[:5].tolist() == [80, 50, 80, (2 << 4) | 4, (8 << 4) | 7] and (out_ops[5:] == 0xDEADBEEF).all()
    st, n = raw_parse(ctx, off, text, out_off, None, 0)                          # offsets alone
    assert (st, n) == (pyivx.OK, 5)
    st, n = raw_parse(ctx, np.zeros(1, np.int32), text, None, None, 0)           # n_reads = 0
    assert (st, n) == (pyivx.OK, 0)
    still_works(ctx)
