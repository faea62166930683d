"""CPU restatement of the text-CIGAR tokeniser for the tests (include/ivx.h ivx_cigar_parse).

The reference (bio-function-pileup) cannot be run here (no Rust toolchain), so parity rests on restatements of its cited
lines that must agree with each other and with the reference's own pinned tables
(tests/golden/pileup_cigar_text_golden.json):

  tokenize        the byte loop of apply_cigar_to_event_list / apply_cigar_to_depth (cigar.rs:92-100, :146-154): every
                  non-digit byte ends a token whose length is `cigar[num_start..i].parse::<u32>()`, 0 on error
  events_direct   the whole of apply_cigar_to_event_list (cigar.rs:141-168) on one read's bytes
  parse_column    tokenize over an Arrow Utf8 column -> the packed (cigar_offsets, cigar_ops) ivx_depth takes
  ident / elem / combine / scan_tokens
                  the capped scan operator of csrc/ivx_cigar.hip, in Python integers, evaluated under any association
                  order; combine_u64 is the same operator in the guarded 64-bit form the kernel computes
"""
import json
import os

import numpy as np

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pileup_cigar_text_golden.json")

U32_MAX = 0xFFFFFFFF
CAP = 1 << 32
LETTERS = b"MIDNSHP=X"                  # BAM codes 0..8
CODE_OF = {c: i for i, c in enumerate(LETTERS)}
MAX_PACKED_LEN = (1 << 28) - 1


def parse_u32(digits):
    """Rust's str::parse::<u32>() on a run of ASCII digits, 0 on its error (empty, or a value above u32::MAX)"""
    digits = bytes(digits).lstrip(b"0")
    if len(digits) == 0:                # no digits, or zeros only
        return 0
    if len(digits) > 10:                # above 2^32 whatever the digits are
        return 0
    v = int(digits)
    return v if v <= U32_MAX else 0


def tokenize(b):
    """one read's bytes -> [(len, code)] of the ops it emits, in order (cigar.rs:146-166 with BAM's codes)"""
    out = []
    num_start = 0
    for i, c in enumerate(b):
        if 48 <= c <= 57:
            continue
        ln = parse_u32(b[num_start:i])
        if c in CODE_OF:
            out.append((ln, CODE_OF[c]))
        num_start = i + 1
    return out


def events_direct(start, b):
    """apply_cigar_to_event_list (cigar.rs:141-168) -> [(position, delta)]"""
    out = []
    ref = start
    num_start = 0
    for i, c in enumerate(b):
        if 48 <= c <= 57:
            continue
        ln = parse_u32(b[num_start:i])
        if c in b"MX=":
            out.append((ref, 1))
            ref = min(ref + ln, U32_MAX)
            out.append((ref, -1))
        elif c in b"DN":
            ref = min(ref + ln, U32_MAX)
        num_start = i + 1
    return out


class PackError(ValueError):
    """an emitted op whose length does not fit 28 bits; .read = the lowest such read"""
    def __init__(self, read):
        super().__init__(f"read {read}")
        self.read = read


def text_column(strings, large=False, first=0, pad=b"#"):
    """[bytes] -> (offsets int32 / int64 [n + 1] starting at `first`, text uint8 with `first` bytes of padding in front)"""
    lens = np.array([len(s) for s in strings], np.int64)
    off = np.zeros(len(strings) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    off += first
    text = np.frombuffer(pad * first + b"".join(strings), np.uint8).copy()
    return off.astype(np.int64 if large else np.int32), text


def reads_of(offsets, text):
    raw = np.asarray(text, np.uint8).tobytes()
    return [raw[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def parse_reads(strings):
    """[bytes] -> (cigar_offsets int32 [n + 1], cigar_ops uint32); PackError for the lowest read with an unpackable op"""
    off = np.zeros(len(strings) + 1, np.int32)
    ops = []
    bad = None
    for i, s in enumerate(strings):
        for ln, code in tokenize(s):
            if ln > MAX_PACKED_LEN:
                bad = i if bad is None else bad
                ln = 0
            ops.append((ln << 4) | code)
        off[i + 1] = 4 * len(ops)
    if bad is not None:
        raise PackError(bad)
    return off, np.array(ops, np.uint32)


def parse_column(offsets, text):
    return parse_reads(reads_of(offsets, text))


def render_ops(ops, rng=None):
    """packed ops -> a CIGAR string; the codes 9..15 (no letter: BAM's 'B' and the unassigned ones, which depth() ignores)
    become bytes that only separate"""
    out = bytearray()
    for w in ops:
        w = int(w)
        ln, code = w >> 4, w & 15
        out += str(ln).encode() if (rng is None or ln or rng.random() < 0.7) else b""
        out += LETTERS[code:code + 1] if code < 9 else b"B*+ Zm\xc3"[code - 9:code - 8]
    return bytes(out)


def render_reads(cigar_offsets, cigar_ops, rng=None):
    """the Binary cigar column of a depth() input -> [bytes], one CIGAR string per read"""
    o = np.asarray(cigar_offsets, np.int64) // 4
    return [render_ops(cigar_ops[o[i]:o[i + 1]], rng) for i in range(len(o) - 1)]


# ---- the scan operator of csrc/ivx_cigar.hip: state (reset, v, p, ops)
def ident():
    return (False, 0, 1, 0)


def elem(c, first):
    """the element of one byte; first = it is its read's first byte"""
    if 48 <= c <= 57:
        return (first, c - 48, 10, 0)
    return (True, 0, 1, 1 if c in CODE_OF else 0)


def combine(a, b):
    """as the header of csrc/ivx_cigar.hip states it, in unbounded integers"""
    if b[0]:
        return (True, b[1], b[2], a[3] + b[3])
    return (a[0], min(a[1] * b[2] + b[1], CAP), min(a[2] * b[2], CAP), a[3] + b[3])


def combine_u64(a, b):
    """the kernel's form: every product stays below 2^64 (checked)"""
    if b[0]:
        return (True, b[1], b[2], a[3] + b[3])
    if a[1] == 0:
        v = b[1]
    elif a[1] >= CAP or b[2] >= CAP:
        v = CAP
    else:
        x = a[1] * b[2] + b[1]
        assert x < (1 << 64)
        v = min(x, CAP)
    if a[2] >= CAP or b[2] >= CAP:
        p = CAP
    else:
        x = a[2] * b[2]
        assert x < (1 << 64)
        p = min(x, CAP)
    return (a[0], v, p, a[3] + b[3])


def _reduce_random(items, op, rng):
    """fold a non-empty list under a random association order"""
    items = list(items)
    while len(items) > 1:
        i = int(rng.integers(0, len(items) - 1))
        items[i:i + 2] = [op(items[i], items[i + 1])]
    return items[0]


def scan_tokens(strings, rng, op=combine):
    """the ops of a column by the scan: the exclusive prefix of every emitting byte is folded under a random association
    order -> [[(len, code)] per read]"""
    flat, first, rid = [], [], []
    for r, s in enumerate(strings):
        for j, c in enumerate(s):
            flat.append(c); first.append(j == 0); rid.append(r)
    els = [elem(c, f) for c, f in zip(flat, first)]
    out = [[] for _ in strings]
    n_ops = 0
    for i, c in enumerate(flat):
        if c not in CODE_OF:
            continue
        ex = _reduce_random([ident()] + els[:i], op, rng)
        assert ex[3] == n_ops
        v = 0 if (first[i] or ex[1] >= CAP) else ex[1]
        out[rid[i]].append((v, CODE_OF[c]))
        n_ops += 1
    return out


# ---- the reference's pinned tables on text CIGARs (tests/golden/pileup_cigar_text_golden.json)
def golden_cases():
    with open(GOLDEN_FILE) as f:
        return json.load(f)["cases"]


def case_columns(case, reads=None):
    """a golden case (or the reads `reads` of it) -> (contig names in byte order, read columns with the cigars as [bytes],
    the other kwargs of the restatements)"""
    rs = case["reads"] if reads is None else [case["reads"][i] for i in reads]
    names = sorted({r["contig"] for r in case["reads"]} | set(case["lengths"] or {}), key=lambda s: s.encode())
    ids = {n: i for i, n in enumerate(names)}
    cols = dict(rkey=np.array([ids[r["contig"]] for r in rs], np.uint32), rpos=np.array([r["pos"] for r in rs], np.uint32),
                rflags=np.array([r["flags"] for r in rs], np.uint32), rmapq=np.array([r["mapq"] for r in rs], np.uint32))
    cigars = [r["cigar"].encode() for r in rs]
    kw = dict(filter_flag=case["filter_flag"], min_mapq=case["min_mapq"],
              key_len=None if case["lengths"] is None else np.array([case["lengths"][n] for n in names], np.uint32))
    return names, cols, cigars, kw
