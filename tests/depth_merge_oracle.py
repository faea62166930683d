"""CPU restatements of streaming depth() for the tests: the merge of two depth profiles and the coverage blocks of one, as
include/ivx.h pins them for ivx_depth_profile_merge / ivx_depth_profile_blocks.

  merge_steps      a two-pointer walk over two (key, pos, c) step lists: coverage is additive, so at every position of
                   either list the result's coverage is the sum of what each list says from there on, and the position is
                   a step iff that sum differs from the sum just before it
  blocks_of_steps  coverage.rs:38-62 restated on steps: step i gives (key, p_i, p_(i+1) - 1, c_i) iff c_i != 0 and step
                   i + 1 has the same key

Both are pinned against depth_oracle / depth_per_base_oracle on random inputs and against the reference's own tables
(tests/test_depth_merge_cpu.py).
"""
import numpy as np

import depth_oracle as orc


def _rows(st):
    k, p, c = st[0], st[1], st[2]
    return [(int(a), int(b), int(d)) for a, b, d in zip(k, p, c)]


def steps_cols(rows, seen):
    a = np.array(rows, np.int64).reshape(-1, 3)
    return a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32), a[:, 2].astype(np.int32), np.asarray(seen, np.uint8)


def merge_steps(a, b):
    """a, b: (key u32, pos u32, coverage i32, key_seen u8[n_keys]) -> the same form for a + b; n_keys = the larger"""
    ra, rb = _rows(a), _rows(b)
    nk = max(len(a[3]), len(b[3]))
    seen = np.zeros(nk, np.uint8)
    seen[:len(a[3])] |= np.asarray(a[3], np.uint8)
    seen[:len(b[3])] |= np.asarray(b[3], np.uint8)
    out = []
    i = j = 0
    ka = kb = None          # key of the last step taken from each list
    ca = cb = 0             # its coverage
    while i < len(ra) or j < len(rb):
        wa = ra[i][:2] if i < len(ra) else None
        wb = rb[j][:2] if j < len(rb) else None
        w = wa if wb is None or (wa is not None and wa <= wb) else wb
        k = w[0]
        pa = ca if ka == k else 0
        pb = cb if kb == k else 0
        prev = orc._wrap32(pa + pb)
        if wa == w:
            ka, ca = k, ra[i][2]
            pa = ca
            i += 1
        if wb == w:
            kb, cb = k, rb[j][2]
            pb = cb
            j += 1
        c = orc._wrap32(pa + pb)
        if c != prev:
            out.append((k, w[1], c))
    return steps_cols(out, seen)


def blocks_of_steps(st):
    """(key, pos, coverage, ...) -> (key u32, start u32, end u32, coverage i32), ordered by (key, start)"""
    r = _rows(st)
    out = [(r[i][0], r[i][1], r[i + 1][1] - 1, r[i][2]) for i in range(len(r) - 1) if r[i][2] != 0 and r[i + 1][0] == r[i][0]]
    return orc._as_cols(out)


_READ_COLS = ("rkey", "rpos", "rflags", "rmapq")
_SEG_COLS = ("skey", "sstart", "send", "sweight")


def concat_cases(x, y):
    """X ++ Y: the kwargs of one call that has the reads and segments of both (n_keys, key_len, filter_flag and min_mapq are
    X's; a nullable column that only one side leaves out is filled with the value that means the same)"""
    out = {k: x[k] for k in ("filter_flag", "min_mapq", "key_len", "n_keys") if k in x}
    fill = dict(rkey=0, rflags=0, rmapq=0xFFFFFFFF, skey=0, sweight=1)
    for cols, ncol in ((_READ_COLS, "rpos"), (_SEG_COLS, "sstart")):
        nx = 0 if x.get(ncol) is None else len(x[ncol])
        ny = 0 if y.get(ncol) is None else len(y[ncol])
        for c in cols:
            vx, vy = x.get(c), y.get(c)
            if vx is None and vy is None:
                out[c] = None
                continue
            dt = np.int32 if c == "sweight" else np.uint32
            vx = np.full(nx, fill.get(c, 0), dt) if vx is None else np.asarray(vx, dt)
            vy = np.full(ny, fill.get(c, 0), dt) if vy is None else np.asarray(vy, dt)
            out[c] = np.concatenate([vx, vy])
    ox, oy = np.asarray(x["cigar_offsets"], np.int64), np.asarray(y["cigar_offsets"], np.int64)
    px, py = np.asarray(x["cigar_ops"], np.uint32), np.asarray(y["cigar_ops"], np.uint32)
    px, py = px[ox[0] // 4:ox[-1] // 4], py[oy[0] // 4:oy[-1] // 4]
    out["cigar_offsets"] = np.concatenate([ox - ox[0], oy[1:] - oy[0] + (ox[-1] - ox[0])]).astype(np.int32)
    out["cigar_ops"] = np.concatenate([px, py])
    return out


def random_pair(rng, max_pos=60, clip=None):
    """two random cases with the same n_keys, key_len, filter and mapq -> (X, Y)"""
    x = orc.random_case(rng, clip=clip, max_pos=max_pos)
    y = orc.random_case(rng, n_keys=x["n_keys"], clip=False, max_pos=max_pos)
    y["key_len"], y["min_mapq"], y["filter_flag"] = x["key_len"], x["min_mapq"], x["filter_flag"]
    return x, y
