"""CPU restatement of the overlap thresholds (include/ivx_where.h), built from the oracle's own pairs: orc.join gives the
matched pairs, passes() is the pass rule in numpy int64 on them, and the surviving pairs go through the existing reductions
(overlap_agg_oracle.from_pairs, overlap_select_oracle.from_pairs).

    W(min_bases=0, probe=(0, 0), build=(0, 0), either=0)        the threshold's six integers
    Want(build, probe)                                          the oracle's pairs, made once; .pairs(w), .per_row(w), .exists(w),
                                                                .marks(w), .agg(w, val), .select(w, by, val)

brute_pairs() is an independent O(n * m) restatement in Python integers, for the hand-made tables; the CPU tests hold the two
against each other."""
import numpy as np

from oracle import oracle as orc
import overlap_agg_oracle as agg
import overlap_select_oracle as sel


class W:
    """an ivx_overlap_where: min_bases, (probe_num, probe_den), (build_num, build_den), either"""

    def __init__(self, min_bases=0, probe=(0, 0), build=(0, 0), either=0):
        self.min_bases, self.probe, self.build, self.either = int(min_bases), tuple(probe), tuple(build), int(either)

    def asks(self):
        return self.min_bases > 0 or self.probe[0] > 0 or self.build[0] > 0

    def kw(self):
        """the keywords of pyivx.OverlapWhere"""
        return dict(min_bases=self.min_bases, probe=self.probe if self.probe[0] else None, build=self.build if self.build[0] else None,
                    either=bool(self.either))

    def __repr__(self):
        return f"W({self.min_bases}, {self.probe}, {self.build}, {self.either})"


def passes(w, bs, be, qs, qe):
    """the pass rule on int64 columns of matched pairs -> bool per pair.  Every product fits int64: |len|, |plen|, |blen| <= 2^32,
    num <= den <= 2^31 - 1."""
    bs, be, qs, qe = (np.asarray(c, np.int64) for c in (bs, be, qs, qe))
    if w is None or not w.asks():
        return np.ones(len(bs), bool)
    ln = np.minimum(qe, be) - np.maximum(qs, bs) + 1
    ok = ln >= 1
    if w.min_bases > 0:
        ok &= ln >= w.min_bases
    fr = []
    if w.probe[0] > 0:
        fr.append(ln * np.int64(w.probe[1]) >= (qe - qs + 1) * np.int64(w.probe[0]))
    if w.build[0] > 0:
        fr.append(ln * np.int64(w.build[1]) >= (be - bs + 1) * np.int64(w.build[0]))
    if len(fr) == 2:
        ok &= (fr[0] | fr[1]) if w.either else (fr[0] & fr[1])
    elif fr:
        ok &= fr[0]
    return ok


def filter_pairs(w, b, p, wb, wp):
    """the pairs of (wb, wp) that pass, in their order"""
    wb, wp = np.asarray(wb, np.int64), np.asarray(wp, np.int64)
    keep = passes(w, np.asarray(b[1])[wb], np.asarray(b[2])[wb], np.asarray(p[1])[wp], np.asarray(p[2])[wp])
    return wb[keep], wp[keep]


class Want:
    """the oracle's pairs of (build, probe), made once; every filtered result from them"""

    def __init__(self, b, p, threads=4):
        self.b, self.p = b, p
        wb, wp = orc.join(*b, *p, threads=threads)
        self.wb, self.wp = np.asarray(wb, np.int64), np.asarray(wp, np.int64)
        self.nb, self.n = len(b[1]), len(p[1])

    def pairs(self, w):
        return filter_pairs(w, self.b, self.p, self.wb, self.wp)

    def per_row(self, w):
        return np.bincount(self.pairs(w)[1], minlength=self.n).astype(np.uint32)

    def exists(self, w):
        return (self.per_row(w) != 0).astype(np.uint8)

    def marks(self, w, prior=None):
        """the build side's mark bitmap (uint32 words, bit b & 31 of word b >> 5), ORed into `prior`"""
        bits = np.zeros(((self.nb + 31) // 32) * 32, bool)
        bits[self.pairs(w)[0]] = True
        words = np.packbits(bits, bitorder="little").view(np.uint32) if len(bits) else np.zeros(0, np.uint32)
        out = np.zeros(max(len(words), 0 if prior is None else len(prior)), np.uint32)
        out[:len(words)] = words
        if prior is not None:
            out[:len(prior)] |= prior
        return out

    def agg(self, w, val):
        return agg.from_pairs(self.b, self.p, val, *self.pairs(w))

    def select(self, w, by, val=None):
        return sel.from_pairs(self.b, self.p, by, val, *self.pairs(w))


def brute_pairs(w, b, p):
    """O(n * m), Python integers: same key, bs <= qe and be >= qs, then the pass rule -> (build rows, probe rows), probe-major"""
    bk, bs, be = [np.asarray(c).tolist() for c in b]
    pk, ps, pe = [np.asarray(c).tolist() for c in p]
    ob, op = [], []
    asks = w is not None and w.asks()
    for i in range(len(ps)):
        for j in range(len(bs)):
            if not (bk[j] == pk[i] and bs[j] <= pe[i] and be[j] >= ps[i]):
                continue
            if asks:
                ln = min(pe[i], be[j]) - max(ps[i], bs[j]) + 1
                if ln < 1 or (w.min_bases > 0 and ln < w.min_bases):
                    continue
                fr = []
                if w.probe[0] > 0:
                    fr.append(ln * w.probe[1] >= (pe[i] - ps[i] + 1) * w.probe[0])
                if w.build[0] > 0:
                    fr.append(ln * w.build[1] >= (be[j] - bs[j] + 1) * w.build[0])
                if fr and not (any(fr) if (w.either and len(fr) == 2) else all(fr)):
                    continue
            ob.append(j); op.append(i)
    return np.array(ob, np.int64), np.array(op, np.int64)


def cols(k, s, e):
    return np.asarray(k, np.uint32), np.asarray(s, np.int32), np.asarray(e, np.int32)


I32_MIN, I32_MAX = -2**31, 2**31 - 1

# The boundary table, one key.  Build rows (closed):
#   0: [100, 199]  blen 100        1: [150, 349]  blen 200        2: [1000, 1009]  blen 10
#   3: [I32_MIN, I32_MAX]  blen 2^32 (key 1)
# Probe rows:
#   0: [150, 249]  plen 100: len 50 with build 0 (exactly half of both), len 100 with build 1 (all of the probe, half of build 1)
#   1: [151, 250]  plen 100: len 49 with build 0 (one base short of half), len 100 with build 1
#   2: [1005, 1024] plen 20: len 5 with build 2 (a quarter of the probe, half of build 2)
#   3: [1006, 1025] plen 20: len 4 with build 2
#   4: [I32_MIN, I32_MAX] key 1, plen 2^32: len 2^32 with build 3
#   5: [0, I32_MAX] key 1, plen 2^31: len 2^31 with build 3 (all of the probe, half of build 3)
#   6: [120, 110]  end < start, inside build 0 (100 <= 110 and 199 >= 120: the join matches it): len = 110 - 120 + 1 < 1
HAND_BUILD = cols([0, 0, 0, 1], [100, 150, 1000, I32_MIN], [199, 349, 1009, I32_MAX])
HAND_PROBE = cols([0, 0, 0, 0, 1, 1, 0], [150, 151, 1005, 1006, I32_MIN, 0, 120], [249, 250, 1024, 1025, I32_MAX, I32_MAX, 110])
HAND_ALL = {(0, 0), (1, 0), (0, 1), (1, 1), (2, 2), (2, 3), (3, 4), (3, 5), (0, 6)}       # (build, probe): the unfiltered join
DEN_MAX = 2**31 - 1
# (threshold, what it stands for, the pairs expected): written out by hand from the comments above
HAND_CASES = [
    (W(), "nothing asked", HAND_ALL),
    # bedtools intersect -f 0.5: at least half of the probe row (A).  len 50 of 100 passes; 49 of 100 fails; 5 of 20 fails
    (W(probe=(1, 2)), "-f 0.5", {(0, 0), (1, 0), (1, 1), (3, 4), (3, 5)}),
    # -f 0.5 -r: reciprocal, half of both.  (1, 0): 100 of build 1's 200 passes; (3, 5): 2^31 of 2^32 passes
    (W(probe=(1, 2), build=(1, 2)), "-f 0.5 -r", {(0, 0), (1, 0), (1, 1), (3, 4), (3, 5)}),
    # -f 0.5 -F 0.5 -e: either.  (2, 2): 5 of build 2's 10 passes on the build side alone; (2, 3): 4 of 10 and 4 of 20 fails;
    # (0, 1): 49 of 100 on both sides fails
    (W(probe=(1, 2), build=(1, 2), either=1), "-f 0.5 -F 0.5 -e", {(0, 0), (1, 0), (1, 1), (2, 2), (3, 4), (3, 5)}),
    (W(build=(1, 2)), "-F 0.5", {(0, 0), (1, 0), (1, 1), (2, 2), (3, 4), (3, 5)}),
    # min_bases at len and at len + 1: 50 keeps (0, 0), 51 drops it; 49 keeps (0, 1)
    (W(min_bases=49), "min 49", {(0, 0), (1, 0), (0, 1), (1, 1), (3, 4), (3, 5)}),
    (W(min_bases=50), "min 50", {(0, 0), (1, 0), (1, 1), (3, 4), (3, 5)}),
    (W(min_bases=51), "min 51", {(1, 0), (1, 1), (3, 4), (3, 5)}),
    (W(min_bases=1), "min 1: only the pair of the row with end < start goes", HAND_ALL - {(0, 6)}),
    (W(min_bases=2**32), "min 2^32", {(3, 4)}),
    (W(min_bases=2**32 + 1), "min 2^32 + 1", set()),
    # the whole int32 range with the largest denominator: 2^32 * (2^31 - 1) on both sides of the comparison
    (W(probe=(DEN_MAX, DEN_MAX)), "probe 1/1 at den 2^31 - 1", {(1, 0), (1, 1), (3, 4), (3, 5)}),
    (W(build=(DEN_MAX, DEN_MAX)), "build 1/1 at den 2^31 - 1", {(3, 4)}),
    (W(build=(DEN_MAX - 1, DEN_MAX)), "build just under 1", {(3, 4)}),
    (W(build=((DEN_MAX + 1) // 2, DEN_MAX)), "build just over a half: 2^31 of 2^32 fails, 50 of 100 fails", {(3, 4)}),
    (W(build=((DEN_MAX - 1) // 2, DEN_MAX)), "build just under a half", {(0, 0), (1, 0), (1, 1), (2, 2), (3, 4), (3, 5)}),
]
