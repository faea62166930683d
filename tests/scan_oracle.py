"""CPU reference for the scan of the test-only operator of csrc/ivx_scan.hip (AffineOp): affine maps x -> a*x + b modulo
2^32.  An element is (a, b) packed as a << 32 | b in one uint64, combine(earlier, later) = (l.a*e.a, l.a*e.b + l.b) in
uint32 arithmetic, the identity is (1, 0).  The operator is associative and does not commute, so a scan kernel that
swaps the operands of one combine gives other values.

affine_scan_serial is the definition, one element at a time (small n).  affine_scan is a numpy doubling scan
(Hillis-Steele): after the step with distance d, element i holds the composition of elements i-2d+1 .. i; the element d
places back covers the earlier indices, so it is the `earlier` operand."""
import numpy as np

IDENTITY = np.uint64(1 << 32)
_M = 0xFFFFFFFF


def pack(a, b):
    return (np.asarray(a, np.uint64) << np.uint64(32)) | np.asarray(b, np.uint64)


def unpack(x):
    x = np.asarray(x, np.uint64)
    return (x >> np.uint64(32)).astype(np.uint32), (x & np.uint64(_M)).astype(np.uint32)


def exclusive_of(incl):
    out = np.empty_like(incl)
    if len(out):
        out[0] = IDENTITY
        out[1:] = incl[:-1]
    return out


def affine_scan_serial(x, inclusive=True):
    """element by element with Python ints"""
    out = np.empty(len(x), np.uint64)
    ra, rb = 1, 0                                     # the running map: everything before (exclusive) / up to (inclusive) i
    for i, v in enumerate(np.asarray(x, np.uint64).tolist()):
        la, lb = v >> 32, v & _M
        na, nb = (la * ra) & _M, (la * rb + lb) & _M  # combine(run, x[i])
        if inclusive:
            out[i] = (na << 32) | nb
        else:
            out[i] = (ra << 32) | rb
        ra, rb = na, nb
    return out


def affine_scan(x, inclusive=True):
    """numpy doubling scan on uint32 arrays (they wrap modulo 2^32)"""
    A, B = unpack(x)
    A, B = A.copy(), B.copy()
    d = 1
    while d < len(A):
        # (right-hand sides are evaluated in full before the assignment; B first, it needs the old A)
        B[d:] = A[d:] * B[:-d] + B[d:]
        A[d:] = A[d:] * A[:-d]
        d *= 2
    incl = pack(A, B)
    return incl if inclusive else exclusive_of(incl)
