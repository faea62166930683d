"""CPU-only: the overlap thresholds' entries at every boundary.  include/ivx_where.h is a companion of include/ivx.h: what it
declares is exported by libivx_hip.so, bound by pyivx from WHERE_SYMBOLS (and from no other list) and declared in
integration/rust/where_ffi.rs with the types the C prototype maps to, the struct's field order and types included; the three
brh_*_where operators are in include/bio_ranges_host.h, in the host library and in the same Rust file."""
import ctypes
import os
import re
import sys

from conftest import ROOT
import test_abi
from test_abi import _c_protos, _rust_protos

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402

HEADER = os.path.join(ROOT, "include", "ivx_where.h")
HOST_HEADER = os.path.join(ROOT, "include", "bio_ranges_host.h")
RUST = os.path.join(ROOT, "integration", "rust", "where_ffi.rs")
ENTRIES = ["ivx_pairs_where", "ivx_probe_mark_build_where", "ivx_probe_overlap_agg_where", "ivx_probe_overlap_count_where",
           "ivx_probe_overlap_select_where"]
HOST_ENTRIES = ["brh_interval_join_where", "brh_overlap_aggregate_where", "brh_overlap_select_where"]
FIELDS = [("min_bases", "int64_t", "i64"), ("probe_num", "uint32_t", "u32"), ("probe_den", "uint32_t", "u32"),
          ("build_num", "uint32_t", "u32"), ("build_den", "uint32_t", "u32"), ("either", "uint32_t", "u32")]


def _strip(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(ivx_[a-z0-9_]+)\s*\(", _strip(HEADER))))


def _c_struct_fields(text, name):
    """[(field, C type)] of `typedef struct name { ... } name;`, in order (`t a, b;` declares two)"""
    body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", text, re.S).group(1)
    out = []
    for decl in body.split(";"):
        toks = decl.replace(",", " ").split()
        out += [(f, toks[0]) for f in toks[1:]]
    return out


def test_companion_header_symbols_are_exported_and_bound():
    names = _declared()
    assert names == ENTRIES
    L = pyivx.lib()
    for n in names:
        assert hasattr(L, n), f"libivx_hip.so does not export {n}"
    assert sorted(pyivx.WHERE_SYMBOLS) == names
    assert not set(pyivx.WHERE_SYMBOLS) & (set(pyivx.SYMBOLS) | set(pyivx.EXT_SYMBOLS))
    # ... and neither include/ivx.h nor include/ivx_select.h declares them a second time
    for other in ("ivx.h", "ivx_select.h"):
        main = _strip(os.path.join(ROOT, "include", other))
        for n in names + ["ivx_overlap_where"]:
            assert not re.search(r"\b" + n + r"\b", main), (other, n)


def test_struct_matches_on_all_sides():
    want = [(f, c) for f, c, _ in FIELDS]
    assert _c_struct_fields(_strip(HEADER), "ivx_overlap_where") == want
    assert _c_struct_fields(_strip(HOST_HEADER), "brh_overlap_where") == want
    assert [(f, t._type_) for f, t in pyivx.OverlapWhereC._fields_] == \
        [(f, {"int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32}[c]._type_) for f, c, _ in FIELDS]
    assert ctypes.sizeof(pyivx.OverlapWhereC) == 32
    rust = re.sub(r"//[^\n]*", "", open(RUST).read())
    assert re.search(r"#\[repr\(C\)\][^{;]*pub struct IvxOverlapWhere\s*\{", rust)
    body = re.search(r"pub struct IvxOverlapWhere\s*\{(.*?)\}", rust, re.S).group(1)
    assert re.findall(r"pub (\w+)\s*:\s*(\w+)", body) == [(f, r) for f, _, r in FIELDS]
    assert re.search(r"pub type BrhOverlapWhere\s*=\s*IvxOverlapWhere\s*;", rust)


def test_rust_declarations_match_the_companion_header(monkeypatch):
    monkeypatch.setitem(test_abi._C_SCALARS, "ivx_overlap_where", "IvxOverlapWhere")
    hdr = _c_protos(HEADER, "ivx_")
    rust = _rust_protos(RUST, "ivx_")
    assert sorted(rust) == sorted(hdr) == _declared()
    for name in hdr:
        assert rust[name] == hdr[name], (name, rust[name], hdr[name])
        assert len(hdr[name][0]) == len(getattr(pyivx.lib(), name).argtypes), name
        assert "*const IvxOverlapWhere" in hdr[name][0], name


def test_host_operators_are_declared_on_both_sides():
    def sigs(text, pat):
        out = {}
        for m in re.finditer(pat, text, re.S):
            args = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
            out[m.group(1)] = 0 if args.strip() in ("", "void") else args.count(",") + 1
        return out

    hdr = sigs(open(HOST_HEADER).read(), r"\b(brh_\w+)\s*\(([^;{]*?)\)\s*;")
    rust_text = re.sub(r"//[^\n]*", "", open(RUST).read())
    rust = sigs(rust_text, r"pub fn (brh_\w+)\(([^;]*?)\)\s*(?:->\s*[\w\* ]+)?;")
    assert sorted(rust) == HOST_ENTRIES
    assert {k: hdr.get(k) for k in rust} == rust
    # each is its unfiltered counterpart's signature plus the threshold
    for name in HOST_ENTRIES:
        assert hdr[name] == hdr[name[:-len("_where")]] + 1, name
        assert re.search(r"pub fn " + name + r"\([^;]*:\s*\*const BrhOverlapWhere\b", rust_text, re.S), name
    lib = os.path.join(ROOT, "datafusion-bio-functions_amd", "lib", "libbio_ranges_hip.so")
    assert os.path.exists(lib)
    pyivx.lib()                                             # (the HIP library first: the host library links it)
    H = ctypes.CDLL(lib)
    for name in HOST_ENTRIES:
        assert hasattr(H, name), name


def test_python_threshold_forms():
    """a fraction is a (num, den) pair, a Fraction or a float; a float is Fraction(f).limit_denominator(10**9)"""
    from fractions import Fraction
    s = pyivx.OverlapWhere(min_bases=3, probe=0.5, build=Fraction(2, 3), either=True).c_struct()
    assert (s.min_bases, s.probe_num, s.probe_den, s.build_num, s.build_den, s.either) == (3, 1, 2, 2, 3, 1)
    s = pyivx.OverlapWhere(probe=(50, 100)).c_struct()                   # a pair goes through as it is
    assert (s.probe_num, s.probe_den, s.build_num, s.build_den) == (50, 100, 0, 0)
    f = Fraction(0.1).limit_denominator(10 ** 9)
    s = pyivx.OverlapWhere(build=0.1).c_struct()
    assert (s.build_num, s.build_den) == (f.numerator, f.denominator) == (1, 10)
    s = pyivx.OverlapWhere(probe=1.0, build=0.0).c_struct()
    assert (s.probe_num, s.probe_den, s.build_num) == (1, 1, 0)
    ref, keep = pyivx.as_where({"probe": 0.5})
    assert (keep.probe_num, keep.probe_den) == (1, 2) and pyivx.as_where(None) == (None, None)
    for bad in (dict(probe="half"), dict(probe=(1, 2, 3)), dict(build=-0.5)):
        try:
            pyivx.OverlapWhere(**bad).c_struct()
        except (TypeError, ValueError):
            continue
        raise AssertionError(bad)
