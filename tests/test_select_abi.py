"""CPU-only: overlap select's entries at every boundary.  include/ivx_select.h is a companion of include/ivx.h: what it declares
is exported by libivx_hip.so, bound by pyivx from EXT_SYMBOLS (and from no other list) and declared in
integration/rust/select_ffi.rs with the types the C prototype maps to; brh_overlap_select is in include/bio_ranges_host.h, in
the host library and in the same Rust file."""
import ctypes
import os
import re
import sys

from conftest import ROOT
from test_abi import _c_protos, _rust_protos

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402

HEADER = os.path.join(ROOT, "include", "ivx_select.h")
RUST = os.path.join(ROOT, "integration", "rust", "select_ffi.rs")


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ivx_[a-z0-9_]+)\s*\(", src)))


def test_companion_header_symbols_are_exported_and_bound():
    names = _declared()
    assert names == ["ivx_probe_overlap_select"]
    L = pyivx.lib()
    for n in names:
        assert hasattr(L, n), f"libivx_hip.so does not export {n}"
    assert sorted(pyivx.EXT_SYMBOLS) == names
    assert not set(pyivx.EXT_SYMBOLS) & set(pyivx.SYMBOLS)
    # ... and include/ivx.h does not declare them a second time
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivx.h")).read(), flags=re.S)
    for n in names:
        assert not re.search(r"\b" + n + r"\s*\(", main), n


def test_criteria_match_the_header():
    # pyivx.SEL_BY names the IVX_SEL_* criteria in the order of the enum; bio_ranges_host.h numbers its BRH_SEL_* alike
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    slots = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bIVX_SEL_(\w+)\s*=\s*(\d+)", src)}
    assert slots.pop("n") == len(slots) == 6
    assert tuple(sorted(slots, key=slots.get)) == pyivx.SEL_BY
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bio_ranges_host.h")).read(), flags=re.S)
    brh = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bBRH_SEL_(\w+)\s*=\s*(\d+)", host)}
    assert brh == dict(slots, n=6)


def test_rust_declarations_match_the_companion_header():
    hdr = _c_protos(HEADER, "ivx_")
    rust = _rust_protos(RUST, "ivx_")
    assert sorted(rust) == sorted(hdr) == _declared()
    for name in hdr:
        assert rust[name] == hdr[name], (name, rust[name], hdr[name])
        assert len(hdr[name][0]) == len(getattr(pyivx.lib(), name).argtypes), name


def test_host_operator_is_declared_on_both_sides():
    def sigs(text, pat):
        out = {}
        for m in re.finditer(pat, text, re.S):
            args = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
            out[m.group(1)] = 0 if args.strip() in ("", "void") else args.count(",") + 1
        return out

    hdr = sigs(open(os.path.join(ROOT, "include", "bio_ranges_host.h")).read(), r"\b(brh_\w+)\s*\(([^;{]*?)\)\s*;")
    rust = sigs(open(RUST).read(), r"pub fn (brh_\w+)\(([^;]*?)\)\s*(?:->\s*[\w\* ]+)?;")
    assert sorted(rust) == ["brh_overlap_select"]
    assert {k: hdr.get(k) for k in rust} == rust
    lib = os.path.join(ROOT, "datafusion-bio-functions_amd", "lib", "libbio_ranges_hip.so")
    assert os.path.exists(lib)
    pyivx.lib()                                             # (the HIP library first: the host library links it)
    assert hasattr(ctypes.CDLL(lib), "brh_overlap_select")
