"""CPU-only: the entry of nearest on one side only / within a distance cap at every boundary.  include/ivx_nearest.h is a
companion of include/ivx.h: what it declares is exported by libivx_hip.so, bound by pyivx from NEAREST_SYMBOLS (and from no
other list) and declared in integration/rust/nearest_ffi.rs with the types the C prototype maps to; brh_nearest_dir is in
include/bio_ranges_host.h, in the host library and in the same Rust file."""
import ctypes
import glob
import os
import re
import sys

from conftest import ROOT
from test_abi import _c_protos, _rust_protos

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402

HEADER = os.path.join(ROOT, "include", "ivx_nearest.h")
HOST_HEADER = os.path.join(ROOT, "include", "bio_ranges_host.h")
RUST = os.path.join(ROOT, "integration", "rust", "nearest_ffi.rs")


def _uncommented(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(ivx_[a-z0-9_]+)\s*\(", _uncommented(HEADER))))


def test_companion_header_symbols_are_exported_and_bound():
    names = _declared()
    assert names == ["ivx_probe_nearest_dir"]
    L = pyivx.lib()
    for n in names:
        assert hasattr(L, n), f"libivx_hip.so does not export {n}"
    assert sorted(pyivx.NEAREST_SYMBOLS) == names
    assert not set(pyivx.NEAREST_SYMBOLS) & (set(pyivx.SYMBOLS) | set(pyivx.EXT_SYMBOLS) | set(pyivx.WHERE_SYMBOLS))
    # ... and no other header declares it a second time
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "ivx_nearest.h"]
    assert len(others) >= 4
    for p in others:
        for n in names:
            assert not re.search(r"\b" + n + r"\s*\(", _uncommented(p)), (n, p)


def test_directions_match_the_header():
    # pyivx.NEAR_DIRECTIONS names the IVX_NEAR_* directions in the order of the enum; bio_ranges_host.h numbers its BRH_NEAR_* alike
    slots = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bIVX_NEAR_(\w+)\s*=\s*(\d+)", _uncommented(HEADER))}
    assert slots.pop("n") == len(slots) == 3
    assert tuple(sorted(slots, key=slots.get)) == pyivx.NEAR_DIRECTIONS
    brh = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bBRH_NEAR_(\w+)\s*=\s*(\d+)", _uncommented(HOST_HEADER))}
    assert brh == slots
    assert set(pyivx.NEAR_ALIASES.values()) <= set(pyivx.NEAR_DIRECTIONS) and not set(pyivx.NEAR_ALIASES) & set(pyivx.NEAR_DIRECTIONS)


def test_rust_declarations_match_the_companion_header():
    hdr = _c_protos(HEADER, "ivx_")
    rust = _rust_protos(RUST, "ivx_")
    assert sorted(rust) == sorted(hdr) == _declared()
    for name in hdr:
        assert rust[name] == hdr[name], (name, rust[name], hdr[name])
        assert len(hdr[name][0]) == len(getattr(pyivx.lib(), name).argtypes), name
    # the entry is ivx_probe_nearest's prototype with (direction, max_distance) between include_overlaps and the outputs
    base = _c_protos(os.path.join(ROOT, "include", "ivx.h"), "ivx_")["ivx_probe_nearest"]
    mine = hdr["ivx_probe_nearest_dir"]
    assert mine[1] == base[1] and mine[0] == base[0][:10] + ["i32", "i64"] + base[0][10:]


def test_host_operator_is_declared_on_both_sides():
    def sigs(text, pat):
        out = {}
        for m in re.finditer(pat, text, re.S):
            args = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
            out[m.group(1)] = 0 if args.strip() in ("", "void") else args.count(",") + 1
        return out

    hdr = sigs(open(HOST_HEADER).read(), r"\b(brh_\w+)\s*\(([^;{]*?)\)\s*;")
    rust = sigs(open(RUST).read(), r"pub fn (brh_\w+)\(([^;]*?)\)\s*(?:->\s*[\w\* ]+)?;")
    assert sorted(rust) == ["brh_nearest_dir"]
    assert {k: hdr.get(k) for k in rust} == rust
    assert hdr["brh_nearest_dir"] == hdr["brh_nearest"] + 2
    # ... the two new parameters sit behind compute_distance, as (int, int64_t)
    r = _rust_protos(RUST, "brh_")["brh_nearest_dir"]
    assert r[0][9:11] == ["c_int", "i64"] and r[1] == "c_int"
    m = re.search(r"\bbrh_nearest_dir\s*\(([^;{]*?)\)\s*;", _uncommented(HOST_HEADER), re.S)
    assert [" ".join(a.split()) for a in m.group(1).split(",")][8:11] == ["int compute_distance", "int direction", "int64_t max_distance"]
    lib = os.path.join(ROOT, "datafusion-bio-functions_amd", "lib", "libbio_ranges_hip.so")
    assert os.path.exists(lib)
    pyivx.lib()                                             # (the HIP library first: the host library links it)
    assert hasattr(ctypes.CDLL(lib), "brh_nearest_dir")
