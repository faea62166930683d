"""No GPU: the catalogue every entry walk iterates over (entry_cases.CASES) cannot fall behind the headers.  Every ivx_*
function include/ivx.h or a companion header include/ivx_*.h declares is either the target of a catalogue case -- the case `name` calls `ivx_` + name -- or stands
in NO_COLUMNS below, the entries that take no column of the caller's and so have nothing to stage, refuse or copy back.
Adding an entry to a header, or a companion header with entries, without a case (or without a reason here) fails this test."""
import glob
import os
import re

from conftest import ROOT
from entry_cases import CASES

# entry -> why no catalogue case walks it
NO_COLUMNS = {
    "ivx_ctx_create": "makes the context the walks run on",
    "ivx_ctx_free": "ends it",
    "ivx_last_error": "reads the context's error text: host string only",
    "ivx_ctx_set_stream": "stream setting: no data",
    "ivx_ctx_use_own_stream": "stream setting: no data",
    "ivx_ctx_synchronize": "waits for the stream: every case calls it after each entry (Env.call)",
    "ivx_ctx_set_build_overlap": "a switch; the walks set it around builds",
    "ivx_ctx_last_kernel_ms": "reads two events: no data",
    "ivx_version": "a constant string",
    "ivx_ctx_metrics": "reads host counters; the refusal walk compares them around every call",
    "ivx_ctx_reset_metrics": "zeroes host counters",
    "ivx_ctx_set_memory_limit": "sets a host word; the refusal walk steps it",
    "ivx_ctx_reserved_bytes": "reads host counters; the refusal walk asserts on it",
    "ivx_ctx_trim": "frees scratch; the refusal walk calls it between attempts",
    "ivx_index_free": "frees what index_build made, inside that case",
    "ivx_index_rows": "getter of a host field (read in the index_build case)",
    "ivx_index_device_bytes": "getter of a host field (read in the index_build case)",
    "ivx_index_layout": "diagnostic read-out of 13 words into a host array: no column, no scratch",
    "ivx_depth_profile_free": "frees what the profile builds and the merge made, inside those cases",
    "ivx_depth_profile_steps": "getter of a host field (read in the profile cases)",
    "ivx_depth_profile_device_bytes": "getter of a host field (read in the profile cases)",
}

DECL = re.compile(r"^(?:ivx_status|void|uint64_t|double|const char \*)\s*\*?(ivx_\w+)\(", re.M)


def headers():
    """include/ivx.h and every companion header beside it"""
    inc = os.path.join(ROOT, "include")
    return [os.path.join(inc, "ivx.h")] + sorted(glob.glob(os.path.join(inc, "ivx_*.h")))


def code_of(path):
    with open(path) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)        # (comments name entries, too)


def declared():
    return sorted({name for h in headers() for name in DECL.findall(code_of(h))})


COMPANIONS = {
    "ivx_select.h": ["ivx_probe_overlap_select"],
    "ivx_where.h": ["ivx_pairs_where", "ivx_probe_mark_build_where", "ivx_probe_overlap_agg_where", "ivx_probe_overlap_count_where",
                    "ivx_probe_overlap_select_where"],
    "ivx_nearest.h": ["ivx_probe_nearest_dir"],
}


def test_the_header_parses():
    names = declared()
    assert len(names) >= 57 + 7 and "ivx_ctx_create" in names and "ivx_take_view" in names, names
    assert len(headers()) >= 4, headers()
    # every `ivx_x(` of a header outside comments and macros is a declaration: the pattern misses no return type
    for h in headers():
        text = code_of(h)
        mine = sorted(set(DECL.findall(text)))
        assert sorted(set(re.findall(r"\b(ivx_\w+)\(", text))) == mine, h
        if os.path.basename(h) in COMPANIONS:
            assert mine == COMPANIONS[os.path.basename(h)], h


def test_every_declared_entry_has_a_case_or_a_reason():
    names = declared()
    cases = {"ivx_" + c for c in CASES}
    assert not cases & set(NO_COLUMNS)
    assert all(NO_COLUMNS.values())
    stale = sorted((cases | set(NO_COLUMNS)) - set(names))
    assert not stale, f"declared in no header under include/: {stale}"
    missing = sorted(set(names) - cases - set(NO_COLUMNS))
    assert not missing, f"declared under include/, no case in tests/entry_cases.py and no reason in NO_COLUMNS: {missing}"
