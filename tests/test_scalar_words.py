"""CPU-only: the context's scalar words (ivx_ctx::d_scalars / h_scalars) are named in ONE table, csrc/ivx_scalars.hpp.
No other source addresses them by number, and no other source keeps an enum of word numbers of its own."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "datafusion-bio-functions_amd", "csrc")
TABLE = "ivx_scalars.hpp"


def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".hpp")) and f != TABLE:
            yield f, open(os.path.join(CSRC, f)).read()


def test_table_exists_and_is_included():
    assert os.path.isfile(os.path.join(CSRC, TABLE))
    assert '#include "ivx_scalars.hpp"' in open(os.path.join(CSRC, "ivx_internal.hpp")).read()
    assert len(list(_sources())) >= 25


def test_no_scalar_word_by_number():
    by_number = re.compile(r"(d_scalars|h_scalars|hd_scalars)\s*(\+|\[)\s*\d")
    for f, txt in _sources():
        hits = [ln for ln in txt.splitlines() if by_number.search(ln)]
        assert not hits, (f, hits)


def test_no_enum_of_word_numbers_outside_the_table():
    # the per-file enums that the table replaced, and any new one in their style or the table's
    old = re.compile(r"\b(DS|CS|MS|PS)_[A-Z0-9]+\b|\bRS_BAD\b|\bIVX_HS_\w+")
    sc_def = re.compile(r"\bSC_[A-Z0-9_]+\s*=[^=]")
    for f, txt in _sources():
        assert not old.search(txt), (f, old.search(txt).group(0))
        assert not sc_def.search(txt), (f, sc_def.search(txt).group(0))
    # an alias of a whole array would hide numbered uses from the check above
    alias = re.compile(r"=\s*ctx->(d_scalars|h_scalars|hd_scalars)\s*[,;]")
    for f, txt in _sources():
        assert not alias.search(txt), (f, alias.search(txt).group(0))


def test_outliving_words_are_listed_next_to_the_table():
    """SC_OUTLIVES, the list the poison hook (ivx_debug_poison) spares, names exactly the words whose comment in the table says
    OUTLIVES: the word defined next after each such comment"""
    txt = open(os.path.join(CSRC, TABLE)).read()
    body = txt[txt.index("enum {\n    // ---- overlap probes"):txt.index("SC_HOST_WORDS =")]
    said = []
    for m in re.finditer(r"OUTLIVES", body):
        said.append(re.search(r"^\s*(SC_[A-Z0-9_]+)\s*=", body[m.end():], re.M).group(1))
    lst = re.search(r"SC_OUTLIVES\[\]\s*=\s*\{(.*?)\};", txt, re.S).group(1)
    listed = re.findall(r"\{\s*(SC_[A-Z0-9_]+)\s*,\s*([^{}]+?)\s*\}", lst)
    assert len(said) >= 2 and [w for w, _ in listed] == said
    # ... each with the length the table gives it: the word defined next is `SC_X + <length>`
    squash = lambda s: re.sub(r"\s+", "", s)
    for word, length in listed:
        nxt = re.search(r"^\s*SC_[A-Z0-9_]+\s*=\s*" + word + r"\s*\+\s*([^,/\n]*(?:/\s*\d+)?)\s*,?\s*(?://.*)?$", txt, re.M)
        assert nxt and squash(nxt.group(1)) == squash(length), (word, length, nxt and nxt.group(1))
    # the hook walks the list, and nothing else decides what it spares
    capi = open(os.path.join(CSRC, "ivx_capi.hip")).read()
    hook = capi[capi.index("ivx_status ivx_debug_poison("):]
    hook = hook[:hook.index("\n}\n")]
    assert "SC_OUTLIVES" in hook and not re.search(r"\bSC_(UNSORTED|HDR_MIRROR)\b", hook)
