"""-m gpu: merge / cluster / complement at the tile, wavefront, thread and key-boundary edges of the run sweep (csrc/ivx_runs.hip
k_pk_max / k_pk_runs, and the fallback scans k_merge_apply / k_head_apply).

The inputs are the designed cases of tests/run_forms.py (tests/test_run_forms_cpu.py shows that each one reaches the edge it is
named for): row counts around 8, 512 and 4096; key boundaries on and beside a thread, a wavefront and a tile, a whole
single-key wavefront opening a key; runs longer than a tile; the largest end on the last row of a thread, a wavefront, a tile;
equal starts across those boundaries; the head test at exactly min_dist - 1, min_dist, min_dist + 1; the bit widths of the
packed word; 1026 tiles (two levels of the tile-summary scans); thousands of tiny keys.  Every result is compared column by
column, bit-exactly, with the CPU oracle -- under default settings and with each form turned off in turn -- and after every
call the form it took is read back (pyivx.Ctx.sweep_form()) and compared with the host rules (run_forms.host_form), so that no
case passes through another path than the one its setting names."""
import os
import sys

import numpy as np
import pytest

import run_forms as rf
from conftest import ROOT
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

# setting -> the environment knobs it sets (monkeypatch) and what every call under it must report
SETTINGS = {
    "default": (),                                                      # packed words + narrow runs where the ranges allow
    "no_narrow_runs": ("IVX_NO_NARROW_RUNS",),                          # the generic path in every wavefront
    "no_lin": ("IVX_NO_LIN",),                                          # key bits in the word
    "rows_narrow": ("IVX_NO_FUSED_SWEEP",),                             # k_merge_apply / k_head_apply over narrow rows
    "rows_wide": ("IVX_NO_FUSED_SWEEP", "IVX_NO_NARROW_SWEEP"),         # ... over wide rows, cur_end as i64
}
WHICH = {None: list(SETTINGS), "fallback": ["rows_narrow", "rows_wide"], "H": ["default", "no_narrow_runs"]}
FORM_WORDS = tuple(pyivx.SWEEP_SLOTS)                                   # every word: host_form states them all
CLUSTER_COLS = ("key", "start", "end", "row", "cluster", "cluster_start", "cluster_end")


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


def _host(x):
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.asarray(x).astype(np.int64)


def _same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        g = _host(g)
        if w.dtype == np.uint32:
            g = g & 0xFFFFFFFF                           # (device key / row columns come back as int32)
        assert len(g) == len(w) and np.array_equal(g, w.astype(np.int64)), f"{what}: column {i}"


def _same_cluster(got, want, what):
    _same([got[c] for c in CLUSTER_COLS], [want[c] for c in CLUSTER_COLS], what)
    assert got["n_clusters"] == want["n_clusters"], what
    assert np.array_equal(_host(got["key_clusters"]), want["key_clusters"].astype(np.int64)), what


def _form(ctx, case, rows, md, strict, op, setting, what):
    """the form the last call took: the host rules word by word, and what the setting is there to force"""
    k, s, e, nk = rows
    got = ctx.sweep_form()
    want = rf.host_form(k, s, e, nk, md, strict, op=op, knobs=SETTINGS[setting], stats=case.stats())
    assert set(want) == set(FORM_WORDS) and got == want, f"{what}: form {got}, the host rules say {want}"
    falls_back = strict and md == 0 and bool(case.claims.get("has_empty"))
    packed = 1 if op == "merge" else 2
    if setting == "default" and case.family != "G":
        assert (got["packed"], got["narrow_runs"]) == ((0, 0) if falls_back else (packed, 1)), what
    elif setting == "no_narrow_runs" and case.family != "G":
        assert (got["packed"], got["narrow_runs"]) == ((0, 0) if falls_back else (packed, 0)), what
    elif setting == "no_lin":
        assert got["lin"] == 0 and got["bits_k"] == int(nk - 1).bit_length(), what
    elif setting in ("rows_narrow", "rows_wide"):
        assert got["packed"] == 0 and got["narrow_runs"] == 0 and got["ntile"] == 0, what
        if setting == "rows_wide":
            assert got["narrow_rows"] == 0 and got["k8"] == 0, what
    if case.family == "G" and op == "merge":                           # (the claims are worded for merge: cluster reads no narrow rows)
        want_g = case.claims["forms"].get({"default": "default", "no_lin": "IVX_NO_LIN"}.get(setting), {})
        assert {w: got[w] for w in want_g} == want_g, what
    if case.family == "G" and setting.startswith("rows") and "starts_equal" in case.name:
        assert got["two_step"] == 1 and got["toolong"] == 1, what         # one run of equal starts far above FIX_MAXRUN
    if "ntile" in case.claims and setting in WHICH["H"]:
        assert got["ntile"] == case.claims["ntile"], what
    return got


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a.view(np.int32) if a.dtype == np.uint32 else a)).cuda()


def _views(k, s, e):
    """one view per key with rows, one base wider than its rows on either side"""
    ks = np.unique(k)
    lo = np.array([s[k == kk].min() - 1 for kk in ks], np.int64)
    hi = np.array([e[k == kk].max() + 1 for kk in ks], np.int64)
    return ks.astype(np.uint32), lo, hi


@pytest.mark.parametrize("name", list(rf.CASES))
def test_run_edges(ctx, monkeypatch, name):
    case = rf.CASES[name]
    rows = k, s, e, nk = case.rows()
    base = np.arange(nk, dtype=np.int64) * 1_000_003 + 17
    want = {(md, st): (orc.merge(k, s, e, min_dist=md, strict=st), orc.cluster(k, s, e, min_dist=md, strict=st, n_keys=nk)) for md, st in case.pairs}
    views = _views(k, s, e) if case.complement else None
    want_x = orc.complement(k, s, e, *views) if views else None
    dev = tuple(_dev(a) for a in (k, s, e)) if case.device else None
    for setting in WHICH[case.only_knobs]:
        with monkeypatch.context() as m:
            for knob in SETTINGS[setting]:
                m.setenv(knob, "1")
            for md, st in case.pairs:
                what = f"{name} {setting} min_dist={md} strict={st}"
                wm, wc = want[(md, st)]
                _same(ctx.merge(k, s, e, n_keys=nk, min_dist=md, strict=st), wm, f"merge {what}")
                _form(ctx, case, rows, md, st, "merge", setting, f"merge {what}")
                got = ctx.cluster(k, s, e, n_keys=nk, min_dist=md, strict=st)
                _form(ctx, case, rows, md, st, "cluster", setting, f"cluster {what}")
                _same_cluster(got, wc, f"cluster {what}")
                cnt = ctx.cluster(k, s, e, n_keys=nk, min_dist=md, strict=st, rows=False)
                _form(ctx, case, rows, md, st, "cluster", setting, f"cluster rows=False {what}")
                assert cnt["n_clusters"] == wc["n_clusters"] and np.array_equal(_host(cnt["key_clusters"]), wc["key_clusters"].astype(np.int64)), what
                based = ctx.cluster(k, s, e, n_keys=nk, min_dist=md, strict=st, key_base=base)
                _form(ctx, case, rows, md, st, "cluster", setting, f"cluster key_base {what}")
                first = np.concatenate([[0], np.cumsum(wc["key_clusters"].astype(np.int64))[:-1]])
                kk = wc["key"].astype(np.int64)
                _same([based[c] for c in CLUSTER_COLS if c != "cluster"], [wc[c] for c in CLUSTER_COLS if c != "cluster"], f"cluster key_base {what}")
                assert np.array_equal(_host(based["cluster"]), wc["cluster"] - first[kk] + base[kk]), f"cluster key_base ids {what}"
                if dev:
                    gm = ctx.merge(*dev, n_keys=nk, min_dist=md, strict=st)
                    _form(ctx, case, rows, md, st, "merge", setting, f"merge device {what}")
                    gc = ctx.cluster(*dev, n_keys=nk, min_dist=md, strict=st)
                    _form(ctx, case, rows, md, st, "cluster", setting, f"cluster device {what}")
                    ctx.synchronize()
                    _same(gm, wm, f"merge device {what}")
                    _same_cluster(gc, wc, f"cluster device {what}")
            if views:
                _same(ctx.complement(k, s, e, *views, n_keys=nk), want_x, f"complement {name} {setting}")
                _form(ctx, case, rows, 0, False, "merge", setting, f"complement {name} {setting}")


def test_refusals_on_a_multi_tile_input(ctx):
    """min_dist < 0 and a key id >= n_keys are refused at 4097 rows as they are on small inputs, and the context stays usable"""
    case = rf.CASES["B_at4096+1_larger"]
    k, s, e, nk = case.rows()
    k, s, e = k[:4097], s[:4097], e[:4097]
    want = orc.merge(k, s, e)
    for call in (ctx.merge, ctx.cluster):
        with pytest.raises(pyivx.IvxError):
            call(k, s, e, n_keys=nk, min_dist=-1)
        _same(ctx.merge(k, s, e, n_keys=nk), want, "merge after a refused min_dist")
        for bad in (nk, 0xFFFFFFFF):
            for at in (0, 2048, 4096):
                bk = k.copy()
                bk[at] = bad
                with pytest.raises(pyivx.IvxError) as ei:
                    call(bk, s, e, n_keys=nk)
                assert ei.value.status == pyivx.ERR_INVALID
                _same(ctx.merge(k, s, e, n_keys=nk), want, "merge after a refused key id")
    assert ctx.sweep_form()["ntile"] == 2
