"""CPU-only: pyivx.DEPTH_EXPAND_TILE is the tile constant of the expand kernel, read from the source as text."""
import os
import re
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402


def test_tile_constant_matches_the_kernel_source():
    src = open(os.path.join(ROOT, "datafusion-bio-functions_amd", "csrc", "ivx_depth_expand.hip")).read()
    m = re.findall(r"\bconstexpr\s+int\s+DEPTH_EXPAND_TILE\s*=\s*(\d+)\s*;", src)
    assert len(m) == 1
    assert int(m[0]) == pyivx.DEPTH_EXPAND_TILE
    assert pyivx.DEPTH_EXPAND_TILE % 8 == 0          # whole 16-byte lines of Int16 coverages
