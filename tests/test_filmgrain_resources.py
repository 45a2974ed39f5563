"""CPU: what the compiler made of the film grain kernels, read from the built library's gfx950 code object (art_amd/codeobj.py), in the
pattern of tests/test_colorcorrection_resources.py.  A region is one pass of 24 B/px: a spilled register or a scratch array would be a second
memory stream next to it, and the LDS figure decides how many workgroups share a CU."""
import os
import re

import pytest

import fg_lib
from art_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "art_amd", "libartgpu.so")

# fg_region_kernel<CH, R>: channel L / C / LC (0 / 1 / 2) by kernel radius 1 / 2 / 3
KERNELS = [r"fg_region_kernel<%d, ?%d>" % (ch, r) for ch in (0, 1, 2) for r in (1, 2, 3)] + [r"fg_indices_kernel"]


@pytest.fixture(scope="module")
def table():
    # properties of the BUILT library: a missing build or a library without a gfx950 bundle is a failure, not a skip
    assert os.path.exists(LIB), "art_amd/libartgpu.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    t = codeobj.kernel_table(LIB)
    assert t, "libartgpu.so holds no gfx950 code object"
    return t


@pytest.mark.parametrize("pattern", KERNELS)
def test_kernels_neither_spill_nor_use_scratch(table, pattern):
    hits = {n: r for n, r in table.items() if re.search(pattern, n)}
    assert len(hits) == 1, (pattern, sorted(hits))
    for name, r in hits.items():
        assert r["scratch_bytes"] == 0 and r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0, (name, r)
        assert r["vgprs"] <= 256, (name, r)          # 256-thread workgroups: at least two of them fit a CU's register file
        assert r["static_lds_bytes"] <= fg_lib.LDS_BYTES_MAX, (name, r)


def test_no_other_film_grain_kernel(table):
    """the list above is the whole file: a kernel added later gets its row here"""
    mine = [n for n in table if re.search(r"\bfg_\w+_kernel", n)]
    assert len(mine) == len(KERNELS), sorted(mine)
