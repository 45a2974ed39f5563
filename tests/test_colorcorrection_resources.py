"""CPU: what the compiler made of the colour-correction kernels, read from the built library's gfx950 code object (art_amd/codeobj.py), in the
pattern of tests/test_textureboost_resources.py.  The tool is one pass of 24 B/px and up to 8 B/px per region: a spilled register or a scratch
array would be a second memory stream next to it."""
import os
import re

import pytest

from art_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "art_amd", "libartgpu.so")

# cc_apply_kernel<NEED>: 0 plain, 1 + the yuv hue shift, 3 + Jzazbz (PQ tables), 5 + the HSL hue shift (fp64).  There is no <7>: a launch
# never carries Jzazbz and the HSL hue shift together (colorcorrection.h, cc_need_fits)
KERNELS = [r"cc_apply_kernel<0>", r"cc_apply_kernel<1>", r"cc_apply_kernel<3>", r"cc_apply_kernel<5>", r"cc_count_kernel"]


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
        assert r["vgprs"] <= 128, (name, r)          # 256-thread workgroups: eight of them fit a CU's register file


def test_no_other_colour_correction_kernel(table):
    """the list above is the whole file: a kernel added later gets its row here"""
    mine = [n for n in table if re.search(r"\bcc_\w+_kernel", n)]
    assert len(mine) == len(KERNELS), sorted(mine)


def test_only_the_count_kernel_uses_lds(table):
    for name, r in table.items():
        if "cc_apply_kernel" in name:
            assert r["static_lds_bytes"] == 0, (name, r)
