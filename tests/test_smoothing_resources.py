"""CPU: what the compiler made of the Smoothing tool's kernels, read from the built library's gfx950 code object (art_amd/codeobj.py), in the
pattern of tests/test_colorcorrection_resources.py.  Every pass of smoothing.hip is a stream over 3 to 11 planes: a spilled register or a
scratch array would be one more memory stream next to them."""
import os
import re

import pytest

from art_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "art_amd", "libartgpu.so")

# channel settings 0 (L), 1 (C), 2 (LC); sm_finish_kernel<channel, last>; sm_scale_kernel<0 to 1, 1 to 65535, 2 both>
KERNELS = ([r"sm_box_kernel", r"sm_subsample_self_kernel", r"sm_ab_self_kernel"] + [r"sm_scale_kernel<%d>" % m for m in range(3)] +
           [r"sm_%s_kernel<%d>" % (k, c) for k in ("prepare", "nlm_split", "nlm_merge") for c in range(3)] +
           [r"sm_finish_kernel<%d, *%s>" % (c, l) for c in range(3) for l in ("true", "false")])


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
        assert r["static_lds_bytes"] == 0, (name, r)


def test_no_other_smoothing_kernel(table):
    """the list above is the whole file: a kernel added later gets its row here"""
    mine = [n for n in table if re.search(r"\bsm_\w+_kernel", n)]
    assert len(mine) == len(KERNELS), sorted(mine)
