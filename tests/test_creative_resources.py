"""CPU: what the compiler made of the creative-gradients, soft-light and black-and-white kernels, read from the built library's gfx950 code
object (art_amd/codeobj.py), in the pattern of tests/test_filmgrain_resources.py.  Each is one pass of 24 B/px: a spilled register or a scratch
array would be a second memory stream next to it.  None declares static LDS (CG_LDS_BYTES, BW_LDS_BYTES in their headers; soft light's kernels are
the tone curve's loops, whose large-frame shape takes its table copy as dynamic LDS, one 1024-thread workgroup per CU)."""
import os
import re

import pytest

import cg_lib
from art_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "art_amd", "libartgpu.so")

# cg_factor_kernel<GRAD, PCV>: gradient alone, vignette alone, both; bw_mix_kernel<GAMMA, CAST>
KERNELS = [r"cg_factor_kernel<%s, ?%s>" % gp for gp in (("true", "false"), ("false", "true"), ("true", "true"))] + \
          [r"bw_mix_kernel<%s, ?%s>" % gc for gc in (("false", "false"), ("true", "false"), ("false", "true"), ("true", "true"))] + \
          [r"\bsl_apply_kernel", r"\bsl_apply_lds_kernel"]


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
        # 256-thread workgroups at full occupancy (eight waves per SIMD); the one 1024-thread workgroup per CU has four waves per SIMD
        assert r["vgprs"] <= (128 if r["max_workgroup"] == 1024 else 64), (name, r)
        assert r["static_lds_bytes"] <= cg_lib.LDS_BYTES_MAX, (name, r)


def test_no_other_creative_kernel(table):
    """the list above is the whole of the three tools: a kernel added later gets its row here"""
    mine = [n for n in table if re.search(r"\b(cg|sl|bw)_\w+_kernel", n)]
    assert len(mine) == len(KERNELS), sorted(mine)
