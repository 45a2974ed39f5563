"""CPU: what the compiler made of the Lanczos resampler, read from the built library's gfx950 code object (art_amd/codeobj.py), in the pattern
of tests/test_filmsim_resources.py.  The vertical stage keeps 3 x 16 accumulators per lane in registers with static indices: an array the
compiler could not keep there, or a spilled register, is a memory round trip per source pixel."""
import os
import re

import pytest

from art_amd import codeobj
import rs_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "art_amd", "libartgpu.so")
# the interpolated rows of a tile, 3 planes x ROWS rows x (SPAN + 1) floats
LDS_BYTES = 3 * rs_lib.ROWS * (rs_lib.SPAN + 1) * 4


@pytest.fixture(scope="module")
def table():
    # properties of the BUILT library: a missing build or a library without a gfx950 bundle is a failure, not a skip
    assert os.path.exists(LIB), "art_amd/libartgpu.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    t = codeobj.kernel_table(LIB)
    assert t, "libartgpu.so holds no gfx950 code object"
    return t


def test_both_instantiations_neither_spill_nor_use_scratch(table):
    """recorded when the kernel was written: 78 VGPRs (rows first) and 76 (columns first), 78 SGPRs each"""
    hits = {n: r for n, r in table.items() if re.search(r"resize_lanczos_kernel<(true|false)>", n)}
    assert len(hits) == 2, sorted(hits)
    for name, r in hits.items():
        print(name, r)
        assert r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["scratch_bytes"] == 0, (name, r)
        assert r["static_lds_bytes"] == LDS_BYTES == 49344, (name, r)       # three workgroups per CU (160 KiB)
        assert r["vgprs"] <= 128, (name, r)                                 # 12 waves per CU is what the LDS allows: 3 per SIMD need <= 170
        assert r["max_workgroup"] == 256, (name, r)


def test_no_other_kernel_in_the_translation_unit(table):
    """resize.hip holds exactly the two instantiations above: a new one has to be listed (and checked) here"""
    mine = [n for n in table if re.search(r"\bresize_[a-z_]*kernel|\brs_[a-z_]+_kernel", n)]
    assert len(mine) == 2, sorted(mine)
