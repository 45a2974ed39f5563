"""CPU: what the compiler made of the tone equalizer's kernels, read from the built library's gfx950 code object (art_amd/codeobj.py), in the
pattern of tests/test_sharpen_resources.py.  Every one of them is a streaming pass over the whole image: a spilled register or a scratch array
is a memory round trip per pixel."""
import os
import re

import pytest

from art_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "art_amd", "libartgpu.so")


@pytest.fixture(scope="module")
def table():
    # properties of the BUILT library: a missing build or a library without a gfx950 bundle is a failure, not a skip
    assert os.path.exists(LIB), "art_amd/libartgpu.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    t = codeobj.kernel_table(LIB)
    assert t, "libartgpu.so holds no gfx950 code object"
    return t


# pattern -> instantiations: te_prepare (Y, log, posterise), te_detail_finish (with and without the posterise), te_apply (Y from the pixel, from the
# Y plane, from the last filter's up-sample) x (one thread per group of four, one pixel per lane)
KERNELS = {r"te_prepare_kernel<[012]>": 3, r"te_detail_finish_kernel<(true|false)>": 2, r"te_apply_kernel<[012], (true|false)>": 6}


@pytest.mark.parametrize("pattern", list(KERNELS))
def test_kernels_neither_spill_nor_use_scratch(table, pattern):
    hits = {n: r for n, r in table.items() if re.search(pattern, n)}
    assert len(hits) == KERNELS[pattern], sorted(hits)
    for name, r in hits.items():
        print(name, r)
        assert r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["scratch_bytes"] == 0, (name, r)
        assert r["static_lds_bytes"] == 0, (name, r)                # the 256 KB table is read through L2, nothing is staged in LDS
        assert r["vgprs"] <= 64, (name, r)                          # 256 threads: eight waves per SIMD stay resident
        assert r["sgprs"] <= 102, (name, r)
        assert r["max_workgroup"] == 256, (name, r)


def test_no_other_kernel_in_the_translation_unit(table):
    """toneequalizer.hip holds exactly the eleven kernels above: a new instantiation has to be listed (and checked) here"""
    mine = [n for n in table if re.search(r"\bte_[a-z_]+_kernel", n)]
    assert len(mine) == sum(KERNELS.values()), sorted(mine)
