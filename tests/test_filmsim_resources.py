"""CPU: what the compiler made of the film simulation's kernel, read from the built library's gfx950 code object (art_amd/codeobj.py), in the
pattern of tests/test_toneeq_resources.py.  The pass streams the whole image and gathers from three tables per pixel: a spilled register or a
scratch array is one more memory round trip per pixel."""
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


def test_both_instantiations_neither_spill_nor_use_scratch(table):
    hits = {n: r for n, r in table.items() if re.search(r"filmsim_kernel<(true|false)>", n)}
    assert len(hits) == 2, sorted(hits)
    for name, r in hits.items():
        print(name, r)
        assert r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["scratch_bytes"] == 0, (name, r)
        assert r["static_lds_bytes"] == 0, (name, r)                # neither gamma table nor the CLUT fits beside useful occupancy
        assert r["vgprs"] <= 64, (name, r)                          # 256 threads: eight waves per SIMD stay resident
        assert r["max_workgroup"] == 256, (name, r)


def test_no_other_kernel_in_the_translation_unit(table):
    """filmsim.hip holds exactly the two instantiations above: a new one has to be listed (and checked) here"""
    mine = [n for n in table if re.search(r"\bfilmsim_[a-z_]*kernel|\bfs_[a-z_]+_kernel", n)]
    assert len(mine) == 2, sorted(mine)
