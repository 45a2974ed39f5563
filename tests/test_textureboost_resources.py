"""CPU: what the compiler made of the texture-boost kernels, read from the built library's gfx950 code object (art_amd/codeobj.py), in the
pattern of tests/test_sharpen_resources.py.  Every kernel of the tool runs once or more per iteration over the whole (up to 1.33 x 1.33
upscaled) plane: a spilled register or a scratch array in one of them is a memory round trip per pixel."""
import os
import re

import pytest

from art_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "art_amd", "libartgpu.so")

KERNELS = [r"tb_prepare_kernel", r"tb_min_final_kernel", r"tb_conv_kernel<3>", r"tb_conv_kernel<5>", r"tb_conv_kernel<7>", r"tb_conv_kernel<9>",
           r"tb_gf_subsample_kernel", r"tb_gf_ab_kernel", r"tb_gf_finish_kernel", r"tb_combine_kernel", r"tb_downscale_kernel"]


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


def test_no_other_texture_boost_kernel(table):
    """the list above is the whole file: a kernel added later gets its row here"""
    mine = [n for n in table if re.search(r"\btb_\w+_kernel", n)]
    assert len(mine) == len(KERNELS), sorted(mine)


def test_convolution_tile_fits_several_workgroups_per_cu(table):
    """64 x 16 pixels and a halo of K / 2: static LDS only, a few KB, so the halo loads of one workgroup hide behind the sums of another"""
    for k in (3, 5, 7, 9):
        (name, r), = [(n, r) for n, r in table.items() if f"tb_conv_kernel<{k}>" in n]
        lw, lh = 64 + 2 * (k // 2), 16 + 2 * (k // 2)
        assert r["static_lds_bytes"] == lh * (lw + 1) * 4, (name, r)
        assert r["static_lds_bytes"] <= 16 * 1024, (name, r)
