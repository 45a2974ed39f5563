"""CPU: what the compiler made of the capture-sharpening kernels, read from the built library's gfx950 code object (art_amd/codeobj.py), in
the pattern of tests/test_kernel_resources.py.  The Richardson-Lucy iteration runs twenty times per frame over the whole image: a spilled
register or a scratch array in it is a memory round trip per pixel and iteration."""
import os
import re

import pytest

from art_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "art_amd", "libartgpu.so")


@pytest.fixture(scope="module")
def table():
    # properties of the BUILT library.  A missing build, a code-object parser that breaks or a library without a gfx950 bundle is a failure,
    # not a skip: nothing may hide these checks.
    assert os.path.exists(LIB), "art_amd/libartgpu.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    t = codeobj.kernel_table(LIB)
    assert t, "libartgpu.so holds no gfx950 code object"
    return t


def _find(table, pattern):
    hits = {n: r for n, r in table.items() if re.search(pattern, n)}
    assert hits, f"no kernel matches {pattern!r}"
    return hits


# the iteration kernel of each stencil regime, the two-kernel forms, and the DIV / MULT steps behind the recursive gaussian's vertical pass
ITERATION = [r"rl_iter_kernel<1>", r"rl_iter_kernel<2>", r"rl_iter_kernel<3>", r"gauss_div_kernel<[123]>", r"gauss_mult_kernel<[123]>",
             r"yvv_div_kernel", r"yvv_mult_kernel", r"rl_point_kernel", r"rl_init_kernel", r"rl_final_kernel"]


@pytest.mark.parametrize("pattern", ITERATION)
def test_iteration_kernels_neither_spill_nor_use_scratch(table, pattern):
    hits = _find(table, pattern)
    if "[123]" in pattern:
        assert len(hits) == 3, sorted(hits)
    for name, r in hits.items():
        assert r["vgpr_spills"] == 0 and r["scratch_bytes"] == 0, (name, r)
        assert r["vgprs"] <= 128, (name, r)                       # 256 threads: at least four workgroups per SIMD row stay resident


def test_lds_fits_the_cu(table):
    """static LDS (the kernels take no dynamic LDS: every launch in sharpen.hip passes 0) within 160 KB, and small enough for several
    workgroups per CU: the halo loads of one hide behind the arithmetic of another"""
    for name, r in _find(table, r"rl_iter_kernel<[123]>").items():
        assert 0 < r["static_lds_bytes"] <= 160 * 1024, (name, r)
        assert r["static_lds_bytes"] <= 32 * 1024, (name, r)
    src = open(os.path.join(ROOT, "art_amd", "csrc", "sharpen.hip")).read()
    launches = re.findall(r"hipLaunchKernelGGL\(([^;]*)\);", src)
    assert launches and all(re.search(r"dim3\([^)]*\), 0, s,", l) or ", 0, s," in l for l in launches), "a launch with dynamic LDS"


def test_every_sharpening_kernel_is_in_the_code_object(table):
    for fam in ("sh_luminance_kernel", "sh_hpf_kernel", "sh_impulse_kernel", "sh_corner_kernel", "sh_multiply_kernel", "sh_count_kernel",
                "sh_radius_partial_kernel", "sh_radius_final_kernel"):
        for name, r in _find(table, fam).items():
            assert r["vgpr_spills"] == 0 and r["scratch_bytes"] == 0, (name, r)
