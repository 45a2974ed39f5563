"""CPU: what the compiler made of the impulse noise reduction's and the defringe kernels, read from the built library's gfx950 code object
(art_amd/codeobj.py), in the pattern of tests/test_creative_resources.py.  The two sparse kernels keep a pixel's window sums on one lane: a
spilled register or a scratch array would put memory traffic into a loop of up to 441 taps.  Their tiles live in static LDS, bounded by the
constants of impulse.h / defringe.h (mirrored below), which have to leave room for several workgroups per CU."""
import os
import re

import pytest

from art_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "art_amd", "libartgpu.so")
CSRC = os.path.join(ROOT, "art_amd", "csrc")

LDS_PER_CU = 160 * 1024          # gfx950
KERNELS = [r"\bimp_correct_kernel", r"\bdf_gauss3x3_kernel", r"df_chroma_kernel<true>", r"df_chroma_kernel<false>", r"\bdf_finish_kernel",
           r"\bdf_average_kernel", r"\bdf_scatter_kernel"]


def _constant(header, name):
    """a `constexpr int NAME = <expression of integers and earlier constants>` of a header, evaluated"""
    text = open(os.path.join(CSRC, header)).read()
    env = {}
    for m in re.finditer(r"constexpr int ([^;]+);", text):
        for part in m.group(1).split(","):
            k, v = part.split("=")
            env[k.strip()] = eval(v, {"__builtins__": {}}, env)
    return env[name]


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
        assert r["vgprs"] <= 64, (name, r)          # 256-thread workgroups at full occupancy (eight waves per SIMD)


def test_static_lds_within_the_headers_constants(table):
    imp = next(r for n, r in table.items() if re.search(r"\bimp_correct_kernel", n))
    avg = next(r for n, r in table.items() if re.search(r"\bdf_average_kernel", n))
    imp_max, df_max = _constant("impulse.h", "IMP_LDS_BYTES"), _constant("defringe.h", "DF_LDS_BYTES")
    print(f"imp_correct_kernel: {imp['static_lds_bytes']} bytes of LDS (IMP_LDS_BYTES {imp_max}); df_average_kernel: {avg['static_lds_bytes']} (DF_LDS_BYTES {df_max})")
    assert 0 < imp["static_lds_bytes"] <= imp_max
    assert 0 < avg["static_lds_bytes"] <= df_max
    assert 2 * df_max <= LDS_PER_CU, "the averaging kernel's tile must leave room for at least two workgroups per CU"
    assert 4 * avg["static_lds_bytes"] <= LDS_PER_CU, "defringe.h says four workgroups per CU"
    assert _constant("defringe.h", "DF_MAX_HALFWIN") == 11      # ARTGPU_DEFRINGE_MAX_HALFWIN


def test_no_other_impulse_or_defringe_kernel(table):
    """the list above is the whole of the two tools: a kernel added later gets its row here"""
    mine = [n for n in table if re.search(r"\b(imp|df)_\w+_kernel", n)]
    assert len(mine) == len(KERNELS), sorted(mine)
