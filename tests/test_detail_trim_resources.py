"""CPU: the trimmed kernels of the DCT detail recovery under the limits tests/test_kernel_resources.py sets for the
kernels they stand in for, read from the built library's gfx950 code objects."""
import os
import re
import shutil

import pytest

from art_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "art_amd", "libartgpu.so")


@pytest.fixture(scope="module")
def table():
    # as in tests/test_kernel_resources.py: nothing to check without a built library and the tools that read it
    if not os.path.exists(LIB):
        pytest.skip("art_amd/libartgpu.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    pytest.importorskip("msgpack")
    if shutil.which("c++filt") is None and shutil.which("llvm-cxxfilt") is None and not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-cxxfilt"):
        pytest.skip("no c++filt to demangle kernel names")
    try:
        t = codeobj.kernel_table(LIB)
    except ValueError as e:
        pytest.skip(str(e))
    if not t:
        pytest.skip("libartgpu.so holds no gfx950 code object (built for another architecture)")
    return t


@pytest.mark.parametrize("pattern,vgprs,count", [
    (r"detail_blocks_trim_kernel<[123]>", 256, 3),      # one wave per workgroup; nine blocks' LDS per CU either way
    (r"detail_gather_rows_kernel", 128, 1),             # 1024 threads
])
def test_trimmed_detail_kernels_neither_spill_nor_use_scratch(table, pattern, vgprs, count):
    hits = {n: r for n, r in table.items() if re.search(pattern, n)}
    assert len(hits) == count, sorted(hits)
    for name, r in hits.items():
        assert r["vgpr_spills"] == 0 and r["scratch_bytes"] == 0, (name, r)
        assert r["vgprs"] <= vgprs, (name, r)
