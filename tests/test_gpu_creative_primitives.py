"""GPU: sleef's scalar xsinf and xcosf as the device has them (devsleef.h: xsinf_s, xcosf_s; ARTGPU_PRIM_XSINF_S / ARTGPU_PRIM_XCOSF_S) against
tests/golden/creative.npz, recorded from the reference's own sleef.h compiled in place (tests/golden/make_golden_creative.py): 4096 arguments
over [-10, 10] and every argument the ramp branches of the fixture's gradient and vignette cases hand to the two functions.  Beside
tests/test_gpu_primitives.py, which holds the older primitives to their fixtures the same way.  Bit for bit."""
import os

import numpy as np
import pytest

from art_amd import capi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "creative.npz")


def _same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def test_xsinf_and_xcosf_equal_the_reference(gpu_ctx):
    g = np.load(GOLDEN)
    assert _same_bits(gpu_ctx.eval_primitive(capi.PRIM_XSINF_S, g["x_trig"]), g["sin_trig"])
    assert _same_bits(gpu_ctx.eval_primitive(capi.PRIM_XCOSF_S, g["x_trig"]), g["cos_trig"])
    n, k = [0, 0], 0
    while "case_%d" % k in g:
        for j, (which, prim) in enumerate((("sin", capi.PRIM_XSINF_S), ("cos", capi.PRIM_XCOSF_S))):
            args = g["%sargs_%d" % (which, k)]
            n[j] += args.size
            if args.size:
                assert _same_bits(gpu_ctx.eval_primitive(prim, args), g["%s_%d" % (which, k)]), (k, which)
        k += 1
    assert min(n) > 100, n


def test_the_older_primitives_kept_their_numbers(gpu_ctx):
    """the two ids are appended: FLOAT_TO_HALF is still 23 and still the half conversion"""
    assert (capi.PRIM_FLOAT_TO_HALF, capi.PRIM_XSINF_S, capi.PRIM_XCOSF_S) == (23, 24, 25)
    got = gpu_ctx.eval_primitive(capi.PRIM_FLOAT_TO_HALF, np.array([1.0, -2.0, 0.5], np.float32))
    assert [int(v) & 0xFFFF for v in got] == [0x3C00, 0xC000, 0x3800]
    with pytest.raises(capi.ArtGpuError):
        gpu_ctx.eval_primitive(26, np.ones(4, np.float32))
