"""GPU: the trimmed kernels of the DCT detail recovery against the kernels they replace, bit for bit.

The default form gives blocks that lie wholly inside the image a path of their own, reads tilemask_in as one register plus eight rows, leaves
out the last block row and column (nothing reads them) and gathers by rows with a table for totwt; option "dn_detail_plain" 1 runs the kernels
as they were.  Every step is the same arithmetic on the same values, so the two must agree in every bit; the new form is also held to the
stage's bound against the checker's exact transform (DCT_ABS_BOUND of tests/test_gpu_denoise.py)."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from art_amd import capi, synth

pytestmark = pytest.mark.gpu

DCT_ABS_BOUND = 0.0625      # on the 0..65535 output scale: DESIGN.md section 3, tests/test_gpu_denoise.py


@functools.lru_cache(maxsize=None)
def _rgb(w, h):
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=w + 1, noise=2048)
    planes = O.amaze(raw, synth.FILTERS_RGGB, 1.0, 4)
    for p in planes:
        p.setflags(write=False)
    return tuple(planes)


def _params(detail, thresh):
    p = capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0)
    p.luminance_detail = detail
    p.luminance_detail_threshold = thresh
    return p


def _run(ctx, w, h, plain, detail=50.0, thresh=0, scale=1.0):
    got = [p.copy() for p in _rgb(w, h)]
    ctx.set_option("dn_detail_plain", plain)
    try:
        ctx.rgb_denoise(capi.host_rgb(got), _params(detail, thresh), O.REC2020_WS, scale=scale, flags=0)
    finally:
        ctx.set_option("dn_detail_plain", 0)
    return got


@pytest.mark.parametrize("w,h,kw", [
    (72, 70, {}),                       # at most one block inside the image
    (300, 275, {}),                     # both sides multiples of 25: the last block row and column start exactly at the image's end
    (299, 276, {}),                     # just off the multiples of 25
    (517, 389, dict(detail=80.0)),      # odd sizes, width not a multiple of 4, several 64-column units per row
    (330, 260, dict(thresh=40)),        # luminanceDetailThreshold > 0: the shrink factor comes from the detail mask
    (231, 187, dict(scale=1.5)),        # blur radius 2
    (187, 231, dict(scale=2.0)),        # blur radius 1
])
def test_trimmed_detail_kernels_same_bits_as_plain(gpu_ctx, w, h, kw):
    plain = _run(gpu_ctx, w, h, 1, **kw)
    new = _run(gpu_ctx, w, h, 0, **kw)
    for name, a, b in zip("RGB", plain, new):
        nbad = int((a.view(np.uint32) != b.view(np.uint32)).sum())
        print(f"{w}x{h} {kw} {name}: {nbad} values differ between the plain and the trimmed kernels")
    # ... and each half alone (2: only the block kernel plain, 3: only the gather plain)
    halves = [_run(gpu_ctx, w, h, f, **kw) for f in (2, 3)]
    ref = O.rgb_denoise(list(_rgb(w, h)), O.default_denoise_params(luminanceDetail=kw.get("detail", 50.0), detail_thresh=kw.get("thresh", 0),
                                                                    scale=kw.get("scale", 1.0)), detail_recovery=True)
    nodetail = O.rgb_denoise(list(_rgb(w, h)), O.default_denoise_params(luminanceDetail=kw.get("detail", 50.0), detail_thresh=kw.get("thresh", 0),
                                                                         scale=kw.get("scale", 1.0)), detail_recovery=False)
    errs = [float(np.abs(g.astype(np.float64) - r.astype(np.float64)).max()) for g, r in zip(new, ref)]
    print(f"{w}x{h} {kw}: max |device - exact| = {errs} (bound {DCT_ABS_BOUND})")
    for a, b in zip(plain, new):
        assert np.array_equal(a, b)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for half in halves:
        for a, b in zip(plain, half):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert all(np.isfinite(p).all() for p in new)
    assert max(errs) <= DCT_ABS_BOUND, errs
    assert max(float(np.abs(r - nd).max()) for r, nd in zip(ref, nodetail)) > 5.0      # the stage really ran


def test_fewer_blocks_written_leaves_nothing_stale(gpu_ctx):
    """517 x 389 twice in a row on one context after a 300 x 275 frame: the block buffer is reused across calls and the trimmed block kernel
    no longer writes its last block row and column, so whatever an earlier frame left there must not reach a pixel."""
    want = _run(gpu_ctx, 517, 389, 1, detail=80.0)
    _run(gpu_ctx, 300, 275, 0)
    for rep in range(2):
        got = _run(gpu_ctx, 517, 389, 0, detail=80.0)
        for a, b in zip(want, got):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), rep
