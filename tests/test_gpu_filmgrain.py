"""GPU: artgpu_add_noise / artgpu_film_grain / artgpu_grain_indices / artgpu_set_pipeline_film_grain (ImProcFunctions::filmGrain, ipgrain.cc:33-98;
add_noise and the frame around a NOISE region, ipsmoothing.cc:565-695, 933-1067) against the CPU checker (tests/fg_lib.py:
tests/emul/filmgrain_ref.cc, which steps rng.h's 64-bit generator serially and knows no jump-ahead).

Every pixel is compared as a bit pattern.  The inputs are NaN-free: that is the tool's contract."""
import ctypes as C

import numpy as np
import pytest
import torch

from art_amd import capi, synth
import fg_lib
import fs_lib
import layout_lib
from test_gpu_pipeline import _lut, _params
from test_gpu_textureboost import _pipe_regions

pytestmark = pytest.mark.gpu

TW, TH = fg_lib.TILE_W, fg_lib.TILE_H
# smaller than the kernel in one or both directions (the clamp hits on both sides); across tile edges in both directions with a last run
# shorter than a lane's
SMALL = [(1, 1), (2, 5), (7, 3)]
TILES = [(TW + 1, TH + 1), (2 * TW + 3, 9)]
CHANNELS = [fg_lib.L, fg_lib.C_, fg_lib.LC]
COARSENESS = [0, 30, 100]              # sz 3, 5, 7 at scale 1
WS = fg_lib.WS


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(img):
    return [torch.from_numpy(np.array(a, dtype=np.float32)).to("cuda:0") for a in img]


def _rgb(d):
    return capi.RGB(*[capi.device_plane(t) for t in d])


def _add_noise(ctx, img, strength, coarseness, channel, scale=1.0, mask=None, first=True, last=True):
    d = _dev(img)
    ctx.add_noise(_rgb(d), strength, coarseness, channel, WS, scale, mask=mask, first=first, last=last)
    ctx.synchronize()
    return [t.cpu().numpy() for t in d]


@pytest.mark.parametrize("coarseness", COARSENESS)
@pytest.mark.parametrize("channel", CHANNELS)
@pytest.mark.parametrize("size", SMALL + TILES, ids=lambda s: "%dx%d" % s)
def test_add_noise_equals_the_checker(gpu_ctx, size, channel, coarseness):
    w, h = size
    img, want = fg_lib.case(w, h, 60, coarseness, channel)
    fg_lib.assert_same(_add_noise(gpu_ctx, img, 60, coarseness, channel), want, f"{w}x{h} channel {channel} coarseness {coarseness}")


@pytest.mark.parametrize("channel", CHANNELS)
@pytest.mark.parametrize("size", [(7, 3), (TW + 1, TH + 1)], ids=lambda s: "%dx%d" % s)
def test_scale_2(gpu_ctx, size, channel):
    w, h = size
    for coarseness in COARSENESS:
        img, want = fg_lib.case(w, h, 60, coarseness, channel, scale=2.0)
        fg_lib.assert_same(_add_noise(gpu_ctx, img, 60, coarseness, channel, scale=2.0), want, f"{w}x{h} channel {channel} coarseness {coarseness} scale 2")


@pytest.mark.parametrize("channel", CHANNELS)
def test_strength_0_still_blends_and_round_trips(gpu_ctx, channel):
    """sf == 0: max(a + 0 * n, 0), the YUV round trip, the blend and both normalise passes still run"""
    w, h = TW + 1, TH + 1
    img, want = fg_lib.case(w, h, 0, 30, channel, family="wild")
    got = _add_noise(gpu_ctx, img, 0, 30, channel)
    fg_lib.assert_same(got, want, f"strength 0 channel {channel}")
    assert any(not np.array_equal(_bits(g), _bits(a)) for g, a in zip(got, img)), "negatives are clamped, the round trip rounds"


@pytest.mark.parametrize("channel", CHANNELS)
@pytest.mark.parametrize("size", [(7, 3), (2 * TW + 3, 9)], ids=lambda s: "%dx%d" % s)
def test_negatives_zeros_and_super_white(gpu_ctx, size, channel):
    w, h = size
    for coarseness in (0, 100):
        img, want = fg_lib.case(w, h, 80, coarseness, channel, family="wild")
        assert min(a.min() for a in img) < 0 and max(a.max() for a in img) > 65535 and any((a == 0).any() for a in img)
        fg_lib.assert_same(_add_noise(gpu_ctx, img, 80, coarseness, channel), want, f"wild {w}x{h} channel {channel} coarseness {coarseness}")


@pytest.mark.parametrize("size", [(1, 1), (7, 3), (TW + 1, TH + 1)], ids=lambda s: "%dx%d" % s)
def test_host_planes_give_the_same_bits(gpu_ctx, size):
    w, h = size
    for channel, coarseness in ((fg_lib.L, 30), (fg_lib.C_, 100), (fg_lib.LC, 0)):
        img, want = fg_lib.case(w, h, 60, coarseness, channel)
        host = [np.array(a, dtype=np.float32) for a in img]
        gpu_ctx.add_noise(capi.host_rgb(host), 60, coarseness, channel, WS)
        fg_lib.assert_same(host, want, f"{w}x{h} (host planes)")


@pytest.mark.parametrize("layout", list(layout_lib.LAYOUTS))
@pytest.mark.parametrize("size", [(7, 3), (TW + 1, TH + 1)], ids=lambda s: "%dx%d" % s)
def test_padded_and_shifted_device_planes(gpu_ctx, size, layout):
    """row-padded, offset device planes: every word outside the window still holds the poison"""
    w, h = size
    for channel, coarseness in ((fg_lib.L, 100), (fg_lib.LC, 30)):
        img, want = fg_lib.case(w, h, 60, coarseness, channel)
        ar = layout_lib.arena(layout_lib.LAYOUTS[layout], img)
        gpu_ctx.add_noise(ar.rgb, 60, coarseness, channel, WS)
        gpu_ctx.synchronize()
        fg_lib.assert_same(layout_lib.check(ar, f"{w}x{h} {layout}"), want, f"{w}x{h} channel {channel}, layout {layout}")


@pytest.mark.parametrize("device_mask", [True, False])
@pytest.mark.parametrize("channel", CHANNELS)
def test_masks_cropped_and_full_copy(gpu_ctx, channel, device_mask):
    """a box under half the frame: the region works on the crop and the draw numbers follow the crop's raster; a box over half: the frame"""
    w, h = 2 * TW + 3, 40
    img = fg_lib.scene(w, h, "wild")
    for box, cropped in (((TW - 3, 5, TW + 30, 27), 1), ((2, 1, w - 1, h - 2), 0)):
        m = fg_lib.box_mask(w, h, *box)
        want, boxes = fg_lib.smoothing_noise(img, [(70, 30, channel)], masks=[m])
        assert boxes[0][4] == cropped and (cropped == 0 or tuple(boxes[0][:4]) == box)
        dm = torch.from_numpy(m).to("cuda:0")
        got = _add_noise(gpu_ctx, img, 70, 30, channel, mask=capi.device_plane(dm) if device_mask else capi.host_plane(m))
        fg_lib.assert_same(got, want, f"box {box} channel {channel}")
        # outside the box a pixel only sees the normalise round trip
        if cropped:
            rt = (np.asarray(img[0]) * np.float32(1.0 / 65535.0)) * np.float32(65535.0)
            assert np.array_equal(_bits(got[0][0]), _bits(rt[0]))


def test_an_empty_mask_skips_the_region(gpu_ctx):
    w, h = 33, 9
    img = fg_lib.scene(w, h)
    m = np.zeros((h, w), np.float32)                # (the descriptor holds the address only: the array has to outlive the call)
    got = _add_noise(gpu_ctx, img, 70, 30, fg_lib.L, mask=capi.host_plane(m))
    want = [(np.asarray(a) * np.float32(1.0 / 65535.0)) * np.float32(65535.0) for a in img]
    fg_lib.assert_same(got, want, "empty mask")


@pytest.mark.parametrize("grid", [1, 2, 3])
@pytest.mark.parametrize("channel", CHANNELS)
def test_a_workgroup_that_walks_many_tiles(channel, grid):
    """option fg_grid: 5 x 3 tiles on 1, 2 or 3 workgroups, so a workgroup walks a whole tile row, wraps into the next row (in mid-chunk with
    2) and meets the clamps at both edges: a run's generator state is carried from tile to tile where its draw number moves on by TILE_W and
    comes from the full jump everywhere else.  Same bits as the checker and as the default grid"""
    w, h = 4 * TW + 3, 2 * TH + 1
    ctx = capi.Context(0)
    try:
        for coarseness in (0, 100):
            img, want = fg_lib.case(w, h, 60, coarseness, channel, family="wild")
            ctx.set_option("fg_grid", grid)
            got = _add_noise(ctx, img, 60, coarseness, channel)
            ctx.set_option("fg_grid", 0)
            fg_lib.assert_same(got, want, f"fg_grid {grid} channel {channel} coarseness {coarseness}")
            fg_lib.assert_same(_add_noise(ctx, img, 60, coarseness, channel), want, f"default grid channel {channel} coarseness {coarseness}")
        # a crop that starts inside a tile column of the frame: the tiles are the crop's
        m = fg_lib.box_mask(w, h, 5, 3, 5 + 2 * TW + 9, 3 + TH + 2)
        src = fg_lib.scene(w, h, "wild")
        want, boxes = fg_lib.smoothing_noise(src, [(70, 30, channel)], masks=[m])
        assert boxes[0][4] == 1
        ctx.set_option("fg_grid", grid)
        fg_lib.assert_same(_add_noise(ctx, src, 70, 30, channel, mask=capi.host_plane(m)), want, f"fg_grid {grid}, cropped")
        with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
            ctx.set_option("fg_grid", -1)
    finally:
        ctx.close()


@pytest.mark.parametrize("color", [False, True])
def test_film_grain_defaults(gpu_ctx, color):
    """iso 400, strength 50: three LUMINANCE regions, with colour a CHROMINANCE region ahead of them; the loop of add_noise calls gives the
    same bits; info is the checker's derivation"""
    w, h = TW + 9, TH + 5
    img = fg_lib.scene(w, h, "wild")
    want, regs = fg_lib.film_grain(img, 400, 50, color)
    assert len(regs) == (4 if color else 3)
    d = _dev(img)
    info = gpu_ctx.film_grain(_rgb(d), capi.film_grain_params(400, 50, color), WS, 1.0, True, want_info=True)
    gpu_ctx.synchronize()
    got = [t.cpu().numpy() for t in d]
    fg_lib.assert_same(got, want, f"film grain, colour {color}")
    mine = info.regions()
    assert [m[:5] for m in mine] == [r[:5] for r in regs]
    assert all(_bits(m[5]) == _bits(r[5]) for m, r in zip(mine, regs))
    d2 = _dev(img)
    for i, r in enumerate(regs):
        gpu_ctx.add_noise(_rgb(d2), r[1], r[2], r[0], WS, 1.0, first=i == 0, last=i == len(regs) - 1)
    gpu_ctx.synchronize()
    fg_lib.assert_same([t.cpu().numpy() for t in d2], got, "the loop of add_noise calls")


def test_film_grain_preview_scale_2_and_disabled(gpu_ctx):
    w, h = 70, 20
    img = fg_lib.scene(w, h)
    want, regs = fg_lib.film_grain(img, 3200, 100, True, output_pipeline=False, scale=2.0)
    assert len(regs) == 3                       # colour + ceil(3 / 2) levels
    d = _dev(img)
    gpu_ctx.film_grain(_rgb(d), capi.film_grain_params(3200, 100, True), WS, 2.0, False)
    gpu_ctx.synchronize()
    fg_lib.assert_same([t.cpu().numpy() for t in d], want, "preview, scale 2")
    d = _dev(img)
    info = gpu_ctx.film_grain(_rgb(d), capi.film_grain_params(enabled=False), WS, want_info=True)
    gpu_ctx.synchronize()
    assert info.nregions == 0 and all(np.array_equal(_bits(t.cpu().numpy()), _bits(a)) for t, a in zip(d, img)), "disabled: returns at once"


@pytest.mark.parametrize("first", [0, 2 ** 24 - 3, 3 * 8256 * 5504 - 5, 3 * 2 ** 27 - 2])
def test_grain_indices_equal_serial_stepping(gpu_ctx, first):
    n = 257
    for seed in (42, 144):
        _, state = fg_lib.table(seed)
        want = fg_lib.draws(state, first, n)
        got = gpu_ctx.grain_indices(state & fg_lib.MASK48, first, n)
        assert np.array_equal(got, want), (seed, first, int((got != want).sum()))


def test_unsupported_and_invalid_calls_leave_the_image_alone(gpu_ctx):
    w, h = 33, 9
    img = fg_lib.scene(w, h)
    d = _dev(img)
    rgb = _rgb(d)
    for kw, code in ((dict(scale=0.5), -4), (dict(strength=101), -4), (dict(strength=-1), -4), (dict(coarseness=101), -4), (dict(coarseness=-1), -4),
                     (dict(channel=3), -1), (dict(channel=-1), -1), (dict(scale=float("nan")), -1), (dict(scale=0.0), -1), (dict(ws=None), -1)):
        a = dict(strength=50, coarseness=30, channel=fg_lib.L, ws=WS, scale=1.0)
        a.update(kw)
        with pytest.raises(capi.ArtGpuError, match=r"^\[%d\]" % code):
            gpu_ctx.add_noise(rgb, a["strength"], a["coarseness"], a["channel"], a["ws"], a["scale"])
    wrong_size = np.ones((h, w + 1), np.float32)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\].*mask"):
        gpu_ctx.add_noise(rgb, 50, 30, fg_lib.L, WS, mask=capi.host_plane(wrong_size))
    for p, scale, code in ((capi.film_grain_params(iso=99), 1.0, -4), (capi.film_grain_params(iso=6401), 1.0, -4), (capi.film_grain_params(strength=101), 1.0, -4),
                           (capi.film_grain_params(strength=-1), 1.0, -4), (capi.film_grain_params(), 0.99, -4), (None, 1.0, -1)):
        with pytest.raises(capi.ArtGpuError, match=r"^\[%d\]" % code):
            gpu_ctx.film_grain(rgb, p, WS, scale)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
        gpu_ctx.film_grain(rgb, capi.film_grain_params(), None)
    # a working area with 3 * ww * hh >= 2^32: only the descriptor is that large, nothing is read
    huge = capi.Plane(d[0].data_ptr(), 65536, 21846, 65536 * 4, 1)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\].*2\^32"):
        gpu_ctx.add_noise(capi.RGB(huge, huge, huge), 50, 30, fg_lib.L, WS)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\].*2\^32"):
        gpu_ctx.film_grain(capi.RGB(huge, huge, huge), capi.film_grain_params(), WS)
    for bad in ((0, -1, 4), (0, 0, 0), (0, 2 ** 32 - 1, 2)):
        with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
            gpu_ctx.grain_indices(*bad)
    gpu_ctx.synchronize()
    assert all(np.array_equal(_bits(t.cpu().numpy()), _bits(a)) for t, a in zip(d, img))


def test_same_call_twice_and_scratch_returns_to_its_base():
    ctx = capi.Context(0)
    try:
        ctx.trim_scratch()
        base = ctx.scratch_bytes()
        w, h = TW + 1, TH + 1
        img, want = fg_lib.case(w, h, 60, 100, fg_lib.C_)
        a = _add_noise(ctx, img, 60, 100, fg_lib.C_)
        b = _add_noise(ctx, img, 60, 100, fg_lib.C_)
        fg_lib.assert_same(a, want, "first call")
        fg_lib.assert_same(b, a, "second call")
        assert ctx.scratch_bytes() > base
        ctx.trim_scratch()
        assert ctx.scratch_bytes() == base
        fg_lib.assert_same(_add_noise(ctx, img, 60, 100, fg_lib.C_), want, "after trim_scratch")
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the per-frame pipe
# ---------------------------------------------------------------------------------------------------------------------------------------
W, H = 392, 296


def _pipeline(ctx, raw, p):
    h, w = raw.shape
    b = p.border
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    ctx.synchronize()
    return [t.cpu().numpy() for t in d_img]


def test_pipeline_between_texture_boost_and_film_simulation(gpu_ctx):
    """texture boost ahead, film simulation and the tone curve behind: the frame equals the pipe up to texture boost, then the tools one by one"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=91, noise=1500)
    lut = _lut()
    p = _params(lut, 0)
    p.denoise_enabled = 0
    regions, arr, keep = _pipe_regions(W, H)
    p.texture_boost_enabled = 1; p.texture_boost_nregions = len(regions); p.texture_boost_regions = arr
    never = _pipeline(gpu_ctx, raw, p)
    p.tone_enabled = 0
    upto = _pipeline(gpu_ctx, raw, p)
    p.tone_enabled = 1
    clut = gpu_ctx.clut(fs_lib.clut("look", 9), 9)
    fp = fs_lib.capi_params(fs_lib.params(0.35, True))
    gp = capi.film_grain_params(800, 60, True)
    try:
        gpu_ctx.set_pipeline_film_simulation(clut, fp, after_tone_curve=False)
        gpu_ctx.set_pipeline_film_grain(gp)
        got = _pipeline(gpu_ctx, raw, p)
        gpu_ctx.set_pipeline_film_grain(None)
        no_grain = _pipeline(gpu_ctx, raw, p)
        # a refused setting fails in the plan, before any stage writes: the output planes keep what they held
        gpu_ctx.set_pipeline_film_grain(capi.film_grain_params(50, 60, False))
        d_raw = torch.from_numpy(raw).to("cuda:0")
        d_img = [torch.full((H - 8, W - 8), 7.0, dtype=torch.float32, device="cuda:0") for _ in range(3)]
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\].*film grain"):
            gpu_ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
        gpu_ctx.synchronize()
        assert all(bool((t == 7.0).all()) for t in d_img)
        # a disabled tool is off
        gpu_ctx.set_pipeline_film_grain(capi.film_grain_params(800, 60, True, enabled=False))
        disabled = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_film_grain(None)
        gpu_ctx.set_pipeline_film_simulation(None)
    d = _dev(upto)
    img = _rgb(d)
    ws = [float(v) for v in p.ws]
    gpu_ctx.film_grain(img, gp, ws, 1.0, True)
    gpu_ctx.film_simulation(img, clut, fp)
    gpu_ctx.tone_curve(img, lut, 1.0, True)
    gpu_ctx.synchronize()
    want = [t.cpu().numpy() for t in d]
    clut.close()
    assert all(np.isfinite(g).all() for g in got)
    fg_lib.assert_same(got, want, "pipe with film grain")
    assert not np.array_equal(got[1], no_grain[1])
    fg_lib.assert_same(disabled, no_grain, "enabled == 0")
    again = _pipeline(gpu_ctx, raw, p)
    fg_lib.assert_same(again, never, "NULL turns the tool off again")
    del keep
