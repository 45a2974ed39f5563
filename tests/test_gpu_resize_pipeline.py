"""GPU: the Resize tool in the per-frame pipe (artgpu_set_pipeline_resize; simpleprocess.cc:402-414 behind ImProcFunctions::process(STAGE_3))
against the same stages called one by one: artgpu_pipeline_run, artgpu_batch_run, artgpu_batch_run_io and artgpu-cli.  Bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from art_amd import capi, synth
import lc_lib
import rs_lib
from test_gpu_batch_io import BLACK, OUTM, SCALE, _sensor
from test_gpu_cli import MAT, MUL, run_cli, tone_lut
from test_gpu_pipeline import _lut, _params

pytestmark = pytest.mark.gpu
W, H, B = 416, 288, 4
FW, FH = W - 2 * B, H - 2 * B
LUT = _lut()       # (PipelineParams only points at its tone table)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _pipeline(ctx, raw, p, size=None):
    h, w = raw.shape
    ow, oh = size or (w - 2 * p.border, h - 2 * p.border)
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.full((oh, ow), float("nan"), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    ctx.synchronize()
    return [t.cpu().numpy() for t in d_img]


def _resize(ctx, frame, size, scale, mode, p, before=(), after=()):
    """entry points one by one on a device copy of `frame`: `before` on the full-size image, the resampler, `after` on the small one"""
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in frame]
    o = [torch.full((size[1], size[0]), float("nan"), device="cuda:0") for _ in range(3)]
    src, dst = capi.RGB(*[capi.device_plane(t) for t in d]), capi.RGB(*[capi.device_plane(t) for t in o])
    ws, iws = [float(v) for v in p.ws], [float(v) for v in p.iws]
    for s in before:
        s(src)
    ctx.resize_lanczos(src, dst, scale, mode, ws, iws)
    for s in after:
        s(dst)
    ctx.synchronize()
    return [t.cpu().numpy() for t in o]


def _same(got, want, what):
    assert all(np.isfinite(g).all() for g in got), what
    rs_lib.assert_same(got, want, what)


@pytest.fixture()
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("rp", [dict(dataspec=0, scale=0.37), dict(dataspec=3, width=150, height=150), dict(dataspec=1, width=600, allow_upscaling=True),
                                dict(dataspec=0, scale=1.25)], ids=["scale0.37", "fit150", "width600", "scale1.25"])
def test_pipe_with_the_setting_equals_the_pipe_then_the_resampler(gpu_ctx, rp):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=91, noise=1500)
    p = _params(LUT, 0)
    full = _pipeline(gpu_ctx, raw, p)
    par = capi.resize_params(**rp)
    imw, imh, scale = capi.resize_scale(par, FW, FH)
    assert (imw, imh) != (FW, FH) and (imw, imh) == rs_lib.resize_scale(rs_lib.params(**rp), FW, FH)[:2]
    try:
        gpu_ctx.set_pipeline_resize(par)
        got = _pipeline(gpu_ctx, raw, p, (imw, imh))
    finally:
        gpu_ctx.set_pipeline_resize(None)
    _same(got, _resize(gpu_ctx, full, (imw, imh), scale, capi.RESIZE_RGB, p), f"pipe + resize {rp}")
    again = _pipeline(gpu_ctx, raw, p)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, full)), "NULL turns the tool off again"


def test_behind_local_contrast_the_lab_planes_are_resampled(gpu_ctx):
    """with local contrast on the image is still in LAB mode when Lanczos finds it: full-size pipe without local contrast, rgb_to_lab,
    local_contrast, resize(PLANES), lab_to_rgb on the small image -- not LAB -> RGB -> LAB at full size, which gives other bits"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=92, noise=1500)
    p = _params(LUT, 0)
    upto = _pipeline(gpu_ctx, raw, p)
    curve = lc_lib.curve_lut(lc_lib.BOOST_CURVE_POINTS)
    lc_arr, keep = capi.local_contrast_regions([(60.0, curve, None)])
    p.local_contrast_enabled = 1; p.local_contrast_nregions = 1; p.local_contrast_regions = lc_arr
    with_lc = _pipeline(gpu_ctx, raw, p)
    par = capi.resize_params(dataspec=0, scale=0.5)
    imw, imh, scale = capi.resize_scale(par, FW, FH)
    try:
        gpu_ctx.set_pipeline_resize(par)
        got = _pipeline(gpu_ctx, raw, p, (imw, imh))
    finally:
        gpu_ctx.set_pipeline_resize(None)
    ws, iws = [float(v) for v in p.ws], [float(v) for v in p.iws]
    want = _resize(gpu_ctx, upto, (imw, imh), scale, capi.RESIZE_PLANES, p,
                   before=[lambda i: gpu_ctx.rgb_to_lab(i, ws), lambda i: gpu_ctx.local_contrast(i.g, [(60.0, curve, None)], 1.0)],
                   after=[lambda i: gpu_ctx.lab_to_rgb(i, iws)])
    _same(got, want, "pipe, local contrast + resize")
    round_trip = _resize(gpu_ctx, with_lc, (imw, imh), scale, capi.RESIZE_RGB, p)
    assert any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, round_trip)), "the round trip through RGB at full size is another image"
    del keep


def test_an_upscale_that_is_not_allowed_leaves_the_frame_at_full_size(gpu_ctx):
    """dataspec 3 without allow_upscaling returns 1; dataspec 1 returns a scale > 1 that simpleprocess.cc:406-407 does not apply: both give the
    bits of the setting being off, at full size"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=93, noise=1500)
    p = _params(LUT, 0)
    off = _pipeline(gpu_ctx, raw, p)
    for rp in (dict(dataspec=3, width=2000, height=2000), dict(dataspec=1, width=600), dict(dataspec=0, scale=1.000005), dict(dataspec=0, scale=0.5, enabled=False)):
        try:
            gpu_ctx.set_pipeline_resize(capi.resize_params(**rp))
            got = _pipeline(gpu_ctx, raw, p)
        finally:
            gpu_ctx.set_pipeline_resize(None)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, off)), rp


def test_setting_off_after_on_equals_a_fresh_context(gpu_ctx, ctx):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=94, noise=1500)
    p = _params(LUT, 0)
    fresh = _pipeline(ctx, raw, p)
    par = capi.resize_params(dataspec=0, scale=0.25)
    imw, imh, _ = capi.resize_scale(par, FW, FH)
    gpu_ctx.set_pipeline_resize(par)
    try:
        small = _pipeline(gpu_ctx, raw, p, (imw, imh))
    finally:
        gpu_ctx.set_pipeline_resize(None)
    assert small[0].shape == (imh, imw)
    after = _pipeline(gpu_ctx, raw, p)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(after, fresh))


def test_wrong_out_size_unsupported_scale_and_degenerate_result_are_refused_before_any_stage(gpu_ctx):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=95, noise=1500)
    p = _params(LUT, 0)
    d_raw = torch.from_numpy(raw).to("cuda:0")
    cases = ((dict(dataspec=0, scale=0.5), (FW, FH), r"^\[-1\].*output must be 204x140"),        # the full size is no longer the output's
             (dict(dataspec=0, scale=0.5), (203, 140), r"^\[-1\].*output must be 204x140"),
             (dict(dataspec=0, scale=1 / 32), (13, 9), r"^\[-4\].*resize"),                       # outside the supported range
             (dict(dataspec=0, scale=0.001), (1, 1), r"^\[-1\].*leaves no image"))                # int(408 * 0.001 + 0.5) = 0
    for rp, (ow, oh), pattern in cases:
        d = [torch.full((oh, ow), 7.0, device="cuda:0") for _ in range(3)]
        gpu_ctx.set_pipeline_resize(capi.resize_params(**rp))
        try:
            before = gpu_ctx.scratch_bytes()
            with pytest.raises(capi.ArtGpuError, match=pattern):
                gpu_ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d]))
            assert gpu_ctx.scratch_bytes() == before, "a refused frame takes no scratch"
        finally:
            gpu_ctx.set_pipeline_resize(None)
        gpu_ctx.synchronize()
        assert all((t.cpu().numpy() == 7.0).all() for t in d), rp


def test_batch_run_on_two_lanes(ctx):
    p = _params(LUT, 0)
    raws = [synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=s, noise=1500) for s in (96, 97, 98)]
    par = capi.resize_params(dataspec=3, width=200, height=200)
    imw, imh, _ = capi.resize_scale(par, FW, FH)
    ctx.set_pipeline_resize(par)
    one = [_pipeline(ctx, r, p, (imw, imh)) for r in raws]
    ctx.set_batch_lanes(2)
    outs = [[np.zeros((imh, imw), np.float32) for _ in range(3)] for _ in raws]
    ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
    for wnt, o in zip(one, outs):
        _same(o, wnt, "batch lane")


@pytest.mark.parametrize("fmt", [(16, False), (8, False)], ids=["u16", "u8"])
def test_batch_run_io_two_lanes_three_frames(ctx, fmt):
    """equals pipeline_run (with the setting), rgb2out_matrix, get_scanlines at imw x imh"""
    w, h = 520, 392
    p = _params(LUT, 0)
    sensors = [_sensor(w, h, 31 + k) for k in range(3)]
    par = capi.resize_params(dataspec=0, scale=0.37)
    imw, imh, _ = capi.resize_scale(par, w - 2 * B, h - 2 * B)
    ctx.set_pipeline_resize(par)
    want = []
    for s in sensors:
        d_cfa = torch.empty((h, w), dtype=torch.float32, device="cuda")
        d_img = [torch.empty((imh, imw), dtype=torch.float32, device="cuda") for _ in range(3)]
        img = capi.RGB(*[capi.device_plane(t) for t in d_img])
        chmax = ctx.scale_colors(s, synth.FILTERS_RGGB, None, BLACK, SCALE, capi.device_plane(d_cfa))
        ctx.pipeline_run(capi.device_plane(d_cfa), p, img)
        ctx.rgb2out_matrix(img, img, OUTM, True, None)
        want.append((ctx.get_scanlines(img, fmt[0], fmt[1]), chmax))
    outs = [np.zeros((imh, imw, 3), np.uint8 if fmt[0] == 8 else np.uint16) for _ in sensors]
    ctx.set_batch_lanes(2)
    res = ctx.batch_run_io([capi.sensor_frame(s, BLACK, SCALE) for s in sensors], p, [capi.scanline_frame(o, OUTM, None, is_float=fmt[1]) for o in outs])
    for k, (o, (scan, chmax)) in enumerate(zip(outs, want)):
        assert res[k].status == 0
        assert [float(v) for v in res[k].chmax] == chmax, k
        assert scan.shape[:2] == (imh, imw) and np.array_equal(o.view(np.uint8), scan.view(np.uint8)), k
    assert not np.array_equal(outs[0], outs[1])


def test_cli_resize_fit(gpu_ctx, tmp_path):
    """artgpu-cli --resize-fit (ImProcFunctions::resizeScale and ImProcFunctions::resize in the C++ mirror behind process(STAGE_3)) equals the
    same stages called one by one"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=99, noise=1200)
    info, got = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--resize-fit", "150x150"])
    par = capi.resize_params(dataspec=3, width=150, height=150)
    imw, imh, scale = capi.resize_scale(par, FW, FH)
    assert (info["out_width"], info["out_height"]) == (imw, imh) == (150, 103) and got.shape == (imh, imw, 3)
    d_raw = torch.from_numpy(raw).to("cuda:0")
    dem = [torch.empty((H, W), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    planes = capi.RGB(*[capi.device_plane(t) for t in dem])
    gpu_ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), synth.FILTERS_RGGB, 1.0, B, planes)
    d_img = [torch.empty((FH, FW), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    gpu_ctx.get_image(planes, B, B, MUL, True, None, img)
    gpu_ctx.convert_color_space(img, MAT)
    gpu_ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    gpu_ctx.tone_curve(img, tone_lut(), 1.0, True)
    d_out = [torch.empty((imh, imw), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    import oracle_lib as O
    gpu_ctx.resize_lanczos(img, capi.RGB(*[capi.device_plane(t) for t in d_out]), scale, capi.RESIZE_RGB, O.REC2020_WS_D, O.REC2020_IWS_D)
    gpu_ctx.synchronize()
    want = np.stack([np.rint(np.clip(t.cpu().numpy(), 0, 65535)).astype(np.uint16) for t in d_out], axis=-1)
    assert np.array_equal(got, want)
    # a box the frame already fits: the full size, as without the option
    info2, same = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--resize-fit", "5000x5000"])
    _, without = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3"])
    assert (info2["out_width"], info2["out_height"]) == (FW, FH) and np.array_equal(same, without)
