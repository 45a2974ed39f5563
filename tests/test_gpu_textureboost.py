"""GPU: artgpu_texture_boost_plane / artgpu_texture_boost (ImProcFunctions::textureBoost, iptextureboost.cc:37-248) against the CPU checker
(tests/tb_lib.py: tests/emul/textureboost_ref.cc around the oracle's guided filter, bilinear rescale, pow_F and YUV switch).

The tool has no device-side libm call and its one reduction is a minimum, so every case is compared bit for bit: the planes and every field
of artgpu_texture_boost_info.  The convolution of the sub-pixel radii is exact against the checker's direct sum, which is its definition
(the reference's FFTW product differs from it by FFT rounding: tests/test_textureboost_checker.py bounds the distance).  The cases and the
branches they take are listed in tb_lib.PLANE_CASES / TOOL_CASES and checked from the checker's counters in test_textureboost_checker.py."""
import json
import subprocess

import numpy as np
import pytest
import torch

from art_amd import capi, synth
import oracle_lib as O
import tb_lib
from test_gpu_cli import CLI, MAT, MUL, read_ppm16, run_cli, tone_lut
from test_gpu_pipeline import _lut, _params

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _device_plane(ctx, Y, stride_pad=0, **kw):
    """artgpu_texture_boost_plane on a device-resident copy (rows stride_pad floats longer than w); returns (plane, info)"""
    h, w = Y.shape
    buf = torch.full((h, w + stride_pad), float("nan"), dtype=torch.float32, device="cuda:0")
    view = buf[:, :w]
    view.copy_(torch.from_numpy(np.array(Y, dtype=np.float32)))
    info = ctx.texture_boost_plane(capi.device_plane(view), kw["strength"], kw["threshold"], kw.get("iterations", 1), kw.get("scale", 1.0),
                                   kw.get("high_detail", True), want_info=True)
    ctx.synchronize()
    if stride_pad:
        assert bool(torch.isnan(buf[:, w:]).all()), "wrote past the row"
    return view.cpu().numpy(), info


def _device_tool(ctx, img, regions, to_rgb, stride_pad=0, device_masks=True, want_info=True):
    """artgpu_texture_boost on device-resident planes; masks on the device (padded rows as well) or on the host"""
    h, w = img[0].shape
    buf = torch.full((3, h, w + stride_pad), float("nan"), dtype=torch.float32, device="cuda:0")
    views = [buf[c, :, :w] for c in range(3)]
    for v, a in zip(views, img):
        v.copy_(torch.from_numpy(np.array(a, dtype=np.float32)))
    keep, regs = [], []
    for s, t, it, m in regions:
        pl = None
        if m is not None and device_masks:
            mb = torch.full((h, w + 5), float("nan"), dtype=torch.float32, device="cuda:0")
            mb[:, :w].copy_(torch.from_numpy(np.array(m)))
            keep.append(mb)
            pl = capi.device_plane(mb[:, :w])
        elif m is not None:
            hm = np.array(m, dtype=np.float32)
            keep.append(hm)
            pl = capi.host_plane(hm)
        regs.append((s, t, it, pl))
    info = ctx.texture_boost(capi.RGB(*[capi.device_plane(v) for v in views]), regs, O.REC2020_WS_D, 1.0, True, to_rgb, want_info=want_info)
    ctx.synchronize()
    del keep
    if stride_pad:
        assert bool(torch.isnan(buf[:, :, w:]).all()), "wrote past the row"
    return [v.cpu().numpy() for v in views], info


def _assert_same(got, want, what):
    bad = [int((_bits(g) != _bits(w)).sum()) for g, w in zip(got, want)]
    print(f"texture boost {what}: values that differ from the checker, per plane: {bad}")
    assert not any(bad), (what, bad)


@pytest.mark.parametrize("name", list(tb_lib.PLANE_CASES))
def test_plane_and_info_equal_the_checker(gpu_ctx, name):
    Y, kw, want, want_info, _ = tb_lib.plane_case(name)
    # host plane
    host = np.array(Y)
    info = gpu_ctx.texture_boost_plane(capi.host_plane(host), kw["strength"], kw["threshold"], kw["iterations"], kw["scale"], True, want_info=True)
    print(f"texture boost {name}: info {tb_lib.info_fields(info)} checker {tb_lib.info_fields(want_info)}")
    assert tb_lib.info_fields(info) == tb_lib.info_fields(want_info)
    _assert_same([host], [want], name)
    assert not np.array_equal(host, Y), "the call changed nothing"
    if name in tb_lib.STRIDED_CASES:
        got, dinfo = _device_plane(gpu_ctx, Y, stride_pad=7, **kw)
        assert bytes(dinfo) == bytes(info)
        _assert_same([got], [want], name + " (device-resident, padded rows)")


@pytest.mark.parametrize("name", list(tb_lib.TOOL_CASES))
def test_whole_tool_equals_the_checker(gpu_ctx, name):
    img, regions, to_rgb, want, want_info, _ = tb_lib.tool_case(name)
    got, info = _device_tool(gpu_ctx, img, regions, to_rgb, stride_pad=3)
    assert tb_lib.info_fields(info) == tb_lib.info_fields(want_info)
    _assert_same(got, want, name)
    # host planes and host masks give the same bits
    host = [np.array(a) for a in img]
    regs, keep = [], []
    for s, t, it, m in regions:
        hm = None if m is None else np.array(m)
        keep.append(hm)
        regs.append((s, t, it, None if hm is None else capi.host_plane(hm)))
    gpu_ctx.texture_boost(capi.host_rgb(host), regs, O.REC2020_WS_D, 1.0, True, to_rgb)
    _assert_same(host, want, name + " (host planes)")


@pytest.mark.parametrize("threshold", [0.2, 0.3])
def test_nan_pixel_lands_where_the_reference_puts_it(gpu_ctx, threshold):
    """one NaN in a column of the reference's 4-wide body, one in a tail column: the clamp (and the max) take the vector or the scalar form by
    column, so the neighbours equal the checker's bit for bit; the two pixels themselves are NaN on both sides (a NaN's payload is not compared)"""
    Y = tb_lib.nan_plane(67, 41, seed=30)
    want, want_info, _ = tb_lib.texture_boost_plane(Y, 1.0, threshold)
    got, info = _device_plane(gpu_ctx, Y, stride_pad=5, strength=1.0, threshold=threshold)
    assert tb_lib.info_fields(info) == tb_lib.info_fields(want_info)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == 2
    ok = ~np.isnan(want)
    assert np.array_equal(_bits(got[ok]), _bits(want[ok])), int((_bits(got[ok]) != _bits(want[ok])).sum())


def test_all_zero_strength_is_the_yuv_round_trip(gpu_ctx):
    img, regions, to_rgb, want, _, _ = tb_lib.tool_case("67x41-all-zero")
    got, info = _device_tool(gpu_ctx, img, regions, to_rgb)
    assert tb_lib.info_fields(info) == (0,) * 9
    _assert_same(got, want, "all strength 0")
    assert any(not np.array_equal(_bits(g), _bits(a)) for g, a in zip(got, img)), "the YUV round trip is not the identity in bits"
    # and an empty region list does the same
    got2, _ = _device_tool(gpu_ctx, img, [], to_rgb)
    _assert_same(got2, want, "no regions")


def test_same_call_twice_same_bits_and_scratch_returns(gpu_ctx):
    Y, kw = tb_lib.plane_case("300x200-t0.43")[:2]
    gpu_ctx.trim_scratch()
    before = gpu_ctx.scratch_bytes()
    a, ia = _device_plane(gpu_ctx, Y, **kw)
    # two planes of the 399 x 266 working size and the statistics grid twice
    assert gpu_ctx.scratch_bytes() - before >= 2 * 399 * 266 * 4 + 4 * 399 * 266 * 4
    b, ib = _device_plane(gpu_ctx, Y, stride_pad=9, **kw)
    assert bytes(ia) == bytes(ib)
    _assert_same([a], [b], "second call")
    gpu_ctx.trim_scratch()
    assert gpu_ctx.scratch_bytes() == before


def test_unsupported_cases_leave_the_image_alone(gpu_ctx):
    Y = tb_lib.textured_plane(67, 41, seed=4)
    thin = tb_lib.textured_plane(701, 3, seed=4)
    # (plane, strength, threshold, iterations, scale, high_detail): the preview's gaussianBlur, no iteration, an 11 x 11 gaussian, an empty grid
    for plane, args in ((Y, (1.0, 0.2, 1, 1.0, False)), (Y, (1.0, 0.2, 0, 1.0, True)), (Y, (1.0, 0.2, 1, 0.5, True)), (thin, (1.0, 2.0, 1, 1.0, True))):
        assert tb_lib.texture_boost_plane(plane, args[0], args[1], iterations=args[2], scale=args[3], high_detail=args[4]) is None
        d = torch.from_numpy(np.array(plane)).to("cuda:0")
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
            gpu_ctx.texture_boost_plane(capi.device_plane(d), *args)
        gpu_ctx.synchronize()
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(plane)), args
        host = np.array(plane)
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
            gpu_ctx.texture_boost_plane(capi.host_plane(host), *args)
        assert np.array_equal(_bits(host), _bits(plane)), args
    # one row below the promised smallest size, above 600 wide (subsampling 5)
    thin5 = tb_lib.textured_plane(605, capi.TEXTURE_BOOST_MIN_SIZE - 1, seed=18)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        gpu_ctx.texture_boost_plane(capi.host_plane(np.array(thin5)), 1.0, 1.43)
    # the whole tool: a later region that is unsupported stops the call before the first one (or the YUV switch) has run
    img = tb_lib.rgb_scene(67, 41, seed=5)
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in img]
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        gpu_ctx.texture_boost(capi.RGB(*[capi.device_plane(t) for t in d]), [(1.0, 0.3, 1, None), (1.0, 0.2, 0, None)], O.REC2020_WS_D)
    gpu_ctx.synchronize()
    assert all(np.array_equal(_bits(t.cpu().numpy()), _bits(a)) for t, a in zip(d, img))
    # a region with strength 0 is not looked at (the reference skips it before texture_boost)
    gpu_ctx.texture_boost(capi.RGB(*[capi.device_plane(t) for t in d]), [(0.0, 0.2, 0, None)], O.REC2020_WS_D)
    # bad arguments are EINVAL
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
        gpu_ctx.texture_boost_plane(capi.host_plane(np.array(Y)), 1.0, 0.0)
    wrong = np.ones((41, 66), np.float32)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
        gpu_ctx.texture_boost(capi.host_rgb([np.array(a) for a in img]), [(1.0, 0.3, 1, capi.host_plane(wrong))], O.REC2020_WS_D)


def _pipeline(ctx, raw, p):
    h, w = raw.shape
    b = p.border
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    ctx.synchronize()
    return d_img


def _stages(ctx, raw, regions):
    """demosaic, get_image, exposure, texture boost, tone curve through the individual entry points"""
    h, w = raw.shape
    d_raw = torch.from_numpy(raw).to("cuda:0")
    dem = [torch.empty((h, w), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    planes = capi.RGB(*[capi.device_plane(t) for t in dem])
    ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), synth.FILTERS_RGGB, 1.0, 4, planes)
    d_img = [torch.empty((h - 8, w - 8), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    ctx.get_image(planes, 4, 4, MUL, True, MAT, img)
    ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    ctx.texture_boost(img, regions, O.REC2020_WS_D, 1.0, True, True)
    ctx.tone_curve(img, _lut(), 1.0, True)
    ctx.synchronize()
    return d_img


def _pipe_regions(w, h):
    mask = tb_lib.smooth_mask(w - 8, h - 8)
    regions = [(1.0, 0.2, 1, None), (-0.8, 1.0, 1, capi.host_plane(mask)), (0.0, 0.43, 1, None)]
    arr, keep = capi.texture_boost_regions(regions)
    return regions, arr, (keep, mask)


def test_pipeline_flag_equals_the_stages(gpu_ctx):
    w, h = 392, 296
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=41, noise=1500)
    lut = _lut()
    p = _params(lut, 0)
    p.denoise_enabled = 0
    plain = _pipeline(gpu_ctx, raw, p)
    regions, arr, keep = _pipe_regions(w, h)
    # flag zero (regions still set): today's output
    p.texture_boost_nregions = len(regions); p.texture_boost_regions = arr
    off = _pipeline(gpu_ctx, raw, p)
    for a, b in zip(off, plain):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    p.texture_boost_enabled = 1
    got = _pipeline(gpu_ctx, raw, p)
    want = _stages(gpu_ctx, raw, regions)
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), int((a.view(torch.int32) != b.view(torch.int32)).sum())
    assert not torch.equal(got[1], plain[1])
    # what the tool does not support fails the frame
    arr[0].iterations = 0
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        _pipeline(gpu_ctx, raw, p)
    del keep


def test_batch_of_two_frames_on_two_lanes():
    w, h = 392, 296
    lut = _lut()
    p = _params(lut, 0)
    p.denoise_enabled = 0
    regions, arr, keep = _pipe_regions(w, h)
    p.texture_boost_enabled = 1; p.texture_boost_nregions = len(regions); p.texture_boost_regions = arr
    raws = [synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=s, noise=1500) for s in (45, 46)]
    outs = [[np.zeros((h - 8, w - 8), np.float32) for _ in range(3)] for _ in raws]
    ctx = capi.Context(0)
    ctx.set_batch_lanes(2)
    ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
    for r, o in zip(raws, outs):
        want = _stages(ctx, r, regions)
        for a, t in zip(o, want):
            assert np.array_equal(_bits(a), _bits(t.cpu().numpy())) and a.max() > 0
    assert not np.array_equal(outs[0][1], outs[1][1])
    ctx.close()
    del keep


def test_cli_texture_boost_through_stage_3(gpu_ctx, tmp_path):
    """artgpu-cli --texture-boost 1.0,0.2,1 (ImProcFunctions::process(STAGE_3) -> ImProcFunctions::textureBoost in the C++ mirror, ahead of the tone
    curve) equals the same stages called one by one; --texture-boost -0.8,1,2 takes the guided, rescaled path"""
    w, h, filt, b = 392, 296, synth.FILTERS_RGGB, 4
    raw = synth.bayer_frame(w, h, filt, seed=42, noise=1200)
    _, without = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3"])
    for flag, region in (("1.0,0.2,1", (1.0, 0.2, 1, None)), ("-0.8,1,2", (-0.8, 1.0, 2, None))):
        _, got = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--texture-boost", flag])
        assert not np.array_equal(got, without)
        d_raw = torch.from_numpy(raw).to("cuda:0")
        dem = [torch.empty((h, w), dtype=torch.float32, device="cuda:0") for _ in range(3)]
        planes = capi.RGB(*[capi.device_plane(t) for t in dem])
        gpu_ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), filt, 1.0, b, planes)
        d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
        img = capi.RGB(*[capi.device_plane(t) for t in d_img])
        gpu_ctx.get_image(planes, b, b, MUL, True, None, img)
        gpu_ctx.convert_color_space(img, MAT)
        gpu_ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
        gpu_ctx.texture_boost(img, [region], O.REC2020_WS_D, 1.0, True, True)
        gpu_ctx.tone_curve(img, tone_lut(), 1.0, True)
        gpu_ctx.synchronize()
        want = np.stack([np.rint(np.clip(t.cpu().numpy(), 0, 65535)).astype(np.uint16) for t in d_img], axis=-1)
        assert np.array_equal(got, want), flag


def test_cli_batch_queue_with_texture_boost(gpu_ctx, tmp_path):
    """artgpu-cli --batch ... --texture-boost: BatchQueue::process (rtengine_gpu.h) hands the regions to artgpu_batch_run_io -- uint16 sensor
    frames in, 16-bit scanlines out, two lanes -- against scaleColors by hand, the stages one by one and getScanline"""
    w, h, filt, black = 392, 296, synth.FILTERS_RGGB, 64.0
    frames = [np.clip(synth.bayer_frame(w, h, filt, seed=50 + k, noise=1500), 0, 65535).astype(np.uint16) for k in range(2)]
    names = []
    for k, f in enumerate(frames):
        n = tmp_path / f"f{k}.u16"
        f.astype("<u2").tofile(n)
        names.append(str(n))
    res = subprocess.run([CLI, "--batch", ",".join(names), "--width", str(w), "--height", str(h), "--lanes", "2", "--black", str(black),
                          "--expcomp", "0.3", "--texture-boost", "1.0,0.2,1", "--out", str(tmp_path / "o")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    assert json.loads(res.stdout.strip().splitlines()[-1])["frames"] == 2
    for k, f in enumerate(frames):
        raw = np.maximum(f.astype(np.float32) - np.float32(black), np.float32(0.0))          # scaleColors with scale_mul 1
        planes = [t.cpu().numpy() for t in _stages(gpu_ctx, raw, [(1.0, 0.2, 1, None)])]
        want = O.get_scanlines(planes, 16, False)
        got = read_ppm16(tmp_path / f"o.{k}.ppm")
        assert np.array_equal(got, want), (k, int((got != want).sum()))
        plain = [t.cpu().numpy() for t in _stages(gpu_ctx, raw, [])]
        assert not np.array_equal(got, O.get_scanlines(plain, 16, False))
