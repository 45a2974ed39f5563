"""GPU: artgpu_dehaze (ImProcFunctions::dehaze, ipdehaze.cc:306-512) and artgpu_dehaze_dark_channel against the CPU checker
(tests/dh_lib.py: tests/emul/dehaze_ref.cc around the oracle's guided filter, box blur, FlatCurve and LUTf).

The tool's reductions are maxima and minima and its few log / exp / double sums run on the host over the thumbnail, so every case is
compared bit for bit: the three planes and every field of artgpu_dehaze_info.  The cases and the branches they take are listed in
dh_lib.CASES and checked from the checker's counters in tests/test_dehaze_checker.py."""

import numpy as np
import pytest
import torch

from art_amd import capi, synth
import dh_lib
import oracle_lib as O
from test_gpu_cli import MAT, MUL, run_cli, tone_lut
from test_gpu_pipeline import _lut, _params

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _device(ctx, img, stride_pad=0, want_info=True, **kw):
    """artgpu_dehaze on device-resident copies of the planes (one allocation, rows stride_pad floats longer than w); returns (planes, info)"""
    h, w = img[0].shape
    scale = kw.pop("scale", 1.0)
    buf = torch.full((3, h, w + stride_pad), float("nan"), dtype=torch.float32, device="cuda:0")
    views = [buf[c, :, :w] for c in range(3)]
    for v, a in zip(views, img):
        v.copy_(torch.from_numpy(np.array(a, dtype=np.float32)))
    p, keep = capi.dehaze_params(**kw)
    info = ctx.dehaze(capi.RGB(*[capi.device_plane(v) for v in views]), p, O.REC2020_WS_D, scale, want_info=want_info)
    ctx.synchronize()
    del keep
    if stride_pad:
        assert bool(torch.isnan(buf[:, :, w:]).all()), "wrote past the row"
    return [v.cpu().numpy() for v in views], info


def _assert_same_planes(got, want, what):
    bad = [int((_bits(g) != _bits(w)).sum()) for g, w in zip(got, want)]
    print(f"dehaze {what}: values that differ from the checker, per plane: {bad}")
    assert bad == [0, 0, 0], (what, bad)


@pytest.mark.parametrize("name", list(dh_lib.CASES))
def test_image_and_info_equal_the_checker(gpu_ctx, name):
    img, kw, want, want_info, _ = dh_lib.case(name)
    got, info = _device(gpu_ctx, img, stride_pad=7, **kw)
    print(f"dehaze {name}: info {dh_lib.info_fields(info)} checker {dh_lib.info_fields(want_info)}")
    assert dh_lib.info_fields(info) == dh_lib.info_fields(want_info)
    assert info.haze_detected == 1
    _assert_same_planes(got, want, name)
    assert all(not np.array_equal(g, a) for g, a in zip(got, img)), "the call changed nothing"


@pytest.mark.parametrize("w,h", [(131, 67), (64, 260)])
def test_dark_channel(gpu_ctx, w, h):
    rng = np.random.default_rng(w)
    # the hazy scene moved down so that part of it is negative; no exact zero (the sign of a zero minimum is not defined without the clip)
    planes = [(a / np.float32(65535.0) - np.float32(0.1) + rng.uniform(-0.02, 0.02, a.shape).astype(np.float32))
              for a in dh_lib.hazy_scene(w, h, seed=w, bright_block=True)]
    assert all((a != 0).all() for a in planes) and min(a.min() for a in planes) < 0 and max(a.max() for a in planes) > 0.6
    d_planes = [torch.from_numpy(a).to("cuda:0") for a in planes]
    rgb = capi.RGB(*[capi.device_plane(t) for t in d_planes])
    ambients = (None, (0.45, 0.5, 0.55), (0.45, -0.25, 0.55), (0.45, 0.5, 0.0))          # none, positive, one negative, one zero component
    for patch in (2, 3, 5, 13, 20):
        for ambient in ambients:
            for clip in (False, True):
                want, _ = dh_lib.dark_channel(*planes, patch, ambient, clip)
                d_dst = torch.full((h, w + 5), float("nan"), dtype=torch.float32, device="cuda:0")
                gpu_ctx.dehaze_dark_channel(rgb, patch, ambient, clip, capi.device_plane(d_dst[:, :w]))
                gpu_ctx.synchronize()
                got = d_dst[:, :w].cpu().numpy()
                assert bool(torch.isnan(d_dst[:, w:]).all())
                assert np.array_equal(_bits(got), _bits(want)), (patch, ambient, clip, int((_bits(got) != _bits(want)).sum()))
    # host planes, host destination
    host_dst = np.full((h, w), np.nan, np.float32)
    gpu_ctx.dehaze_dark_channel(capi.host_rgb(planes), 13, ambients[1], True, capi.host_plane(host_dst))
    assert np.array_equal(_bits(host_dst), _bits(dh_lib.dark_channel(*planes, 13, ambients[1], True)[0]))
    with pytest.raises(capi.ArtGpuError):
        gpu_ctx.dehaze_dark_channel(rgb, 0, None, False, capi.host_plane(host_dst))


def test_no_haze_returns_the_normalised_image_restored(gpu_ctx):
    img = dh_lib.hazy_scene(300, 200, seed=11)
    img[1] = -np.abs(img[1]) - np.float32(1.0)            # one channel negative everywhere: no dark-channel value in [0, 1)
    want, want_info, counts = dh_lib.dehaze(img, blackpoint=0)
    assert counts["no_haze"] == 1 and want_info.haze_detected == 0
    got, info = _device(gpu_ctx, img, stride_pad=3)
    assert info.haze_detected == 0 and info.max_t < 0 and info.t0 == 0.0
    assert dh_lib.info_fields(info) == dh_lib.info_fields(want_info)
    _assert_same_planes(got, want, "no haze")
    # x * (1 / maxval) * maxval is not x in bits
    assert any(not np.array_equal(_bits(g), _bits(a)) for g, a in zip(got, img))


def test_unsupported_aspect_with_black_point_leaves_the_image_alone(gpu_ctx):
    img = dh_lib.hazy_scene(1803, 97, seed=12)
    assert dh_lib.dehaze(img, blackpoint=50) is None
    d = [torch.from_numpy(a).to("cuda:0") for a in img]
    p, keep = capi.dehaze_params(blackpoint=50)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        gpu_ctx.dehaze(capi.RGB(*[capi.device_plane(t) for t in d]), p, O.REC2020_WS_D)
    gpu_ctx.synchronize()
    assert all(np.array_equal(_bits(t.cpu().numpy()), _bits(a)) for t, a in zip(d, img))
    host = [a.copy() for a in img]
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        gpu_ctx.dehaze(capi.host_rgb(host), p, O.REC2020_WS_D)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(host, img))
    # disabled: nothing happens
    q, keep2 = capi.dehaze_params(enabled=False)
    gpu_ctx.dehaze(capi.host_rgb(host), q, O.REC2020_WS_D)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(host, img))


def test_host_planes_equal_strided_device_planes(gpu_ctx):
    img, kw, want, want_info, _ = dh_lib.case("723x481-crossing-black50-depth100")
    h, w = img[0].shape
    bufs = [np.full((h, w + 3), np.nan, np.float32) for _ in range(3)]
    host = [b[:, :w] for b in bufs]
    for v, a in zip(host, img):
        v[:] = a
    kw = dict(kw)
    scale = kw.pop("scale")
    p, keep = capi.dehaze_params(**kw)
    info = gpu_ctx.dehaze(capi.RGB(*[capi.host_plane(v) for v in host]), p, O.REC2020_WS_D, scale, want_info=True)
    assert all(np.isnan(b[:, w:]).all() for b in bufs)
    dev, dev_info = _device(gpu_ctx, img, stride_pad=11, **dh_lib.case("723x481-crossing-black50-depth100")[1])
    assert bytes(info) == bytes(dev_info)
    _assert_same_planes(host, dev, "host planes against device planes")
    _assert_same_planes(host, want, "host planes")


def test_same_call_twice_same_bits(gpu_ctx):
    img, kw = dh_lib.case("481x723-luminance")[:2]
    a, ia = _device(gpu_ctx, img, **kw)
    b, ib = _device(gpu_ctx, img, stride_pad=9, **kw)
    assert bytes(ia) == bytes(ib)
    _assert_same_planes(a, b, "second call")


def test_trim_scratch_returns_the_dehaze_storage(gpu_ctx):
    img, kw = dh_lib.case("723x481-crossing-black50-depth100")[:2]
    gpu_ctx.trim_scratch()
    before = gpu_ctx.scratch_bytes()
    _device(gpu_ctx, img, **kw)
    # at least the transmission plane, the statistics grids (six planes of 144 x 96 twice) and the strength table
    assert gpu_ctx.scratch_bytes() - before >= 723 * 481 * 4 + 12 * (723 // 5) * (481 // 5) * 4 + 65536 * 4
    gpu_ctx.trim_scratch()
    assert gpu_ctx.scratch_bytes() == before


def _pipeline(ctx, raw, p):
    h, w = raw.shape
    b = p.border
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    ctx.synchronize()
    return d_img


def _stages(ctx, raw, p, dh, denoise):
    """demosaic, get_image, [denoise,] dehaze, exposure, tone curve through the individual entry points"""
    h, w = raw.shape
    d_raw = torch.from_numpy(raw).to("cuda:0")
    dem = [torch.empty((h, w), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    planes = capi.RGB(*[capi.device_plane(t) for t in dem])
    ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), synth.FILTERS_RGGB, 1.0, 4, planes)
    d_img = [torch.empty((h - 8, w - 8), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    ctx.get_image(planes, 4, 4, MUL, True, MAT, img)
    if denoise:
        curve, _ = capi.noise_curve_lut()
        ctx.improc_denoise(img, p.denoise, O.REC2020_WS_D, ecomp=0.3, calclum_mat=MAT, noise_c_curve=curve, iws=O.REC2020_IWS_D)
    ctx.dehaze(img, dh, O.REC2020_WS_D, 1.0)
    ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    ctx.tone_curve(img, _lut(), 1.0, True)
    ctx.synchronize()
    return d_img


@pytest.mark.parametrize("denoise", [True, False])
def test_pipeline_flag_equals_the_stages(gpu_ctx, denoise):
    w, h = 520, 392
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=31, noise=1500)
    lut = _lut()
    dh, keep = capi.dehaze_params(strength=dh_lib.CROSSING_STRENGTH, depth=60, blackpoint=30)
    p = _params(lut, 0)
    p.denoise_enabled = 1 if denoise else 0
    plain = _pipeline(gpu_ctx, raw, p)
    # flag zero (parameters still set): today's output
    p.dehaze = dh
    off = _pipeline(gpu_ctx, raw, p)
    for a, b in zip(off, plain):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    p.dehaze_enabled = 1
    got = _pipeline(gpu_ctx, raw, p)
    want = _stages(gpu_ctx, raw, p, dh, denoise)
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), int((a.view(torch.int32) != b.view(torch.int32)).sum())
    assert not torch.equal(got[1], plain[1])
    # what the stage does not support fails the frame
    p.dehaze.nstrength = -1
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
        _pipeline(gpu_ctx, raw, p)
    del keep


def test_batch_of_two_frames_on_two_lanes():
    w, h = 392, 296
    lut = _lut()
    dh, keep = capi.dehaze_params(depth=50)
    p = _params(lut, 0)
    p.dehaze_enabled = 1; p.dehaze = dh
    raws = [synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=s, noise=1500) for s in (35, 36)]
    outs = [[np.zeros((h - 8, w - 8), np.float32) for _ in range(3)] for _ in raws]
    ctx = capi.Context(0)
    ctx.set_batch_lanes(2)
    ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
    for r, o in zip(raws, outs):
        want = _stages(ctx, r, p, dh, True)
        for a, t in zip(o, want):
            assert np.array_equal(_bits(a), _bits(t.cpu().numpy())) and a.max() > 0
    ctx.close()
    del keep


def test_cli_dehaze_through_stage_0(gpu_ctx, tmp_path):
    """artgpu-cli --dehaze 40,0.9,20 (ImProcFunctions::process(STAGE_0) -> ImProcFunctions::dehaze in the C++ mirror, between the denoise
    stage and STAGE_1) equals the same stages called one by one"""
    w, h, filt, b = 520, 392, synth.FILTERS_RGGB, 4
    raw = synth.bayer_frame(w, h, filt, seed=32, noise=1200)
    _, got = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--dehaze", "40,0.9,20"])
    _, without = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3"])
    assert not np.array_equal(got, without)
    d_raw = torch.from_numpy(raw).to("cuda:0")
    dem = [torch.empty((h, w), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    planes = capi.RGB(*[capi.device_plane(t) for t in dem])
    gpu_ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), filt, 1.0, b, planes)
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    gpu_ctx.get_image(planes, b, b, MUL, True, None, img)
    gpu_ctx.convert_color_space(img, MAT)
    dh, keep = capi.dehaze_params(strength=(1.0, 0.0, 0.9, 0.0, 0.0, 1.0, 0.9, 0.0, 0.0), depth=40, blackpoint=20)
    gpu_ctx.dehaze(img, dh, O.REC2020_WS_D, 1.0)
    gpu_ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    gpu_ctx.tone_curve(img, tone_lut(), 1.0, True)
    gpu_ctx.synchronize()
    want = np.stack([np.rint(np.clip(t.cpu().numpy(), 0, 65535)).astype(np.uint16) for t in d_img], axis=-1)
    assert np.array_equal(got, want)
    # the defaults behind the depth: strength 0.75, no black point, RGB mode
    _, got2 = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--dehaze", "40"])
    assert not np.array_equal(got2, got) and not np.array_equal(got2, without)
