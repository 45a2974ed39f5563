"""GPU: capture sharpening (artgpu_sharpening = ImProcFunctions::doSharpening for the rld method, ipsharpen.cc:712-788) and its staged entry
points artgpu_gaussian_blur_ex, artgpu_rl_deconvolution and artgpu_deconv_auto_radius.

artgpu_gaussian_blur_ex is compared with what the COMPILED reference recorded (tests/golden/gauss_divmult.npz), everything else with the CPU
checker (tests/sh_lib.py: tests/emul/sharpen_ref.cc, itself pinned to that file).  Every operation of the stage is an IEEE float add, multiply,
divide, square root, maximum or comparison in a fixed order, plus host-side doubles, so every comparison is bit for bit (NaN payloads
aside).  The cases and the branches they take are listed in sh_lib.CASES and checked from the checker's counters in
tests/test_sharpen_checker.py.  The iteration kernel's tile is 64 x 32: the sizes 23 x 9, 67 x 41, 131 x 67, 300 x 200 and 257 x 514 lie on
both sides of it in both directions."""

import ctypes as C

import numpy as np
import pytest
import torch

from art_amd import capi, synth
import oracle_lib as O
import sh_lib
from test_gpu_cli import MAT, MUL, run_cli, tone_lut
from test_gpu_pipeline import _lut, _params

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _nbad(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return int((~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want)))).sum())


def _dev_plane(a, pad):
    """a device copy of a plane whose rows are `pad` floats longer than w, the padding NaN; (buffer, view)"""
    h, w = a.shape
    buf = torch.full((h, w + pad), float("nan"), dtype=torch.float32, device="cuda:0")
    buf[:, :w].copy_(torch.from_numpy(np.array(a, dtype=np.float32)))
    return buf, buf[:, :w]


def _untouched_padding(buf, w):
    return bool(torch.isnan(buf[:, w:]).all())


# ---- artgpu_gaussian_blur_ex against the compiled reference

@pytest.mark.parametrize("w,h", sh_lib.GOLDEN_SIZES)
def test_blur_forms_equal_the_compiled_reference(gpu_ctx, w, h):
    g = sh_lib.golden()
    src, div, dst0 = g[f"src_{w}x{h}"], g[f"div_{w}x{h}"], g[f"dst0_{w}x{h}"]
    for sigma in sh_lib.GOLDEN_SIGMAS:
        k = sh_lib.golden_key(sigma, w, h)
        # strided device planes
        sb, sv = _dev_plane(src, 3)
        vb, vv = _dev_plane(div, 5)
        db, dv = _dev_plane(np.full((h, w), np.nan, np.float32), 2)
        gpu_ctx.gaussian_blur_ex(capi.device_plane(sv), capi.device_plane(dv), capi.device_plane(vv), sigma, capi.GAUSS_DIV)
        gpu_ctx.synchronize()
        d_dev = dv.cpu().numpy()
        assert _untouched_padding(db, w) and _untouched_padding(sb, w)
        assert np.array_equal(_bits(sv.cpu().numpy()), _bits(src)), "GAUSS_DIV changed src"
        mb, mv = _dev_plane(dst0, 7)
        gpu_ctx.gaussian_blur_ex(capi.device_plane(sv), capi.device_plane(mv), None, sigma, capi.GAUSS_MULT)
        gpu_ctx.synchronize()
        m_dev = mv.cpu().numpy()
        assert _untouched_padding(mb, w) and _untouched_padding(sb, w)
        if sigma <= 1.15:
            assert np.array_equal(_bits(sv.cpu().numpy()), _bits(src)), "GAUSS_MULT changed src below 1.15"
        print(f"gaussian_blur_ex {k}: DIV differs in {_nbad(d_dev, g['d_' + k])}, MULT in {_nbad(m_dev, g['m_' + k])}")
        assert _nbad(d_dev, g["d_" + k]) == 0, ("DIV", k)
        assert _nbad(m_dev, g["m_" + k]) == 0, ("MULT", k)
        # host planes equal the strided device planes
        hs, hd, hm = src.copy(), np.full((h, w), np.nan, np.float32), dst0.copy()
        gpu_ctx.gaussian_blur_ex(capi.host_plane(hs), capi.host_plane(hd), capi.host_plane(np.ascontiguousarray(div)), sigma, capi.GAUSS_DIV)
        gpu_ctx.gaussian_blur_ex(capi.host_plane(hs), capi.host_plane(hm), None, sigma, capi.GAUSS_MULT)
        assert _nbad(hd, d_dev) == 0 and _nbad(hm, m_dev) == 0, k


def test_blur_ex_rejects_what_it_does_not_do(gpu_ctx):
    a, b = np.ones((9, 9), np.float32), np.ones((9, 9), np.float32)
    for sigma, gt in ((25.0, capi.GAUSS_MULT), (float("nan"), capi.GAUSS_MULT), (float("inf"), capi.GAUSS_MULT), (1.0, capi.GAUSS_STANDARD)):
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
            gpu_ctx.gaussian_blur_ex(capi.host_plane(a), capi.host_plane(b), None, sigma, gt)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
        gpu_ctx.gaussian_blur_ex(capi.host_plane(a), capi.host_plane(b), None, 1.0, capi.GAUSS_DIV)      # no divisor
    assert (a == 1).all() and (b == 1).all()


# ---- artgpu_rl_deconvolution against the checker

def _rl_device(ctx, Y, bl, imp, sigma, amount, pad=5):
    lb, lv = _dev_plane(Y, pad)
    bb, bv = _dev_plane(bl, 1)
    d_imp = torch.from_numpy(np.array(imp)).to("cuda:0")
    info = ctx.rl_deconvolution(capi.device_plane(lv), capi.device_plane(bv), d_imp.data_ptr(), sigma, amount, want_info=True)
    ctx.synchronize()
    assert _untouched_padding(lb, Y.shape[1])
    return lv.cpu().numpy(), info


@pytest.mark.parametrize("w,h", sh_lib.RL_SIZES)
def test_rl_deconvolution_equals_the_checker(gpu_ctx, w, h):
    Y, bl, imp = sh_lib.rl_inputs(w, h)
    for sigma in sh_lib.RL_SIGMAS:
        for amount in sh_lib.RL_AMOUNTS:
            want, want_info, _ = sh_lib.deconv(Y, bl, imp, sigma, amount)
            got, info = _rl_device(gpu_ctx, Y, bl, imp, sigma, amount)
            print(f"rl_deconvolution {w}x{h} sigma {sigma} amount {amount}: {_nbad(got, want)} differ, info {sh_lib.info_fields(info)} "
                  f"checker {sh_lib.info_fields(want_info)}")
            assert sh_lib.info_fields(info) == sh_lib.info_fields(want_info), (sigma, amount)
            assert _nbad(got, want) == 0, (sigma, amount)
    # host planes, host impulse map
    want, want_info, _ = sh_lib.deconv(Y, bl, imp, 0.75, 1.0)
    host = Y.copy()
    info = gpu_ctx.rl_deconvolution(capi.host_plane(host), capi.host_plane(np.ascontiguousarray(bl)), np.ascontiguousarray(imp).ctypes.data, 0.75, 1.0,
                                    want_info=True)
    assert _nbad(host, want) == 0 and sh_lib.info_fields(info) == sh_lib.info_fields(want_info)


def test_rl_two_kernel_form_equals_the_fused_kernel(gpu_ctx):
    Y, bl, imp = sh_lib.rl_inputs(131, 67)
    for sigma in (0.45, 0.75, 1.0):
        fused, fi = _rl_device(gpu_ctx, Y, bl, imp, sigma, 1.0)
        gpu_ctx.set_option("sharpen_fused", 0)
        try:
            plain, pi = _rl_device(gpu_ctx, Y, bl, imp, sigma, 1.0)
        finally:
            gpu_ctx.set_option("sharpen_fused", 1)
        assert _nbad(fused, plain) == 0 and bytes(fi) == bytes(pi), sigma


def test_rl_early_returns_leave_the_bits_alone(gpu_ctx):
    Y, bl, imp = sh_lib.rl_inputs(67, 41)
    for sigma, amount, early in ((0.75, 0.0, 4), (0.1, 1.0, 5)):
        got, info = _rl_device(gpu_ctx, Y, bl, imp, sigma, amount)
        assert np.array_equal(_bits(got), _bits(Y)) and info.early_out == early and info.regime == -1
    for sigma in (25.0, float("nan")):
        lb, lv = _dev_plane(Y, 0)
        d_imp = torch.from_numpy(np.array(imp)).to("cuda:0")
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
            gpu_ctx.rl_deconvolution(capi.device_plane(lv), capi.host_plane(np.ascontiguousarray(bl)), d_imp.data_ptr(), sigma, 1.0)
        gpu_ctx.synchronize()
        assert np.array_equal(_bits(lv.cpu().numpy()), _bits(Y))


# ---- artgpu_sharpening against the checker

def _device(ctx, img, scale=1.0, stride_pad=0, want_info=True, **kw):
    """artgpu_sharpening on device-resident copies of the planes (one allocation, rows stride_pad floats longer than w); (planes, info)"""
    h, w = img[0].shape
    buf = torch.full((3, h, w + stride_pad), float("nan"), dtype=torch.float32, device="cuda:0")
    views = [buf[c, :, :w] for c in range(3)]
    for v, a in zip(views, img):
        v.copy_(torch.from_numpy(np.array(a, dtype=np.float32)))
    p = capi.sharpening_params(**kw)
    info = ctx.sharpening(capi.RGB(*[capi.device_plane(v) for v in views]), p, O.REC2020_WS_D, scale, want_info=want_info)
    ctx.synchronize()
    if stride_pad:
        assert bool(torch.isnan(buf[:, :, w:]).all()), "wrote past the row"
    return [v.cpu().numpy() for v in views], info


def _assert_same_planes(got, want, what):
    bad = [_nbad(g, w) for g, w in zip(got, want)]
    print(f"sharpening {what}: values that differ from the checker, per plane: {bad}")
    assert bad == [0, 0, 0], (what, bad)


@pytest.mark.parametrize("name", list(sh_lib.CASES))
def test_image_and_info_equal_the_checker(gpu_ctx, name):
    img, scale, kw, want, want_info, _ = sh_lib.case(name)
    got, info = _device(gpu_ctx, img, scale=scale, stride_pad=7, **kw)
    print(f"sharpening {name}: info {sh_lib.info_fields(info)} checker {sh_lib.info_fields(want_info)}")
    assert sh_lib.info_fields(info) == sh_lib.info_fields(want_info)
    _assert_same_planes(got, want, name)
    assert any(not np.array_equal(g, a) for g, a in zip(got, img)), "the call changed nothing"


def test_early_outs_and_deconvolution_early_returns(gpu_ctx):
    img = sh_lib.edge_scene(23, 9, seed=3)
    for kw, early in ((dict(enabled=False), 1), (dict(amount=0), 2)):
        got, info = _device(gpu_ctx, img, stride_pad=3, **kw)
        assert info.early_out == early and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, img))
    small = [np.ascontiguousarray(a[:7, :]) for a in img]
    got, info = _device(gpu_ctx, small)
    assert info.early_out == 3 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, small))
    # deconvsharpening's own early returns: the planes still go through multiply (Y / Y)
    for kw, early in ((dict(deconvamount=0), 4), (dict(deconvradius=0.1), 5)):
        want, want_info, _ = sh_lib.sharpening(img, **kw)
        got, info = _device(gpu_ctx, img, stride_pad=1, **kw)
        assert info.early_out == early == want_info.early_out
        _assert_same_planes(got, want, f"early return {early}")


def test_unsupported_leaves_the_image_alone(gpu_ctx):
    img = sh_lib.edge_scene(67, 41, seed=4)
    for scale, kw in ((1.0, dict(method=capi.SHARPEN_USM)), (1.0, dict(method=capi.SHARPEN_PSF)), (1.0, dict(deconvradius=25.0)),
                      (1.0, dict(deconvradius=float("nan"))), (1.0, dict(deconvradius=24.9, corner_boost=0.2)), (12.0, dict())):
        assert sh_lib.sharpening(img, scale=scale, **kw) is None
        d = [torch.from_numpy(a).to("cuda:0") for a in img]
        p = capi.sharpening_params(**kw)
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
            gpu_ctx.sharpening(capi.RGB(*[capi.device_plane(t) for t in d]), p, O.REC2020_WS_D, scale)
        gpu_ctx.synchronize()
        assert all(np.array_equal(_bits(t.cpu().numpy()), _bits(a)) for t, a in zip(d, img))
        host = [a.copy() for a in img]
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
            gpu_ctx.sharpening(capi.host_rgb(host), p, O.REC2020_WS_D, scale)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(host, img))


def test_host_planes_and_second_call_same_bits(gpu_ctx):
    img, scale, kw, want, want_info, _ = sh_lib.case("131x67-scale2-radius1.5")
    h, w = img[0].shape
    bufs = [np.full((h, w + 3), np.nan, np.float32) for _ in range(3)]
    host = [b[:, :w] for b in bufs]
    for v, a in zip(host, img):
        v[:] = a
    info = gpu_ctx.sharpening(capi.RGB(*[capi.host_plane(v) for v in host]), capi.sharpening_params(**kw), O.REC2020_WS_D, scale, want_info=True)
    assert all(np.isnan(b[:, w:]).all() for b in bufs)
    a, ia = _device(gpu_ctx, img, scale=scale, stride_pad=11, **kw)
    b, ib = _device(gpu_ctx, img, scale=scale, **kw)
    assert bytes(info) == bytes(ia) == bytes(ib)
    _assert_same_planes(host, a, "host planes against device planes")
    _assert_same_planes(a, b, "second call")
    _assert_same_planes(host, want, "host planes")
    # without info the call does not wait and gives the same planes
    c, none = _device(gpu_ctx, img, scale=scale, want_info=False, **kw)
    assert none is None
    _assert_same_planes(c, want, "no info")


def test_trim_scratch_returns_the_stage_storage(gpu_ctx):
    img, scale, kw = sh_lib.case("300x200-arp-default")[:3]
    gpu_ctx.trim_scratch()
    before = gpu_ctx.scratch_bytes()
    _device(gpu_ctx, img, scale=scale, **kw)
    assert gpu_ctx.scratch_bytes() - before >= 8 * 300 * 200 * 4 + 300 * 200      # eight planes and the byte plane
    gpu_ctx.trim_scratch()
    assert gpu_ctx.scratch_bytes() == before


# ---- artgpu_deconv_auto_radius

@pytest.mark.parametrize("w,h,filters,seed", sh_lib.RADIUS_CASES)
def test_auto_radius_equals_the_checker(gpu_ctx, w, h, filters, seed):
    raw = sh_lib.mosaic(w, h, seed, filters)
    want_r, want_m, _ = sh_lib.radius(raw, filters, upper=sh_lib.RADIUS_CLIP)
    rb, rv = _dev_plane(raw, 5)
    r, m = gpu_ctx.deconv_auto_radius(capi.device_plane(rv), filters, 1000.0, sh_lib.RADIUS_CLIP)
    print(f"auto radius {w}x{h} {filters:#x}: {r} ({m}), checker {want_r} ({want_m})")
    assert m.view(np.uint32) == want_m.view(np.uint32) and r.view(np.uint32) == want_r.view(np.uint32)
    r2, m2 = gpu_ctx.deconv_auto_radius(capi.host_plane(raw), filters, 1000.0, sh_lib.RADIUS_CLIP)
    assert (r2.view(np.uint32), m2.view(np.uint32)) == (r.view(np.uint32), m.view(np.uint32))


def test_auto_radius_flat_plane_and_xtrans(gpu_ctx):
    flat = np.full((48, 64), 5000.0, np.float32)
    r, m = gpu_ctx.deconv_auto_radius(capi.host_plane(flat), sh_lib.FILTERS_RGGB)
    assert m == 1.0 and np.isnan(r)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        gpu_ctx.deconv_auto_radius(capi.host_plane(flat), 9)


# ---- the pipeline flag, the batch lanes, the command line

SH_CLIP = 65535.0


def _pipeline(ctx, raw, p):
    h, w = raw.shape
    b = p.border
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    ctx.synchronize()
    return d_img


def _stages(ctx, raw, p, sp, denoise, auto):
    """demosaic, get_image, [denoise,] exposure, sharpening, tone curve through the individual entry points"""
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
    ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    q = capi.SharpeningParams.from_buffer_copy(sp)
    if auto:
        r, _ = ctx.deconv_auto_radius(capi.device_plane(d_raw), synth.FILTERS_RGGB, 1000.0, SH_CLIP)
        q.deconvradius = float(r)
    ctx.sharpening(img, q, O.REC2020_WS_D, 1.0)
    ctx.tone_curve(img, _lut(), 1.0, True)
    ctx.synchronize()
    return d_img


@pytest.mark.parametrize("denoise", [True, False])
def test_pipeline_flag_equals_the_stages(gpu_ctx, denoise):
    w, h = 520, 392
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=31, noise=1500)
    lut = _lut()
    sp = capi.sharpening_params(deconvradius=0.9)
    p = _params(lut, 0)
    p.denoise_enabled = 1 if denoise else 0
    plain = _pipeline(gpu_ctx, raw, p)
    # flag zero (parameters still set): today's output
    p.sharpening = sp; p.sharpening_auto_radius = 1; p.sharpening_clip_val = SH_CLIP
    off = _pipeline(gpu_ctx, raw, p)
    for a, b in zip(off, plain):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    p.sharpening_enabled = 1
    results = []
    for auto in (0, 1):
        p.sharpening_auto_radius = auto
        got = _pipeline(gpu_ctx, raw, p)
        want = _stages(gpu_ctx, raw, p, sp, denoise, bool(auto))
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (auto, int((a.view(torch.int32) != b.view(torch.int32)).sum()))
        assert not torch.equal(got[1], plain[1])
        results.append(got)
    assert not torch.equal(results[0][1], results[1][1]), "the automatic radius changed nothing"
    # what the stage does not support fails the frame before any stage has run
    p.sharpening.method = capi.SHARPEN_USM
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        _pipeline(gpu_ctx, raw, p)
    p.sharpening.method = capi.SHARPEN_RLD
    p.scale = 12.0
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        _pipeline(gpu_ctx, raw, p)


def test_pipeline_rejects_xtrans_with_the_automatic_radius(gpu_ctx):
    w, h = 390, 294
    raw = synth.xtrans_frame(w, h, seed=5)
    p = _params(_lut(), 0, xtrans=True)
    p.denoise_enabled = 0
    p.sharpening_enabled = 1; p.sharpening = capi.sharpening_params(); p.sharpening_auto_radius = 1; p.sharpening_clip_val = SH_CLIP
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.full((h - 14, w - 14), 7.0, dtype=torch.float32, device="cuda:0") for _ in range(3)]
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        gpu_ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    gpu_ctx.synchronize()
    assert all(bool((t == 7.0).all()) for t in d_img)


def test_batch_of_two_frames_on_two_lanes():
    w, h = 392, 296
    lut = _lut()
    sp = capi.sharpening_params()
    p = _params(lut, 0)
    p.sharpening_enabled = 1; p.sharpening = sp; p.sharpening_auto_radius = 1; p.sharpening_clip_val = SH_CLIP
    raws = [synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=s, noise=1500) for s in (35, 36)]
    outs = [[np.zeros((h - 8, w - 8), np.float32) for _ in range(3)] for _ in raws]
    ctx = capi.Context(0)
    ctx.set_batch_lanes(2)
    ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
    for r, o in zip(raws, outs):
        want = _stages(ctx, r, p, sp, True, True)
        for a, t in zip(o, want):
            assert np.array_equal(_bits(a), _bits(t.cpu().numpy())) and a.max() > 0
    ctx.close()


def test_cli_sharpen_through_stage_2(gpu_ctx, tmp_path):
    """artgpu-cli --sharpen 20,auto (RawImageSource::getDeconvAutoRadius, then ImProcFunctions::process(STAGE_2) -> ImProcFunctions::sharpening in
    the C++ mirror, between STAGE_1 and STAGE_3) equals the same stages with the CHECKER's radius and sharpening in the middle"""
    w, h, filt, b = 520, 392, synth.FILTERS_RGGB, 4
    raw = synth.bayer_frame(w, h, filt, seed=32, noise=1200)
    _, got = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--sharpen", "20,auto"])
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
    gpu_ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    gpu_ctx.synchronize()
    radius, ratio, _ = sh_lib.radius(raw, filt, upper=SH_CLIP)
    assert ratio > 1 and 0.2 <= radius < 25
    sharp, info, _ = sh_lib.sharpening([t.cpu().numpy() for t in d_img], deconvradius=float(radius))
    assert info.early_out == 0
    for t, a in zip(d_img, sharp):
        t.copy_(torch.from_numpy(a))
    gpu_ctx.tone_curve(img, tone_lut(), 1.0, True)
    gpu_ctx.synchronize()
    want = np.stack([np.rint(np.clip(t.cpu().numpy(), 0, 65535)).astype(np.uint16) for t in d_img], axis=-1)
    assert np.array_equal(got, want)
    # a fixed radius with amount and corner boost goes another way
    _, got2 = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--sharpen", "20,0.6,80,0.4,30"])
    assert not np.array_equal(got2, got) and not np.array_equal(got2, without)
