"""GPU: artgpu_color_correction / artgpu_set_pipeline_color_correction (ImProcFunctions::colorCorrection, ipcolorcorrection.cc:39-866) against
the CPU checker (tests/cc_lib.py: tests/emul/colorcorrection_ref.cc around the oracle's sleef forms, PQ tables and YUV switch).

Every pixel outside the checker's `oor` map (a Jzazbz PQ / PQ_inv argument above 1: the device's powf there) and every field of
artgpu_color_correction_info is compared as a float32 bit pattern; pixels inside the map with rtol 2e-4 / atol 0.5, the bound
test_gpu_tonecurve.py uses for the same powf.  A NaN compares equal to a NaN (cc_lib.bits).  The cases and the branches they take are listed
in cc_lib.CASES and checked from the checker's counters in test_colorcorrection_checker.py."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest
import torch

from art_amd import capi, synth
import cc_lib
import mk_lib
import oracle_lib as O
import tb_lib
from test_gpu_cli import CLI, MAT, MUL, read_ppm16, run_cli, tone_lut
from test_gpu_pipeline import _lut, _params

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _capi_regions(regions, device_masks, w, h, keep):
    """cc_lib region dicts (mask arrays) -> capi region dicts (Planes); one array used twice becomes one Plane used twice"""
    planes = {}

    def plane(m):
        if m is None:
            return None
        if id(m) not in planes:
            if device_masks:
                mb = torch.full((h, w + 5), float("nan"), dtype=torch.float32, device="cuda:0")
                mb[:, :w].copy_(torch.from_numpy(np.array(m)))
                keep.append(mb)
                planes[id(m)] = capi.device_plane(mb[:, :w])
            else:
                hm = np.array(m, dtype=np.float32)
                keep.append(hm)
                planes[id(m)] = capi.host_plane(hm)
        return planes[id(m)]

    return [dict(r, lmask=plane(r.get("lmask")), abmask=plane(r.get("abmask"))) for r in regions]


def _device_tool(ctx, img, regions, to_rgb, stride_pad=0, device_masks=False, want_info=True):
    h, w = img[0].shape
    buf = torch.full((3, h, w + stride_pad), float("nan"), dtype=torch.float32, device="cuda:0")
    views = [buf[c, :, :w] for c in range(3)]
    for v, a in zip(views, img):
        v.copy_(torch.from_numpy(np.array(a, dtype=np.float32)))
    keep = []
    info = ctx.color_correction(capi.RGB(*[capi.device_plane(v) for v in views]), _capi_regions(regions, device_masks, w, h, keep), O.REC2020_WS_D,
                                O.REC2020_IWS_D, to_rgb, want_info=want_info)
    ctx.synchronize()
    del keep
    if stride_pad:
        assert bool(torch.isnan(buf[:, :, w:]).all()), "wrote past the row"
    return [v.cpu().numpy() for v in views], info


def _host_tool(ctx, img, regions, to_rgb, want_info=False):
    host = [np.array(a, dtype=np.float32) for a in img]
    h, w = host[0].shape
    keep = []
    info = ctx.color_correction(capi.host_rgb(host), _capi_regions(regions, False, w, h, keep), O.REC2020_WS_D, O.REC2020_IWS_D, to_rgb, want_info=want_info)
    return host, info


@pytest.mark.parametrize("name", list(cc_lib.CASES))
def test_planes_and_info_equal_the_checker(gpu_ctx, name):
    img, regions, to_rgb, want, want_info, oor, _ = cc_lib.case(name)
    got, info = _device_tool(gpu_ctx, img, regions, to_rgb, stride_pad=7 if name in cc_lib.STRIDED_CASES else 0,
                             device_masks=name in cc_lib.DEVICE_MASK_CASES)
    print(f"colour correction {name}: {int(oor.sum())} powf pixels; info {[cc_lib.info_fields(i) for i in info]}")
    assert [cc_lib.info_fields(i) for i in info] == [cc_lib.info_fields(i) for i in want_info]
    assert all(int(i.oor_pixels) == int(oor.sum()) for i in info)
    cc_lib.assert_same(got, want, oor, name)
    # host planes and host masks, without info: the same bits
    host, _ = _host_tool(gpu_ctx, img, regions, to_rgb)
    cc_lib.assert_same(host, want, oor, name + " (host planes)")


def test_no_regions_is_the_yuv_switch(gpu_ctx):
    img = cc_lib.scene(67, 45, seed=5)
    for to_rgb in (False, True):
        got, info = _device_tool(gpu_ctx, img, [], to_rgb)
        assert info == []
        want = cc_lib.color_correction(img, [], to_rgb=to_rgb)[0]
        cc_lib.assert_same(got, want, np.zeros((45, 67), bool), "no regions")
    assert any(not np.array_equal(cc_lib.bits(g), cc_lib.bits(a)) for g, a in zip(got, img)), "the YUV round trip is not the identity in bits"


def test_same_call_twice_same_bits(gpu_ctx):
    img, regions, to_rgb, *_ = cc_lib.case("67x45-superwhite")
    a, ia = _device_tool(gpu_ctx, img, regions, to_rgb)
    b, ib = _device_tool(gpu_ctx, img, regions, to_rgb, stride_pad=9, device_masks=True)
    assert [bytes(x) for x in ia] == [bytes(x) for x in ib]
    assert all(np.array_equal(cc_lib.bits(p), cc_lib.bits(q)) for p, q in zip(a, b))


def test_one_host_mask_read_through_several_entries(gpu_ctx):
    """one host plane is both masks of the first region and the lmask of the second: staged once, read through three entries; the same bits
    as with three separate device planes"""
    w, h = 4, 3
    img = cc_lib.scene(w, h, seed=13)
    m = cc_lib.mask("onelane", w, h)
    first, second = dict(mode=cc_lib.RGB, **cc_lib.VARIANTS["pivot"]), dict(mode=cc_lib.YUV, **cc_lib.VARIANTS["sop"])
    a, ia = _device_tool(gpu_ctx, img, [dict(first, lmask=m, abmask=m), dict(second, lmask=m, abmask=None)], True)
    b, ib = _device_tool(gpu_ctx, img, [dict(first, lmask=m.copy(), abmask=m.copy()), dict(second, lmask=m.copy(), abmask=None)], True, device_masks=True)
    assert [bytes(x) for x in ia] == [bytes(x) for x in ib]
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, b))
    assert any(not np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, img)), "the regions changed nothing"


UNSUPPORTED = {
    "lut-mode": [dict(mode=cc_lib.JZAZBZ), dict(mode=cc_lib.LUT)],
    "power-zero": [dict(mode=cc_lib.RGB, power=(1.0, 0.0, 1.0))],
    "power-zero-yuv": [dict(mode=cc_lib.YUV, power=(0.0, 1.0, 1.0))],
    "pivot-zero": [dict(mode=cc_lib.RGB, slope=1.1, pivot=(1.0, 1.0, 0.0), compression=0.3)],
    "slope-overflow": [dict(mode=cc_lib.YUV, slope=1e300)],
    "hsl-gamma-zero": [dict(mode=cc_lib.HSL, hsl_gamma=0.0)],
    "hsl-gamma-negative": [dict(mode=cc_lib.YUV), dict(mode=cc_lib.HSL, hsl_gamma=-2.0, hue=(10.0, 20.0, 30.0), sat=(10.0, 10.0, 10.0))],
}


@pytest.mark.parametrize("name", list(UNSUPPORTED))
def test_unsupported_cases_leave_the_image_alone(gpu_ctx, name):
    regions = UNSUPPORTED[name]
    img = cc_lib.scene(67, 45, seed=13, nans=False)
    assert cc_lib.color_correction(img, regions) is None
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in img]
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        gpu_ctx.color_correction(capi.RGB(*[capi.device_plane(t) for t in d]), regions, O.REC2020_WS_D, O.REC2020_IWS_D)
    gpu_ctx.synchronize()
    assert all(np.array_equal(_bits(t.cpu().numpy()), _bits(a)) for t, a in zip(d, img))
    host = [np.array(a) for a in img]
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        gpu_ctx.color_correction(capi.host_rgb(host), regions, O.REC2020_WS_D, O.REC2020_IWS_D, True, want_info=True)
    assert all(np.array_equal(_bits(h), _bits(a)) for h, a in zip(host, img))


def test_bad_arguments_are_einval(gpu_ctx):
    img = cc_lib.scene(67, 45, seed=13, nans=False)
    wrong = np.ones((45, 66), np.float32)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
        gpu_ctx.color_correction(capi.host_rgb([np.array(a) for a in img]), [dict(mode=cc_lib.YUV, lmask=capi.host_plane(wrong))], O.REC2020_WS_D, O.REC2020_IWS_D)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
        gpu_ctx.color_correction(capi.host_rgb([np.array(a) for a in img]), [dict(mode=7)], O.REC2020_WS_D, O.REC2020_IWS_D)
    assert capi.LIB.artgpu_set_pipeline_color_correction(gpu_ctx._h, None, 2, None) == -1
    assert capi.LIB.artgpu_set_pipeline_color_correction(gpu_ctx._h, None, -1, None) == -1


# two regions with generateMasks' planes: a hue / chroma / lightness mask with a blur, and an inverted one with an opacity
GEN_MASKS = [mk_lib.mask(parametric_enabled=True, hue=mk_lib.HUE_A, chromaticity=mk_lib.CHROMA_A, lightness=mk_lib.LIGHT_A, blur=2.0),
             mk_lib.mask(parametric_enabled=True, lightness=mk_lib.LIGHT_A, inverted=True, opacity=60)]
GEN_REGIONS = [dict(mode=cc_lib.YUV, **cc_lib.VARIANTS["compression"]), dict(mode=cc_lib.RGB, in_saturation=30.0, **cc_lib.VARIANTS["pivot"])]


def _capi_masks(masks):
    return [{k: v for k, v in m.items() if not (k == "area" and v is None)} for m in masks]


def test_generated_masks_feed_the_tool(gpu_ctx):
    """artgpu_generate_masks(Lmask, abmask) on the RGB image, then the tool on the same planes without leaving the device, against
    the masks checker feeding the colour-correction checker"""
    w, h = 131, 97
    img = mk_lib.scene(w, h, seed=3)
    rc, L, ab, _, _ = mk_lib.generate(img, capi.MASKS_MODE_RGB, GEN_MASKS, want_L=True, want_ab=True)
    assert rc == 0
    assert not np.array_equal(L[0], ab[0]), "the two planes of a blurred region differ (their guided radii do)"
    regions = [dict(r, lmask=L[i], abmask=ab[i]) for i, r in enumerate(GEN_REGIONS)]
    want, want_info, oor, _ = cc_lib.color_correction(img, regions, to_rgb=True)
    assert not oor.any()
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in img]
    dimg = capi.RGB(*[capi.device_plane(t) for t in d])
    dL = torch.full((2, h, w), float("nan"), device="cuda:0")
    dab = torch.full((2, h, w), float("nan"), device="cuda:0")
    Lp, abp = [capi.device_plane(dL[i]) for i in range(2)], [capi.device_plane(dab[i]) for i in range(2)]
    gpu_ctx.generate_masks(dimg, capi.MASKS_MODE_RGB, O.REC2020_WS_D, _capi_masks(GEN_MASKS), Lmask=Lp, abmask=abp)
    info = gpu_ctx.color_correction(dimg, [dict(r, lmask=Lp[i], abmask=abp[i]) for i, r in enumerate(GEN_REGIONS)], O.REC2020_WS_D, O.REC2020_IWS_D, True,
                                    want_info=True)
    gpu_ctx.synchronize()
    assert [cc_lib.info_fields(i) for i in info] == [cc_lib.info_fields(i) for i in want_info]
    cc_lib.assert_same([t.cpu().numpy() for t in d], want, oor, "generated masks")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the per-frame pipe
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pipeline(ctx, raw, p):
    h, w = raw.shape
    b = p.border
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    ctx.synchronize()
    return [t.cpu().numpy() for t in d_img]


def _pipe_params():
    """demosaic, getImage, exposure: everything behind colour correction and texture boost off, so that the frame ahead of the tool is what
    a run without it returns"""
    p = _params(_lut(), 0)
    p.denoise_enabled = 0
    p.tone_enabled = 0
    return p


def _yuv_to_rgb(planes):
    """Imagefloat::setMode(RGB) on copies of three planes in YUV mode (the oracle's restatement)"""
    out = [np.array(a, dtype=np.float32, order="C") for a in planes]
    h, w = out[0].shape
    fp = C.POINTER(C.c_float)
    ptrs = (fp * 3)(*[a.ctypes.data_as(fp) for a in out])
    wsf = (C.c_float * 9)(*[float(np.float32(v)) for v in np.asarray(O.REC2020_WS_D).ravel()])
    O.lib().oracle_yuv_to_rgb(ptrs, C.c_size_t(w), w, h, wsf)
    return out


PIPE_REGIONS = [dict(mode=cc_lib.YUV, hueshift=20.0, **cc_lib.VARIANTS["compression"]), dict(mode=cc_lib.RGB, rgbluminance=True, **cc_lib.VARIANTS["pivot"])]
W, H = 392, 296


def test_pipeline_setting_set_and_cleared(gpu_ctx):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=41, noise=1500)
    p = _pipe_params()
    plain = _pipeline(gpu_ctx, raw, p)
    mask = tb_lib.smooth_mask(W - 8, H - 8)
    regions = [dict(PIPE_REGIONS[0], lmask=mask, abmask=mask), dict(PIPE_REGIONS[1])]
    keep = []
    try:
        gpu_ctx.set_pipeline_color_correction(_capi_regions(regions, True, W - 8, H - 8, keep))
        got = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_color_correction(None)
    want, _, oor, _ = cc_lib.color_correction(plain, regions, to_rgb=True)
    assert not oor.any()
    cc_lib.assert_same(got, want, oor, "pipe")
    assert not np.array_equal(got[1], plain[1])
    again = _pipeline(gpu_ctx, raw, p)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, plain)), "clearing the setting restores the frame"


def test_pipeline_generates_both_planes(gpu_ctx):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=42, noise=1500)
    p = _pipe_params()
    plain = _pipeline(gpu_ctx, raw, p)
    try:
        gpu_ctx.set_pipeline_color_correction(GEN_REGIONS, _capi_masks(GEN_MASKS))
        got = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_color_correction(None)
    rc, L, ab, _, _ = mk_lib.generate(plain, capi.MASKS_MODE_RGB, GEN_MASKS, want_L=True, want_ab=True, full_w=W - 8, full_h=H - 8, scale=1.0)
    assert rc == 0
    want, _, oor, _ = cc_lib.color_correction(plain, [dict(r, lmask=L[i], abmask=ab[i]) for i, r in enumerate(GEN_REGIONS)], to_rgb=True)
    assert not oor.any()
    cc_lib.assert_same(got, want, oor, "pipe, generated masks")


def test_pipeline_hands_yuv_to_texture_boost(gpu_ctx):
    """with texture boost behind it the image stays in YUV mode between the tools: one trip to YUV, the regions of both tools, one trip back"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=43, noise=1500)
    p = _pipe_params()
    plain = _pipeline(gpu_ctx, raw, p)
    arr, keep = capi.texture_boost_regions([(1.0, 0.2, 1, None)])
    p.texture_boost_enabled = 1; p.texture_boost_nregions = 1; p.texture_boost_regions = arr
    tb_only = _pipeline(gpu_ctx, raw, p)
    try:
        gpu_ctx.set_pipeline_color_correction(PIPE_REGIONS)
        got = _pipeline(gpu_ctx, raw, p)
        # pipe-generated texture-boost masks need an RGB image: unsupported behind colour correction, before any stage runs
        gpu_ctx.set_pipeline_masks(None, _capi_masks([mk_lib.mask(parametric_enabled=True, lightness=mk_lib.LIGHT_A)]))
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
            _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_masks(None, None)
        gpu_ctx.set_pipeline_color_correction(None)
    yuv, _, oor, _ = cc_lib.color_correction(plain, PIPE_REGIONS, to_rgb=False)
    assert not oor.any()
    Y, _, _ = tb_lib.texture_boost_plane(yuv[1], 1.0, 0.2)
    Y = (np.float32(1.0) * Y + (np.float32(1.0) - np.float32(1.0)) * yuv[1]).astype(np.float32)      # intp(1.f, Y_new, Y): the region's blend without a mask
    want = _yuv_to_rgb([yuv[0], Y, yuv[2]])
    cc_lib.assert_same(got, want, oor, "pipe, texture boost behind")
    assert not np.array_equal(got[1], tb_only[1])
    del keep


def test_batch_of_two_frames_on_two_lanes():
    p = _pipe_params()
    raws = [synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=s, noise=1500) for s in (45, 46)]
    ctx = capi.Context(0)
    plain = [_pipeline(ctx, r, p) for r in raws]
    ctx.set_batch_lanes(2)
    ctx.set_pipeline_color_correction(PIPE_REGIONS)
    outs = [[np.zeros((H - 8, W - 8), np.float32) for _ in range(3)] for _ in raws]
    ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
    for pl, o in zip(plain, outs):
        want, _, oor, _ = cc_lib.color_correction(pl, PIPE_REGIONS, to_rgb=True)
        cc_lib.assert_same(o, want, oor, "batch lane")
    assert not np.array_equal(outs[0][1], outs[1][1])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# artgpu-cli
# ---------------------------------------------------------------------------------------------------------------------------------------
CLI_FLAG = "rgb,slope=1.15:0.9:1.05,offset=0.04:-0.3:0.03,power=1.2:0.85:1.1,pivot=0.8:1.2:0.6,in_saturation=25"
CLI_REGION = dict(mode=cc_lib.RGB, in_saturation=25.0, **cc_lib.VARIANTS["pivot"])


def _cli_stages(ctx, raw, regions, convert=True):
    h, w = raw.shape
    b = 4
    d_raw = torch.from_numpy(raw).to("cuda:0")
    dem = [torch.empty((h, w), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    planes = capi.RGB(*[capi.device_plane(t) for t in dem])
    ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), synth.FILTERS_RGGB, 1.0, b, planes)
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    if convert:
        ctx.get_image(planes, b, b, MUL, True, None, img)
        ctx.convert_color_space(img, MAT)
    else:
        ctx.get_image(planes, b, b, MUL, True, MAT, img)
    ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    if regions is not None:
        ctx.color_correction(img, regions, O.REC2020_WS_D, O.REC2020_IWS_D, True)
    ctx.tone_curve(img, tone_lut() if convert else _lut(), 1.0, True)
    ctx.synchronize()
    return [t.cpu().numpy() for t in d_img]


def test_cli_color_correction_through_stage_2(gpu_ctx, tmp_path):
    """artgpu-cli --color-correction (ImProcFunctions::process(STAGE_2) -> ImProcFunctions::colorCorrection in the C++ mirror, behind the
    sharpening) equals the same stages called one by one"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=42, noise=1200)
    _, without = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3"])
    _, got = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--color-correction", CLI_FLAG])
    assert not np.array_equal(got, without)
    planes = _cli_stages(gpu_ctx, raw, [CLI_REGION])
    want = np.stack([np.rint(np.clip(t, 0, 65535)).astype(np.uint16) for t in planes], axis=-1)
    assert np.array_equal(got, want)
    # with a generated mask the result differs from the unmasked one
    _, masked = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--color-correction", CLI_FLAG, "--color-correction-mask", "0.2,0.7"])
    assert not np.array_equal(masked, got) and not np.array_equal(masked, without)


def test_cli_batch_queue_with_color_correction(gpu_ctx, tmp_path):
    w, h, black = W, H, 64.0
    frames = [np.clip(synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=50 + k, noise=1500), 0, 65535).astype(np.uint16) for k in range(2)]
    names = []
    for k, f in enumerate(frames):
        n = tmp_path / f"f{k}.u16"
        f.astype("<u2").tofile(n)
        names.append(str(n))
    res = subprocess.run([CLI, "--batch", ",".join(names), "--width", str(w), "--height", str(h), "--lanes", "2", "--black", str(black),
                          "--expcomp", "0.3", "--color-correction", CLI_FLAG, "--out", str(tmp_path / "o")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    assert json.loads(res.stdout.strip().splitlines()[-1])["frames"] == 2
    for k, f in enumerate(frames):
        raw = np.maximum(f.astype(np.float32) - np.float32(black), np.float32(0.0))          # scaleColors with scale_mul 1
        want = O.get_scanlines(_cli_stages(gpu_ctx, raw, [CLI_REGION], convert=False), 16, False)
        got = read_ppm16(tmp_path / f"o.{k}.ppm")
        assert np.array_equal(got, want), (k, int((got != want).sum()))
        plain = O.get_scanlines(_cli_stages(gpu_ctx, raw, None, convert=False), 16, False)
        assert not np.array_equal(got, plain)
