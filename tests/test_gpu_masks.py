"""GPU: artgpu_generate_masks (rtengine::generateMasks' parametric path, masks.cc:1037-1516) against the CPU checker (tests/mk_lib.py:
tests/emul/masks_ref.cc around the oracle's guided filter, FlatCurve, rgb2lab, xatan2f / xlin2log, rescaleBilinear and gaussian).

Every comparison is equality of float32 bit patterns: the planes and every field of artgpu_masks_info.  The cases and the branches they take
are listed in mk_lib.CASES and checked from the checker's counters in tests/test_masks_checker.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from art_amd import capi
import oracle_lib as O
import mk_lib

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _capi_masks(masks, area_device=False):
    """mk_lib's region dicts -> what capi.mask_params() takes; the area planes on the host or on the device (rows five floats longer)"""
    out, keep = [], []
    for m in masks:
        m = dict(m)
        if m["area"] is not None:
            if area_device:
                h, w = m["area"].shape
                t = torch.full((h, w + 5), float("nan"), dtype=torch.float32, device="cuda:0")
                t[:, :w].copy_(torch.from_numpy(np.array(m["area"])))
                keep.append(t)
                m["area"] = capi.device_plane(t[:, :w])
            else:
                a = np.array(m["area"], dtype=np.float32)
                keep.append(a)
                m["area"] = capi.host_plane(a)
        out.append(m)
    return out, keep


def _run(ctx, name, where="host", area_device=False, image_device=False):
    """artgpu_generate_masks on a case of mk_lib -> (L planes or None, ab planes or None, [MasksInfo]).  where: the output planes on the
    "host", on the "device", or "strided" (device rows seven floats longer than w, checked for writes past the row)"""
    img, mode, masks, kw, _, _, _, _ = mk_lib.case(name)
    h, w = img[0].shape
    n = len(masks)
    cm, keep = _capi_masks(masks, area_device)
    if image_device:
        ibuf = torch.stack([torch.from_numpy(np.array(a)) for a in img]).to("cuda:0")
        image = capi.RGB(*[capi.device_plane(ibuf[c]) for c in range(3)])
    else:
        himg = [np.array(a) for a in img]
        image = capi.host_rgb(himg)
    sets, bufs = [], []
    for want in (kw["want_L"], kw["want_ab"]):
        if not want:
            sets.append(None); bufs.append(None)
        elif where == "host":
            b = np.full((n, h, w), np.nan, np.float32)
            bufs.append(b); sets.append([capi.host_plane(b[i]) for i in range(n)])
        else:
            pad = 7 if where == "strided" else 0
            b = torch.full((n, h, w + pad), float("nan"), dtype=torch.float32, device="cuda:0")
            bufs.append(b); sets.append([capi.device_plane(b[i, :, :w]) for i in range(n)])
    info = ctx.generate_masks(image, mode, O.REC2020_WS_D, cm, kw["full_w"], kw["full_h"], kw["scale"], sets[0], sets[1], want_info=True)
    ctx.synchronize()
    del keep
    got = []
    for b in bufs:
        if b is None:
            got.append(None)
        elif where == "host":
            got.append(b)
        else:
            if where == "strided":
                assert bool(torch.isnan(b[:, :, w:]).all()), "wrote past the row"
            got.append(b[:, :, :w].cpu().numpy())
    return got[0], got[1], info


def _assert_same(got, want, what):
    assert (got is None) == (want is None), what
    if got is None:
        return
    bad = [int((_bits(g) != _bits(w)).sum()) for g, w in zip(got, want)]
    worst = [float(np.nanmax(np.abs(np.asarray(g, np.float64) - np.asarray(w, np.float64)))) for g, w in zip(got, want)]
    print(f"masks {what}: values that differ from the checker, per region: {bad} (largest difference {worst})")
    assert not any(bad), (what, bad, worst)


@pytest.mark.parametrize("name", list(mk_lib.CASES))
def test_planes_and_info_equal_the_checker(gpu_ctx, name):
    _, _, _, _, wantL, wantab, want_info, _ = mk_lib.case(name)
    L, ab, info = _run(gpu_ctx, name, "host")
    print(f"masks {name}: info {[mk_lib.info_fields(i) for i in info]} checker {[mk_lib.info_fields(i) for i in want_info]}")
    assert [mk_lib.info_fields(i) for i in info] == [mk_lib.info_fields(i) for i in want_info]
    _assert_same(L, wantL, name + " L")
    _assert_same(ab, wantab, name + " ab")


@pytest.mark.parametrize("name", ["67x45-rgb-both-three-regions", "256x131-lab-both-threshold+30-area", "256x131-rgb-L-posterize"])
@pytest.mark.parametrize("where", ["device", "strided"])
def test_device_and_strided_outputs(gpu_ctx, name, where):
    _, _, _, _, wantL, wantab, want_info, _ = mk_lib.case(name)
    L, ab, info = _run(gpu_ctx, name, where, area_device=True, image_device=True)
    assert [mk_lib.info_fields(i) for i in info] == [mk_lib.info_fields(i) for i in want_info]
    _assert_same(L, wantL, f"{name} L ({where})")
    _assert_same(ab, wantab, f"{name} ab ({where})")


def test_scale_two_halves_the_radii(gpu_ctx):
    """the five-region case runs at scale 2: r1 = max(int(4 / 2 * blur + 0.5), 1)"""
    _, _, _, _, _, _, want_info, _ = mk_lib.case("67x45-rgb-ab-five-regions")
    assert [(i.r1, i.r2) for i in want_info] == [(2, 13), (2, 13), (4, 25), (2, 13), (2, 13)]


UNSUPPORTED = {
    "deltae": dict(deltae_enabled=True), "drawn": dict(drawn_enabled=True), "external": dict(external_enabled=True),
    "linked": dict(linked_enabled=True), "mask-curve": dict(curve_is_identity=False), "show-mask": dict(show_mask=True),
}


def _expect_unsupported(ctx, img, mode, masks, full_w=-1, full_h=-1, both=True):
    h, w = img[0].shape
    n = len(masks)
    outs = [np.full((n, h, w), -7.25, np.float32) for _ in range(2 if both else 1)]
    sets = [[capi.host_plane(o[i]) for i in range(n)] for o in outs] + ([None] if not both else [])
    cm, keep = _capi_masks(masks)
    arr, keep2 = capi.mask_params(cm)
    wsd = (C.c_double * 9)(*np.asarray(O.REC2020_WS_D, np.float64).ravel())
    pl = [(capi.Plane * n)(*s) if s is not None else None for s in sets]
    himg = [np.array(a) for a in img]
    rc = capi.LIB.artgpu_generate_masks(ctx._h, C.byref(capi.host_rgb(himg)), int(mode), wsd, arr, n, full_w, full_h, 1.0, pl[0], pl[1], None)
    assert rc == -4, rc                                                      # ARTGPU_EUNSUPPORTED
    for o in outs:
        assert np.all(o == np.float32(-7.25)), "the output was touched"
    return capi.LIB.artgpu_last_error(ctx._h).decode()


@pytest.mark.parametrize("what", list(UNSUPPORTED))
def test_unsupported_masks_leave_the_output_untouched(gpu_ctx, what):
    img = mk_lib.scene(67, 45, seed=3)
    masks = [mk_lib.mask(parametric_enabled=True, hue=mk_lib.HUE_A), mk_lib.mask(parametric_enabled=True, hue=mk_lib.HUE_A, **UNSUPPORTED[what])]
    rc, *_ = mk_lib.generate(img, mk_lib.MODE_RGB, masks)
    assert rc == mk_lib.EUNSUPPORTED
    msg = _expect_unsupported(gpu_ctx, img, mk_lib.MODE_RGB, masks)
    assert "region 1" in msg, msg


@pytest.mark.parametrize("mode", [mk_lib.MODE_YUV, mk_lib.MODE_XYZ])
def test_unsupported_modes(gpu_ctx, mode):
    img = mk_lib.scene(67, 45, seed=3)
    masks = [mk_lib.mask(parametric_enabled=True, hue=mk_lib.HUE_A)]
    assert mk_lib.generate(img, mode, masks)[0] == mk_lib.EUNSUPPORTED
    _expect_unsupported(gpu_ctx, img, mode, masks)


def test_unsupported_sizes(gpu_ctx):
    """below ARTGPU_MASKS_MIN_SIZE; and a lightness-detail radius of 907 (a prime: subsampling 1) on a plane large enough for the box radius
    to stay above the 900 the blur kernels hold"""
    assert capi.MASKS_MIN_SIZE == 8
    small = [np.full((7, 9), 1000.0, np.float32) for _ in range(3)]
    msg = _expect_unsupported(gpu_ctx, small, mk_lib.MODE_RGB, [mk_lib.mask(parametric_enabled=True, hue=mk_lib.HUE_A)])
    assert "below" in msg, msg
    big = [np.full((1820, 1824), 1000.0, np.float32) for _ in range(3)]
    msg = _expect_unsupported(gpu_ctx, big, mk_lib.MODE_RGB, [mk_lib.mask(parametric_enabled=True, lightness=mk_lib.LIGHT_A)], full_w=907 * 30,
                              both=False)
    assert "box radius" in msg, msg


def test_smallest_plane(gpu_ctx):
    """8 x 8 with every stage on: the guided filters' box radii are clamped by f_mean, buildBlendMask's frame is most of the plane"""
    img = mk_lib.scene(8, 8, seed=5)
    masks = [mk_lib.mask(parametric_enabled=True, hue=mk_lib.HUE_A, lightness=mk_lib.LIGHT_A, lightness_detail=50, contrast_threshold=30,
                         posterization=3, smoothing=60, opacity=40)]
    rc, wantL, wantab, want_info, _ = mk_lib.generate(img, mk_lib.MODE_RGB, masks, want_L=True, want_ab=True)
    assert rc == 0
    L, ab = np.full((1, 8, 8), np.nan, np.float32), np.full((1, 8, 8), np.nan, np.float32)
    cm, keep = _capi_masks(masks)
    info = gpu_ctx.generate_masks(capi.host_rgb([np.array(a) for a in img]), mk_lib.MODE_RGB, O.REC2020_WS_D, cm, -1, -1, 1.0,
                                  [capi.host_plane(L[0])], [capi.host_plane(ab[0])], want_info=True)
    assert [mk_lib.info_fields(i) for i in info] == [mk_lib.info_fields(i) for i in want_info]
    _assert_same(L, wantL, "8x8 L")
    _assert_same(ab, wantab, "8x8 ab")


# ---- the per-frame pipe: artgpu_set_pipeline_masks ----
from art_amd import synth                                         # noqa: E402
import lc_lib                                                     # noqa: E402
from test_gpu_cli import MAT, MUL, run_cli, tone_lut              # noqa: E402
from test_gpu_pipeline import _lut, _params                       # noqa: E402

TB_REGIONS = [(1.0, 0.2, 1), (-0.8, 1.0, 1)]
TB_MASKS = [mk_lib.mask(parametric_enabled=True, lightness=mk_lib.LIGHT_A, lightness_detail=50, blur=1.0),
            mk_lib.mask(parametric_enabled=True, hue=mk_lib.HUE_A, contrast_threshold=30, posterization=3, smoothing=60, opacity=70)]
LC_MASKS = [mk_lib.mask(parametric_enabled=True, chromaticity=mk_lib.CHROMA_A, lightness=mk_lib.LIGHT_B, lightness_detail=100, inverted=True)]


def _pipeline(ctx, raw, p):
    h, w = raw.shape
    b = p.border
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    ctx.synchronize()
    return d_img


def _generated(ctx, img, mode, masks, w, h):
    """artgpu_generate_masks' L planes for a device image -> (tensor, [Plane])"""
    t = torch.full((len(masks), h, w), float("nan"), dtype=torch.float32, device="cuda:0")
    planes = [capi.device_plane(t[i]) for i in range(len(masks))]
    ctx.generate_masks(img, mode, O.REC2020_WS_D, masks, w, h, 1.0, planes, None)
    return t, planes


def _stages(ctx, raw, tb_masks=None, lc_masks=None, tb=True, lc=False, null_masks=False):
    """demosaic, get_image, exposure, [generate_masks +] texture boost, tone curve, [rgb_to_lab, generate_masks, local contrast, lab_to_rgb]
    through the individual entry points: the plane-fed path the pipe had before it could generate its masks"""
    h, w = raw.shape
    d_raw = torch.from_numpy(raw).to("cuda:0")
    dem = [torch.empty((h, w), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    planes = capi.RGB(*[capi.device_plane(t) for t in dem])
    ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), synth.FILTERS_RGGB, 1.0, 4, planes)
    d_img = [torch.empty((h - 8, w - 8), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    ctx.get_image(planes, 4, 4, MUL, True, MAT, img)
    ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    keep = []
    if tb:
        mp = [None] * len(TB_REGIONS)
        if tb_masks is not None:
            t, mp = _generated(ctx, img, mk_lib.MODE_RGB, tb_masks, w - 8, h - 8)
            keep.append(t)
        ctx.texture_boost(img, [r + (m,) for r, m in zip(TB_REGIONS, mp)], O.REC2020_WS_D, 1.0, True, True)
    ctx.tone_curve(img, _lut(), 1.0, True)
    if lc:
        ctx.rgb_to_lab(img, O.REC2020_WS_D)
        mp = [None]
        if lc_masks is not None:
            t, mp = _generated(ctx, img, mk_lib.MODE_LAB, lc_masks, w - 8, h - 8)
            keep.append(t)
        ctx.local_contrast(img.g, [(60.0, lc_lib.curve_lut(lc_lib.BOOST_CURVE_POINTS), mp[0])])
        ctx.lab_to_rgb(img, O.REC2020_IWS_D)
    ctx.synchronize()
    return d_img


def _pipe_params(ctx, tb_masks=None, lc_masks=None, lc=False):
    """the frame's parameters; the masks become the context's setting (None: cleared)"""
    ctx.set_pipeline_masks(lc_masks if lc else None, tb_masks)
    lut = _lut()
    p = _params(lut, 0)
    p.denoise_enabled = 0
    keep = [lut]                                   # (the parameters point at the tone LUT)
    arr, k = capi.texture_boost_regions([r + (None,) for r in TB_REGIONS])
    keep += [arr, k]
    p.texture_boost_enabled = 1; p.texture_boost_nregions = len(TB_REGIONS); p.texture_boost_regions = arr
    if lc:
        la, k = capi.local_contrast_regions([(60.0, lc_lib.curve_lut(lc_lib.BOOST_CURVE_POINTS), None)])
        keep += [la, k]
        p.local_contrast_enabled = 1; p.local_contrast_nregions = 1; p.local_contrast_regions = la
    return p, keep


def _same(got, want, what):
    bad = [int((a.view(torch.int32) != b.view(torch.int32)).sum()) for a, b in zip(got, want)]
    print(f"masks pipeline {what}: values that differ, per plane: {bad}")
    assert not any(bad), (what, bad)


def test_pipeline_masks_equal_generate_masks_plus_the_plane_fed_run(gpu_ctx):
    w, h = 392, 296
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=61, noise=1500)
    # the new fields NULL: the parent's path, which is the plane-fed call with a NULL mask
    p, keep = _pipe_params(gpu_ctx, lc=True)
    plain = _pipeline(gpu_ctx, raw, p)
    _same(plain, _stages(gpu_ctx, raw, lc=True), "NULL fields")
    # texture boost
    p, keep = _pipe_params(gpu_ctx, tb_masks=TB_MASKS)
    got = _pipeline(gpu_ctx, raw, p)
    _same(got, _stages(gpu_ctx, raw, tb_masks=TB_MASKS), "texture_boost_masks")
    assert not torch.equal(got[1], _stages(gpu_ctx, raw)[1])
    # local contrast, with texture boost's masks beside it
    p, keep = _pipe_params(gpu_ctx, tb_masks=TB_MASKS, lc_masks=LC_MASKS, lc=True)
    got = _pipeline(gpu_ctx, raw, p)
    _same(got, _stages(gpu_ctx, raw, tb_masks=TB_MASKS, lc_masks=LC_MASKS, lc=True), "both tools")
    assert not torch.equal(got[1], plain[1])
    # what generateMasks does not support fails the frame before any stage has run
    bad = [dict(m) for m in TB_MASKS]
    bad[1]["deltae_enabled"] = True
    p, keep = _pipe_params(gpu_ctx, tb_masks=bad)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        _pipeline(gpu_ctx, raw, p)
    # a count that is not the frame's region count
    gpu_ctx.set_pipeline_masks(None, TB_MASKS[:1])
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
        _pipeline(gpu_ctx, raw, p)
    # cleared: the session's other tests see the default
    gpu_ctx.set_pipeline_masks(None, None)
    p, keep = _pipe_params(gpu_ctx, lc=True)
    _same(_pipeline(gpu_ctx, raw, p), plain, "cleared")
    del keep


def test_batch_of_two_frames_on_two_lanes_with_masks():
    w, h = 392, 296
    ctx = capi.Context(0)
    p, keep = _pipe_params(ctx, tb_masks=TB_MASKS, lc_masks=LC_MASKS, lc=True)
    raws = [synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=s, noise=1500) for s in (65, 66)]
    outs = [[np.zeros((h - 8, w - 8), np.float32) for _ in range(3)] for _ in raws]
    ctx.set_batch_lanes(2)
    ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
    for r, o in zip(raws, outs):
        want = _stages(ctx, r, tb_masks=TB_MASKS, lc_masks=LC_MASKS, lc=True)
        for a, t in zip(o, want):
            assert np.array_equal(_bits(a), _bits(t.cpu().numpy())) and a.max() > 0
    assert not np.array_equal(outs[0][1], outs[1][1])
    ctx.close()
    del keep


def test_cli_texture_boost_mask(gpu_ctx, tmp_path):
    """artgpu-cli --texture-boost 1.0,0.2,1 --texture-boost-mask 0.2,0.6,1,50,30,70: ImProcFunctions::textureBoost of the C++ mirror generates
    the region's plane through ImProcFunctions::generateMasks and equals the entry points called one by one"""
    w, h, filt, b = 392, 296, synth.FILTERS_RGGB, 4
    raw = synth.bayer_frame(w, h, filt, seed=62, noise=1200)
    _, unmasked = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--texture-boost", "1.0,0.2,1"])
    _, got = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--texture-boost", "1.0,0.2,1", "--texture-boost-mask", "0.2,0.6,1,50,30,70"])
    assert not np.array_equal(got, unmasked)
    light = (1.0, 0.0, 0.0, 0.35, 0.35, 0.2, 1.0, 0.35, 0.35, 0.6, 1.0, 0.35, 0.35, 1.0, 0.0, 0.35, 0.35)
    m = mk_lib.mask(parametric_enabled=True, lightness=light, blur=1.0, lightness_detail=50, contrast_threshold=30, opacity=70)
    d_raw = torch.from_numpy(raw).to("cuda:0")
    dem = [torch.empty((h, w), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    planes = capi.RGB(*[capi.device_plane(t) for t in dem])
    gpu_ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), filt, 1.0, b, planes)
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    gpu_ctx.get_image(planes, b, b, MUL, True, None, img)
    gpu_ctx.convert_color_space(img, MAT)
    gpu_ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    t = torch.empty((1, h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0")
    gpu_ctx.generate_masks(img, mk_lib.MODE_RGB, O.REC2020_WS_D, [m], -1, -1, 1.0, [capi.device_plane(t[0])], None)
    gpu_ctx.texture_boost(img, [(1.0, 0.2, 1, capi.device_plane(t[0]))], O.REC2020_WS_D, 1.0, True, True)
    gpu_ctx.tone_curve(img, tone_lut(), 1.0, True)
    gpu_ctx.synchronize()
    want = np.stack([np.rint(np.clip(t.cpu().numpy(), 0, 65535)).astype(np.uint16) for t in d_img], axis=-1)
    assert np.array_equal(got, want)
