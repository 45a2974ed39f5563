"""GPU: impulse noise reduction (artgpu_impulse_denoise = ImProcFunctions::impulsedenoise, impulse_denoise.cc:33-189) and defringe (artgpu_defringe =
ImProcFunctions::defringe, PF_correct_RT.cc:44-218) against the CPU checker (tests/id_lib.py: tests/emul/impulse_defringe_ref.cc).

Every operation of both tools is an IEEE float or double add, multiply, divide or comparison in a fixed order, the sleef atan2 and the Lab
conversions the library already reproduces bit for bit, so every comparison is bit for bit on all three planes, and `info` field by field.
For defringe the checker runs order 0, the definition of include/artgpu.h (every window reads the tool's input); its chromave is summed in the
defined order.  The sizes (id_lib.SIZES) are the smallest that reach every branch: the gates' minimum, windows clamped on both sides at once,
every W mod 4 tail, and 67 x 70, which crosses the averaging kernel's 32 x 32 tile twice in each direction with the largest halo (and the
impulse kernel's 64 x 16 tile).  tests/test_impulse_defringe_checker.py shows that every scene flags a share of its pixels."""
import numpy as np
import pytest
import torch

from art_amd import capi
import id_lib as I
import layout_lib as LL

pytestmark = pytest.mark.gpu


def _run(ctx, call, img, layout=LL.DENSE, **kw):
    """`call` on device-resident copies of the planes in `layout`; (planes, what the call returned), after checking the words around the image"""
    ar = LL.arena(layout, img)
    ret = call(ar.rgb, **kw)
    ctx.synchronize()
    return LL.check(ar, repr(layout)), ret


def _same(got, want, what):
    bad = [I.nbad(g, w) for g, w in zip(got, want)]
    print(f"{what}: values that differ from the checker, per plane: {bad}")
    assert bad == [0, 0, 0], (what, bad)


def _imp(ctx, thresh, scale, to_rgb=True, enabled=True, want_info=True):
    p = capi.impulse_denoise_params(enabled, thresh)
    return lambda rgb: ctx.impulse_denoise(rgb, p, I.WS, I.IWS if to_rgb else None, scale, to_rgb, want_info=want_info)


def _df(ctx, radius, scale, threshold, curve="default", to_rgb=True, enabled=True, want_info=True):
    p = capi.defringe_params(enabled, radius, threshold, I.CURVES[curve])
    return lambda rgb: ctx.defringe(rgb, p, I.WS, I.IWS if to_rgb else None, scale, to_rgb, want_info=want_info)


# ---- impulse noise reduction

@pytest.mark.parametrize("w,h", I.SIZES)
def test_impulse_image_and_info_equal_the_checker(gpu_ctx, w, h):
    for k, (thresh, scale) in enumerate(I.IMPULSE_PARAMS):
        img, want, want_info, _ = I.impulse_case(w, h, thresh, scale)
        layout = list(LL.LAYOUTS.values())[k % len(LL.LAYOUTS)]       # row-padded and offset device images, guard words around them
        got, info = _run(gpu_ctx, _imp(gpu_ctx, thresh, scale), img, layout)
        print(f"impulse {w}x{h} thresh {thresh} scale {scale}: info {I.impulse_info_fields(info)} checker {I.impulse_info_fields(want_info)}")
        assert I.impulse_info_fields(info) == I.impulse_info_fields(want_info)
        _same(got, want, f"impulse {w}x{h} thresh {thresh} scale {scale} {layout!r}")
        assert info.impulse_pixels > 0 and any(not np.array_equal(g, a) for g, a in zip(got, img))
    # host planes; without info the call gives the same planes
    img, want, want_info, _ = I.impulse_case(w, h, 50, 1.0)
    host = [np.array(a) for a in img]
    info = gpu_ctx.impulse_denoise(capi.host_rgb(host), capi.impulse_denoise_params(True, 50), I.WS, I.IWS, 1.0, True, want_info=True)
    assert I.impulse_info_fields(info) == I.impulse_info_fields(want_info)
    _same(host, want, f"impulse {w}x{h} host planes")
    got, none = _run(gpu_ctx, _imp(gpu_ctx, 50, 1.0, want_info=False), img)
    assert none is None
    _same(got, want, f"impulse {w}x{h} without info")


@pytest.mark.parametrize("w,h", I.BLOCK_SIZES)
def test_impulse_keeps_a_pixel_whose_whole_neighbourhood_is_impish(gpu_ctx, w, h):
    img, want, want_info, kept = I.impulse_case(w, h, 100, 1.0, to_rgb=False, block=True)
    assert kept >= 1
    got, info = _run(gpu_ctx, _imp(gpu_ctx, 100, 1.0, to_rgb=False), img, LL.LAYOUTS["mixed"])       # to_rgb 0: the image stays in LAB mode
    assert I.impulse_info_fields(info) == I.impulse_info_fields(want_info)
    _same(got, want, f"impulse {w}x{h} block, LAB out")


def test_impulse_gates_leave_the_image_alone(gpu_ctx):
    cases = [(w, h, True, 1.0) for w, h in I.GATE_SIZES] + [(11, 13, False, 1.0), (11, 13, True, 0.49), (11, 13, True, float("nan"))]
    for w, h, enabled, scale in cases:
        img = I.impulse_scene(w, h, seed=2)
        got, info = _run(gpu_ctx, _imp(gpu_ctx, 50, scale, enabled=enabled), img, LL.LAYOUTS["odd"])
        assert info.early_out == I.impulse_gate(w, h, enabled, scale) != 0 and info.impulse_pixels == 0
        assert all(np.array_equal(I.bits(a), I.bits(b)) for a, b in zip(got, img)), (w, h, enabled, scale)
    # scale 0.5 is inside the gate
    img, want, want_info, _ = I.impulse_case(11, 13, 50, 0.5)
    got, info = _run(gpu_ctx, _imp(gpu_ctx, 50, 0.5), img)
    assert info.early_out == 0 and I.impulse_info_fields(info) == I.impulse_info_fields(want_info)
    _same(got, want, "impulse 11x13 scale 0.5")
    # a missing inverse matrix with to_rgb is refused before anything runs
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in img]
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
        gpu_ctx.impulse_denoise(capi.RGB(*[capi.device_plane(t) for t in d]), capi.impulse_denoise_params(), I.WS, None, 1.0, True)
    gpu_ctx.synchronize()
    assert all(np.array_equal(I.bits(t.cpu().numpy()), I.bits(a)) for t, a in zip(d, img))


# ---- defringe

@pytest.mark.parametrize("w,h", I.SIZES + (I.DEFRINGE_WIDE,))
def test_defringe_image_and_info_equal_the_checker(gpu_ctx, w, h):
    k = 0
    for radius, scale in I.DEFRINGE_PARAMS:
        for threshold in I.DEFRINGE_THRESHOLDS:
            for curve in I.CURVES:
                img, res = I.defringe_case(w, h, radius, scale, threshold, curve)
                layout = list(LL.LAYOUTS.values())[k % len(LL.LAYOUTS)]
                k += 1
                if res is None:         # W < 2 halfwin - 2: refused, image untouched
                    ar = LL.arena(layout, img)
                    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
                        _df(gpu_ctx, radius, scale, threshold, curve)(ar.rgb)
                    gpu_ctx.synchronize()
                    assert all(np.array_equal(I.bits(a), I.bits(b)) for a, b in zip(LL.check(ar), img))
                    continue
                want, want_info, flagged = res
                got, info = _run(gpu_ctx, _df(gpu_ctx, radius, scale, threshold, curve), img, layout)
                what = f"defringe {w}x{h} radius {radius} scale {scale} threshold {threshold} curve {curve} {layout!r}"
                print(f"{what}: info {I.defringe_info_fields(info)} checker {I.defringe_info_fields(want_info)}")
                assert I.defringe_info_fields(info) == I.defringe_info_fields(want_info), what
                _same(got, want, what)
                assert info.corrected_pixels > 0
    # host planes; LAB out; without info
    img, res = I.defringe_case(w, h, 2.0, 1.0, 13)
    host = [np.array(a) for a in img]
    info = gpu_ctx.defringe(capi.host_rgb(host), capi.defringe_params(True, 2.0, 13), I.WS, I.IWS, 1.0, True, want_info=True)
    assert I.defringe_info_fields(info) == I.defringe_info_fields(res[1])
    _same(host, res[0], f"defringe {w}x{h} host planes")
    img, res = I.defringe_case(w, h, 2.0, 1.0, 13, to_rgb=False)
    got, none = _run(gpu_ctx, _df(gpu_ctx, 2.0, 1.0, 13, to_rgb=False, want_info=False), img, LL.LAYOUTS["mixed"])
    assert none is None
    _same(got, res[0], f"defringe {w}x{h} LAB out, without info")


def test_defringe_flat_image_takes_the_early_out(gpu_ctx):
    img, res = I.defringe_case(14, 9, 2.0, 1.0, 13, flat=True)
    want, want_info, flagged = res
    assert want_info.chromave == 0.0 and want_info.corrected_pixels == 0
    got, info = _run(gpu_ctx, _df(gpu_ctx, 2.0, 1.0, 13), img, LL.LAYOUTS["planar16"])
    assert I.defringe_info_fields(info) == I.defringe_info_fields(want_info)
    _same(got, want, "defringe flat image")


def test_defringe_gates_and_refusals_leave_the_image_alone(gpu_ctx):
    for w, h, enabled in [(w, h, True) for w, h in I.GATE_SIZES] + [(11, 13, False)]:
        img = I.fringe_scene(w, h, seed=2)
        got, info = _run(gpu_ctx, _df(gpu_ctx, 2.0, 1.0, 13, enabled=enabled), img, LL.LAYOUTS["odd"])
        assert info.early_out == (1 if not enabled else 2) and info.corrected_pixels == 0
        assert all(np.array_equal(I.bits(a), I.bits(b)) for a, b in zip(got, img))
    img = I.fringe_scene(67, 70, seed=2)
    refusals = [(-4, 25.0, 1.0), (-4, float("nan"), 1.0), (-4, float("inf"), 1.0), (-4, 5.0, 0.99), (-4, 2.0, 0.39), (-4, 5.5, 1.0),
                (-1, -1.0, 1.0), (-1, 2.0, 0.0), (-1, 2.0, -1.0)]
    for code, radius, scale in refusals:
        for host in (False, True):
            p = capi.defringe_params(True, radius, 13)
            if host:
                planes = [np.array(a) for a in img]
                with pytest.raises(capi.ArtGpuError, match=r"^\[%d\]" % code):
                    gpu_ctx.defringe(capi.host_rgb(planes), p, I.WS, I.IWS, scale)
                after = planes
            else:
                ar = LL.arena(LL.LAYOUTS["even_off"], img)
                with pytest.raises(capi.ArtGpuError, match=r"^\[%d\]" % code):
                    gpu_ctx.defringe(ar.rgb, p, I.WS, I.IWS, scale)
                gpu_ctx.synchronize()
                after = LL.check(ar)
            assert all(np.array_equal(I.bits(a), I.bits(b)) for a, b in zip(after, img)), (radius, scale, host)
    # the largest window there is: radius / scale == 5 exactly
    assert I.defringe(img, 2.0, 13, scale=0.4) is not None
    info = _run(gpu_ctx, _df(gpu_ctx, 2.0, 0.4, 13), img)[1]
    assert info.halfwin == capi.DEFRINGE_MAX_HALFWIN
    # a curve that is not one: nhuecurve without huecurve
    p = capi.defringe_params(True, 2.0, 13)
    p.huecurve = None
    ar = LL.arena(LL.DENSE, img)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
        gpu_ctx.defringe(ar.rgb, p, I.WS, I.IWS, 1.0)
    gpu_ctx.synchronize()
    assert all(np.array_equal(I.bits(a), I.bits(b)) for a, b in zip(LL.check(ar), img))


# ---- determinism

def test_two_runs_with_different_cu_reserve_give_the_same_bits(gpu_ctx):
    w, h = 67, 70
    img_i = I.impulse_case(w, h, 50, 1.0)[0]
    img_d = I.defringe_case(w, h, 5.0, 1.0, 13)[0]
    runs = []
    try:
        for reserve in (0, 7):
            gpu_ctx.set_option("cu_reserve", reserve)
            a, ia = _run(gpu_ctx, _imp(gpu_ctx, 50, 1.0), img_i, LL.LAYOUTS["planar16"])
            b, ib = _run(gpu_ctx, _df(gpu_ctx, 5.0, 1.0, 13), img_d, LL.LAYOUTS["planar16"])
            runs.append((a, bytes(ia), b, bytes(ib)))
    finally:
        gpu_ctx.set_option("cu_reserve", 0)
    assert runs[0][1] == runs[1][1] and runs[0][3] == runs[1][3]
    _same(runs[0][0], runs[1][0], "impulse, cu_reserve 0 against 7")
    _same(runs[0][2], runs[1][2], "defringe, cu_reserve 0 against 7")


# ---- lab_to_yuv on its own

@pytest.mark.parametrize("w,h", [(8, 8), (11, 13), (14, 9), (9, 8)])
def test_lab_to_yuv_is_the_lab_image_seen_in_yuv_mode(gpu_ctx, w, h):
    """Imagefloat::lab_to_yuv at every W mod 4: Y is bit for bit the Y of lab_to_rgb's XYZ step -- with the identity as inverse matrix lab_to_rgb
    returns X, Y, Z, and lab_to_yuv (g = Y, b = Y - B, r = R - Y) then gives Y, Y - Z, X - Y.  With the real matrix, R and B are lab_to_rgb's."""
    import oracle_lib as O
    lab = O.image_rgb_to_lab(I.fringe_scene(w, h, seed=3), I.WS)
    ident = np.eye(3)
    xyz = O.image_lab_to_rgb(lab, ident)                    # the oracle's restatement of Lab2XYZ, vector body and scalar tail
    rgb = O.image_lab_to_rgb(lab, I.IWS)
    for iws, (X, Yw, Z) in ((ident, xyz),):
        got, _ = _run(gpu_ctx, lambda r: gpu_ctx.lab_to_yuv(r, iws), lab, LL.LAYOUTS["odd"])
        _same(got, [X - Yw, Yw, Yw - Z], f"lab_to_yuv {w}x{h}, identity matrix")
    got, _ = _run(gpu_ctx, lambda r: gpu_ctx.lab_to_yuv(r, I.IWS), lab, LL.LAYOUTS["planar16"])
    _same(got, [rgb[0] - xyz[1], xyz[1], xyz[1] - rgb[2]], f"lab_to_yuv {w}x{h}")
    host = [np.array(a) for a in lab]
    gpu_ctx.lab_to_yuv(capi.host_rgb(host), I.IWS)
    _same(host, got, f"lab_to_yuv {w}x{h} host planes")


# ---- the per-frame pipe and the batch lanes

from test_gpu_colorcorrection import GEN_MASKS, GEN_REGIONS, PIPE_REGIONS as CC_REGIONS, _capi_masks, _pipe_params, _pipeline, _yuv_to_rgb      # noqa: E402
from test_gpu_smoothing import PIPE_REGIONS as SM_REGIONS      # noqa: E402
from art_amd import synth      # noqa: E402

PW, PH = 392, 296
IMP = capi.impulse_denoise_params(True, 80)
DF = capi.defringe_params(True, 2.0, 13)


def _stages(ctx, plain, imp, df, then="rgb"):
    """the tools one by one on the frame a pipe without them returns: the first switches to LAB, the image stays LAB, `then` is the hand-over"""
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in plain]
    rgb = capi.RGB(*[capi.device_plane(t) for t in d])
    lab = False
    if imp is not None:
        ctx.impulse_denoise(rgb, imp, I.WS, None, 1.0, to_rgb=False)
        lab = True
    if df is not None:
        ctx.defringe(rgb, df, None if lab else I.WS, None, 1.0, to_rgb=False, from_lab=lab)
    h, w = plain[0].shape
    if then == "rgb":
        ctx.lab_to_rgb(rgb, I.IWS)
    elif then == "cc":
        ctx.lab_to_yuv(rgb, I.IWS)
        ctx.color_correction(rgb, CC_REGIONS, I.WS, I.IWS, to_rgb=True, from_yuv=True)
    elif then == "cc-masks":
        dL = torch.full((2, h, w), float("nan"), device="cuda:0")
        dab = torch.full((2, h, w), float("nan"), device="cuda:0")
        Lp, abp = [capi.device_plane(dL[i]) for i in range(2)], [capi.device_plane(dab[i]) for i in range(2)]
        ctx.generate_masks(rgb, capi.MASKS_MODE_LAB, None, _capi_masks(GEN_MASKS), full_w=w, full_h=h, scale=1.0, Lmask=Lp, abmask=abp)
        ctx.lab_to_yuv(rgb, I.IWS)
        ctx.color_correction(rgb, [dict(r, lmask=Lp[i], abmask=abp[i]) for i, r in enumerate(GEN_REGIONS)], I.WS, I.IWS, to_rgb=True, from_yuv=True)
    elif then == "sm":
        ctx.lab_to_rgb(rgb, I.IWS)
        ctx.smoothing(rgb, SM_REGIONS, I.WS, 1.0)
    elif then == "tb":
        ctx.lab_to_yuv(rgb, I.IWS)
        ctx.texture_boost_plane(rgb.g, 1.0, 0.2)
    ctx.synchronize()
    out = [t.cpu().numpy() for t in d]
    if then == "tb":        # the region's blend without a mask, intp(1.f, Y_new, Y), and textureBoost's closing setMode(RGB)
        out = _yuv_to_rgb(out)
    return out


@pytest.fixture(scope="module")
def frame(gpu_ctx):
    raw = synth.bayer_frame(PW, PH, synth.FILTERS_RGGB, seed=51, noise=1500)
    p = _pipe_params()
    return raw, p, _pipeline(gpu_ctx, raw, p)


@pytest.mark.parametrize("imp,df,then", [(True, False, "rgb"), (False, True, "rgb"), (True, True, "rgb"), (True, True, "cc"), (True, True, "cc-masks"),
                                         (True, True, "sm"), (True, True, "tb")])
def test_pipeline_setting_equals_the_tools_one_by_one(gpu_ctx, frame, imp, df, then):
    raw, p, plain = frame
    p = capi.PipelineParams.from_buffer_copy(p)
    keep = None
    try:
        gpu_ctx.set_pipeline_impulse_defringe(IMP if imp else None, DF if df else None)
        if then == "cc":
            gpu_ctx.set_pipeline_color_correction(CC_REGIONS)
        elif then == "cc-masks":
            gpu_ctx.set_pipeline_color_correction(GEN_REGIONS, _capi_masks(GEN_MASKS))
        elif then == "sm":
            gpu_ctx.set_pipeline_smoothing(SM_REGIONS)
        elif then == "tb":
            arr, keep = capi.texture_boost_regions([(1.0, 0.2, 1, None)])
            p.texture_boost_enabled = 1; p.texture_boost_nregions = 1; p.texture_boost_regions = arr
        got = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_impulse_defringe(None, None)
        gpu_ctx.set_pipeline_color_correction(None)
        gpu_ctx.set_pipeline_smoothing(None)
    want = _stages(gpu_ctx, plain, IMP if imp else None, DF if df else None, then)
    _same(got, want, f"pipe, impulse {imp} defringe {df} then {then}")
    assert not np.array_equal(got[1], plain[1])
    del keep


def test_pipeline_setting_off_is_the_frame_as_before(gpu_ctx, frame):
    raw, p, plain = frame
    off = (capi.impulse_denoise_params(False, 80), capi.defringe_params(False, 2.0, 13))
    for imp, df in ((None, None), off):
        try:
            gpu_ctx.set_pipeline_impulse_defringe(imp, df)
            got = _pipeline(gpu_ctx, raw, p)
        finally:
            gpu_ctx.set_pipeline_impulse_defringe(None, None)
        assert all(np.array_equal(I.bits(a), I.bits(b)) for a, b in zip(got, plain))
    # what defringe refuses fails the frame before any stage runs
    gpu_ctx.set_pipeline_impulse_defringe(None, capi.defringe_params(True, 5.5, 13))
    try:
        d_raw = torch.from_numpy(raw).to("cuda:0")
        d_img = [torch.full((PH - 8, PW - 8), 7.0, dtype=torch.float32, device="cuda:0") for _ in range(3)]
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
            gpu_ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
        gpu_ctx.synchronize()
        assert all(bool((t == 7.0).all()) for t in d_img)
    finally:
        gpu_ctx.set_pipeline_impulse_defringe(None, None)


def test_batch_of_two_frames_on_two_lanes():
    p = _pipe_params()
    raws = [synth.bayer_frame(PW, PH, synth.FILTERS_RGGB, seed=s, noise=1500) for s in (52, 53)]
    ctx = capi.Context(0)
    plain = [_pipeline(ctx, r, p) for r in raws]
    ctx.set_batch_lanes(2)
    ctx.set_pipeline_impulse_defringe(IMP, DF)
    ctx.set_pipeline_color_correction(CC_REGIONS)
    outs = [[np.zeros((PH - 8, PW - 8), np.float32) for _ in range(3)] for _ in raws]
    ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
    ctx.set_pipeline_impulse_defringe(None, None)
    ctx.set_pipeline_color_correction(None)
    for pl, o in zip(plain, outs):
        _same(o, _stages(ctx, pl, IMP, DF, "cc"), "batch lane")
    assert not np.array_equal(outs[0][1], outs[1][1])
    ctx.close()
