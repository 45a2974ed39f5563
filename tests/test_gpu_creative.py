"""GPU: artgpu_creative_gradients, artgpu_soft_light and artgpu_black_and_white (ImProcFunctions::creativeGradients, softLight and
blackAndWhite: iptransform.cc:677-1048, 1390-1408, ipsoftlight.cc:31-82, ipbw.cc:50-365) and their pipe settings against the CPU checker
(tests/cg_lib.py: tests/emul/creative_ref.cc around the oracle's leaves).

Every pixel is compared as a bit pattern; only where input and factor make a NaN (inf x 0) is NaN-ness compared.  The cases and the
branches they take are listed in cg_lib and checked from the checker's counters in tests/test_creative_checker.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from art_amd import capi, synth
import cg_lib
import layout_lib
import lc_lib
from test_gpu_cli import run_cli
from test_gpu_pipeline import _lut, _params

pytestmark = pytest.mark.gpu
SHAPE_IDS = ["%dx%d" % (w, h) for h, w in cg_lib.SHAPES]
FAMS = cg_lib.FAMILIES


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _device(ctx, img, call):
    d = [torch.from_numpy(np.array(a, dtype=np.float32)).to("cuda:0") for a in img]
    call(capi.RGB(*[capi.device_plane(t) for t in d]))
    ctx.synchronize()
    return [t.cpu().numpy() for t in d]


def _cg(ctx, h, w, family, p, what):
    img, want, _ = cg_lib.cg_case(h, w, family, p)
    cp = cg_lib.capi_cg_params(p)
    cg_lib.assert_same(_device(ctx, img, lambda i: ctx.creative_gradients(i, cp)), want, f"{w}x{h} {family} {what}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# creative gradients
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cg_lib.SHAPES, ids=SHAPE_IDS)
def test_gradient_equals_the_checker(gpu_ctx, shape):
    """every degree x feather x strength x centre, the value families taking turns"""
    h, w = shape
    for i, p in enumerate(cg_lib.gradient_configs()):
        _cg(gpu_ctx, h, w, FAMS[i % len(FAMS)], p, f"gradient {p.gradient_degree}/{p.gradient_feather}/{p.gradient_strength}/{p.gradient_center_x},{p.gradient_center_y}")


@pytest.mark.parametrize("shape", cg_lib.SHAPES, ids=SHAPE_IDS)
def test_vignette_equals_the_checker(gpu_ctx, shape):
    """every roundness x feather x strength x centre on landscape, portrait and square frames"""
    h, w = shape
    for i, p in enumerate(cg_lib.pcvignette_configs()):
        _cg(gpu_ctx, h, w, FAMS[(i + 5) % len(FAMS)], p,
            f"vignette {p.pcvignette_strength}/{p.pcvignette_feather}/{p.pcvignette_roundness}/{p.pcvignette_center_x},{p.pcvignette_center_y}")


@pytest.mark.parametrize("family", FAMS)
def test_every_value_family_through_the_three_kernel_forms(gpu_ctx, family):
    """gradient alone, vignette alone (one float multiply each) and both (the channel product rounded twice, in double)"""
    for h, w in ((45, 67), (9, 7), (3, 259)):
        for name, p in (("gradient", cg_lib.gradient_configs()[20]), ("vignette", cg_lib.pcvignette_configs()[13]), ("both", cg_lib.BOTH), ("both, bright", cg_lib.BOTH_BRIGHT)):
            _cg(gpu_ctx, h, w, family, p, name)


def test_both_tools_round_the_channel_product_twice(gpu_ctx):
    """the case the double form exists for: somewhere the twice-rounded product differs from the float product of the float factors' float product"""
    h, w = cg_lib.WINDOW
    img, want, _ = cg_lib.cg_case(h, w, "scaled_frac", cg_lib.BOTH)
    _, _, gf, vf = cg_lib.creative_gradients(img, cg_lib.BOTH, want_factors=True)
    once = [a * (gf * vf) for a in img]
    assert any(not np.array_equal(_bits(o), _bits(wt)) for o, wt in zip(once, want))
    _cg(gpu_ctx, h, w, "scaled_frac", cg_lib.BOTH, "both")


def test_window_of_a_larger_picture_and_crop_at_scale_two(gpu_ctx):
    h, w = cg_lib.WINDOW
    for fam in ("scaled_frac", "inf_plane", "negzero"):
        _cg(gpu_ctx, h, w, fam, cg_lib.GRAD_WINDOW, "offset (13, 7) in 300x200")
        _cg(gpu_ctx, h, w, fam, cg_lib.PCV_CROP, "crop at scale 2")
    _, _, counts = cg_lib.cg_case(h, w, "scaled_frac", cg_lib.PCV_CROP)
    assert counts["v_faded"] > 0 and counts["v_fade_out"] > 0


@pytest.mark.parametrize("layout", list(layout_lib.LAYOUTS))
def test_padded_and_shifted_device_planes(gpu_ctx, layout):
    """131x70 with a row stride larger than the width and a non-zero offset: the three tools in place, nothing outside the window written"""
    h, w = cg_lib.STRIDED
    ul, vl = cg_lib.cast_tables()
    cfg = cg_lib.bw_configs()[0]
    bp, keep = capi.black_and_white_params(cfg[0], cfg[1], cfg[2], cfg[3])
    bpc, keepc = capi.black_and_white_params(cfg[0], cfg[1], cfg[2], cfg[3], cast=(30, 40), ulut=ul, vlut=vl)
    runs = [(cg_lib.cg_case(h, w, "scaled_frac", cg_lib.BOTH), lambda i: gpu_ctx.creative_gradients(i, cg_lib.capi_cg_params(cg_lib.BOTH))),
            (cg_lib.cg_case(h, w, "dark_offset", cg_lib.gradient_configs()[40]), lambda i: gpu_ctx.creative_gradients(i, cg_lib.capi_cg_params(cg_lib.gradient_configs()[40]))),
            (cg_lib.sl_case(h, w, "nan_plane", 50), lambda i: gpu_ctx.soft_light(i, capi.soft_light_params(50))),
            (cg_lib.bw_case(h, w, "scaled_frac", cfg), lambda i: gpu_ctx.black_and_white(i, bp)),
            (cg_lib.bw_case(h, w, "scaled_frac", cfg, cast=True), lambda i: gpu_ctx.black_and_white(i, bpc, cg_lib.oracle_lib.REC2020_WS_D))]
    for k, ((img, want, _), call) in enumerate(runs):
        ar = layout_lib.arena(layout_lib.LAYOUTS[layout], img)
        call(ar.rgb)
        gpu_ctx.synchronize()
        cg_lib.assert_same(layout_lib.check(ar, f"run {k} {layout}"), want, f"{w}x{h} run {k}, layout {layout}")
    del keep, keepc


def test_host_planes_give_the_same_bits(gpu_ctx):
    for h, w in ((1, 1), (5, 3), (45, 67)):
        img, want, _ = cg_lib.cg_case(h, w, "scaled_frac", cg_lib.BOTH)
        host = [np.array(a, dtype=np.float32) for a in img]
        gpu_ctx.creative_gradients(capi.host_rgb(host), cg_lib.capi_cg_params(cg_lib.BOTH))
        cg_lib.assert_same(host, want, f"{w}x{h} gradients (host planes)")
        img, want, _ = cg_lib.sl_case(h, w, "scaled_frac", 50)
        host = [np.array(a, dtype=np.float32) for a in img]
        gpu_ctx.soft_light(capi.host_rgb(host), capi.soft_light_params(50))
        cg_lib.assert_same(host, want, f"{w}x{h} soft light (host planes)")
        cfg = cg_lib.bw_configs()[2]
        img, want, _ = cg_lib.bw_case(h, w, "scaled_frac", cfg)
        host = [np.array(a, dtype=np.float32) for a in img]
        bp, keep = capi.black_and_white_params(*cfg)
        gpu_ctx.black_and_white(capi.host_rgb(host), bp)
        cg_lib.assert_same(host, want, f"{w}x{h} black and white (host planes)")


def test_disabled_tools_and_zero_strengths_leave_the_image_alone(gpu_ctx):
    img = cg_lib.scene(9, 7, "scaled_frac")
    off = [capi.creative_gradients_params(),
           capi.creative_gradients_params(gradient=(30, 25, 0.0, 0, 0), pcvignette=(1e-16, 50, 50, 0, 0))]
    for p in off:
        got = _device(gpu_ctx, img, lambda i: gpu_ctx.creative_gradients(i, p))
        assert all(np.array_equal(_bits(g), _bits(a)) for g, a in zip(got, img))
    for sp in (capi.soft_light_params(50, enabled=False), capi.soft_light_params(0), capi.soft_light_params(-3)):
        got = _device(gpu_ctx, img, lambda i: gpu_ctx.soft_light(i, sp))
        assert all(np.array_equal(_bits(g), _bits(a)) for g, a in zip(got, img))
    bp, _ = capi.black_and_white_params(enabled=False)
    got = _device(gpu_ctx, img, lambda i: gpu_ctx.black_and_white(i, bp))
    assert all(np.array_equal(_bits(g), _bits(a)) for g, a in zip(got, img))


def test_refusals_leave_the_image_alone(gpu_ctx):
    img = cg_lib.scene(9, 7, "scaled_frac")
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in img]
    rgb = capi.RGB(*[capi.device_plane(t) for t in d])
    for p, code in ((capi.creative_gradients_params(pcvignette=(0.6, 50, 101, 0, 0)), -4), (capi.creative_gradients_params(pcvignette=(0.6, 50, -1, 0, 0)), -4),
                    (capi.creative_gradients_params(gradient=(0, 101, 1.0, 0, 0)), -4), (capi.creative_gradients_params(gradient=(float("nan"), 25, 1.0, 0, 0)), -1),
                    (capi.creative_gradients_params(gradient=(0, 25, 1.0, 0, 0), full=(40000, 100)), -4), (capi.creative_gradients_params(gradient=(0, 25, 1.0, 0, 0), scale=0.0), -1),
                    (capi.creative_gradients_params(gradient=(0, 25, 1.0, 0, 0), offset=(-1, 0)), -4)):
        with pytest.raises(capi.ArtGpuError, match=r"^\[%d\]" % code):
            gpu_ctx.creative_gradients(rgb, p)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\].*strength"):
        gpu_ctx.soft_light(rgb, capi.soft_light_params(101))
    ul, vl = cg_lib.cast_tables()
    for kw, code in ((dict(setting=15), -1), (dict(filter=9), -1), (dict(mixer=(201, 0, 0)), -4), (dict(gamma=(0, 101, 0)), -4), (dict(cast=(30, 0)), -1),
                     (dict(cast=(30, 0), ulut=ul), -1)):
        bp, keep = capi.black_and_white_params(**kw)
        with pytest.raises(capi.ArtGpuError, match=r"^\[%d\]" % code):
            gpu_ctx.black_and_white(rgb, bp, cg_lib.oracle_lib.REC2020_WS_D)
    bp, keep = capi.black_and_white_params(cast=(30, 0), ulut=ul, vlut=vl)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
        gpu_ctx.black_and_white(rgb, bp, None)
    gpu_ctx.synchronize()
    assert all(np.array_equal(_bits(t.cpu().numpy()), _bits(a)) for t, a in zip(d, img))


# ---------------------------------------------------------------------------------------------------------------------------------------
# soft light, black-and-white
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strength", cg_lib.STRENGTHS)
def test_soft_light_equals_the_checker(gpu_ctx, strength):
    """every shape x every family and a plane with NaNs: below 0 takes entry 0, above 65535 and NaN stay"""
    for h, w in cg_lib.SHAPES:
        for fam in FAMS + ("nan_plane",):
            img, want, _ = cg_lib.sl_case(h, w, fam, strength)
            got = _device(gpu_ctx, img, lambda i: gpu_ctx.soft_light(i, capi.soft_light_params(strength)))
            cg_lib.assert_same(got, want, f"soft light {strength} {w}x{h} {fam}")
            keep = [~(a <= np.float32(65535.0)) for a in img]
            assert all(np.array_equal(_bits(g[k]), _bits(np.asarray(a)[k])) for g, a, k in zip(got, img, keep)), "values above the table and NaNs keep their bits"


def test_soft_light_lds_and_plain_kernels_agree(gpu_ctx):
    """the LUT-in-LDS shape large frames take and the plain kernel give the same bits (the option switches between them)"""
    h, w = 2050, 2049
    rng = np.random.default_rng(5)
    img = [(rng.random((h, w), dtype=np.float32) * np.float32(80000.0) - np.float32(3000.0)) for _ in range(3)]
    img[1][7, 9] = np.nan
    a = _device(gpu_ctx, img, lambda i: gpu_ctx.soft_light(i, capi.soft_light_params(70)))
    gpu_ctx.set_option("lut_lds", 0)
    try:
        b = _device(gpu_ctx, img, lambda i: gpu_ctx.soft_light(i, capi.soft_light_params(70)))
    finally:
        gpu_ctx.set_option("lut_lds", 1)
    cg_lib.assert_same(a, b, "LDS / plain")
    want, _, _ = cg_lib.soft_light([p[:64] for p in img], 70)
    cg_lib.assert_same([p[:64] for p in a], want, "first 64 rows against the checker")


@pytest.mark.parametrize("shape", cg_lib.SHAPES, ids=SHAPE_IDS)
def test_black_and_white_equals_the_checker(gpu_ctx, shape):
    """every setting and every filter, gamma on and off, the families taking turns; then the colour cast, whose result comes back as RGB"""
    h, w = shape
    ul, vl = cg_lib.cast_tables()
    for i, cfg in enumerate(cg_lib.bw_configs()):
        fam = FAMS[i % len(FAMS)]
        img, want, _ = cg_lib.bw_case(h, w, fam, cfg)
        bp, keep = capi.black_and_white_params(*cfg)
        cg_lib.assert_same(_device(gpu_ctx, img, lambda im: gpu_ctx.black_and_white(im, bp)), want, f"bw {cfg} {w}x{h} {fam}")
    for i, cfg in enumerate(cg_lib.bw_configs()[:4]):
        fam = ("scaled_frac", "dark_offset", "inf_plane", "huge")[i]
        img, want, _ = cg_lib.bw_case(h, w, fam, cfg, cast=True)
        bp, keep = capi.black_and_white_params(*cfg, cast=(30, 40), ulut=ul, vlut=vl)
        got = _device(gpu_ctx, img, lambda im: gpu_ctx.black_and_white(im, bp, cg_lib.oracle_lib.REC2020_WS_D))
        cg_lib.assert_same(got, want, f"bw + cast {cfg} {w}x{h} {fam}")


@pytest.mark.parametrize("family", FAMS)
def test_black_and_white_every_value_family(gpu_ctx, family):
    for h, w in ((45, 67), (9, 7)):
        for cfg in (cg_lib.bw_configs()[0], cg_lib.bw_configs()[11]):
            img, want, _ = cg_lib.bw_case(h, w, family, cfg)
            bp, keep = capi.black_and_white_params(*cfg)
            cg_lib.assert_same(_device(gpu_ctx, img, lambda im: gpu_ctx.black_and_white(im, bp)), want, f"bw {cfg} {w}x{h} {family}")


def test_tables_follow_their_parameters_between_calls(gpu_ctx):
    """the context keeps the tables of the last call: another strength, other gammas and other cast tables must not find stale ones"""
    h, w = 9, 7
    for s in (50, 1, 50, 100):
        img, want, _ = cg_lib.sl_case(h, w, "scaled_frac", s)
        cg_lib.assert_same(_device(gpu_ctx, img, lambda i: gpu_ctx.soft_light(i, capi.soft_light_params(s))), want, f"soft light {s}")
    ul, vl = cg_lib.cast_tables()
    img = cg_lib.scene(h, w, "scaled_frac")
    for gam, tabs in (((20, -35, 60), (ul, vl)), ((20, 10, 60), (vl, ul)), ((0, 0, 0), (ul, vl)), ((20, -35, 60), (ul, vl))):
        want, _ = cg_lib.black_and_white(img, gamma=gam, cast_bottom=30, ulut=tabs[0], vlut=tabs[1])
        bp, keep = capi.black_and_white_params(gamma=gam, cast=(30, 0), ulut=tabs[0], vlut=tabs[1])
        got = _device(gpu_ctx, img, lambda im: gpu_ctx.black_and_white(im, bp, cg_lib.oracle_lib.REC2020_WS_D))
        cg_lib.assert_same(got, want, f"bw gamma {gam}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the per-frame pipe
# ---------------------------------------------------------------------------------------------------------------------------------------
W, H, B = 416, 288, 4
FW, FH = W - 2 * B, H - 2 * B
LUT = _lut()
PIPE_CG = capi.creative_gradients_params(gradient=(30, 40, 1.2, 10, -20), pcvignette=(1.5, 60, 30, -20, 10), offset=(5, 5), full=(17, 17), scale=3.0)   # (the pipe overrides the geometry)


def _pipeline(ctx, raw, p, size=None):
    h, w = raw.shape
    ow, oh = size or (w - 2 * p.border, h - 2 * p.border)
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.full((oh, ow), float("nan"), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    ctx.synchronize()
    return [t.cpu().numpy() for t in d_img]


def _tools(ctx, frame, steps):
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in frame]
    img = capi.RGB(*[capi.device_plane(t) for t in d])
    for s in steps:
        s(img)
    ctx.synchronize()
    return [t.cpu().numpy() for t in d]


def _same(got, want, what):
    assert all(np.isfinite(g).all() for g in got), what
    cg_lib.assert_same(got, want, what)


def _lc(p):
    curve = lc_lib.curve_lut(lc_lib.BOOST_CURVE_POINTS)
    lc_arr, keep = capi.local_contrast_regions([(60.0, curve, None)])
    p.local_contrast_enabled = 1; p.local_contrast_nregions = 1; p.local_contrast_regions = lc_arr
    return curve, keep


def test_pipe_gradients_are_the_first_step_of_stage_3(gpu_ctx):
    """the pipe with the filters on equals the pipe without any STAGE_3 step and without the tone curve, then the stand-alone call (offset 0, the
    frame as the full size, scale 1) -- and with the tone curve on, that call followed by the tone curve"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=101, noise=1500)
    p = _params(LUT, 0)
    p.tone_enabled = 0
    upto = _pipeline(gpu_ctx, raw, p)
    alone = capi.creative_gradients_params(gradient=(30, 40, 1.2, 10, -20), pcvignette=(1.5, 60, 30, -20, 10))
    try:
        gpu_ctx.set_pipeline_creative_gradients(PIPE_CG)
        got_off = _pipeline(gpu_ctx, raw, p)
        p.tone_enabled = 1
        got_on = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_creative_gradients(None)
    _same(got_off, _tools(gpu_ctx, upto, [lambda i: gpu_ctx.creative_gradients(i, alone)]), "pipe, gradients, no tone curve")
    _same(got_on, _tools(gpu_ctx, upto, [lambda i: gpu_ctx.creative_gradients(i, alone), lambda i: gpu_ctx.tone_curve(i, LUT, 1.0, True)]), "pipe, gradients, tone curve")
    assert not np.array_equal(got_off[1], upto[1])


def test_pipe_soft_light_follows_the_tone_curve(gpu_ctx):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=102, noise=1500)
    p = _params(LUT, 0)
    plain = _pipeline(gpu_ctx, raw, p)
    sp = capi.soft_light_params(40)
    try:
        gpu_ctx.set_pipeline_soft_light(sp)
        got = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_soft_light(None)
    _same(got, _tools(gpu_ctx, plain, [lambda i: gpu_ctx.soft_light(i, sp)]), "pipe, soft light")
    assert not np.array_equal(got[1], plain[1])


@pytest.mark.parametrize("cast", [False, True], ids=["plain", "cast"])
def test_pipe_black_and_white_follows_local_contrast(gpu_ctx, cast):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=103, noise=1500)
    p = _params(LUT, 0)
    curve, keep = _lc(p)
    with_lc = _pipeline(gpu_ctx, raw, p)
    ul, vl = cg_lib.cast_tables()
    bp, keep2 = capi.black_and_white_params("Landscape", "Orange", (40, 30, 25), (20, -35, 60), cast=(30, 40) if cast else (0, 0), ulut=ul if cast else None, vlut=vl if cast else None)
    ws = [float(v) for v in p.ws]
    try:
        gpu_ctx.set_pipeline_black_and_white(bp)
        ul[:] = 0                     # the library copied the tables
        got = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_black_and_white(None)
    ul, vl = cg_lib.cast_tables()
    bp, keep2 = capi.black_and_white_params("Landscape", "Orange", (40, 30, 25), (20, -35, 60), cast=(30, 40) if cast else (0, 0), ulut=ul if cast else None, vlut=vl if cast else None)
    _same(got, _tools(gpu_ctx, with_lc, [lambda i: gpu_ctx.black_and_white(i, bp, ws)]), "pipe, local contrast, black and white")
    assert cast == (not np.array_equal(got[0], got[1]))
    del keep


def test_pipe_black_and_white_then_resize_takes_the_rgb_path(gpu_ctx):
    """with the Resize tool as well: the Lab image goes back to RGB for the tool, so the pipe equals the unresized pipe, then artgpu_resize_lanczos in RGB mode"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=104, noise=1500)
    p = _params(LUT, 0)
    curve, keep = _lc(p)
    bp, keep2 = capi.black_and_white_params("Portrait", "Yellow")
    par = capi.resize_params(dataspec=0, scale=0.5)
    imw, imh, scale = capi.resize_scale(par, FW, FH)
    ws, iws = [float(v) for v in p.ws], [float(v) for v in p.iws]
    try:
        gpu_ctx.set_pipeline_black_and_white(bp)
        full = _pipeline(gpu_ctx, raw, p)
        gpu_ctx.set_pipeline_resize(par)
        got = _pipeline(gpu_ctx, raw, p, (imw, imh))
        ul, vl = cg_lib.cast_tables()
        bpc, keep3 = capi.black_and_white_params("Portrait", "Yellow", cast=(30, 40), ulut=ul, vlut=vl)
        gpu_ctx.set_pipeline_black_and_white(bpc)
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\].*YUV"):
            _pipeline(gpu_ctx, raw, p, (imw, imh))
    finally:
        gpu_ctx.set_pipeline_black_and_white(None)
        gpu_ctx.set_pipeline_resize(None)
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in full]
    o = [torch.full((imh, imw), float("nan"), device="cuda:0") for _ in range(3)]
    gpu_ctx.resize_lanczos(capi.RGB(*[capi.device_plane(t) for t in d]), capi.RGB(*[capi.device_plane(t) for t in o]), scale, capi.RESIZE_RGB, ws, iws)
    gpu_ctx.synchronize()
    _same(got, [t.cpu().numpy() for t in o], "pipe, black and white, resize")
    del keep


def test_cleared_setters_give_the_frame_of_a_context_that_never_set_them(gpu_ctx):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=105, noise=1500)
    p = _params(LUT, 0)
    fresh = capi.Context(0)
    try:
        never = _pipeline(fresh, raw, p)
        bp, keep = capi.black_and_white_params()
        fresh.set_pipeline_creative_gradients(PIPE_CG)
        fresh.set_pipeline_soft_light(capi.soft_light_params(40))
        fresh.set_pipeline_black_and_white(bp)
        on = _pipeline(fresh, raw, p)
        assert not np.array_equal(on[1], never[1]) and np.array_equal(on[0], on[2])
        fresh.set_pipeline_creative_gradients(None)
        fresh.set_pipeline_soft_light(None)
        fresh.set_pipeline_black_and_white(None)
        again = _pipeline(fresh, raw, p)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, never))
        # set but disabled is off as well
        fresh.set_pipeline_creative_gradients(capi.creative_gradients_params())
        fresh.set_pipeline_soft_light(capi.soft_light_params(40, enabled=False))
        fresh.set_pipeline_black_and_white(capi.black_and_white_params(enabled=False)[0])
        again = _pipeline(fresh, raw, p)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, never))
    finally:
        fresh.close()


def test_a_refusing_setting_fails_the_frame_before_it_runs(gpu_ctx):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=106, noise=1500)
    p = _params(LUT, 0)
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.full((FH, FW), float("nan"), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    out = capi.RGB(*[capi.device_plane(t) for t in d_img])
    for setter, val in ((gpu_ctx.set_pipeline_soft_light, capi.soft_light_params(101)),
                        (gpu_ctx.set_pipeline_creative_gradients, capi.creative_gradients_params(pcvignette=(0.6, 50, 101, 0, 0))),
                        (gpu_ctx.set_pipeline_black_and_white, capi.black_and_white_params(gamma=(0, 0, 101))[0])):
        try:
            setter(val)
            with pytest.raises(capi.ArtGpuError, match=r"^\[-4\].*pipeline_run"):
                gpu_ctx.pipeline_run(capi.device_plane(d_raw), p, out)
        finally:
            setter(None)
    gpu_ctx.synchronize()
    assert all(torch.isnan(t).all().item() for t in d_img), "a refused frame writes nothing"


def test_batch_lanes_inherit_the_three_settings():
    p = _params(LUT, 0)
    raws = [synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=s, noise=1500) for s in (107, 108, 109)]
    ctx = capi.Context(0)
    try:
        ul, vl = cg_lib.cast_tables()
        bp, keep = capi.black_and_white_params("Landscape", "Orange", (40, 30, 25), (20, -35, 60), cast=(30, 40), ulut=ul, vlut=vl)
        ctx.set_pipeline_creative_gradients(PIPE_CG)
        ctx.set_pipeline_soft_light(capi.soft_light_params(40))
        ctx.set_pipeline_black_and_white(bp)
        one = [_pipeline(ctx, r, p) for r in raws]
        ctx.set_batch_lanes(2)
        outs = [[np.zeros((FH, FW), np.float32) for _ in range(3)] for _ in raws]
        ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
        for wnt, o in zip(one, outs):
            _same(o, wnt, "batch lane")
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# artgpu-cli
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_cli_with_the_four_switches_equals_the_stages_one_by_one(gpu_ctx, tmp_path):
    """artgpu-cli --gradient --vignette --soft-light --bw (ImProcFunctions::process(STAGE_3) in the C++ mirror: creativeGradients first, softLight
    behind the tone curve, blackAndWhite last) equals the same entry points called from here"""
    from test_gpu_cli import MAT, MUL, tone_lut
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=110, noise=1200)
    _, without = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3"])
    _, got = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--gradient", "30,40,1.2,10,-20", "--vignette", "1.5,60,30,-20,10", "--soft-light", "40",
                                               "--bw", "Landscape,Orange,40,30,25,20,-35,60"])
    assert not np.array_equal(got, without)
    h, w = raw.shape
    d_raw = torch.from_numpy(raw).to("cuda:0")
    dem = [torch.empty((h, w), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    planes = capi.RGB(*[capi.device_plane(t) for t in dem])
    gpu_ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), synth.FILTERS_RGGB, 1.0, B, planes)
    d_img = [torch.empty((FH, FW), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    gpu_ctx.get_image(planes, B, B, MUL, True, None, img)
    gpu_ctx.convert_color_space(img, MAT)
    gpu_ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    gpu_ctx.creative_gradients(img, capi.creative_gradients_params(gradient=(30, 40, 1.2, 10, -20), pcvignette=(1.5, 60, 30, -20, 10)))
    gpu_ctx.tone_curve(img, tone_lut(), 1.0, True)
    gpu_ctx.soft_light(img, capi.soft_light_params(40))
    bp, keep = capi.black_and_white_params("Landscape", "Orange", (40, 30, 25), (20, -35, 60))
    gpu_ctx.black_and_white(img, bp)
    gpu_ctx.synchronize()
    want = np.stack([np.rint(np.clip(t.cpu().numpy(), 0, 65535)).astype(np.uint16) for t in d_img], axis=-1)
    assert np.array_equal(got, want)
