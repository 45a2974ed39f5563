"""GPU: every entry point that uses a caller's device planes IN PLACE, on device images whose rows are longer than the image, whose planes
start at different alignments and which have rows of memory above and below them (tests/layout_lib.py).

Host planes are staged into a dense copy, so the kernels see stride == w on an aligned base there; a device-resident PlanarRGBData has a row
stride of ceil16(w * 4) bytes and is used where it lies.  Each case is one call on arena planes followed by three statements, all evaluated
and reported together under their letters:
 (a) the window equals the CPU checker, the function and arguments of the entry's own dense test, in every bit.  A NaN has to be a NaN in
     the same place; which NaN (sign, payload) is the one thing the two machines' arithmetic does not share (cc_lib.bits says the same).
     The NEUTRAL tone curve is compared outside the checker's `oor` map (a powf per pixel above the curve), as its own test does;
 (b) the window equals the same call on host planes in every bit, NaNs included;
 (c) no word outside the window changed: left shift, right padding, guard rows.
Calls with a separate source and destination get the two on different layouts and the source's arena is checked too.  No tolerances, no
skips; shapes are the smallest at which the kernel has all its parts (137 x 91: w % 4 == 1, more than one 256-thread block per row pair)."""
import functools

import numpy as np
import pytest
import torch

import cc_lib
import layout_lib as L
import oracle_lib as O
import sh_lib
import test_gpu_hsl as HSL
import test_gpu_lab as LAB
import test_gpu_logenc as LOG
import test_gpu_nlmeans as NL
import test_gpu_pixelops as PX
import test_gpu_tonecurve as TC
import test_oracle_value_domains as R
import value_domains as VD
from art_amd import capi, synth
from test_gpu_pipeline import _lut, _params

pytestmark = pytest.mark.gpu

NAMES = list(L.LAYOUTS)
layouts = pytest.mark.parametrize("layout", NAMES)
W, H = 137, 91
MUL = (2.1374, 1.0, 1.5918)
MAT = R.MAT
WS, IWS = O.REC2020_WS_D, O.REC2020_IWS_D


def other(layout, step=1):
    """the layout `step` places further along: what the second image of a call lies on"""
    return NAMES[(NAMES.index(layout) + step) % len(NAMES)]


def _ro(planes):
    out = tuple(np.ascontiguousarray(p, dtype=np.float32) for p in planes)
    for p in out:
        p.setflags(write=False)
    return out


def _nan_as_one(a):
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def vs_checker(got, want, what, keep=None):
    """(a): messages, one per plane that differs"""
    msgs = []
    for k, (g, w) in enumerate(zip(got, want)):
        bad = _nan_as_one(g) != _nan_as_one(w)
        if keep is not None:
            bad &= keep
        if bad.any():
            i = tuple(int(v) for v in np.argwhere(bad)[0])
            msgs.append(f"(a) {what} plane {k}: {int(bad.sum())} of {bad.size} values differ from the checker, first at {i}: "
                        f"{int(np.asarray(g).view(np.uint32)[i]):#010x} != {int(np.asarray(w).view(np.uint32)[i]):#010x}")
    return msgs


def vs_host(got, host, what):
    """(b): every bit"""
    return ["(b) " + m for m in (VD.report_mismatch(g, h, f"{what} plane {k} against host planes") for k, (g, h) in enumerate(zip(got, host))) if m]


def outside(*arenas, what=""):
    """(c)"""
    return ["(c) " + m for m in (L.stray(a, what) for a in arenas) if m]


def unchanged(ar, planes, what):
    """a source arena's window still holds what was put there"""
    return ["(c) " + m for m in (VD.report_mismatch(g, p, f"{what}: the source plane {k} changed") for k, (g, p) in enumerate(zip(L.contents(ar), planes))) if m]


def verdict(*lists):
    msgs = [m for l in lists for m in l]
    assert not msgs, "\n".join(msgs)


def inplace_rgb(ctx, layout, img, call, ref, what, keep=None):
    """`call(rgb)` on host copies and on an arena of `img`; the three statements.  ref None: (b) and (c) only."""
    host = [np.array(p, dtype=np.float32) for p in img]
    call(capi.host_rgb(host))
    ar = L.arena(L.LAYOUTS[layout] if isinstance(layout, str) else layout, img)
    call(ar.rgb)
    ctx.synchronize()
    got = L.contents(ar)
    verdict([] if ref is None else vs_checker(got, ref, what, keep), vs_host(got, host, what), outside(ar, what=what))
    return got


def inplace_plane(ctx, layout, img, call, ref, what):
    host = np.array(img, dtype=np.float32)
    call(capi.host_plane(host))
    ar = L.arena(L.LAYOUTS[layout] if isinstance(layout, str) else layout, [img])
    call(ar.plane)
    ctx.synchronize()
    got = L.contents(ar)
    verdict(vs_checker(got, [ref], what), vs_host(got, [host], what), outside(ar, what=what))


# ---- pixel passes -----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene(w=W, h=H, wild=True):
    return _ro(LAB.scene(w, h, w * 3 + h, wild=wild))


def _curve():
    x = np.arange(65536, dtype=np.float64) / 65535.0
    return ((1.0 - np.cos(np.pi * x ** 0.7)) / 2.0).astype(np.float32) * np.float32(65535.0)


ES, BLACK = float(np.float32(2.0) ** np.float32(0.3)), float(np.float32(0.01 * 2000.0))
MIX = np.array([1.1, -0.2, 0.1, -0.05, 1.2, -0.15, 0.02, -0.3, 1.28], np.float32)
_X = np.arange(65536, dtype=np.float64) / 65535.0
LR, LB = (65535.0 * _X ** 0.8).astype(np.float32), (65535.0 * (1.0 - (1.0 - _X) ** 1.3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pixel_ref(name):
    """(checker's planes, mask of the pixels (a) covers or None) of a pixel pass on scene()"""
    img = list(scene())
    if name == "convert_color_space":
        return _ro(O.convert_color_space(img, PX.MAT)), None
    if name == "exposure":
        return _ro(O.exposure(img, ES, BLACK)), None
    if name == "tone_curve":
        return _ro(O.tone_std(img, _curve(), 1.0, True)), None
    if name == "tone_curve_no_lut":
        return _ro(O.tone_std(img, None, 1.0, True)), None
    if name == "tone_curve_neutral":
        ref, oor = O.tone_neutral(img, TC.s_curve(), 1.0, want_oor=True)
        return _ro(ref), ~oor
    if name == "channel_mixer":
        return _ro(O.channel_mixer(img, MIX)), None
    if name == "rgb_curves":
        return _ro(O.rgb_curves(img, (LR, None, LB))), None
    if name == "saturation_35_0":
        return _ro(O.saturation_vibrance(img, 35, 0)), None
    if name == "saturation_-20_-60":
        return _ro(O.saturation_vibrance(img, -20, -60)), None
    raise KeyError(name)


def pixel_call(ctx, name):
    return {
        "convert_color_space": lambda rgb: ctx.convert_color_space(rgb, PX.MAT),
        "exposure": lambda rgb: ctx.exposure(rgb, ES, BLACK),
        "tone_curve": lambda rgb: ctx.tone_curve(rgb, _curve(), 1.0, True),
        "tone_curve_no_lut": lambda rgb: ctx.tone_curve(rgb, None, 1.0, True),
        "tone_curve_neutral": lambda rgb: ctx.tone_curve_neutral(rgb, TC.s_curve(), 1.0, WS, IWS),
        "channel_mixer": lambda rgb: ctx.channel_mixer(rgb, MIX),
        "rgb_curves": lambda rgb: ctx.rgb_curves(rgb, LR, None, LB),
        "saturation_35_0": lambda rgb: ctx.saturation_vibrance(rgb, 35, 0, WS),
        "saturation_-20_-60": lambda rgb: ctx.saturation_vibrance(rgb, -20, -60, WS),
    }[name]


PIXEL_PASSES = ["convert_color_space", "exposure", "tone_curve", "tone_curve_no_lut", "tone_curve_neutral", "channel_mixer", "rgb_curves",
                "saturation_35_0", "saturation_-20_-60"]


@layouts
@pytest.mark.parametrize("name", PIXEL_PASSES)
def test_pixel_pass(gpu_ctx, name, layout):
    ref, keep = pixel_ref(name)
    inplace_rgb(gpu_ctx, layout, scene(), pixel_call(gpu_ctx, name), ref, name, keep)


def two_images(ctx, layout, src, out_shape, call, ref, what, src_layout=None):
    """call(src rgb, dst rgb) with the source on one layout and the destination on another"""
    oh, ow = out_shape
    host = [np.full((oh, ow), np.nan, np.float32) for _ in range(3)]
    hsrc = [np.array(p, dtype=np.float32) for p in src]
    call(capi.host_rgb(hsrc), capi.host_rgb(host))
    a_src = L.arena(L.LAYOUTS[src_layout or other(layout)], src)
    a_dst = L.arena(L.LAYOUTS[layout], (oh, ow))
    call(a_src.rgb, a_dst.rgb)
    ctx.synchronize()
    got = L.contents(a_dst)
    verdict(vs_checker(got, ref, what), vs_host(got, host, what), outside(a_dst, a_src, what=what), unchanged(a_src, src, what))


@layouts
def test_get_image_crop(gpu_ctx, layout):
    ow, oh = W - 6, H - 4
    ref = O.convert_color_space(O.get_image(list(scene()), 3, 2, ow, oh, MUL, True), PX.MAT)
    two_images(gpu_ctx, layout, scene(), (oh, ow), lambda s, d: gpu_ctx.get_image(s, 3, 2, MUL, True, PX.MAT, d), ref, "get_image crop")


@layouts
def test_get_image_skip(gpu_ctx, layout):
    cw, ch, skip = W - 6, H - 4, 2
    ow, oh = (cw + skip - 1) // skip, (ch + skip - 1) // skip
    mul = [m / (skip * skip) for m in MUL]
    ref = O.get_image_skip(list(scene()), 3, 2, ow, oh, skip, mul, True)
    two_images(gpu_ctx, layout, scene(), (oh, ow), lambda s, d: gpu_ctx.get_image(s, 3, 2, mul, True, None, d, skip=skip), ref, "get_image skip 2")


OUT_M = np.array([[1.66, -0.59, -0.07], [-0.12, 1.13, -0.01], [-0.02, -0.10, 1.12]], np.float32)


@layouts
def test_rgb2out_matrix_linear(gpu_ctx, layout):
    ref, bad = O.rgb2out_matrix(list(scene()), OUT_M, True)
    assert bad == 0
    two_images(gpu_ctx, layout, scene(), (H, W), lambda s, d: gpu_ctx.rgb2out_matrix(s, d, OUT_M, True), ref, "rgb2out linear")


@layouts
def test_rgb2out_matrix_trc(gpu_ctx, layout):
    """the TRC table refuses values above 1 (artgpu_rgb2out_matrix's rule), so: the scene without its out-of-range pixels, halved"""
    x = np.arange(1024, dtype=np.float64) / 1023.0
    lut = np.where(x <= 0.0031308, 12.92 * x, 1.055 * x ** (1 / 2.4) - 0.055).astype(np.float32)
    dim = _ro([(p * 0.5).astype(np.float32) for p in scene(wild=False)])
    ref, bad = O.rgb2out_matrix(list(dim), OUT_M, False, lut)
    assert bad == 0
    two_images(gpu_ctx, layout, dim, (H, W), lambda s, d: gpu_ctx.rgb2out_matrix(s, d, OUT_M, False, lut), ref, "rgb2out TRC")


@functools.lru_cache(maxsize=None)
def lab_case(w, h):
    """(rgb, lab, lab with labAdjustments' out-of-curve values, curves, lab adjusted): test_gpu_lab.py's inputs"""
    rgb = scene(w, h)
    lab = _ro(O.image_rgb_to_lab(list(rgb)))
    adj = [p.copy() for p in lab]
    adj[1][1, :3] = [-50.0, 40000.0, 70000.0]
    adj[0][4 % h, :4] = [-50000.0, 50000.0, 1e9, -1e9]
    adj = _ro(adj)
    cv = LAB.curves(w)
    return rgb, lab, adj, cv, _ro(O.lab_adjustments(list(adj), *cv, 1.35))


@layouts
@pytest.mark.parametrize("w,h", [(W, H), (6, 5)])
def test_rgb_to_lab_and_back(gpu_ctx, w, h, layout):
    rgb, lab, _, _, _ = lab_case(w, h)
    inplace_rgb(gpu_ctx, layout, rgb, lambda im: gpu_ctx.rgb_to_lab(im, WS), lab, "rgb_to_lab")
    inplace_rgb(gpu_ctx, layout, lab, lambda im: gpu_ctx.lab_to_rgb(im, IWS), O.image_lab_to_rgb(list(lab), IWS), "lab_to_rgb")


@layouts
@pytest.mark.parametrize("w,h", [(W, H), (6, 5)])
def test_lab_adjustments_and_histogram(gpu_ctx, w, h, layout):
    _, _, adj, cv, ref = lab_case(w, h)
    inplace_rgb(gpu_ctx, layout, adj, lambda im: gpu_ctx.lab_adjustments(im, *cv, 1.35), ref, "lab_adjustments")
    ar = L.arena(L.LAYOUTS[layout], adj)
    hist = gpu_ctx.lab_histogram(ar.rgb)
    gpu_ctx.synchronize()
    keep = [np.array(p) for p in adj]
    host_hist = gpu_ctx.lab_histogram(capi.host_rgb(keep))
    want = O.lab_histogram(adj[1])
    assert np.array_equal(hist, want) and np.array_equal(hist, host_hist) and int(hist.sum()) == w * h
    verdict(outside(ar, what="lab_histogram"), unchanged(ar, adj, "lab_histogram"))


@functools.lru_cache(maxsize=None)
def logenc_case(reg):
    img = _ro(LOG.scene(W, H, W + H))
    return img, _ro(O.log_encoding(list(img), regularization=reg))


@layouts
@pytest.mark.parametrize("reg", [0, 60])
def test_log_encoding(gpu_ctx, reg, layout):
    img, ref = logenc_case(reg)
    inplace_rgb(gpu_ctx, layout, img, lambda im: gpu_ctx.log_encoding(im, WS, regularization=reg), ref, f"log_encoding regularization {reg}")


@functools.lru_cache(maxsize=None)
def hsl_case(smoothing):
    img = _ro(HSL.scene(420, 300, 420))
    return img, _ro(O.hsl_equalizer(list(img), HSL.H_CURVE, HSL.S_CURVE, HSL.L_CURVE, smoothing, scale=1.0, to_rgb=True))


@layouts
@pytest.mark.parametrize("smoothing", [0, 5])
def test_hsl_equalizer(gpu_ctx, smoothing, layout):
    img, ref = hsl_case(smoothing)
    inplace_rgb(gpu_ctx, layout, img, lambda im: gpu_ctx.hsl_equalizer(im, HSL.H_CURVE, HSL.S_CURVE, HSL.L_CURVE, smoothing, WS, 1.0, True), ref,
                f"hsl_equalizer smoothing {smoothing}")


# ---- the kernels that keep a table in LDS: only reached from 2^22 pixels -------------------------------------------------------------------------

BW, BH = 2049, 2048


def _with_plain(ctx, run):
    """run() as it is and with option lut_lds 0, the option put back whatever happens"""
    lds = run()
    ctx.set_option("lut_lds", 0)
    try:
        plain = run()
    finally:
        ctx.set_option("lut_lds", 1)
    return lds, plain


def _large(ctx, img, call, ref, what, keep=None):
    def run():
        ar = L.arena(L.LAYOUTS["odd"], img)
        call(ar.rgb)
        ctx.synchronize()
        return ar
    lds, plain = _with_plain(ctx, run)
    got = L.contents(lds)
    verdict([] if ref is None else vs_checker(got, ref, what, keep), vs_host(got, L.contents(plain), what + " (lut_lds 1 against 0)"),
            outside(lds, plain, what=what))


def test_tone_std_lds_curve(gpu_ctx):
    img = scene(BW, BH)
    _large(gpu_ctx, img, lambda im: gpu_ctx.tone_curve(im, _curve(), 1.0, True), O.tone_std(list(img), _curve(), 1.0, True), "tone_std_lds")


def test_tone_neutral_lds_table(gpu_ctx):
    img = scene(BW, BH)
    ref, oor = O.tone_neutral(list(img), TC.s_curve(), 1.0, want_oor=True)
    _large(gpu_ctx, img, lambda im: gpu_ctx.tone_curve_neutral(im, TC.s_curve(), 1.0, WS, IWS), ref, "tone_neutral LDS", ~oor)


def test_denoise_yuv_lds_tables(gpu_ctx):
    """the two *_lds YUV passes of the denoiser (wide-range data of test_large_frame_lds_gamma_tables_same_bits_as_plain_kernels)"""
    rng = np.random.default_rng(12)
    base = rng.uniform(0, 1, (BH, BW)).astype(np.float32) ** 3 * 9000.0
    img = [(base * rng.uniform(0.5, 1.5, (BH, BW))).astype(np.float32) for _ in range(3)]
    img[0][:4, :64] = 0.0
    img[1][4:8, :64] = -5.0
    img[2][8:12, :64] = 66000.0
    tp = capi.DenoiseToolParams(capi.DenoiseParams(30.0, 50.0, 0, 12.0, 0.0, 0.0, 1.7, 0, 0, 0), 0, 3, 0, 80)
    ref = O.improc_denoise(img, dict(luminance=30.0, chrominance=12.0), smoothing=False, ecomp=0.3, detail_recovery=False)
    _large(gpu_ctx, img, lambda im: gpu_ctx.improc_denoise(im, tp, WS, ecomp=0.3, flags=capi.DN_SKIP_DETAIL_RECOVERY), ref, "denoise LDS tables")


# ---- denoise ----------------------------------------------------------------------------------------------------------------------------------

FAMILY = "scaled_frac"          # fractions, a few negatives, values up to ~89 000 (tests/value_domains.py)
DN = capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0)


@layouts
@pytest.mark.parametrize("w,h,crop_h", [(R.W, R.H, None), (R.W, R.H, 120), (R.CA_W, R.CA_H, None)], ids=["262x198", "262x120", "700x500"])
def test_rgb_denoise(gpu_ctx, w, h, crop_h, layout):
    """the sizes of DN_SIZES in test_gpu_value_domains.py: the fused shrink pass and, below its threshold, the three-kernel form"""
    img = R.dn_input(FAMILY, w, h, crop_h)
    inplace_rgb(gpu_ctx, layout, img, lambda im: gpu_ctx.rgb_denoise(im, DN, O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY),
                R.o_rgb_denoise(FAMILY, w, h, crop_h), f"rgb_denoise {w}x{crop_h or h}")


TOOL = capi.DenoiseToolParams(capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0), 1, 3, 50, 80)
DEM_W, DEM_H = R.W + 8, R.H + 8


@functools.lru_cache(maxsize=None)
def tool_case():
    """test_fuzz_config4_chain's frame ahead of the tool at 262 x 198 -> (demosaiced planes, image, image denoised, ... and exposed)"""
    raw = synth.bayer_frame(DEM_W, DEM_H, synth.FILTERS_GRBG, seed=100, noise=1500)
    dem = _ro(O.amaze(raw, synth.FILTERS_GRBG, 1.0, 4))
    img = _ro(O.convert_color_space(O.get_image(list(dem), 4, 4, R.W, R.H, MUL, True), MAT))
    curve, _ = capi.noise_curve_lut()
    den = _ro(O.improc_denoise(list(img), calclum_mat=MAT, noise_c_curve=curve, smoothing=True, radius=3, nl_strength=50, nl_detail=80, ecomp=0.3,
                               detail_recovery=False))
    return dem, img, den, _ro(O.exposure(list(den), ES, 12.5))


@layouts
def test_improc_denoise(gpu_ctx, layout):
    _, img, den, _ = tool_case()
    curve, _ = capi.noise_curve_lut()
    inplace_rgb(gpu_ctx, layout, img, lambda im: gpu_ctx.improc_denoise(im, TOOL, WS, ecomp=0.3, calclum_mat=MAT, noise_c_curve=curve,
                                                                        flags=capi.DN_SKIP_DETAIL_RECOVERY), den, "improc_denoise")


@pytest.mark.parametrize("dem_layout,img_layout", [("planar16", "odd"), ("mixed", "even_off"), ("odd", "planar16")])
def test_improc_denoise_fused(gpu_ctx, dem_layout, img_layout):
    """two strides in one kernel: the demosaiced planes' and the image's"""
    dem, _, _, ref = tool_case()
    curve, _ = capi.noise_curve_lut()

    def call(s, d):
        gpu_ctx.improc_denoise_fused(d, TOOL, WS, demosaiced=s, sx1=4, sy1=4, mul=MUL, do_clip=True, cam_to_work=MAT, exposure=(ES, 12.5), ecomp=0.3,
                                     calclum_mat=MAT, noise_c_curve=curve, flags=capi.DN_SKIP_DETAIL_RECOVERY)
    two_images(gpu_ctx, img_layout, dem, (R.H, R.W), call, ref, f"improc_denoise_fused {dem_layout} -> {img_layout}", src_layout=dem_layout)


@layouts
def test_denoise_chroma_map(gpu_ctx, layout):
    w, h = 333, 251
    rng = np.random.default_rng(5)
    img = [rng.uniform(-200.0, 70000.0, (h, w)).astype(np.float32) for _ in range(3)]
    img[0][:40] *= 3.0
    img[2][60:90] = 0.0
    curve, _ = capi.noise_curve_lut()
    ref = O.chroma_noise_map(img, MAT, WS, curve)
    host = np.zeros_like(ref)
    gpu_ctx.denoise_chroma_map(capi.host_rgb(img), MAT, WS, curve, capi.host_plane(host))
    a_img = L.arena(L.LAYOUTS[other(layout)], img)
    a_map = L.arena(L.LAYOUTS[layout], [np.zeros_like(ref)])
    gpu_ctx.denoise_chroma_map(a_img.rgb, MAT, WS, curve, a_map.plane)
    gpu_ctx.synchronize()
    got = L.contents(a_map)
    verdict(vs_checker(got, [ref], "chroma map"), vs_host(got, [host], "chroma map"), outside(a_map, a_img, what="chroma map"), unchanged(a_img, img, "chroma map"))


@functools.lru_cache(maxsize=None)
def guided_case(w, h):
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=w, noise=2048)
    img = _ro(O.amaze(raw, synth.FILTERS_RGGB, 1.0, 4))
    return img, _ro(O.guided_smoothing(list(img), WS, 3, 1.0))


@layouts
@pytest.mark.parametrize("w,h", [(480, 360), (720, 640)])
def test_denoise_guided_smoothing(gpu_ctx, w, h, layout):
    img, ref = guided_case(w, h)
    inplace_rgb(gpu_ctx, layout, img, lambda im: gpu_ctx.denoise_guided_smoothing(im, WS, 3, 1.0), ref, f"guided smoothing {w}x{h}")


@layouts
def test_denoise_compute_params(gpu_ctx, layout):
    """numbers only: what the call estimates from padded device planes is what it estimates from host planes"""
    pl = [np.array(p) for p in R.dn_input(FAMILY)]
    stores = []
    ar = L.arena(L.LAYOUTS[layout], pl)
    for rgb in (capi.host_rgb(pl), ar.rgb):
        dn = capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 1)
        st = gpu_ctx.denoise_compute_params(rgb, 4, R.DN_MUL, True, MAT, WS, dn)
        stores.append((bytes(st), bytes(dn)))
    gpu_ctx.synchronize()
    assert stores[0][0] == stores[1][0] and stores[0][1] == stores[1][1]
    store, info = R.o_dninfo(FAMILY)
    assert np.array_equal(np.array([list(st.crop_info[k]) for k in range(9)], np.float32)[:, :11].view(np.uint32), np.ascontiguousarray(info[:, :11]).view(np.uint32))
    verdict(outside(ar, what="denoise_compute_params"), unchanged(ar, pl, "denoise_compute_params"))


@layouts
def test_rgb_denoise_with_detail_recovery(gpu_ctx, layout):
    """(b) and (c) only: the DCT stage's distance from the checker is a tolerance test_gpu_value_domains.py owns.  The host call is run twice
    first and has to give the same bits, or (b) would say nothing."""
    img = R.dn_input(FAMILY, 300, 275)
    p = capi.DenoiseParams(40.0, 80.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0)
    runs = []
    for _ in range(2):
        h = [np.array(x) for x in img]
        gpu_ctx.rgb_denoise(capi.host_rgb(h), p, O.REC2020_WS, flags=0)
        runs.append(h)
    verdict([m for m in (VD.report_mismatch(a, b, f"detail recovery on host planes, second run, plane {k}") for k, (a, b) in enumerate(zip(*runs))) if m])
    inplace_rgb(gpu_ctx, layout, img, lambda im: gpu_ctx.rgb_denoise(im, p, O.REC2020_WS, flags=0), None, "rgb_denoise with detail recovery")


# ---- planes -------------------------------------------------------------------------------------------------------------------------------------

def _wavelet_src():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_golden_inputs import wavelet_input
    return wavelet_input(129, 97, 129 + 97)


@layouts
def test_wavelet_decompose_from_a_padded_source(gpu_ctx, layout):
    src = _wavelet_src()
    d = O.wavelet_decompose(src, 5)
    bands, c0, _ = O.wavelet_bands(d)
    O.lib().oracle_wavelet_free(d)
    ar = L.arena(L.LAYOUTS[layout], [src])
    wv = gpu_ctx.wavelet_decompose(ar.plane, 5)
    try:
        got = [gpu_ctx.wavelet_get_band(wv, l, k + 1) for l in range(5) for k in range(3)] + [gpu_ctx.wavelet_get_band(wv, 0, 0)]
    finally:
        gpu_ctx.wavelet_free(wv)
    want = [bands[l, k] for l in range(5) for k in range(3)] + [c0]
    hv = gpu_ctx.wavelet_decompose(capi.host_plane(src), 5)
    try:
        host = [gpu_ctx.wavelet_get_band(hv, l, k + 1) for l in range(5) for k in range(3)] + [gpu_ctx.wavelet_get_band(hv, 0, 0)]
    finally:
        gpu_ctx.wavelet_free(hv)
    verdict(vs_checker(got, want, "wavelet band"), vs_host(got, host, "wavelet band"), outside(ar, what="wavelet_decompose"), unchanged(ar, [src], "wavelet_decompose"))


@layouts
@pytest.mark.parametrize("blend", [1.0, 0.5])
def test_wavelet_reconstruct_into_a_padded_destination(gpu_ctx, blend, layout):
    """the destination holds a ramp: with blend != 1 the kernel reads it"""
    src = _wavelet_src()
    h, w = src.shape
    ramp = (np.arange(h * w, dtype=np.float32).reshape(h, w) * np.float32(0.37) - np.float32(900.0))
    ref = O.wavelet_reconstruct(O.wavelet_decompose(src, 5), h, w, blend, ramp)
    ar = L.arena(L.LAYOUTS[layout], [ramp])
    host = ramp.copy()
    for dst in (capi.host_plane(host), ar.plane):
        wv = gpu_ctx.wavelet_decompose(capi.host_plane(src), 5)
        try:
            gpu_ctx.wavelet_reconstruct(wv, dst, blend)
            gpu_ctx.synchronize()
        finally:
            gpu_ctx.wavelet_free(wv)
    got = L.contents(ar)
    if blend != 1.0:
        assert not np.array_equal(ref, O.wavelet_reconstruct(O.wavelet_decompose(src, 5), h, w, blend, 7.0))
    verdict(vs_checker(got, [ref], f"wavelet_reconstruct blend {blend}"), vs_host(got, [host], "wavelet_reconstruct"), outside(ar, what="wavelet_reconstruct"))


@functools.lru_cache(maxsize=None)
def gf_case(w, h, r):
    rng = np.random.default_rng(w + r)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    guide = (0.4 + 0.3 * np.sin(0.02 * x) * np.cos(0.017 * y) + 0.15 * ((x.astype(np.int32) // 40 + y.astype(np.int32) // 40) % 2)).astype(np.float32)
    src = (guide * 0.8 + rng.normal(0, 0.05, (h, w))).astype(np.float32)
    return _ro([guide, src, O.guided_filter(guide, src, r, 0.001)])


@layouts
@pytest.mark.parametrize("w,h,r", [(300, 200, 3), (700, 500, 4)])
def test_guided_filter(gpu_ctx, w, h, r, layout):
    guide, src, ref = gf_case(w, h, r)
    host = np.zeros_like(src)
    gpu_ctx.guided_filter(capi.host_plane(guide), capi.host_plane(src), capi.host_plane(host), r, 0.001)
    a_g, a_s, a_d = L.arena(L.LAYOUTS[layout], [guide]), L.arena(L.LAYOUTS[other(layout)], [src]), L.arena(L.LAYOUTS[other(layout, 2)], [np.zeros_like(src)])
    gpu_ctx.guided_filter(a_g.plane, a_s.plane, a_d.plane, r, 0.001)
    gpu_ctx.synchronize()
    got = L.contents(a_d)
    out_of_place = [vs_checker(got, [ref], "guided_filter"), vs_host(got, [host], "guided_filter"), outside(a_g, a_s, a_d, what="guided_filter"),
                    unchanged(a_g, [guide], "guided_filter guide"), unchanged(a_s, [src], "guided_filter")]
    gpu_ctx.guided_filter(a_g.plane, a_s.plane, a_s.plane, r, 0.001)           # in place on the source, as hslEqualizer calls it
    gpu_ctx.synchronize()
    got = L.contents(a_s)
    verdict(*out_of_place, vs_checker(got, [ref], "guided_filter in place"), vs_host(got, [host], "guided_filter in place"),
            outside(a_g, a_s, what="guided_filter in place"), unchanged(a_g, [guide], "guided_filter in place, guide"))


@functools.lru_cache(maxsize=None)
def y_plane(w, h, seed):
    p = NL._Y(w, h, seed)
    p.setflags(write=False)
    return p


@layouts
@pytest.mark.parametrize("sigma", [0.7, 3.3])
def test_gaussian_blur(gpu_ctx, sigma, layout):
    img = y_plane(W, H, W)
    inplace_plane(gpu_ctx, layout, img, lambda pl: gpu_ctx.gaussian_blur(pl, sigma), O.gaussian_blur(img, sigma), f"gaussian_blur sigma {sigma}")


@layouts
@pytest.mark.parametrize("sigma", [0.75, 1.6])
def test_gaussian_blur_ex_division_form(gpu_ctx, sigma, layout):
    """gaussianBlur(src, dst, .., GAUSS_DIV, div): three planes on three layouts; the checker is tests/sh_lib.py's (pinned to the compiled
    reference's recordings by test_gpu_sharpen.py)"""
    src = y_plane(W, H, W)
    div = (np.abs(y_plane(W, H, W + 1)) + np.float32(50.0)).astype(np.float32)
    ref = sh_lib.gauss(src, None, div, sigma, capi.GAUSS_DIV)[0]
    host = np.full((H, W), np.nan, np.float32)
    hs, hd = np.array(src), np.array(div)
    gpu_ctx.gaussian_blur_ex(capi.host_plane(hs), capi.host_plane(host), capi.host_plane(hd), sigma, capi.GAUSS_DIV)
    a_s, a_v, a_d = L.arena(L.LAYOUTS[layout], [src]), L.arena(L.LAYOUTS[other(layout)], [div]), L.arena(L.LAYOUTS[other(layout, 2)], [np.zeros((H, W), np.float32)])
    gpu_ctx.gaussian_blur_ex(a_s.plane, a_d.plane, a_v.plane, sigma, capi.GAUSS_DIV)
    gpu_ctx.synchronize()
    got = L.contents(a_d)
    verdict(vs_checker(got, [ref], "gaussian_blur_ex DIV"), vs_host(got, [host], "gaussian_blur_ex DIV"), outside(a_s, a_v, a_d, what="gaussian_blur_ex"),
            unchanged(a_s, [src], "gaussian_blur_ex"), unchanged(a_v, [div], "gaussian_blur_ex divisor"))


@layouts
def test_detail_mask(gpu_ctx, layout):
    img = y_plane(320, 240, 321)
    ref = O.detail_mask(img, 65535.0, np.float32(1e-3) * np.float32(65535.0), 65535.0, 0.8, 2.0)
    host, himg = np.empty_like(ref), np.array(img)
    gpu_ctx.detail_mask(capi.host_plane(himg), capi.host_plane(host), 65535.0, 65.535, 65535.0, 0.8, 2.0)
    a_s, a_m = L.arena(L.LAYOUTS[other(layout)], [img]), L.arena(L.LAYOUTS[layout], [np.zeros_like(ref)])
    gpu_ctx.detail_mask(a_s.plane, a_m.plane, 65535.0, 65.535, 65535.0, 0.8, 2.0)
    gpu_ctx.synchronize()
    got = L.contents(a_m)
    verdict(vs_checker(got, [ref], "detail_mask"), vs_host(got, [host], "detail_mask"), outside(a_s, a_m, what="detail_mask"), unchanged(a_s, [img], "detail_mask"))


@layouts
@pytest.mark.parametrize("patch,ambient,clip", [(13, (0.45, 0.5, 0.55), True), (5, None, False), (3, (0.45, -0.25, 0.55), False)])
def test_dehaze_dark_channel(gpu_ctx, patch, ambient, clip, layout):
    """test_gpu_dehaze.py's scene at 131 x 67: partial patches at both edges; positive ambient (one division per patch), none, one negative
    component (a division per pixel)"""
    import dh_lib
    w, h = 131, 67
    rng = np.random.default_rng(w)
    planes = [(a / np.float32(65535.0) - np.float32(0.1) + rng.uniform(-0.02, 0.02, a.shape).astype(np.float32))
              for a in dh_lib.hazy_scene(w, h, seed=w, bright_block=True)]
    ref, _ = dh_lib.dark_channel(*planes, patch, ambient, clip)
    host = np.full((h, w), np.nan, np.float32)
    gpu_ctx.dehaze_dark_channel(capi.host_rgb(planes), patch, ambient, clip, capi.host_plane(host))
    a_src, a_dst = L.arena(L.LAYOUTS[other(layout)], planes), L.arena(L.LAYOUTS[layout], [np.zeros((h, w), np.float32)])
    gpu_ctx.dehaze_dark_channel(a_src.rgb, patch, ambient, clip, a_dst.plane)
    gpu_ctx.synchronize()
    got = L.contents(a_dst)
    verdict(vs_checker(got, [ref], "dark channel"), vs_host(got, [host], "dark channel"), outside(a_src, a_dst, what="dark channel"),
            unchanged(a_src, planes, "dark channel"))


@functools.lru_cache(maxsize=None)
def nlm_case():
    img = y_plane(260, 406, 262)
    return img, O.nlmeans(img, 50, 80, 1.0)


@pytest.mark.parametrize("layout", ["dense"] + NAMES)
def test_nlmeans(gpu_ctx, layout):
    """260 x 406 leaves a sliver tile (test_gpu_fuzz.py).  A dense device plane runs in place; a padded one is copied to the pool and back.
    (planar16 is dense at this width: 260 % 4 == 0.)"""
    img, ref = nlm_case()
    inplace_plane(gpu_ctx, L.DENSE if layout == "dense" else layout, img, lambda pl: gpu_ctx.nlmeans(pl, 50, 80, 1.0), ref, f"nlmeans on {layout}")


# ---- raw side -----------------------------------------------------------------------------------------------------------------------------------

RW, RH, RFILT = 330, 270, synth.FILTERS_RGGB


@functools.lru_cache(maxsize=None)
def raw_frame(w=RW):
    f = synth.bayer_frame(w, RH, RFILT, seed=11)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def demosaic_ref(method, w=RW):
    raw = raw_frame(w)
    if method == "amaze":
        return _ro(O.amaze(raw, RFILT, 1.0, 4))
    if method == "rcd":
        return _ro(O.rcd(raw, RFILT))
    if method == "vng4":
        return _ro(O.vng4(raw, RFILT))
    if method == "dual":
        return _ro(O.dual_demosaic_blend(raw, list(demosaic_ref("amaze")), RFILT, 20.0, False)[0])
    raise KeyError(method)


def raw_to_rgb(ctx, layout, raw, call, ref, what, keep=None, prefill=None):
    """call(raw plane, out rgb): raw on one layout, the three outputs on another"""
    h, w = raw.shape
    host = [np.full((h, w), np.nan, np.float32) if prefill is None else prefill.copy() for _ in range(3)]
    hraw = np.array(raw)                     # host_plane borrows the array: it has to outlive the call
    call(capi.host_plane(hraw), capi.host_rgb(host))
    a_raw = L.arena(L.LAYOUTS[other(layout)], [raw])
    a_out = L.arena(L.LAYOUTS[layout], (h, w) if prefill is None else [prefill] * 3)
    call(a_raw.plane, a_out.rgb)
    ctx.synchronize()
    got = L.contents(a_out)
    verdict(vs_checker(got, ref, what, keep), vs_host(got, host, what), outside(a_out, a_raw, what=what), unchanged(a_raw, [raw], what))


@pytest.fixture
def rcd_rows(gpu_ctx):
    yield lambda rows: gpu_ctx.set_option("rcd_rows", rows)
    gpu_ctx.set_option("rcd_rows", 8)


@layouts
@pytest.mark.parametrize("method", ["amaze", "vng4"])
def test_demosaic_bayer(gpu_ctx, method, layout):
    m = {"amaze": capi.BAYER_AMAZE, "vng4": capi.BAYER_VNG4}[method]
    raw_to_rgb(gpu_ctx, layout, raw_frame(), lambda r, o: gpu_ctx.demosaic_bayer(m, r, RFILT, 1.0, 4, o), demosaic_ref(method), method)


@layouts
@pytest.mark.parametrize("w", [RW, RW + 1])
@pytest.mark.parametrize("rows", [4, 8])
def test_demosaic_rcd(gpu_ctx, rcd_rows, rows, w, layout):
    """RCD stores column pairs as one 64-bit word when the stride is even and all three outputs start on 8 bytes.  At 330 the strides of `odd`
    and `mixed` are odd; at 331 `mixed` has an even stride (340) and planes that disagree: r and b start on 8 bytes, g does not."""
    rcd_rows(rows)
    raw_to_rgb(gpu_ctx, layout, raw_frame(w), lambda r, o: gpu_ctx.demosaic_bayer(capi.BAYER_RCD, r, RFILT, 1.0, 4, o), demosaic_ref("rcd", w),
               f"rcd {w} wide, rows {rows}")


@layouts
def test_dual_demosaic(gpu_ctx, layout):
    raw_to_rgb(gpu_ctx, layout, raw_frame(), lambda r, o: gpu_ctx.dual_demosaic_bayer(capi.BAYER_AMAZE, r, RFILT, 1.0, 4, 20.0, False, o), demosaic_ref("dual"),
               "dual demosaic")


@layouts
def test_border_interpolate2(gpu_ctx, layout):
    """writes a frame of three pixels and nothing else: the planes are pre-filled, the frame is the one AMaZE with border 0 leaves
    (amaze_demosaic_RT.cc ends in border_interpolate2(.., 3, ..)), the inside keeps the fill"""
    raw = raw_frame()
    fill = np.full((RH, RW), np.float32(-3.0))
    frame = np.ones((RH, RW), bool)
    frame[3:-3, 3:-3] = False
    ref = [np.where(frame, p, fill) for p in O.amaze(raw, RFILT, 1.0, 0)]
    raw_to_rgb(gpu_ctx, layout, raw, lambda r, o: gpu_ctx.border_interpolate2(r, RFILT, 3, o), ref, "border_interpolate2", prefill=fill)


@functools.lru_cache(maxsize=None)
def xtrans_case(passes, lab):
    raw = synth.xtrans_frame(330, 250, seed=7, noise=1500)
    raw.setflags(write=False)
    return raw, _ro(O.xtrans_demosaic(raw, synth.XTRANS_FUJI, synth.XTRANS_RGB_CAM, passes, lab))


@layouts
@pytest.mark.parametrize("passes,lab", [(1, False), (3, True)])
def test_demosaic_xtrans(gpu_ctx, passes, lab, layout):
    raw, ref = xtrans_case(passes, lab)
    raw_to_rgb(gpu_ctx, layout, raw, lambda r, o: gpu_ctx.demosaic_xtrans(passes, lab, r, synth.XTRANS_FUJI, synth.XTRANS_RGB_CAM, o), ref, f"xtrans {passes} passes")


@layouts
def test_raw_ca_correct(gpu_ctx, layout):
    raw = R.frame(FAMILY, R.CA_W, R.CA_H)
    want, wfit, _ = R.o_ca(FAMILY, "auto2", True)
    p = capi.CaParams(1, 2, 0.0, 0.0, 1)
    host = np.array(raw)
    hfit = gpu_ctx.raw_ca_correct(capi.host_plane(host), R.FILT, p, want_fit=True)
    ar = L.arena(L.LAYOUTS[layout], [raw])
    fit = gpu_ctx.raw_ca_correct(ar.plane, R.FILT, p, want_fit=True)
    gpu_ctx.synchronize()
    got = L.contents(ar)
    assert np.array_equal(fit.reshape(-1).view(np.uint64), wfit.reshape(-1).view(np.uint64)) and np.array_equal(fit.view(np.uint64), hfit.view(np.uint64))
    verdict(vs_checker(got, [want], "raw_ca_correct"), vs_host(got, [host], "raw_ca_correct"), outside(ar, what="raw_ca_correct"))


# ---- frames -------------------------------------------------------------------------------------------------------------------------------------

FW, FH = 400, 300


def _frame_raw(xtrans, seed=2):
    return synth.xtrans_frame(FW, FH, seed=seed, noise=2048) if xtrans else synth.bayer_frame(FW, FH, synth.FILTERS_RGGB, seed=seed, noise=2048)


def _pipe_on(ctx, layout, raw, p):
    """pipeline_run with raw and out on `layout` -> (window, messages of (c))"""
    b = p.border
    h, w = raw.shape
    a_raw = L.arena(L.LAYOUTS[layout], [raw])
    a_out = L.arena(L.LAYOUTS[layout], (h - 2 * b, w - 2 * b))
    ctx.pipeline_run(a_raw.plane, p, a_out.rgb)
    ctx.synchronize()
    return L.contents(a_out), outside(a_raw, a_out, what="pipeline_run") + unchanged(a_raw, [raw], "pipeline_run")


def _pipe_host(ctx, raw, p):
    b = p.border
    h, w = raw.shape
    out = [np.zeros((h - 2 * b, w - 2 * b), np.float32) for _ in range(3)]
    ctx.pipeline_run(capi.host_plane(raw), p, capi.host_rgb(out))
    return out


@pytest.mark.parametrize("tone_mode,xtrans", [(0, False), (1, True)], ids=["bayer_std", "xtrans_neutral"])
def test_pipeline_run_on_padded_planes(gpu_ctx, tone_mode, xtrans):
    """against the same call on host planes and against the stage-by-stage chain of test_pipeline_run_equals_stage_by_stage (the tools' own
    entry points on dense device planes)"""
    raw = _frame_raw(xtrans)
    b = 7 if xtrans else 4
    lut = _lut()
    p = _params(lut, tone_mode, xtrans)
    got, c = _pipe_on(gpu_ctx, "mixed", raw, p)
    host = _pipe_host(gpu_ctx, raw, p)
    d_raw = torch.from_numpy(raw).cuda()
    d_dem = [torch.empty((FH, FW), dtype=torch.float32, device="cuda") for _ in range(3)]
    dem = capi.RGB(*[capi.device_plane(t) for t in d_dem])
    if xtrans:
        gpu_ctx.demosaic_xtrans(3, True, capi.device_plane(d_raw), synth.XTRANS_FUJI, synth.XTRANS_RGB_CAM, dem)
    else:
        gpu_ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), synth.FILTERS_RGGB, 1.0, 4, dem)
    d_img = [torch.empty((FH - 2 * b, FW - 2 * b), dtype=torch.float32, device="cuda") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    gpu_ctx.get_image(dem, b, b, MUL, True, MAT, img)
    curve, _ = capi.noise_curve_lut()
    gpu_ctx.improc_denoise(img, p.denoise, WS, ecomp=0.3, calclum_mat=MAT, noise_c_curve=curve, iws=IWS)
    gpu_ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    if tone_mode == 1:
        gpu_ctx.tone_curve_neutral(img, lut, 1.0, WS, IWS)
    else:
        gpu_ctx.tone_curve(img, lut, 1.0, True)
    gpu_ctx.synchronize()
    stages = [t.cpu().numpy() for t in d_img]
    verdict(["(a) " + m for m in (VD.report_mismatch(g, s, f"pipeline_run plane {k} against the stages") for k, (g, s) in enumerate(zip(got, stages))) if m],
            vs_host(got, host, "pipeline_run"), c)


def test_pipeline_all_tools_on_padded_planes(gpu_ctx):
    """the frame of test_pipeline_all_tools_equal_the_tools_one_by_one on layout `odd`, against its run on host planes"""
    import lc_lib
    import sm_lib
    import tb_lib
    import test_gpu_colorcorrection as CC
    import test_gpu_masks as MK
    import test_gpu_smoothing as SM
    Wf, Hf = 392, 296
    w, h = Wf - 8, Hf - 8
    raw = synth.bayer_frame(Wf, Hf, synth.FILTERS_RGGB, seed=71, noise=1500)
    lut = _lut()
    p = _params(lut, 0)
    p.denoise_enabled = 0
    dh, keep_dh = capi.dehaze_params(depth=50)
    sp = capi.sharpening_params(deconvradius=0.9)
    keep = []
    mask = tb_lib.smooth_mask(w, h)
    box = np.zeros((h, w), np.float32); box[40:140, 60:200] = 0.8
    cc = CC._capi_regions([dict(CC.PIPE_REGIONS[0], lmask=mask, abmask=mask), dict(CC.PIPE_REGIONS[1])], True, w, h, keep)
    sm = SM._capi_regions([dict(SM.PIPE_REGIONS[0], mask=sm_lib.mask("between", w, h)), dict(SM.PIPE_REGIONS[1], mask=box)], True, w, h, keep)
    tb_masks, lc_masks = SM._capi_masks(MK.TB_MASKS), SM._capi_masks(MK.LC_MASKS)
    lc_curve = lc_lib.curve_lut(lc_lib.BOOST_CURVE_POINTS)
    tb_arr, keep_tb = capi.texture_boost_regions([r + (None,) for r in MK.TB_REGIONS])
    lc_arr, keep_lc = capi.local_contrast_regions([(60.0, lc_curve, None)])
    p.dehaze_enabled = 1; p.dehaze = dh
    p.sharpening_enabled = 1; p.sharpening = sp; p.sharpening_auto_radius = 0
    p.texture_boost_enabled = 1; p.texture_boost_nregions = len(MK.TB_REGIONS); p.texture_boost_regions = tb_arr
    p.local_contrast_enabled = 1; p.local_contrast_nregions = 1; p.local_contrast_regions = lc_arr
    try:
        gpu_ctx.set_pipeline_color_correction(cc)
        gpu_ctx.set_pipeline_smoothing(sm)
        gpu_ctx.set_pipeline_masks(lc_masks, tb_masks)
        got, c = _pipe_on(gpu_ctx, "odd", raw, p)
        host = _pipe_host(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_masks(None, None)
        gpu_ctx.set_pipeline_smoothing(None)
        gpu_ctx.set_pipeline_color_correction(None)
    assert all(np.isfinite(g).all() for g in got)
    verdict(vs_host(got, host, "all tools"), c)
    del keep, keep_dh, keep_tb, keep_lc


def test_batch_run_two_lanes_two_layouts():
    """two frames on two lanes, each on its own layout, against the frames one by one"""
    lut = _lut()
    p = _params(lut, 0)
    raws = [_frame_raw(False, seed=s) for s in (5, 6)]
    ctx = capi.Context(0)
    try:
        singles = [_pipe_host(ctx, r, p) for r in raws]
        ctx.set_batch_lanes(2)
        a_raws = [L.arena(L.LAYOUTS[n], [r]) for n, r in zip(("mixed", "odd"), raws)]
        a_outs = [L.arena(L.LAYOUTS[n], (FH - 8, FW - 8)) for n in ("even_off", "planar16")]
        ctx.batch_run([a.plane for a in a_raws], p, [a.rgb for a in a_outs])
        ctx.synchronize()
        msgs = []
        for f, (ao, ar, s, r) in enumerate(zip(a_outs, a_raws, singles, raws)):
            msgs += vs_host(L.contents(ao), s, f"batch_run frame {f}") + outside(ao, ar, what=f"batch_run frame {f}") + unchanged(ar, [r], f"batch_run frame {f}")
        verdict(msgs)
        assert not np.array_equal(singles[0][1], singles[1][1])
    finally:
        ctx.close()


# ---- two ABI paths: a device source with its own row stride, a device destination with any row stride ------------------------------------------------

@pytest.mark.parametrize("kind", ["bayer_u16", "xtrans_u16", "bayer_f32"])
def test_scale_colors_from_a_strided_device_source(gpu_ctx, kind):
    w, h = 515, 389
    rng = np.random.default_rng(7)
    data = rng.integers(0, 16384, (h, w)).astype(np.uint16)
    if kind == "bayer_f32":
        data = data.astype(np.float32) + np.float32(0.25)
    bayer = not kind.startswith("xtrans")
    filt = synth.FILTERS_GRBG
    cfa = synth.XTRANS_FUJI if not bayer else np.array([[synth.fc(filt, r, c) for c in range(6)] for r in range(6)], np.int32)
    black, mul = (511.0, 512.5, 509.0, 513.0), (2.31, 1.0, 1.57, 1.02)
    ref, rmx = O.scale_colors(data, cfa, bayer, black, mul)
    host = np.zeros((h, w), np.float32)
    hmx = gpu_ctx.scale_colors(data, filt, None if bayer else synth.XTRANS_FUJI, black, mul, capi.host_plane(host))
    wide = np.full((h, w + 3), 0x5A5A if data.dtype == np.uint16 else 12345.0, data.dtype)          # rows of w + 3 elements
    wide[:, :w] = data
    d_src = torch.from_numpy(wide.view(np.int16) if data.dtype == np.uint16 else wide).to(L.DEVICE)
    ar = L.arena(L.LAYOUTS["odd"], [np.zeros((h, w), np.float32)])
    mx = gpu_ctx.scale_colors(None, filt, None if bayer else synth.XTRANS_FUJI, black, mul, ar.plane, device_src=d_src[:, :w])
    gpu_ctx.synchronize()
    got = L.contents(ar)
    assert [np.float32(v) for v in mx] == [np.float32(v) for v in rmx] and mx == hmx
    assert np.array_equal(d_src.cpu().numpy().view(wide.dtype), wide), "scale_colors wrote its source"
    verdict(vs_checker(got, [ref], "scale_colors"), vs_host(got, [host], "scale_colors"), outside(ar, what="scale_colors"))


@pytest.mark.parametrize("extra", ["16", "4esz"])
@pytest.mark.parametrize("bps,fl", [(8, False), (16, False), (16, True), (32, True)])
def test_get_scanlines_into_a_strided_device_buffer(gpu_ctx, bps, fl, extra):
    """rows rowb + 16 and rowb + 4 x (element size) bytes apart; everything around them holds 0xA5 before and after"""
    rng = np.random.default_rng(21)
    h, w = 97, 211
    img = [rng.uniform(-200.0, 60000.0, (h, w)).astype(np.float32) for _ in range(3)]
    img[0][0, :8] = [np.nan, -1.0, 0.49, 0.5, 65534.6, 65535.0, 70000.0, 1e-3]
    esz = bps // 8
    rowb = w * 3 * esz
    stride = rowb + (16 if extra == "16" else 4 * esz)
    ref = O.get_scanlines(img, bps, fl)
    host = gpu_ctx.get_scanlines(capi.host_rgb(img), bps, fl)
    ar = L.arena(L.LAYOUTS["mixed"], img)
    buf = L.byte_arena(h, rowb, stride)
    gpu_ctx.get_scanlines(ar.rgb, bps, fl, device_dst=buf[2:2 + h])
    gpu_ctx.synchronize()
    got = L.byte_check(buf, h, rowb, what=f"(c) get_scanlines {bps} bit")
    assert np.array_equal(got, np.ascontiguousarray(ref).view(np.uint8).reshape(h, rowb)), "(a) scanlines differ from the checker"
    assert np.array_equal(got, np.ascontiguousarray(host).view(np.uint8).reshape(h, rowb)), "(b) scanlines differ from the host destination"
    verdict(outside(ar, what="get_scanlines"), unchanged(ar, img, "get_scanlines"))


# ---- the reference's four-wide body is followed by COLUMN, never by address ---------------------------------------------------------------------

AW, AH = 139, 37


def _shifted(ctx, img, call):
    """call(rgb) on the same planes starting 0, 1, 2 and 3 floats into their rows -> the four windows, messages of (c)"""
    outs, msgs = [], []
    for s in range(4):
        ar = L.arena(L.Layout(5, (s, s, s), name=f"shift{s}"), img)
        call(ar.rgb)
        ctx.synchronize()
        outs.append(L.contents(ar))
        msgs += outside(ar, what=f"shift {s}")
    return outs, msgs


def _all_equal(outs, what):
    return [m for s in range(1, 4) for m in vs_host(outs[s], outs[0], f"{what} at shift {s} against shift 0")]


def test_rgb_to_lab_does_not_depend_on_the_address(gpu_ctx):
    rgb, lab, _, _, _ = lab_case(AW, AH)
    outs, c = _shifted(gpu_ctx, rgb, lambda im: gpu_ctx.rgb_to_lab(im, WS))
    verdict(vs_checker(outs[0], lab, "rgb_to_lab"), _all_equal(outs, "rgb_to_lab"), c)


def test_lab_adjustments_does_not_depend_on_the_address(gpu_ctx):
    _, _, adj, cv, ref = lab_case(AW, AH)
    outs, c = _shifted(gpu_ctx, adj, lambda im: gpu_ctx.lab_adjustments(im, *cv, 1.35))
    verdict(vs_checker(outs[0], ref, "lab_adjustments"), _all_equal(outs, "lab_adjustments"), c)


def test_color_correction_does_not_depend_on_the_address(gpu_ctx):
    """one Jzazbz region; the checker is tests/cc_lib.py's, outside its powf pixels as in test_gpu_colorcorrection.py"""
    img = cc_lib.scene(AW, AH, seed=5, nans=False)
    img[0][22, 21] = np.nan                  # a column of the four-wide body
    img[1][AH - 2, AW - 1] = np.nan          # the last column of a width with w % 4 == 3
    region = dict(mode=cc_lib.JZAZBZ, **cc_lib.SOP)
    want, _, oor, _ = cc_lib.color_correction(img, [region], to_rgb=True)
    outs, c = _shifted(gpu_ctx, img, lambda im: gpu_ctx.color_correction(im, [dict(region)], WS, IWS, True))
    verdict(vs_checker(outs[0], want, "color_correction", ~oor), _all_equal(outs, "color_correction"), c)
