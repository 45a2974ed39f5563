"""GPU: the value-domain families of tests/value_domains.py (negatives, fractions, runs of zeros, constant tiles, -0.0, subnormals, values far
above 65535) through every raw and denoise stage, device against the CPU checker.

The comparison is `view(np.uint32)` equality over ALL pixels: no NaN mask, nothing excluded.  tests/test_oracle_value_domains.py asserts that
the checker's output is finite on every family, so the device's must be too; it also asserts that the checker's output holds -0.0 on `negzero`
and subnormals on `tiny`, the bits that part a GPU from an SSE2 CPU first (the sign of a zero, a flushed subnormal, which operand a min / max
returns on a tie, a float-to-index conversion).  A failure names the family, the stage, the count, the first coordinates and both values in hex.

Two families go beyond the nine the stages were first run on: `mixed_zeros` puts +0.0 next to -0.0, the only finite operands on which an SSE
min / max and the device's own can return different bits, and `small` (up to 1e-9) makes the shrink update c x sf^2 subnormal.  Neither a min / max
swapped for fminf / fmaxf in the AMaZE or CA kernels nor a flush-to-zero build of shrinkblur.hip changes any bit these cases see (DESIGN.md section
3.1 says what was tried): the cases pin the families' bits, they do not detect those two mutations.

Only the DCT detail recovery is a tolerance stage; its bound scales with the magnitude of the planes."""
import numpy as np
import pytest
import torch

import oracle_lib as O
import value_domains as VD
import test_oracle_value_domains as R
from art_amd import capi, synth
from test_gpu_pipeline import _lut, _params

pytestmark = pytest.mark.gpu

FAMILIES = R.FAMILIES
W, H, FILT = R.W, R.H, R.FILT
BAYER_SIZES = [(262, 198, synth.FILTERS_GRBG), (389, 275, synth.FILTERS_RGGB)]     # the second: odd sizes, a second tile row
DCT_ABS_BOUND = 0.0625          # on data up to 65535: DESIGN.md section 3, tests/test_gpu_denoise.py
DCT_FAMILIES = ["dark_offset", "scaled_frac", "zero_and_sat_blocks", "constant", "all_zero", "negzero"]
DCT_RAN = {"scaled_frac", "zero_and_sat_blocks", "negzero", "dark_offset"}       # where the checker with and without the stage differs by > 5
DCT_W, DCT_H = 300, 275
DCT_DETAIL = 80.0               # luminanceDetail: at 50 the stage moves `dark_offset` (|v| < 600) by 3.3 only, at 80 by 19.7


def _check(pairs):
    """pairs: (what, got, want) of float32 arrays; every bit of every value, all failures in one message.  The checker's side must be finite
    (asserted here for every case, at every size; tests/test_oracle_value_domains.py asserts it on the CPU for the 262 x 198 cases): that is
    what makes a comparison without a mask a statement about the device."""
    for what, _, w in pairs:
        assert np.isfinite(w).all(), f"{what}: the checker's output is not finite"
    msgs = [m for m in (VD.report_mismatch(g, w, what) for what, g, w in pairs) if m]
    assert not msgs, "\n".join(msgs)


def _planes(what, got, want):
    return [(f"{what} {c}", g, w) for c, g, w in zip("RGB", got, want)]


def _demosaic(ctx, method, raw, filters, gain=1.0):
    h, w = raw.shape
    out = [np.full((h, w), np.nan, np.float32) for _ in range(3)]
    ctx.demosaic_bayer(method, capi.host_plane(np.ascontiguousarray(raw)), filters, gain, 4, capi.host_rgb(out))
    return out


OPTION_DEFAULTS = {"amaze_path": 0, "rcd_rows": 8, "dn_fused": 1, "dn_detail_plain": 0}       # include/artgpu.h


class _options:
    """context options for the length of a with block, then back to their defaults (the session's context is shared with every other test)"""
    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.ctx.set_option(k, OPTION_DEFAULTS[k])


# ---- Bayer demosaic -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,filters", BAYER_SIZES, ids=lambda v: hex(v) if v > 4096 else str(v))
@pytest.mark.parametrize("name", FAMILIES)
def test_amaze(gpu_ctx, name, w, h, filters):
    raw = R.frame(name, w, h, filters)
    gains = [1.0] + ([2.1] if name in ("scaled_frac", "zero_and_sat_blocks") else [])          # 2.1: clip point below the data
    pairs = []
    for gain in gains:
        ref = R.o_amaze(name, w, h, filters, gain)
        for path in (0, 1):                          # 0: LDS streaming kernel (+ arena for partial tiles), 1: arena kernel for every tile
            with _options(gpu_ctx, amaze_path=path):
                got = _demosaic(gpu_ctx, capi.BAYER_AMAZE, raw, filters, gain)
            pairs += _planes(f"{name} {w}x{h} amaze path {path} gain {gain}", got, ref)
    _check(pairs)


@pytest.mark.parametrize("w,h,filters", BAYER_SIZES, ids=lambda v: hex(v) if v > 4096 else str(v))
@pytest.mark.parametrize("name", FAMILIES)
def test_rcd(gpu_ctx, name, w, h, filters):
    raw = R.frame(name, w, h, filters)
    ref = R.o_rcd(name, w, h, filters)
    pairs = []
    for rows in (8, 4):
        with _options(gpu_ctx, rcd_rows=rows):
            pairs += _planes(f"{name} {w}x{h} rcd rows {rows}", _demosaic(gpu_ctx, capi.BAYER_RCD, raw, filters), ref)
    _check(pairs)


@pytest.mark.parametrize("w,h,filters", BAYER_SIZES, ids=lambda v: hex(v) if v > 4096 else str(v))
@pytest.mark.parametrize("name", FAMILIES)
def test_vng4(gpu_ctx, name, w, h, filters):
    raw = R.frame(name, w, h, filters)
    _check(_planes(f"{name} {w}x{h} vng4", _demosaic(gpu_ctx, capi.BAYER_VNG4, raw, filters), R.o_vng4(name, w, h, filters)))


# ---- X-Trans --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("passes,lab,roll", [(1, False, (0, 0)), (3, True, (0, 0)), (3, True, (2, 3))], ids=["1pass", "3pass_lab", "3pass_lab_rolled"])
@pytest.mark.parametrize("name", FAMILIES)
def test_xtrans(gpu_ctx, name, passes, lab, roll):
    xt = R.xtrans_map(roll)
    raw = R.frame(name, W, H, 0, roll)
    out = [np.full((H, W), np.nan, np.float32) for _ in range(3)]
    gpu_ctx.demosaic_xtrans(passes, lab, capi.host_plane(np.ascontiguousarray(raw)), xt, synth.XTRANS_RGB_CAM, capi.host_rgb(out))
    _check(_planes(f"{name} xtrans passes {passes} lab {lab} roll {roll}", out, R.o_xtrans(name, passes, lab, roll)))


# ---- dual demosaic --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method,contrast", [("amaze", None), ("rcd", None), ("amaze", 20.0)], ids=["amaze_auto", "rcd_auto", "amaze_20"])
@pytest.mark.parametrize("name", FAMILIES)
def test_dual_demosaic_with_vng4(gpu_ctx, name, method, contrast):
    """auto contrast as the issue sets it (the search finds no flat tile on any family: threshold 0); a fixed threshold in addition, so that
    the blend itself sees the families too"""
    raw = np.ascontiguousarray(R.frame(name))
    out = [np.full((H, W), np.nan, np.float32) for _ in range(3)]
    got_c = gpu_ctx.dual_demosaic_bayer(capi.BAYER_RCD if method == "rcd" else capi.BAYER_AMAZE, capi.host_plane(raw), FILT, 1.0, 4, contrast or 0.0,
                                        contrast is None, capi.host_rgb(out), second=capi.DUAL_VNG4)
    ref, ref_c = R.o_dual(name, method, contrast)
    assert got_c == ref_c, f"{name} dual {method}: contrast {got_c!r}, checker {ref_c!r}"
    _check(_planes(f"{name} dual {method} + vng4 contrast {contrast}", out, ref))


# ---- raw CA correction ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("guard", [True, False], ids=["guard", "noguard"])
@pytest.mark.parametrize("mode", list(R.CA_MODES))
@pytest.mark.parametrize("name", FAMILIES)
def test_raw_ca_correct(gpu_ctx, name, mode, guard):
    raw = R.frame(name, R.CA_W, R.CA_H)
    want, wfit, info = R.o_ca(name, mode, guard)
    if mode == "auto2":
        assert info["processpasstwo"] == R.CA_PASS_TWO[name], info
    kw = R.CA_MODES[mode]
    d = torch.from_numpy(raw.copy()).to("cuda:0")
    p = capi.CaParams(1 if kw["autocorrect"] else 0, kw["iterations"], kw.get("red", 0.0), kw.get("blue", 0.0), 1 if guard else 0)
    fit = gpu_ctx.raw_ca_correct(capi.device_plane(d), FILT, p, want_fit=True)
    gpu_ctx.synchronize()
    got = d.cpu().numpy()
    bad_fit = fit.reshape(-1).view(np.uint64) != wfit.reshape(-1).view(np.uint64)
    msg = VD.report_mismatch(got, want, f"{name} ca {mode} guard {guard} raw")
    assert not msg and not bad_fit.any(), f"{msg}\nfitparams: {int(bad_fit.sum())} of 64 differ: got {fit.reshape(-1)[bad_fit][:5]} want {wfit.reshape(-1)[bad_fit][:5]}"


# ---- rgb_denoise without the DCT stage --------------------------------------------------------------------------------------------------------

def _fused_taken(w, h):
    """shrink_blur_supported (art_amd/csrc/shrinkblur.hip:577-587, `w < 64 || h < 64`; if that threshold moves, move this with it, or the
    262 x 120 case stops exercising the three-kernel fall-back): the fused shrink pass takes a frame whose bands -- (w + 1) / 2 x (h + 1) / 2 -- are 64 x 64 or more"""
    return (w + 1) // 2 >= 64 and (h + 1) // 2 >= 64


# 262 x 198 and one size well above it as the issue sets them; 262 x 120 in addition, because 262 x 198 (bands of 131 x 99) is already taken by
# the fused pass and the fall-back to the three-kernel form below the threshold would otherwise see no family
DN_SIZES = [(W, H, None), (W, H, 120), (R.CA_W, R.CA_H, None)]
assert _fused_taken(W, H) and not _fused_taken(W, 120) and _fused_taken(R.CA_W, R.CA_H)


@pytest.mark.parametrize("lum,chrom", [(40.0, 15.0), (0.0, 60.0)], ids=["l40c15", "l0c60"])
@pytest.mark.parametrize("w,h,crop_h", DN_SIZES, ids=["262x198", "262x120", "700x500"])
@pytest.mark.parametrize("name", FAMILIES)
def test_rgb_denoise_shrink_forms(gpu_ctx, name, w, h, crop_h, lum, chrom):
    img = R.dn_input(name, w, h, crop_h)
    ref = R.o_rgb_denoise(name, w, h, crop_h, lum, chrom)
    p = capi.DenoiseParams(lum, 50.0, 0, chrom, 0.0, 0.0, 1.7, 0, 0, 0)
    pairs = []
    for form in (1, 0, 2):          # one launch for the three channels / three kernels per channel / one fused launch per channel
        got = [x.copy() for x in img]
        with _options(gpu_ctx, dn_fused=form):
            gpu_ctx.rgb_denoise(capi.host_rgb(got), p, O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY)
        pairs += _planes(f"{name} {w}x{crop_h or h} rgb_denoise lum {lum} chrom {chrom} dn_fused {form}", got, ref)
    _check(pairs)


# ---- the denoise tool ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_guided_smoothing(gpu_ctx, name):
    got = [x.copy() for x in R.dn_input(name)]
    gpu_ctx.denoise_guided_smoothing(capi.host_rgb(got), O.REC2020_WS_D, 3, 1.0)
    _check(_planes(f"{name} guided smoothing radius 3", got, R.o_guided(name)))


@pytest.mark.parametrize("name", FAMILIES)
def test_improc_denoise_tool(gpu_ctx, name):
    got = [x.copy() for x in R.dn_input(name)]
    tp = capi.DenoiseToolParams(capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0), 1, 3, 50, 80)
    gpu_ctx.improc_denoise(capi.host_rgb(got), tp, O.REC2020_WS_D, ecomp=0.3, calclum_mat=R.MAT, noise_c_curve=O.noise_curve()[0],
                           flags=capi.DN_SKIP_DETAIL_RECOVERY)
    _check(_planes(f"{name} improc_denoise (noise map, guided 3, NL-means 50/80, ecomp 0.3)", got, R.o_improc(name)))


@pytest.mark.parametrize("name", FAMILIES)
def test_denoise_compute_params(gpu_ctx, name):
    pl = [x.copy() for x in R.dn_input(name)]
    dn = capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 1)
    st = gpu_ctx.denoise_compute_params(capi.host_rgb(pl), 4, R.DN_MUL, True, R.MAT, O.REC2020_WS_D, dn)
    store, info = R.o_dninfo(name)
    assert st.valid == 1
    got_info = np.array([list(st.crop_info[k]) for k in range(9)], np.float32)
    got_store = np.array([st.chrominance, st.chrominance_red_green, st.chrominance_blue_yellow] + list(st.ch_M) + list(st.max_r) + list(st.max_b), np.float32)
    _check([(f"{name} denoise_compute_params info", got_info[:, :11], np.ascontiguousarray(info[:, :11])), (f"{name} denoise_compute_params store", got_store, store)])


# ---- DCT detail recovery (tolerance stage) ------------------------------------------------------------------------------------------------------

def _detail(ctx, img, plain):
    got = [x.copy() for x in img]
    p = capi.DenoiseParams(40.0, DCT_DETAIL, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0)
    with _options(ctx, dn_detail_plain=plain):
        ctx.rgb_denoise(capi.host_rgb(got), p, O.REC2020_WS, flags=0)
    return got


@pytest.mark.parametrize("name", FAMILIES)
def test_detail_recovery_trimmed_equals_plain(gpu_ctx, name):
    img = R.dn_input(name, DCT_W, DCT_H)
    _check(_planes(f"{name} detail recovery, trimmed against plain kernels", _detail(gpu_ctx, img, 0), _detail(gpu_ctx, img, 1)))


@pytest.mark.parametrize("name", DCT_FAMILIES)
def test_detail_recovery_within_scaled_bound(gpu_ctx, name):
    """max |device - checker| <= DCT_ABS_BOUND x max(1, peak / 65535), peak the largest |value| handed to rgb_denoise: 0.0625 was established
    for data up to 65535 and the error of an fp32 transform scales with the block's magnitude."""
    img = R.dn_input(name, DCT_W, DCT_H)
    peak = max(float(np.abs(p).max()) for p in img)
    got = _detail(gpu_ctx, img, 0)
    ref = R.o_rgb_denoise(name, DCT_W, DCT_H, detail=True, lum_detail=DCT_DETAIL)
    nodetail = R.o_rgb_denoise(name, DCT_W, DCT_H, detail=False, lum_detail=DCT_DETAIL)
    assert all(np.isfinite(p).all() for p in got), f"{name}: {[VD.describe(p) for p in got]}"
    errs = [float(np.abs(g.astype(np.float64) - r.astype(np.float64)).max()) for g, r in zip(got, ref)]
    bound = DCT_ABS_BOUND * max(1.0, peak / 65535.0)
    ran = max(float(np.abs(r.astype(np.float64) - nd.astype(np.float64)).max()) for r, nd in zip(ref, nodetail))
    print(f"DCT {name} {DCT_W}x{DCT_H}: peak {peak:.6g}, max |device - checker| = {errs} (bound {bound:.6g}), checker with - without = {ran:.6g}")
    assert max(errs) <= bound, (name, errs, bound)
    if name in DCT_RAN:
        assert ran > 5.0           # the stage really ran
    else:
        assert ran == 0.0


# ---- one context, families in sequence ------------------------------------------------------------------------------------------------------------

def test_extreme_frames_leave_nothing_behind_on_a_context():
    """huge, all_zero, tiny, then scaled_frac through AMaZE and rgb_denoise (shrink passes, then with the DCT stage) on ONE context: the last must
    give the bits a fresh context gives -- pooled scratch, the LDS tables and the fused pass's hand-over slots carry nothing over."""
    p = capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0)

    def run(ctx, name):
        dem = _demosaic(ctx, capi.BAYER_AMAZE, R.frame(name), FILT)
        a = [x.copy() for x in R.dn_input(name)]
        ctx.rgb_denoise(capi.host_rgb(a), p, O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY)
        b = [x.copy() for x in R.dn_input(name)]
        ctx.rgb_denoise(capi.host_rgb(b), p, O.REC2020_WS, flags=0)
        return dem, a, b

    fresh = capi.Context(0)
    try:
        want = run(fresh, "scaled_frac")
    finally:
        fresh.close()
    used = capi.Context(0)
    try:
        for name in ("huge", "all_zero", "tiny"):
            run(used, name)
        got = run(used, "scaled_frac")
    finally:
        used.close()
    pairs = []
    for stage, g, w in zip(("amaze", "rgb_denoise", "rgb_denoise + detail recovery"), got, want):
        pairs += _planes(f"scaled_frac after huge, all_zero, tiny: {stage}", g, w)
    pairs += _planes("scaled_frac on a fresh context: amaze", want[0], R.o_amaze("scaled_frac"))
    pairs += _planes("scaled_frac on a fresh context: rgb_denoise", want[1], R.o_rgb_denoise("scaled_frac"))
    _check(pairs)


# ---- pipe equals stages -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["scaled_frac", "zero_and_sat_blocks"])
def test_pipeline_with_ca_equals_stages(gpu_ctx, name):
    w, h, b = R.CA_W, R.CA_H, 4
    raw = R.frame(name, w, h)
    lut = _lut()
    p = _params(lut, 0)
    p.filters = FILT
    p.ca_enabled = 1
    p.ca = capi.CaParams(1, 2, 0.0, 0.0, 1)
    d_raw = torch.from_numpy(raw.copy()).cuda()
    d_out = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda") for _ in range(3)]
    gpu_ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_out]))
    gpu_ctx.synchronize()
    assert np.array_equal(d_raw.cpu().numpy().view(np.uint32), raw.view(np.uint32)), "pipeline_run wrote the caller's raw"
    # the same stages one by one
    d_cfa = torch.from_numpy(raw.copy()).cuda()
    gpu_ctx.raw_ca_correct(capi.device_plane(d_cfa), FILT, p.ca)
    d_dem = [torch.empty((h, w), dtype=torch.float32, device="cuda") for _ in range(3)]
    dem = capi.RGB(*[capi.device_plane(t) for t in d_dem])
    gpu_ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_cfa), FILT, 1.0, b, dem)
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    gpu_ctx.get_image(dem, b, b, tuple(p.mul), True, R.MAT, img)
    gpu_ctx.improc_denoise(img, p.denoise, O.REC2020_WS_D, ecomp=0.3, calclum_mat=R.MAT, noise_c_curve=capi.noise_curve_lut()[0], iws=O.REC2020_IWS_D)
    gpu_ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    gpu_ctx.tone_curve(img, lut, 1.0, True)
    gpu_ctx.synchronize()
    assert not np.array_equal(d_cfa.cpu().numpy(), raw), "CA changed nothing"
    _check(_planes(f"{name} pipeline_run with CA against the stages", [t.cpu().numpy() for t in d_out], [t.cpu().numpy() for t in d_img]))
