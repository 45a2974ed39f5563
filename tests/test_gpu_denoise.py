"""GPU parity: wavelet part of RGB_denoise (gamma/YUV, MAD, shrink + box blurs, reconstruct) vs the oracle."""
import numpy as np
import pytest

import oracle_lib as O
from art_amd import capi, synth

pytestmark = pytest.mark.gpu


def _same(a, b):
    return [int((x.view(np.uint32) != y.view(np.uint32)).sum()) for x, y in zip(a, b)]


def _rgb(w, h, seed, noise=2048):
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=seed, noise=noise)
    return O.amaze(raw, synth.FILTERS_RGGB, 1.0, 4)


def _params(**kw):
    from art_amd import capi
    p = capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("w,h,kw", [
    (640, 480, {}),
    (517, 389, {}),                                         # odd sizes: N % 4 != 0 tails, W % 4 != 0 blur columns
    (642, 482, dict(chrominance=90.0)),                     # more wavelet levels (realred >= 8 -> 6 levels)
    (512, 384, dict(luminance=0.0)),                        # chroma only
    (512, 384, dict(chrominance_red_green=-30.0, chrominance_blue_yellow=40.0, gamma=1.0)),
])
def test_rgb_denoise_wavelet_bit_exact(gpu_ctx, w, h, kw):
    from art_amd import capi
    img = _rgb(w, h, w)
    got = [p.copy() for p in img]
    gpu_ctx.rgb_denoise(capi.host_rgb(got), _params(**kw), O.REC2020_WS)
    okw = dict(luminance=kw.get("luminance", 40.0), chrominance=kw.get("chrominance", 15.0),
               chrominanceRedGreen=kw.get("chrominance_red_green", 0.0), chrominanceBlueYellow=kw.get("chrominance_blue_yellow", 0.0),
               gamma=kw.get("gamma", 1.7))
    ref = O.rgb_denoise(img, O.default_denoise_params(**okw))
    assert _same(got, ref) == [0, 0, 0]
    assert all(np.isfinite(p).all() for p in got)


def test_rgb_denoise_with_chroma_curve_map(gpu_ctx):
    from art_amd import capi
    w, h = 500, 380
    img = _rgb(w, h, 21)
    rng = np.random.default_rng(0)
    ccalc = (1.0 + 4.0 * rng.uniform(0.01, 0.5, ((h + 1) // 2, (w + 1) // 2))).astype(np.float32) ** 2
    got = [p.copy() for p in img]
    gpu_ctx.rgb_denoise(capi.host_rgb(got), _params(), O.REC2020_WS, ccalc=capi.host_plane(ccalc))
    ref = O.rgb_denoise(img, O.default_denoise_params(), noisevarchrom=ccalc)
    assert _same(got, ref) == [0, 0, 0]


def test_unsupported_modes_fail_loudly(gpu_ctx):
    from art_amd import capi
    img = _rgb(256, 256, 1)
    with pytest.raises(capi.ArtGpuError):
        gpu_ctx.rgb_denoise(capi.host_rgb(img), _params(color_space=1), O.REC2020_WS)   # LAB without the inverse matrix
    with pytest.raises(capi.ArtGpuError):
        gpu_ctx.rgb_denoise(capi.host_rgb(img), _params(chrominance_method=2), O.REC2020_WS)   # not MANUAL / AUTOMATIC


# detail_recovery (FTblockDN.cc:1479-1635) is the one stage of the path that cannot be compared bit for bit: the reference calls
# FFTW's single-precision REDFT10 / REDFT01 plans (planner-dependent round-off, library not part of the reference tree).  The checker
# evaluates FFTW's documented transform definitions with double accumulation; the device uses an fp32 Lee fast DCT.  What can be
# asserted: (i) the device is as close to the exact transform as a plain fp32 direct-form evaluation is (its error distribution is
# measured against that yardstick in the same test), (ii) an absolute bound on the final R, G, B, stated in DESIGN.md section 3.
# Measured on MI355X (this test prints the figures): max |device - exact| = 0.031 on the 0..65535 output scale (16 ulp of a mid-scale
# value; the fp32 direct form has the same maximum), 99.9th percentile 0.012, median 0 (most values come out bit-identical).
DCT_ABS_BOUND = 0.0625      # 2 x the measured maximum; the same number is in DESIGN.md section 3 and tests/test_gpu_fullsize.py
DCT_MEDIAN_BOUND = 0.002


def _ulp(x):
    """ulp of the value's binade, floored at the ulp of 256 (a relative figure is meaningless for the few near-zero outputs)"""
    return np.spacing(np.maximum(np.abs(x), 256.0).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("w,h,detail", [(640, 480, 50.0), (517, 389, 80.0), (330, 260, 0.0)])
def test_rgb_denoise_with_detail_recovery_tolerance(gpu_ctx, w, h, detail):
    from art_amd import capi
    img = _rgb(w, h, w + 1)
    got = [p.copy() for p in img]
    gpu_ctx.rgb_denoise(capi.host_rgb(got), _params(luminance_detail=detail), O.REC2020_WS, flags=0)
    ref = O.rgb_denoise(img, O.default_denoise_params(luminanceDetail=detail), detail_recovery=True)
    f32 = O.rgb_denoise(img, O.default_denoise_params(luminanceDetail=detail), detail_recovery="f32")
    nodetail = O.rgb_denoise(img, O.default_denoise_params(luminanceDetail=detail), detail_recovery=False)
    for g, r, d32, nd in zip(got, ref, f32, nodetail):
        err = np.abs(g.astype(np.float64) - r.astype(np.float64))
        err32 = np.abs(d32.astype(np.float64) - r.astype(np.float64))
        u = _ulp(r)
        print(f"detail {detail} {w}x{h}: device max {err.max():.4f} ({(err / u).max():.0f} ulp) median {np.median(err):.5f} ({np.median(err / u):.2f} ulp) p99.9 "
              f"{np.percentile(err, 99.9):.4f} | fp32 direct form max {err32.max():.4f} ({(err32 / u).max():.0f} ulp) median {np.median(err32):.5f} "
              f"({np.median(err32 / u):.2f} ulp) p99.9 {np.percentile(err32, 99.9):.4f}")
        assert err.max() <= DCT_ABS_BOUND, err.max()
        assert np.median(err) <= DCT_MEDIAN_BOUND
        # no worse than a straightforward fp32 evaluation of the same transforms (the 1.5 covers the different error pattern)
        assert np.percentile(err, 99.9) <= 1.5 * np.percentile(err32, 99.9) + 1e-3
        assert np.median(err) <= 1.5 * np.median(err32) + 1e-4
        # the stage really ran: result is far from the no-detail-recovery image
        assert np.abs(r - nd).max() > 50.0


def test_rgb_denoise_survives_non_finite_pixels(gpu_ctx):
    """An Inf / NaN / 1e30 pixel makes wavelet coefficients the MAD histogram (MadRgb, FTblockDN.cc:569-603) cannot bin as an int: they
    go to the top bin instead of indexing out of range (the reference's own conversion is undefined there; its running-sum box blurs
    then spread the non-finite values along whole rows and columns, so the frame itself is not comparable).  The call has to
    complete without touching memory it does not own: the next frame through the same context is the oracle's bit for bit."""
    from art_amd import capi
    w, h = 384, 320
    img = _rgb(w, h, 5)
    clean = [p.copy() for p in img]
    img[0][40, 50] = np.inf
    img[1][41, 300] = np.nan
    img[2][200, 60] = -1e30
    got = [p.copy() for p in img]
    gpu_ctx.rgb_denoise(capi.host_rgb(got), _params(), O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY)
    gpu_ctx.synchronize()
    got = [p.copy() for p in clean]
    gpu_ctx.rgb_denoise(capi.host_rgb(got), _params(), O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY)
    ref = O.rgb_denoise(clean, O.default_denoise_params(), detail_recovery=False)
    for g, r in zip(got, ref):
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32))


def test_chroma_noise_map_bit_exact(gpu_ctx):
    """calclum + ccalc (ipdenoise.cc:1113-1131, FTblockDN.cc:1716-1777) incl. the f<0 and f>65535 branches of XYZ2Lab."""
    w, h = 333, 251
    rng = np.random.default_rng(5)
    img = [rng.uniform(-200.0, 70000.0, (h, w)).astype(np.float32) for _ in range(3)]
    img[0][:40] *= 3.0                      # strongly coloured band: cN > 100 and X/D50x > 65535
    img[2][60:90] = 0.0
    mat = np.array([[0.6325, 0.2312, 0.0921], [0.2198, 0.7712, 0.0090], [0.0166, 0.0713, 0.7514]])
    curve, s = capi.noise_curve_lut()
    assert s > 5.0
    for m in (mat, None):
        got = np.zeros(((h + 1) // 2, (w + 1) // 2), np.float32)
        gpu_ctx.denoise_chroma_map(capi.host_rgb(img), m, O.REC2020_WS_D, curve, capi.host_plane(got))
        ref = O.chroma_noise_map(img, m, O.REC2020_WS_D, curve)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        assert len(np.unique(ref)) > 100     # the map is not the cN<=100 constant everywhere


def test_improc_denoise_with_noise_curve_bit_exact(gpu_ctx):
    """ImProcFunctions::denoise as ART runs it: fixed chroma noise curve, exposure bracketing; DCT stage skipped so every
    remaining stage must agree bit for bit."""
    import torch
    w, h = 400, 296
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=4, noise=2048)
    img = O.amaze(raw, synth.FILTERS_RGGB, 1.0, 4)
    mat = np.array([[0.6325, 0.2312, 0.0921], [0.2198, 0.7712, 0.0090], [0.0166, 0.0713, 0.7514]])
    curve, _ = capi.noise_curve_lut()
    d = [torch.from_numpy(p.copy()).cuda() for p in img]
    rgb = capi.RGB(*[capi.device_plane(t) for t in d])
    tp = capi.DenoiseToolParams(capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0), 0, 3, 0, 80)
    gpu_ctx.improc_denoise(rgb, tp, O.REC2020_WS_D, ecomp=0.3, calclum_mat=mat, noise_c_curve=curve, flags=capi.DN_SKIP_DETAIL_RECOVERY)
    gpu_ctx.synchronize()
    ref = O.improc_denoise(img, calclum_mat=mat, noise_c_curve=curve, smoothing=False, ecomp=0.3, detail_recovery=False)
    for t, r in zip(d, ref):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), r.view(np.uint32))
    # host-pointer (drop-in) form of the same call
    got = [p.copy() for p in img]
    gpu_ctx.improc_denoise(capi.host_rgb(got), tp, O.REC2020_WS_D, ecomp=0.3, calclum_mat=mat, noise_c_curve=curve, flags=capi.DN_SKIP_DETAIL_RECOVERY)
    for g, r in zip(got, ref):
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32))


def test_noise_residuals_match_oracle(gpu_ctx):
    """nresi / highresi of RGB_denoise (Noise_residualAB, FTblockDN.cc:605-635,2389-2396): exact integer-histogram medians"""
    w, h = 360, 264
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=8, noise=2500)
    img = O.amaze(raw, synth.FILTERS_RGGB, 1.0, 4)
    got = [p.copy() for p in img]
    nresi, highresi = gpu_ctx.rgb_denoise(capi.host_rgb(got), capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0), O.REC2020_WS,
                                          want_resid=True)
    ref, rn, rh = O.rgb_denoise(img, O.default_denoise_params(), want_resid=True)
    assert np.float32(nresi) == np.float32(rn) and np.float32(highresi) == np.float32(rh) and rn > 0
    for g, r in zip(got, ref):
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32))


@pytest.mark.parametrize("chroma", [15.0, 95.0])
def test_aggressive_mode_bit_exact(gpu_ctx, chroma):
    """DenoiseParams::aggressive (QUALITY_HIGH): two more wavelet levels, WaveletDenoiseAll_BiShrinkAB/L before the standard
    passes, stronger chroma boost (FTblockDN.cc:842-1108,1671-1672,2260,2335-2421)."""
    w, h = 520, 392
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=10, noise=2500)
    img = O.amaze(raw, synth.FILTERS_RGGB, 1.0, 4)
    rng = np.random.default_rng(2)
    ccalc = (1.0 + 4.0 * rng.uniform(0.01, 0.5, ((h + 1) // 2, (w + 1) // 2))).astype(np.float32) ** 2
    for cc in (None, ccalc):
        got = [p.copy() for p in img]
        gpu_ctx.rgb_denoise(capi.host_rgb(got), capi.DenoiseParams(40.0, 50.0, 0, chroma, 0.0, 0.0, 1.7, 1, 0, 0), O.REC2020_WS,
                            ccalc=None if cc is None else capi.host_plane(cc))
        ref = O.rgb_denoise(img, O.default_denoise_params(aggressive=1, chrominance=chroma), noisevarchrom=cc)
        plain = O.rgb_denoise(img, O.default_denoise_params(chrominance=chroma), noisevarchrom=cc)
        assert not np.array_equal(ref[1], plain[1])
        for g, r in zip(got, ref):
            assert np.array_equal(g.view(np.uint32), r.view(np.uint32))


def test_detail_recovery_with_detail_mask_threshold(gpu_ctx):
    """luminanceDetailThreshold > 0: detail_mask (double-precision YvV gaussian, sigma 25) scales the per-position DCT shrink
    strength (FTblockDN.cc:1502-1507,1583).  Same tolerance as the plain detail-recovery test (FFTW boundary)."""
    w, h = 600, 440
    img = _rgb(w, h, 33)
    got = [p.copy() for p in img]
    gpu_ctx.rgb_denoise(capi.host_rgb(got), _params(luminance_detail=60.0, luminance_detail_threshold=40), O.REC2020_WS, flags=0)
    ref = O.rgb_denoise(img, O.default_denoise_params(luminanceDetail=60.0, detail_thresh=40), detail_recovery=True)
    plain = O.rgb_denoise(img, O.default_denoise_params(luminanceDetail=60.0), detail_recovery=True)
    for g, r, pl in zip(got, ref, plain):
        err = np.abs(g.astype(np.float64) - r.astype(np.float64))
        assert err.max() <= 65535.0 * 2e-5 and np.median(err) <= 0.02
        assert np.abs(r - pl).max() > 5.0          # the mask changes the result


@pytest.mark.parametrize("w,h", [(512, 384), (517, 389)])
def test_lab_colour_space_mode_bit_exact(gpu_ctx, w, h):
    """DenoiseParams::colorSpace == LAB: denoiseIGammaTab -> gamma -> rgb2lab ... lab2rgb -> inverse gamma -> denoiseGammaTab
    (FTblockDN.cc:2094-2116,2522-2537)."""
    img = _rgb(w, h, w + 5)
    img[0][:6] *= 2.5                      # values above 65535 exercise the LUT extrapolation and the xcbrtf branch
    got = [p.copy() for p in img]
    gpu_ctx.rgb_denoise(capi.host_rgb(got), _params(color_space=1), O.REC2020_WS, iws=O.REC2020_IWS_D)
    ref = O.rgb_denoise(img, O.default_denoise_params(lab_mode=1))
    plain = O.rgb_denoise(img, O.default_denoise_params())
    assert not np.array_equal(ref[0], plain[0])
    assert _same(got, ref) == [0, 0, 0]


def test_improc_denoise_preview_scale_bit_exact(gpu_ctx):
    """scale > 1 (dcrop.cc preview crops): adjust_params (ipdenoise.cc:35-63) rescales the strengths, RGB_denoise shortens
    its blur radii, guided smoothing and NL-means shrink their radii; DCT stage skipped so everything must agree bit for bit."""
    w, h = 400, 296
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=14, noise=2048)
    img = O.amaze(raw, synth.FILTERS_RGGB, 1.0, 4)
    mat = np.array([[0.6325, 0.2312, 0.0921], [0.2198, 0.7712, 0.0090], [0.0166, 0.0713, 0.7514]])
    curve, _ = capi.noise_curve_lut()
    tp = capi.DenoiseToolParams(capi.DenoiseParams(60.0, 50.0, 0, 25.0, 5.0, -8.0, 1.7, 0, 0, 0), 1, 3, 50, 80)
    got = [p.copy() for p in img]
    gpu_ctx.improc_denoise(capi.host_rgb(got), tp, O.REC2020_WS_D, ecomp=0.3, scale=2.0, calclum_mat=mat, noise_c_curve=curve,
                           flags=capi.DN_SKIP_DETAIL_RECOVERY)
    ref = O.improc_denoise(img, dict(luminance=60.0, chrominance=25.0, chrominanceRedGreen=5.0, chrominanceBlueYellow=-8.0), calclum_mat=mat,
                           noise_c_curve=curve, smoothing=True, radius=3, nl_strength=50, nl_detail=80, ecomp=0.3, scale=2.0, detail_recovery=False)
    for g, r in zip(got, ref):
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32))
    # and the strengths really were rescaled: the same call with scale 1 gives a different image
    got1 = [p.copy() for p in img]
    gpu_ctx.improc_denoise(capi.host_rgb(got1), tp, O.REC2020_WS_D, ecomp=0.3, scale=1.0, calclum_mat=mat, noise_c_curve=curve,
                           flags=capi.DN_SKIP_DETAIL_RECOVERY)
    assert not np.array_equal(got1[1], got[1])


def test_large_frame_lds_gamma_tables_same_bits_as_plain_kernels(gpu_ctx, monkeypatch):
    """frames of >= 4 Mpx run RGB->YUV / YUV->RGB with the lower 40704 gamma-table entries in LDS: wide-range data (both sides of the
    split, above the table, zeros and negatives) must give the bits of the plain kernels (option "lut_lds" 0) and of the oracle"""
    w, h = 2308, 1822
    rng = np.random.default_rng(12)
    base = rng.uniform(0, 1, (h, w)).astype(np.float32) ** 3 * 9000.0           # gain 2^5 * 2^0.3 later: spans 0 .. ~350000
    img = [(base * rng.uniform(0.5, 1.5, (h, w))).astype(np.float32) for _ in range(3)]
    img[0][:4, :64] = 0.0
    img[1][4:8, :64] = -5.0
    img[2][8:12, :64] = 66000.0
    tp = capi.DenoiseToolParams(capi.DenoiseParams(30.0, 50.0, 0, 12.0, 0.0, 0.0, 1.7, 0, 0, 0), 0, 3, 0, 80)
    got = [p.copy() for p in img]
    gpu_ctx.improc_denoise(capi.host_rgb(got), tp, O.REC2020_WS_D, ecomp=0.3, flags=capi.DN_SKIP_DETAIL_RECOVERY)
    gpu_ctx.set_option("lut_lds", 0)
    plain = [p.copy() for p in img]
    try:
        gpu_ctx.improc_denoise(capi.host_rgb(plain), tp, O.REC2020_WS_D, ecomp=0.3, flags=capi.DN_SKIP_DETAIL_RECOVERY)
    finally:
        gpu_ctx.set_option("lut_lds", 1)
    ref = O.improc_denoise(img, dict(luminance=30.0, chrominance=12.0), smoothing=False, ecomp=0.3, detail_recovery=False)
    for g, p, r in zip(got, plain, ref):
        assert np.array_equal(g.view(np.uint32), p.view(np.uint32))
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32))


@pytest.mark.parametrize("w,h,kw", [
    (640, 480, {}),                                         # band 320 x 240: 4 strips, 5 + 1 column blocks
    (517, 389, {}),                                         # band 259 x 195: W % 4 != 0 (scalar-form columns), ragged last strip and block
    (258, 130, {}),                                         # band 129 x 65: one row in the last strip, one column in the last block
    (256, 256, {}),                                         # band 128 x 128: strips and blocks end exactly at the edge
    (130, 900, {}),                                         # band 65 x 450: tall and narrow (8 strips, a column block of one)
    (1400, 134, {}),                                        # band 700 x 67: wide and flat
    (642, 482, dict(chrominance=90.0)),                     # six levels: radii up to 7
    (512, 384, dict(aggressive=1)),                         # the L pass twice, BiShrink's top level on its own
    (700, 500, dict(aggressive=1, chrominance=95.0)),       # radii above 7: the wide-window instantiation
])
def test_fused_shrink_pass_same_bits_as_three_kernels(gpu_ctx, w, h, kw):
    """ShrinkAllL / ShrinkAllAB as one kernel (shrinkblur.hip: strips of 64 rows handing their column sums down) against the three-kernel
    form (option "dn_fused" 0), with and without the side stream (which moves the L pass to a second band set), and against the oracle"""
    img = _rgb(w, h, w + 3 * h)
    outs = {}
    try:
        for fused in (1, 2, 0):                    # one launch for the three channels / one per channel / the three-kernel form
            for streams in (1, 0):
                gpu_ctx.set_option("dn_fused", fused)
                gpu_ctx.set_option("dn_streams", streams)
                got = [p.copy() for p in img]
                gpu_ctx.rgb_denoise(capi.host_rgb(got), _params(**kw), O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY if streams == 0 else 0)
                outs[(fused, streams)] = got
    finally:
        gpu_ctx.set_option("dn_fused", 1)
        gpu_ctx.set_option("dn_streams", 0)        # (the default since round 5)
    for f in (1, 2):
        assert _same(outs[(f, 0)], outs[(0, 0)]) == [0, 0, 0]
        assert _same(outs[(f, 1)], outs[(0, 1)]) == [0, 0, 0]      # (with the DCT stage on: the same kernels on the same L plane)
    okw = dict(luminance=40.0, chrominance=kw.get("chrominance", 15.0))
    if not kw.get("aggressive"):
        ref = O.rgb_denoise(img, O.default_denoise_params(**okw))
        assert _same(outs[(1, 0)], ref) == [0, 0, 0]


@pytest.mark.parametrize("lum,chrom", [(3.0, 2.0), (12.0, 6.0)])
def test_fused_shrink_pass_strong_edges_faint_noise(gpu_ctx, lum, chrom):
    """The fused pass scales its exponentials with one v_ldexp_f32 where the three-kernel form and the oracle multiply by powers of two five
    times (shrinkblur.hip, FASTEXP): the two differ only in subnormal results, for arguments in [-99.4, -89.1] (scripts/exp_ldexp_check.c),
    which the factor then swallows.  Here nearly every coefficient is far above the noise -- flat squares with hard edges under faint noise and weak
    denoising: arguments of -10 to -1e9, thousands of them in that window -- and the three forms still have to agree bit for bit, with and
    without the chroma noise map (the map's coefficients take the fast form only through artgpu_improc_denoise, which knows its sign)."""
    w, h = 1100, 820
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w]
    img = []
    for k, (per, amp) in enumerate(((23, 50000.0), (31, 42000.0), (19, 30000.0))):
        base = (((xx + 3 * k) // per + (yy + 5 * k) // per) % 2).astype(np.float32) * amp + 4000.0
        img.append((base + rng.normal(0.0, 2.5, (h, w))).clip(0, 65535).astype(np.float32))
    p = _params(luminance=lum, chrominance=chrom)
    outs = {}
    try:
        for fused in (1, 0):
            gpu_ctx.set_option("dn_fused", fused)
            got = [q.copy() for q in img]
            gpu_ctx.rgb_denoise(capi.host_rgb(got), p, O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY)
            tool = [q.copy() for q in img]
            curve, _ = capi.noise_curve_lut()
            tp = capi.DenoiseToolParams(p, 0, 3, 0, 80)
            gpu_ctx.improc_denoise(capi.host_rgb(tool), tp, O.REC2020_WS_D, ecomp=0.0, noise_c_curve=curve, flags=capi.DN_SKIP_DETAIL_RECOVERY)
            outs[fused] = (got, tool)
    finally:
        gpu_ctx.set_option("dn_fused", 1)
    assert _same(outs[1][0], outs[0][0]) == [0, 0, 0]
    assert _same(outs[1][1], outs[0][1]) == [0, 0, 0]
    ref = O.rgb_denoise(img, O.default_denoise_params(luminance=lum, chrominance=chrom))
    assert _same(outs[1][0], ref) == [0, 0, 0]
    assert _same(outs[1][0], img) != [0, 0, 0]


def test_fused_shrink_pass_repeats_on_one_context(gpu_ctx):
    """the strips of a band wait for each other through counters in global memory: ten calls in a row, different sizes in between"""
    img = _rgb(1000, 760, 5)
    first = None
    for k in range(10):
        got = [p.copy() for p in img]
        gpu_ctx.rgb_denoise(capi.host_rgb(got), _params(), O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY)
        if first is None:
            first = got
        assert _same(got, first) == [0, 0, 0]
        if k % 3 == 1:
            small = _rgb(300 + 16 * k, 200, k)
            gpu_ctx.rgb_denoise(capi.host_rgb(small), _params(), O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY)
    gpu_ctx.set_option("dn_fused", 0)
    try:
        got = [p.copy() for p in img]
        gpu_ctx.rgb_denoise(capi.host_rgb(got), _params(), O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY)
    finally:
        gpu_ctx.set_option("dn_fused", 1)
    assert _same(got, first) == [0, 0, 0]


def test_gamma_tables_are_rebuilt_when_they_have_to_be(gpu_ctx):
    """RGB_denoise keeps its gamma / inverse-gamma tables on the context between calls with the same gamma: another gamma, and the
    AUTOMATIC estimation (which builds its own table in the same slot), have to invalidate them -- every result equals a fresh context's"""
    img = _rgb(520, 390, 11)
    MATX = np.array([[0.6325, 0.2312, 0.0921], [0.2198, 0.7712, 0.0090], [0.0166, 0.0713, 0.7514]])

    def run(ctx, gamma):
        got = [p.copy() for p in img]
        ctx.rgb_denoise(capi.host_rgb(got), _params(gamma=gamma), O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY)
        return got

    ref = {}
    for g in (1.7, 2.4):
        fresh = capi.Context(0)
        ref[g] = run(fresh, g)
        fresh.close()
    assert _same(ref[1.7], ref[2.4]) != [0, 0, 0]
    for g in (1.7, 1.7, 2.4, 1.7):
        assert _same(run(gpu_ctx, g), ref[g]) == [0, 0, 0]
    auto = capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 1)
    planes = [p.copy() for p in img]
    gpu_ctx.denoise_compute_params(capi.host_rgb(planes), 0, (1.0, 1.0, 1.0), False, MATX, O.REC2020_WS_D, auto)
    assert _same(run(gpu_ctx, 1.7), ref[1.7]) == [0, 0, 0]


def test_context_moves_to_another_stream_between_calls():
    """artgpu_set_stream: the scratch planes and the tables a context keeps between calls belong to whichever stream wrote them last, so
    work on the new stream is ordered behind the work left on the old one -- calls alternating between two streams without any host
    synchronisation in between give the bits of the same calls on one stream"""
    import torch
    dev = torch.device("cuda:0")
    img = _rgb(1400, 1000, 21)
    ref_ctx = capi.Context(0)
    ref = []
    for g in (1.7, 2.2, 1.7):
        got = [p.copy() for p in img]
        ref_ctx.rgb_denoise(capi.host_rgb(got), _params(gamma=g), O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY)
        ref.append(got)
    ref_ctx.close()
    s = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    ctx = capi.Context(0, s[0].cuda_stream)
    src = [torch.from_numpy(p).to(dev) for p in img]
    outs = []
    torch.cuda.synchronize()
    for k, g in enumerate((1.7, 2.2, 1.7)):
        st = s[k % 2]
        ctx.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            work = [t.clone() for t in src]
            ctx.rgb_denoise(capi.RGB(*[capi.device_plane(t) for t in work]), _params(gamma=g), O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY)
        outs.append((st, work))
    torch.cuda.synchronize()
    ctx.close()
    for (st, work), r in zip(outs, ref):
        assert _same([t.cpu().numpy() for t in work], r) == [0, 0, 0]


def test_fused_shrink_pass_under_uneven_load():
    """The strips of a band hand their column sums to each other through global memory while the workgroups that hold them come and go:
    three contexts on three host threads run RGB_denoise on frames of different sizes at the same time, ten rounds each, and every result
    has to be the bits of the same call on an idle device (a stale or torn hand-over shows as a difference in some strip)."""
    import threading
    sizes = [(2600, 1900), (1800, 2500), (3100, 1300)]
    imgs = [_rgb(w, h, 7 + k, noise=1500 + 700 * k) for k, (w, h) in enumerate(sizes)]
    alone = []
    ctxs = [capi.Context(0) for _ in sizes]
    try:
        for ctx, img in zip(ctxs, imgs):
            got = [p.copy() for p in img]
            ctx.rgb_denoise(capi.host_rgb(got), _params(), O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY)
            alone.append(got)
        bad, errs = [], []

        def worker(k):
            try:
                for it in range(10):
                    got = [p.copy() for p in imgs[k]]
                    ctxs[k].rgb_denoise(capi.host_rgb(got), _params(), O.REC2020_WS, flags=0 if it % 2 else capi.DN_SKIP_DETAIL_RECOVERY)
                    if it % 2 == 0 and _same(got, alone[k]) != [0, 0, 0]:
                        bad.append((k, it, _same(got, alone[k])))
            except Exception as e:      # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=worker, args=(k,)) for k in range(len(sizes))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        assert not bad, bad
    finally:
        for c in ctxs:
            c.close()
    # and the idle-device result is the three-kernel form's
    ctx = capi.Context(0)
    try:
        ctx.set_option("dn_fused", 0)
        got = [p.copy() for p in imgs[0]]
        ctx.rgb_denoise(capi.host_rgb(got), _params(), O.REC2020_WS, flags=capi.DN_SKIP_DETAIL_RECOVERY)
        assert _same(got, alone[0]) == [0, 0, 0]
    finally:
        ctx.close()


@pytest.mark.parametrize("w,h,smoothing,nl,ecomp,lum", [
    (645, 483, 0, 0, 0.3, 40.0),       # W % 4 != 0: the exposure's scalar-form columns; both neighbours fused
    (640, 480, 0, 0, 0.0, 40.0),       # no exposure compensation inside the tool: the STAGE_1 exposure is the only scaling of the last pass
    (520, 392, 1, 50, 0.3, 40.0),      # guided smoothing + NL-means stand between RGB_denoise and the exposure: expcomp(-) and the exposure ride on setMode(RGB)
    (523, 390, 1, 0, 0.3, 40.0),       # guided smoothing only: expcomp(-) and the exposure as one pass
    (520, 392, 1, 50, 0.0, 40.0),      # no exposure compensation: the exposure alone rides on setMode(RGB)
    (300, 260, 0, 0, 0.3, 0.0),        # luminance 0 (chroma only)
])
def test_improc_denoise_fused_equals_the_separate_calls(gpu_ctx, w, h, smoothing, nl, ecomp, lum):
    """artgpu_improc_denoise_fused: getImage + convertColorSpace read by the tool's first passes straight from the demosaiced planes,
    ImProcFunctions::exposure applied by its last pass -- against get_image, improc_denoise, exposure called one after the other (and
    those against the oracle elsewhere in this file)"""
    import torch
    raw = synth.bayer_frame(w + 8, h + 8, synth.FILTERS_RGGB, seed=w, noise=2048)
    dem = O.amaze(raw, synth.FILTERS_RGGB, 1.0, 4)
    mul = (2.1374, 1.0, 1.5918)
    mat = np.array([[0.6325, 0.2312, 0.0921], [0.2198, 0.7712, 0.0090], [0.0166, 0.0713, 0.7514]])
    curve, _ = capi.noise_curve_lut()
    tp = capi.DenoiseToolParams(capi.DenoiseParams(lum, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0), smoothing, 3, nl, 80)
    exp_scale = float(np.float32(2.0 ** 0.3))
    d_dem = [torch.from_numpy(p).cuda() for p in dem]
    p_dem = capi.RGB(*[capi.device_plane(t) for t in d_dem])
    outs = []
    for fused in (True, False):
        d_img = [torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
        img = capi.RGB(*[capi.device_plane(t) for t in d_img])
        if fused:
            gpu_ctx.improc_denoise_fused(img, tp, O.REC2020_WS_D, demosaiced=p_dem, sx1=4, sy1=4, mul=mul, do_clip=True, cam_to_work=mat,
                                         exposure=(exp_scale, 12.5), ecomp=ecomp, calclum_mat=mat, noise_c_curve=curve, flags=capi.DN_SKIP_DETAIL_RECOVERY)
        else:
            gpu_ctx.get_image(p_dem, 4, 4, mul, True, mat, img)
            gpu_ctx.improc_denoise(img, tp, O.REC2020_WS_D, ecomp=ecomp, calclum_mat=mat, noise_c_curve=curve, flags=capi.DN_SKIP_DETAIL_RECOVERY)
            gpu_ctx.exposure(img, exp_scale, 12.5)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in d_img])
    assert _same(outs[0], outs[1]) == [0, 0, 0]
    assert all(np.isfinite(p).all() for p in outs[0])
    # host planes: nothing can be fused (the tool stages them itself), the neighbours run as separate calls -- same result
    h_img = [np.full((h, w), np.nan, np.float32) for _ in range(3)]
    gpu_ctx.improc_denoise_fused(capi.host_rgb(h_img), tp, O.REC2020_WS_D, demosaiced=capi.host_rgb(dem), sx1=4, sy1=4, mul=mul, do_clip=True, cam_to_work=mat,
                                 exposure=(exp_scale, 12.5), ecomp=ecomp, calclum_mat=mat, noise_c_curve=curve, flags=capi.DN_SKIP_DETAIL_RECOVERY)
    assert _same(h_img, outs[1]) == [0, 0, 0]
    # a crop that leaves the demosaiced planes is an error, not a clamp
    with pytest.raises(capi.ArtGpuError):
        gpu_ctx.improc_denoise_fused(img, tp, O.REC2020_WS_D, demosaiced=p_dem, sx1=9, sy1=4, mul=mul)
    # nothing to denoise at all: both neighbours run as the calls they stand for
    tp0 = capi.DenoiseToolParams(capi.DenoiseParams(0.0, 50.0, 0, 0.0, 0.0, 0.0, 1.7, 0, 0, 0), 0, 3, 0, 80)
    d_img = [torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    gpu_ctx.improc_denoise_fused(img, tp0, O.REC2020_WS_D, demosaiced=p_dem, sx1=4, sy1=4, mul=mul, do_clip=True, cam_to_work=mat, exposure=(exp_scale, 0.0))
    ref = O.exposure(O.convert_color_space(O.get_image(dem, 4, 4, w, h, mul, True), mat), exp_scale, 0.0)
    torch.cuda.synchronize()
    assert _same([t.cpu().numpy() for t in d_img], ref) == [0, 0, 0]


def _fused_call(ctx, dem, w, h, tp, ecomp=0.3):
    """improc_denoise_fused on device planes with getImage + matrix in front and the exposure behind (the arguments of the 300 x 260 case
    above); returns the planes on the host"""
    import torch
    mat = np.array([[0.6325, 0.2312, 0.0921], [0.2198, 0.7712, 0.0090], [0.0166, 0.0713, 0.7514]])
    curve, _ = capi.noise_curve_lut()
    d_dem = [torch.from_numpy(p).cuda() for p in dem]
    d_img = [torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
    ctx.improc_denoise_fused(capi.RGB(*[capi.device_plane(t) for t in d_img]), tp, O.REC2020_WS_D,
                             demosaiced=capi.RGB(*[capi.device_plane(t) for t in d_dem]), sx1=4, sy1=4, mul=(2.1374, 1.0, 1.5918), do_clip=True,
                             cam_to_work=mat, exposure=(float(np.float32(2.0 ** 0.3)), 12.5), ecomp=ecomp, calclum_mat=mat, noise_c_curve=curve,
                             flags=capi.DN_SKIP_DETAIL_RECOVERY)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in d_img]


def test_fusion_does_not_outlive_the_call():
    """What artgpu_improc_denoise_fused fuses into the tool's pixel passes belongs to that one call: after fused calls of both forms (front +
    exposure in rgb2yuv / yuv2rgb; the exposure on the tail pass behind NL-means) and one that fails inside RGB_denoise after the fusion has
    been decided, the plain entry points compute on that context what they compute on a fresh one."""
    w, h = 300, 260                      # the merged one-launch form of the shrink passes
    dem = _rgb(w + 8, h + 8, w)
    img = _rgb(w, h, 7)
    curve, _ = capi.noise_curve_lut()
    rng = np.random.default_rng(0)
    ccalc = (1.0 + 4.0 * rng.uniform(0.01, 0.5, ((h + 1) // 2, (w + 1) // 2))).astype(np.float32) ** 2
    mat = np.array([[0.6325, 0.2312, 0.0921], [0.2198, 0.7712, 0.0090], [0.0166, 0.0713, 0.7514]])

    def plain_calls(ctx):
        a = [p.copy() for p in img]
        ctx.rgb_denoise(capi.host_rgb(a), _params(), O.REC2020_WS, ccalc=capi.host_plane(ccalc))
        m = np.zeros(((h + 1) // 2, (w + 1) // 2), np.float32)
        ctx.denoise_chroma_map(capi.host_rgb(img), mat, O.REC2020_WS_D, curve, capi.host_plane(m))
        c = [p.copy() for p in img]
        ctx.improc_denoise(capi.host_rgb(c), capi.DenoiseToolParams(_params(), 0, 3, 0, 80), O.REC2020_WS_D, ecomp=0.3, calclum_mat=mat,
                           noise_c_curve=curve, flags=capi.DN_SKIP_DETAIL_RECOVERY)
        return a + [m] + c

    used, fresh = capi.Context(0), capi.Context(0)
    try:
        out = _fused_call(used, dem, w, h, capi.DenoiseToolParams(_params(luminance=0.0), 0, 3, 0, 80))
        assert all(np.isfinite(p).all() for p in out)
        out = _fused_call(used, dem, w, h, capi.DenoiseToolParams(_params(), 1, 3, 50, 80))
        assert all(np.isfinite(p).all() for p in out)
        with pytest.raises(capi.ArtGpuError):
            _fused_call(used, dem, w, h, capi.DenoiseToolParams(_params(color_space=2), 0, 3, 0, 80))
        got, ref = plain_calls(used), plain_calls(fresh)
    finally:
        used.close()
        fresh.close()
    assert _same(got, ref) == [0] * 7
    assert ref[3].any() and not any(np.array_equal(r, p) for r, p in zip(ref[:3] + ref[4:], img + img))


def test_one_progress_pair_per_call(gpu_ctx):
    """artgpu.h promises one (name, 0.0) / (name, 1.0) pair per entry point: the fused tool and its host-plane form report
    ImProcFunctions::denoise once around everything else, and the RGB_denoise they run once inside it."""
    w, h = 300, 260
    dem = _rgb(w + 8, h + 8, w)
    curve, _ = capi.noise_curve_lut()
    tp = capi.DenoiseToolParams(_params(), 0, 3, 0, 80)
    host = [p.copy() for p in _rgb(w, h, 7)]
    calls = {
        "fused, device planes": lambda: _fused_call(gpu_ctx, dem, w, h, tp),
        "host planes": lambda: gpu_ctx.improc_denoise(capi.host_rgb(host), tp, O.REC2020_WS_D, ecomp=0.3, noise_c_curve=curve,
                                                      flags=capi.DN_SKIP_DETAIL_RECOVERY),
    }
    for what, call in calls.items():
        events = []
        gpu_ctx.set_progress_callback(lambda stage, frac: events.append((stage, frac)))
        try:
            call()
        finally:
            gpu_ctx.set_progress_callback(None)
        tool, inner = "ImProcFunctions::denoise", "denoise::RGB_denoise"
        assert events[0] == (tool, 0.0) and events[-1] == (tool, 1.0), (what, events)
        for ev in ((tool, 0.0), (tool, 1.0), (inner, 0.0), (inner, 1.0)):
            assert events.count(ev) == 1, (what, ev, events)
        assert 0 < events.index((inner, 0.0)) < events.index((inner, 1.0)) < len(events) - 1, (what, events)


def test_trim_scratch_gives_the_pool_back_and_the_next_call_rebuilds_it():
    """artgpu_trim_scratch (round 5): the context's arenas / staging / pool go back to the driver, the next call grows them again and rebuilds
    the tables that lived there (gamma pair, chroma noise curve table) -- same bits; the fused pass's hand-over ring is a few MB, not a slot
    per strip (round 4 held nsub * nstrips of them)"""
    ctx = capi.Context(0)
    img = _rgb(1000, 760, 11)
    curve, _ = capi.noise_curve_lut()
    tp = capi.DenoiseToolParams(_params(), 0, 3, 0, 80)

    def run():
        got = [p.copy() for p in img]
        ctx.improc_denoise(capi.host_rgb(got), tp, O.REC2020_WS_D, ecomp=0.3, noise_c_curve=curve, flags=capi.DN_SKIP_DETAIL_RECOVERY)
        return got
    first = run()
    held = ctx.scratch_bytes()
    assert held > 20 * 1000 * 760 * 4 // 4                   # planes, three band sets, histograms ...
    # 45 bands x 2 slots x 16 rows x (500 + 15 -> 576 columns) floats = 3.3 MB of hand-over ring: everything the frame needs stays below what
    # the per-strip slots alone took before (45 x 6 strips x 16 x 576 x 4 = 10 MB at this size, 0.5 GB at 45 MP)
    ctx.trim_scratch()
    assert ctx.scratch_bytes() <= 65536 * 4                  # (the tone LUT is not scratch: it stays)
    again = run()
    assert _same(again, first) == [0, 0, 0]
    assert ctx.scratch_bytes() == held
    ctx.trim_scratch()
    ctx.trim_scratch()                                       # (idempotent)
    del ctx


def test_slots_of_the_other_shrink_form_survive_an_alternation_and_go_after_four_calls():
    """round-5 advisor: a context that alternates between the fused and the three-kernel form of the shrink passes (`fused` depends on the frame
    size) must not free and re-allocate band-sized slots per frame.  The other form's slots stay across a switch and are released once four
    calls in a row used the same form; the results are the same bits throughout."""
    ctx = capi.Context(0)
    img = _rgb(1000, 760, 12)
    curve, _ = capi.noise_curve_lut()
    tp = capi.DenoiseToolParams(_params(), 0, 3, 0, 80)

    def run(form):
        ctx.set_option("dn_fused", form)
        got = [p.copy() for p in img]
        ctx.improc_denoise(capi.host_rgb(got), tp, O.REC2020_WS_D, ecomp=0.3, noise_c_curve=curve, flags=capi.DN_SKIP_DETAIL_RECOVERY)
        return got
    ref = run(1)
    fused_only = ctx.scratch_bytes()
    sizes = []
    for form in (0, 1, 0, 1):                               # alternating: both forms' slots are held, nothing is dropped
        assert _same(run(form), ref) == [0, 0, 0]
        sizes.append(ctx.scratch_bytes())
    assert sizes[0] > fused_only and sizes[1:] == [sizes[0]] * 3
    for _ in range(4):
        assert _same(run(0), ref) == [0, 0, 0]
    assert ctx.scratch_bytes() < sizes[0]                   # four three-kernel calls in a row: the fused form's second band set and ring went back
    assert _same(run(1), ref) == [0, 0, 0]                   # ... and come back when asked for
    assert ctx.scratch_bytes() == sizes[0]
    del ctx


def test_fused_shrink_pass_reports_a_strip_that_never_hands_down_instead_of_hanging_or_trapping():
    """round-5 advisor: the bounded wait of the strip wavefront (shrinkblur.hip).  A strip that never publishes its progress (test hook, option
    dn_debug_stall) makes the strip below give up after the bound (option dn_wait_ms: 30 ms here instead of five seconds): the launch ends, the
    process lives, artgpu_synchronize returns an error that names band, strip and block, and the context goes on to produce the right bits."""
    ctx = capi.Context(0)
    img = _rgb(1000, 760, 13)
    curve, _ = capi.noise_curve_lut()
    tp = capi.DenoiseToolParams(_params(), 0, 3, 0, 80)

    def run():
        got = [p.copy() for p in img]
        ctx.improc_denoise(capi.host_rgb(got), tp, O.REC2020_WS_D, ecomp=0.3, noise_c_curve=curve, flags=capi.DN_SKIP_DETAIL_RECOVERY)
        ctx.synchronize()
        return got
    ref = run()
    ctx.set_option("dn_wait_ms", 30)
    ctx.set_option("dn_debug_stall", (4 << 16) | 1)          # band 4, strip 1 of 6 keeps its progress to itself
    with pytest.raises(capi.ArtGpuError) as ei:
        run()
    msg = str(ei.value)
    # (the strips below the waiting one wait too and give up within moments of each other; the first to give up is reported -- normally
    # strip 2, the stalled strip's successor, but the order in which they started to wait is not guaranteed)
    import re
    m = re.search(r"shrink_blur_kernel: band 4 strip (\d+) gave up waiting", msg)
    assert m and 2 <= int(m.group(1)) <= 5, msg
    with pytest.raises(capi.ArtGpuError) as ei2:            # a second faulty frame on the same context is reported again
        run()
    assert "gave up waiting" in str(ei2.value)
    ctx.set_option("dn_debug_stall", -1)
    ctx.set_option("dn_wait_ms", 0)
    assert _same(run(), ref) == [0, 0, 0]                   # reported once per fault, and the context is as good as new
    del ctx


def test_fused_hand_over_ring_under_many_short_strips():
    """round-5 advisor: the two-slot hand-over ring (FS_RING, shrinkblur.hip) reuses its global addresses within a launch -- strip s + 2 reads
    where strip s read -- and relies on `sc1` loads never seeing a stale line.  A tall, narrow frame makes the case as sharp as it gets: 47 strips
    per band that are two blocks long, so a slot is rewritten microseconds after it was read; fresh data in every repetition, and every
    repetition against the three-kernel form (dn_fused 0), bit for bit."""
    ctx = capi.Context(0)
    curve, _ = capi.noise_curve_lut()
    tp = capi.DenoiseToolParams(_params(), 0, 3, 0, 80)
    for rep in range(6):
        img = _rgb(200, 6000, 100 + rep)
        out = []
        for form in (1, 0):
            ctx.set_option("dn_fused", form)
            got = [p.copy() for p in img]
            ctx.improc_denoise(capi.host_rgb(got), tp, O.REC2020_WS_D, ecomp=0.3, noise_c_curve=curve, flags=capi.DN_SKIP_DETAIL_RECOVERY)
            out.append(got)
        assert _same(out[0], out[1]) == [0, 0, 0], rep
    del ctx


def test_large_chroma_noise_map_lds_table_same_bits_as_plain_kernel(gpu_ctx):
    """maps of >= 1 Mpx run calclum + ccalc with the lower 40704 entries of the Lab f() table in LDS (chroma_map_lds_kernel, round 5): values on
    both sides of the split, negative, above 65535 and NaN, with and without the colour matrix -- the bits of the plain kernel and of the oracle"""
    w, h = 2310, 1826                       # map 1155 x 913 = 1.05 Mpx: odd width, a ragged last chunk, rows that do not fill the last batch
    rng = np.random.default_rng(15)
    base = rng.uniform(0, 1, (h, w)).astype(np.float32) ** 2 * 60000.0
    img = [(base * rng.uniform(0.3, 1.4, (h, w))).astype(np.float32) for _ in range(3)]
    img[0][:60] *= 3.0                      # strongly coloured band: cN > 100, X / D50x above the table
    img[1][100:130] = -40.0
    img[2][200:230] = 0.0
    img[0][300, ::7] = np.nan
    mat = np.array([[0.6325, 0.2312, 0.0921], [0.2198, 0.7712, 0.0090], [0.0166, 0.0713, 0.7514]])
    curve, _ = capi.noise_curve_lut()
    for m in (mat, None):
        got = np.zeros(((h + 1) // 2, (w + 1) // 2), np.float32)
        gpu_ctx.denoise_chroma_map(capi.host_rgb(img), m, O.REC2020_WS_D, curve, capi.host_plane(got))
        gpu_ctx.set_option("lut_lds", 0)
        try:
            plain = np.zeros_like(got)
            gpu_ctx.denoise_chroma_map(capi.host_rgb(img), m, O.REC2020_WS_D, curve, capi.host_plane(plain))
        finally:
            gpu_ctx.set_option("lut_lds", 1)
        ref = O.chroma_noise_map(img, m, O.REC2020_WS_D, curve)

        def same(x, y):        # bit for bit; a NaN has to be a NaN (its payload is the host's / the device's own)
            nx, ny = np.isnan(x), np.isnan(y)
            return np.array_equal(nx, ny) and np.array_equal(x.view(np.uint32)[~nx], y.view(np.uint32)[~ny])
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))
        assert same(got, ref)
        assert len(np.unique(ref[np.isfinite(ref)])) > 100
