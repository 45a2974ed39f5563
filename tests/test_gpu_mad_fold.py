"""GPU: MadRgb from the bins the wavelet analysis kernels count while they write the bands (option "dn_mad_fold")
against launch_mad's pass over the bands (option 0) and against the oracle.  Every comparison is bit for bit on the output planes."""
import os
import re
import shutil

import numpy as np
import pytest

import oracle_lib as O
from art_amd import capi, codeobj, synth

pytestmark = pytest.mark.gpu

NB0, NB = 1024, 4096            # kernels.h: MAD_FOLD_NB0 / MAD_FOLD_NB, the bins the level-0 / the Haar analysis kernel counts
SKIP = capi.DN_SKIP_DETAIL_RECOVERY
MAT = np.array([[0.6325, 0.2312, 0.0921], [0.2198, 0.7712, 0.0090], [0.0166, 0.0713, 0.7514]])


def _bits(planes):
    return [p.view(np.uint32) for p in planes]


def _same(a, b):
    return [int((x != y).sum()) for x, y in zip(_bits(a), _bits(b))]


def _params(**kw):
    p = capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


_IMG = {}


def _rgb(w, h):
    if (w, h) not in _IMG:
        raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=w + 3 * h, noise=2048)
        _IMG[(w, h)] = O.amaze(raw, synth.FILTERS_RGGB, 1.0, 4)
    return _IMG[(w, h)]


class _Options:
    """options of the shared context for the length of a with block"""
    DEFAULTS = dict(dn_mad_fold=1, dn_mad_fold_grid=0, dn_fused=1)

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.ctx.set_option(k, self.DEFAULTS[k])


def _denoise(ctx, img, fold, grid=0, fused=1, **kw):
    """rgb_denoise without the DCT stage; returns the planes and (bands settled from the counts, bands left to the full histogram)"""
    got = [p.copy() for p in img]
    with _Options(ctx, dn_mad_fold=fold, dn_mad_fold_grid=grid, dn_fused=fused):
        ctx.rgb_denoise(capi.host_rgb(got), _params(**kw), O.REC2020_WS, flags=SKIP)
        counts = (ctx.get_option("dn_mad_fold_settled"), ctx.get_option("dn_mad_fold_fallback"))
    return got, counts


def _oracle(img, **kw):
    okw = dict(luminance=kw.get("luminance", 40.0), chrominance=kw.get("chrominance", 15.0), gamma=kw.get("gamma", 1.7))
    return O.rgb_denoise(img, O.default_denoise_params(**okw))


def _median_bins(plane, levels):
    """the bin MadRgb's walk stops in (FTblockDN.cc:569-603), for every band of the oracle's decomposition of `plane`"""
    d = O.wavelet_decompose(plane, levels)
    bands, _, _ = O.wavelet_bands(d)
    O.lib().oracle_wavelet_free(d)
    out = []
    for band in bands.reshape(-1, bands.shape[2] * bands.shape[3]):
        with np.errstate(invalid="ignore"):
            bins = np.sort(np.minimum(np.abs(np.trunc(band.astype(np.float64))), 65535.0).astype(np.int64))
        out.append(int(bins[len(bins) // 2 - 1]))          # `while (count < half) count += histo[median++]` ends in the bin of the half-th smallest
    return out


def _uncounted(bins):
    """how many of a channel's bands (level-major) have their median bin above the bins counted"""
    return sum(b >= (NB0 if k < 3 else NB) for k, b in enumerate(bins))


# ---- 1. geometries: ragged bands, w2 % 4 != 0, bands with fewer coefficients than one launch has threads; six levels (a MadRgb launch set per
# channel) and five (one for all three channels)
@pytest.mark.parametrize("w,h", [(640, 480), (517, 389), (258, 130), (130, 900), (642, 482)])
def test_geometries_same_bits_as_the_pass_over_the_bands(gpu_ctx, w, h):
    img = _rgb(w, h)
    for kw in (dict(chrominance=90.0), {}):
        new, (settled, fallback) = _denoise(gpu_ctx, img, 1, **kw)
        old, none = _denoise(gpu_ctx, img, 0, **kw)
        assert _same(new, old) == [0, 0, 0]
        assert _same(new, _oracle(img, **kw)) == [0, 0, 0]
        assert settled + fallback == (54 if kw else 45) and none == (0, 0)
    # the tool around it (chroma noise map, exposure bracketing), full size and preview scale
    curve, _ = capi.noise_curve_lut()
    tp = capi.DenoiseToolParams(_params(chrominance=90.0), 0, 3, 0, 80)
    outs = {}
    for fold in (1, 0):
        with _Options(gpu_ctx, dn_mad_fold=fold):
            for scale in (1.0, 2.0):
                got = [p.copy() for p in img]
                gpu_ctx.improc_denoise(capi.host_rgb(got), tp, O.REC2020_WS_D, ecomp=0.3, scale=scale, calclum_mat=MAT, noise_c_curve=curve, flags=SKIP)
                outs[(fold, scale)] = got
    for scale in (1.0, 2.0):
        assert _same(outs[(1, scale)], outs[(0, scale)]) == [0, 0, 0]
    ref = O.improc_denoise(img, dict(luminance=40.0, chrominance=90.0), calclum_mat=MAT, noise_c_curve=curve, smoothing=False, ecomp=0.3,
                           detail_recovery=False)
    assert _same(outs[(1, 1.0)], ref) == [0, 0, 0]


# ---- 2. the packed 8-bit counters of bins 0 .. 7.  The grid is sized so that a thread counts at most 248 (level 0) / 255 (Haar) values of a
# band before the flush at the kernel's end (kernels.h: mad_fold_*_fits); with two workgroups for the whole band a thread counts many values, all of
# them in one bin (constant image) or nearly all in bins 0 .. 7 (faint noise)
@pytest.mark.parametrize("kind,w,h", [("constant", 1400, 134), ("faint", 1400, 134)])
def test_packed_counters_hold_a_workgroups_whole_share(gpu_ctx, kind, w, h):
    rng = np.random.default_rng(7)
    if kind == "constant":
        img = [np.full((h, w), v, np.float32) for v in (21000.0, 18000.0, 9000.0)]
    else:
        img = [(v + rng.normal(0.0, 3.0, (h, w))).astype(np.float32) for v in (21000.0, 18000.0, 9000.0)]
    old, _ = _denoise(gpu_ctx, img, 0)
    ref = _oracle(img)
    for grid in (0, 2):                 # band 700 x 67: 33 tiles / 46 steps of 1024 -> 17 tiles and 23 steps per workgroup
        new, counts = _denoise(gpu_ctx, img, 1, grid=grid)
        assert _same(new, old) == [0, 0, 0]
        assert _same(new, ref) == [0, 0, 0]
        assert counts == (45, 0)
    # (one workgroup's threads would count more than their 8-bit counters hold: the plan keeps the pass over the bands)
    new, counts = _denoise(gpu_ctx, img, 1, grid=1)
    assert _same(new, old) == [0, 0, 0] and counts == (0, 0)


# ---- 3. fallback: medians above the bins counted take the full histogram
def test_broad_bands_fall_back_to_the_full_histogram(gpu_ctx):
    w, h = 258, 130
    rng = np.random.default_rng(11)
    img = [rng.uniform(0.0, 65535.0, (h, w)).astype(np.float32) for _ in range(3)]
    ref, Lin, _ = O.rgb_denoise(img, O.default_denoise_params(), want_L=True)
    high = _uncounted(_median_bins(Lin, 5))
    assert high >= 1                                        # the frame does what it was chosen for, for the bins chosen
    new, (settled, fallback) = _denoise(gpu_ctx, img, 1)
    old, _ = _denoise(gpu_ctx, img, 0)
    assert _same(new, old) == [0, 0, 0]
    assert _same(new, ref) == [0, 0, 0]
    assert fallback >= high and settled + fallback == 45     # (the L bands the oracle shows, plus whatever chroma bands are as broad)


# ---- 4. boundary: the walk ends in the last bin counted / in the first one that is not
def _gray_noise(w, h, s):
    rng = np.random.default_rng(3)
    return (32768.0 + np.float32(s) * rng.normal(0.0, 1.0, (h, w)).astype(np.float32)).astype(np.float32)


def _gray_L(v):
    # rgb2yuv's L of a gray pixel with gamma 1 and gain 1 (FTblockDN.cc:2084-2128), fp32 step by step
    ws = O.REC2020_WS.astype(np.float32)
    return (v * ws[1, 0] + v * ws[1, 1]) + v * ws[1, 2]


def _scale_for_top_bin(w, h, first, target):
    lo, hi = 1500.0, 60000.0                                 # median |coefficient| of the broadest level-0 band: about a third of sigma
    for _ in range(60):
        s = 0.5 * (lo + hi)
        top = max(_median_bins(_gray_L(_gray_noise(w, h, s)), 5)[first:][:12])
        if top == target:
            return s
        lo, hi = (s, hi) if top < target else (lo, s)
    raise AssertionError(f"no noise scale puts the broadest band's median into bin {target}")


@pytest.mark.parametrize("first,target", [(0, NB0 - 1), (0, NB0), (3, NB - 1), (3, NB)])      # the broadest level-0 band / the broadest Haar band
def test_median_in_the_last_counted_bin_and_in_the_first_uncounted_one(gpu_ctx, first, target):
    w, h = 258, 130
    v = _gray_noise(w, h, _scale_for_top_bin(w, h, first, target))
    img = [v.copy(), v.copy(), v.copy()]                     # gray: the chroma bands are all but zero, only L decides
    ref, Lin, _ = O.rgb_denoise(img, O.default_denoise_params(gamma=1.0), want_L=True)
    assert np.array_equal(Lin.view(np.uint32), _gray_L(v).view(np.uint32))
    bins = _median_bins(Lin, 5)
    assert max(bins[first:]) == target
    new, (settled, fallback) = _denoise(gpu_ctx, img, 1, gamma=1.0)
    old, _ = _denoise(gpu_ctx, img, 0, gamma=1.0)
    assert _same(new, old) == [0, 0, 0]
    assert _same(new, ref) == [0, 0, 0]
    assert (settled, fallback) == (45 - _uncounted(bins), _uncounted(bins))
    assert _uncounted(bins) - _uncounted(bins[:first]) == (0 if target in (NB0 - 1, NB - 1) else 1)


# ---- 5. coefficients no int holds
def test_non_finite_and_huge_samples(gpu_ctx):
    w, h = 384, 320
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=5, noise=2048)
    clean = O.amaze(raw, synth.FILTERS_RGGB, 1.0, 4)
    img = [p.copy() for p in clean]
    img[0][40, 50] = np.inf
    img[1][41, 300] = np.nan
    img[2][200, 60] = -1e30
    new, _ = _denoise(gpu_ctx, img, 1)
    old, _ = _denoise(gpu_ctx, img, 0)
    assert _same(new, old) == [0, 0, 0]
    new, _ = _denoise(gpu_ctx, clean, 1)                     # and the next frame through the context is untouched by it
    old, _ = _denoise(gpu_ctx, clean, 0)
    assert _same(new, old) == [0, 0, 0]


# ---- 6. one context, several sizes in a row: nothing stale from the workgroups' rows
@pytest.mark.parametrize("fused", [1, 0, 2])                # one MadRgb launch set for the three channels / one per channel (both other forms)
def test_sizes_in_a_row_on_one_context(gpu_ctx, fused):
    seq = [(640, 480), (258, 130), (640, 480)]
    for _ in range(2):
        news = [_denoise(gpu_ctx, _rgb(w, h), 1, fused=fused)[0] for w, h in seq]
        assert _same(news[0], news[2]) == [0, 0, 0]
        for (w, h), new in zip(seq[:2], news):
            old, _ = _denoise(gpu_ctx, _rgb(w, h), 0, fused=fused)
            assert _same(new, old) == [0, 0, 0]


# ---- 7. resources of the two counting kernels, from the built library's gfx950 code objects
def test_counting_kernels_neither_spill_nor_use_scratch():
    lib = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "art_amd", "libartgpu.so")
    pytest.importorskip("msgpack")
    if shutil.which("c++filt") is None and shutil.which("llvm-cxxfilt") is None and not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-cxxfilt"):
        pytest.skip("no c++filt to demangle kernel names")
    table = codeobj.kernel_table(lib)
    # level 0: its 34 KB tile and 3 x NB0 counters three times per CU; Haar: two workgroups of 1024 per CU need 64 registers or fewer
    for pattern, vgprs, lds in ((r"wavelet_analysis0_count_kernel", 128, 160 * 1024 // 3), (r"wavelet_haar_analysis_count_kernel", 64, 3 * NB * 4)):
        hits = {n: r for n, r in table.items() if re.search(pattern, n)}
        assert len(hits) == 1, sorted(hits)
        for name, r in hits.items():
            assert r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["scratch_bytes"] == 0, (name, r)
            assert r["vgprs"] <= vgprs and r["static_lds_bytes"] <= lds, (name, r)
