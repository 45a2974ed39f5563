"""CPU: the value-domain families of tests/value_domains.py through the checker alone.

tests/test_gpu_value_domains.py compares the device with the checker in every bit of every pixel, with no NaN mask and nothing excluded.
That is only meaningful if the checker's own output is finite on every family, and only tests what it claims if the checker's output really
holds the bits a device can get wrong unnoticed: -0.0 on `negzero`, subnormals on `tiny`.  Both are asserted here, together with the
properties the families are named for and which families send the raw CA correction into its second pass.  `mixed_zeros` (zeros of both
signs side by side) and `small` (values up to 1e-9, whose fifth powers -- the shrink update -- are subnormal) get the same assertions.

The cached stage functions below are shared with the GPU file (one checker run per stage, family and size in a session)."""
import functools

import numpy as np
import pytest

import ca_lib
import oracle_lib as O
import value_domains as VD
from art_amd import synth

W, H, FILT = 262, 198, synth.FILTERS_GRBG          # more than one AMaZE tile, more than one RCD tile wide, sliver tiles
CA_W, CA_H = 700, 500                              # the smallest size here at which CA pass two runs
MAT = np.array([[0.6325, 0.2312, 0.0921], [0.2198, 0.7712, 0.0090], [0.0166, 0.0713, 0.7514]])
DN_MUL = (2.1, 1.0, 1.55)
CA_MODES = {"auto2": dict(autocorrect=True, iterations=2), "manual": dict(autocorrect=False, iterations=1, red=0.7, blue=-0.6)}
# which families run CA pass two at 700 x 500 GRBG, automatic, 2 iterations (the flat and the dark ones stop after pass one)
CA_PASS_TWO = {"dark_offset": False, "scaled_frac": True, "zero_and_sat_blocks": True, "all_zero": False, "constant": False, "tiny": False,
               "tiny2": False, "negzero": True, "huge": True, "mixed_zeros": True, "small": False}
FAMILIES = list(VD.NAMES)


def _ro(planes):
    planes = tuple(np.ascontiguousarray(p) for p in planes)
    for p in planes:
        p.setflags(write=False)
    return planes


def xtrans_map(roll=(0, 0)):
    return np.roll(np.roll(synth.XTRANS_FUJI, roll[0], axis=0), roll[1], axis=1)


@functools.lru_cache(maxsize=None)
def frame(name, w=W, h=H, filters=FILT, roll=None):
    f = VD.family(name, w, h, filters, None if roll is None else xtrans_map(roll))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def o_amaze(name, w=W, h=H, filters=FILT, gain=1.0):
    return _ro(O.amaze(frame(name, w, h, filters), filters, gain, 4))


@functools.lru_cache(maxsize=None)
def o_rcd(name, w=W, h=H, filters=FILT):
    return _ro(O.rcd(frame(name, w, h, filters), filters))


@functools.lru_cache(maxsize=None)
def o_vng4(name, w=W, h=H, filters=FILT):
    return _ro(O.vng4(frame(name, w, h, filters), filters))


@functools.lru_cache(maxsize=None)
def o_xtrans(name, passes, lab, roll=(0, 0)):
    return _ro(O.xtrans_demosaic(frame(name, W, H, 0, roll), xtrans_map(roll), synth.XTRANS_RGB_CAM, passes, lab))


@functools.lru_cache(maxsize=None)
def o_dual(name, method, contrast=None):
    """VNG4 second, contrast None: automatic -> (planes, contrast)"""
    first = o_rcd(name) if method == "rcd" else o_amaze(name)
    planes, c = O.dual_demosaic_blend(frame(name), list(first), FILT, contrast or 0.0, contrast is None, vng4=True)
    return _ro(planes), c


@functools.lru_cache(maxsize=None)
def o_ca(name, mode="auto2", guard=True):
    raw, fit, info = ca_lib.ca_correct(frame(name, CA_W, CA_H), FILT, avoid_colour_shift=guard, want_info=True, **CA_MODES[mode])
    raw.setflags(write=False)
    return raw, fit, info


@functools.lru_cache(maxsize=None)
def dn_input(name, w=W, h=H, crop_h=None):
    """what rgb_denoise is handed: the checker's RCD planes of the family (optionally only the first crop_h rows)"""
    return _ro([p[:crop_h] if crop_h else p for p in o_rcd(name, w, h)])


@functools.lru_cache(maxsize=None)
def o_rgb_denoise(name, w=W, h=H, crop_h=None, lum=40.0, chrom=15.0, detail=False, lum_detail=50.0):
    return _ro(O.rgb_denoise(list(dn_input(name, w, h, crop_h)), O.default_denoise_params(luminance=lum, chrominance=chrom, luminanceDetail=lum_detail),
                             detail_recovery=detail))


@functools.lru_cache(maxsize=None)
def o_guided(name):
    """denoise's guided smoothing straight on the checker's RCD planes (after rgb_denoise nothing subnormal is left on `tiny`)"""
    return _ro(O.guided_smoothing(list(dn_input(name)), O.REC2020_WS_D, 3, 1.0))


@functools.lru_cache(maxsize=None)
def o_improc(name):
    """the denoise tool: chroma noise map, guided smoothing radius 3, NL-means 50 / 80, ecomp 0.3, DCT skipped"""
    return _ro(O.improc_denoise(list(dn_input(name)), calclum_mat=MAT, noise_c_curve=O.noise_curve()[0], smoothing=True, radius=3, nl_strength=50,
                                nl_detail=80, ecomp=0.3, detail_recovery=False))


@functools.lru_cache(maxsize=None)
def o_dninfo(name):
    return O.denoise_compute_params(list(dn_input(name)), 4, DN_MUL, True, MAT, O.REC2020_WS_D, 1.7, False)


def _finite(planes, what):
    for k, p in enumerate(planes):
        assert np.isfinite(p).all(), f"{what}: plane {k} of the checker's output is not finite: {VD.describe(p)}"


def _count(planes, key):
    return sum(VD.describe(p)[key] for p in planes)


def test_families_have_the_properties_they_are_named_for():
    fam = dict(VD.families(W, H, FILT))
    assert list(fam) == FAMILIES
    d = {k: VD.describe(v) for k, v in fam.items()}
    for k, v in fam.items():
        assert v.dtype == np.float32 and v.shape == (H, W) and np.isfinite(v).all(), k
        print(k, d[k])
    n = W * H
    base = VD.describe(VD.base_frame(W, H, FILT))
    assert base["negatives"] == base["non_integers"] == base["neg_zeros"] == base["subnormals"] == 0 and base["max"] <= 65535.0
    assert 0.5 * n < d["dark_offset"]["negatives"] < 0.75 * n and d["dark_offset"]["non_integers"] > 0.9 * n
    assert max(abs(d["dark_offset"]["min"]), d["dark_offset"]["max"]) < 600.0
    assert d["scaled_frac"]["non_integers"] > 0.9 * n and 0 < d["scaled_frac"]["negatives"] < 0.05 * n and 80000.0 < d["scaled_frac"]["max"] < 90000.0
    z = fam["zero_and_sat_blocks"]
    assert (z[H // 4:H // 2, W // 4:W // 2] == 0).all() and (z[H // 2:3 * H // 4, W // 2:3 * W // 4] == 65535.0).all()
    assert (H // 2 - H // 4) > 40 and (W // 2 - W // 4) > 40             # wider than any stage's reach (AMaZE 16, RCD 9, X-Trans 11, CA 8)
    assert (W // 4) % 16 and (H // 4) % 16 and (W // 2) % 16 and (H // 2) % 16        # off the tile grids
    assert d["all_zero"]["zeros"] == n and d["all_zero"]["neg_zeros"] == 0
    assert d["constant"]["min"] == d["constant"]["max"] == 12345.0
    # 1e-41 x [0, 65535]: everything is below 6.6e-37, the dark end (below 1176) is subnormal itself and every difference, eps-guarded
    # ratio and product of two such values is subnormal or underflows
    assert d["tiny"]["subnormals"] > 100 and d["tiny"]["max"] < 1e-36 and d["tiny"]["negatives"] == 0
    t2 = fam["tiny2"]
    # normal values; the square of anything below 36 142 x 3e-24 is below 2^-126 (most of the frame), every product of three is zero
    assert d["tiny2"]["subnormals"] == 0 and (np.square(t2) < np.finfo(np.float32).tiny).sum() > 0.5 * n and not (t2 * t2 * t2).any()
    assert 0.25 * n < d["negzero"]["neg_zeros"] < 0.35 * n and d["negzero"]["max"] == 65535.0
    mz = fam["mixed_zeros"]
    assert 0.25 * n < d["mixed_zeros"]["neg_zeros"] < 0.35 * n and 0.25 * n < d["mixed_zeros"]["zeros"] - d["mixed_zeros"]["neg_zeros"] < 0.35 * n
    both = (mz[:, :-1] == 0) & (mz[:, 1:] == 0) & (np.signbit(mz[:, :-1]) != np.signbit(mz[:, 1:]))
    assert both.sum() > 0.02 * n                 # +0 next to -0 in a row, thousands of times
    sm = fam["small"]
    assert d["small"]["subnormals"] == 0 and d["small"]["max"] < 1e-9 and (np.square(sm[sm > 0]) > np.finfo(np.float32).tiny).all()
    assert (sm.astype(np.float64) ** 5 < np.finfo(np.float32).tiny).all()       # c x sf^2 with sf ~ c^2 / eps: what the shrink update multiplies
    assert d["huge"]["max"] > 6.5e10 and float(np.float32(d["huge"]["max"]) * np.float32(d["huge"]["max"])) > 1e21


@pytest.mark.parametrize("name", FAMILIES)
def test_checker_is_finite_on_every_stage(name):
    _finite(o_amaze(name), "amaze")
    _finite(o_rcd(name), "rcd")
    _finite(o_vng4(name), "vng4")
    _finite(o_xtrans(name, 1, False), "xtrans 1 pass")
    _finite(o_xtrans(name, 3, True), "xtrans 3 passes CIELab")
    for method in ("amaze", "rcd"):
        planes, c = o_dual(name, method)
        _finite(planes, f"dual {method}")
        assert np.isfinite(c)
    _finite(o_dual(name, "amaze", 20.0)[0], "dual amaze, contrast 20")
    for lum, chrom in ((40.0, 15.0), (0.0, 60.0)):
        _finite(o_rgb_denoise(name, lum=lum, chrom=chrom), f"rgb_denoise {lum}/{chrom}")
    _finite(o_rgb_denoise(name, detail=True), "rgb_denoise with detail recovery")
    _finite(o_guided(name), "guided_smoothing")
    _finite(O.nlmeans(o_guided(name)[1]), "nlmeans")
    _finite(o_improc(name), "improc_denoise")
    ref = o_dninfo(name)
    assert ref is not None
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    if name in ("scaled_frac", "zero_and_sat_blocks"):
        _finite(o_amaze(name, gain=2.1), "amaze gain 2.1")


@pytest.mark.parametrize("name", FAMILIES)
def test_checker_ca_is_finite_and_pass_two_is_as_recorded(name):
    raw, fit, info = o_ca(name)
    assert np.isfinite(raw).all() and np.isfinite(fit).all()
    assert info["processpasstwo"] == CA_PASS_TWO[name], info
    if not CA_PASS_TWO[name]:
        assert info["iterations_run"] == 1


def test_checker_output_holds_negative_zeros_on_negzero():
    """otherwise the GPU comparison on `negzero` would not be about the sign of a zero"""
    counts = {"rcd": _count(o_rcd("negzero"), "neg_zeros"), "vng4": _count(o_vng4("negzero"), "neg_zeros"),
              "xtrans": _count(o_xtrans("negzero", 3, True), "neg_zeros"), "dual": _count(o_dual("negzero", "rcd")[0], "neg_zeros"),
              "ca": VD.describe(o_ca("negzero")[0])["neg_zeros"]}
    print(counts)
    assert all(v > 1000 for v in counts.values()), counts


def test_checker_output_holds_subnormals_on_tiny():
    counts = {"amaze": _count(o_amaze("tiny"), "subnormals"), "rcd": _count(o_rcd("tiny"), "subnormals"), "vng4": _count(o_vng4("tiny"), "subnormals"),
              "xtrans": _count(o_xtrans("tiny", 3, True), "subnormals"), "guided": _count(o_guided("tiny"), "subnormals")}
    print(counts)
    assert all(v > 500 for v in counts.values()), counts
