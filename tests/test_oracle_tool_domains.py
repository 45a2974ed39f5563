"""CPU: the twelve local tools behind the colour steps (dehaze, capture sharpening, local contrast, texture boost, region masks, colour
correction, smoothing, tone equalizer, film simulation, film grain, impulse noise reduction, defringe), each through its own CPU checker
(tests/emul/*_ref.cc behind tests/*_lib.py) alone, on the eleven value-domain families of tests/value_domains.py.

tests/test_gpu_tool_domains.py compares the device with these runs in every bit of every value.  That is a statement about the device only where
the checker's output is finite, and it tests what it claims only where the checker's output holds the bits a device gets wrong first: -0.0 on
`negzero` / `mixed_zeros`, subnormals on `tiny`.  Asserted here, step by step, from the checker alone, every figure a literal in this file:

  - NONFINITE: the (step, family) pairs whose output is not finite, with their NaN and +-inf counts -- on `tiny` only: colour correction with a
    pivot in YUV and Jzazbz mode, with rgbluminance under either variant, and local contrast with a curve.  The GPU file compares those NaN for
    NaN, inf by its bits, everything else by its bits;
  - UNCHANGED: the pairs whose output is the input in every bit (the comparison there says nothing about the arithmetic);
  - the count of -0.0 on `negzero` / `mixed_zeros` and of subnormals on `tiny`, per step;
  - that the tool worked where its info says so: impulse and defringe corrected pixels, the sharpening regime, dehaze's haze_detected, a mask
    plane that is neither all 0 nor all 1;
  - colour correction's share of host-powf pixels (the checker's `oor` map), capped per family.

The inputs are test_oracle_value_domains.dn_input(name): the checker's RCD planes of each family at 262 x 198, 65 groups of four columns and a
2-pixel tail per row.  Local contrast takes the L plane of their Lab form, texture_boost_plane their G plane, the LAB-mode mask step their Lab
form.  The cached runs below are shared with the GPU file (one checker run per step and family in a session)."""
import functools
import math

import numpy as np
import pytest

import cc_lib
import dh_lib
import fg_lib
import fs_lib
import id_lib
import lc_lib
import mk_lib
import oracle_lib as O
import sh_lib
import sm_lib
import tb_lib
import te_lib
import value_domains as VD
import test_oracle_value_domains as R

FAMILIES = R.FAMILIES
W, H = R.W, R.H

# step -> (kind, parameters).  The kind is what both this file's run_step and the GPU file's device call dispatch on; the parameters are those of
# a case of the tool's own GPU test, so that the device call is one that test already makes.
STEPS = {
    "dehaze default depth 25": ("dehaze", dict(strength=dh_lib.DEFAULT_STRENGTH, depth=25, luminance=False)),
    "dehaze crossing luminance": ("dehaze", dict(strength=dh_lib.CROSSING_STRENGTH, depth=25, luminance=True)),
    "sharpening defaults": ("sharpen", dict()),
    "sharpening radius 0.9": ("sharpen", dict(deconvradius=0.9)),
    "local contrast 0.5 no curve": ("lc", dict(contrast=0.5, curve=None)),
    "local contrast 60 boost curve": ("lc", dict(contrast=60.0, curve=lc_lib.BOOST_CURVE_POINTS)),
    "texture boost tool": ("tb", dict(regions=[(1.0, 0.2, 1, None)])),
    "texture boost plane 2 iterations": ("tb_plane", dict(strength=1.0, threshold=0.2, iterations=2)),
    "masks rgb three curves ld50 blur 3": ("masks", dict(lab=False, masks=[mk_lib.mask(parametric_enabled=True, hue=mk_lib.HUE_A, chromaticity=mk_lib.CHROMA_A,
                                                                                       lightness=mk_lib.LIGHT_A, lightness_detail=50, blur=3.0)])),
    "masks lab threshold 30": ("masks", dict(lab=True, masks=[mk_lib.mask(parametric_enabled=True, hue=mk_lib.HUE_A, contrast_threshold=30)])),
}
for _m in cc_lib.MODES:
    for _v in ("pivot", "compression"):
        STEPS[f"colour correction {_m} {_v}"] = ("cc", dict(region=dict(cc_lib.MODES[_m], **cc_lib.VARIANTS[_v])))
STEPS.update({
    "smoothing default region": ("sm", dict(region=dict())),           # SmoothingParams::Region's defaults: GUIDED, radius 0 -- the YUV round trip alone
    "smoothing guided LC r3": ("sm", dict(region=dict(mode=sm_lib.GUIDED, channel=sm_lib.LC, radius=3, epsilon=0))),
    "smoothing nlmeans LC 50": ("sm", dict(region=dict(mode=sm_lib.NLMEANS, channel=sm_lib.LC, nlstrength=50))),
    "tone equalizer mixed reg 0": ("te", dict(bands=te_lib.MIXED, regularization=0, pivot=-4.0)),
    "tone equalizer mixed reg 1": ("te", dict(bands=te_lib.MIXED, regularization=1, pivot=-4.0)),
    "tone equalizer mixed reg 4": ("te", dict(bands=te_lib.MIXED, regularization=4, pivot=-4.0)),
    "tone equalizer mixed2 pivot 2.55": ("te", dict(bands=te_lib.MIXED2, regularization=1, pivot=2.55)),
    "film simulation 9 look other profile": ("fs", dict(level=9, kind="look", same_profile=False, strength=1.0)),
    "film simulation 9 look same profile": ("fs", dict(level=9, kind="look", same_profile=True, strength=1.0)),
    "film simulation 64 random 0.35": ("fs", dict(level=64, kind="random", same_profile=False, strength=0.35)),
    "film grain 400/50": ("fg", dict(iso=400, strength=50, color=False)),
    "film grain 400/50 colour": ("fg", dict(iso=400, strength=50, color=True)),
    "impulse 50": ("impulse", dict(thresh=50, scale=1.0)),
    "impulse 80": ("impulse", dict(thresh=80, scale=1.0)),
    "defringe 2.0/13": ("defringe", dict(radius=2.0, threshold=13, scale=1.0)),
    "defringe 5.0/13": ("defringe", dict(radius=5.0, threshold=13, scale=1.0)),
})
STEP_NAMES = list(STEPS)
KIND = {s: STEPS[s][0] for s in STEP_NAMES}
CC_STEPS = [s for s in STEP_NAMES if KIND[s] == "cc"]


def steps_of(*kinds):
    return [s for s in STEP_NAMES if KIND[s] in kinds]


def lc_curve(points):
    return None if points is None else lc_lib.curve_lut(points)


def step_input(step, planes):
    """what the step is handed for the three float32 planes `planes`: the planes, their Lab form (the LAB-mode masks), or one plane of either"""
    kind, kw = STEPS[step]
    if kind == "lc":
        return R._ro([O.image_rgb_to_lab(list(planes))[1]])            # Imagefloat in LAB mode keeps L in its g plane
    if kind == "tb_plane":
        return R._ro([planes[1]])
    if kind == "masks" and kw["lab"]:
        return R._ro(O.image_rgb_to_lab(list(planes)))
    return planes


def run_step(step, img):
    """the checker's output for the step's input `img` -> (planes, info or None, oor map or None).  info is what the tool's own structure
    reduces to through its *_info_fields helper (a tuple, or a list of tuples for the tools with one structure per region)."""
    kind, kw = STEPS[step]
    img = list(img)
    if kind == "dehaze":
        planes, info, _ = dh_lib.dehaze(img, **kw)
        return planes, dh_lib.info_fields(info), None
    if kind == "sharpen":
        planes, info, _ = sh_lib.sharpening(img, **kw)
        return planes, sh_lib.info_fields(info), None
    if kind == "lc":
        plane, info, _ = lc_lib.local_contrast_wavelets(img[0], kw["contrast"], lc_curve(kw["curve"]))
        return [plane], lc_lib.info_fields(info), None
    if kind == "tb":
        planes, info, _ = tb_lib.texture_boost(img, kw["regions"])
        return planes, tb_lib.info_fields(info), None
    if kind == "tb_plane":
        plane, info, _ = tb_lib.texture_boost_plane(img[0], kw["strength"], kw["threshold"], kw["iterations"])
        return [plane], tb_lib.info_fields(info), None
    if kind == "masks":
        rc, L, ab, info, _ = mk_lib.generate(img, mk_lib.MODE_LAB if kw["lab"] else mk_lib.MODE_RGB, kw["masks"], want_L=True, want_ab=True)
        assert rc == 0, (step, rc)
        return list(L) + list(ab), [mk_lib.info_fields(i) for i in info], None
    if kind == "cc":
        planes, info, oor, _ = cc_lib.color_correction(img, [kw["region"]], to_rgb=True)
        return planes, [cc_lib.info_fields(i) for i in info], oor
    if kind == "sm":
        planes, info, _ = sm_lib.smoothing(img, [kw["region"]])
        return planes, [sm_lib.info_fields(i) for i in info], None
    if kind == "te":
        planes, info, _ = te_lib.tone_equalizer(img, te_lib.params(**kw))
        return planes, te_lib.info_fields(info), None
    if kind == "fs":
        planes, _ = fs_lib.film_simulation(img, fs_lib.clut(kw["kind"], kw["level"]), kw["level"], fs_lib.params(kw["strength"], kw["same_profile"]))
        return planes, None, None
    if kind == "fg":
        planes, regs = fg_lib.film_grain(img, **kw)
        return planes, [r[:5] + (int(np.float32(r[5]).view(np.uint32)),) for r in regs], None
    if kind == "impulse":
        planes, info, _ = id_lib.impulse_denoise(img, kw["thresh"], kw["scale"])
        return planes, id_lib.impulse_info_fields(info), None
    if kind == "defringe":
        planes, info, _ = id_lib.defringe(img, kw["radius"], kw["threshold"], scale=kw["scale"])
        return planes, id_lib.defringe_info_fields(info), None
    raise KeyError(step)


@functools.lru_cache(maxsize=None)
def family_input(step, name):
    return step_input(step, R.dn_input(name))


@functools.lru_cache(maxsize=None)
def o_family(step, name):
    """-> (planes, info, oor or None), the arrays read-only"""
    planes, info, oor = run_step(step, family_input(step, name))
    if oor is not None:
        oor.setflags(write=False)
    return R._ro(planes), info, oor


def _count(planes, key):
    return sum(VD.describe(p)[key] for p in planes)


def _nonfinite(planes):
    """(NaN count, +-inf count) over the planes"""
    return sum(int(np.isnan(p).sum()) for p in planes), sum(int(np.isinf(p).sum()) for p in planes)


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


# ---- finite, or listed -----------------------------------------------------------------------------------------------------------------------------

# (step, family) -> (NaN, +-inf) of the checker's 3 x 262 x 198 = 155 628 output values.  Colour correction's pivot divides by it and multiplies
# back in the tool's normalised units; on `tiny` (everything below 6.6e-37 / 65535) the quotients and the YY / Y ratios behind them are 0 / 0 and
# x / 0.  The RGB mode without rgbluminance and the HSL mode never form those ratios.
NONFINITE = {
    ("colour correction yuv pivot", "tiny"): (22407, 133209),
    ("colour correction jzazbz pivot", "tiny"): (155616, 0),
    ("colour correction rgblum pivot", "tiny"): (22407, 133209),
    ("colour correction rgblum compression", "tiny"): (22407, 133209),       # rgbluminance forms YY / Y whatever the variant
    # not a colour-correction pair: with a curve, local_contrast_wavelets divides by the level's sigma and MaxP, which are 0 on a plane whose
    # L is below 1e-30 throughout; all 262 x 198 = 51 876 values of the plane are NaN.  Without a curve (contrast 0.5) the plane stays finite.
    ("local contrast 60 boost curve", "tiny"): (51876, 0),
}


def test_inputs_are_finite():
    for step in STEP_NAMES:
        for name in FAMILIES:
            assert all(np.isfinite(p).all() for p in family_input(step, name)), f"{step} on {name}: the step's input is not finite"


@pytest.mark.parametrize("name", FAMILIES)
def test_checker_is_finite_except_where_recorded(name):
    for step in STEP_NAMES:
        got = _nonfinite(o_family(step, name)[0])
        if got != (0, 0):
            print(f"{step} on {name}: {got[0]} NaN, {got[1]} inf")
        assert got == NONFINITE.get((step, name), (0, 0)), f"{step} on {name}: (NaN, inf) = {got}, recorded {NONFINITE.get((step, name), (0, 0))}"


def test_nonfinite_holds_only_tiny_and_only_two_tools():
    assert all(KIND[s] in ("cc", "lc") and n == "tiny" and sum(c) > 0 for (s, n), c in NONFINITE.items())
    assert [s for s, _ in NONFINITE if KIND[s] == "lc"] == ["local contrast 60 boost curve"]


# ---- does the step do anything ---------------------------------------------------------------------------------------------------------------------

# (step, family) pairs whose output equals the input in every bit.  An all-zero frame comes back as it is from dehaze, tone equalizer, smoothing,
# texture boost, impulse, defringe and sharpening, and also from local contrast, film grain, film simulation with the `look` table (whose first
# entry is 0; the random table's is not) and colour correction in YUV mode without an offset on channel 0; a constant frame from sharpening at its
# default radius and from smoothing with a radius of 0.  The masks write planes of their own and are never in it.  No other family is in it for
# any step.
UNCHANGED = {(s, "all_zero") for s in steps_of("dehaze", "sharpen", "lc", "tb", "tb_plane", "sm", "te", "fg", "impulse", "defringe")} | {
    ("film simulation 9 look other profile", "all_zero"), ("film simulation 9 look same profile", "all_zero"),
    ("colour correction yuv compression", "all_zero"), ("sharpening defaults", "constant"), ("smoothing default region", "constant")}


def unchanged(step, name):
    return _same_bits(o_family(step, name)[0], family_input(step, name))


def test_every_step_changes_every_family_or_is_listed():
    found = {(s, n) for s in STEP_NAMES for n in FAMILIES if unchanged(s, n)}
    print(sorted(found))
    assert found == UNCHANGED, f"unchanged but not listed: {sorted(found - UNCHANGED)}; listed but changed: {sorted(UNCHANGED - found)}"
    assert {n for _, n in UNCHANGED} <= {"all_zero", "constant"}
    assert not (UNCHANGED & set(NONFINITE))


# ---- the sign of a zero, subnormals ------------------------------------------------------------------------------------------------------------------

# step -> -0.0 in the checker's output on (negzero, mixed_zeros), as measured; every step that is not listed has none on either.  2369 is the
# count of -0.0 in the input planes (the RCD border copies them): tone equalizer, sharpening, dehaze in luminance mode and the smoothing round
# trip scale a pixel by a factor and keep its zero's sign; the texture boost plane call is handed the G plane, whose 1190 are kept on `negzero`
# and become +0.0 on `mixed_zeros`.  Everything that leaves through Lab -> RGB, a LUT or a clamp has none.
NEG_ZEROS_OUT = {
    "dehaze crossing luminance": (2369, 2369), "sharpening defaults": (2369, 2369), "sharpening radius 0.9": (2369, 2369),
    "texture boost plane 2 iterations": (1190, 0), "smoothing default region": (2369, 2369), "tone equalizer mixed reg 0": (2369, 2369),
    "tone equalizer mixed reg 1": (2369, 2369), "tone equalizer mixed reg 4": (2369, 2369), "tone equalizer mixed2 pivot 2.55": (2369, 2369),
}
# step -> subnormals in the checker's output on `tiny`, as measured (finite values only where the pair is in NONFINITE); not listed: none.
# Sharpening and the masks return normal values or zeros there, colour correction returns zeros, NaN and inf, the guided and NL-means smoothing
# and the second texture boost iteration flush everything through their 1e-5 / epsilon floors.
SUBNORMALS_OUT_ON_TINY = {
    "dehaze default depth 25": 1592, "dehaze crossing luminance": 967, "local contrast 0.5 no curve": 920, "texture boost tool": 90573,
    "smoothing default region": 967, "tone equalizer mixed reg 0": 339, "tone equalizer mixed reg 1": 339, "tone equalizer mixed reg 4": 339,
    "tone equalizer mixed2 pivot 2.55": 3680, "film simulation 9 look other profile": 20057, "film simulation 9 look same profile": 20852,
    "film grain 400/50": 4119, "impulse 50": 57438, "impulse 80": 57666, "defringe 2.0/13": 57436, "defringe 5.0/13": 57436,
}


@pytest.mark.parametrize("step", STEP_NAMES)
def test_negative_zeros_in_the_checkers_output_are_where_recorded(step):
    want = NEG_ZEROS_OUT.get(step, (0, 0))
    for name, w in zip(("negzero", "mixed_zeros"), want):
        n = _count(o_family(step, name)[0], "neg_zeros")
        print(f"{step} on {name}: {n} negative zeros in the checker's output (recorded {w})")
        assert (n > 0) == (w > 0), f"{step} on {name}: {n} negative zeros, recorded {w}"


@pytest.mark.parametrize("step", STEP_NAMES)
def test_subnormals_in_the_checkers_output_on_tiny_are_where_recorded(step):
    """SSE does not flush subnormals and neither may the device"""
    w = SUBNORMALS_OUT_ON_TINY.get(step, 0)
    n = _count([np.where(np.isfinite(p), p, np.float32(0)) for p in o_family(step, "tiny")[0]], "subnormals")
    print(f"{step} on tiny: {n} subnormals in the checker's output (recorded {w})")
    assert (n > 0) == (w > 0), f"{step} on tiny: {n} subnormals, recorded {w}"


# ---- did the tool work -------------------------------------------------------------------------------------------------------------------------------

# families on which defringe corrects no pixel: chromave, the mean squared chroma difference, underflows to exactly 0 and PF_correct_RT flags
# nothing; the case then pins the Lab round trip and the detection pass only.  Impulse noise reduction flags pixels on every family but all_zero.
DEFRINGE_CORRECTS_NOTHING = {"all_zero", "tiny", "tiny2", "small"}
IMPULSE_FLAGS_NOTHING = {"all_zero"}
SHARPEN_REGIME = {"sharpening defaults": 2, "sharpening radius 0.9": 3}        # 5 x 5 and 7 x 7 kernels; on every family, with no early out
MASKS_WORK_ON = ("scaled_frac", "dark_offset", "zero_and_sat_blocks")


@pytest.mark.parametrize("name", FAMILIES)
def test_tools_work_where_their_info_says_so(name):
    for step in steps_of("impulse"):
        n = o_family(step, name)[1][4]
        assert (n > 0) == (name not in IMPULSE_FLAGS_NOTHING), f"{step} on {name}: impulse_pixels {n}"
    for step in steps_of("defringe"):
        info = o_family(step, name)[1]
        assert info[0] == 0, f"{step} on {name}: early_out {info[0]}"
        assert (info[7] > 0) == (name not in DEFRINGE_CORRECTS_NOTHING), f"{step} on {name}: corrected_pixels {info[7]}"
        assert (info[5] == 0) == (name in DEFRINGE_CORRECTS_NOTHING), f"{step} on {name}: chromave bits {info[5]:#x}"
    for step in steps_of("sharpen"):
        info = o_family(step, name)[1]
        assert info[1] == SHARPEN_REGIME[step] and info[2] == 0, f"{step} on {name}: regime {info[1]} early_out {info[2]}"
    for step in steps_of("dehaze"):
        info = o_family(step, name)[1]
        assert info[0] == 1 and info[1] == 2, f"{step} on {name}: haze_detected {info[0]} patchsize {info[1]}"       # no early out on any family, all_zero included


@pytest.mark.parametrize("step", steps_of("masks"))
def test_masks_are_neither_all_zero_nor_all_one(step):
    for name in MASKS_WORK_ON:
        for k, p in enumerate(o_family(step, name)[0]):
            assert 0.0 <= p.min() < p.max() <= 1.0 and p.max() > 0.03, f"{step} on {name}: plane {k} spans {p.min()} .. {p.max()}"


# ---- colour correction's powf pixels -------------------------------------------------------------------------------------------------------------------

# (step, family) -> the share of pixels on the checker's `oor` map (Jzazbz values outside the PQ tables: the host's powf), as measured; not
# listed: none.  `huge` under a pivot is out of range in all but 15 of 51 876 pixels: that case pins the 15 and bounds the rest.
OOR_SHARE = {
    ("colour correction jzazbz pivot", "scaled_frac"): 0.01982, ("colour correction jzazbz pivot", "zero_and_sat_blocks"): 0.08114,
    ("colour correction jzazbz pivot", "negzero"): 0.01255, ("colour correction jzazbz pivot", "huge"): 0.9999,
    ("colour correction jzazbz pivot", "mixed_zeros"): 0.00973, ("colour correction jzazbz compression", "scaled_frac"): 0.0001,
    ("colour correction jzazbz compression", "negzero"): 0.03512, ("colour correction jzazbz compression", "huge"): 0.15338,
    ("colour correction jzazbz compression", "mixed_zeros"): 0.07919,
}


def oor_cap(step, name):
    """the measured share rounded up to the next 0.01; 0 where the checker has no such pixel"""
    s = OOR_SHARE.get((step, name), 0.0)
    return math.ceil(s * 100.0 - 1e-9) / 100.0


@pytest.mark.parametrize("step", CC_STEPS)
def test_colour_correction_out_of_range_share_is_capped(step):
    for name in FAMILIES:
        oor = o_family(step, name)[2]
        print(f"{step} on {name}: out-of-range share {oor.mean():.5f}, cap {oor_cap(step, name)}")
        assert oor.mean() <= oor_cap(step, name)
        assert oor.any() == ((step, name) in OOR_SHARE)
        if (step, name) in NONFINITE:
            assert not oor.any()            # the non-finite pairs are compared in bits throughout


# ---- texture boost's minimum -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["negzero", "mixed_zeros"])
def test_texture_boost_minimum_is_the_first_zero_in_raster_order(name):
    """iptextureboost.cc:92 / :99 fold min(minval, v...) over the plane in raster order and rt_math.h:54-58 keeps its first operand when the two
    compare equal: of the zeros of both signs that share the minimum, the first in raster order is `minval` (and what every pixel that
    `minval` wins is given).  On `mixed_zeros` that is a +0.0 although the plane holds 1190 -0.0; a reduction tree's own order gave -0.0."""
    step = "texture boost plane 2 iterations"
    plane = family_input(step, name)[0]
    assert plane.min() == 0.0 and _count([plane], "neg_zeros") == 1190
    first = plane.ravel()[int(np.argmax(plane.ravel() == 0))]
    minval_bits = o_family(step, name)[1][6]
    assert minval_bits == int((first / np.float32(65535.0)).astype(np.float32).view(np.uint32))
    assert minval_bits == {"negzero": 0x80000000, "mixed_zeros": 0}[name]
