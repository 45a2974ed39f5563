"""CPU: the colour-correction checker (tests/cc_lib.py, tests/emul/colorcorrection_ref.cc) -- that the cases of test_gpu_colorcorrection.py
reach every branch of the tool, that the scenes meet the conditions the GPU comparison relies on, the ABI, an independent float64 model of
the RGB chain, and two properties of the reference's 4-wide body."""
import ctypes as C
import os
import subprocess

import numpy as np

import cc_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cases_reach_every_branch():
    total = {n: 0 for n in cc_lib.COUNTERS}
    for name in cc_lib.CASES:
        for k, v in cc_lib.case(name)[6].items():
            total[k] += v
    print("colour-correction checker, counters over all cases:", total)
    # groups activated with a zero-blend lane, tail pixels skipped, pixels per mode, the hue shift per form, pivot != 1, compression in its
    # vector-clamp and scalar-zero forms (and taken), gamma, the rgbluminance branch, Y <= 0 in the rescale, v <= 0 in the chain, PQ low / high
    for k in cc_lib.COUNTERS:
        assert total[k] > 0, k
    # and single cases take what their names say
    c = lambda n: cc_lib.case(n)[6]
    assert c("3x5-tail-only")["groups_zero_lane"] == 0 and c("3x5-tail-only")["tail_skipped"] > 0
    assert c("4x3-one-group")["tail_skipped"] == 0 and c("4x3-one-group")["groups_zero_lane"] == 3
    assert c("67x45-onelane")["groups_zero_lane"] == 3 * 45 * 16                 # every group of every row, in all three regions
    assert c("67x45-hsl-g1")["gamma"] == 0 and c("67x45-hsl-g2.4")["gamma"] > 0
    assert c("67x45-jzazbz-defaults")["px_jzazbz"] > 0 and c("67x45-jzazbz-defaults")["pq_low"] > 0      # defaults still do the Jzazbz round trip
    assert c("67x45-hsl-hue+30")["hue_hsl"] > 0 and c("67x45-yuv-hue-30")["hue_yuv"] > 0 and c("67x45-jzazbz-hue+30")["hue_jzazbz"] > 0
    assert c("67x45-rgblum-sop")["rgbluminance"] > 0 and c("67x45-rgb-sop")["rgbluminance"] == 0
    assert c("67x45-rgb-compression")["compression_vector_clamp"] > 0 and c("67x45-onelane")["compression_scalar_zero"] > 0


def test_scenes_meet_the_comparisons_conditions():
    """scenes without a super-white block have an EMPTY powf map (so every pixel is compared in bits); the one super-white case has some, below a
    quarter of the image; Info's count is the map's"""
    for name, spec in cc_lib.CASES.items():
        _, _, _, _, info, oor, _ = cc_lib.case(name)
        if spec[5]:
            assert 0 < oor.sum() < 0.25 * oor.size, (name, int(oor.sum()))
        else:
            assert not oor.any(), (name, int(oor.sum()))
        assert all(int(i.oor_pixels) == int(oor.sum()) for i in info)
    # the scene carries what the issue lists
    img = cc_lib.scene(67, 45, seed=3)
    assert np.isnan(img[0][cc_lib.NAN_BODY]) and cc_lib.NAN_BODY[1] < 64 and np.isnan(img[1][cc_lib.NAN_TAIL_ROW, 66])
    assert any((a < 0).any() for a in img) and (img[1] == 0).any() and np.signbit(img[1][img[1] == 0]).any() and not np.signbit(img[1][img[1] == 0]).all()
    one = cc_lib.mask("onelane", 67, 45)
    # the NaNs lie under a zero blend of an active group (body) / a skipped pixel (tail) in the one-lane mask, under 1.f without a mask
    assert one[cc_lib.NAN_BODY] == 0 and one[cc_lib.NAN_BODY[0], 20:24].max() > 0 and one[cc_lib.NAN_TAIL_ROW, 66] == 0
    assert ((one[:, :64].reshape(45, 16, 4) > 0).sum(axis=2) == 1).all(), "exactly one non-zero lane per group"


def test_nan_pixels_stay_single_pixels():
    """the tool is pointwise: the NaN of a body column under a zero blend of an active group, and the one of a skipped tail pixel, are NaN
    in the output and their neighbours are finite"""
    want = cc_lib.case("67x45-onelane")[3]
    y, x = cc_lib.NAN_BODY
    assert all(np.isnan(p[y, x]) and np.isfinite(p[y, x + 1]) and np.isfinite(p[y, x - 1]) for p in want)
    assert all(np.isnan(p[cc_lib.NAN_TAIL_ROW, 66]) and np.isfinite(p[cc_lib.NAN_TAIL_ROW, 65]) for p in want)


def test_abi_of_the_new_structures(tmp_path):
    from art_amd import capi
    for sym in ("artgpu_color_correction", "artgpu_set_pipeline_color_correction"):
        assert sym in capi.EXPORTS and hasattr(capi.LIB, sym), sym
    rf = [n for n, _ in capi.ColorCorrectionRegion._fields_]
    nf = [n for n, _ in capi.ColorCorrectionInfo._fields_]
    exprs = (["sizeof(artgpu_color_correction_region)"] + [f"offsetof(artgpu_color_correction_region, {n})" for n in rf] +
             ["sizeof(artgpu_color_correction_info)"] + [f"offsetof(artgpu_color_correction_info, {n})" for n in nf] +
             ["sizeof(artgpu_pipeline_params)", "ARTGPU_CC_YUV", "ARTGPU_CC_RGB", "ARTGPU_CC_HSL", "ARTGPU_CC_JZAZBZ", "ARTGPU_CC_LUT"])
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "artgpu.h"\nint main(void){' +
                     "".join(f'printf("%zu\\n", (size_t)({e}));' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = ([C.sizeof(capi.ColorCorrectionRegion)] + [getattr(capi.ColorCorrectionRegion, n).offset for n in rf] +
            [C.sizeof(capi.ColorCorrectionInfo)] + [getattr(capi.ColorCorrectionInfo, n).offset for n in nf] +
            [C.sizeof(capi.PipelineParams), capi.CC_YUV, capi.CC_RGB, capi.CC_HSL, capi.CC_JZAZBZ, capi.CC_LUT])
    assert got == want, list(zip(exprs, got, want))
    # the checker's structures are the library's
    assert C.sizeof(cc_lib.Region) == C.sizeof(capi.ColorCorrectionRegion) and C.sizeof(cc_lib.Info) == C.sizeof(capi.ColorCorrectionInfo)
    assert [(n, getattr(cc_lib.Region, n).offset) for n, _ in cc_lib.Region._fields_] == [(n, getattr(capi.ColorCorrectionRegion, n).offset) for n in rf]
    assert [(n, getattr(cc_lib.Info, n).offset) for n, _ in cc_lib.Info._fields_] == [(n, getattr(capi.ColorCorrectionInfo, n).offset) for n in nf]
    assert (cc_lib.YUV, cc_lib.RGB, cc_lib.HSL, cc_lib.JZAZBZ, cc_lib.LUT) == (capi.CC_YUV, capi.CC_RGB, capi.CC_HSL, capi.CC_JZAZBZ, capi.CC_LUT)


# The checker's largest deviation from the float64 model below, relative to max(|model|, 1.0) (one unit of the 0 .. 65535 scale, so that the
# exact zeros of the chain have a denominator), measured on this scene over the three cases: 1.988291973248124e-03 (the compression case; it is
# the absolute rounding of the float YUV round trip, ~0.002 units at |Y| ~ 4e4, seen against outputs of about one unit in the near-black
# block -- pow_F's own error is ~1e-6).  The bound is twice that.  A restatement error (a missing pivot, offset instead of offset / 2, power
# instead of 1 / power) moves whole regions by percent.
MODEL_MEASURED = 1.988291973248124e-03
MODEL_BOUND = 2.0 * MODEL_MEASURED


def _model(img, r):
    """slope / offset / power / pivot / compression on RGB, in float64, per channel, without masks and without the 4-wide subtleties (its
    compression form gives log(1) / c1 = 0 where the scalar one writes 0)"""
    out = []
    for c in range(3):
        s, o, pw, pv, cp = (cc_lib.triple(r.get(k, d))[c] for k, d in (("slope", 1.0), ("offset", 0.0), ("power", 1.0), ("pivot", 1.0), ("compression", 0.0)))
        x = np.asarray(img[c], np.float64) / 65535.0 * s + o / 2.0
        p = 1.0 / pw
        pos = x > 0
        t = np.where(pos, np.power(np.where(pos, x, 1.0) / pv, p) * pv, 0.0)
        if cp > 0:
            c0 = cp * 100.0
            y0 = ((s + o) / pv) ** p * pv
            t = np.log(1.0 + t * c0) / (np.log(1.0 + y0 * c0) / s)
        out.append(t * 65535.0)
    return out


def test_rgb_chain_against_a_float64_model():
    img = cc_lib.scene(67, 45, seed=3, nans=False)
    worst = 0.0
    for name in ("sop", "pivot", "compression"):
        want = cc_lib.color_correction(img, [dict(mode=cc_lib.RGB, **cc_lib.VARIANTS[name])], to_rgb=True)[0]
        dev = max(float((np.abs(w - m) / np.maximum(np.abs(m), 1.0)).max()) for w, m in zip(want, _model(img, cc_lib.VARIANTS[name])))
        print(f"colour-correction checker against the float64 model, {name}: largest relative deviation {dev:.6e} (bound {MODEL_BOUND:.6e})")
        worst = max(worst, dev)
    assert worst <= MODEL_BOUND


def test_zero_mask_on_a_tail_only_image_is_the_yuv_round_trip():
    img = cc_lib.scene(3, 5, seed=11)
    zero = cc_lib.mask("zero", 3, 5)
    for to_rgb in (False, True):
        got, _, _, cn = cc_lib.color_correction(img, [dict(mode=cc_lib.JZAZBZ, lmask=zero, abmask=zero, **cc_lib.SOP)], to_rgb=to_rgb)
        plain = cc_lib.color_correction(img, [], to_rgb=to_rgb)[0]
        assert cn["tail_skipped"] == 15 and cn["px_jzazbz"] == 0
        assert all(np.array_equal(cc_lib.bits(g), cc_lib.bits(p)) for g, p in zip(got, plain))


def test_zero_blend_lane_of_an_active_group_turns_minus_zero_into_plus_zero():
    """4 x 1, all channels -0.f: Y is -0.f after the switch (u = Y - b and v = r - Y are +0.f).  With a zero mask everywhere the group is not
    entered and Y stays -0.f; with one other lane active the zero-blend lanes get intp(0.f, new, -0.f) = 0.f * new + 1.f * -0.f with new > 0
    (the offset lifts it): +0.f"""
    img = [np.full((1, 4), -0.0, np.float32) for _ in range(3)]
    img[0][0, 3] = img[1][0, 3] = img[2][0, 3] = 5000.0
    region = dict(mode=cc_lib.YUV, slope=1.1, offset=0.1)
    zero = np.zeros((1, 4), np.float32)
    one = zero.copy(); one[0, 3] = 1.0
    idle = cc_lib.color_correction(img, [dict(region, lmask=zero, abmask=zero)])[0]
    live = cc_lib.color_correction(img, [dict(region, lmask=one, abmask=one)])[0]
    assert (cc_lib.bits(idle[1][0, :3]) == 0x80000000).all() and (cc_lib.bits(live[1][0, :3]) == 0).all(), (idle[1], live[1])
    # a tail pixel with a zero mask next to an active one keeps its -0.f (W = 3: no group)
    img3 = [a[:, 1:].copy() for a in img]
    tail = cc_lib.color_correction(img3, [dict(region, lmask=one[:, 1:], abmask=one[:, 1:])])[0]
    assert (cc_lib.bits(tail[1][0, :2]) == 0x80000000).all()
