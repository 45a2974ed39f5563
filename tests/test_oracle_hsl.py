"""CPU: oracle/hsl.c and the saturation / vibrance oracle (oracle/pixelops.c) against float64 models that share no code with them.

Both oracles were pinned by reading only.  The models below are written from the reference text -- rtengine/iphsl.cc:92-221, color.cc's yuv2hsl /
hsl2yuv and imagefloat.cc's rgb_to_yuv / yuv_to_rgb for HSL, ipsaturation.cc:30-83 for saturation / vibrance -- in numpy float64, with numpy's own
arctan2, hypot, sin, cos and power instead of the sleef forms, and whole-array expressions instead of pixel loops.

What the HSL model takes from the oracle side are the FlatCurves: O.flat_curve_sample at 2^20 + 1 points, linearly interpolated (a polyline of
~1000 points per unit sampled 1000 times as densely).  The curve construction is pinned by tests/test_noise_curve.py; what this model checks is
the pixel arithmetic around it: Y / u / v from the working-space row, atan2 / hypot, hue01, the three steps in the reference's order (saturation,
luminance, hue), tolin with bases 2, 10 and 32, the exponent 1 + (f < 0 ? c : 1 - c) from the fixed coefficient curve, sin / cos back and the
to_rgb solve for G.  Smoothing is 0: the guided filter has its own tests."""
import functools

import numpy as np
import pytest

import hsl_lib
import oracle_lib as O
from test_gpu_hsl import H_CURVE, L_CURVE, S_CURVE, scene

CURVE_SAMPLES = (1 << 20) + 1
COEFF_POINTS = (1, 0.25, 0.0, 0.5, 0.18, 1, 1, 0, 0.35)              # iphsl.cc:126-130
SCENES = [("smooth", 420, 300), ("wild", 421, 301), ("wild", 37, 29)]
SATVIB = [(35, 40), (-20, -60)]


@functools.lru_cache(maxsize=None)
def _scene(kind, w, h):
    img = scene(w, h, w) if kind == "smooth" else hsl_lib.wild_scene(w, h, w)
    for p in img:
        p.setflags(write=False)
    return tuple(img)


@functools.lru_cache(maxsize=None)
def _curve(points):
    """-> (samples over [0, 1], is identity); periodic with period 1"""
    if points is None:
        return None, True
    v, ident = O.flat_curve_sample(points, True, 1000, 0.5, CURVE_SAMPLES)
    return v, ident


def _curve_val(points, t):
    v, _ = _curve(points)
    t = np.mod(t, 1.0)
    return np.interp(t, np.linspace(0.0, 1.0, CURVE_SAMPLES), v)


def _hue01(h):
    v = h / (2.0 * np.pi)
    return np.where(v < 0.0, 1.0 + v, np.where(v > 1.0, v - 1.0, v))


def _tolin(y, base):
    v = (y - 0.5) * 2.0
    return np.sign(v) * np.clip((np.power(base, np.abs(v)) - 1.0) / (base - 1.0), 0.0, 1.0)


def hsl_model(img, hcurve, scurve, lcurve, to_rgb, hue_first=False):
    """hslEqualizer with smoothing 0 in float64 -> three planes in the reference's slots (RGB, or v, Y, u in YUV mode).  hue_first: a deliberately
    wrong order (the hue step ahead of the other two, whose masks then see the shifted hue) for the test that the bound tells it apart."""
    ws1 = np.asarray(O.REC2020_WS_D, np.float64).reshape(3, 3)[1].astype(np.float32).astype(np.float64)     # Imagefloat keeps the row as floats
    r, g, b = (np.asarray(p, np.float64) for p in img)
    Y = r * ws1[0] + g * ws1[1] + b * ws1[2]                  # rgb_to_yuv
    u, v = Y - b, r - Y
    Y, u, v = Y / 65535.0, u / 65535.0, v / 65535.0           # normalizeFloatTo1
    s, h = np.hypot(u, v), np.arctan2(u, v)                   # yuv2hsl
    hue = _hue01(h)                                           # all three masks are taken from the hue as it comes in (the hue step is the last)
    assert s.max() < 1.25                                     # the coefficient curve is evaluated by its period below
    if hue_first and not _curve(hcurve)[1]:
        h = h + _tolin(_curve_val(hcurve, hue), 32.0) * np.pi
        hue = _hue01(h)
    if not _curve(scurve)[1]:
        f = _tolin(_curve_val(scurve, hue), 2.0)
        c = _curve_val(COEFF_POINTS, s)
        e = 1.0 + np.where(f < 0.0, c, 1.0 - c)
        s = s * (1.0 + np.sign(f) * np.power(np.clip(np.abs(f), 0.0, 1.0), e))
    if not _curve(lcurve)[1]:
        Y = Y * (1.0 + _tolin(_curve_val(lcurve, hue), 10.0))
    if not hue_first and not _curve(hcurve)[1]:
        h = h + _tolin(_curve_val(hcurve, hue), 32.0) * np.pi
    u, v = s * np.sin(h), s * np.cos(h)                       # hsl2yuv
    Y, u, v = Y * 65535.0, u * 65535.0, v * 65535.0           # normalizeFloatTo65535
    if not to_rgb:
        return [v, Y, u]
    B, R = Y - u, v + Y                                       # yuv_to_rgb
    return [R, (Y - R * ws1[0] - B * ws1[2]) / ws1[1], B]


def satvib_model(img, saturation, vibrance):
    """saturationVibrance in float64, the 2^-16 threshold of apply_vibrance and the output floor included"""
    ws1 = np.asarray(O.REC2020_WS_D, np.float64).reshape(3, 3)[1]
    sat, vib, noise = 1.0 + saturation / 100.0, 1.0 - vibrance / 1000.0, 2.0 ** -16
    r, g, b = (np.asarray(p, np.float64) for p in img)
    lum = r * ws1[0] + g * ws1[1] + b * ws1[2]
    out = []
    for c in (r, g, b):
        x = c - lum
        if vibrance:
            ax = np.abs(x / 65535.0)
            x = np.where(ax > noise, np.sign(x) * np.power(ax, vib) * 65535.0, x)
        out.append(np.maximum(lum + sat * x, noise))
    return out


def _deviation(got, model, floor):
    return max(float((np.abs(g.astype(np.float64) - m) / np.maximum(np.abs(m), floor)).max()) for g, m in zip(got, model))


def _peak_deviation(got, model, img):
    """the same relative to the pixel's own magnitude: the largest |channel| of the input pixel (at least 1)"""
    peak = np.maximum(np.max(np.abs(np.stack([np.asarray(p, np.float64) for p in img])), axis=0), 1.0)
    return max(float((np.abs(g.astype(np.float64) - m) / np.maximum(np.abs(m), peak)).max()) for g, m in zip(got, model))


# Largest deviation of the oracle from the model over SCENES x {all three curves, the saturation curve alone} x both to_rgb (HSL) and over
# SCENES x SATVIB (saturation / vibrance), measured on the CPU; the tests print the current values and assert 4 x these, the project's margin for
# float32 rounding chains.  No pixel is excepted (the issue allows up to 1e-4 of them next to a curve knot or the hue wrap: the curves are
# continuous there and none was needed).
#
# MODEL_MEASURED is |oracle - model| / max(|model|, 1.0).  The floor is one unit of the 0 .. 65535 scale: the float32 chain carries Y with an
# absolute rounding of up to 0.004 units (half an ulp at 65535), u = Y - b and v = r - Y inherit it, and wherever an output is a difference of
# such values that nearly cancels -- u and v of a near-grey pixel in YUV mode, a channel pushed to about zero -- the deviation is that absolute
# rounding and has no relative meaning.  That is what these two figures are: 0.003 units on outputs of 0.1 .. 1 unit.
MODEL_MEASURED = {"hsl": 3.132e-03, "satvib": 3.700e-03}
# PEAK_MEASURED is the same with the pixel's own magnitude as the floor, max(|model|, largest |input channel| of the pixel, 1.0): the cancelling
# outputs then weigh what they are worth and the figure is the rounding chain's.  HSL with all three curves: 2.96e-06, on near-grey pixels
# (chroma 15 on a level of 28 000), where the hue is the arc tangent of two rounding residues and the luminance and hue curves turn its 1e-4 rad of
# noise into 20 ulps of Y; with the saturation curve alone 3.0e-07.  Saturation / vibrance: 3.65e-07, three ulps.  A restatement error -- another
# base, the steps in another order, c for 1 - c -- moves pixels by 1e-3 and more (test_the_bound_tells_a_wrong_restatement_apart).
PEAK_MEASURED = {"hsl": 2.958e-06, "satvib": 3.652e-07}
MARGIN = 4.0
NOISE_FLOOR = 2.0 ** -16 * (1.0 - 1e-6)          # the reference's floor is pow_F(2.f, -16.f) = xexpf(-16 x xlogf(2)), 2^-16 to an ulp or two
HSL_CURVES = [("all three", (H_CURVE, S_CURVE, L_CURVE)), ("saturation only", (None, S_CURVE, None))]


def test_scenes_hold_what_they_are_for():
    img = _scene("wild", 37, 29)
    big = _scene("wild", 421, 301)
    for r, g, b in (img, big):
        grey = (r == g) & (g == b)
        assert (grey & (r > 0)).sum() >= 6 and (grey & (r == 0)).sum() >= 6          # achromatic above zero, and exact zeros: xatan2f(0, 0)
        assert ((r < 0) & (g < 0) & (b < 0)).sum() >= 6                               # negative luminance
        assert (grey & (r == np.float32(1.5 * 65535.0))).sum() >= 6 and ((r == np.float32(1.5 * 65535.0)) & ~grey).sum() >= 6
        one_negative = ((r < 0).astype(int) + (g < 0) + (b < 0)) == 1
        assert one_negative.sum() >= 3
    smooth = _scene("smooth", 420, 300)
    assert min(float(p.min()) for p in smooth) >= 10.0 and max(float(p.max()) for p in smooth) < 40000.0
    # both signs of tolin and both branches of the exponent occur, and hue01 takes its v < 0 wrap; its v > 1 wrap is dead code behind xatan2f,
    # whose range is [-pi, pi]
    ws1 = np.asarray(O.REC2020_WS_D, np.float64).reshape(3, 3)[1]
    r, g, b = (np.asarray(p, np.float64) for p in big)
    Y = r * ws1[0] + g * ws1[1] + b * ws1[2]
    h = np.arctan2(Y - b, r - Y)
    assert (h < 0).any() and (h > 0).any() and (Y < 0).any()
    f = _tolin(_curve_val(S_CURVE, _hue01(h)), 2.0)
    assert (f < 0).any() and (f > 0).any()


def test_hsl_oracle_agrees_with_the_float64_model():
    worst, worst_peak = 0.0, 0.0
    for kind, w, h in SCENES:
        img = _scene(kind, w, h)
        for cname, (hc, sc, lc) in HSL_CURVES:
            for to_rgb in (True, False):
                ref = O.hsl_equalizer(list(img), hc, sc, lc, 0, to_rgb=to_rgb)
                model = hsl_model(img, hc, sc, lc, to_rgb)
                assert all(np.isfinite(p).all() for p in ref) and all(np.isfinite(m).all() for m in model)
                d, dp = _deviation(ref, model, 1.0), _peak_deviation(ref, model, img)
                print(f"hsl {kind} {w}x{h} {cname} to_rgb {to_rgb}: deviation {d:.4g}, relative to the pixel's peak {dp:.4g}")
                worst, worst_peak = max(worst, d), max(worst_peak, dp)
    print(f"hsl: MODEL_MEASURED now {worst:.4g} (recorded {MODEL_MEASURED['hsl']:.4g}), PEAK_MEASURED now {worst_peak:.4g} (recorded {PEAK_MEASURED['hsl']:.4g})")
    assert worst <= MARGIN * MODEL_MEASURED["hsl"]
    assert worst_peak <= MARGIN * PEAK_MEASURED["hsl"]


def test_saturation_vibrance_oracle_agrees_with_the_float64_model():
    worst, worst_peak = 0.0, 0.0
    for kind, w, h in SCENES:
        img = _scene(kind, w, h)
        for sat, vib in SATVIB:
            ref = O.saturation_vibrance(list(img), sat, vib)
            model = satvib_model(img, sat, vib)
            assert all(np.isfinite(p).all() for p in ref)
            assert all(float(p.min()) >= NOISE_FLOOR for p in ref)                       # the output floor
            d, dp = _deviation(ref, model, 1.0), _peak_deviation(ref, model, img)
            print(f"saturation / vibrance {kind} {w}x{h} ({sat}, {vib}): deviation {d:.4g}, relative to the pixel's peak {dp:.4g}")
            worst, worst_peak = max(worst, d), max(worst_peak, dp)
    print(f"satvib: MODEL_MEASURED now {worst:.4g} (recorded {MODEL_MEASURED['satvib']:.4g}), PEAK_MEASURED now {worst_peak:.4g} (recorded {PEAK_MEASURED['satvib']:.4g})")
    assert worst <= MARGIN * MODEL_MEASURED["satvib"]
    assert worst_peak <= MARGIN * PEAK_MEASURED["satvib"]


def test_vibrance_threshold_and_floor_in_the_oracle():
    """apply_vibrance leaves |x| / 65535 <= 2^-16 alone (a grey pixel keeps its chroma residue), and every output is at least 2^-16: black comes
    out as 2^-16, not 0"""
    grey = [np.full((3, 7), 1234.5, np.float32)] * 3
    black = [np.zeros((3, 7), np.float32)] * 3
    for sat, vib in SATVIB:
        for img in (grey, black):
            ref = O.saturation_vibrance(img, sat, vib)
            model = satvib_model(img, sat, vib)
            for p, m in zip(ref, model):
                assert np.allclose(p, m, rtol=1e-6, atol=0.0)
        out = O.saturation_vibrance(black, sat, vib)
        assert all((p == out[0][0, 0]).all() and NOISE_FLOOR <= out[0][0, 0] <= 2.0 ** -16 * (1 + 1e-6) for p in out)


@pytest.mark.parametrize("wrong", ["base", "order", "exponent"])
def test_the_bound_tells_a_wrong_restatement_apart(wrong, monkeypatch):
    """the model with one thing restated wrongly is further from the oracle than the bound allows: luminance base 8 for 10, the hue step ahead of
    the masks, c for 1 - c in the exponent"""
    import sys
    me = sys.modules[__name__]
    img = _scene("smooth", 420, 300)
    ref = O.hsl_equalizer(list(img), H_CURVE, S_CURVE, L_CURVE, 0, to_rgb=True)
    if wrong == "base":
        tolin = me._tolin
        monkeypatch.setattr(me, "_tolin", lambda y, base: tolin(y, 8.0 if base == 10.0 else base))
    elif wrong == "exponent":
        monkeypatch.setattr(me, "COEFF_POINTS", (1, 0.25, 1.0, 0.5, 0.18, 1, 0, 0, 0.35))
        _curve.cache_clear()
    dp = _peak_deviation(ref, hsl_model(img, H_CURVE, S_CURVE, L_CURVE, True, hue_first=(wrong == "order")), img)
    print(f"wrong {wrong}: {dp:.4g}")
    assert dp > 100 * MARGIN * PEAK_MEASURED["hsl"]
