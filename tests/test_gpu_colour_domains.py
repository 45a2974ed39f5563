"""GPU: the per-pixel colour steps that have a C oracle (HSL equalizer, log encoding, saturation / vibrance, channel mixer, RGB curves, exposure,
STD tone curve, NEUTRAL, the Lab switch and adjustments, the matrix conversion), device against the cached oracle runs of
tests/test_oracle_colour_domains.py, each through its own entry point:

  - the eleven value-domain families of tests/value_domains.py at 262 x 198 (65 groups of four columns and a 2-pixel tail per row);
  - uniform(-500, 70000) planes at 1 x 1, 1 x 7, 7 x 1, 3 x 9 (only a tail), 5 x 5 and 9 x 3 with zeros of both signs in body and tail columns;
  - HSL on the wild scene of tests/hsl_lib.py (achromatic, negative, 1.5 x 65535 and exact-zero blocks, single negative channels);
  - one context used for `huge`, `all_zero`, `tiny`, then `scaled_frac`, against a fresh one.

Every bit of every value is compared (value_domains.report_mismatch: step, family or shape, count, first coordinates, both values in hex), with no
mask; the CPU file asserts that the oracle's side is finite and holds -0.0 and subnormals where it says.  The one exception is NEUTRAL, which keeps
the rule of tests/test_gpu_tonecurve.py: bit equality off the oracle's `oor` mask (pixels whose LMS exceed 1 go through the host's powf there),
rtol 2e-4 / atol 0.5 on it, and the mask's share capped (0.02, `huge` 0.2).

Log encoding at regularization 60 and HSL at smoothing 5 go through the shared guided filter: its band statistics see constant, all-zero and
subnormal planes here, and at the small shapes its radius clamp makes the box radius 0 or 1.

What these cases catch and what they do not (mutant libraries): sse_max and std_max swapped in exposure_kernel fails exposure
with black 0 on `negzero` / `mixed_zeros` and every small shape but 1 x 1; flush-to-zero builds of pixelops.hip and hsl.hip fail on `tiny`, `tiny2`
and `small`; neither change to hue01's comparisons nor the std_max(r, 0.f) dropped from tone_std_kernel moves a bit on any finite input."""
import numpy as np
import pytest

import oracle_lib as O
import hsl_lib
import test_oracle_colour_domains as CD
from art_amd import capi
from test_gpu_hsl import H_CURVE, L_CURVE, S_CURVE
from test_gpu_lab import curves as lab_curves
from test_gpu_tonecurve import s_curve
from test_gpu_value_domains import _check, _planes

pytestmark = pytest.mark.gpu

FAMILIES = CD.FAMILIES
NEUTRAL_RTOL, NEUTRAL_ATOL = 2e-4, 0.5          # tests/test_gpu_tonecurve.py


def device_step(ctx, step, img):
    """the step on copies of the three planes `img`, through its own entry point -> the three planes"""
    kind, kw = CD.STEPS[step]
    got = [np.array(p, dtype=np.float32, order="C") for p in img]
    rgb = capi.host_rgb(got)
    if kind == "hsl":
        hc, sc, lc = kw["curves"]
        ctx.hsl_equalizer(rgb, hc, sc, lc, kw["smoothing"], O.REC2020_WS_D, 1.0, kw["to_rgb"])
    elif kind == "logenc":
        ctx.log_encoding(rgb, O.REC2020_WS_D, **kw)
    elif kind == "satvib":
        ctx.saturation_vibrance(rgb, kw["saturation"], kw["vibrance"], O.REC2020_WS_D)
    elif kind == "chmix":
        ctx.channel_mixer(rgb, CD.MIXER)
    elif kind == "rgbcurves":
        ctx.rgb_curves(rgb, *CD.rgb_curve_luts())
    elif kind == "exposure":
        ctx.exposure(rgb, kw["exp_scale"], kw["black"])
    elif kind == "tone_std":
        ctx.tone_curve(rgb, s_curve(), kw["whitept"], kw["filmlike_clip"])
    elif kind == "neutral":
        ctx.tone_curve_neutral(rgb, s_curve(), kw["whitecoeff"], O.REC2020_WS_D, O.REC2020_IWS_D)
    elif kind == "rgb2lab":
        ctx.rgb_to_lab(rgb, O.REC2020_WS_D)
    elif kind == "labadj":
        ctx.lab_adjustments(rgb, *lab_curves(3), kw["chroma"])
    elif kind == "lab2rgb":
        ctx.lab_to_rgb(rgb, O.REC2020_IWS_D)
    elif kind == "convert":
        ctx.convert_color_space(rgb, CD.R.MAT)
    else:
        raise KeyError(step)
    return got


def _neutral_msgs(what, got, want, oor, cap):
    """NEUTRAL: every bit off the oracle's out-of-range mask, the tolerance of tests/test_gpu_tonecurve.py on it, the mask's share capped"""
    msgs = []
    share = float(oor.mean())
    if share > cap:
        msgs.append(f"{what}: the oracle's out-of-range share {share:.4f} exceeds {cap}")
    for c, g, w in zip("RGB", got, want):
        assert np.isfinite(w).all(), f"{what} {c}: the oracle's output is not finite"
        m = CD.VD.report_mismatch(np.where(oor, w, g), w, f"{what} {c} (off the out-of-range mask)")
        if m:
            msgs.append(m)
        if not np.isfinite(g).all():
            msgs.append(f"{what} {c}: the device's output is not finite")
        elif not np.allclose(g[oor], w[oor], rtol=NEUTRAL_RTOL, atol=NEUTRAL_ATOL):
            d = np.abs(g[oor].astype(np.float64) - w[oor])
            msgs.append(f"{what} {c}: {int((d > NEUTRAL_ATOL + NEUTRAL_RTOL * np.abs(w[oor])).sum())} of {int(oor.sum())} out-of-range values beyond "
                        f"rtol {NEUTRAL_RTOL} atol {NEUTRAL_ATOL}, largest difference {d.max():.6g}")
    return msgs


def _compare(ctx, step, what, src, want, oor, cap):
    """-> (pairs for _check, messages of the NEUTRAL rule)"""
    got = device_step(ctx, step, src)
    if oor is None:
        return _planes(f"{step} on {what}", got, want), []
    return [], _neutral_msgs(f"{step} on {what}", got, want, oor, cap)


# ---- the families --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("step", CD.STEP_NAMES)
def test_step_on_family(gpu_ctx, step, name):
    want, oor = CD.o_family(step, name)
    pairs, msgs = _compare(gpu_ctx, step, f"{name} {CD.W}x{CD.H}", CD.family_input(step, name), want, oor, CD.oor_cap(name))
    assert not msgs, "\n".join(msgs)
    _check(pairs)


# ---- the small shapes ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", CD.SHAPES)
def test_every_step_on_small_shape(gpu_ctx, w, h):
    """one group of four columns at most: 3 x 9 and 1 x 7 are all tail, 5 x 5 and 9 x 3 a body and a one-column tail, 7 x 1 a single row.  At
    these sizes the guided filter's radius clamp leaves a box radius of 0 or 1 (log encoding 60, HSL smoothing 5)."""
    pairs, msgs = [], []
    for step in CD.STEP_NAMES:
        want, oor = CD.o_shape(step, w, h)
        p, m = _compare(gpu_ctx, step, f"uniform(-500, 70000) {w}x{h}", CD.shape_input(step, w, h), want, oor, 1.0)
        pairs += p
        msgs += m
    assert not msgs, "\n".join(msgs)
    _check(pairs)


# ---- HSL on the wild scene -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("smoothing", [0, 5])
@pytest.mark.parametrize("w,h", [(421, 301), (37, 29)])
def test_hsl_on_the_wild_scene(gpu_ctx, w, h, smoothing):
    img = hsl_lib.wild_scene(w, h, w)
    pairs = []
    for to_rgb in (True, False):
        got = [p.copy() for p in img]
        gpu_ctx.hsl_equalizer(capi.host_rgb(got), H_CURVE, S_CURVE, L_CURVE, smoothing, O.REC2020_WS_D, 1.0, to_rgb)
        ref = O.hsl_equalizer(img, H_CURVE, S_CURVE, L_CURVE, smoothing, to_rgb=to_rgb)
        assert all(np.isfinite(g).all() for g in got), f"wild scene {w}x{h} smoothing {smoothing} to_rgb {to_rgb}: the device's output is not finite"
        pairs += _planes(f"hsl wild scene {w}x{h} smoothing {smoothing} to_rgb {to_rgb}", got, ref)
    _check(pairs)


# ---- one context, families in sequence -----------------------------------------------------------------------------------------------------------------

def test_extreme_frames_leave_nothing_behind_on_a_context():
    """huge, all_zero, tiny, then scaled_frac through HSL smoothing 5 and log encoding regularization 60 (both through the pooled guided filter) on
    ONE context: the last must give the bits a fresh context gives, and those are the oracle's."""
    steps = ("hsl hsl smoothing 5 rgb", "logenc reg 60")

    def run(ctx, name):
        return [device_step(ctx, s, CD.family_input(s, name)) for s in steps]

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
    for s, g, w in zip(steps, got, want):
        pairs += _planes(f"scaled_frac after huge, all_zero, tiny: {s}", g, w)
        pairs += _planes(f"scaled_frac on a fresh context: {s}", w, CD.o_family(s, "scaled_frac")[0])
    _check(pairs)
