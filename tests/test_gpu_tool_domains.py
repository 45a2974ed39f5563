"""GPU: the twelve local tools behind the colour steps (dehaze, capture sharpening, local contrast, texture boost, region masks, colour
correction, smoothing, tone equalizer, film simulation, film grain, impulse noise reduction, defringe), device against the cached checker runs of
tests/test_oracle_tool_domains.py, each through its own entry point on host planes:

  - the eleven value-domain families of tests/value_domains.py at 262 x 198 (65 groups of four columns and a 2-pixel tail per row);
  - one context used for `huge`, `all_zero`, `tiny`, then `scaled_frac` through the tools with pooled scratch, guided-filter grids or reductions
    whose partial results live on the context, against a fresh one;
  - `scaled_frac` and `zero_and_sat_blocks` as the raw frame of the all-tools pipe of tests/test_gpu_pipeline.py.

Every bit of every value is compared (value_domains.report_mismatch: step, family, count, first coordinates, both values in hex), with no mask and
no tolerance, and every info structure field by field.  The CPU file asserts that the checker's side is finite and holds -0.0 and subnormals
where it says.  Two rules beside that, both from tests/cc_lib.py:

  - on the (step, family) pairs of NONFINITE -- colour correction with a pivot or rgbluminance on `tiny`, local contrast with a curve on `tiny` --
    the NaNs of both sides are mapped to one pattern first (which NaN an operation returns is the one thing the two machines' arithmetic does
    not share); a NaN must then be a NaN in the same place, +-inf is compared by its bits, sign included, and so is every finite value;
  - colour-correction pixels on the checker's `oor` map are a powf per pixel outside the PQ tables and keep cc_lib's
    rtol 2e-4 / atol 0.5; the map's share is
    capped per step and family at what the CPU file measured, rounded up to the next 0.01.

First run on an MI355X: 392 of 399 cases passed.  `texture boost plane 2 iterations` on `mixed_zeros` gave -0.0 where the
checker has +0.0 in 1190 values and in info.minval: the kernel's minimum kept whichever zero its reduction tree met first, the reference's
serial fold keeps the first in raster order (rt_math.h:54-64).  Fixed in textureboost.hip (tb_min_first); the case passes since.

Six Jzazbz colour-correction cases missed rtol 2e-4 / atol 0.5 on their powf pixels on `negzero`, `huge` and `mixed_zeros` (3 of 651 values up to
383 of 155 613, differences up to 2.36e6): PQ_inv has a pole at X = 3.2, pixels with a channel at zero or 1e6 times too bright land beside it, and
there one ulp of the inner powf is tens of units of the pixel.  The checker with its own powf moved one ulp misses the same bound on the same
six pairs, and with a correctly rounded powf still on `huge`: the reference's pixel is what glibc's powf returns.  art_amd/csrc/libmpowf.h
restates glibc's powf (tests/test_libmpowf.py holds it to the host's in every bit); since then every value on every `oor` map has the checker's
bits and all 399 cases pass.  The tolerance stays as the issue sets it.

Mutant libraries (scripts/mkvariant.sh, not committed), MI355X: -fgpu-flush-denormals-to-zero builds of dehaze.hip, toneequalizer.hip,
impulse.hip and filmsim.hip fail 2, 4, 2 and 2 cases on `tiny` (every step of the tool; film simulation: the two `look` cases) while
test_gpu_dehaze / _toneeq / _impulse_defringe / _filmsim stay green.  Not caught: the same build of textureboost.hip, and sse_max <-> std_max
swapped in tb_combine_kernel (test_gpu_textureboost stays green under both as well)."""
import numpy as np
import pytest

import cc_lib
import fs_lib
import id_lib
import lc_lib
import mk_lib
import oracle_lib as O
import sh_lib
import sm_lib
import tb_lib
import te_lib
import dh_lib
import test_oracle_tool_domains as TD
import test_oracle_value_domains as R
import value_domains as VD
from art_amd import capi, synth

pytestmark = pytest.mark.gpu

FAMILIES = TD.FAMILIES
WS, IWS = O.REC2020_WS_D, O.REC2020_IWS_D
CC_RTOL, CC_ATOL = 2e-4, 0.5            # tests/cc_lib.py::assert_same


def _capi_masks(masks):
    return [{k: v for k, v in m.items() if not (k == "area" and v is None)} for m in masks]


def device_step(ctx, step, img):
    """the step on copies of the planes `img`, through the tool's own entry point -> (planes, info in the form TD.run_step returns it)"""
    kind, kw = TD.STEPS[step]
    got = [np.array(p, dtype=np.float32, order="C") for p in img]
    if kind == "dehaze":
        p, keep = capi.dehaze_params(**kw)
        info = ctx.dehaze(capi.host_rgb(got), p, WS, 1.0, want_info=True)
        del keep
        return got, dh_lib.info_fields(info)
    if kind == "sharpen":
        info = ctx.sharpening(capi.host_rgb(got), capi.sharpening_params(**kw), WS, 1.0, want_info=True)
        return got, sh_lib.info_fields(info)
    if kind == "lc":
        info = ctx.local_contrast(capi.host_plane(got[0]), [(kw["contrast"], TD.lc_curve(kw["curve"]), None)], want_info=True)
        return got, lc_lib.info_fields(info)
    if kind == "tb":
        info = ctx.texture_boost(capi.host_rgb(got), kw["regions"], WS, 1.0, True, True, want_info=True)
        return got, tb_lib.info_fields(info)
    if kind == "tb_plane":
        info = ctx.texture_boost_plane(capi.host_plane(got[0]), kw["strength"], kw["threshold"], kw["iterations"], 1.0, True, want_info=True)
        return got, tb_lib.info_fields(info)
    if kind == "masks":
        n = len(kw["masks"])
        h, w = got[0].shape
        L, ab = np.full((n, h, w), np.nan, np.float32), np.full((n, h, w), np.nan, np.float32)
        info = ctx.generate_masks(capi.host_rgb(got), mk_lib.MODE_LAB if kw["lab"] else mk_lib.MODE_RGB, WS, _capi_masks(kw["masks"]), -1, -1, 1.0,
                                  [capi.host_plane(L[i]) for i in range(n)], [capi.host_plane(ab[i]) for i in range(n)], want_info=True)
        return list(L) + list(ab), [mk_lib.info_fields(i) for i in info]
    if kind == "cc":
        info = ctx.color_correction(capi.host_rgb(got), [kw["region"]], WS, IWS, True, want_info=True)
        return got, [cc_lib.info_fields(i) for i in info]
    if kind == "sm":
        info = ctx.smoothing(capi.host_rgb(got), [kw["region"]], WS, 1.0, want_info=True)
        return got, [sm_lib.info_fields(i) for i in info]
    if kind == "te":
        info = ctx.tone_equalizer(capi.host_rgb(got), te_lib.capi_params(te_lib.params(**kw)), WS, 1.0, want_info=True)
        return got, te_lib.info_fields(info)
    if kind == "fs":
        clut = ctx.clut(fs_lib.clut(kw["kind"], kw["level"]), kw["level"])
        try:
            ctx.film_simulation(capi.host_rgb(got), clut, fs_lib.capi_params(fs_lib.params(kw["strength"], kw["same_profile"])))
        finally:
            clut.close()
        return got, None
    if kind == "fg":
        info = ctx.film_grain(capi.host_rgb(got), capi.film_grain_params(kw["iso"], kw["strength"], kw["color"]), WS, 1.0, True, want_info=True)
        return got, [tuple(r[:5]) + (int(np.float32(r[5]).view(np.uint32)),) for r in info.regions()]
    if kind == "impulse":
        info = ctx.impulse_denoise(capi.host_rgb(got), capi.impulse_denoise_params(True, kw["thresh"]), WS, IWS, kw["scale"], True, want_info=True)
        return got, id_lib.impulse_info_fields(info)
    if kind == "defringe":
        info = ctx.defringe(capi.host_rgb(got), capi.defringe_params(True, kw["radius"], kw["threshold"]), WS, IWS, kw["scale"], True, want_info=True)
        return got, id_lib.defringe_info_fields(info)
    raise KeyError(step)


def _as_float(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def compare(step, what, got, info, want, want_info, oor=None, cap=0.0, nonfinite=False):
    """-> the list of failure messages.  Off `oor` every bit through value_domains.report_mismatch; with `nonfinite` the NaNs of both sides are
    one pattern first (cc_lib.bits) and everything else, +-inf included, still goes by its bits; on `oor` cc_lib's tolerance."""
    msgs = []
    if info != want_info:
        msgs.append(f"{what}: info {info} != the checker's {want_info}")
    assert len(got) == len(want), (what, len(got), len(want))
    if oor is not None:
        share = float(oor.mean())
        if share > cap:
            msgs.append(f"{what}: the checker's out-of-range share {share:.5f} exceeds {cap}")
    for k, (g, w) in enumerate(zip(got, want)):
        if not nonfinite:
            assert np.isfinite(w).all(), f"{what} plane {k}: the checker's output is not finite"
        gb, wb = (_as_float(cc_lib.bits(g)), _as_float(cc_lib.bits(w))) if nonfinite else (g, w)
        if oor is not None and oor.any():
            gb = np.where(oor, wb, gb)
            if not np.allclose(g[oor], w[oor], rtol=CC_RTOL, atol=CC_ATOL):
                d = np.abs(g[oor].astype(np.float64) - w[oor])
                msgs.append(f"{what} plane {k}: {int((~(d <= CC_ATOL + CC_RTOL * np.abs(w[oor]))).sum())} of {int(oor.sum())} powf values beyond rtol {CC_RTOL} "
                            f"atol {CC_ATOL}, largest difference {np.nanmax(d):.6g}")
        m = VD.report_mismatch(gb, wb, f"{what} plane {k}")
        if m:
            msgs.append(m)
    return msgs


def compare_family(ctx, step, name):
    want, want_info, oor = TD.o_family(step, name)
    got, info = device_step(ctx, step, TD.family_input(step, name))
    return compare(step, f"{step} on {name} {TD.W}x{TD.H}", got, info, want, want_info, oor, TD.oor_cap(step, name), (step, name) in TD.NONFINITE)


# ---- the families --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("step", TD.STEP_NAMES)
def test_step_on_family(gpu_ctx, step, name):
    msgs = compare_family(gpu_ctx, step, name)
    assert not msgs, "\n".join(msgs)


# ---- one context, families in sequence -----------------------------------------------------------------------------------------------------------------

def test_extreme_frames_leave_nothing_behind_on_a_context():
    """huge, all_zero, tiny, then scaled_frac through dehaze, the tone equalizer at regularization 4, NL-means smoothing, the masks with a blur and
    defringe on ONE context: the last must give the bits a fresh context gives, and those are the checker's."""
    steps = ("dehaze default depth 25", "tone equalizer mixed reg 4", "smoothing nlmeans LC 50", "masks rgb three curves ld50 blur 3", "defringe 2.0/13")

    def run(ctx, name):
        return [device_step(ctx, s, TD.family_input(s, name)) for s in steps]

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
    msgs = []
    for s, (g, gi), (w, wi) in zip(steps, got, want):
        msgs += compare(s, f"scaled_frac after huge, all_zero, tiny: {s}", g, gi, w, wi)
        o, oi, _ = TD.o_family(s, "scaled_frac")
        msgs += compare(s, f"scaled_frac on a fresh context: {s}", w, wi, o, oi)
    assert not msgs, "\n".join(msgs)


# ---- the families as the raw frame of the all-tools pipe ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["scaled_frac", "zero_and_sat_blocks"])
def test_families_through_the_all_tools_pipe(gpu_ctx, name):
    """the frame set-up of test_gpu_pipeline.test_pipeline_all_tools_equal_the_tools_one_by_one with the family as the raw frame: pipeline_run
    against the tools one by one, in bits"""
    from test_gpu_pipeline import all_tools_pipe_against_the_tools_one_by_one
    all_tools_pipe_against_the_tools_one_by_one(gpu_ctx, np.array(R.frame(name, 392, 296, synth.FILTERS_RGGB)))
