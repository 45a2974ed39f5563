"""CPU: the raw CA correction's checker (tests/emul/ca_correct_ref.cc) on frames with known lateral CA, its control-flow branches,
and the C ABI of artgpu_raw_ca_correct (declared, bound, exported)."""
import os
import re

import numpy as np
import pytest

from art_amd import synth
import ca_lib
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHASES = [synth.FILTERS_RGGB, synth.FILTERS_BGGR, synth.FILTERS_GRBG, synth.FILTERS_GBRG]
K_RED, K_BLUE = 0.002, -0.0015


def _poly(fit, c, d, vb, hb, order=4):
    return sum(vb ** i * hb ** j * fit[c, d, order * i + j] for i in range(order) for j in range(order))


@pytest.mark.parametrize("filters", PHASES)
def test_fitted_shifts_follow_the_lateral_ca(filters):
    """R(x) = G(x + (x - c) k): the fitted shift of the inner blocks has the sign of (x - c) k and its size.  The checker is the
    reference's arithmetic, and on this scene its 4th-order fit lands within 0.094 px of the model on average but up to 0.31 px
    off at single block centres (the per-tile estimates scatter and the fit follows them); a 0.15 px bound at every centre would
    hold the reference's algorithm to more than it does, so the mean is held to 0.12 px and every centre to 0.35 px."""
    w, h = 1200, 800
    raw = ca_lib.lateral_ca_frame(w, h, filters, K_RED, K_BLUE)
    _, fit, info = ca_lib.ca_correct(raw, filters, True, 1, avoid_colour_shift=False, want_info=True)
    assert info["processpasstwo"] and info["polyord"] == 4
    errs = []
    for vb in range(2, info["vblsz"] - 2):
        for hb in range(2, info["hblsz"] - 2):
            yc, xc = -8 + (vb - 1) * 112 + 64, -8 + (hb - 1) * 112 + 64
            for c, k in ((0, K_RED), (1, K_BLUE)):
                for d, (pos, cen) in enumerate(((yc, (h - 1) / 2), (xc, (w - 1) / 2))):
                    want, got = (pos - cen) * k, _poly(fit, c, d, vb, hb)
                    if abs(want) > 0.2:
                        assert np.sign(got) == np.sign(want), (vb, hb, c, d, got, want)
                    errs.append(abs(got - want))
    assert np.mean(errs) < 0.12 and max(errs) < 0.35, (np.mean(errs), max(errs))


def _fringe(raw, filters):
    r, g, b = oracle_lib.amaze(raw, filters, 1.0, 4)
    s = (slice(40, -40), slice(40, -40))
    return float(np.mean((r[s] - g[s]) ** 2 + (b[s] - g[s]) ** 2))


@pytest.mark.parametrize("filters", [synth.FILTERS_RGGB, synth.FILTERS_GRBG])
def test_colour_fringes_drop_after_correction(filters):
    raw = ca_lib.lateral_ca_frame(1200, 800, filters, K_RED, K_BLUE)
    out, _ = ca_lib.ca_correct(raw, filters, True, 2, avoid_colour_shift=True)
    before, after = _fringe(raw, filters), _fringe(out, filters)
    assert after < 0.7 * before, (before, after)


def test_flat_frame_vanishing_block_denominator():
    raw = ca_lib.lateral_ca_frame(600, 400, synth.FILTERS_RGGB, flat=True)
    out, fit, info = ca_lib.ca_correct(raw, synth.FILTERS_RGGB, True, 2, avoid_colour_shift=False, want_info=True)
    assert info == dict(info, iterations_run=1, processpasstwo=False)
    assert not fit.any()
    assert np.array_equal(out, raw)


def test_small_frame_skips_pass_two():
    """300 x 200: 2 x 3 inner blocks, under the 10 the fit needs (L816-821)"""
    raw = ca_lib.lateral_ca_frame(300, 200, synth.FILTERS_RGGB, K_RED, K_BLUE)
    out, fit, info = ca_lib.ca_correct(raw, synth.FILTERS_RGGB, True, 2, avoid_colour_shift=False, want_info=True)
    assert not info["processpasstwo"] and info["iterations_run"] == 1 and info["polyord"] == 2
    assert np.array_equal(out, raw)


def test_linear_fit_under_32_blocks():
    """600 x 400: 4 x 6 inner blocks -> linear fit, only fitparams[c][dir][0..3] written"""
    raw = ca_lib.lateral_ca_frame(600, 400, synth.FILTERS_RGGB, K_RED, K_BLUE)
    out, fit, info = ca_lib.ca_correct(raw, synth.FILTERS_RGGB, True, 1, avoid_colour_shift=False, want_info=True)
    assert info["processpasstwo"] and info["polyord"] == 2
    assert fit[:, :, :4].any() and not fit[:, :, 4:].any()
    assert not np.array_equal(out, raw)


@pytest.mark.parametrize("w,h", [(1201, 800), (1200, 801), (1199, 799)])
def test_odd_sizes(w, h):
    filters = synth.FILTERS_GBRG
    raw = ca_lib.lateral_ca_frame(w, h, filters, K_RED, K_BLUE)
    out, fit, info = ca_lib.ca_correct(raw, filters, True, 2, avoid_colour_shift=True, want_info=True)
    assert info["processpasstwo"] and np.isfinite(out).all() and (out >= 0).all()
    # the two-pixel frame border is never corrected, only scaled by the guard's factors at R / B sites
    for r in range(2):
        for c in range(2):
            if ca_lib.fc(filters, r, c) == 1:
                assert np.array_equal(out[r::2, c::2][:1], raw[r::2, c::2][:1])
    assert _fringe(out, filters) < _fringe(raw, filters)


def test_c_abi_declared_bound_exported():
    from art_amd import capi
    src = open(os.path.join(ROOT, "include", "artgpu.h")).read()
    assert re.search(r"int\s+artgpu_raw_ca_correct\s*\(\s*artgpu_ctx\s*\*ctx,\s*artgpu_plane\s*\*raw,\s*uint32_t\s+filters,", src)
    assert "artgpu_raw_ca_correct" in capi.EXPORTS
    assert hasattr(capi.LIB, "artgpu_raw_ca_correct")
    assert hasattr(capi.Context, "raw_ca_correct")
    names = [f[0] for f in capi.CaParams._fields_]
    assert names == ["autocorrect", "iterations", "red", "blue", "avoid_colour_shift"]


def test_ca_params_layout_matches_header(tmp_path):
    """ctypes CaParams and the CA fields at the end of PipelineParams: size and offsets from a probe compiled against include/artgpu.h"""
    import ctypes as C
    import subprocess
    from art_amd import capi
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "artgpu.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                     'sizeof(artgpu_ca_params), offsetof(artgpu_ca_params, autocorrect), offsetof(artgpu_ca_params, iterations),'
                     'offsetof(artgpu_ca_params, red), offsetof(artgpu_ca_params, blue), offsetof(artgpu_ca_params, avoid_colour_shift),'
                     'sizeof(artgpu_pipeline_params), offsetof(artgpu_pipeline_params, ca_enabled), offsetof(artgpu_pipeline_params, ca));return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(capi.CaParams)] + [getattr(capi.CaParams, n).offset for n, _ in capi.CaParams._fields_]
    want += [C.sizeof(capi.PipelineParams), capi.PipelineParams.ca_enabled.offset, capi.PipelineParams.ca.offset]
    assert got == want
