"""CPU: the capture-sharpening checker (tests/sh_lib.py, tests/emul/sharpen_ref.cc) against what the compiled reference recorded, the branch
coverage of the cases the GPU tests use, the auto-radius inputs' condition, and the ABI of the new structures."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import sh_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    """bit for bit, NaN payloads aside"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("w,h", sh_lib.GOLDEN_SIZES)
def test_blur_forms_equal_the_compiled_reference(w, h):
    """every regime and size of tests/golden/gauss_divmult.npz (recorded from the reference's own gauss.cc, tests/golden/make_golden_sharpen.py)"""
    g = sh_lib.golden()
    src, div, dst0 = g[f"src_{w}x{h}"], g[f"div_{w}x{h}"], g[f"dst0_{w}x{h}"]
    assert (src == 0).any() and (src < 0).any() and (src > 65535).any()
    for sigma in sh_lib.GOLDEN_SIGMAS:
        k = sh_lib.golden_key(sigma, w, h)
        d, coef, _ = sh_lib.gauss(src, None, div, sigma, sh_lib.GAUSS_DIV)
        m, _, _ = sh_lib.gauss(src, dst0, None, sigma, sh_lib.GAUSS_MULT)
        if coef is not None:
            # a difference here would be libm's (exp in double), not the stencil's
            assert np.array_equal(_bits(coef), _bits(g[f"k_{sigma:g}"])), (sigma, coef, g[f"k_{sigma:g}"])
        assert _same(d, g["d_" + k]), ("DIV", k, int((_bits(d) != _bits(g["d_" + k])).sum()))
        assert _same(m, g["m_" + k]), ("MULT", k, int((_bits(m) != _bits(g["m_" + k])).sum()))
    # what the compiled reference does with a negative divisor in the recursive regime (gauss.cc:1079-1140): kept in the last three rows of
    # the 8-column groups, clamped to zero in the rows above and in the scalar tail columns.  Read from the recording, not from the checker.
    for sigma in (1.6, 2.5):
        d = g["d_" + sh_lib.golden_key(sigma, w, h)]
        assert div[h - 1, 1] < 0 and div[h - 3, 5] < 0 and d[h - 1, 1] < 0 and d[h - 3, 5] < 0, (sigma, d[h - 1, 1], d[h - 3, 5])
        assert div[h - 4, 6] < 0 and d[h - 4, 6] == 0, (sigma, d[h - 4, 6])
        if w % 8:
            assert div[h - 2, w - 1] < 0 and d[h - 2, w - 1] == 0, (sigma, d[h - 2, w - 1])
        else:
            assert d[h - 2, w - 1] < 0, (sigma, d[h - 2, w - 1])
    # the recorded forms are not all the same thing: the 7x7 form differs from a 7x7 form without the doubled c21 by construction
    assert not _same(g["d_" + sh_lib.golden_key(0.84, w, h)], g["d_" + sh_lib.golden_key(1.0, w, h)])


def test_mask_restatement_equals_the_oracle_at_radius_2():
    """sh_ref_blend_mask is buildBlendMask with the blur radius as a parameter; at 2 it is oracle_build_blend_mask"""
    Y = sh_lib.luminance(sh_lib.edge_scene(131, 67, seed=2)).astype(np.float32)
    thr = sh_lib.pow_F(np.float32(0.2), 1.2)
    L = O.lib()
    fp = C.POINTER(C.c_float)
    L.oracle_build_blend_mask.argtypes = [fp, fp, C.c_int, C.c_int, C.c_float, C.c_int]
    L.oracle_build_blend_mask.restype = C.c_float
    want = np.zeros_like(Y)
    L.oracle_build_blend_mask(Y.ctypes.data_as(fp), want.ctypes.data_as(fp), 131, 67, C.c_float(float(thr)), 0)
    assert np.array_equal(_bits(sh_lib.blend_mask(Y, thr, 2.0)), _bits(want))
    assert not np.array_equal(_bits(sh_lib.blend_mask(Y, thr, 2.0 / np.sqrt(np.float32(2.0)))), _bits(want))


def test_cases_reach_every_branch():
    regimes, early, late, never = set(), 0, 0, 0
    total = {}
    for name in sh_lib.CASES:
        img, scale, kw, want, info, cn = sh_lib.case(name)
        assert info.early_out == 0, name
        regimes.add(info.regime)
        early += sum(cn["frozen_iter"][:3]); late += sum(cn["frozen_iter"][15:]); never += cn["never_frozen"]
        for k, v in cn.items():
            if k != "frozen_iter":
                total[k] = total.get(k, 0) + v
        assert any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(want, img)), name
        assert info.frozen_pixels == sum(cn["frozen_iter"][:19]), name
    print("sharpening cases:", sorted(regimes), early, late, never, total)
    assert regimes == {1, 2, 3, 4}                               # 3x3, 5x5, 7x7, recursive (the copy regime: the deconvolution cases below)
    assert early > 0 and late > 0 and never > 0                  # frozen in an early iteration, in a late one, not at all
    assert total["impulse_vec"] > 0 and total["impulse_lo"] > 0 and total["impulse_body"] > 0 and total["impulse_hi"] > 0   # both forms of the test, every column range
    assert total["mask_low"] > 0 and total["mask_high"] > 0      # mask values below 0.01 and above 0.99
    assert total["y_nonpos"] > 0 and total["ring_pixels"] > 0
    one = sh_lib.case("300x200-arp-default")
    assert one[5]["mask_low"] > 0 and one[5]["mask_high"] > 0
    assert sh_lib.case("67x41-contrast0")[4].contrast_threshold == 0.0
    bright = sh_lib.luminance(sh_lib.case("300x200-zeros-and-bright")[0])
    assert (bright > 65535).any() and (bright == 0).any()


def test_deconvolution_cases_reach_every_regime():
    regimes = set()
    for sigma in sh_lib.RL_SIGMAS:
        Y, bl, imp = sh_lib.rl_inputs(67, 41)
        out, info, cn = sh_lib.deconv(Y, bl, imp, sigma, 1.0)
        regimes.add(info.regime)
        assert not np.array_equal(_bits(out), _bits(Y)) or info.regime == 0
    assert regimes == {0, 1, 2, 3, 4}
    Y, bl, imp = sh_lib.rl_inputs(67, 41)
    assert imp.any() and (bl < 0.01).any() and (bl > 0.99).any()
    for sigma, amount, early in ((0.75, 0.0, 4), (0.1, 1.0, 5)):
        out, info, _ = sh_lib.deconv(Y, bl, imp, sigma, amount)
        assert info.early_out == early and np.array_equal(_bits(out), _bits(Y))


def test_early_outs_and_unsupported():
    img = sh_lib.edge_scene(23, 9, seed=3)
    for kw, early in ((dict(enabled=False), 1), (dict(amount=0), 2)):
        out, info, _ = sh_lib.sharpening(img, **kw)
        assert info.early_out == early and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(out, img))
    small = [a[:7, :] for a in img]
    out, info, _ = sh_lib.sharpening(small)
    assert info.early_out == 3
    # deconvsharpening's own early returns still go through multiply: Y / Y
    for kw, early in ((dict(deconvamount=0), 4), (dict(deconvradius=0.1), 5)):
        out, info, _ = sh_lib.sharpening(img, **kw)
        assert info.early_out == early
    assert sh_lib.sharpening(img, method=sh_lib.USM) is None
    assert sh_lib.sharpening(img, deconvradius=25.0) is None
    assert sh_lib.sharpening(img, deconvradius=float("nan")) is None
    assert sh_lib.sharpening(img, deconvradius=24.9, corner_boost=0.2) is None
    assert sh_lib.sharpening(img, scale=12.0) is None            # 2 / sqrt(12) < 0.6


@pytest.mark.parametrize("w,h,filters,seed", sh_lib.RADIUS_CASES)
def test_auto_radius_inputs_serial_loop_equals_pure_maximum(w, h, filters, seed):
    """The library's contract is the pure maximum; the reference's loop adopts a pair only when it beats the running maximum times the
    minimum, which can differ in the last place.  The GPU test's inputs are chosen (seeds picked until this held) so that both agree."""
    raw = sh_lib.mosaic(w, h, seed, filters)
    r1, m1, _ = sh_lib.radius(raw, filters, upper=sh_lib.RADIUS_CLIP, serial=True)
    r2, m2, cn = sh_lib.radius(raw, filters, upper=sh_lib.RADIUS_CLIP, serial=False)
    assert m1.view(np.uint32) == m2.view(np.uint32) and r1.view(np.uint32) == r2.view(np.uint32)
    assert m2 > 1 and np.isfinite(r2)
    assert cn["clip_rule_a"] > 0 and cn["clip_rule_b"] > 0 and cn["pairs"] > 0
    # without the clipped rules the maximum would be another one
    _, m3, _ = sh_lib.radius(raw, filters, upper=1e30, serial=False)
    assert m3 > m2


def test_flat_plane_has_no_pair_and_a_nan_radius():
    r, m, _ = sh_lib.radius(np.full((48, 64), 5000.0, np.float32), sh_lib.FILTERS_RGGB)
    assert m == 1.0 and np.isnan(r)


def test_abi_of_the_new_structures(tmp_path):
    """the new symbols exist; ctypes SharpeningParams / SharpeningInfo and the tail of PipelineParams against a probe compiled with
    include/artgpu.h; artgpu_pipeline_params is what it was up to and including `dehaze`"""
    from art_amd import capi
    for sym in ("artgpu_sharpening", "artgpu_rl_deconvolution", "artgpu_gaussian_blur_ex", "artgpu_deconv_auto_radius"):
        assert sym in capi.EXPORTS and hasattr(capi.LIB, sym), sym
    pf = [n for n, _ in capi.SharpeningParams._fields_]
    nf = [n for n, _ in capi.SharpeningInfo._fields_]
    tail = ["dehaze_enabled", "dehaze", "sharpening_enabled", "sharpening_auto_radius", "sharpening_clip_val", "sharpening"]
    exprs = (["sizeof(artgpu_sharpening_params)"] + [f"offsetof(artgpu_sharpening_params, {n})" for n in pf] +
             ["sizeof(artgpu_sharpening_info)"] + [f"offsetof(artgpu_sharpening_info, {n})" for n in nf] +
             ["sizeof(artgpu_pipeline_params)"] + [f"offsetof(artgpu_pipeline_params, {n})" for n in tail])
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "artgpu.h"\nint main(void){' +
                     "".join(f'printf("%zu\\n", {e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = ([C.sizeof(capi.SharpeningParams)] + [getattr(capi.SharpeningParams, n).offset for n in pf] +
            [C.sizeof(capi.SharpeningInfo)] + [getattr(capi.SharpeningInfo, n).offset for n in nf] +
            [C.sizeof(capi.PipelineParams)] + [getattr(capi.PipelineParams, n).offset for n in tail])
    assert got == want, list(zip(exprs, got, want))
    # the structure before this stage: 800 bytes ending with `dehaze` at 760; every earlier field where it was
    before = {"sensor": 0, "bayer_method": 4, "filters": 8, "initial_gain": 16, "xtrans_passes": 24, "xtrans": 28, "rgb_cam": 172, "border": 220,
              "mul": 224, "do_clip": 236, "has_cam_to_work": 240, "cam_to_work": 248, "ws": 320, "iws": 392, "denoise_enabled": 464, "denoise": 472,
              "exposure_enabled": 560, "expcomp": 568, "black": 576, "tone_enabled": 584, "tone_mode": 588, "tone_lut": 592, "white_point": 600,
              "to_out": 604, "to_work": 640, "scale": 680, "chrominance_auto_factor": 688, "ca_enabled": 696, "ca": 704,
              "local_contrast_enabled": 736, "local_contrast_nregions": 740, "local_contrast_regions": 744, "dehaze_enabled": 752, "dehaze": 760}
    assert {n: getattr(capi.PipelineParams, n).offset for n in before} == before
    assert capi.PipelineParams.sharpening_enabled.offset == 800 == capi.PipelineParams.dehaze.offset + C.sizeof(capi.DehazeParams)
    assert [n for n, _ in capi.PipelineParams._fields_][:len(before)] == list(before)
    # the checker's structures are the library's
    assert C.sizeof(sh_lib.Params) == C.sizeof(capi.SharpeningParams) and C.sizeof(sh_lib.Info) == C.sizeof(capi.SharpeningInfo)
    assert [(n, getattr(sh_lib.Params, n).offset) for n, _ in sh_lib.Params._fields_] == [(n, getattr(capi.SharpeningParams, n).offset) for n in pf]
    assert [(n, getattr(sh_lib.Info, n).offset) for n, _ in sh_lib.Info._fields_] == [(n, getattr(capi.SharpeningInfo, n).offset) for n in nf]
