"""CPU: the region-mask checker (tests/mk_lib.py, tests/emul/masks_ref.cc) -- that the scenes and cases of tests/test_gpu_masks.py take
every branch of generateMasks' parametric path (from the checker's counters), the rules of masks.cc:1059-1084 and 1244-1308 that the device
code restates, the new entry point's ABI, and what the compiler made of the new kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from art_amd import capi, codeobj
import mk_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "art_amd", "libartgpu.so")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_abi_has_the_entry_point_and_the_structures():
    """fails without the feature: the two symbols and the two structure sizes; artgpu_pipeline_params keeps its layout (the pipe's masks are
    a setting of the context)"""
    for sym in ("artgpu_generate_masks", "artgpu_set_pipeline_masks"):
        assert hasattr(capi.LIB, sym) and sym in capi.EXPORTS, sym
    assert C.sizeof(capi.MaskParams) == 104 and C.sizeof(mk_lib.Mask) == 104
    assert C.sizeof(capi.MasksInfo) == 40 and C.sizeof(mk_lib.Info) == 40
    assert [f[0] for f in capi.PipelineParams._fields_][-1] == "texture_boost_regions"
    assert capi.LIB.artgpu_set_pipeline_masks(None, None, 0, None, 0) == -1     # ARTGPU_EINVAL without a context, no crash
    hdr = open(os.path.join(ROOT, "include", "artgpu.h")).read()
    assert "#define ARTGPU_MASKS_MIN_SIZE %d" % capi.MASKS_MIN_SIZE in hdr


@pytest.fixture(scope="module")
def totals():
    """the counters of all GPU cases added up"""
    tot = {}
    for name in mk_lib.CASES:
        cn = mk_lib.case(name)[7]
        for k, v in cn.items():
            if k == "curve_evals":
                v = [sum(col) for col in zip(*v)]
            if isinstance(v, list):
                tot[k] = [a + b for a, b in zip(tot.get(k, [0] * len(v)), v)]
            else:
                tot[k] = tot.get(k, 0) + v
    return tot


def test_scenes_reach_all_nine_hue_segments_and_the_wrap(totals):
    assert all(c > 0 for c in totals["hue_segment"][:9]), totals["hue_segment"]
    assert totals["hue_wraps"] > 0


def test_scenes_reach_both_sides_of_both_clamps(totals):
    assert totals["guide_low"] > 0 and totals["guide_high"] > 0               # LIM01(l): negative and out-of-range pixels of the scene
    assert totals["clamp_low"] > 0 and totals["clamp_high"] > 0               # LIM01 behind the guided blur


def test_cases_evaluate_every_kind_of_curve(totals):
    assert all(c > 0 for c in totals["curve_evals"]), totals["curve_evals"]   # hue, chromaticity, lightness
    assert totals["curve_identity"] > 0                                        # a present curve FlatCurve found to be the identity: 0.5
    assert totals["ll_built"] > 0 and totals["ll_read"] > 0
    for name in mk_lib.CASES:
        c = mk_lib.CASES[name]
        cn = mk_lib.case(name)[7]
        for i, m in enumerate(c["masks"]):
            want = [m["parametric_enabled"] and m[k] not in (mk_lib.EMPTY, mk_lib.LINEAR, d)
                    for k, d in (("hue", mk_lib.DEFAULT_HUE), ("chromaticity", mk_lib.DEFAULT_CL), ("lightness", mk_lib.DEFAULT_CL))]
            assert [v > 0 for v in cn["curve_evals"][i]] == want, (name, i)


def test_cases_take_the_threshold_posterize_and_tail_branches(totals):
    assert totals["cthr_rescaled"] > 0 and totals["cthr_plain"] > 0 and totals["cthr_negative"] > 0
    assert totals["area_pixels"] > 0
    assert totals["poster_level"][0] > 0 and totals["poster_level"][30] > 0 and totals["poster_level"][2] > 0
    assert sum(1 for c in totals["poster_level"] if c > 0) >= 20
    assert totals["thr_fill"] > 0 and totals["thr_one"] > 0
    assert totals["inverted_planes"] > 0 and totals["opacity_planes"] > 0
    assert totals["filled_planes"] > 0 and totals["blurred_regions"] > 0
    assert mk_lib.case("1930x48-rgb-L-threshold-rescaled")[6][0].cthr_w == 1919
    assert mk_lib.case("1930x48-rgb-L-threshold-rescaled")[6][0].cthr_h == 47


@pytest.mark.parametrize("curve", [mk_lib.EMPTY, mk_lib.LINEAR, "default"])
def test_empty_linear_and_default_curves_count_as_absent(curve):
    img = mk_lib.scene(40, 24, seed=2)
    kw = {k: (d if curve == "default" else curve) for k, d in (("hue", mk_lib.DEFAULT_HUE), ("chromaticity", mk_lib.DEFAULT_CL),
                                                              ("lightness", mk_lib.DEFAULT_CL))}
    rc, L, ab, info, cn = mk_lib.generate(img, mk_lib.MODE_RGB, [mk_lib.mask(parametric_enabled=True, **kw)], want_L=True, want_ab=True)
    assert rc == 0 and info[0].has_mask == 0 and info[0].blurred == 0
    assert cn["filled_planes"] == 2 and sum(map(sum, cn["curve_evals"])) == 0
    assert np.all(_bits(L) == _bits(np.float32(1.0))) and np.all(_bits(ab) == _bits(np.float32(1.0)))


def test_curves_of_a_disabled_parametric_mask_do_not_count():
    _, _, _, _, L, ab, info, cn = mk_lib.case("67x45-rgb-L-no-mask")
    assert [i.has_mask for i in info] == [0, 0] and cn["blurred_regions"] == 0
    assert np.all(L == 1.0) and np.all(ab == 1.0)


def test_opacity_alone_makes_has_mask_and_blurs_every_region():
    """has_mask is global: opacity < 100 in one region sends the other, which has no curve, through the guided blur and LIM01 as well"""
    img = mk_lib.scene(40, 24, seed=4)
    rc, L, _, info, cn = mk_lib.generate(img, mk_lib.MODE_RGB, [mk_lib.mask(), mk_lib.mask(opacity=40)])
    assert rc == 0 and [i.has_mask for i in info] == [1, 1] and [i.blurred for i in info] == [1, 1]
    assert cn["blurred_regions"] == 2 and cn["filled_planes"] == 0
    assert [(i.r1, i.r2) for i in info] == [(4, 25), (4, 25)]                  # blur = 0 while the parametric mask is disabled: 1.f + 0
    assert np.allclose(L[0], 1.0, atol=1e-5) and np.allclose(L[1], 0.4, atol=1e-5)


def test_region_without_curves_beside_one_with_a_curve_is_blurred():
    _, _, _, _, L, ab, info, cn = mk_lib.case("67x45-rgb-both-three-regions")
    assert [i.blurred for i in info] == [1, 1, 0]                              # the third region's blur is below -10
    assert cn["blurred_regions"] == 2
    assert (info[0].r1, info[0].r2) == (16, 100) and (info[1].r1, info[1].r2) == (4, 25)


@pytest.mark.parametrize("name", ["67x45-rgb-both-three-regions", "256x131-rgb-L-ld0-ld100", "67x45-lab-L-absent-curves"])
def test_skipping_the_unread_lightness_detail_plane_changes_no_bit(name):
    """the reference builds LL whenever an L mask is asked for; only a lightness curve reads it"""
    img, mode, masks, kw, L, ab, _, cn = mk_lib.case(name)
    rc, L2, ab2, _, cn2 = mk_lib.generate(img, mode, masks, always_ll=True, **kw)
    assert rc == 0 and cn2["ll_built"] == 1
    assert np.array_equal(_bits(L), _bits(L2))
    if ab is not None:
        assert np.array_equal(_bits(ab), _bits(ab2))
    if name == "67x45-lab-L-absent-curves":
        assert cn["ll_built"] == 0 and cn["ll_read"] == 0                      # no lightness curve: skipped


def test_lightness_detail_changes_the_mask():
    img = mk_lib.scene(64, 40, seed=6)
    out = [mk_lib.generate(img, mk_lib.MODE_RGB, [mk_lib.mask(parametric_enabled=True, lightness=mk_lib.LIGHT_A, lightness_detail=d)])[1]
           for d in (0, 50, 100)]
    assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[1], out[2])


def test_checker_reports_what_is_not_on_the_device_path():
    img = mk_lib.scene(16, 16, seed=1)
    for kw in (dict(deltae_enabled=True), dict(drawn_enabled=True), dict(external_enabled=True), dict(linked_enabled=True),
               dict(curve_is_identity=False), dict(show_mask=True)):
        assert mk_lib.generate(img, mk_lib.MODE_RGB, [mk_lib.mask(**kw)])[0] == mk_lib.EUNSUPPORTED, kw
    for mode in (mk_lib.MODE_YUV, mk_lib.MODE_XYZ):
        assert mk_lib.generate(img, mode, [mk_lib.mask()])[0] == mk_lib.EUNSUPPORTED
    assert mk_lib.generate(img, mk_lib.MODE_RGB, [mk_lib.mask()], want_L=False, want_ab=False)[0] == mk_lib.EINVAL


# ---- what the compiler made of the kernels (art_amd/codeobj.py), in the pattern of tests/test_textureboost_resources.py ----
KERNELS = [r"mk_ll_kernel", r"mk_fused_kernel", r"mk_tail_kernel", r"mk_rescale_kernel"]


@pytest.fixture(scope="module")
def table():
    assert os.path.exists(LIB), "art_amd/libartgpu.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    t = codeobj.kernel_table(LIB)
    assert t, "libartgpu.so holds no gfx950 code object"
    return t


@pytest.mark.parametrize("pattern", KERNELS)
def test_kernels_neither_spill_nor_use_scratch(table, pattern):
    hits = {n: r for n, r in table.items() if re.search(pattern, n)}
    assert len(hits) == 1, (pattern, sorted(hits))
    for name, r in hits.items():
        assert r["scratch_bytes"] == 0 and r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0, (name, r)


def test_fused_pass_keeps_eight_waves_per_simd(table):
    """512-thread workgroups with the polylines in dynamic LDS (no static LDS): at 64 registers or fewer the register file holds four of them
    per CU, so what limits the residency is the LDS the launch asks for (72 KB for one region's three curves: two workgroups)"""
    (name, r), = [(n, r) for n, r in table.items() if "mk_fused_kernel" in n]
    assert r["vgprs"] <= 64 and r["static_lds_bytes"] == 0 and r["max_workgroup"] == 512, (name, r)


def test_no_other_mask_kernel(table):
    mine = [n for n in table if re.search(r"\bmk_\w+_kernel", n)]
    assert len(mine) == len(KERNELS), sorted(mine)
