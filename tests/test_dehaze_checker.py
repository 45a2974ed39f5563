"""CPU: the dehaze checker (tests/emul/dehaze_ref.cc around the oracle's guided filter, box blur, FlatCurve and LUTf) and the library's
two host routines, artgpu_dehaze_strength_lut (ipdehaze.cc:419-424) and artgpu_dehaze_estimate_ambient (L128-230, L385-386).  No GPU:
libartgpu.so loads without a device, both routines are pure host code."""
import os

import numpy as np
import pytest

import dh_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,points", [("default", dh_lib.DEFAULT_STRENGTH), ("crossing", dh_lib.CROSSING_STRENGTH),
                                         ("identity", dh_lib.IDENTITY_STRENGTH), ("empty", ()), ("linear", (0.0,)),
                                         ("linear-with-points", (0.0, 0.0, 0.9, 0.0, 0.0, 1.0, 0.9, 0.0, 0.0))])
def test_library_strength_lut_matches_checker(name, points):
    from art_amd import capi
    got, want = capi.dehaze_strength_lut(points), dh_lib.strength_lut(points)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    if name == "default":
        assert np.all(got == np.float32((0.75 - 0.5) * np.float64(np.float32(1.3))))
    elif name == "crossing":
        assert got.min() < 0 < got.max()
    else:
        assert not got.any()


def _thumb(w, h, seed):
    img = dh_lib.hazy_scene(w, h, seed=seed, zero_block=True, bright_block=True)
    return [a / np.float32(131070.0) for a in img]


@pytest.mark.parametrize("w,h", [(200, 150), (300, 200), (200, 21)])
def test_library_ambient_estimate_matches_checker(w, h):
    from art_amd import capi
    R, G, B = _thumb(w, h, seed=w + h)
    got_a, got_t = capi.dehaze_estimate_ambient(R, G, B)
    want_a, want_t = dh_lib.estimate_ambient(R, G, B)
    assert np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32)), (got_a, want_a)
    assert got_t.view(np.uint32) == want_t.view(np.uint32) and got_t > 0
    assert np.all(got_a > 0.1) and np.all(got_a < 0.6)


def test_ambient_estimate_reports_no_haze():
    from art_amd import capi
    R, G, B = _thumb(200, 150, seed=9)
    G = -np.abs(G) - np.float32(0.01)          # the dark channel is negative everywhere
    got_a, got_t = capi.dehaze_estimate_ambient(R, G, B)
    want_a, want_t = dh_lib.estimate_ambient(R, G, B)
    assert got_t < 0 and want_t < 0 and not got_a.any() and not want_a.any()


def test_thumbnail_size_rule():
    assert dh_lib.thumb_size(723, 481) == (200, 133)
    assert dh_lib.thumb_size(481, 723) == (300, 200)          # portrait: ww = 200 / r is the larger number
    assert dh_lib.thumb_size(7801, 41) == (200, 1)


def test_checker_hand_in_values_are_used():
    img, kw, own, info, _ = dh_lib.case("300x200-default")
    again, info2, _ = dh_lib.dehaze(img, hand=dh_lib.hand_from(info), **kw)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(own, again))
    assert dh_lib.info_fields(info2) == dh_lib.info_fields(info)
    hd = dh_lib.hand_from(info)
    hd.ambient[1] = np.float32(info.ambient[1]) * np.float32(0.8)
    hd.max_t = np.float32(info.max_t) * np.float32(1.5)
    moved, info3, _ = dh_lib.dehaze(img, hand=hd, **kw)
    assert info3.ambient[1] == hd.ambient[1] and info3.max_t == hd.max_t and info3.t0 < info.t0
    assert not np.array_equal(own[1], moved[1])
    hd = dh_lib.hand_from(info)
    hd.maxval = np.float32(info.maxval) * np.float32(2.0)
    scaled, info4, _ = dh_lib.dehaze(img, hand=hd, **kw)
    assert info4.maxval == hd.maxval and not np.array_equal(own[0], scaled[0])
    # black is only read with a black point
    img, kw, own, info, _ = dh_lib.case("723x481-crossing-black50-depth100")
    assert all(info.black[k] > 0 for k in range(3))
    hd = dh_lib.hand_from(info)
    hd.black[2] = np.float32(0.0)
    moved, info5, _ = dh_lib.dehaze(img, hand=hd, **kw)
    assert info5.black[2] == 0.0 and not np.array_equal(own[2], moved[2])


def test_checker_changes_the_image_and_removes_haze():
    img, kw, out, info, _ = dh_lib.case("300x200-default")
    assert info.haze_detected == 1 and info.patchsize == 2 and (info.small_w, info.small_h) == (200, 133)
    assert info.maxval == 65535.0 and max(a.max() for a in img) < 32768        # normalize's floor
    big = dh_lib.case("7801x41-patch13")
    assert big[3].maxval == np.float32(2.0) * max(a.max() for a in big[0]) > 65535.0
    assert all(not np.array_equal(a, b) for a, b in zip(img, out))
    # (rgb - A) / t + A with t < 1 spreads the values around the ambient light: more contrast where the haze is (top right)
    assert out[1][:40, -60:].std() > 1.1 * img[1][:40, -60:].std()


def test_depth_map_lies_in_0_maxval():
    img, kw, out, info, counts = dh_lib.case("1803x97-depthmap-scale2")
    assert info.patchsize == 3
    for a in out:
        assert a.min() >= 0.0 and a.max() <= info.maxval
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[1], out[2]) and out[0].max() > out[0].min()


def test_unsupported_aspect_with_black_point():
    img = dh_lib.hazy_scene(1803, 97, seed=7)
    assert dh_lib.dehaze(img, blackpoint=50) is None and dh_lib.dehaze(img, blackpoint=0) is not None


def test_cases_take_every_branch():
    """a green comparison is not one that skipped a branch: the checker's counts over the GPU cases"""
    total = {}
    for name in dh_lib.CASES:
        for k, v in dh_lib.case(name)[4].items():
            total[k] = total.get(k, 0) + v
    for k in ("add_haze", "y_small", "won_t", "won_t0", "won_tl", "dark_clipped_high", "partial_patches"):
        assert total[k] > 0, (k, total)
    assert total["no_haze"] == 0
    assert dh_lib.case("481x723-luminance")[4]["y_small"] > 0 and dh_lib.case("481x723-luminance")[4]["add_haze"] > 0
    assert dh_lib.case("723x481-crossing-black50-depth100")[4]["add_haze"] > 0
    c = dh_lib.case("300x200-strong-depth0")[4]
    assert c["won_t"] == 0 and c["won_t0"] > 0 and c["won_tl"] > 0           # t0 = 1: only the zero block's tl + teps is larger
    assert dh_lib.case("723x481-crossing-black50-depth100")[4]["partial_patches"] > 0        # 723 = 361 * 2 + 1
    assert dh_lib.case("7801x41-patch13")[3].patchsize == 13 and dh_lib.case("7801x41-patch13")[4]["partial_patches"] > 0


def test_dehaze_kernels_have_no_scratch_and_no_spills():
    """the resources of the new kernels in the built gfx950 code object (art_amd/codeobj.py, as tests/test_kernel_resources.py reads them)"""
    pytest.importorskip("msgpack")
    from art_amd import codeobj
    table = codeobj.kernel_table(os.path.join(ROOT, "art_amd", "libartgpu.so"))
    mine = {k: v for k, v in table.items() if "dh_" in k and "_kernel" in k}
    for fam in ("dh_max_partial_kernel", "dh_max_final_kernel", "dh_thumb_kernel", "dh_black_kernel", "dh_normalize_kernel", "dh_restore_kernel",
                "dh_gf_subsample_kernel", "dh_gf_ab_kernel", "dh_dark_kernel<true>", "dh_dark_kernel<false>", "dh_expand_kernel",
                "dh_transmission_kernel", "dh_recover_kernel"):
        assert any(fam in k for k in mine), (fam, sorted(mine))
    for name, r in mine.items():
        assert r["scratch_bytes"] == 0 and r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0, (name, r)
        assert r["vgprs"] <= 128, (name, r)          # 256-thread workgroups: eight of them fit a CU's register file
