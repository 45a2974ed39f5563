"""GPU: artgpu_resize_lanczos (ImProcFunctions::Lanczos, ipresize.cc:53-223) against the CPU checker (tests/rs_lib.py: tests/emul/resize_ref.cc
around the oracle's mode switches).  Every value is compared as a bit pattern; a NaN equals a NaN whatever its payload.  The scenes and
the branches they take are listed in rs_lib and checked from the checker's counters in test_resize_checker.py.

The launch geometry the sizes are chosen for (art_amd/csrc/resize.h, mirrored by rs_lib.ROWS / SPAN / tile_width): a workgroup of 256 lanes
produces 16 destination rows of tile_w destination columns, tile_w being the largest count whose horizontal taps lie within 256 source
columns (about 121 at scale 0.5, 25 at 1/8, 990 at 4)."""
import ctypes as C

import numpy as np
import pytest
import torch

from art_amd import capi
import layout_lib
import oracle_lib as O
import rs_lib

pytestmark = pytest.mark.gpu

DOWN = (0.5, 1 / 3, 0.37, 0.8, 1 / 8)
UP = (1.5, 2.0, 4.0)


def _dev(planes):
    return [torch.from_numpy(np.array(a, dtype=np.float32)).to("cuda:0") for a in planes]


def _rgb(tensors):
    return capi.RGB(*[capi.device_plane(t) for t in tensors])


def _device(ctx, img, dw, dh, scale, mode=rs_lib.PLANES):
    s = _dev(img)
    d = [torch.full((dh, dw), float("nan"), device="cuda:0") for _ in range(3)]
    ctx.resize_lanczos(_rgb(s), _rgb(d), scale, mode, O.REC2020_WS_D, O.REC2020_IWS_D)
    ctx.synchronize()
    return [t.cpu().numpy() for t in d]


def _check(ctx, w, h, dw, dh, scale, mode=rs_lib.PLANES, families=rs_lib.FAMILIES):
    for fam in families:
        img, want, _ = rs_lib.case(w, h, dw, dh, scale, mode, fam)
        rs_lib.assert_same(_device(ctx, img, dw, dh, scale, mode), want, f"{w}x{h} -> {dw}x{dh} at {scale:g}, mode {mode}, {fam}")


@pytest.mark.parametrize("case", [(1, 1, 1, 1, 0.7), (3, 2, 1, 1, 0.4)], ids=lambda c: "%dx%d" % c[:2])
def test_every_tap_clipped(gpu_ctx, case):
    """1 x 1 -> 1 x 1 and 3 x 2 -> 1 x 1: sW < 4, every range cut on both sides"""
    _check(gpu_ctx, *case)
    _check(gpu_ctx, *case, mode=rs_lib.RGB, families=rs_lib.RGB_FAMILIES)


@pytest.mark.parametrize("scale", DOWN, ids=lambda s: "%.4g" % s)
@pytest.mark.parametrize("size", [(67, 45), (131, 70)], ids=lambda s: "%dx%d" % s)
def test_downscales_equal_the_checker(gpu_ctx, size, scale):
    """both modes; super-white, negative and subnormal planes, an inf of either sign in one pixel each (where their taps meet: NaN)"""
    w, h = size
    dw, dh = rs_lib.dst_size(w, h, scale)
    _check(gpu_ctx, w, h, dw, dh, scale)
    _check(gpu_ctx, w, h, dw, dh, scale, mode=rs_lib.RGB, families=rs_lib.RGB_FAMILIES)


@pytest.mark.parametrize("scale", UP, ids=lambda s: "%.4g" % s)
def test_upscales_equal_the_checker(gpu_ctx, scale):
    w, h = 23, 17
    dw, dh = rs_lib.dst_size(w, h, scale)
    _check(gpu_ctx, w, h, dw, dh, scale)
    _check(gpu_ctx, w, h, dw, dh, scale, mode=rs_lib.RGB, families=rs_lib.RGB_FAMILIES)


@pytest.mark.parametrize("extra", (1, 2, 4, 5))
def test_destination_larger_than_the_scale_implies(gpu_ctx, extra):
    """one and two pixels more cut the last ranges; four and five more leave columns and rows without a tap: 0.0f.  Also at 1/7, where float
    rounding puts taps into Lanc's zero branch, and for an upscale"""
    w, h, s = 67, 45, 0.5
    dw, dh = rs_lib.dst_size(w, h, s)
    counts = rs_lib.case(w, h, dw + extra, dh + extra, s)[2]
    assert (counts["empty_cols"] > 0 and counts["empty_rows"] > 0) == (extra >= 4)
    _check(gpu_ctx, w, h, dw + extra, dh + extra, s)
    _check(gpu_ctx, w, h, dw + extra, dh + extra, s, mode=rs_lib.RGB, families=("plain",))
    if extra == 5:
        dw, dh = rs_lib.dst_size(w, h, 1 / 7)
        assert rs_lib.case(w, h, dw, dh, 1 / 7)[2]["lanc_zero"] > 0
        _check(gpu_ctx, w, h, dw, dh, 1 / 7)
        _check(gpu_ctx, 23, 17, 23 * 2 + 16, 17 * 2 + 14, 2.0, families=("plain", "inf_pixel"))


# (w, h, scale): at least two tile boundaries in each direction of the geometry the library chooses (16 rows x tile_w columns)
TILE_CASES = ((520, 80, 0.5), (480, 300, 1 / 8), (520, 110, 0.37), (520, 10, 4.0))


@pytest.mark.parametrize("case", TILE_CASES, ids=lambda c: "%dx%d@%.3g" % c)
def test_sizes_that_cross_tile_boundaries(gpu_ctx, case):
    w, h, s = case
    dw, dh = rs_lib.dst_size(w, h, s)
    tw = rs_lib.tile_width(w, dw, s)
    assert tw >= 8 and (dw - 1) // tw >= 2 and (dh - 1) // rs_lib.ROWS >= 2, (dw, dh, tw)
    _check(gpu_ctx, w, h, dw, dh, s, families=("scaled_frac", "inf_pixel"))
    _check(gpu_ctx, w, h, dw, dh, s, mode=rs_lib.RGB, families=("plain",))


@pytest.mark.parametrize("case", [(67, 45, 0.37), (3, 2, 0.4), (23, 17, 1.5)], ids=lambda c: "%dx%d@%.3g" % c)
def test_host_planes_give_the_same_bits(gpu_ctx, case):
    """host src and host dst; host src and device dst; device src and host dst"""
    w, h, s = case
    dw, dh = (1, 1) if w == 3 else rs_lib.dst_size(w, h, s)
    for mode, fam in ((rs_lib.PLANES, "inf_pixel"), (rs_lib.RGB, "scaled_frac")):
        img, want, _ = rs_lib.case(w, h, dw, dh, s, mode, fam)
        for src_host, dst_host in ((True, True), (True, False), (False, True)):
            hs = [np.array(a, dtype=np.float32) for a in img]
            ds = _dev(img)
            hd = [np.full((dh, dw), np.nan, np.float32) for _ in range(3)]
            dd = [torch.full((dh, dw), float("nan"), device="cuda:0") for _ in range(3)]
            gpu_ctx.resize_lanczos(capi.host_rgb(hs) if src_host else _rgb(ds), capi.host_rgb(hd) if dst_host else _rgb(dd), s, mode,
                                   O.REC2020_WS_D, O.REC2020_IWS_D)
            gpu_ctx.synchronize()
            rs_lib.assert_same(hd if dst_host else [t.cpu().numpy() for t in dd], want, f"{case} mode {mode} host src {src_host} dst {dst_host}")
            if src_host:      # a host source is read, never written
                rs_lib.assert_same(hs, img, "host src")


@pytest.mark.parametrize("layout", list(layout_lib.LAYOUTS))
def test_padded_and_shifted_device_planes(gpu_ctx, layout):
    """row-padded, offset planes for src and for dst: every word outside dst's window still holds the poison, and nothing outside src's window
    reaches a result (the poison is a NaN)"""
    lay = layout_lib.LAYOUTS[layout]
    for w, h, s, mode, fam in ((67, 45, 0.37, rs_lib.PLANES, "scaled_frac"), (131, 70, 1 / 8, rs_lib.RGB, "plain"), (23, 17, 1.5, rs_lib.PLANES, "dark_offset"),
                               (400, 110, 0.37, rs_lib.PLANES, "plain")):
        dw, dh = rs_lib.dst_size(w, h, s)
        img, want, _ = rs_lib.case(w, h, dw, dh, s, mode, fam)
        src, dst = layout_lib.arena(lay, img), layout_lib.arena(lay, (dh, dw))
        gpu_ctx.resize_lanczos(src.rgb, dst.rgb, s, mode, O.REC2020_WS_D, O.REC2020_IWS_D)
        gpu_ctx.synchronize()
        rs_lib.assert_same(layout_lib.check(dst, f"dst {dw}x{dh} {layout}"), want, f"{w}x{h} at {s:g}, layout {layout}")
        assert layout_lib.stray(src, "src") is None
        if mode == rs_lib.PLANES:
            rs_lib.assert_same(layout_lib.contents(src), img, "src in PLANES mode is not written")


def test_unsupported_and_degenerate_scales_are_refused_and_dst_untouched(gpu_ctx):
    img = rs_lib.scene(600, 45)         # (1/32 of a source no wider than 256 columns would fit the geometry: every tap lies within them)
    s = _dev(img)
    for host_dst in (False, True):
        for scale, code, word in ((1.0, -1, "scale"), (float("nan"), -1, "scale"), (float("inf"), -1, "scale"), (0.0, -1, "scale"), (-0.5, -1, "scale"),
                                  (1 / 32, -4, "source columns"), (1e-3, -4, "taps")):
            d = [torch.full((6, 9), 7.0, device="cuda:0") for _ in range(3)]
            hd = [np.full((6, 9), 7.0, np.float32) for _ in range(3)]
            with pytest.raises(capi.ArtGpuError, match=r"^\[%d\].*%s" % (code, word)):
                gpu_ctx.resize_lanczos(_rgb(s), capi.host_rgb(hd) if host_dst else _rgb(d), scale)
            gpu_ctx.synchronize()
            assert all((t.cpu().numpy() == 7.0).all() for t in d) and all((a == 7.0).all() for a in hd), scale
    d = [torch.full((6, 9), 7.0, device="cuda:0") for _ in range(3)]
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\].*mode"):
        gpu_ctx.resize_lanczos(_rgb(s), _rgb(d), 0.5, 2)
    with pytest.raises(capi.ArtGpuError, match=r"^\[-1\].*ws"):
        gpu_ctx.resize_lanczos(_rgb(s), _rgb(d), 0.5, rs_lib.RGB)
    assert all((t.cpu().numpy() == 7.0).all() for t in d)
    rs_lib.assert_same([t.cpu().numpy() for t in s], img, "src after refused calls")
    # 1/16 is supported (the header's promise): eight columns' taps lie within 256 source columns
    w, h = 300, 40
    dw, dh = rs_lib.dst_size(w, h, 1 / 16)
    _check(gpu_ctx, w, h, dw, dh, 1 / 16, families=("plain",))


def test_table_cache_two_sizes_then_the_first_again(gpu_ctx):
    a = (67, 45) + rs_lib.dst_size(67, 45, 0.37) + (0.37,)
    b = (131, 70) + rs_lib.dst_size(131, 70, 0.5) + (0.5,)
    c = (67, 45) + rs_lib.dst_size(67, 45, 0.37) + (1 / 3,)          # the sizes of `a` at another scale: the scale is part of the key
    for case in (a, a, b, a, c, a, b):
        w, h, dw, dh, s = case
        img, want, _ = rs_lib.case(w, h, dw, dh, s, rs_lib.PLANES, "scaled_frac")
        rs_lib.assert_same(_device(gpu_ctx, img, dw, dh, s), want, f"{case}")
    # ... and after the scratch pool is given back, the tables are uploaded again
    gpu_ctx.trim_scratch()
    w, h, dw, dh, s = b
    img, want, _ = rs_lib.case(w, h, dw, dh, s, rs_lib.PLANES, "scaled_frac")
    rs_lib.assert_same(_device(gpu_ctx, img, dw, dh, s), want, "after trim_scratch")
