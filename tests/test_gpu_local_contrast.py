"""GPU: artgpu_local_contrast (ImProcFunctions::localContrast, iplocalcontrast.cc:251-487) against the CPU checker
(tests/lc_lib.py: tests/emul/local_contrast_ref.cc around the oracle's wavelet).

Statistics: min0, max0, MaxP and the level count must equal the checker's serial-order values; ave, mean and sigma are double sums of
the same terms in another fixed order, so one float ulp is accepted on at most one of those values per case.
Image: with the device's own statistics handed to the checker the result is bit-identical, and wherever the statistics matched
exactly it is also bit-identical to the checker's own-statistics result."""
import functools

import numpy as np
import pytest
import torch

from art_amd import capi, synth
import lc_lib
from test_gpu_cli import MAT, MUL, run_cli, tone_lut
from test_gpu_pipeline import _lut, _params

pytestmark = pytest.mark.gpu

# a hand-made LUT with entries below -0.5 (kc < -1: the 0.01 floor) and above 0.5
_x = np.arange(501, dtype=np.float64) / 500.0
FLOOR_LUT = (0.5 + 1.3 * np.sin(2 * np.pi * _x * 1.5)).astype(np.float32)
assert FLOOR_LUT.min() < -0.5

CURVES = {"boost": lc_lib.curve_lut(lc_lib.BOOST_CURVE_POINTS), "cut": lc_lib.curve_lut(lc_lib.CUT_CURVE_POINTS), "floor": FLOOR_LUT,
          "default": lc_lib.curve_lut(lc_lib.DEFAULT_CURVE_POINTS), "unset": None}
# name: (w, h, seed, contrast, curve, highlight patch, flat value, levels)
CASES = {
    "131x129-boost+60": (131, 129, 1, 60.0, "boost", False, None, 7),
    "129x200-cut-40": (129, 200, 2, -40.0, "cut", False, None, 7),
    "128x97-boost0": (128, 97, 3, 0.0, "boost", False, None, 6),
    "128x97-unset+60": (128, 97, 4, 60.0, "unset", False, None, 6),
    "64x90-floor+60": (64, 90, 5, 60.0, "floor", False, None, 5),
    "515x389-boost-40-highlight": (515, 389, 6, -40.0, "boost", True, None, 7),
    "515x389-cut+60": (515, 389, 7, 60.0, "cut", False, None, 7),
    "64x90-flat0": (64, 90, 0, 0.0, "cut", False, 12000.0, 5),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """the case's plane and the checker's own-statistics run, computed once"""
    w, h, seed, contrast, curve, highlight, flat, nl = CASES[name]
    L = lc_lib.l_plane(w, h, seed=seed, highlight=highlight, flat=flat)
    L.setflags(write=False)
    want, info, counts = lc_lib.local_contrast_wavelets(L, contrast, CURVES[curve])
    want.setflags(write=False)
    return L, contrast, CURVES[curve], want, info, counts, nl


def _device(ctx, L, regions, stride_pad=0, scale=1.0):
    """artgpu_local_contrast on a device-resident copy of L (rows stride_pad floats longer than w); returns (plane, info)"""
    h, w = L.shape
    buf = torch.full((h, w + stride_pad), float("nan"), dtype=torch.float32, device="cuda:0")
    d = buf[:, :w]
    d.copy_(torch.from_numpy(np.array(L, dtype=np.float32)))
    info = ctx.local_contrast(capi.device_plane(d), regions, scale, want_info=True)
    ctx.synchronize()
    if stride_pad:
        assert bool(torch.isnan(buf[:, w:]).all()), "wrote past the row"
    return d.cpu().numpy(), info


def _ulps(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def _compare_info(got, want):
    """asserts the equalities, returns the list of (name, ulps) of ave / mean / sigma values that differ"""
    g, w = lc_lib.info_tuple(got), lc_lib.info_tuple(want)
    assert g[0] == w[0], ("nlevels", g[0], w[0])
    assert g[2] == w[2] and g[3] == w[3], ("min0 / max0", g[2:4], w[2:4])
    assert np.array_equal(g[6], w[6]), ("maxp", g[6], w[6])
    off = []
    for name, a, b in (("ave", [g[1]], [w[1]]), ("mean", g[4], w[4]), ("sigma", g[5], w[5])):
        for k, u in enumerate(_ulps(a, b)):
            if u:
                off.append((f"{name}[{k}]", int(u)))
    return off


@pytest.mark.parametrize("name", list(CASES))
def test_statistics_and_image(gpu_ctx, name):
    L, contrast, curve, want, want_info, counts, nl = _case(name)
    got, info = _device(gpu_ctx, L, [(contrast, curve, None)])
    assert info.nlevels == nl
    off = _compare_info(info, want_info)
    print(f"local contrast {name}: values off the serial-order statistics: {off if off else 'none'}")
    assert len(off) <= 1 and all(u <= 1 for _, u in off), off
    if contrast == 0:
        assert info.ave == 0.0 and info.min0 == 0.0 and info.max0 == 0.0
    # the device's own statistics handed to the checker: the same bits
    fed, _, _ = lc_lib.local_contrast_wavelets(L, contrast, curve, stats=lc_lib.copy_info(info))
    assert np.array_equal(got.view(np.uint32), fed.view(np.uint32)), int((got.view(np.uint32) != fed.view(np.uint32)).sum())
    if not off:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    if CASES[name][6] is None:
        assert not np.array_equal(got, lc_lib.plain_round_trip(L)), "the call changed nothing"


def test_cases_take_every_branch():
    """a green run is not a run that skipped a branch: the checker's counts over the cases"""
    total = {}
    for name in CASES:
        for k, v in _case(name)[5].items():
            total[k] = total.get(k, 0) + v
    for k in ("branch_max", "branch_mid", "branch_low", "clipped_above", "floor_hits", "c0_skipped", "levels_skipped"):
        assert total[k] > 0, (k, total)
    assert _case("64x90-floor+60")[5]["floor_hits"] > 0
    assert _case("515x389-boost-40-highlight")[5]["c0_skipped"] > 0
    flat = _case("64x90-flat0")
    assert flat[5]["levels_skipped"] == 5 and flat[5]["branch_low"] == 0        # MaxP == 0: the band loop is skipped
    for name in ("131x129-boost+60", "515x389-cut+60"):                         # coefficients on both sides of 5 at every level
        info = _case(name)[4]
        assert all(info.maxp[k] > 0 and info.sigma[k] > 0 for k in range(info.nlevels))


def test_two_regions_masked_on_a_strided_device_plane(gpu_ctx):
    w, h = 131, 129
    L = lc_lib.l_plane(w, h, seed=11)
    ramp = np.ascontiguousarray(np.broadcast_to(np.linspace(0.0, 1.0, w, dtype=np.float32), (h, w)))
    d_mask = torch.from_numpy(ramp).to("cuda:0")
    regions = [(60.0, CURVES["boost"], None), (-40.0, CURVES["cut"], capi.device_plane(d_mask))]
    got, info = _device(gpu_ctx, L, regions, stride_pad=13)
    # region by region on the device: the same bits, and the statistics of both regions for the checker
    one, i1 = _device(gpu_ctx, L, regions[:1], stride_pad=5)
    two, i2 = _device(gpu_ctx, one, regions[1:])
    assert np.array_equal(got.view(np.uint32), two.view(np.uint32))
    assert lc_lib.info_tuple(info)[:4] == lc_lib.info_tuple(i2)[:4] and all(np.array_equal(a, b) for a, b in zip(lc_lib.info_tuple(info)[4:], lc_lib.info_tuple(i2)[4:]))
    host_regions = [(60.0, CURVES["boost"], None), (-40.0, CURVES["cut"], ramp)]
    fed, _, _ = lc_lib.local_contrast(L, host_regions, stats=[lc_lib.copy_info(i1), lc_lib.copy_info(i2)])
    assert np.array_equal(got.view(np.uint32), fed.view(np.uint32))
    own, infos, _ = lc_lib.local_contrast(L, host_regions)
    if not _compare_info(i1, infos[0]) and not _compare_info(i2, infos[1]):
        assert np.array_equal(got.view(np.uint32), own.view(np.uint32))
    assert np.array_equal(got[:, 0].view(np.uint32), one[:, 0].view(np.uint32))      # mask 0: the second region leaves the column alone
    assert not np.array_equal(got[:, -1], one[:, -1])


def test_host_plane_and_host_mask_equal_the_device_plane(gpu_ctx):
    w, h = 129, 200
    L = lc_lib.l_plane(w, h, seed=12)
    mask = np.ascontiguousarray(np.broadcast_to(np.linspace(1.0, 0.0, h, dtype=np.float32)[:, None], (h, w)))
    d_mask = torch.from_numpy(mask).to("cuda:0")
    want, want_info = _device(gpu_ctx, L, [(60.0, CURVES["cut"], capi.device_plane(d_mask))])
    buf = np.full((h, w + 3), np.nan, np.float32)
    host = buf[:, :w]
    host[:] = L
    info = gpu_ctx.local_contrast(capi.host_plane(host), [(60.0, CURVES["cut"], capi.host_plane(mask))], want_info=True)
    assert np.array_equal(host.view(np.uint32), want.view(np.uint32)) and np.isnan(buf[:, w:]).all()
    assert bytes(info) == bytes(want_info)


def test_same_call_twice_same_bits(gpu_ctx):
    L, contrast, curve = _case("515x389-cut+60")[:3]
    a, ia = _device(gpu_ctx, L, [(contrast, curve, None)])
    b, ib = _device(gpu_ctx, L, [(contrast, curve, None)], stride_pad=9)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and bytes(ia) == bytes(ib)


def test_unsupported_leaves_the_plane_alone(gpu_ctx):
    for shape, scale in (((129, 131), 2.0), ((40, capi.LOCAL_CONTRAST_MIN_SIZE - 1), 1.0), ((capi.LOCAL_CONTRAST_MIN_SIZE - 1, 40), 1.0)):
        L = lc_lib.l_plane(shape[1], shape[0], seed=13)
        d = torch.from_numpy(L).to("cuda:0")
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
            gpu_ctx.local_contrast(capi.device_plane(d), [(60.0, CURVES["boost"], None)], scale)
        gpu_ctx.synchronize()
        assert np.array_equal(d.cpu().numpy().view(np.uint32), L.view(np.uint32))
        host = L.copy()
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
            gpu_ctx.local_contrast(capi.host_plane(host), [(60.0, CURVES["boost"], None)], scale)
        assert np.array_equal(host.view(np.uint32), L.view(np.uint32))
    # the smallest supported frame runs
    L = lc_lib.l_plane(8, 8, seed=14)
    got, info = _device(gpu_ctx, L, [(60.0, CURVES["boost"], None)])
    assert info.nlevels == lc_lib.levels(8, 8) == 2 and np.isfinite(got).all()
    fed, _, _ = lc_lib.local_contrast_wavelets(L, 60.0, CURVES["boost"], stats=lc_lib.copy_info(info))
    assert np.array_equal(got.view(np.uint32), fed.view(np.uint32))


def test_trim_scratch_returns_the_band_storage(gpu_ctx):
    L = _case("515x389-cut+60")[0]
    gpu_ctx.trim_scratch()
    before = gpu_ctx.scratch_bytes()
    _device(gpu_ctx, L, [(60.0, CURVES["cut"], None)])
    n2 = ((515 + 1) // 2) * ((389 + 1) // 2)
    assert gpu_ctx.scratch_bytes() - before >= (21 + 2) * n2 * 4 + 515 * 389 * 4
    gpu_ctx.trim_scratch()
    assert gpu_ctx.scratch_bytes() == before


def _pipeline(ctx, raw, p):
    h, w = raw.shape
    b = p.border
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    ctx.synchronize()
    return d_img


def test_pipeline_flag_equals_the_stages(gpu_ctx):
    w, h = 520, 392
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=21, noise=1500)
    lut = _lut()
    plain = _pipeline(gpu_ctx, raw, _params(lut, 0))
    mask = np.ascontiguousarray(np.broadcast_to(np.linspace(0.0, 1.0, w - 8, dtype=np.float32), (h - 8, w - 8)))
    regions = [(40.0, CURVES["boost"], None), (-30.0, CURVES["cut"], capi.host_plane(mask))]
    arr, keep = capi.local_contrast_regions(regions)
    p = _params(lut, 0)
    p.local_contrast_enabled = 1; p.local_contrast_nregions = len(regions); p.local_contrast_regions = arr
    got = _pipeline(gpu_ctx, raw, p)
    # flag zero (regions still set): today's output
    q = _params(lut, 0)
    q.local_contrast_nregions = len(regions); q.local_contrast_regions = arr
    off = _pipeline(gpu_ctx, raw, q)
    for a, b in zip(off, plain):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the stages one by one on the plain output
    img = capi.RGB(*[capi.device_plane(t) for t in plain])
    gpu_ctx.rgb_to_lab(img, p.ws[:])
    gpu_ctx.local_contrast(img.g, regions)
    gpu_ctx.lab_to_rgb(img, p.iws[:])
    gpu_ctx.synchronize()
    for a, b in zip(got, plain):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(got[1], off[1])
    del keep
    # what the stage does not support fails the frame
    p.scale = 2.0
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        _pipeline(gpu_ctx, raw, p)


def test_cli_local_contrast(gpu_ctx, tmp_path):
    """artgpu-cli --local-contrast 30 (ImProcFunctions::localContrast in the C++ mirror, one region, the default curve) equals the same
    stages called one by one"""
    w, h, filt, b = 520, 392, synth.FILTERS_RGGB, 4
    raw = synth.bayer_frame(w, h, filt, seed=22, noise=1200)
    _, got = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--local-contrast", "30"])
    _, without = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3"])
    assert not np.array_equal(got, without)
    d_raw = torch.from_numpy(raw).to("cuda:0")
    dem = [torch.empty((h, w), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    planes = capi.RGB(*[capi.device_plane(t) for t in dem])
    gpu_ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), filt, 1.0, b, planes)
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    gpu_ctx.get_image(planes, b, b, MUL, True, None, img)
    gpu_ctx.convert_color_space(img, MAT)
    gpu_ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    gpu_ctx.tone_curve(img, tone_lut(), 1.0, True)
    import oracle_lib as O
    gpu_ctx.rgb_to_lab(img, O.REC2020_WS_D)
    gpu_ctx.local_contrast(img.g, [(30.0, CURVES["default"], None)])
    gpu_ctx.lab_to_rgb(img, O.REC2020_IWS_D)
    gpu_ctx.synchronize()
    want = np.stack([np.rint(np.clip(t.cpu().numpy(), 0, 65535)).astype(np.uint16) for t in d_img], axis=-1)
    assert np.array_equal(got, want)
    # a curve on the command line: FlatCurve control points behind the contrast
    pts = ",".join(str(v) for v in lc_lib.CUT_CURVE_POINTS)
    _, got2 = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--local-contrast", "30," + pts])
    assert not np.array_equal(got2, got)
