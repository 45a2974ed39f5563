"""CPU: the texture-boost checker (tests/emul/textureboost_ref.cc: texture_boost and the region loop restated around the oracle's guided filter,
bilinear rescale, pow_F and YUV switch), the parameters it derives, its gaussian kernel and the distance of its fp32 convolution from the exact
one, and the new symbols of the C ABI.  No GPU."""
import numpy as np
import pytest

import tb_lib

U = 2.0 ** -24          # fp32 unit roundoff


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_abi_exports_texture_boost():
    from art_amd import capi
    for sym in ("artgpu_texture_boost_plane", "artgpu_texture_boost"):
        assert sym in capi.EXPORTS and hasattr(capi.LIB, sym), sym
    assert dict(capi.PipelineParams._fields_)["texture_boost_regions"] is not None
    assert [n for n, _ in capi.PipelineParams._fields_][-3:] == ["texture_boost_enabled", "texture_boost_nregions", "texture_boost_regions"]
    assert C_sizeof(capi.TextureBoostInfo) == C_sizeof(tb_lib.Info) and C_sizeof(capi.TextureBoostRegion) == C_sizeof(tb_lib.Region)


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_checker_builds_and_is_deterministic():
    Y = tb_lib.textured_plane(67, 41, seed=3, low=True)
    for thr in (0.2, 1.0):
        a, ia, ca = tb_lib.texture_boost_plane(Y, 1.0, thr, iterations=2)
        b, ib, cb = tb_lib.texture_boost_plane(Y, 1.0, thr, iterations=2)
        assert np.array_equal(_bits(a), _bits(b)) and tb_lib.info_fields(ia) == tb_lib.info_fields(ib) and ca == cb
        assert not np.array_equal(a, Y) and np.isfinite(a).all()
    img, regions, to_rgb, want, info, counts = tb_lib.tool_case("130x97-two-regions-rgb")
    again, info2, counts2 = tb_lib.texture_boost(img, regions, to_rgb=to_rgb)
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(want, again)) and counts == counts2


def test_cases_take_every_branch():
    """a green comparison is not one that skipped a branch: the checker's counts over the GPU cases"""
    total = dict.fromkeys(tb_lib.COUNTERS, 0)
    for name in tb_lib.PLANE_CASES:
        for k, v in tb_lib.plane_case(name)[4].items():
            total[k] += v
    for name in tb_lib.TOOL_CASES:
        for k, v in tb_lib.tool_case(name)[5].items():
            total[k] += v
    for k in tb_lib.COUNTERS:
        assert total[k] > 0, (k, total)
    # where each one comes from
    assert tb_lib.plane_case("130x97-t0.2-high")[4]["clamp_high"] > 0 and tb_lib.plane_case("130x97-t1-high")[4]["clamp_high"] > 0
    for name in ("67x41-t0.3-low", "130x97-t0.2-low-it3"):
        c = tb_lib.plane_case(name)[4]
        assert c["clamp_low"] > 0 and c["minval_won"] > 0, (name, c)
        assert tb_lib.plane_case(name)[3].minval < 0
    assert tb_lib.plane_case("67x41-t1")[4]["tail_columns"] == 47 * (77 % 4)             # the tail is that of the 77 x 47 working plane
    assert tb_lib.plane_case("67x41-t2")[4]["tail_columns"] == 41 * (67 % 4)
    assert tb_lib.plane_case("130x97-t0.43-neg-it3")[4] == dict(tb_lib.plane_case("130x97-t0.43-neg-it3")[4], rescale=1, guided=3, convolution=0)
    assert tb_lib.plane_case("130x97-t0.2-neg-it3")[4]["convolution"] == 3
    assert tb_lib.tool_case("130x97-two-regions-rgb")[5]["mask_partial"] > 0
    c = tb_lib.tool_case("67x41-all-zero")[5]
    assert c["guided"] == 0 and c["convolution"] == 0 and c["mask_partial"] == 0          # no region ran


@pytest.mark.parametrize("threshold,K,guided,rescaled,radius", tb_lib.THRESHOLDS)
def test_derived_parameters(threshold, K, guided, rescaled, radius):
    """L39-63 and build_gaussian_kernel by hand, at scale 1 on 67 x 41:
       0.01 -> sigma 0.035: 1 + 2 * sqrt(2 * sigma^2 * 5.2983) = 1.23 -> (1 + 1) | 1 = 3;   0.2 -> 0.7: 5.56 -> 7;   0.28 -> 0.98: 7.38 -> 9;
       0.3 -> 1.05: radius 1, delta 0.95 (no rescale);   0.43 -> 1.505: radius 2, delta 1.329;   1.0 -> 3.5: radius 4, delta 1.143;
       2.0 -> 7.0: radius int(7.5) = 7, delta 1"""
    info = tb_lib.plane_case("67x41-t%g" % threshold)[3]
    assert (info.kernel_size, info.isguided, info.rescaled, info.radius) == (K, guided, rescaled, radius)
    fr = np.float32(np.float64(threshold) * np.float64(np.float32(3.5)))
    delta = np.float32(radius) / fr
    want = (int(np.float32(67) * delta + np.float32(0.5)), int(np.float32(41) * delta + np.float32(0.5))) if rescaled else (67, 41)
    assert (info.work_w, info.work_h) == want
    if threshold == 0.43:
        assert want == (89, 54)         # 1.33x
    if threshold == 1.0:
        assert want == (77, 47)         # 1.14x
    # strength 1: s = pow_F(0.5, 0.3) * 2
    s = 2.0 * 0.5 ** 0.3
    assert abs(info.strength - (1 + s)) < 4 * U * (1 + s) and abs(info.strength2 - (1 + s / 4)) < 4 * U * (1 + s / 4)


def test_scale_and_negative_strength():
    info = tb_lib.plane_case("130x97-t2-scale2")[3]
    assert (info.isguided, info.radius, info.rescaled) == (1, 4, 1) and (info.work_w, info.work_h) == (149, 111)
    info = tb_lib.plane_case("130x97-t0.2-neg-it3")[3]
    assert abs(info.strength - 1 / 1.8) < 4 * U and abs(info.strength2 - 1 / 1.4) < 4 * U


@pytest.mark.parametrize("sigma,K", [(0.035, 3), (0.5, 5), (0.7, 7), (0.98, 9)])
def test_gaussian_kernel_sums_to_one_and_is_symmetric(sigma, K):
    k = tb_lib.gaussian_kernel(np.float32(sigma))
    assert k.shape == (K, K) and (k >= 0).all() and k[K // 2, K // 2] == k.max()
    # every entry is fl(val / fl(total)): two roundings against the double total, the sum here in double
    assert abs(k.astype(np.float64).sum() - 1.0) <= 3 * U
    assert np.array_equal(k, k.T)                                       # row[i] * row[j] commutes
    # x -> -x swaps the end points of Simpson's rule, whose three terms are then added in the other order
    assert np.allclose(k, k[::-1, ::-1], rtol=8 * U, atol=0)


@pytest.mark.parametrize("sigma", [0.035, 0.7, 0.98])
def test_fp32_convolution_is_within_its_rounding_bound_of_the_exact_one(sigma):
    """K * K products (one rounding each) and K * K - 1 additions of positive terms, the first one to 0.f exact: every term carries at most
    K * K roundings, so the fp32 sum is within ((1 + u)^(K*K) - 1) <= (K * K + 1) u relative of the sum in double.  That is the distance
    from the definition to the exact convolution FFTW approximates."""
    k = tb_lib.gaussian_kernel(np.float32(sigma))
    K = k.shape[0]
    Y = tb_lib.textured_plane(130, 97, seed=5, high=True, low=True)
    mid = np.clip(Y / np.float32(65535.0), np.float32(1e-5), np.float32(32.0))
    got, exact = tb_lib.conv(mid, k), tb_lib.conv(mid, k, double=True)
    assert (exact > 0).all()
    rel = np.abs(got.astype(np.float64) - exact) / exact
    assert rel.max() <= (K * K + 1) * U, (K, rel.max() / U)
    if K > 3:
        assert rel.max() > 0                                            # (the two are not the same computation; at sigma 0.035 the kernel is a delta)


def test_convolution_clamps_to_edge():
    k = tb_lib.gaussian_kernel(np.float32(0.7))
    a = np.zeros((9, 11), np.float32)
    a[0, 0] = 1.0
    got = tb_lib.conv(a, k)
    r = k.shape[0] // 2
    # the corner pixel is read for every tap that clamps onto it: the kernel's upper-left quadrant (centre row and column included)
    assert np.isclose(got[0, 0], k[r:, r:].astype(np.float64).sum(), rtol=64 * U) and got[r + 1:, :].max() == 0 and got[:, r + 1:].max() == 0
    const = np.full((9, 11), np.float32(3.25))
    assert np.allclose(tb_lib.conv(const, k), 3.25, rtol=50 * U)


def test_unsupported_cases_in_the_checker():
    Y = tb_lib.textured_plane(67, 41, seed=4)
    assert tb_lib.texture_boost_plane(Y, 1.0, 0.2, high_detail=False) is None            # gaussianBlur at a sub-pixel sigma
    assert tb_lib.texture_boost_plane(Y, 1.0, 0.3, high_detail=False) is not None
    assert tb_lib.texture_boost_plane(Y, 1.0, 0.2, iterations=0) is None
    assert tb_lib.texture_boost_plane(Y, 1.0, 0.2, scale=0.5) is None                    # sigma 1.4: an 11 x 11 gaussian
    thin = tb_lib.textured_plane(701, 3, seed=4)
    assert tb_lib.texture_boost_plane(thin, 1.0, 2.0) is None                            # 3 / 4 rows for the radius-28 filter
    assert tb_lib.texture_boost_plane(thin, 1.0, 0.3) is None and tb_lib.texture_boost_plane(thin[:, :600], 1.0, 0.3) is not None


def test_smallest_planes():
    """both sides >= MIN_SIZE is always accepted; one row less above 600 is not (5 is the largest subsampling)"""
    for name in ("5x5-t0.2", "5x5-t2", "605x5-t1.43"):
        Y, kw, want, info, _ = tb_lib.plane_case(name)
        assert np.isfinite(want).all() and not np.array_equal(want, Y), name
    assert tb_lib.plane_case("605x5-t1.43")[3].radius == 5 and tb_lib.plane_case("605x5-t1.43")[3].rescaled == 0
    thin = tb_lib.textured_plane(605, tb_lib.MIN_SIZE - 1, seed=18)
    assert tb_lib.texture_boost_plane(thin, 1.0, 1.43) is None


@pytest.mark.parametrize("threshold", [0.2, 0.3])
def test_nan_pixel_lands_by_column(threshold):
    """the reference clamps with vmaxf(vminf(v, hi), lo) in its 4-wide body and with LIM in the tail: a NaN becomes 32 there and 1e-5 here in
    `mid`, which its neighbours then see; the pixel itself stays NaN"""
    Y = tb_lib.nan_plane(67, 41, seed=30)
    out, info, _ = tb_lib.texture_boost_plane(Y, 1.0, threshold)
    assert info.minval == np.float32(100.0) / np.float32(65535.0)
    assert np.isnan(out[20, 20]) and np.isnan(out[37, 66]) and np.isnan(out).sum() == 2
    clean = np.array(Y)
    clean[20, 20], clean[37, 66] = Y[20, 19], Y[37, 65]
    ref = tb_lib.texture_boost_plane(clean, 1.0, threshold)[0]
    # mid = 32 next to values around 0.15 pushes the neighbours of the body's NaN down; mid = 1e-5 moves the tail's neighbours as well
    assert out[20, 21] < ref[20, 21] - 100.0 and out[37, 65] != ref[37, 65]


def test_all_zero_strength_is_the_yuv_round_trip_not_the_input():
    img, regions, to_rgb, want, info, _ = tb_lib.tool_case("67x41-all-zero")
    assert tb_lib.info_fields(info) == (0,) * 9
    assert any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(img, want))
    assert all(np.allclose(a, b, rtol=1e-5, atol=1e-2) for a, b in zip(img, want))
