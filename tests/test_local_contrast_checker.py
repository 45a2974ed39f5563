"""CPU: the local-contrast checker (tests/emul/local_contrast_ref.cc around the oracle's wavelet) and the library's host-side curve
table (artgpu_local_contrast_curve_lut = WavOpacityCurveWL::Set, iplocalcontrast.cc:85-94).  No GPU: libartgpu.so loads without a
device, the curve table is pure host code."""
import numpy as np
import pytest

import lc_lib
import oracle_lib as O


def test_default_curve_and_no_contrast_is_the_plain_round_trip():
    """contrast 0 and the default region's curve (0.5 everywhere): kc = 0, every kinterm is exactly 1"""
    curve = lc_lib.curve_lut(lc_lib.DEFAULT_CURVE_POINTS)
    assert curve is not None and np.all(curve == np.float32(0.5))
    L = lc_lib.l_plane(131, 129, seed=3)
    got, info, counts = lc_lib.local_contrast_wavelets(L, 0.0, curve)
    want = lc_lib.plain_round_trip(L)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert info.nlevels == 7 and info.ave == 0.0 and info.min0 == 0.0 and info.max0 == 0.0
    assert counts["floor_hits"] == 0 and counts["levels_skipped"] == 0
    assert counts["branch_max"] > 0 and counts["branch_mid"] > 0 and counts["branch_low"] > 0
    assert all(info.maxp[k] > 0 and info.mean[k] >= 5.0 and info.sigma[k] > 0 for k in range(7))


@pytest.mark.parametrize("dim,want", [(129, 7), (128, 6), (65, 6), (64, 5), (33, 5)])
def test_level_rule(dim, want):
    assert lc_lib.levels(dim, 300) == want and lc_lib.levels(300, dim) == want


def test_checker_statistics_handed_in_are_used():
    L = lc_lib.l_plane(128, 97, seed=5)
    curve = lc_lib.curve_lut(lc_lib.BOOST_CURVE_POINTS)
    own, info, _ = lc_lib.local_contrast_wavelets(L, 60.0, curve)
    again, info2, _ = lc_lib.local_contrast_wavelets(L, 60.0, curve, stats=info)
    assert np.array_equal(own.view(np.uint32), again.view(np.uint32)) and lc_lib.info_tuple(info2)[1:4] == lc_lib.info_tuple(info)[1:4]
    other = lc_lib.copy_info(info)
    other.mean[2] = np.float32(info.mean[2]) * np.float32(1.25)
    moved, info3, _ = lc_lib.local_contrast_wavelets(L, 60.0, curve, stats=other)
    assert info3.mean[2] == other.mean[2] and not np.array_equal(own, moved)
    assert not np.array_equal(own, lc_lib.plain_round_trip(L))


def test_flat_plane_skips_the_band_loop():
    L = lc_lib.l_plane(64, 90, flat=12000.0)
    got, info, counts = lc_lib.local_contrast_wavelets(L, 0.0, lc_lib.curve_lut(lc_lib.CUT_CURVE_POINTS))
    assert counts["levels_skipped"] == info.nlevels == 5 and counts["branch_low"] == 0
    assert np.array_equal(got.view(np.uint32), lc_lib.plain_round_trip(L).view(np.uint32))


def test_library_curve_lut_matches_oracle():
    from art_amd import capi
    for pts in (lc_lib.DEFAULT_CURVE_POINTS, lc_lib.BOOST_CURVE_POINTS, lc_lib.CUT_CURVE_POINTS,
                (1.0, 0.2, 0.3, 0.9, 0.8, 0.5, 0.6, 0.7, 0.6)):
        lut, is_set = capi.local_contrast_curve_lut(pts)
        v, ident = O.flat_curve_sample(pts, False, 500, 0.0, 501)
        assert is_set and not ident
        assert np.array_equal(lut.view(np.uint32), v.astype(np.float32).view(np.uint32))
    for pts in ((1.0, 0.1, 0.0, 0.35, 0.35, 0.6, 0.0, 0.35, 0.35),      # identity: every y is the identity value 0
                (),                                                    # empty
                (0.0,),                                                # FCT_Linear
                (0.0, 0.0, 0.5, 0.0, 0.0, 1.0, 0.9, 0.0, 0.0)):        # FCT_Linear with points behind it
        lut, is_set = capi.local_contrast_curve_lut(pts)
        assert not is_set and not lut.any()
        assert lc_lib.curve_lut(pts) is None
