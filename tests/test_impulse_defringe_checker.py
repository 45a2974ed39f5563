"""CPU: the checker of the impulse noise reduction and of defringe (tests/id_lib.py, tests/emul/impulse_defringe_ref.cc) against what it rests on.

  - impulse_nr gives the same bits whether the pixels are walked first to last or last to first: only impish pixels are written and only other
    pixels are read, which is why the device may correct them in any order, in place.
  - markImpulse at thresh 2 is the sharpening checker's map (tests/sh_lib.py), an independent restatement.
  - Defringe's three orders (0: every window reads the input, the device's definition; 1: raster order in place, the reference with one thread;
    2: 16-row chunks last to first, another schedule the reference may run) correct the same pixels and agree bit for bit wherever no other
    corrected pixel lies in a pixel's window.  How far they are apart elsewhere is printed, not bounded: it is the reference's own spread.
  - gauss3x3 and the ordered sum against float64 models.  (No compiled reference body of gaussianBlur exists after build(): oracle/Makefile.ref
    compiles the wavelet decomposition only, so the pin is a model, as in tests/test_oracle_hsl.py.)
  - Every scene of the GPU comparison flags a share of its pixels inside stated bounds: a scene that flags nothing would pass everything."""
import numpy as np
import pytest

import oracle_lib as O
import id_lib as I
import sh_lib


@pytest.mark.parametrize("w,h", [(23, 21), (67, 70)])
@pytest.mark.parametrize("thresh", [0.0, 2.5, 5.0])
def test_impulse_nr_does_not_depend_on_the_order_of_the_pixels(w, h, thresh):
    lab = O.image_rgb_to_lab(I.impulse_scene(w, h, seed=1, block=True), I.WS)
    fwd, imp_f, kept_f = I.impulse_nr(lab, thresh)
    bwd, imp_b, kept_b = I.impulse_nr(lab, thresh, backwards=True)
    assert np.array_equal(imp_f, imp_b) and kept_f == kept_b and imp_f.any()
    assert [I.nbad(a, b) for a, b in zip(fwd, bwd)] == [0, 0, 0]
    changed = (I.bits(fwd[1]) != I.bits(lab[1]))
    assert changed.any() and not (changed & (imp_f == 0)).any(), "a pixel that is not impish changed"


@pytest.mark.parametrize("w,h", [(8, 8), (11, 13), (14, 9), (67, 41)])
def test_mark_impulse_equals_the_sharpening_checker(w, h):
    Y = sh_lib.luminance(sh_lib.edge_scene(w, h, seed=5)).astype(np.float32)
    mine, n = I.mark_impulse(Y, 2.0)
    theirs, _ = sh_lib.mark_impulse(Y, 2.0)
    assert np.array_equal(mine, theirs) and n == int(np.count_nonzero(theirs)) and n > 0


def test_impulse_derived_parameters():
    for thresh, scale, want in ((50, 1.0, (2.5, 2.0, 3.0)), (0, 1.0, (0.0, 2.0, 5.5)), (100, 1.0, (5.0, 4.0, 1.0)), (50, 2.0, (1.25, 2.0, 4.25)), (100, 0.5, (10.0, 9.0, 1.0))):
        assert tuple(float(v) for v in I.impulse_derived(thresh, scale)) == want
    t = I.impulse_derived(33, 0.7)[0]           # float(thresh / scale) first, then the double quotient by 20.0, narrowed again
    assert t == np.float32(np.float64(np.float32(33 / 0.7)) / 20.0)


def test_whole_neighbourhood_impish_keeps_the_pixel():
    for w, h in I.BLOCK_SIZES:
        img, want, info, kept = I.impulse_case(w, h, 100, 1.0, block=True)
        assert kept >= 1, "no pixel with norm == 0 in the block scene"


@pytest.mark.parametrize("w,h", I.SIZES)
def test_impulse_scenes_flag_a_share_inside_the_bounds(w, h):
    for thresh, scale in I.IMPULSE_PARAMS:
        info = I.impulse_case(w, h, thresh, scale)[2]
        share = info["impulse_pixels"] / (w * h)
        print(f"impulse {w}x{h} thresh {thresh} scale {scale}: {share:.4f} of the pixels impish")
        assert I.IMPULSE_SHARE[0] <= share <= I.IMPULSE_SHARE[1]
    for bw, bh in I.BLOCK_SIZES:
        share = I.impulse_case(bw, bh, 100, 1.0, block=True)[2]["impulse_pixels"] / (bw * bh)
        assert I.IMPULSE_SHARE[0] <= share <= I.IMPULSE_SHARE[1]


@pytest.mark.parametrize("w,h", I.SIZES + (I.DEFRINGE_WIDE,))
def test_defringe_scenes_flag_a_share_inside_the_bounds(w, h):
    ran = 0
    for radius, scale in I.DEFRINGE_PARAMS:
        for threshold in I.DEFRINGE_THRESHOLDS:
            for curve in I.CURVES:
                res = I.defringe_case(w, h, radius, scale, threshold, curve)[1]
                if res is None:         # refused on the device path too: W < 2 halfwin - 2 (the GPU test asserts the refusal)
                    assert w < 2 * (int(np.ceil(2 * radius / scale)) + 1) - 2
                    continue
                share = res[1].corrected_pixels / (w * h)
                print(f"defringe {w}x{h} radius {radius} scale {scale} threshold {threshold} curve {curve}: {share:.4f} of the pixels corrected")
                assert I.DEFRINGE_SHARE[0] <= share <= I.DEFRINGE_SHARE[1]
                assert int(res[2].sum()) == res[1].corrected_pixels
                ran += 1
    assert ran >= 18


def _window_has_other(flagged, halfwin):
    """for every pixel: does its (2 halfwin - 1)^2 window hold a corrected pixel other than itself"""
    h, w = flagged.shape
    f = flagged.astype(np.int64)
    c = np.zeros((h + 1, w + 1), np.int64)
    c[1:, 1:] = f.cumsum(0).cumsum(1)
    r = halfwin - 1
    y0, y1 = np.maximum(np.arange(h) - r, 0), np.minimum(np.arange(h) + r + 1, h)
    x0, x1 = np.maximum(np.arange(w) - r, 0), np.minimum(np.arange(w) + r + 1, w)
    box = c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]
    return (box - f) > 0


@pytest.mark.parametrize("radius,threshold", [(0.5, 13), (2.0, 13), (5.0, 13), (2.0, 60), (5.0, 60)])
def test_defringe_orders_differ_only_where_corrected_pixels_see_each_other(radius, threshold):
    w, h = 131, 96
    lab = O.image_rgb_to_lab(I.fringe_scene(w, h, seed=7), I.WS)
    res = [I.pf_correct(lab, radius, threshold, I.DEFAULT_HUECURVE, order) for order in (0, 1, 2)]
    (p0, i0, f0), (p1, i1, f1), (p2, i2, f2) = res
    assert np.array_equal(f0, f1) and np.array_equal(f0, f2), "the orders correct different pixels"
    assert I.defringe_info_fields(i0) == I.defringe_info_fields(i1) == I.defringe_info_fields(i2)
    share = f0.mean()
    assert I.DEFRINGE_SHARE[0] <= share <= I.DEFRINGE_SHARE[1]
    alone = ~_window_has_other(f0, i0.halfwin)
    assert (alone & (f0 != 0)).any(), "no corrected pixel without a corrected neighbour: the scene does not test the claim"
    for k in (0, 2):
        for q in (p1, p2):
            same = I.bits(p0[k]) == I.bits(q[k])
            assert same[f0 == 0].all(), "an uncorrected pixel differs between orders"
            assert same[alone].all(), "a corrected pixel whose window holds no other corrected pixel differs between orders"
    assert I.nbad(p0[1], lab[1]) == 0, "L changed"
    d10 = max(np.abs(p1[k].astype(np.float64) - p0[k]).max() for k in (0, 2)) / 327.68
    d12 = max(np.abs(p1[k].astype(np.float64) - p2[k]).max() for k in (0, 2)) / 327.68
    m10 = np.mean([np.abs(p1[k].astype(np.float64) - p0[k])[f0 != 0].mean() for k in (0, 2)]) / 327.68
    m12 = np.mean([np.abs(p1[k].astype(np.float64) - p2[k])[f0 != 0].mean() for k in (0, 2)]) / 327.68
    # reported, not bounded: the distance between the definition and the reference's own spread
    print(f"defringe {w}x{h} radius {radius} threshold {threshold}: {share:.3f} corrected; |order 1 - order 0| max {d10:.3g} mean {m10:.3g} Lab units; "
          f"|order 1 - order 2| max {d12:.3g} mean {m12:.3g} (means over the corrected pixels)")


# ---- gauss3x3 and the ordered sum against float64 models

def _gauss3x3_model(src, sigma):
    s = src.astype(np.float64)
    c1, c2 = np.exp(-0.5 / sigma ** 2), np.exp(-1.0 / sigma ** 2)
    tot = 1.0 + 4.0 * (c1 + c2)
    c0, c1, c2 = 1.0 / tot, c1 / tot, c2 / tot
    b1 = np.exp(-1.0 / (2.0 * sigma * sigma))
    b0, b1 = 1.0 / (2.0 * b1 + 1.0), b1 / (2.0 * b1 + 1.0)
    out = s.copy()
    out[1:-1, 1:-1] = c2 * (s[:-2, :-2] + s[:-2, 2:] + s[2:, :-2] + s[2:, 2:]) + c1 * (s[:-2, 1:-1] + s[1:-1, :-2] + s[1:-1, 2:] + s[2:, 1:-1]) + c0 * s[1:-1, 1:-1]
    out[0, 1:-1] = b1 * (s[0, :-2] + s[0, 2:]) + b0 * s[0, 1:-1]
    out[-1, 1:-1] = b1 * (s[-1, :-2] + s[-1, 2:]) + b0 * s[-1, 1:-1]
    out[1:-1, 0] = b1 * (s[:-2, 0] + s[2:, 0]) + b0 * s[1:-1, 0]
    out[1:-1, -1] = b1 * (s[:-2, -1] + s[2:, -1]) + b0 * s[1:-1, -1]
    return out


@pytest.mark.parametrize("sigma", [0.25, 0.4, 0.5, 0.59])
@pytest.mark.parametrize("w,h", [(8, 8), (23, 9)])
def test_gauss3x3_against_a_float64_model(w, h, sigma):
    src = np.random.default_rng(w * h).uniform(1000.0, 60000.0, (h, w)).astype(np.float32)
    got = I.gauss3x3(src, sigma)
    assert not np.isnan(got).any(), "a pixel was not written"
    model = _gauss3x3_model(src, sigma)
    # positive terms with coefficients narrowed to float (2^-24 relative each), three float additions per group of four, one multiplication
    # per group and two additions of the groups: at most eight roundings of 2^-24 along any path, ten with slack.  Measured: 1.22e-7 (2 * 2^-24).
    # The corners are copies.
    err = np.abs(got - model) / model
    print(f"gauss3x3 {w}x{h} sigma {sigma}: max relative error against the float64 model {err.max():.3g}")
    assert err.max() <= 10 * 2.0 ** -24
    assert got[0, 0] == src[0, 0] and got[0, -1] == src[0, -1] and got[-1, 0] == src[-1, 0] and got[-1, -1] == src[-1, -1]
    k = I.gauss3x3_coef(sigma).astype(np.float64)
    assert abs(k[0] + 4 * (k[1] + k[2]) - 1.0) < 1e-6 and abs(k[3] + 2 * k[4] - 1.0) < 1e-6


@pytest.mark.parametrize("n", [1, 255, 4096, 4097, 70 * 67, 300001])
def test_ordered_sum_is_a_sum(n):
    x = np.random.default_rng(n).uniform(0.0, 1.0e9, n).astype(np.float32)
    got = I.ordered_sum(x)
    exact = float(np.sum(x.astype(np.float64)))       # (numpy's pairwise double sum: itself within n * 2^-53 relative)
    assert abs(got - exact) <= n * 2.0 ** -52 * exact
    assert I.ordered_sum(x) == got
