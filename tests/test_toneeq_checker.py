"""CPU: the tone equalizer's checker (tests/te_lib.py, tests/emul/toneeq_ref.cc) against the library's host table, against a float64 model that
shares no code with it, and the branches its scenes take."""
import ctypes as C

import numpy as np
import pytest

from art_amd import capi
import oracle_lib as O
import te_lib


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("bands", list(te_lib.BANDS))
@pytest.mark.parametrize("pivot", [-4.0, 0.0, 2.55])
def test_host_table_equals_the_checker(bands, pivot):
    """artgpu_tone_equalizer_lut's table, gain, w_sum and factors equal tone_eq's restatement bit for bit, at every regularization level"""
    for reg in range(5):
        p = te_lib.params(te_lib.BANDS[bands], reg, pivot)
        want, wi = te_lib.lut(p)
        got, gi = capi.tone_equalizer_lut(te_lib.capi_params(p))
        assert np.array_equal(_bits(got), _bits(want)), (bands, pivot, reg, int((_bits(got) != _bits(want)).sum()))
        assert te_lib.info_fields(gi)[:14] == te_lib.info_fields(wi)[:14]
        if reg:
            continue                 # (the table does not depend on the level: once is enough for the values below)
        assert np.isfinite(got).all() and (got > 0).all()
        if bands == "zero":         # every factor 1: the sum of the windows over its value at 0 EV, which is the table's last entry
            assert got[65535] == 1.0 and abs(got[0] - 0.9896) < 1e-4


# -------------------------------------------------------------------------------------------------------------------------------------------
# a float64 model of steps 1, 4 and 5 (regularization 0): luminance, the table, the group-of-four rule
# -------------------------------------------------------------------------------------------------------------------------------------------
CENTERS = np.arange(-16.0, 7.0, 2.0)


def _model_factors(bands):
    b = np.asarray(bands, np.float64)
    idx = [0, 0, 0, 0, 0, 1, 2, 3, 4, 4, 4, 4]
    lo = np.array([2, 2, 2, 2, 2, 2, 2.5, 3, 3, 3, 3, 3.0])
    hi = np.array([3, 3, 3, 3, 3, 3, 2.5, 2, 2, 2, 2, 2.0])
    v = b[idx]
    return 2.0 ** (v / 100.0 * np.where(v < 0, lo, hi))


def _model_corr(y, factors):
    with np.errstate(divide="ignore"):
        luma = np.clip(np.log2(np.maximum(y, 0.0)), -14.0, 4.0)
    g = np.exp(-(luma[..., None] - CENTERS) ** 2 / 4.0)
    return (g * factors).sum(-1) / np.exp(-CENTERS ** 2 / 4.0).sum()


def _model(img, bands, pivot, ws):
    gain = 2.0 ** -pivot / 65535.0
    r, g, b = (np.asarray(a, np.float64) * gain for a in img)
    Y = np.clip(r * ws[1][0] + g * ws[1][1] + b * ws[1][2], 1e-5, 32.0)
    h, w = Y.shape
    f = _model_factors(bands)
    table = _model_corr(np.arange(65536) / 65535.0, f)
    idx = Y * 65535.0
    i0 = np.clip(np.floor(idx).astype(np.int64), 0, 65534)
    from_table = table[i0] + (table[i0 + 1] - table[i0]) * (np.minimum(idx, 65535.0) - i0)
    analytic = _model_corr(Y, f)
    above = Y > 1.0
    wb = w // 4 * 4
    group_any = np.zeros_like(above)
    if wb:
        group_any[:, :wb] = np.repeat(above[:, :wb].reshape(h, wb // 4, 4).any(-1), 4, axis=1)
    group_any[:, wb:] = above[:, wb:]
    corr = np.where(group_any, analytic, from_table)
    return [c * corr / gain for c in (r, g, b)]


MODEL_CASES = [n for n in te_lib.CASES if te_lib.CASES[n][5] == 0]
MODEL_MEASURED = 4.25e-7  # measured on the CPU with the scenes of MODEL_CASES (the test prints the current value)
MODEL_BOUND = 4 * MODEL_MEASURED


def test_float64_model_agrees_with_the_checker():
    """Largest relative deviation |checker - model| / |model| over every pixel of every regularization-0 scene of te_lib.CASES, pixels whose
    model value is below 1e-30 in magnitude excepted (exact zeros stay exact zeros: asserted).  Measured on the CPU: 4.25e-07 (MODEL_MEASURED), about
    seven float32 ulps: the chain of roundings through xlogf, twelve xexpf, their sum and the three multiplications.  The bound is four times
    that, 1.7e-06: it only has to absorb float rounding -- the model shares no code with the checker."""
    ws = np.asarray(O.REC2020_WS_D, np.float64).reshape(3, 3)
    worst = 0.0
    for name in MODEL_CASES:
        img, p, scale, want, _, _ = te_lib.case(name)
        _, _, _, _, bands, _, pivot = te_lib.CASES[name]
        model = _model(img, bands, pivot, ws)
        for gp, mp in zip(want, model):
            small = np.abs(mp) < 1e-30
            assert (np.asarray(gp)[small] == 0).all()
            dev = np.abs(np.asarray(gp, np.float64)[~small] - mp[~small]) / np.abs(mp[~small])
            worst = max(worst, float(dev.max()))
    print("float64 model: largest relative deviation %.3e (bound %.3e)" % (worst, MODEL_BOUND))
    assert worst <= MODEL_BOUND


def test_scenes_take_every_branch():
    """every counter of the checker is non-zero over the test scenes (te_lib.NEVER: provably zero, asserted as such)"""
    total = {n: 0 for n in te_lib.COUNTERS}
    for name in te_lib.SMALL_CASES:
        for k, v in te_lib.case(name)[5].items():
            total[k] += v
    print("tone equalizer branch counters:", total)
    for n in te_lib.COUNTERS:
        if n in te_lib.NEVER:
            assert total[n] == 0, n
        else:
            assert total[n] > 0, n
    # tail only / body + tail
    c = te_lib.case("3x9-reg0")[5]
    assert c["groups_analytic"] + c["groups_table"] == 0 and c["tail_above"] + c["tail_table"] == 27
    c = te_lib.case("37x29-reg0")[5]
    assert c["groups_analytic"] + c["groups_table"] == 9 * 29 and c["tail_above"] + c["tail_table"] == 29 and c["groups_one_lane"] > 0


def test_plans_of_the_cases():
    """the filters each case runs: radii, subsampling and box radii as the issue's case list names them"""
    def plan(name):
        i = te_lib.case(name)[4]
        return int(i.filters), list(i.radius), list(i.subsampling), list(i.box_radius)
    assert plan("37x29-reg0") == (0, [0, 0, 0], [0, 0, 0], [0, 0, 0])
    assert plan("64x48-reg1") == (1, [5, 0, 0], [1, 0, 0], [5, 0, 0])
    assert plan("64x48-reg4") == (2, [5, 350, 0], [1, 1, 0], [5, 22, 0])
    assert plan("64x48-reg2") == (3, [5, 350, 700], [1, 1, 1], [5, 22, 22])
    assert plan("640x45-reg4") == (2, [5, 350, 0], [5, 5, 0], [1, 3, 0])
    assert plan("724x720-reg4") == (2, [5, 350, 0], [5, 5, 0], [1, 70, 0])
    assert plan("1420x1416-reg2") == (3, [5, 350, 700], [5, 5, 5], [1, 70, 140])
    assert plan("130x97-scale2-reg3") == (3, [3, 175, 175], [1, 1, 1], [3, 47, 47])
    assert plan("701x33-scale2-reg4") == (2, [3, 175, 0], [3, 5, 0], [1, 1, 0])
    e = te_lib.case("64x48-reg2")[4].epsilon
    assert [np.float32(v) for v in e] == [np.float32(0.01) + np.float32(0.002) * np.float32(2), np.float32(0.004), np.float32(0.004) / np.float32(100)]


def test_abi_and_unsupported_cases():
    lib = te_lib.checker()
    assert C.sizeof(capi.ToneEqualizerParams) == C.sizeof(te_lib.Params) == lib.te_ref_sizes(0) == 40
    assert C.sizeof(capi.ToneEqualizerInfo) == C.sizeof(te_lib.Info) == lib.te_ref_sizes(1) == 108
    for name, (w, h, scale, kw) in te_lib.UNSUPPORTED.items():
        assert te_lib.tone_equalizer(te_lib.scene(w, h, seed=13), te_lib.params(**kw), scale=scale) is None, name
    # enabled == 0 leaves the planes alone; regularization 0 accepts 1 x 1
    img = te_lib.scene(67, 41, seed=13)
    out, _, _ = te_lib.tone_equalizer(img, te_lib.params(te_lib.MIXED, 4, -4.0, enabled=False))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(out, img))
    one = [np.full((1, 1), v, np.float32) for v in (30000.0, 20000.0, 10000.0)]
    assert te_lib.tone_equalizer(one, te_lib.params(te_lib.MIXED, 0, -4.0)) is not None
    # the library without a context: no crash, an error; the table call checks its pointers
    p = capi.tone_equalizer_params(te_lib.MIXED, 0, -4.0)
    assert capi.LIB.artgpu_tone_equalizer(None, None, C.byref(p), None, 1.0, None) == -1
    assert capi.LIB.artgpu_set_pipeline_tone_equalizer(None, C.byref(p)) == -1
    assert capi.LIB.artgpu_tone_equalizer_lut(None, None, None) == -1
    assert capi.LIB.artgpu_tone_equalizer_lut(C.byref(p), None, None) == -1
