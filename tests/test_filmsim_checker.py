"""CPU: the film simulation's checker (tests/fs_lib.py, tests/emul/filmsim_ref.cc) against the library's two host tables, against a float64 model
that shares no code with it, and the branches its scenes take."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from art_amd import capi
import fs_lib
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_host_tables_equal_the_checker():
    """artgpu_film_simulation_tables: Color::gamma2curve's values and Color::igammatab_srgb, bit for bit"""
    want_g, want_ig = fs_lib.tables()
    got_g, got_ig = capi.film_simulation_tables()
    assert np.array_equal(_bits(got_g), _bits(want_g)), int((_bits(got_g) != _bits(want_g)).sum())
    assert np.array_equal(_bits(got_ig), _bits(want_ig)), int((_bits(got_ig) != _bits(want_ig)).sum())
    assert got_g[0] == 0.0 and got_g[65535] == 65535.0 and got_ig[0] == 0.0 and got_ig[65535] == 65535.0
    assert (np.diff(got_g) > 0).all() and (np.diff(got_ig) > 0).all()
    # either pointer may be null
    assert capi.LIB.artgpu_film_simulation_tables(None, None) == 0
    # dehaze's strength table is built from the same gamma2curve: FlatCurve at gamma2curve[i] / 65535.f.  With a curve through (0, 0) and
    # (1, 1) ... it stays what it was: the existing dehaze tests pin its bits; here only that the call still works
    assert np.isfinite(capi.dehaze_strength_lut()).all()


def test_abi_declared_bound_exported(tmp_path):
    src = open(os.path.join(ROOT, "include", "artgpu.h")).read()
    for sym in ("artgpu_clut_create", "artgpu_clut_destroy", "artgpu_film_simulation", "artgpu_film_simulation_tables", "artgpu_set_pipeline_film_simulation"):
        assert re.search(r"\b(int|void)\s+%s\s*\(" % sym, src), sym
        assert sym in capi.EXPORTS and hasattr(capi.LIB, sym) and getattr(capi.LIB, sym).argtypes is not None, sym
    for m in ("clut", "film_simulation", "film_simulation_tables", "set_pipeline_film_simulation"):
        assert hasattr(capi.Context, m), m
    pf = [n for n, _ in capi.FilmSimulationParams._fields_]
    exprs = ["sizeof(artgpu_film_simulation_params)"] + [f"offsetof(artgpu_film_simulation_params, {n})" for n in pf] + ["sizeof(artgpu_pipeline_params)"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "artgpu.h"\nint main(void){' +
                     "".join(f'printf("%zu\\n", (size_t)({e}));' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(capi.FilmSimulationParams)] + [getattr(capi.FilmSimulationParams, n).offset for n in pf] + [C.sizeof(capi.PipelineParams)]
    assert got == want, list(zip(exprs, got, want))
    assert got[0] == 296 and got[1:7] == [0, 4, 8, 80, 152, 224]
    # the checker's structure is the library's
    assert C.sizeof(fs_lib.Params) == C.sizeof(capi.FilmSimulationParams) == fs_lib.checker().fs_ref_sizes(0)
    assert [(n, getattr(fs_lib.Params, n).offset) for n, _ in fs_lib.Params._fields_] == [(n, getattr(capi.FilmSimulationParams, n).offset) for n in pf]
    assert C.sizeof(fs_lib.Counts) == fs_lib.checker().fs_ref_sizes(1)


def test_levels_that_are_no_square_of_2_to_16_are_refused():
    """5, 3, 1 and 289 are ARTGPU_EINVAL; the checker refuses them too.  (Without a device there is no context to refuse them with a message:
    tests/test_gpu_filmsim.py repeats this with one.)  Nothing is read from the table and *out stays null."""
    table = np.zeros((8, 3), np.uint16)
    one = [np.zeros((1, 1), np.float32) for _ in range(3)]
    p = fs_lib.params()
    for level in (5, 3, 1, 289, 0, -4):
        h = C.c_void_p(1)
        assert capi.LIB.artgpu_clut_create(None, table.ctypes.data_as(C.POINTER(C.c_uint16)), level, 3, C.byref(h)) == -1, level
        rc = fs_lib.checker().fs_ref_tool(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in one], 1, 1, table.ctypes.data_as(C.POINTER(C.c_uint16)),
                                          level, 3, C.byref(p), None, None)
        assert rc == 2, level
    # the library without a context or a handle: an error, no crash
    cp = capi.film_simulation_params()
    assert capi.LIB.artgpu_film_simulation(None, None, None, C.byref(cp)) == -1
    assert capi.LIB.artgpu_set_pipeline_film_simulation(None, None, None, 0) == -1
    capi.LIB.artgpu_clut_destroy(None)


# -------------------------------------------------------------------------------------------------------------------------------------------
# a float64 model: matrix, analytic sRGB, trilinear on the table, blend, inverse
# -------------------------------------------------------------------------------------------------------------------------------------------
def _mat(a):
    return np.asarray(list(a), np.float64).reshape(3, 3)


def _model(img, table, level, p):
    """returns (planes, cells (H, W, 3))"""
    v = np.stack([np.asarray(a, np.float64) for a in img], -1)
    if not p.same_profile:
        v = v @ (_mat(p.xyz_to_clut) @ _mat(p.work_to_xyz)).T
    x = np.clip(v / 65535.0, 0.0, 1.0)
    enc = np.where(x <= 0.003040, x * 12.92310, 1.055 * np.power(np.maximum(x, 1e-300), 1.0 / 2.4) - 0.055) * 65535.0
    t = enc * (level - 1) / 65535.0
    cell = np.minimum(np.floor(t), level - 2).astype(np.int64)
    f = t - cell
    cube = np.asarray(table[:, :3], np.float64).reshape(level, level, level, 3)         # [blue][green][red]
    cr, cg, cb = cell[..., 0], cell[..., 1], cell[..., 2]
    fr, fg, fb = f[..., 0:1], f[..., 1:2], f[..., 2:3]
    out = 0.0
    for db in (0, 1):
        for dg in (0, 1):
            for dr in (0, 1):
                wgt = (fr if dr else 1 - fr) * (fg if dg else 1 - fg) * (fb if db else 1 - fb)
                out = out + wgt * cube[cb + db, cg + dg, cr + dr]
    out = p.strength * out + (1.0 - p.strength) * enc
    y = out / 65535.0
    lin = np.where(y <= 0.039286, y / 12.92310, np.power(np.maximum((y + 0.055) / 1.055, 1e-300), 2.4)) * 65535.0
    if not p.same_profile:
        lin = lin @ (_mat(p.xyz_to_work) @ _mat(p.clut_to_xyz)).T
    return [lin[..., c] for c in range(3)], cell


MODEL_SIZES = ((41, 67), (48, 64))
# Largest deviation |checker - model| / max(|model|, 1.0) (one unit of the 0 .. 65535 scale, so that the zeros have a denominator) over
# MODEL_SIZES x levels 4, 9, 64 x the three tables x both same_profile values x strengths 1, 0.35, 0, measured on the CPU (the test prints the
# current value).  The largest is the random table at level 64: neighbouring entries differ by up to the whole range, so the float rounding of
# the position inside a cell (2^-19 of a cell) and the gamma table's linear interpolation are multiplied by up to 63 x 65535 units per unit.
MODEL_MEASURED = 4.598e-05
MODEL_BOUND = 4 * MODEL_MEASURED
# Likewise the identity table at strength 1 with same_profile against clip(input, 0, 65535).  The two tables' round trip alone (strength 0) is
# ROUNDTRIP_MEASURED; through the identity table the uint16 rounding of its entries comes on top (up to half an encoded unit wherever
# 65535 / (level - 1) is no integer: a few hundredths of a unit in the linear toe, seen against inputs of a few hundred).
IDENTITY_MEASURED = 2.290e-04
ROUNDTRIP_MEASURED = 1.529e-06


def test_float64_model_agrees_with_the_checker():
    worst, worst_at, left_out = 0.0, None, 0.0
    for h, w in MODEL_SIZES:
        for level in fs_lib.LEVELS:
            for kind, same, strength in fs_lib.combos():
                img, table, p, want, _ = fs_lib.case(h, w, level, kind, same, strength)
                _, _, cells = fs_lib.film_simulation(img, table, level, p, want_cells=True)
                model, mcells = _model(img, table, level, p)
                keep = (cells == mcells).all(-1)             # a value on a cell face falls either way in float
                left_out = max(left_out, 1.0 - keep.mean())
                assert 1.0 - keep.mean() <= 0.001, (h, w, level, kind, same, strength, 1.0 - keep.mean())
                for gp, mp in zip(want, model):
                    dev = np.abs(np.asarray(gp, np.float64) - mp)[keep] / np.maximum(np.abs(mp[keep]), 1.0)
                    if dev.max() > worst:
                        worst, worst_at = float(dev.max()), (h, w, level, kind, same, strength)
    print("float64 model: largest relative deviation %.3e at %s (bound %.3e); at most %.4f %% of a case left out" % (worst, worst_at, MODEL_BOUND, 100 * left_out))
    assert worst <= MODEL_BOUND


def test_identity_table_returns_the_input_and_strength_zero_the_round_trip():
    """strength 1, same_profile, the identity table: the input clipped to 0 .. 65535, within IDENTITY_MEASURED x 4.  Strength 0 is NOT the input: it is
    igamma_srgb(gamma_srgbclipped(x)) exactly, whatever the table holds -- vintpf(0, out, in) is 0 * out + 1 * in -- and that is asserted bit for
    bit against the two lookups, and within ROUNDTRIP_MEASURED x 4 of the clipped input."""
    g, ig = fs_lib.tables()
    L = O.lib()
    L.oracle_lutf.restype = L.oracle_lutf_noclip.restype = C.c_float
    fp = C.POINTER(C.c_float)
    ident, trip = 0.0, 0.0
    for h, w in MODEL_SIZES:
        for level in fs_lib.LEVELS:
            img, _, _, want, _ = fs_lib.case(h, w, level, "identity", True, 1.0)
            for a, b in zip(want, img):
                clipped = np.clip(np.asarray(b, np.float64), 0.0, 65535.0)
                ident = max(ident, float((np.abs(np.asarray(a, np.float64) - clipped) / np.maximum(clipped, 1.0)).max()))
            for kind in fs_lib.KINDS:
                img, _, _, want, _ = fs_lib.case(h, w, level, kind, True, 0.0)
                for a, b in zip(want, img):
                    two = np.array([L.oracle_lutf_noclip(ig.ctypes.data_as(fp), 65536, C.c_float(L.oracle_lutf(g.ctypes.data_as(fp), 65536, C.c_float(float(v)))))
                                    for v in np.asarray(b).ravel()], np.float32).reshape(b.shape)
                    assert np.array_equal(_bits(a), _bits(two)), (h, w, level, kind)
                    clipped = np.clip(np.asarray(b, np.float64), 0.0, 65535.0)
                    trip = max(trip, float((np.abs(np.asarray(a, np.float64) - clipped) / np.maximum(clipped, 1.0)).max()))
                    assert not np.array_equal(_bits(a), _bits(b))
    print("identity table: largest relative deviation %.3e; the tables' round trip alone: %.3e" % (ident, trip))
    assert ident <= 4 * IDENTITY_MEASURED and trip <= 4 * ROUNDTRIP_MEASURED


def test_scenes_take_every_branch():
    """every counter of the checker is non-zero over the case list; the inverse table is entered outside 0 .. 65535 by the OVERDRIVE cases only
    (fs_lib says why), below zero and above 65535"""
    total = {n: 0 for n in fs_lib.COUNTERS}
    for h, w in fs_lib.SIZES:
        for level in fs_lib.LEVELS:
            per = {n: 0 for n in fs_lib.COUNTERS}
            for kind, same, strength in fs_lib.combos():
                for k, v in fs_lib.case(h, w, level, kind, same, strength)[4].items():
                    per[k] += v
            assert per["body"] == (w // 4 * 4) * h * 9 and per["tail"] == (w % 4) * h * 9, (h, w, per)     # (9 of the 18 combinations convert)
            if w * h >= 35:      # a cell 0 and a cell level - 2 pixel on each axis, at every level (the smallest planes hold too few pixels)
                assert all(per[n] > 0 for n in fs_lib.COUNTERS if n.startswith("cell_")), (h, w, level, per)
            for k, v in per.items():
                total[k] += v
    assert total["igamma_below"] == 0 and total["igamma_above"] == 0, total
    for args in fs_lib.OVERDRIVE:
        for k, v in fs_lib.case(*args)[4].items():
            total[k] += v
    h, w = fs_lib.BIG_SIZE
    big = fs_lib.case(h, w, fs_lib.BIG_LEVEL, "look", False, 0.35)[4]
    assert all(big[n] > 0 for n in fs_lib.COUNTERS if not n.startswith("igamma")), big
    print("film simulation branch counters:", total)
    for n in fs_lib.COUNTERS:
        assert total[n] > 0, n
    assert total["at_max"] == total["frac_one"]          # the position inside the last cell is exactly 1 at 65535, at every level
