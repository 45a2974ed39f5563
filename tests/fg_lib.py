"""Film grain: the CPU checker (tests/emul/filmgrain_ref.cc: filmGrain's region derivation, add_noise and guidedSmoothing's frame around a
NOISE region restated serially, with rng.h's 64-bit generator stepping only), the scenes and the cases the tests use.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
SRC = os.path.join(HERE, "emul", "filmgrain_ref.cc")
SO = os.path.join(HERE, "emul", "libfilmgrain_ref.so")
GOLDEN = os.path.join(HERE, "golden", "filmgrain_rng.npz")
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)
_dp = C.POINTER(C.c_double)
_LIB = None

L, C_, LC = 0, 1, 2                     # SmoothingParams::Region::Channel: LUMINANCE, CHROMINANCE, RGB
NORMD = 5233
MASK48 = (1 << 48) - 1
# The launch geometry of art_amd/csrc/filmgrain.h, which the GPU tests' tile-crossing sizes are chosen for: a workgroup owns TILE_W x TILE_H
# pixels, a lane updates PX of them and fills runs of RUN noise values of the tile's neighbourhood
TILE_W, TILE_H, PX, RUN = 64, 16, 4, 7
LDS_BYTES_MAX = 28 * 1024               # table 20932 + taps 196 + noise tile 6248 + jump maps 528, with alignment, within 28 KiB

WS = oracle_lib.REC2020_WS_D


def checker():
    global _LIB
    if _LIB is None:
        oracle_lib.lib()            # builds liboracle.so when needed and leaves it loaded
        if not os.path.exists(SO) or os.path.getmtime(SRC) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-msse2", "-o", SO, SRC,
                                   "-L" + ORACLE_DIR, "-loracle", "-Wl,-rpath," + ORACLE_DIR])
        _LIB = C.CDLL(SO)
        _LIB.fg_ref_table.restype = None
        _LIB.fg_ref_table.argtypes = [C.c_int, _fp, C.POINTER(C.c_uint64)]
        _LIB.fg_ref_draws.restype = None
        _LIB.fg_ref_draws.argtypes = [C.c_uint64, C.c_longlong, C.c_longlong, C.POINTER(C.c_uint32)]
        _LIB.fg_ref_stream48_mismatches.restype = C.c_longlong
        _LIB.fg_ref_stream48_mismatches.argtypes = [C.c_uint64, C.c_longlong]
        _LIB.fg_ref_kernel.argtypes = [C.c_float, _fp]
        _LIB.fg_ref_conv.restype = None
        _LIB.fg_ref_conv.argtypes = [_fp, C.c_int, C.c_int, _fp, C.c_int, _fp, _dp, _dp]
        _LIB.fg_ref_regions.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _ip, _fp]
        _LIB.fg_ref_smoothing_noise.restype = None
        _LIB.fg_ref_smoothing_noise.argtypes = [_fp, _fp, _fp, C.c_int, C.c_int, _dp, C.c_double, C.c_int, _ip, C.POINTER(_fp), C.c_int, C.c_int, _ip]
    return _LIB


def fnv1a64(data: bytes) -> int:
    """the hash tests/golden/filmgrain_rng.npz holds of every table's bytes"""
    h = 0xcbf29ce484222325
    for x in data:
        h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def table(seed):
    """(normd[5233], the generator's full 64-bit state behind it)"""
    normd = np.empty(NORMD, np.float32)
    st = C.c_uint64(0)
    checker().fg_ref_table(int(seed), normd.ctypes.data_as(_fp), C.byref(st))
    return normd, int(st.value)


def draws(state, skip, n):
    """randint(5233) of draws skip .. skip + n - 1 counted from `state`, stepping serially"""
    out = np.zeros(n, np.uint32)
    checker().fg_ref_draws(int(state), int(skip), int(n), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out


def stream48_mismatches(state, n):
    return int(checker().fg_ref_stream48_mismatches(int(state), int(n)))


def radius_of(coarseness, scale=1.0):
    return np.float32(np.float64(np.float32(0.5) + np.float32(1.75) * np.float32(coarseness) / np.float32(100.0)) / np.float64(scale))


def kernel(radius):
    taps = np.zeros(49 * 4, np.float32)         # room for a kernel the library would refuse
    sz = checker().fg_ref_kernel(np.float32(radius), taps.ctypes.data_as(_fp))
    assert sz * sz <= taps.size, sz
    return taps[:sz * sz].reshape(sz, sz).copy(), sz


def conv(nb, k):
    """(the fp32 direct sum, the float64 one, sum |k * x| per pixel)"""
    nb = np.ascontiguousarray(nb, np.float32)
    k = np.ascontiguousarray(k, np.float32)
    h, w = nb.shape
    out, out64, ab = np.empty_like(nb), np.empty((h, w), np.float64), np.empty((h, w), np.float64)
    checker().fg_ref_conv(nb.ctypes.data_as(_fp), w, h, k.ctypes.data_as(_fp), k.shape[0], out.ctypes.data_as(_fp), out64.ctypes.data_as(_dp), ab.ctypes.data_as(_dp))
    return out, out64, ab


def regions(iso, strength, color, output_pipeline=True, scale=1.0):
    """filmGrain's regions as (channel, strength, coarseness, seed, sz, sf) tuples"""
    out = np.zeros(5 * 8, np.int32)
    sf = np.zeros(8, np.float32)
    n = checker().fg_ref_regions(int(iso), int(strength), int(bool(color)), int(bool(output_pipeline)), float(scale), out.ctypes.data_as(_ip), sf.ctypes.data_as(_fp))
    return [tuple(int(v) for v in out[5 * i:5 * i + 5]) + (np.float32(sf[i]),) for i in range(n)]


def smoothing_noise(img, regs, scale=1.0, masks=None, first=True, last=True, ws=None):
    """guidedSmoothing over NOISE regions [(strength, coarseness, channel)] on three H x W planes.  Returns (planes, boxes (n, 5))"""
    pl = [np.array(a, dtype=np.float32, order="C", copy=True) for a in img]
    h, w = pl[0].shape
    n = len(regs)
    flat = np.ascontiguousarray(np.asarray(regs, np.int32).reshape(-1))
    wsd = (C.c_double * 9)(*[float(v) for v in np.asarray(WS if ws is None else ws, np.float64).reshape(9)])
    keep = [None if m is None else np.ascontiguousarray(m, np.float32) for m in (masks or [None] * n)]
    mp = (_fp * max(n, 1))(*[None if m is None else m.ctypes.data_as(_fp) for m in keep])
    boxes = np.zeros((max(n, 1), 5), np.int32)
    checker().fg_ref_smoothing_noise(*[a.ctypes.data_as(_fp) for a in pl], w, h, wsd, float(scale), n, flat.ctypes.data_as(_ip), mp, int(bool(first)), int(bool(last)),
                                     boxes.ctypes.data_as(_ip))
    return pl, boxes[:n]


def film_grain(img, iso=400, strength=50, color=False, output_pipeline=True, scale=1.0):
    regs = regions(iso, strength, color, output_pipeline, scale)
    return smoothing_noise(img, [(r[1], r[2], r[0]) for r in regs], scale)[0], regs


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------
_SCENES = {}


def scene(w, h, family="plain"):
    """three read-only h x w planes of an image in RGB mode, 0 .. 65535.  plain: a ramp with texture; wild: the same with negatives, exact zeros
    and super-white values sprinkled over a fifth of the pixels (what an image holds behind the exposure and texture boost)"""
    key = (w, h, family)
    if key not in _SCENES:
        rng = np.random.default_rng(7 + 977 * w + h)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        planes = []
        for f in (1.0, 0.8, 0.55):
            base = 300.0 + 60000.0 * f * (xx / max(w - 1, 1)) * (0.3 + 0.7 * yy / max(h - 1, 1)) + rng.normal(0.0, 900.0, (h, w))
            base = np.clip(base, 0.0, 65535.0)
            if family == "wild":
                pick = rng.random((h, w))
                base = np.where(pick < 0.07, -rng.random((h, w)) * 800.0, base)
                base = np.where((pick >= 0.07) & (pick < 0.13), 0.0, base)
                base = np.where((pick >= 0.13) & (pick < 0.20), 65535.0 * (1.0 + rng.random((h, w)) * 3.0), base)
            p = base.astype(np.float32)
            p.setflags(write=False)
            planes.append(p)
        _SCENES[key] = planes
    return _SCENES[key]


def box_mask(w, h, x0, y0, x1, y1, seed=5):
    """a blend plane that is zero outside [x0, x1) x [y0, y1) and in (0, 1] inside, with both corners of the box above zero"""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.float32)
    m[y0:y1, x0:x1] = (0.05 + 0.95 * rng.random((y1 - y0, x1 - x0))).astype(np.float32)
    return m


_CACHE = {}


def case(w, h, strength, coarseness, channel, scale=1.0, family="plain"):
    """(input planes, the checker's planes) of one mask-less NOISE region with both normalise passes, computed once and read-only"""
    key = (w, h, strength, coarseness, channel, float(scale), family)
    if key not in _CACHE:
        img = scene(w, h, family)
        want, _ = smoothing_noise(img, [(strength, coarseness, channel)], scale)
        for a in want:
            a.setflags(write=False)
        _CACHE[key] = (img, want)
    return _CACHE[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what=""):
    """equality of float32 bit patterns; NaNs compare equal to NaNs whatever their payload"""
    for name, gp, wp in zip("rgb", got, want):
        gp, wp = np.asarray(gp, np.float32), np.asarray(wp, np.float32)
        assert gp.shape == wp.shape, (what, name, gp.shape, wp.shape)
        bad = (bits(gp) != bits(wp)) & ~(np.isnan(gp) & np.isnan(wp))
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            raise AssertionError("%s plane %s: %d of %d values differ, first at %s: %r (%#010x) != %r (%#010x)" % (
                what, name, int(bad.sum()), bad.size, i, gp[i], int(bits(gp)[i]), wp[i], int(bits(wp)[i])))
