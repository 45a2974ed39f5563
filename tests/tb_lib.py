"""Texture boost: the CPU checker (tests/emul/textureboost_ref.cc: texture_boost and the region loop of ImProcFunctions::textureBoost restated
serially around the oracle's guided filter, bilinear rescale, pow_F and YUV switch) and the planes the tests use.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
SRC = os.path.join(HERE, "emul", "textureboost_ref.cc")
SO = os.path.join(HERE, "emul", "libtextureboost_ref.so")
_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
_LIB = None

COUNTERS = ("rescale", "guided", "convolution", "minval_won", "clamp_low", "clamp_high", "tail_columns", "mask_partial")


class Region(C.Structure):
    _fields_ = [("strength", C.c_double), ("detail_threshold", C.c_double), ("iterations", C.c_int32), ("mask", _fp)]


class Info(C.Structure):
    """tb_ref_info, the layout of artgpu_texture_boost_info"""
    _fields_ = [("radius", C.c_int32), ("isguided", C.c_int32), ("rescaled", C.c_int32), ("work_w", C.c_int32), ("work_h", C.c_int32),
                ("kernel_size", C.c_int32), ("minval", C.c_float), ("strength", C.c_float), ("strength2", C.c_float)]


class Counts(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in COUNTERS]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def checker():
    global _LIB
    if _LIB is None:
        oracle_lib.lib()            # builds liboracle.so when needed and leaves it loaded
        if not os.path.exists(SO) or os.path.getmtime(SRC) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-msse2", "-o", SO, SRC,
                                   "-L" + ORACLE_DIR, "-loracle", "-Wl,-rpath," + ORACLE_DIR])
        _LIB = C.CDLL(SO)
    return _LIB


def info_fields(i):
    """the fields of an Info-shaped structure as a tuple of ints and float32 bit patterns"""
    f = lambda v: int(np.float32(v).view(np.uint32))
    return (int(i.radius), int(i.isguided), int(i.rescaled), int(i.work_w), int(i.work_h), int(i.kernel_size), f(i.minval), f(i.strength),
            f(i.strength2))


def gaussian_kernel(sigma):
    """build_gaussian_kernel (rt_algo.cc:902-939) -> K x K float32"""
    coef = np.zeros(81, np.float32)
    k = checker().tb_ref_gaussian_kernel(C.c_float(float(sigma)), coef.ctypes.data_as(_fp), 81)
    assert k * k <= 81, k
    return coef[:k * k].reshape(k, k).copy()


def conv(src, coef, double=False):
    """the convolution stage's definition on an H x W plane: fp32 (the checker's) or the same sum accumulated in double"""
    a = np.ascontiguousarray(src, dtype=np.float32)
    k = np.ascontiguousarray(coef, dtype=np.float32)
    h, w = a.shape
    if double:
        out = np.zeros((h, w), np.float64)
        checker().tb_ref_conv_double(a.ctypes.data_as(_fp), out.ctypes.data_as(_dp), w, h, k.shape[0], k.ctypes.data_as(_fp))
    else:
        out = np.zeros((h, w), np.float32)
        checker().tb_ref_conv(a.ctypes.data_as(_fp), out.ctypes.data_as(_fp), w, h, k.shape[0], k.ctypes.data_as(_fp))
    return out


def texture_boost_plane(Y, strength, threshold, iterations=1, scale=1.0, high_detail=True):
    """texture_boost on a copy of an H x W plane -> (plane, Info, counts dict), or None where the device path is unsupported"""
    out = np.array(Y, dtype=np.float32, order="C")
    h, w = out.shape
    reg = Region(float(strength), float(threshold), int(iterations), None)
    info, cn = Info(), Counts()
    rc = checker().tb_ref_texture_boost(out.ctypes.data_as(_fp), w, h, C.byref(reg), C.c_double(float(scale)), 1 if high_detail else 0,
                                        C.byref(info), C.byref(cn))
    if rc:
        return None
    return out, info, cn.as_dict()


def texture_boost(img, regions, ws=None, scale=1.0, high_detail=True, to_rgb=True):
    """ImProcFunctions::textureBoost on copies of three H x W planes in RGB mode.  regions: [(strength, threshold, iterations, mask array or
    None), ...].  Returns (planes, Info, counts dict), or None where a region is unsupported."""
    ws = oracle_lib.REC2020_WS_D if ws is None else ws
    out = [np.array(a, dtype=np.float32, order="C") for a in img]
    h, w = out[0].shape
    arr = (Region * max(len(regions), 1))()
    keep = []
    for k, (s, t, it, m) in enumerate(regions):
        arr[k].strength, arr[k].detail_threshold, arr[k].iterations = float(s), float(t), int(it)
        if m is not None:
            mm = np.ascontiguousarray(m, dtype=np.float32)
            assert mm.shape == (h, w)
            keep.append(mm)
            arr[k].mask = mm.ctypes.data_as(_fp)
    wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
    info, cn = Info(), Counts()
    rc = checker().tb_ref_tool(*[a.ctypes.data_as(_fp) for a in out], w, h, arr, len(regions), wsd, C.c_double(float(scale)),
                               1 if high_detail else 0, 1 if to_rgb else 0, C.byref(info), C.byref(cn))
    if rc:
        return None
    return out, info, cn.as_dict()


def textured_plane(w, h, seed=1, high=False, low=False, base=9000.0):
    """A luminance-like plane (structure at several scales, edges and noise, 300 .. 40000).  high: a block above 65535 with pixels above
    32 * 65535 (the clamp's high side).  low: a dark block with an exact zero, a negative pixel and values below 1e-5 * 65535 (the clamp's low
    side; the negative pixel is minval, which the bright-to-dark edges around the block then undershoot)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    v = base + 6000.0 * np.sin(2 * np.pi * xx / 37.0) * np.cos(2 * np.pi * yy / 29.0)
    v += 5000.0 * np.sign(np.sin(2 * np.pi * xx / 17.0) * np.sin(2 * np.pi * yy / 13.0))
    v += 2500.0 * np.sin(2 * np.pi * (xx + yy) / 5.0)
    v += rng.normal(0.0, 600.0, v.shape)
    v = np.clip(v, 300.0, 40000.0)
    if high:
        by, bx = slice(h // 8, h // 8 + max(h // 4, 6)), slice(w // 2, w // 2 + max(w // 5, 12))
        v[by, bx] = 70000.0 + rng.uniform(0.0, 50000.0, v[by, bx].shape)
        v[h // 8 + 2, w // 2 + 3] = 2.5e6
        v[h // 8 + 3, w - 1] = 3.0e6              # (in the tail columns when w % 4 != 0)
    if low:
        zy, zx = slice(h // 2, h // 2 + max(h // 5, 5)), slice(w // 10, w // 10 + max(w // 6, 10))
        v[zy, zx] = rng.uniform(0.0, 1.2, v[zy, zx].shape)
        v[h // 2 + 1, w // 10 + 2] = 0.0
        v[h // 2 + 2, w // 10 + 4] = -300.0
        v[h // 2 + 3, w - 1] = 0.25
    return v.astype(np.float32)


def nan_plane(w, h, seed=1):
    """textured_plane with one NaN in a column of the reference's 4-wide body (x = 20, first of its group of four, so that the variadic min of
    L92 still sees the other three) and one in a tail column (x = w - 1, w % 4 != 0), far from the minimum's pixel"""
    assert w % 4 != 0 and w > 40 and h > 20
    v = textured_plane(w, h, seed=seed)
    v[2, 3] = 100.0                                            # the minimum, away from both
    v[h // 2, 20] = np.nan
    v[h - 4, w - 1] = np.nan
    return v


def rgb_scene(w, h, seed=1, **kw):
    """three planes in RGB mode around textured_plane"""
    return [textured_plane(w, h, seed=seed + 10 * c, base=9000.0 + 1500.0 * c, **kw) for c in range(3)]


def smooth_mask(w, h):
    """a blend plane with exact zeros, exact ones and a smooth ramp between them"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    m = 1.5 * (0.6 * xx / max(w - 1, 1) + 0.4 * yy / max(h - 1, 1)) - 0.25
    return np.clip(m, 0.0, 1.0).astype(np.float32)


# detail thresholds and what L39-63 and build_gaussian_kernel derive from them at scale 1: (threshold, K, isguided, rescaled, radius)
THRESHOLDS = ((0.01, 3, 0, 0, 1), (0.2, 7, 0, 0, 1), (0.28, 9, 0, 0, 1), (0.3, 0, 1, 0, 1), (0.43, 0, 1, 1, 2), (1.0, 0, 1, 1, 4),
              (2.0, 0, 1, 0, 7))

# The cases of the GPU comparison of artgpu_texture_boost_plane (tests/test_gpu_textureboost.py); tests/test_textureboost_checker.py shows from
# the checker's counters that they take every branch.  name: (w, h, seed, strength, threshold, iterations, scale, high, low)
PLANE_CASES = {}
for _t, *_ in THRESHOLDS:                                                   # 67 x 41: w % 4 == 3, partial convolution tiles (64 x 16) on both edges
    PLANE_CASES["67x41-t%g" % _t] = (67, 41, 1, 1.0, _t, 1, 1.0, False, False)
PLANE_CASES.update({
    "130x97-t0.2-neg-it3": (130, 97, 2, -0.8, 0.2, 3, 1.0, False, False),   # several tiles
    "130x97-t0.43-neg-it3": (130, 97, 3, -0.8, 0.43, 3, 1.0, False, False), # upscaled to 173 x 129
    "130x97-t1-it3": (130, 97, 4, 1.0, 1.0, 3, 1.0, False, False),
    "130x97-t2-scale2": (130, 97, 5, 1.0, 2.0, 1, 2.0, False, False),       # fradius 3.5: radius 4, rescaled
    "130x97-t0.2-high": (130, 97, 6, 1.0, 0.2, 1, 1.0, True, False),
    "130x97-t1-high": (130, 97, 7, -0.8, 1.0, 1, 1.0, True, False),
    "67x41-t0.3-low": (67, 41, 8, 1.0, 0.3, 1, 1.0, False, True),
    "130x97-t0.2-low-it3": (130, 97, 9, 1.0, 0.2, 3, 1.0, False, True),
    "701x33-t1": (701, 33, 10, 1.0, 1.0, 1, 1.0, False, False),             # above 600: both guided filters subsample by 4
    "701x33-t2": (701, 33, 11, 1.0, 2.0, 1, 1.0, False, True),              # radius 7 (subsampling 1) and 28 (subsampling 4)
    "300x200-t0.43": (300, 200, 12, 1.0, 0.43, 1, 1.0, False, False),       # (also run device-resident with a padded row stride)
    "300x200-t0.2": (300, 200, 13, 1.0, 0.2, 1, 1.0, False, False),
    "67x11-t0.2": (67, 11, 14, 1.0, 0.2, 2, 1.0, False, True),              # lower than one convolution tile (64 x 16)
    "40x41-t0.28": (40, 41, 15, -0.8, 0.28, 1, 1.0, True, False),           # narrower than one tile, 9 x 9 kernel
    # the smallest planes the header promises (ARTGPU_TEXTURE_BOOST_MIN_SIZE = 5): box radii clamped by f_mean, and above 600 a one-row grid
    "5x5-t0.2": (5, 5, 16, 1.0, 0.2, 1, 1.0, False, False),
    "5x5-t2": (5, 5, 17, 1.0, 2.0, 2, 1.0, False, False),
    "605x5-t1.43": (605, 5, 18, 1.0, 1.43, 1, 1.0, False, False),           # radius 5 and 20: both filters subsample by 5, grids of 121 x 1
})
MIN_SIZE = 5
STRIDED_CASES = ("300x200-t0.43", "300x200-t0.2")

# the whole tool: name: (w, h, seed, [(strength, threshold, iterations, masked), ...], to_rgb, low)
TOOL_CASES = {
    "130x97-two-regions-rgb": (130, 97, 21, [(1.0, 0.2, 1, False), (-0.8, 1.0, 2, True)], True, False),
    "130x97-two-regions-yuv": (130, 97, 21, [(1.0, 0.2, 1, False), (-0.8, 1.0, 2, True)], False, False),
    "67x41-skip-zero-strength": (67, 41, 22, [(0.0, 0.2, 1, False), (1.5, 0.3, 1, True), (0.0, 1.0, 1, True)], True, True),
    "67x41-all-zero": (67, 41, 23, [(0.0, 0.2, 1, False), (0.0, 1.0, 3, True)], True, False),
}
_CACHE = {}


def plane_case(name):
    """(input plane, keyword arguments of texture_boost_plane(), the checker's plane, Info and counts), computed once and read-only"""
    if name not in _CACHE:
        w, h, seed, strength, threshold, iterations, scale, high, low = PLANE_CASES[name]
        Y = textured_plane(w, h, seed=seed, high=high, low=low)
        kw = dict(strength=strength, threshold=threshold, iterations=iterations, scale=scale)
        want, info, counts = texture_boost_plane(Y, **kw)
        Y.setflags(write=False)
        want.setflags(write=False)
        _CACHE[name] = (Y, kw, want, info, counts)
    return _CACHE[name]


def tool_case(name):
    """(input planes, region list with mask arrays, to_rgb, the checker's planes, Info and counts), computed once and read-only"""
    if name not in _CACHE:
        w, h, seed, regs, to_rgb, low = TOOL_CASES[name]
        img = rgb_scene(w, h, seed=seed, low=low)
        mask = smooth_mask(w, h)
        regions = [(s, t, it, mask if masked else None) for s, t, it, masked in regs]
        want, info, counts = texture_boost(img, regions, to_rgb=to_rgb)
        for a in img + want + [mask]:
            a.setflags(write=False)
        _CACHE[name] = (img, regions, to_rgb, want, info, counts)
    return _CACHE[name]
