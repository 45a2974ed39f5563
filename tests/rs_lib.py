"""Resize: the CPU checker (tests/emul/resize_ref.cc: ImProcFunctions::Lanczos and resizeScale restated serially around the oracle's mode
switches), the scenes and the cases the tests use.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib
import value_domains as VD

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
SRC = os.path.join(HERE, "emul", "resize_ref.cc")
SO = os.path.join(HERE, "emul", "libresize_ref.so")
GOLDEN = os.path.join(HERE, "golden", "lanczos.npz")
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)
_LIB = None

PLANES, RGB = 0, 1
COUNTERS = ("clip_left", "clip_right", "clip_top", "clip_bottom", "empty_cols", "empty_rows", "lanc_one", "lanc_zero", "lanc_sinc")

# The launch geometry of art_amd/csrc/resize.h, which the GPU tests' tile-crossing sizes are chosen for: a workgroup produces ROWS destination
# rows of tile_w destination columns, tile_w being the largest count (up to MAX_TILE_W) whose horizontal taps lie within SPAN source columns
ROWS, SPAN, MAX_TILE_W = 16, 256, 1024


class Params(C.Structure):
    """rs_ref_params, the layout of artgpu_resize_params"""
    _fields_ = [("enabled", C.c_int32), ("dataspec", C.c_int32), ("scale", C.c_double), ("width", C.c_int32), ("height", C.c_int32),
                ("allow_upscaling", C.c_int32)]


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
        _LIB.rs_ref_xsinf.restype = None
        _LIB.rs_ref_xsinf.argtypes = [_fp, _fp, C.c_size_t]
        _LIB.rs_ref_support.argtypes = [C.c_float]
        _LIB.rs_ref_weights.restype = C.c_longlong
        _LIB.rs_ref_weights.argtypes = [C.c_int, C.c_int, C.c_float, _fp, _ip, _ip, _fp, C.c_longlong]
        _LIB.rs_ref_lanczos.argtypes = [_fp, _fp, _fp, C.c_int, C.c_int, _fp, _fp, _fp, C.c_int, C.c_int, C.c_float, C.c_int,
                                        C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(Counts)]
        _LIB.rs_ref_scale.restype = C.c_float
        _LIB.rs_ref_scale.argtypes = [C.POINTER(Params), C.c_int, C.c_int, _ip, _ip]
    return _LIB


def params(dataspec=0, scale=1.0, width=900, height=900, allow_upscaling=False, enabled=True):
    return Params(int(bool(enabled)), int(dataspec), float(scale), int(width), int(height), int(bool(allow_upscaling)))


def capi_params(p):
    from art_amd import capi
    return capi.ResizeParams.from_buffer_copy(bytes(p))


def xsinf(x):
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    checker().rs_ref_xsinf(x.ctypes.data_as(_fp), y.ctypes.data_as(_fp), x.size)
    return y


def support(scale):
    return int(checker().rs_ref_support(np.float32(scale)))


def weights(n, length, scale, want_args=False):
    """(w (n, support), first (n), last (n)[, xsinf's arguments in call order]) of n destination positions over `length` source positions"""
    sup = support(scale)
    w, lo, hi = np.zeros((n, sup), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    args = np.zeros(2 * n * sup, np.float32)
    cnt = checker().rs_ref_weights(n, length, np.float32(scale), w.ctypes.data_as(_fp), lo.ctypes.data_as(_ip), hi.ctypes.data_as(_ip),
                                   args.ctypes.data_as(_fp), args.size)
    assert cnt <= args.size
    return (w, lo, hi, args[:cnt]) if want_args else (w, lo, hi)


def lanczos(img, dw, dh, scale, mode=PLANES, ws=None, iws=None):
    """ImProcFunctions::Lanczos from three H x W planes (r, g, b order: a, L, b in LAB mode) into dh x dw ones.  Returns (planes, counts dict)"""
    src = [np.ascontiguousarray(a, dtype=np.float32) for a in img]
    h, w = src[0].shape
    out = [np.full((dh, dw), np.nan, np.float32) for _ in range(3)]
    cn = Counts()
    wsd = (C.c_double * 9)(*[float(v) for v in np.asarray(oracle_lib.REC2020_WS_D if ws is None else ws, np.float64).reshape(9)])
    iwsd = (C.c_double * 9)(*[float(v) for v in np.asarray(oracle_lib.REC2020_IWS_D if iws is None else iws, np.float64).reshape(9)])
    rc = checker().rs_ref_lanczos(*[a.ctypes.data_as(_fp) for a in src], w, h, *[a.ctypes.data_as(_fp) for a in out], dw, dh, np.float32(scale), int(mode),
                                  wsd, iwsd, C.byref(cn))
    assert rc == 0, rc
    return out, cn.as_dict()


def resize_scale(p, fw, fh):
    """(imw, imh, scale) of ImProcFunctions::resizeScale"""
    imw, imh = C.c_int(), C.c_int()
    sc = checker().rs_ref_scale(C.byref(p) if p is not None else None, fw, fh, C.byref(imw), C.byref(imh))
    return imw.value, imh.value, np.float32(sc)


def dst_size(w, h, scale):
    """the size resizeScale gives a w x h frame at dataspec 0"""
    return int(w * float(scale) + 0.5), int(h * float(scale) + 0.5)


def tile_width(sw, dw, scale):
    """destination columns per workgroup as the library chooses them (see ROWS / SPAN above); 0: none fits"""
    _, lo, hi = weights(dw, sw, scale)
    for tw in range(min(MAX_TILE_W, dw), 0, -1):
        if all(max(min(hi[min(c0 + tw, dw) - 1], sw), min(lo[c0], sw)) - min(lo[c0], sw) <= SPAN for c0 in range(0, dw, tw)):
            return tw
    return 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes: the value-domain families of tests/value_domains.py on three planes, and one of them with an inf in one pixel
# ---------------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("plain", "scaled_frac", "dark_offset", "tiny", "inf_pixel")
RGB_FAMILIES = ("plain", "scaled_frac")          # what an image in RGB mode holds in front of the Resize tool: super-white and a few negatives
_SCENES = {}


def scene(w, h, family="plain"):
    """three read-only h x w planes.  plain: a smooth ramp with noise in 0 .. 65535; scaled_frac: fractional, a few negatives, super-white;
    dark_offset: mostly negative; tiny: subnormal; inf_pixel: scaled_frac with +inf in one pixel of the first plane and -inf in one of the
    second (the taps spread them, and where both meet inf - inf = NaN)"""
    key = (w, h, family)
    if key not in _SCENES:
        rng = np.random.default_rng(11 + 131 * w + h)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        planes = []
        for c, f in enumerate((1.0, 0.8, 0.55)):
            base = np.clip(300.0 + 60000.0 * f * (xx / max(w - 1, 1)) * (0.3 + 0.7 * yy / max(h - 1, 1)) + rng.normal(0.0, 900.0, (h, w)), 0.0, 65535.0)
            base = np.rint(base)
            planes.append(base.astype(np.float32) if family == "plain" else VD.derive("scaled_frac" if family == "inf_pixel" else family, base))
        if family == "inf_pixel":
            planes[0][h // 2, w // 2] = np.inf
            planes[1][h // 3, min(w // 2 + 2, w - 1)] = -np.inf
        for p in planes:
            p.setflags(write=False)
        _SCENES[key] = planes
    return _SCENES[key]


_CACHE = {}


def case(w, h, dw, dh, scale, mode=PLANES, family="plain"):
    """(input planes, the checker's planes, counts), computed once and read-only"""
    key = (w, h, dw, dh, float(np.float32(scale)), mode, family)
    if key not in _CACHE:
        img = scene(w, h, family)
        want, counts = lanczos(img, dw, dh, scale, mode)
        for a in want:
            a.setflags(write=False)
        _CACHE[key] = (img, want, counts)
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
