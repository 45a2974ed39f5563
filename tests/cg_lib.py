"""Creative gradients, soft light and black-and-white: the CPU checker (tests/emul/creative_ref.cc: ImProcFunctions::creativeGradients,
ImProcFunctions::softLight, ImProcFunctions::blackAndWhite and computeBWMixerConstants restated serially around the oracle's LUTf lookups, xcbrtf,
pow_F and YUV mode switches), the scenes and the cases the tests use.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib
import value_domains as VD

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
SRC = os.path.join(HERE, "emul", "creative_ref.cc")
SO = os.path.join(HERE, "emul", "libcreative_ref.so")
_fp = C.POINTER(C.c_float)
_LIB = None

SETTINGS = ("NormalContrast", "Panchromatic", "HyperPanchromatic", "LowSensitivity", "HighSensitivity", "Orthochromatic", "HighContrast", "Luminance",
            "Landscape", "Portrait", "InfraRed", "RGB-Rel", "RGB-Abs", "ROYGCBPM-Rel", "ROYGCBPM-Abs")
FILTERS = ("None", "Red", "Orange", "Yellow", "YellowGreen", "Green", "Cyan", "Blue", "Purple")
STRENGTHS = (1, 50, 100)
LDS_BYTES_MAX = 0            # art_amd/csrc/blackwhite.h: BW_LDS_BYTES

# (h, w).  1x1 .. 8x8 move black-and-white's body / tail boundary through every residue of W mod 4 (and W < 4, where there is no body); 67x45 and 259x3
# cross a 256-lane workgroup in x and are narrower than one in y
SHAPES = ((1, 1), (1, 2), (5, 3), (4, 4), (3, 5), (9, 7), (8, 8), (45, 67), (3, 259))
STRIDED = (70, 131)          # one plane with a row stride larger than its width and a non-zero offset (layout_lib)


class SlCounts(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in ("below_zero", "in_table", "above_max", "nan")]


class BwCounts(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in ("body", "tail")]


CG_COUNTERS = ("g_top", "g_bottom", "g_ramp_sin", "g_ramp_cos", "g_angle_zero", "g_angled", "g_transposed",
               "v_faded", "v_fade_out", "v_inside", "v_outside", "v_ramp_cos", "v_ramp_sin", "v_normn2", "v_normn4", "v_normn6", "v_normn8", "v_portrait", "v_dist_zero")


class CgCounts(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in CG_COUNTERS]


class CgParams(C.Structure):
    """cr_cg_params, the layout of artgpu_creative_gradients_params"""
    _fields_ = [("gradient_enabled", C.c_int32), ("gradient_degree", C.c_double), ("gradient_feather", C.c_int32), ("gradient_strength", C.c_double),
                ("gradient_center_x", C.c_int32), ("gradient_center_y", C.c_int32),
                ("pcvignette_enabled", C.c_int32), ("pcvignette_strength", C.c_double), ("pcvignette_feather", C.c_int32), ("pcvignette_roundness", C.c_int32),
                ("pcvignette_center_x", C.c_int32), ("pcvignette_center_y", C.c_int32),
                ("crop_enabled", C.c_int32), ("crop_x", C.c_int32), ("crop_y", C.c_int32), ("crop_w", C.c_int32), ("crop_h", C.c_int32),
                ("offset_x", C.c_int32), ("offset_y", C.c_int32), ("full_width", C.c_int32), ("full_height", C.c_int32), ("scale", C.c_double)]


DERIVED_INT_A = ("apply_gradient", "apply_pcvignette", "cx", "cy", "angle_is_zero", "transpose", "bright_top", "h")
DERIVED_FLOAT = ("ta", "yc", "xc", "ys", "ys_inv", "scale", "botmul", "topmul", "top_edge_0",
                 "oe_a", "oe_b", "oe1_a", "oe1_b", "oe2_a", "oe2_b", "ie_mul", "ie1_mul", "ie2_mul", "sepmix", "feather")
DERIVED_INT_B = ("x1", "x2", "y1", "y2", "ex", "ey", "ew", "eh", "sep", "is_super_ellipse_mode", "is_portrait")


class CgDerived(C.Structure):
    """cr_cg_derived, the layout of artgpu_creative_gradient_derived"""
    _fields_ = ([(n, C.c_int32) for n in DERIVED_INT_A] + [(n, C.c_float) for n in DERIVED_FLOAT] + [(n, C.c_int32) for n in DERIVED_INT_B] +
                [("pcv_scale", C.c_float), ("fadeout_mul", C.c_float)])


class Mixer(C.Structure):
    _fields_ = [("bwr", C.c_float), ("bwg", C.c_float), ("bwb", C.c_float), ("kcorec", C.c_float), ("filcor", C.c_float),
                ("rrm", C.c_double), ("ggm", C.c_double), ("bbm", C.c_double)]

    def as_tuple(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


def _dict(c):
    return {n: int(getattr(c, n)) for n, _ in c._fields_}


def checker():
    global _LIB
    if _LIB is None:
        oracle_lib.lib()            # builds liboracle.so when needed and leaves it loaded
        if not os.path.exists(SO) or os.path.getmtime(SRC) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-msse2", "-o", SO, SRC,
                                   "-L" + ORACLE_DIR, "-loracle", "-Wl,-rpath," + ORACLE_DIR])
        _LIB = C.CDLL(SO)
        _LIB.cr_soft_light_lut.restype = None
        _LIB.cr_soft_light_lut.argtypes = [C.c_int, _fp]
        _LIB.cr_soft_light.argtypes = [_fp, _fp, _fp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SlCounts)]
        _LIB.cr_bw_mixer_constants.restype = None
        _LIB.cr_bw_mixer_constants.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(Mixer)]
        _LIB.cr_black_and_white.restype = None
        _LIB.cr_black_and_white.argtypes = [_fp, _fp, _fp, C.c_size_t, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.c_int, _fp, _fp, _fp, C.POINTER(BwCounts)]
        _LIB.cr_yuv_to_rgb.restype = None
        _LIB.cr_yuv_to_rgb.argtypes = [_fp, _fp, _fp, C.c_size_t, C.c_int, C.c_int, _fp]
        for name in ("cr_xsinf", "cr_xcosf", "cr_xcbrtf"):
            getattr(_LIB, name).restype = None
            getattr(_LIB, name).argtypes = [_fp, _fp, C.c_size_t]
        _LIB.cr_pow_F.restype = None
        _LIB.cr_pow_F.argtypes = [_fp, _fp, _fp, C.c_size_t]
        _LIB.cr_cg_derive.restype = None
        _LIB.cr_cg_derive.argtypes = [C.POINTER(CgParams), C.c_int, C.c_int, C.POINTER(CgDerived)]
        _LIB.cr_creative_gradients.argtypes = [_fp, _fp, _fp, C.c_size_t, C.c_int, C.c_int, C.POINTER(CgParams), _fp, _fp, _fp, _fp, C.c_longlong,
                                               C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(CgCounts)]
    return _LIB


WS_F = np.asarray(oracle_lib.REC2020_WS_D, np.float64).reshape(9).astype(np.float32)      # Imagefloat::ws_: the working-space matrix as floats


def _copies(img):
    out = [np.array(a, dtype=np.float32, order="C") for a in img]
    h, w = out[0].shape
    return out, w, h


def soft_light_lut(strength):
    f = np.empty(65536, np.float32)
    checker().cr_soft_light_lut(int(strength), f.ctypes.data_as(_fp))
    return f


def soft_light(img, strength, enabled=True):
    """ImProcFunctions::softLight on three H x W planes -> (planes, counts, ran)"""
    out, w, h = _copies(img)
    cn = SlCounts()
    ran = checker().cr_soft_light(*[a.ctypes.data_as(_fp) for a in out], w, w, h, int(bool(enabled)), int(strength), C.byref(cn))
    return out, _dict(cn), bool(ran)


def bw_mixer(setting, filt, mixer=(33, 33, 33)):
    m = Mixer()
    checker().cr_bw_mixer_constants(setting.encode(), filt.encode(), int(mixer[0]), int(mixer[1]), int(mixer[2]), C.byref(m))
    return m


def black_and_white(img, setting="RGB-Rel", filt="None", mixer=(33, 33, 33), gamma=(0, 0, 0), cast_bottom=0, ulut=None, vlut=None, to_rgb=True):
    """ImProcFunctions::blackAndWhite on three H x W planes -> (planes, counts).  With a cast the reference leaves YUV; to_rgb takes that result
    through the oracle's setMode(RGB), which is what the stand-alone entry point hands back"""
    out, w, h = _copies(img)
    cn = BwCounts()
    mix, gam = (C.c_int * 3)(*[int(v) for v in mixer]), (C.c_int * 3)(*[int(v) for v in gamma])
    up = None if ulut is None else np.ascontiguousarray(ulut, np.float32).ctypes.data_as(_fp)
    vp = None if vlut is None else np.ascontiguousarray(vlut, np.float32).ctypes.data_as(_fp)
    ptrs = [a.ctypes.data_as(_fp) for a in out]
    checker().cr_black_and_white(*ptrs, w, w, h, setting.encode(), filt.encode(), mix, gam, int(cast_bottom), up, vp, WS_F.ctypes.data_as(_fp), C.byref(cn))
    if cast_bottom > 0 and to_rgb:
        checker().cr_yuv_to_rgb(*ptrs, w, w, h, WS_F.ctypes.data_as(_fp))
    return out, _dict(cn)


def leaf(name, *args):
    """the checker's own xsinf / xcosf / xcbrtf (one array) or pow_F (two)"""
    arrs = [np.ascontiguousarray(a, np.float32) for a in args]
    out = np.empty_like(arrs[0])
    getattr(checker(), "cr_" + name)(*[a.ctypes.data_as(_fp) for a in arrs], out.ctypes.data_as(_fp), out.size)
    return out


def cg_params(gradient=None, pcvignette=None, crop=None, offset=(0, 0), full=(-1, -1), scale=1.0):
    """gradient: (degree, feather, strength, center_x, center_y) or None; pcvignette: (strength, feather, roundness, center_x, center_y) or None;
    crop: (x, y, w, h) or None"""
    g = gradient if gradient is not None else (0.0, 25, 0.6, 0, 0)
    v = pcvignette if pcvignette is not None else (0.6, 50, 50, 0, 0)
    c = crop if crop is not None else (0, 0, 0, 0)
    return CgParams(int(gradient is not None), float(g[0]), int(g[1]), float(g[2]), int(g[3]), int(g[4]),
                    int(pcvignette is not None), float(v[0]), int(v[1]), int(v[2]), int(v[3]), int(v[4]),
                    int(crop is not None), int(c[0]), int(c[1]), int(c[2]), int(c[3]),
                    int(offset[0]), int(offset[1]), int(full[0]), int(full[1]), float(scale))


def capi_cg_params(p):
    from art_amd import capi
    return capi.CreativeGradientsParams.from_buffer_copy(bytes(p))


def cg_derive(p, w, h):
    d = CgDerived()
    checker().cr_cg_derive(C.byref(p), int(w), int(h), C.byref(d))
    return d


def creative_gradients(img, p, want_factors=False, want_args=False):
    """ImProcFunctions::creativeGradients on three H x W planes -> (planes, counts[, gradient factors, vignette factors][, xsinf args, xcosf args])"""
    out, w, h = _copies(img)
    cn = CgCounts()
    gf = np.ones((h, w), np.float32) if want_factors else None
    vf = np.ones((h, w), np.float32) if want_factors else None
    cap = 2 * w * h
    sa = np.zeros(cap, np.float32) if want_args else None
    ca = np.zeros(cap, np.float32) if want_args else None
    ns, nc = C.c_longlong(0), C.c_longlong(0)
    ptr = lambda a: None if a is None else a.ctypes.data_as(_fp)
    checker().cr_creative_gradients(*[a.ctypes.data_as(_fp) for a in out], w, w, h, C.byref(p), ptr(gf), ptr(vf), ptr(sa), ptr(ca), cap,
                                    C.byref(ns), C.byref(nc), C.byref(cn))
    res = [out, _dict(cn)]
    if want_factors:
        res += [gf, vf]
    if want_args:
        res += [sa[:ns.value], ca[:nc.value]]
    return tuple(res)


# The cases of the GPU tests.  The factors do not depend on the pixel values, so every configuration runs on one value family, the families
# taking turns down the list, and one configuration of each tool runs on all of them
GRAD_DEGREES = (0, 0.05, 45, 90, 135, 180, 225, 270, 315, -30, 400)       # 0.05 degrees is below the 0.001 rad snap
GRAD_FEATHERS = (0, 25, 100)
GRAD_STRENGTHS = (2.0, -1.5)                                               # scale < 1: the sin form; scale > 1: the cos form
GRAD_CENTRES = ((0, 0), (100, -60), (-100, 60))
PCV_ROUNDNESS = (0, 20, 49, 50, 51, 100)
PCV_FEATHERS = (0, 50, 100)
PCV_STRENGTHS = (0.6, 6.0, -2.0)                                           # 6.0: scale exactly 0; -2: the sin form
PCV_CENTRES = ((0, 0), (40, -30))


def gradient_configs():
    return [cg_params(gradient=(d, f, s, cx, cy)) for d in GRAD_DEGREES for f in GRAD_FEATHERS for s in GRAD_STRENGTHS for cx, cy in GRAD_CENTRES]


def pcvignette_configs():
    return [cg_params(pcvignette=(s, f, r, cx, cy)) for r in PCV_ROUNDNESS for f in PCV_FEATHERS for s in PCV_STRENGTHS for cx, cy in PCV_CENTRES]


WINDOW = (45, 67)            # (h, w) of the two geometry cases
# a 67 x 45 window at (13, 7) of a 300 x 200 picture
GRAD_WINDOW = cg_params(gradient=(-30, 25, 2.0, 20, -10), offset=(13, 7), full=(300, 200))
# a crop at scale 2: the box is (10, 8) + 30 x 20 of the 67 x 45 frame, the fade reaches 1 about four pixels outside it
PCV_CROP = cg_params(pcvignette=(0.6, 50, 20, 0, 0), crop=(20, 16, 60, 40), scale=2.0)
BOTH = cg_params(gradient=(30, 40, 1.2, 10, -20), pcvignette=(1.5, 60, 30, -20, 10))
BOTH_BRIGHT = cg_params(gradient=(200, 60, -0.8, 0, 0), pcvignette=(-1.0, 80, 70, 0, 0))


def cg_case(h, w, family, p):
    key = ("cg", h, w, family, bytes(p))
    if key not in _CACHE:
        img = scene(h, w, family)
        want, counts = creative_gradients(img, p)
        for a in want:
            a.setflags(write=False)
        _CACHE[key] = (img, want, counts)
    return _CACHE[key]


def cast_tables():
    """two smooth synthetic tables in the range ART's have (y * u, y * v with |u|, |v| well below 1): not ART's, which need DiagonalCurve's spline"""
    x = np.arange(65536, dtype=np.float64) / 65535.0
    sat = np.sin(np.pi * x) ** 2
    y = 65535.0 * x ** 0.8
    return (y * 0.11 * sat).astype(np.float32), (y * -0.07 * sat).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes: the value-domain families of tests/value_domains.py on three planes, one with +-inf in it and one with NaNs
# ---------------------------------------------------------------------------------------------------------------------------------------
FAMILIES = VD.NAMES + ("inf_plane",)
_SCENES = {}
_CACHE = {}


def scene(h, w, family):
    """three read-only h x w planes.  inf_plane: scaled_frac with +inf and -inf spread over the planes; nan_plane (soft light only): with NaNs too"""
    key = (h, w, family)
    if key not in _SCENES:
        rng = np.random.default_rng(17 + 131 * w + h)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        planes = []
        for c, f in enumerate((1.0, 0.8, 0.55)):
            base = np.clip(300.0 + 60000.0 * f * ((xx + 1) / w) * (0.3 + 0.7 * (yy + 1) / h) + rng.normal(0.0, 900.0, (h, w)), 0.0, 65535.0)
            base = np.rint(base)
            p = VD.derive("scaled_frac" if family in ("inf_plane", "nan_plane") else family, base)
            if family in ("inf_plane", "nan_plane"):
                flat = p.reshape(-1)
                flat[c::5] = np.inf
                flat[(c + 2)::7] = -np.inf
                if family == "nan_plane":
                    flat[(c + 1)::3] = np.nan
            planes.append(p)
        for p in planes:
            p.setflags(write=False)
        _SCENES[key] = planes
    return _SCENES[key]


# black-and-white: every setting once and every filter once, gamma on and off, free mixers; (setting, filter, mixer, gamma)
def bw_configs():
    out = []
    for i, s in enumerate(SETTINGS):
        out.append((s, FILTERS[i % len(FILTERS)], (40 + i, 30 - 2 * i, 25 + 3 * i), (0, 0, 0) if i % 2 else (20, -35, 60)))
    out.append(("RGB-Abs", "None", (-40, 200, -17), (0, 0, 1)))
    out.append(("RGB-Rel", "Blue", (0, 0, 0), (0, 0, 0)))
    return out


def sl_case(h, w, family, strength):
    key = ("sl", h, w, family, strength)
    if key not in _CACHE:
        img = scene(h, w, family)
        want, counts, ran = soft_light(img, strength)
        assert ran
        for a in want:
            a.setflags(write=False)
        _CACHE[key] = (img, want, counts)
    return _CACHE[key]


def bw_case(h, w, family, cfg, cast=False):
    key = ("bw", h, w, family, cfg, cast)
    if key not in _CACHE:
        img = scene(h, w, family)
        setting, filt, mixer, gamma = cfg
        ul, vl = cast_tables() if cast else (None, None)
        want, counts = black_and_white(img, setting, filt, mixer, gamma, 30 if cast else 0, ul, vl)
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
