"""Dehaze: the CPU checker (tests/emul/dehaze_ref.cc: ImProcFunctions::dehaze restated serially around the oracle's guided filter,
box blur, FlatCurve and LUTf) and the hazy scenes the tests use.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
SRC = os.path.join(HERE, "emul", "dehaze_ref.cc")
SO = os.path.join(HERE, "emul", "libdehaze_ref.so")
_fp = C.POINTER(C.c_float)
_LIB = None

DEFAULT_STRENGTH = (1.0, 0.0, 0.75, 0.0, 0.0, 1.0, 0.75, 0.0, 0.0)                  # DehazeParams (procparams.cc:2694-2711)
# crosses 0.5: negative strengths (add haze) in the highlights
CROSSING_STRENGTH = (1.0, 0.0, 0.9, 0.35, 0.35, 0.45, 0.7, 0.35, 0.35, 0.8, 0.2, 0.35, 0.35, 1.0, 0.1, 0.35, 0.35)
IDENTITY_STRENGTH = (1.0, 0.0, 0.5, 0.35, 0.35, 0.6, 0.5, 0.35, 0.35, 1.0, 0.5, 0.0, 0.0)
STRONG_STRENGTH = (1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0)


class Params(C.Structure):
    _fields_ = [("show_depth_map", C.c_int32), ("depth", C.c_int32), ("luminance", C.c_int32), ("blackpoint", C.c_int32)]


class Info(C.Structure):
    """dh_ref_info, the layout of artgpu_dehaze_info"""
    _fields_ = [("haze_detected", C.c_int32), ("patchsize", C.c_int32), ("small_w", C.c_int32), ("small_h", C.c_int32),
                ("maxval", C.c_float), ("black", C.c_float * 3), ("ambient", C.c_float * 3), ("max_t", C.c_float), ("t0", C.c_float)]


class Hand(C.Structure):
    _fields_ = [("use", C.c_int32), ("ambient", C.c_float * 3), ("max_t", C.c_float), ("maxval", C.c_float), ("black", C.c_float * 3)]


class Counts(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in ("add_haze", "y_small", "won_t", "won_t0", "won_tl", "dark_clipped_low", "dark_clipped_high",
                                            "partial_patches", "no_haze", "depth_below", "depth_above")]

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
        _LIB.dh_ref_estimate_ambient.restype = C.c_float
    return _LIB


def info_fields(i):
    """the fields of an Info-shaped structure as a tuple of ints and float32 bit patterns"""
    f = lambda v: int(np.float32(v).view(np.uint32))
    return (int(i.haze_detected), int(i.patchsize), int(i.small_w), int(i.small_h), f(i.maxval), tuple(f(v) for v in i.black),
            tuple(f(v) for v in i.ambient), f(i.max_t), f(i.t0))


def thumb_size(w, h):
    ww, hh = C.c_int(0), C.c_int(0)
    checker().dh_ref_thumb_size(int(w), int(h), C.byref(ww), C.byref(hh))
    return ww.value, hh.value


def strength_lut(points):
    pts = (C.c_double * max(len(points), 1))(*[float(p) for p in points])
    lut = np.zeros(65536, np.float32)
    checker().dh_ref_strength_lut(pts, len(points), lut.ctypes.data_as(_fp))
    return lut


def estimate_ambient(R, G, B):
    planes = [np.ascontiguousarray(a, dtype=np.float32) for a in (R, G, B)]
    hh, ww = planes[0].shape
    ambient = (C.c_float * 3)()
    max_t = checker().dh_ref_estimate_ambient(*[a.ctypes.data_as(_fp) for a in planes], ww, hh, ambient)
    return np.array(ambient[:], np.float32), np.float32(max_t)


def dark_channel(R, G, B, patchsize, ambient=None, clip=False):
    planes = [np.ascontiguousarray(a, dtype=np.float32) for a in (R, G, B)]
    h, w = planes[0].shape
    dst = np.full((h, w), np.nan, np.float32)
    amb = None if ambient is None else (C.c_float * 3)(*[float(v) for v in ambient])
    cn = Counts()
    checker().dh_ref_dark_channel(*[a.ctypes.data_as(_fp) for a in planes], w, h, int(patchsize), amb, 1 if clip else 0, dst.ctypes.data_as(_fp),
                                  C.byref(cn))
    return dst, cn.as_dict()


def dehaze(img, strength=DEFAULT_STRENGTH, depth=25, show_depth_map=False, luminance=False, blackpoint=0, ws=None, scale=1.0, hand=None):
    """ImProcFunctions::dehaze on copies of three H x W planes.  hand: a Hand (use = 1) whose maxval, black, ambient and max_t replace the
    checker's own.  Returns (planes, Info, counts dict), or None where the reference would read out of bounds."""
    ws = oracle_lib.REC2020_WS_D if ws is None else ws
    out = [np.array(a, dtype=np.float32, order="C") for a in img]
    h, w = out[0].shape
    pts = (C.c_double * max(len(strength), 1))(*[float(p) for p in strength])
    wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
    p = Params(1 if show_depth_map else 0, int(depth), 1 if luminance else 0, int(blackpoint))
    info, cn = Info(), Counts()
    rc = checker().dh_ref_dehaze(*[a.ctypes.data_as(_fp) for a in out], w, h, pts, len(strength), C.byref(p), wsd, C.c_double(float(scale)),
                                 None if hand is None else C.byref(hand), C.byref(info), C.byref(cn))
    if rc:
        return None
    return out, info, cn.as_dict()


def hand_from(info):
    """a Hand carrying the values of an Info-shaped structure (the library's artgpu_dehaze_info, or the checker's)"""
    hd = Hand()
    hd.use = 1
    hd.max_t = info.max_t
    hd.maxval = info.maxval
    for k in range(3):
        hd.ambient[k] = info.ambient[k]
        hd.black[k] = info.black[k]
    return hd


def hazy_scene(w, h, seed=1, zero_block=False, bright_block=False, veil=(30000.0, 31000.0, 32500.0)):
    """A synthetic frame J (coloured structure at several scales, 200 .. 28000) seen through haze: I = J * t + A * (1 - t) with the
    transmission t a ramp from 0.95 (bottom left) to 0.15 (top right) and the veil A.  zero_block: a block of exact zeros;
    bright_block: a block at 45000 .. 60000 (above 32768, brighter than the veil in every channel)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    t = 0.95 - 0.8 * (0.6 * xx / max(w - 1, 1) + 0.4 * (1.0 - yy / max(h - 1, 1)))
    for c in range(3):
        j = 9000.0 + 6000.0 * np.sin(2 * np.pi * (xx + 7 * c) / (37.0 + 5 * c)) * np.cos(2 * np.pi * yy / (29.0 + 3 * c))
        j += 5000.0 * np.sign(np.sin(2 * np.pi * xx / 17.0) * np.sin(2 * np.pi * (yy + 3 * c) / 13.0))
        j += rng.normal(0.0, 400.0, j.shape)
        j = np.clip(j, 200.0, 28000.0)
        v = j * t + veil[c] * (1.0 - t)
        if bright_block:
            by, bx = slice(h // 8, h // 8 + max(h // 4, 6)), slice(w // 2, w // 2 + max(w // 5, 12))
            v[by, bx] = 45000.0 + 5000.0 * c + rng.uniform(0.0, 5000.0, v[by, bx].shape)
        if zero_block:
            zy, zx = slice(h // 2, h // 2 + max(h // 5, 5)), slice(w // 10, w // 10 + max(w // 6, 10))
            v[zy, zx] = 0.0
        planes.append(v.astype(np.float32))
    return planes


# The cases of the GPU comparison (tests/test_gpu_dehaze.py); tests/test_dehaze_checker.py shows from the checker's counters that they take
# every branch.  name: (w, h, seed, strength, depth, show_depth_map, luminance, blackpoint, scale, zero block, bright block)
CASES = {
    "300x200-default": (300, 200, 1, DEFAULT_STRENGTH, 25, False, False, 0, 1.0, False, False),             # guided subsampling 1, patch 2
    "300x200-strong-depth0": (300, 200, 2, STRONG_STRENGTH, 0, False, False, 0, 1.0, True, False),
    "723x481-crossing-black50-depth100": (723, 481, 3, CROSSING_STRENGTH, 100, False, False, 50, 1.0, False, True),   # subsampling 5 and 4, 1-wide edge patches
    "481x723-luminance": (481, 723, 4, CROSSING_STRENGTH, 25, False, True, 0, 1.0, True, True),             # portrait thumbnail rule
    "1803x97-depthmap-scale2": (1803, 97, 5, STRONG_STRENGTH, 100, True, False, 0, 2.0, True, True),         # patch 3, radius 12
    "7801x41-patch13": (7801, 41, 6, DEFAULT_STRENGTH, 100, False, False, 0, 1.0, False, True),             # patch 13 through the whole call
}
_CASE_CACHE = {}


def case(name):
    """(input planes, keyword arguments of dehaze(), the checker's planes, Info and counts), computed once and read-only"""
    if name not in _CASE_CACHE:
        w, h, seed, strength, depth, show, lum, bp, scale, zero, bright = CASES[name]
        img = hazy_scene(w, h, seed=seed, zero_block=zero, bright_block=bright)
        kw = dict(strength=strength, depth=depth, show_depth_map=show, luminance=lum, blackpoint=bp, scale=scale)
        want, info, counts = dehaze(img, **kw)
        for a in img + want:
            a.setflags(write=False)
        _CASE_CACHE[name] = (img, kw, want, info, counts)
    return _CASE_CACHE[name]
