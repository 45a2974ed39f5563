"""Raw CA correction: the CPU checker (tests/emul/ca_correct_ref.cc) driven through the reference's iteration loop, and a synthetic
Bayer frame with known lateral CA.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "ca_correct_ref.cc")
SO = os.path.join(HERE, "emul", "libca_correct_ref.so")
_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
_LIB = None


def checker():
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO) or os.path.getmtime(SRC) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-math-errno", "-msse2",
                                   "-o", SO, SRC])
        _LIB = C.CDLL(SO)
    return _LIB


def sizes(w, h):
    out = (C.c_int * 8)()
    checker().ca_ref_sizes(w, h, out)
    return list(out)


def ca_correct(raw, filters, autocorrect=True, iterations=2, red=0.0, blue=0.0, avoid_colour_shift=True, want_info=False):
    """CA_correct_RT on a copy of `raw` (float32 H x W): returns (raw, fitparams (2, 2, 16)[, info])."""
    lib = checker()
    raw = np.ascontiguousarray(raw, dtype=np.float32).copy()
    h, w = raw.shape
    s = sizes(w, h)
    gtmp = np.zeros(s[0], np.float32)
    rdt = np.zeros(s[0], np.float32)
    blocks = np.zeros(s[1], np.float32)
    fit = np.zeros(64, np.float64)
    fw, fh = s[2], s[3]
    oldraw = np.zeros((s[5], s[4]), np.float32)
    if avoid_colour_shift:
        lib.ca_ref_capture(raw.ctypes.data_as(_fp), w, h, C.c_uint(filters), oldraw.ctypes.data_as(_fp))
    red_f = np.zeros((fh, fw), np.float32)
    blue_f = np.zeros((fh, fw), np.float32)
    n = max(int(iterations), 1) if autocorrect else 1
    pp, ran, polyord = 1, 0, C.c_int(4)
    for _ in range(n):
        if not pp:
            break
        pp = lib.ca_ref_iteration(raw.ctypes.data_as(_fp), w, h, C.c_uint(filters), 1 if autocorrect else 0, C.c_double(red),
                                  C.c_double(blue), gtmp.ctypes.data_as(_fp), rdt.ctypes.data_as(_fp), blocks.ctypes.data_as(_fp),
                                  fit.ctypes.data_as(_dp), C.byref(polyord))
        ran += 1
        if avoid_colour_shift:
            lib.ca_ref_factors(raw.ctypes.data_as(_fp), oldraw.ctypes.data_as(_fp), w, h, C.c_uint(filters), red_f.ctypes.data_as(_fp),
                               blue_f.ctypes.data_as(_fp))
            red_f = oracle_lib.gaussian_blur(red_f, 30.0)
            blue_f = oracle_lib.gaussian_blur(blue_f, 30.0)
            lib.ca_ref_apply(raw.ctypes.data_as(_fp), w, h, C.c_uint(filters), red_f.ctypes.data_as(_fp), blue_f.ctypes.data_as(_fp))
    info = {"iterations_run": ran, "processpasstwo": bool(pp), "polyord": polyord.value, "vblsz": s[6], "hblsz": s[7]}
    return (raw, fit.reshape(2, 2, 16), info) if want_info else (raw, fit.reshape(2, 2, 16))


def fc(filters, r, c):
    return (filters >> ((((r << 1) & 14) + (c & 1)) << 1)) & 3


def scene(x, y):
    """a neutral scene with edges in every direction (values 3000 .. 43000)"""
    v = np.sin(2 * np.pi * x / 37.0) * np.sin(2 * np.pi * y / 29.0) + 0.6 * np.sin(2 * np.pi * (x + y) / 53.0)
    return 3000.0 + 40000.0 / (1.0 + np.exp(-6.0 * v))


def lateral_ca_frame(w, h, filters, k_red=0.002, k_blue=-0.0015, noise=60.0, seed=1, flat=False):
    """Bayer frame of `scene` where R / B are rendered at coordinates scaled by 1 + k about the centre: at pixel x, R sees the scene at
    c + (x - c)(1 + k), i.e. R(x) = G(x + (x - c) k)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    col = np.zeros((h, w), np.int64)
    for r in range(2):
        for c in range(2):
            col[r::2, c::2] = fc(filters, r, c)
    scale = np.where(col == 0, 1.0 + k_red, np.where(col == 2, 1.0 + k_blue, 1.0))
    X = cx + (xx - cx) * scale
    Y = cy + (yy - cy) * scale
    v = np.full((h, w), 20000.0) if flat else scene(X, Y)
    if noise and not flat:
        v = v + rng.normal(0.0, noise, v.shape)
    return np.clip(v, 0.0, 65535.0).astype(np.float32)
