"""Local contrast: the CPU checker (tests/emul/local_contrast_ref.cc) driven around the oracle's wavelet decomposition, the mask blend
of ImProcFunctions::localContrast, and the L planes the tests use.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
SRC = os.path.join(HERE, "emul", "local_contrast_ref.cc")
SO = os.path.join(HERE, "emul", "liblocal_contrast_ref.so")
_fp = C.POINTER(C.c_float)
_LIB = None

DEFAULT_CURVE_POINTS = (1.0, 0.0, 0.5, 0.0, 0.0, 1.0, 0.5, 0.0, 0.0)        # LocalContrastParams::Region (procparams.cc:1700-1714)
BOOST_CURVE_POINTS = (1.0, 0.0, 0.5, 0.35, 0.35, 0.3, 0.85, 0.35, 0.35, 0.75, 0.6, 0.35, 0.35, 1.0, 0.5, 0.35, 0.35)
CUT_CURVE_POINTS = (1.0, 0.0, 0.45, 0.35, 0.35, 0.4, 0.15, 0.35, 0.35, 1.0, 0.3, 0.35, 0.35)


class Info(C.Structure):
    """lc_ref_info, the layout of artgpu_local_contrast_info"""
    _fields_ = [("nlevels", C.c_int32), ("ave", C.c_float), ("min0", C.c_float), ("max0", C.c_float),
                ("mean", C.c_float * 10), ("sigma", C.c_float * 10), ("maxp", C.c_float * 10)]


class Counts(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in ("branch_max", "branch_mid", "branch_low", "clipped_above", "floor_hits", "c0_skipped",
                                            "nan_left", "levels_skipped")]

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


def levels(w, h):
    return int(checker().lc_ref_levels(int(w), int(h)))


def curve_lut(points):
    """WavOpacityCurveWL::Set from the oracle's FlatCurve: the 501-entry LUT, or None where the reference leaves it unset"""
    if not (len(points) > 0 and 0.0 < points[0] < 2.0):
        return None
    v, ident = oracle_lib.flat_curve_sample(points, False, 500, 0.0, 501)
    return None if ident else v.astype(np.float32)


def info_tuple(i):
    """(nlevels, ave, min0, max0, mean, sigma, maxp) of an Info-shaped structure, floats as float32 arrays"""
    n = int(i.nlevels)
    return (n, np.float32(i.ave), np.float32(i.min0), np.float32(i.max0), np.array(i.mean[:n], np.float32),
            np.array(i.sigma[:n], np.float32), np.array(i.maxp[:n], np.float32))


def info_fields(i):
    """every field of an Info-shaped structure (all ten entries of the three arrays) as a tuple of ints and float32 bit patterns, each NaN as
    one pattern: which NaN an operation returns is not shared between the two machines"""
    def f(v):
        v = np.float32(v)
        return 0x7fc00000 if np.isnan(v) else int(v.view(np.uint32))
    return (int(i.nlevels), f(i.ave), f(i.min0), f(i.max0)) + tuple(f(v) for name in ("mean", "sigma", "maxp") for v in getattr(i, name))


def copy_info(src):
    """an Info with the fields of any structure of that layout (capi.LocalContrastInfo)"""
    dst = Info()
    C.memmove(C.byref(dst), C.byref(src), C.sizeof(Info))
    return dst


def local_contrast_wavelets(L, contrast, curve, stats=None):
    """local_contrast_wavelets (iplocalcontrast.cc:251-420) on a copy of L (float32 H x W): decomposition and reconstruction by the
    oracle, everything between them by the checker, on views of the oracle's own bands and coeff0.
    stats: an Info to use in place of the checker's own statistics.  Returns (L_new, Info, counts dict)."""
    lib = checker()
    L = np.ascontiguousarray(L, dtype=np.float32)
    h, w = L.shape
    nl = levels(w, h)
    d = oracle_lib.wavelet_decompose(L, nl)
    o = d.contents
    n = o.w2 * o.h2
    bands = (_fp * (3 * nl))(*[o.band[l][k + 1] for l in range(nl) for k in range(3)])
    cv = None if curve is None else np.ascontiguousarray(curve, dtype=np.float32)
    assert cv is None or cv.shape == (501,)
    out, counts = Info(), Counts()
    lib.lc_ref_apply(bands, o.coeff0, n, nl, C.c_double(float(contrast)), None if cv is None else cv.ctypes.data_as(_fp),
                     None if stats is None else C.byref(stats), C.byref(out), C.byref(counts))
    rec = oracle_lib.wavelet_reconstruct(d, h, w, 1.0)
    return rec, out, counts.as_dict()


def plain_round_trip(L):
    L = np.ascontiguousarray(L, dtype=np.float32)
    h, w = L.shape
    return oracle_lib.wavelet_reconstruct(oracle_lib.wavelet_decompose(L, levels(w, h)), h, w, 1.0)


def blend(mask, L_new, l):
    """rgb->g = intp(blend, L, l) = blend * L + (1 - blend) * l in float (rt_math.h:109-118)"""
    m = np.float32(1.0) if mask is None else np.asarray(mask, np.float32)
    return (m * L_new + (np.float32(1.0) - m) * l).astype(np.float32)


def local_contrast(L, regions, stats=None):
    """ImProcFunctions::localContrast's region loop (L463-481): regions = [(contrast, curve LUT or None, mask or None), ...];
    stats: per region an Info or None.  Returns (L, [Info per region], [counts per region])."""
    L = np.ascontiguousarray(L, dtype=np.float32).copy()
    infos, counts = [], []
    for k, (contrast, curve, mask) in enumerate(regions):
        new, info, cn = local_contrast_wavelets(L, contrast, curve, None if stats is None else stats[k])
        L = blend(mask, new, L)
        infos.append(info)
        counts.append(cn)
    return L, infos, counts


def l_plane(w, h, seed=1, noise=300.0, highlight=False, flat=None):
    """An L plane in 0 .. 32768: smooth structure at several scales plus noise of a few hundred units, so that every wavelet level has
    coefficients on both sides of +-5; highlight: a patch rising to about 40000 (coeff0 entries at and above 32768)."""
    if flat is not None:
        return np.full((h, w), flat, np.float32)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 15000.0 + 7000.0 * np.sin(2 * np.pi * xx / 97.0) * np.cos(2 * np.pi * yy / 71.0) + 4000.0 * np.sin(2 * np.pi * (xx + 2 * yy) / 23.0)
    v += 1500.0 * np.sign(np.sin(2 * np.pi * xx / 11.0) * np.sin(2 * np.pi * yy / 13.0))
    v += rng.normal(0.0, noise, v.shape)
    v = np.clip(v, 0.0, 32768.0)
    if highlight:
        r2 = ((xx - 0.7 * w) / (0.22 * w)) ** 2 + ((yy - 0.35 * h) / (0.22 * h)) ** 2
        v = np.maximum(v, 40000.0 * np.exp(-0.5 * r2))
    return v.astype(np.float32)
