"""Impulse noise reduction and defringe: the CPU checker (tests/emul/impulse_defringe_ref.cc: markImpulse, impulse_nr, gauss3x3 and PF_correct_RT
restated serially around the oracle's gaussian blur, xatan2f, FlatCurve and Lab conversions) and the scenes the tests use.  Test infrastructure only.

The tools take an image in RGB mode; the checker works on the LAB planes, so impulse_denoise() and defringe() here switch modes with the oracle's
Imagefloat::rgb_to_lab / lab_to_rgb around it, as the entry points do with artgpu_rgb_to_lab / artgpu_lab_to_rgb."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
SRC = os.path.join(HERE, "emul", "impulse_defringe_ref.cc")
SO = os.path.join(HERE, "emul", "libimpulse_defringe_ref.so")
_fp = C.POINTER(C.c_float)
_bp = C.POINTER(C.c_ubyte)
_dp = C.POINTER(C.c_double)
_LIB = None

WS, IWS = oracle_lib.REC2020_WS_D, oracle_lib.REC2020_IWS_D
# DefringeParams' default hue curve (procparams.cc:1839-1865)
DEFAULT_HUECURVE = (1.0, 0.166666667, 0., 0.35, 0.35, 0.347, 0., 0.35, 0.35, 0.513667426, 0., 0.35, 0.35, 0.668944571, 0., 0.35, 0.35,
                    0.8287775246, 0.97835991, 0.35, 0.35, 0.9908883827, 0., 0.35, 0.35)
# a curve that is below 0.5 over the yellow and green hues of the scenes' background and green spots: chparam < 0 there (the `*= 2.f` branch)
NEGATIVE_HUECURVE = (1.0, 0.1, 0.3, 0.35, 0.35, 0.45, 0.1, 0.35, 0.35, 0.8, 0.9, 0.35, 0.35)
CURVES = {"default": DEFAULT_HUECURVE, "none": (), "negative": NEGATIVE_HUECURVE}

# the share of flagged pixels every scene must have, from the checker alone: a scene that flags nothing would pass every comparison
IMPULSE_SHARE = (0.002, 0.25)
DEFRINGE_SHARE = (0.01, 0.30)


class DefringeInfo(C.Structure):
    """id_ref_defringe_info, the layout of artgpu_defringe_info"""
    _fields_ = [("early_out", C.c_int32), ("halfwin", C.c_int32), ("blur", C.c_int32), ("curve", C.c_int32), ("radius", C.c_double),
                ("chromave", C.c_double), ("threshfactor", C.c_float), ("pad_", C.c_int32), ("corrected_pixels", C.c_int64)]


def checker():
    global _LIB
    if _LIB is None:
        oracle_lib.lib()            # builds liboracle.so when needed and leaves it loaded
        if not os.path.exists(SO) or os.path.getmtime(SRC) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-msse2", "-o", SO, SRC,
                                   "-L" + ORACLE_DIR, "-loracle", "-Wl,-rpath," + ORACLE_DIR])
        _LIB = C.CDLL(SO)
        _LIB.id_ref_mark_impulse.restype = C.c_longlong
        _LIB.id_ref_impulse_nr.restype = C.c_longlong
        _LIB.id_ref_ordered_sum.restype = C.c_double
    return _LIB


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def nbad(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return int((~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)))).sum())


# ---- impulse noise reduction

def mark_impulse(L, thresh):
    L = np.ascontiguousarray(L, dtype=np.float32)
    h, w = L.shape
    imp = np.zeros((h, w), np.uint8)
    n = checker().id_ref_mark_impulse(L.ctypes.data_as(_fp), imp.ctypes.data_as(_bp), w, h, C.c_float(thresh))
    return imp, int(n)


def impulse_derived(thresh, scale):
    """(thresh, sigma, impthr) as float32, what markImpulse receives and derives"""
    out = np.zeros(3, np.float32)
    checker().id_ref_impulse_derived(int(thresh), C.c_double(float(scale)), out.ctypes.data_as(_fp))
    return out


def impulse_nr(lab, thresh, backwards=False):
    """impulse_nr on copies of the LAB planes [a, L, b] -> (planes, impulse map, pixels kept because norm == 0)"""
    a, L, b = [np.array(p, dtype=np.float32, order="C") for p in lab]
    h, w = L.shape
    imp = np.zeros((h, w), np.uint8)
    kept = C.c_longlong(0)
    checker().id_ref_impulse_nr(L.ctypes.data_as(_fp), a.ctypes.data_as(_fp), b.ctypes.data_as(_fp), w, h, C.c_float(thresh), 1 if backwards else 0,
                                imp.ctypes.data_as(_bp), C.byref(kept))
    return [a, L, b], imp, int(kept.value)


def impulse_gate(w, h, enabled, scale):
    """artgpu_impulse_denoise_info::early_out"""
    return 1 if not enabled else 2 if (w < 8 or h < 8) else 3 if not (scale >= 0.5) else 0


def impulse_denoise(img, thresh=50, scale=1.0, enabled=True, to_rgb=True):
    """ImProcFunctions::impulsedenoise on copies of RGB planes -> (planes, dict of what artgpu_impulse_denoise_info holds, pixels kept)"""
    h, w = img[0].shape
    early = impulse_gate(w, h, enabled, scale)
    info = dict(early_out=early, thresh=np.float32(0), sigma=np.float32(0), impthr=np.float32(0), impulse_pixels=0)
    if early:
        return [np.array(p, dtype=np.float32) for p in img], info, 0
    t, sigma, impthr = impulse_derived(thresh, scale)
    lab = oracle_lib.image_rgb_to_lab(img, WS)
    out, imp, kept = impulse_nr(lab, t)
    info.update(thresh=t, sigma=sigma, impthr=impthr, impulse_pixels=int(np.count_nonzero(imp)))
    if to_rgb:
        out = oracle_lib.image_lab_to_rgb(out, IWS)
    return out, info, kept


def impulse_info_fields(i):
    """an ImpulseDenoiseInfo structure or the dict above as a tuple of ints and bit patterns"""
    g = (lambda k: i[k]) if isinstance(i, dict) else (lambda k: getattr(i, k))
    return (int(g("early_out")),) + tuple(int(np.float32(g(k)).view(np.uint32)) for k in ("thresh", "sigma", "impthr")) + (int(g("impulse_pixels")),)


# ---- defringe

def gauss3x3(src, sigma):
    src = np.ascontiguousarray(src, dtype=np.float32)
    h, w = src.shape
    dst = np.full((h, w), np.nan, np.float32)
    checker().id_ref_gauss3x3(src.ctypes.data_as(_fp), dst.ctypes.data_as(_fp), w, h, C.c_double(sigma))
    return dst


def gauss3x3_coef(sigma):
    out = np.zeros(5, np.float32)
    checker().id_ref_gauss3x3_coef(C.c_double(sigma), out.ctypes.data_as(_fp))
    return out


def ordered_sum(x):
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    return float(checker().id_ref_ordered_sum(x.ctypes.data_as(_fp), C.c_longlong(x.size)))


def pf_correct(lab, radius, thresh, huecurve=DEFAULT_HUECURVE, order=0):
    """PF_correct_RT on copies of the LAB planes [a, L, b] -> (planes, DefringeInfo, map of corrected pixels), or None where the device path
    refuses.  order 0: the definition; 1: raster order in place; 2: 16-row chunks last to first, in place."""
    a, L, b = [np.array(p, dtype=np.float32, order="C") for p in lab]
    h, w = L.shape
    pts = np.asarray(huecurve, np.float64)
    flagged = np.zeros((h, w), np.uint8)
    info = DefringeInfo()
    rc = checker().id_ref_defringe(a.ctypes.data_as(_fp), b.ctypes.data_as(_fp), w, h, C.c_double(float(radius)), int(thresh),
                                   pts.ctypes.data_as(_dp) if pts.size else None, int(pts.size), int(order), flagged.ctypes.data_as(_bp), C.byref(info))
    if rc:
        return None
    info.curve = 0 if not (pts.size and int(pts[0]) > 0) else 1        # (none of the curves used here is one FlatCurve leaves empty)
    return [a, L, b], info, flagged


def defringe(img, radius=2.0, threshold=13, huecurve=DEFAULT_HUECURVE, scale=1.0, enabled=True, to_rgb=True, order=0):
    """ImProcFunctions::defringe on copies of RGB planes -> (planes, DefringeInfo, map of corrected pixels), or None where the device path refuses"""
    h, w = img[0].shape
    if not enabled or w < 8 or h < 8:
        info = DefringeInfo()
        info.early_out = 1 if not enabled else 2
        return [np.array(p, dtype=np.float32) for p in img], info, np.zeros((h, w), np.uint8)
    lab = oracle_lib.image_rgb_to_lab(img, WS)
    res = pf_correct(lab, radius / scale, threshold, huecurve, order)
    if res is None:
        return None
    out, info, flagged = res
    if to_rgb:
        out = oracle_lib.image_lab_to_rgb(out, IWS)
    return out, info, flagged


def defringe_info_fields(i):
    return (int(i.early_out), int(i.halfwin), int(i.blur), int(i.curve), int(np.float64(i.radius).view(np.uint64)), int(np.float64(i.chromave).view(np.uint64)),
            int(np.float32(i.threshfactor).view(np.uint32)), int(i.corrected_pixels))


# ---- scenes (RGB mode, values 0 .. 65535)

def impulse_scene(w, h, seed=1, density=0.10, block=False):
    """A gentle luminance ramp (with a soft edge in the larger images) whose only noise is sparse: `density` of the pixels are off, a fifth of them
    by a large factor (salt and pepper), the others by 15 % times a log-normal amplitude; every column range of markImpulse's loops gets one.
    Dense noise would not do: at impthr 1 a pixel is impish when its high-pass value exceeds the mean of its neighbours', which symmetric noise
    does for a third of all pixels.  block: a 5 x 5 cone, brightest in the middle, whose every pixel exceeds the mean of its own window at
    impthr 1: the centre's whole neighbourhood is impish, norm == 0."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for c in range(3):
        v = 9000.0 + 2000.0 * c + 3.0 * xx + 2.0 * yy
        if w * h >= 1000:       # (a small image is all edge to a blur of sigma 4: its high-pass plane would be the edge, not the speckles)
            v += 8000.0 / (1.0 + np.exp(-(xx - 0.45 * w - 0.3 * yy) / 1.5))
        planes.append(v + rng.normal(0.0, 0.5, v.shape))
    spk = np.random.default_rng(seed + 100)
    small = w * h < 1000        # to a blur of sigma 4 a small image is all neighbourhood of its salt and pepper: mild deviations only, and fewer
    hit = spk.uniform(0.0, 1.0, (h, w)) < (density * 0.6 if small else density)
    for x in (0, 1, 2, 3, w // 2, w - 6, w - 5, w - 4, w - 3, w - 2, w - 1) if not small else (0, w // 2, w - 1):
        hit[int(spk.integers(0, h)), x] = True
    strong = spk.choice([6.0, 0.08, 2.2, 0.35], size=(h, w))
    mild = 1.0 + spk.choice([-0.15, 0.15], size=(h, w)) * np.exp(spk.normal(0.0, 0.7, (h, w)))
    f = np.where(spk.uniform(0.0, 1.0, (h, w)) < (0.0 if small else 0.2), strong, mild)
    tint = spk.uniform(0.9, 1.1, (3, h, w))
    for c in range(3):
        planes[c] = np.where(hit, planes[c] * f * tint[c], planes[c])
    if block:
        assert w >= 11 and h >= 11
        cy, cx = h // 2, w // 2
        ring = np.maximum(np.abs(np.arange(-2, 3))[:, None], np.abs(np.arange(-2, 3))[None, :])
        for c in range(3):
            planes[c][cy - 4:cy + 5, cx - 4:cx + 5] = 8000.0 + 1000.0 * c
            planes[c][cy - 2:cy + 3, cx - 2:cx + 3] = np.choose(ring, [62000.0, 50000.0, 38000.0]) + 500.0 * c
    return [np.clip(p, 0.0, 65535.0).astype(np.float32) for p in planes]


def fringe_scene(w, h, seed=1, flat=False):
    """A smooth colour ramp with a little noise and saturated purple / green spots (colour fringes: chroma far from its neighbourhood's).  The
    spots have to stay rare: at threshold 60 a pixel is corrected only if its chroma is 16.5 times the image's mean, which three equal spots
    among 64 pixels already miss.  Small images get single pixels on 2 % of the pixels, larger ones discs of radius 1.2 .. 3 and a few single pixels.  flat: one colour
    everywhere, so that a - blur(a) is exactly 0 and chromave == 0."""
    if flat:
        return [np.full((h, w), v, np.float32) for v in (21000.0, 18000.0, 15000.0)]
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = [14000.0 + 90.0 * xx + 20.0 * yy, 15000.0 + 40.0 * xx + 70.0 * yy, 13000.0 + 30.0 * xx + 50.0 * yy]
    planes = [b + rng.normal(0.0, 15.0, b.shape) for b in base]
    small = w * h < 1000
    ndisc, nsingle = (0, max(1, int(round(w * h * 0.02)))) if small else ((w * h) // 600, (w * h) // 1500)
    for k in range(ndisc + nsingle):
        single = k >= ndisc         # (a corrected pixel with no other in its window is what every order of the averaging loop agrees on)
        cy, cx = (float(rng.integers(0, h)), float(rng.integers(0, w))) if single else (rng.uniform(0, h), rng.uniform(0, w))
        r = 0.5 if single else rng.uniform(1.2, 3.0)
        m = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        col = (30000.0, 5000.0, 42000.0) if k % 3 != 2 else (6000.0, 34000.0, 8000.0)
        for c in range(3):
            planes[c] = np.where(m, col[c] + rng.normal(0.0, 300.0, planes[c].shape), planes[c])
    return [np.clip(p, 0.0, 65535.0).astype(np.float32) for p in planes]


# The sizes of the GPU comparison (tests/test_gpu_impulse_defringe.py): the gates' minimum; windows clamped on both sides at once; every W mod 4
# tail of the Lab bodies and markImpulse's W - 5 range; and the averaging kernel's 32 x 32 tile crossed twice in both directions with the largest
# halo (2 tiles + 3 and 2 tiles + 6)
SIZES = ((8, 8), (9, 8), (10, 23), (11, 13), (14, 9), (67, 70))
DEFRINGE_WIDE = (21, 9)       # the narrowest class of widths radius 5 runs at (W >= 2 halfwin - 2 = 20): its windows are clamped on both sides at once
BLOCK_SIZES = ((23, 21), (67, 70))
GATE_SIZES = ((7, 9), (9, 7))
IMPULSE_PARAMS = ((0, 1.0), (50, 1.0), (100, 1.0), (50, 2.0))                 # (thresh, scale)
DEFRINGE_PARAMS = ((0.5, 1.0), (2.0, 1.0), (5.0, 1.0), (2.0, 2.0))            # (radius, scale): 3 x 3 blur + halfwin 2; 5; 11; 3 again at sigma 1
DEFRINGE_THRESHOLDS = (13, 60)
# the impulse scenes' seeds: for each size the first one with which the checker flags 1 % .. 20 % of the pixels at all four parameter sets (on a
# 64-pixel image one mild deviation more or less moves the share at impthr 1 by several per cent)
IMPULSE_SEEDS = {(8, 8): 3, (9, 8): 3, (10, 23): 2, (11, 13): 1, (14, 9): 3, (67, 70): 1}
_CACHE = {}


def impulse_case(w, h, thresh, scale, to_rgb=True, block=False):
    """(input planes, the checker's planes, info dict, pixels kept), computed once and read-only"""
    key = ("imp", w, h, thresh, scale, to_rgb, block)
    if key not in _CACHE:
        img = impulse_scene(w, h, seed=IMPULSE_SEEDS.get((w, h), 1), block=block)
        want, info, kept = impulse_denoise(img, thresh, scale, to_rgb=to_rgb)
        for a in img + want:
            a.setflags(write=False)
        _CACHE[key] = (img, want, info, kept)
    return _CACHE[key]


def defringe_case(w, h, radius, scale, threshold, curve="default", to_rgb=True, flat=False):
    """(input planes, the checker's result as defringe() returns it -- None where the device path refuses), computed once and read-only"""
    key = ("df", w, h, radius, scale, threshold, curve, to_rgb, flat)
    if key not in _CACHE:
        img = fringe_scene(w, h, seed=w * 131 + h, flat=flat)
        res = defringe(img, radius, threshold, CURVES[curve], scale, to_rgb=to_rgb)
        for a in img + (res[0] if res else []):
            a.setflags(write=False)
        _CACHE[key] = (img, res)
    return _CACHE[key]
