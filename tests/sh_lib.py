"""Capture sharpening: the CPU checker (tests/emul/sharpen_ref.cc: doSharpening for the rld method, the GAUSS_DIV / GAUSS_MULT blur forms,
markImpulse, deconvsharpening, CornerBoostMask, calcRadiusBayer restated serially around the oracle's gaussian blur, xexpf and pow_F), the
recorded outputs of the compiled reference's blur forms (tests/golden/gauss_divmult.npz) and the scenes the tests use.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
SRC = os.path.join(HERE, "emul", "sharpen_ref.cc")
SO = os.path.join(HERE, "emul", "libsharpen_ref.so")
GOLDEN = os.path.join(HERE, "golden", "gauss_divmult.npz")
_fp = C.POINTER(C.c_float)
_bp = C.POINTER(C.c_ubyte)
_LIB = None

GAUSS_MULT, GAUSS_DIV = 1, 2
RLD, USM, PSF = 0, 1, 2
# what tests/golden/make_golden_sharpen.py recorded
GOLDEN_SIGMAS = (0.22, 0.45, 0.6, 0.75, 0.84, 1.0, 1.15, 1.6, 2.5)
GOLDEN_SIZES = ((8, 8), (23, 9), (67, 41))
FILTERS_RGGB, FILTERS_GBRG = 0x94949494, 0x49494949


class Params(C.Structure):
    """sh_ref_params, the layout of artgpu_sharpening_params"""
    _fields_ = [("enabled", C.c_int32), ("method", C.c_int32), ("amount", C.c_int32), ("deconvamount", C.c_int32),
                ("contrast", C.c_double), ("deconvradius", C.c_double), ("deconvCornerBoost", C.c_double),
                ("deconvCornerLatitude", C.c_int32), ("offset_x", C.c_int32), ("offset_y", C.c_int32),
                ("full_width", C.c_int32), ("full_height", C.c_int32), ("pad_", C.c_int32)]


class Info(C.Structure):
    """sh_ref_info, the layout of artgpu_sharpening_info"""
    _fields_ = [("sigma", C.c_double), ("regime", C.c_int32), ("early_out", C.c_int32), ("contrast_threshold", C.c_float),
                ("pad_", C.c_int32), ("impulse_pixels", C.c_int64), ("frozen_pixels", C.c_int64)]


class Counts(C.Structure):
    _fields_ = [("frozen_iter", C.c_longlong * 20)] + [(n, C.c_longlong) for n in (
        "never_frozen", "impulse_lo", "impulse_vec", "impulse_body", "impulse_hi", "est_nan", "y_nonpos", "ring_pixels", "mask_low", "mask_high",
        "clip_rule_a", "clip_rule_b", "pairs")]

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n, _ in self._fields_[1:]}
        d["frozen_iter"] = [int(v) for v in self.frozen_iter]
        return d


def checker():
    global _LIB
    if _LIB is None:
        oracle_lib.lib()            # builds liboracle.so when needed and leaves it loaded
        if not os.path.exists(SO) or os.path.getmtime(SRC) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-msse2", "-o", SO, SRC,
                                   "-L" + ORACLE_DIR, "-loracle", "-Wl,-rpath," + ORACLE_DIR])
        _LIB = C.CDLL(SO)
        _LIB.sh_ref_radius.restype = C.c_float
        _LIB.sh_ref_pow_F.restype = C.c_float
        _LIB.sh_ref_pow_F.argtypes = [C.c_float, C.c_float]
    return _LIB


def info_fields(i):
    """the fields of an Info-shaped structure as a tuple of ints and bit patterns"""
    return (int(np.float64(i.sigma).view(np.uint64)), int(i.regime), int(i.early_out), int(np.float32(i.contrast_threshold).view(np.uint32)),
            int(i.impulse_pixels), int(i.frozen_pixels))


def golden():
    return np.load(GOLDEN)


def golden_key(sigma, w, h):
    return f"{sigma:g}_{w}x{h}"


def gauss(src, dst0, div, sigma, gausstype):
    """the checker's gaussianBlur(src, dst, .., gausstype, div) for src != dst -> (dst, kernel coefficients or None, src afterwards)"""
    s = np.array(src, dtype=np.float32, order="C")
    h, w = s.shape
    d = np.full((h, w), np.nan, np.float32) if gausstype == GAUSS_DIV else np.array(dst0, dtype=np.float32, order="C")
    v = None if div is None else np.ascontiguousarray(div, dtype=np.float32)
    coef = np.zeros(8, np.float32)
    rg = checker().sh_ref_gauss(s.ctypes.data_as(_fp), d.ctypes.data_as(_fp), None if v is None else v.ctypes.data_as(_fp), w, h, C.c_double(sigma),
                                int(gausstype), coef.ctypes.data_as(_fp))
    return d, (coef[:5] if rg == 2 else coef[:8] if rg == 3 else None), s


def mark_impulse(Y, thresh=2.0):
    Y = np.ascontiguousarray(Y, dtype=np.float32)
    h, w = Y.shape
    imp = np.zeros((h, w), np.uint8)
    cn = Counts()
    checker().sh_ref_mark_impulse(Y.ctypes.data_as(_fp), imp.ctypes.data_as(_bp), w, h, C.c_float(thresh), C.byref(cn))
    return imp, cn.as_dict()


def blend_mask(Y, contrast_threshold, blur_radius=2.0):
    Y = np.ascontiguousarray(Y, dtype=np.float32)
    h, w = Y.shape
    bl = np.zeros((h, w), np.float32)
    checker().sh_ref_blend_mask(Y.ctypes.data_as(_fp), bl.ctypes.data_as(_fp), w, h, C.c_float(contrast_threshold), C.c_float(blur_radius))
    return bl


def deconv(lum, blend, impulse, sigma, amount):
    """deconvsharpening on a copy -> (luminance, Info with sigma / regime / early_out / the two counts, counts dict)"""
    out = np.array(lum, dtype=np.float32, order="C")
    h, w = out.shape
    bl = np.ascontiguousarray(blend, dtype=np.float32)
    imp = np.ascontiguousarray(impulse, dtype=np.uint8)
    cn, rg, frozen = Counts(), C.c_int(-1), C.c_longlong(0)
    early = checker().sh_ref_deconv(out.ctypes.data_as(_fp), bl.ctypes.data_as(_fp), imp.ctypes.data_as(_bp), w, h, C.c_double(sigma), C.c_float(amount),
                                    C.byref(rg), C.byref(cn), C.byref(frozen))
    info = Info()
    info.sigma = sigma; info.regime = rg.value; info.early_out = early
    info.impulse_pixels = int(np.count_nonzero(imp)); info.frozen_pixels = frozen.value
    return out, info, cn.as_dict()


def params(enabled=True, method=RLD, amount=200, contrast=20.0, deconvradius=0.75, deconvamount=100, corner_boost=0.0, corner_latitude=25,
           offset_x=0, offset_y=0, full_width=0, full_height=0):
    return Params(1 if enabled else 0, int(method), int(amount), int(deconvamount), float(contrast), float(deconvradius), float(corner_boost),
                  int(corner_latitude), int(offset_x), int(offset_y), int(full_width), int(full_height), 0)


def sharpening(img, scale=1.0, ws=None, **kw):
    """doSharpening on copies of three H x W planes -> (planes, Info, counts dict), or None where the library returns ARTGPU_EUNSUPPORTED"""
    ws = oracle_lib.REC2020_WS_D if ws is None else ws
    out = [np.array(a, dtype=np.float32, order="C") for a in img]
    h, w = out[0].shape
    wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
    p = params(**kw)
    info, cn = Info(), Counts()
    rc = checker().sh_ref_sharpening(*[a.ctypes.data_as(_fp) for a in out], w, h, C.byref(p), wsd, C.c_double(float(scale)), C.byref(info), C.byref(cn))
    if rc:
        return None
    return out, info, cn.as_dict()


def fc_of(filters):
    if not filters:
        return 0, 0
    fc = lambda row, col: (filters >> ((((row << 1) & 14) + (col & 1)) << 1)) & 3
    return fc(0, 0), fc(1, 0)


def radius(raw, filters, lower=1000.0, upper=65535.0, serial=False):
    """calcRadiusBayer -> (radius, max_ratio, counts dict); serial: the reference's loop as written, else the pure maximum"""
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    h, w = raw.shape
    fc0, fc1 = fc_of(filters)
    r, cn = C.c_float(0), Counts()
    m = checker().sh_ref_radius(raw.ctypes.data_as(_fp), w, h, C.c_float(lower), C.c_float(upper), fc0, fc1, 1 if serial else 0, C.byref(r), C.byref(cn))
    return np.float32(r.value), np.float32(m), cn.as_dict()


def pow_F(a, b):
    return np.float32(checker().sh_ref_pow_F(float(a), float(b)))


# ---- scenes

def edge_scene(w, h, seed=1, zero_block=False, bright_block=False):
    """Blurred edges at several scales and orientations (values 300 .. 30000, flat areas in between so that the contrast mask reaches both
    ends), with speckles: single hot and dark pixels in every column range of markImpulse, and strong ones that make the estimate leave
    l +- 0.2 l early.  zero_block: a block of exact zeros; bright_block: a block at 66000 .. 90000 (above 65535)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for c in range(3):
        v = 6000.0 + 2500.0 * c + 0.0 * xx
        v += 9000.0 / (1.0 + np.exp(-(xx - 0.3 * w - 0.2 * yy) / 1.3))                     # a slanted soft edge
        v += 7000.0 / (1.0 + np.exp(-(yy - 0.6 * h) / 0.8))                                # a horizontal one, sharper
        v += 3000.0 * (np.sin(2 * np.pi * xx / 9.0) * np.sin(2 * np.pi * yy / 7.0) > 0.6) * (xx > 0.6 * w)    # small squares on the right
        v += rng.normal(0.0, 15.0, v.shape)
        v = np.clip(v, 300.0, 30000.0)
        planes.append(v)
    spk = np.random.default_rng(seed + 100)
    cols = [0, 1, 2, 3, max(w // 2, 4), w - 6, w - 5, w - 4, w - 3, w - 2, w - 1]
    for k, x in enumerate(cols * 2):
        y = int(spk.integers(0, h))
        f = (8.0, 0.05, 2.5, 0.3)[k % 4]
        for c in range(3):
            planes[c][y, x] *= f
    for _ in range(max(4, w * h // 400)):
        y, x = int(spk.integers(0, h)), int(spk.integers(0, w))
        f = float(spk.choice([5.0, 0.1, 1.6, 0.55]))
        for c in range(3):
            planes[c][y, x] *= f
    out = []
    for c in range(3):
        v = planes[c]
        if bright_block:
            by, bx = slice(h // 8, h // 8 + max(h // 5, 3)), slice(w // 2, w // 2 + max(w // 6, 3))
            v[by, bx] = 66000.0 + 8000.0 * c + spk.uniform(0.0, 8000.0, v[by, bx].shape)
        if zero_block:
            zy, zx = slice(h // 2, h // 2 + max(h // 6, 3)), slice(w // 10, w // 10 + max(w // 6, 3))
            v[zy, zx] = 0.0
        out.append(v.astype(np.float32))
    return out


def luminance(img, ws=None):
    ws = oracle_lib.REC2020_WS_D if ws is None else ws
    w1 = np.asarray(ws, np.float64).reshape(9)[3:6].astype(np.float32)
    return ((img[0] * w1[0]) + img[1] * w1[1]) + img[2] * w1[2]


def rl_inputs(w, h, seed=1):
    """(luminance, blend, impulse) of an edge scene as doSharpening hands them to deconvsharpening (contrast 20, scale 1)"""
    key = ("rl", w, h, seed)
    if key not in _CASE_CACHE:
        Y = luminance(edge_scene(w, h, seed=seed)).astype(np.float32)
        bl = blend_mask(Y, pow_F(np.float32(20.0 / 100.0), 1.2), 2.0)
        imp, _ = mark_impulse(Y)
        for a in (Y, bl, imp):
            a.setflags(write=False)
        _CASE_CACHE[key] = (Y, bl, imp)
    return _CASE_CACHE[key]


RL_SIGMAS = (0.22, 0.45, 0.75, 0.84, 1.0, 1.15, 1.6)
RL_AMOUNTS = (1.0, 0.35)
RL_SIZES = ((8, 8), (23, 9), (67, 41), (131, 67))

# The cases of artgpu_sharpening's GPU comparison (tests/test_gpu_sharpen.py); tests/test_sharpen_checker.py shows from the checker's counters
# that they take every branch.  name: (w, h, seed, scale, zero block, bright block, keyword arguments of params())
CASES = {
    "300x200-arp-default": (300, 200, 1, 1.0, False, False, dict()),                                       # Sharpening.arp: rld, contrast 20, amount 100, radius 0.75
    "131x67-scale2-radius1.5": (131, 67, 2, 2.0, False, False, dict(deconvradius=1.5)),                     # sigma 0.75 after / scale; mask blur 2 / sqrt(2)
    "257x514-corner-boost-crop": (257, 514, 3, 1.0, False, False, dict(corner_boost=0.5, corner_latitude=25, offset_x=900, offset_y=40,
                                                                        full_width=1600, full_height=1200)),   # 0.75 (5x5) and 1.25 (recursive)
    "67x41-contrast0": (67, 41, 4, 1.0, False, False, dict(contrast=0.0)),                                  # mask all ones
    "300x200-zeros-and-bright": (300, 200, 5, 1.0, True, True, dict(deconvradius=1.0)),                     # 7x7; Y == 0 and Y > 65535
    "23x9-radius0.45": (23, 9, 6, 1.0, False, False, dict(deconvradius=0.45, deconvamount=60)),             # 3x3
    "8x8-radius1.6": (8, 8, 7, 1.0, False, False, dict(deconvradius=1.6)),                                  # the stage's minimum, recursive gaussian
}
_CASE_CACHE = {}


def case(name):
    """(input planes, scale, keyword arguments, the checker's planes, Info and counts), computed once and read-only"""
    if name not in _CASE_CACHE:
        w, h, seed, scale, zero, bright, kw = CASES[name]
        img = edge_scene(w, h, seed=seed, zero_block=zero, bright_block=bright)
        want, info, counts = sharpening(img, scale=scale, **kw)
        for a in img + want:
            a.setflags(write=False)
        _CASE_CACHE[name] = (img, scale, kw, want, info, counts)
    return _CASE_CACHE[name]


def mosaic(w, h, seed, filters, clipped=True, clip_val=60000.0):
    """A CFA plane whose green sites carry diagonal pairs with ratios up to about 3 (values 1200 .. 40000), some below the lower limit, some
    zeros, and patches at the clip value so that both clipped-neighbourhood rules reject pairs."""
    rng = np.random.default_rng(seed)
    raw = rng.uniform(1200.0, 14000.0, (h, w)).astype(np.float32)
    raw *= (1.0 + 1.8 * (rng.uniform(0.0, 1.0, (h, w)) > 0.93)).astype(np.float32)
    raw[rng.uniform(0.0, 1.0, (h, w)) > 0.97] = np.float32(400.0)
    raw[rng.uniform(0.0, 1.0, (h, w)) > 0.99] = np.float32(0.0)
    if clipped:
        for k in range(6):
            y, x = int(rng.integers(4, h - 8)), int(rng.integers(4, w - 8))
            raw[y:y + 3, x:x + 3] = np.float32(clip_val)
            raw[y + 1, x + 1] = np.float32(300.0 + 50.0 * k)          # a dark site in a clipped neighbourhood
        # pairs with a ratio of 500 that only the clipped rules reject: a bright green site above a dark neighbour with a clipped value
        # beside it (rule a), a dark green site above a bright neighbour whose own neighbourhood is clipped (rule b)
        fc = fc_of(filters)
        for k in range(4):
            y, x = int(rng.integers(8, h - 10)), int(rng.integers(10, w - 12))
            x += (x ^ (5 + (fc[y & 1] & 1))) & 1                      # a column the loop visits in this row
            hi, lo = (50000.0, 100.0) if k % 2 == 0 else (100.0, 50000.0)
            raw[y - 2:y + 4, x - 3:x + 4] = np.float32(5000.0)
            raw[y, x], raw[y + 1, x - 1] = np.float32(hi), np.float32(lo)
            if k % 2 == 0:
                raw[y - 1, x - 1] = np.float32(clip_val)
            else:
                raw[y, x - 2] = np.float32(clip_val)
    return raw


# the auto-radius inputs of the GPU test: (w, h, filters, seed).  The seeds were picked so that the reference's serial loop and the pure
# maximum give the same bits (tests/test_sharpen_checker.py asserts it): that is a condition on the inputs, not a measurement.
RADIUS_CASES = [(64, 48, FILTERS_RGGB, 11), (64, 48, FILTERS_GBRG, 12), (64, 48, 0, 13),
                (301, 203, FILTERS_RGGB, 21), (301, 203, FILTERS_GBRG, 22), (301, 203, 0, 23)]
RADIUS_CLIP = 60000.0
