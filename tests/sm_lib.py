"""Smoothing: the CPU checker (tests/emul/smoothing_ref.cc: the region loop of ImProcFunctions::guidedSmoothing, find_region, guided_smoothing
and nlmeans_smoothing restated serially around the oracle's guided filter, NL-means, log forms and double-matrix YUV forms), the scenes, masks
and cases the tests use.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
SRC = os.path.join(HERE, "emul", "smoothing_ref.cc")
SO = os.path.join(HERE, "emul", "libsmoothing_ref.so")
_fp = C.POINTER(C.c_float)
_LIB = None

GUIDED, GAUSSIAN, GAUSSIAN_GLOW, NLMEANS, MOTION, LENS, NOISE, HALATION, WAVELETS = range(9)
L, CH, LC = 0, 1, 2
SKIP_RADIUS, SKIP_STRENGTH, SKIP_EMPTY = 1, 2, 3
COUNTERS = ("cropped", "full_frame", "skipped_radius", "skipped_strength", "skipped_empty", "bump_one", "chan_clamped", "q_clamped", "mask_between",
            "mask_zero_in_box")
# SmoothingParams::Region's fields in artgpu_smoothing_region's order, with the defaults of procparams.cc:2753-2775
FIELDS = (("mode", C.c_int32, GUIDED), ("channel", C.c_int32, LC), ("radius", C.c_int32, 0), ("epsilon", C.c_int32, 0), ("sigma", C.c_double, 0.0),
          ("iterations", C.c_int32, 1), ("nldetail", C.c_int32, 50), ("falloff", C.c_double, 1.0), ("nlstrength", C.c_int32, 0), ("numblades", C.c_int32, 9),
          ("angle", C.c_double, 0.0), ("curvature", C.c_double, 0.0), ("offset", C.c_double, 0.0), ("noise_strength", C.c_int32, 10),
          ("noise_coarseness", C.c_int32, 30), ("halation_size", C.c_double, 1.0), ("halation_color", C.c_double, 0.0), ("wav_strength", C.c_double, 0.0),
          ("wav_levels", C.c_int32, 5), ("pad_", C.c_int32, 0), ("wav_gamma", C.c_double, 2.2))
INFO_FIELDS = ("r", "epsilon", "min_x", "min_y", "max_x", "max_y", "cropped", "work_w", "work_h", "subsampling", "box_radius", "skipped")


class Region(C.Structure):
    """sm_ref_region, the layout of artgpu_smoothing_region with a float pointer for the mask"""
    _fields_ = [(n, t) for n, t, _ in FIELDS] + [("mask", _fp)]


class Info(C.Structure):
    """sm_ref_info, the layout of artgpu_smoothing_info"""
    _fields_ = [(n, C.c_float if n == "epsilon" else C.c_int32) for n in INFO_FIELDS]


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
    """the fields of an Info-shaped structure as a tuple of ints, epsilon as its float32 bit pattern"""
    return tuple(int(np.float32(i.epsilon).view(np.uint32)) if n == "epsilon" else int(getattr(i, n)) for n in INFO_FIELDS)


def smoothing(img, regions, scale=1.0, ws=None):
    """ImProcFunctions::guidedSmoothing on copies of three H x W planes in RGB mode.  regions: [dict, ...] with Region's field names (what is
    left out takes SmoothingParams::Region's default) and a `mask` array or None.  Returns (planes, [Info], counts dict), or None where the
    device path is unsupported (the checker then leaves its planes alone)."""
    ws = oracle_lib.REC2020_WS_D if ws is None else ws
    out = [np.array(a, dtype=np.float32, order="C") for a in img]
    h, w = out[0].shape
    n = len(regions)
    arr = (Region * max(n, 1))()
    keep = []
    for k, r in enumerate(regions):
        r = dict(r)
        for name, typ, dflt in FIELDS:
            v = r.pop(name, dflt)
            setattr(arr[k], name, float(v) if typ is C.c_double else int(v))
        m = r.pop("mask", None)
        if m is not None:
            mm = np.ascontiguousarray(m, dtype=np.float32)
            assert mm.shape == (h, w)
            keep.append(mm)
            arr[k].mask = mm.ctypes.data_as(_fp)
        assert not r, sorted(r)
    wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
    info = (Info * max(n, 1))()
    cn = Counts()
    before = [a.copy() for a in out]
    rc = checker().sm_ref_tool(*[a.ctypes.data_as(_fp) for a in out], w, h, arr, n, wsd, C.c_double(scale), info, C.byref(cn))
    if rc:
        assert rc == 1 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(out, before))
        return None
    return out, list(info)[:n], cn.as_dict()


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes and masks
# ---------------------------------------------------------------------------------------------------------------------------------------
def scene(w, h, seed=1):
    """three NaN-free planes, 0..65535 and beyond: a smooth ramp with noise; a block of independent, log-uniform channels (colour contrast far
    above the luminance contrast: guided coefficients above 1); a block of exact zeros and a block dark enough for oY <= 1e-5f after the
    filter; a negative block; a block above 65535.  The blocks scale with the plane."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 1500.0 + 30000.0 * (xx / max(w - 1, 1)) * (0.3 + 0.7 * yy / max(h - 1, 1))
    img = [(base * f + rng.normal(0.0, 900.0, (h, w))).astype(np.float32) for f in (1.0, 0.8, 0.55)]
    bw, bh = max(w // 6, 6), max(h // 4, 6)

    def block(ix, iy):
        x0, y0 = min(ix * (bw + 2) + 2, w - bw), min(iy * (bh + 2) + 1, h - bh)
        return slice(y0, y0 + bh), slice(x0, x0 + bw)

    sy, sx = block(0, 0)
    for c in range(3):
        img[c][sy, sx] = np.exp(rng.uniform(np.log(5.0), np.log(60000.0), img[c][sy, sx].shape)).astype(np.float32)
    sy, sx = block(1, 0)
    for c in range(3):
        img[c][sy, sx] = 0.0
    sy, sx = block(2, 0)
    for c in range(3):
        img[c][sy, sx] = rng.uniform(0.005, 0.3, img[c][sy, sx].shape).astype(np.float32)
    sy, sx = block(0, 1)
    for c in range(3):
        img[c][sy, sx] = -rng.uniform(50.0, 900.0, img[c][sy, sx].shape).astype(np.float32)
    sy, sx = block(1, 1)
    for c in range(3):
        img[c][sy, sx] = (70000.0 + rng.uniform(0.0, 150000.0, img[c][sy, sx].shape)).astype(np.float32)
    return img


BOX = (31, 22, 50, 40)            # x0, y0, w, h on the 130 x 97 plane: touches no border
CORNER_BOX = (0, 0, 46, 39)       # touches the top-left corner


def mask(kind, w, h):
    """blend planes: `between` (strictly between 0 and 1 everywhere: its box is the frame); `box` / `corner` (positive only inside BOX /
    CORNER_BOX, a ramp that reaches 1, with exact zeros inside the box); `box2` (a box that overlaps BOX); `corners2` (only two opposite corner
    pixels are positive: the box is the frame); `empty`; `narrow` (a 31 x 40 box); `tiny` (a 4 x 4 box); None"""
    if kind is None:
        return None
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    if kind == "between":
        return (np.float32(0.05) + np.float32(0.9) * (xx / np.float32(max(w - 1, 1))) * (yy / np.float32(max(h - 1, 1)))).astype(np.float32)
    m = np.zeros((h, w), np.float32)
    if kind == "empty":
        return m
    if kind == "corners2":
        m[0, 0] = 0.6
        m[h - 1, w - 1] = 1.0
        return m
    x0, y0, bw, bh = {"box": BOX, "corner": CORNER_BOX, "box2": (60, 40, 45, 36), "narrow": (40, 30, 31, 40), "tiny": (50, 50, 4, 4)}[kind]
    assert x0 + bw <= w and y0 + bh <= h
    ramp = np.minimum(np.float32(1.0), np.float32(0.2) + np.float32(1.6) * (xx[y0:y0 + bh, x0:x0 + bw] - x0) / np.float32(bw))
    m[y0:y0 + bh, x0:x0 + bw] = ramp
    if bw > 8 and bh > 8:
        m[y0 + 3:y0 + 6, x0 + 4:x0 + 9] = 0.0           # exact zeros inside the box
    return m


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases: name -> (w, h, seed, scale, [(region fields, mask kind), ...])
# ---------------------------------------------------------------------------------------------------------------------------------------
CHANNELS = {"L": L, "C": CH, "LC": LC}
CASES = {}
for _c, _ch in CHANNELS.items():
    for _r in (1, 3):
        for _e in (-10, 0, 10):                                     # 10 reaches the 1e-6 floor
            CASES["67x41-guided-%s-r%d-e%d" % (_c, _r, _e)] = (67, 41, 3, 1.0, [(dict(mode=GUIDED, channel=_ch, radius=_r, epsilon=_e), "between")])
        CASES["67x41-guided-%s-r%d-it3" % (_c, _r)] = (67, 41, 4, 1.0, [(dict(mode=GUIDED, channel=_ch, radius=_r, epsilon=2, iterations=3), "between")])
    # the longer side above 600: radius 4 -> subsampling 4 on a 175 x 8 grid, radius 5 -> subsampling 5 on 140 x 6; radius 12 -> subsampling 4,
    # box radius 3 clamped to 2 by f_mean; scale 2: radius 20 -> r 10, subsampling 5, box radius 2 clamped to 1
    for _r, _s in ((4, 1.0), (5, 1.0), (12, 1.0), (20, 2.0)):
        CASES["701x33-guided-%s-r%d-s%g" % (_c, _r, _s)] = (701, 33, 5, _s, [(dict(mode=GUIDED, channel=_ch, radius=_r, epsilon=1), None)])
    for _k in ("box", "corner"):
        CASES["130x97-%s-guided-%s" % (_k, _c)] = (130, 97, 6, 1.0, [(dict(mode=GUIDED, channel=_ch, radius=3, epsilon=1, iterations=2), _k)])
        CASES["130x97-%s-nlmeans-%s" % (_k, _c)] = (130, 97, 7, 1.0, [(dict(mode=NLMEANS, channel=_ch, nlstrength=60, nldetail=40, iterations=2), _k)])
CASES.update({
    "130x97-corners2-guided": (130, 97, 8, 1.0, [(dict(mode=GUIDED, channel=CH, radius=2), "corners2")]),
    "130x97-corners2-nlmeans": (130, 97, 8, 1.0, [(dict(mode=NLMEANS, channel=L, nlstrength=40), "corners2")]),
    # the second region reads the first's output where the boxes overlap; an empty mask; radius 0; strength 0 (L: the YUV round trip remains)
    "130x97-regions": (130, 97, 9, 1.0, [(dict(mode=GUIDED, channel=CH, radius=3), "box"), (dict(mode=NLMEANS, channel=LC, nlstrength=50), "box2"),
                                          (dict(mode=GUIDED, channel=L, radius=4), "empty"), (dict(mode=GUIDED, channel=LC, radius=0), "between"),
                                          (dict(mode=NLMEANS, channel=L, nlstrength=0), "corner"), (dict(mode=NLMEANS, channel=CH, nlstrength=0), None),
                                          (dict(mode=NLMEANS, channel=LC, nlstrength=0), "box")]),
    "67x41-no-regions": (67, 41, 10, 1.0, []),
    "67x41-null-mask": (67, 41, 11, 1.0, [(dict(mode=GUIDED, channel=L, radius=2), None), (dict(mode=NLMEANS, channel=CH, nlstrength=30), None)]),
})
STRIDED_CASES = ("130x97-regions", "130x97-box-guided-C", "67x41-guided-L-r3-e0")
DEVICE_MASK_CASES = ("130x97-regions", "130x97-box-nlmeans-L", "67x41-guided-LC-r3-it3")
# what artgpu_smoothing refuses before it writes: name -> (w, h, [(fields, mask kind)])
UNSUPPORTED = {m: (67, 41, [(dict(mode=GUIDED, radius=2), None), (dict(mode=v), "between")])
               for m, v in (("gaussian", GAUSSIAN), ("gaussian_glow", GAUSSIAN_GLOW), ("motion", MOTION), ("lens", LENS), ("noise", NOISE),
                            ("halation", HALATION), ("wavelets", WAVELETS))}
UNSUPPORTED.update({
    "iterations-0": (67, 41, [(dict(mode=GUIDED, radius=2, iterations=0), None)]),
    "nlmeans-crop-31x40": (130, 97, [(dict(mode=GUIDED, radius=2), "box"), (dict(mode=NLMEANS, nlstrength=50), "narrow")]),
    "guided-grid-below-min-size": (130, 97, [(dict(mode=GUIDED, radius=1), "tiny")]),
    "box-radius-above-hblur-max": (1830, 1812, [(dict(mode=GUIDED, radius=901), None)]),
})
_CACHE = {}


def case(name):
    """(input planes, region dicts with mask arrays, scale, the checker's planes, [Info], counts), computed once and read-only"""
    if name not in _CACHE:
        w, h, seed, scale, regs = CASES[name]
        img = scene(w, h, seed=seed)
        masks = {}
        for _, k in regs:
            if k not in masks:
                masks[k] = mask(k, w, h)
        regions = [dict(r, mask=masks[k]) for r, k in regs]
        res = smoothing(img, regions, scale=scale)
        assert res is not None, name
        want, info, counts = res
        for a in img + want + [m for m in masks.values() if m is not None]:
            a.setflags(write=False)
        _CACHE[name] = (img, regions, scale, want, info, counts)
    return _CACHE[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what=""):
    """equality of float32 bit patterns"""
    for name, gp, wp in zip("rgb", got, want):
        bad = bits(gp) != bits(wp)
        assert not bad.any(), "%s plane %s: %d values differ, first at %s: %r != %r" % (
            what, name, int(bad.sum()), tuple(np.argwhere(bad)[0]), gp[tuple(np.argwhere(bad)[0])], wp[tuple(np.argwhere(bad)[0])])
