"""Colour correction: the CPU checker (tests/emul/colorcorrection_ref.cc: the host derivation and the row loop of
ImProcFunctions::colorCorrection restated serially around the oracle's sleef forms, PQ tables and YUV switch), the scenes, masks and cases the
tests use.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib
import tb_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
SRC = os.path.join(HERE, "emul", "colorcorrection_ref.cc")
SO = os.path.join(HERE, "emul", "libcolorcorrection_ref.so")
_fp = C.POINTER(C.c_float)
_LIB = None

YUV, RGB, HSL, JZAZBZ, LUT = 0, 1, 2, 3, 4
COUNTERS = ("groups_zero_lane", "tail_skipped", "px_yuv", "px_jzazbz", "px_rgb", "px_rgbluminance", "px_hsl", "hue_hsl", "hue_yuv", "hue_jzazbz",
            "pivot", "compression_vector_clamp", "compression_scalar_zero", "compression_taken", "gamma", "rgbluminance", "y_nonpositive",
            "v_nonpositive", "pq_low", "pq_high")
SCALARS = (("a", 0.0), ("b", 0.0), ("in_saturation", 0.0), ("out_saturation", 0.0), ("hueshift", 0.0), ("hsl_gamma", 2.4))
TRIPLES = (("slope", 1.0), ("offset", 0.0), ("power", 1.0), ("pivot", 1.0), ("compression", 0.0), ("hue", 0.0), ("sat", 0.0), ("factor", 0.0))


class Region(C.Structure):
    """cc_ref_region, the layout of artgpu_color_correction_region with float pointers for the masks"""
    _fields_ = ([("mode", C.c_int32), ("rgbluminance", C.c_int32)] + [(n, C.c_double) for n, _ in SCALARS] + [(n, C.c_double * 3) for n, _ in TRIPLES] +
                [("lmask", _fp), ("abmask", _fp)])


class Info(C.Structure):
    """cc_ref_info, the layout of artgpu_color_correction_info"""
    _fields_ = [("abca", C.c_float), ("abcb", C.c_float), ("enabled", C.c_int32), ("rgbmode", C.c_int32), ("slope", C.c_float * 3),
                ("offset", C.c_float * 3), ("power", C.c_float * 3), ("pivot", C.c_float * 3), ("compression", C.c_float * 6), ("rhs", C.c_float),
                ("oor_pixels", C.c_int64)]


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
    return ((f(i.abca), f(i.abcb), int(i.enabled), int(i.rgbmode)) + tuple(f(v) for name in ("slope", "offset", "power", "pivot", "compression")
                                                                           for v in getattr(i, name)) + (f(i.rhs), int(i.oor_pixels)))


def triple(v):
    return [float(v)] * 3 if np.isscalar(v) else [float(x) for x in v]


def color_correction(img, regions, to_rgb=False, ws=None, iws=None):
    """ImProcFunctions::colorCorrection on copies of three H x W planes in RGB mode.  regions: [dict, ...] with Region's field names (what is
    left out takes ColorCorrectionParams::Region's default) and `lmask` / `abmask` arrays or None.  Returns (planes, [Info], oor map, counts
    dict), or None where the device path is unsupported."""
    ws = oracle_lib.REC2020_WS_D if ws is None else ws
    iws = oracle_lib.REC2020_IWS_D if iws is None else iws
    out = [np.array(a, dtype=np.float32, order="C") for a in img]
    h, w = out[0].shape
    n = len(regions)
    arr = (Region * max(n, 1))()
    keep = []
    for k, r in enumerate(regions):
        r = dict(r)
        arr[k].mode = int(r.pop("mode", JZAZBZ))
        arr[k].rgbluminance = 1 if r.pop("rgbluminance", False) else 0
        for name, dflt in SCALARS:
            setattr(arr[k], name, float(r.pop(name, dflt)))
        for name, dflt in TRIPLES:
            setattr(arr[k], name, (C.c_double * 3)(*triple(r.pop(name, dflt))))
        for name in ("lmask", "abmask"):
            m = r.pop(name, None)
            if m is not None:
                mm = np.ascontiguousarray(m, dtype=np.float32)
                assert mm.shape == (h, w)
                keep.append(mm)
                setattr(arr[k], name, mm.ctypes.data_as(_fp))
        assert not r, sorted(r)
    wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
    iwsd = (C.c_double * 9)(*np.asarray(iws, np.float64).ravel())
    info = (Info * max(n, 1))()
    oor = np.zeros((h, w), np.uint8)
    cn = Counts()
    rc = checker().cc_ref_tool(*[a.ctypes.data_as(_fp) for a in out], w, h, arr, n, wsd, iwsd, 1 if to_rgb else 0, info,
                               oor.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(cn))
    if rc:
        return None
    return out, list(info)[:n], oor.astype(bool), cn.as_dict()


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes and masks
# ---------------------------------------------------------------------------------------------------------------------------------------
NAN_BODY = (22, 21)       # 67 x 45 and 256 x 131: a column of the 4-wide body (x % 4 == 1)
NAN_TAIL_ROW = 41         # ... and the last column of a width with w % 4 == 3, on an odd row


def scene(w, h, seed=1, superwhite=False, nans=True):
    """tb_lib.rgb_scene plus a hue wheel; a negative block, an exact-zero pixel, a -0.f pixel (all three channels) and, with `nans`, one NaN
    in a body column and one in a tail column (planes 0 and 1).  superwhite: a block above 65535 (Jzazbz's per-pixel powf).  Planes smaller
    than rgb_scene supports are drawn directly with the same special pixels."""
    rng = np.random.default_rng(seed)
    if w >= 40 and h >= 20:
        img = tb_lib.rgb_scene(w, h, seed=seed, low=True)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        wy, wx = slice(2, 2 + h // 3), slice(w // 2, w // 2 + w // 3)              # the hue wheel: every hue at two saturations
        ang = 2 * np.pi * (xx[wy, wx] - w // 2) / max(w // 3 - 1, 1)
        sat = 0.35 + 0.6 * ((yy[wy, wx] - 2) / max(h // 3 - 1, 1))
        for c, ph in enumerate((0.0, 2 * np.pi / 3, 4 * np.pi / 3)):
            img[c][wy, wx] = (7000.0 * (1.0 + sat * np.cos(ang - ph))).astype(np.float32)      # (dim: the brightening cases keep it below 1)
        ny, nx = slice(h - 9, h - 4), slice(4, 13)                                 # a negative block
        for c in range(3):
            img[c][ny, nx] = -rng.uniform(50.0, 900.0, img[c][ny, nx].shape).astype(np.float32)
            img[c][h - 3, 5] = 0.0
            img[c][h - 3, 10] = -0.0
            img[c][h - 3, w - 1] = -0.0
        if superwhite:
            sy, sx = slice(h // 2, h // 2 + 6), slice(w - 14, w)
            for c in range(3):
                img[c][sy, sx] = (90000.0 + rng.uniform(0.0, 250000.0, img[c][sy, sx].shape)).astype(np.float32)
        if nans:
            assert w % 4 == 3 or w % 4 == 0
            img[0][NAN_BODY] = np.nan
            if w % 4:
                img[1][NAN_TAIL_ROW, w - 1] = np.nan
    else:
        img = [rng.uniform(800.0, 12000.0, (h, w)).astype(np.float32) for _ in range(3)]
        for c in range(3):
            img[c][0, 0] = -0.0
            img[c][h - 1, w - 1] = 0.0
            img[c][1, 1] = -120.0 - 40.0 * c
        if nans:
            img[0][h - 1, 0] = np.nan
    return img


def mask(kind, w, h):
    """blend planes: `smooth` (tb_lib.smooth_mask: exact zeros top left, exact ones bottom right), `flip` (its mirror: zeros in the tail
    columns of the upper rows), `onelane` (in every group of four columns exactly one non-zero lane, lane y % 4; a tail column is non-zero
    where x + y is even), `zero`, None"""
    if kind is None:
        return None
    if kind == "smooth":
        return tb_lib.smooth_mask(w, h)
    if kind == "flip":
        return np.ascontiguousarray(tb_lib.smooth_mask(w, h)[:, ::-1])
    if kind == "zero":
        return np.zeros((h, w), np.float32)
    assert kind == "onelane"
    yy, xx = np.mgrid[0:h, 0:w]
    wvec = (w // 4) * 4
    m = np.where(xx < wvec, (xx % 4) == (yy % 4), ((xx + yy) % 2) == 0)
    return (m * np.float32(0.7)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
SOP = dict(slope=(1.15, 0.9, 1.05), offset=(0.04, -0.3, 0.03), power=(1.2, 0.85, 1.1))
HSLP = dict(hue=(30.0, 200.0, 310.0), sat=(40.0, 25.0, 60.0), factor=(10.0, -15.0, 20.0))
VARIANTS = {
    "defaults": {},
    "sop": SOP,
    "pivot": dict(SOP, pivot=(0.8, 1.2, 0.6)),
    "compression": dict(SOP, slope=(0.8, 0.7, 0.85), offset=(0.0, -0.3, 0.03), compression=(0.4, 0.2, 0.7)),
    # (slopes below 1: the curve ends at `slope`; no offset on channel 0: with one, YY / Y of the near-black block's pixels reaches 1e5 in
    # the YUV and JZAZBZ modes, their chroma leaves [0, 1] and the scene would have powf pixels without a super-white block)
    "ab": dict(a=0.35, b=-0.2),
    "sat": dict(in_saturation=25.0, out_saturation=-30.0),
    "hue+30": dict(SOP, hueshift=30.0),
    "hue-30": dict(hueshift=-30.0, a=-0.1, b=0.25),
}
HSL_VARIANTS = {
    "defaults": {},
    "g2.4": HSLP,
    "g1": dict(HSLP, hsl_gamma=1.0),
    "sat": dict(HSLP, in_saturation=25.0, out_saturation=-30.0),
    "hue+30": dict(HSLP, hueshift=30.0),
    "hue-30": dict(hueshift=-30.0),
}
MODES = {"yuv": dict(mode=YUV), "jzazbz": dict(mode=JZAZBZ), "rgb": dict(mode=RGB), "rgblum": dict(mode=RGB, rgbluminance=True), "hsl": dict(mode=HSL)}

# name: (w, h, seed, [(region fields, lmask kind, abmask kind), ...], to_rgb, superwhite)
CASES = {}
for _m, _mode in MODES.items():
    for _v, _par in (HSL_VARIANTS if _m == "hsl" else VARIANTS).items():
        if _m in ("rgb", "rgblum") and _v.startswith("hue"):
            continue                                                                # (rhs is zero in RGB mode)
        CASES["67x45-%s-%s" % (_m, _v)] = (67, 45, 3, [(dict(_mode, **_par), "smooth", "smooth")], False, False)
_FIVE = [(dict(mode=JZAZBZ, **VARIANTS["compression"]), "smooth", "smooth"), (dict(mode=HSL, **HSL_VARIANTS["hue+30"]), None, None),
         (dict(mode=RGB, rgbluminance=True, **VARIANTS["pivot"]), "onelane", "onelane"), (dict(mode=YUV, **VARIANTS["hue-30"]), "flip", None),
         (dict(mode=JZAZBZ, hueshift=30.0, a=0.2, b=0.1), None, "smooth")]
for _n in range(1, 6):                                                              # four regions fill a launch; Jzazbz next to an HSL hue shift cuts it earlier
    CASES["67x45-%d-regions" % _n] = (67, 45, 4, _FIVE[:_n], _n % 2 == 0, False)
CASES.update({
    "67x45-no-regions-yuv": (67, 45, 5, [], False, False),
    "67x45-no-regions-rgb": (67, 45, 5, [], True, False),
    "67x45-null-masks": (67, 45, 6, [(dict(mode=JZAZBZ, **SOP), None, None), (dict(mode=RGB, **VARIANTS["compression"]), None, None)], True, False),
    "67x45-onelane": (67, 45, 7, [(dict(mode=RGB, **VARIANTS["compression"]), "onelane", "onelane"), (dict(mode=JZAZBZ, **VARIANTS["ab"]), "onelane", "onelane"),
                                  (dict(mode=YUV, **VARIANTS["compression"]), "onelane", "onelane")], False, False),
    "67x45-l-ab-differ": (67, 45, 8, [(dict(mode=YUV, **VARIANTS["sop"]), "smooth", "flip"), (dict(mode=HSL, **HSLP), "flip", "zero")], True, False),
    "67x45-superwhite": (67, 45, 9, [(dict(mode=JZAZBZ, **SOP), "smooth", "smooth"), (dict(mode=JZAZBZ, **VARIANTS["hue+30"]), None, None)], True, True),
    "4x3-one-group": (4, 3, 10, [(dict(mode=JZAZBZ, **SOP), None, None), (dict(mode=RGB, **VARIANTS["pivot"]), "onelane", "onelane")], False, False),
    "3x5-tail-only": (3, 5, 11, [(dict(mode=JZAZBZ, **VARIANTS["compression"]), None, None), (dict(mode=HSL, **HSL_VARIANTS["hue-30"]), "onelane", "onelane")], True, False),
    "256x131-mixed": (256, 131, 12, _FIVE[:3], True, False),
})
STRIDED_CASES = ("67x45-3-regions", "256x131-mixed")
DEVICE_MASK_CASES = ("67x45-5-regions", "67x45-l-ab-differ")
_CACHE = {}


def case(name):
    """(input planes, region dicts with mask arrays, to_rgb, the checker's planes, [Info], oor map, counts), computed once and read-only"""
    if name not in _CACHE:
        w, h, seed, regs, to_rgb, superwhite = CASES[name]
        img = scene(w, h, seed=seed, superwhite=superwhite)
        masks = {k: mask(k, w, h) for k in (None, "smooth", "flip", "onelane", "zero")}
        regions = [dict(r, lmask=masks[lk], abmask=masks[ak]) for r, lk, ak in regs]
        want, info, oor, counts = color_correction(img, regions, to_rgb=to_rgb)
        for a in img + want + [oor] + [m for m in masks.values() if m is not None]:
            a.setflags(write=False)
        _CACHE[name] = (img, regions, to_rgb, want, info, oor, counts)
    return _CACHE[name]


def bits(a):
    """float32 bit patterns with every NaN mapped to one pattern: which NaN an operation returns (sign, payload) is the one thing the two
    machines' arithmetic does not share"""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


def assert_same(got, want, oor, what=""):
    """equality of bit patterns outside `oor`; rtol 2e-4 / atol 0.5 inside it (the per-pixel powf, the bound of test_gpu_tonecurve.py)"""
    for name, gp, wp in zip("rgb", got, want):
        bad = (bits(gp) != bits(wp)) & ~oor
        assert not bad.any(), "%s plane %s: %d values differ outside the powf pixels, first at %s: %r != %r" % (
            what, name, int(bad.sum()), tuple(np.argwhere(bad)[0]), gp[tuple(np.argwhere(bad)[0])], wp[tuple(np.argwhere(bad)[0])])
        if oor.any():
            assert np.allclose(gp[oor], wp[oor], rtol=2e-4, atol=0.5, equal_nan=True), "%s plane %s: powf pixels" % (what, name)
