"""Region masks: the CPU checker (tests/emul/masks_ref.cc: the parametric path of rtengine::generateMasks restated serially around the
oracle's guided filter, FlatCurve, rgb2lab, xatan2f / xlin2log, rescaleBilinear and gaussian), the scenes and the cases the tests use.
Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib
from art_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
SRC = os.path.join(HERE, "emul", "masks_ref.cc")
SO = os.path.join(HERE, "emul", "libmasks_ref.so")
_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
_LIB = None

MODE_RGB, MODE_LAB, MODE_YUV, MODE_XYZ = 0, 1, 2, 3
MAX_REGIONS = 8
EUNSUPPORTED, EINVAL = -4, -1


class Mask(C.Structure):
    """mk_ref_mask: artgpu_mask_params with the area plane as a bare pointer"""
    _fields_ = [("parametric_enabled", C.c_int32), ("lightness_detail", C.c_int32), ("hue", _dp), ("chromaticity", _dp), ("lightness", _dp),
                ("nhue", C.c_int32), ("nchromaticity", C.c_int32), ("nlightness", C.c_int32), ("contrast_threshold", C.c_int32),
                ("blur", C.c_double), ("area", _fp), ("posterization", C.c_int32), ("smoothing", C.c_int32), ("inverted", C.c_int32),
                ("opacity", C.c_int32), ("deltae_enabled", C.c_int32), ("drawn_enabled", C.c_int32), ("external_enabled", C.c_int32),
                ("linked_enabled", C.c_int32), ("curve_is_identity", C.c_int32), ("show_mask", C.c_int32)]


INFO_FIELDS = ("has_mask", "has_lmask", "ll_radius_small", "ll_radius", "blurred", "r1", "r2", "cthr_w", "cthr_h", "smoothing_radius")


class Info(C.Structure):
    """mk_ref_info, the layout of artgpu_masks_info"""
    _fields_ = [(n, C.c_int32) for n in INFO_FIELDS]


class Counts(C.Structure):
    _fields_ = [("hue_segment", C.c_longlong * 10), ("hue_fix_low", C.c_longlong), ("hue_fix_high", C.c_longlong), ("hue_wraps", C.c_longlong),
                ("curve_evals", (C.c_longlong * 3) * MAX_REGIONS), ("curve_identity", C.c_longlong),
                ("guide_low", C.c_longlong), ("guide_high", C.c_longlong), ("clamp_low", C.c_longlong), ("clamp_high", C.c_longlong),
                ("blurred_regions", C.c_longlong), ("filled_planes", C.c_longlong), ("ll_built", C.c_longlong), ("ll_read", C.c_longlong),
                ("cthr_rescaled", C.c_longlong), ("cthr_plain", C.c_longlong), ("cthr_negative", C.c_longlong), ("area_pixels", C.c_longlong),
                ("poster_level", C.c_longlong * 31), ("thr_fill", C.c_longlong), ("thr_one", C.c_longlong),
                ("inverted_planes", C.c_longlong), ("opacity_planes", C.c_longlong)]

    def as_dict(self):
        out = {}
        for n, _ in self._fields_:
            v = getattr(self, n)
            if n == "curve_evals":
                out[n] = [[int(x) for x in row] for row in v]
            elif hasattr(v, "__len__"):
                out[n] = [int(x) for x in v]
            else:
                out[n] = int(v)
        return out


def checker():
    global _LIB
    if _LIB is None:
        oracle_lib.lib()            # builds liboracle.so when needed and leaves it loaded
        if not os.path.exists(SO) or os.path.getmtime(SRC) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-msse2", "-o", SO, SRC,
                                   "-L" + ORACLE_DIR, "-loracle", "-Wl,-rpath," + ORACLE_DIR])
        _LIB = C.CDLL(SO)
        _LIB.mk_ref_generate.restype = C.c_int
    return _LIB


def info_fields(i):
    return tuple(int(getattr(i, n)) for n in INFO_FIELDS)


# ParametricMask's default curves (procparams.cc:1014-1053)
DEFAULT_HUE = (1.0, 0.166666667, 1.0, 0.35, 0.35, 0.8287775246, 1.0, 0.35, 0.35)
DEFAULT_CL = (1.0, 0.0, 1.0, 0.35, 0.35, 1.0, 1.0, 0.35, 0.35)
# curves of the tests: FCT_MinMaxCPoints, then (x, y, left tangent, right tangent) per knot
HUE_A = (1.0, 0.1, 1.0, 0.35, 0.35, 0.45, 0.0, 0.35, 0.35, 0.8, 0.6, 0.2, 0.2)
HUE_B = (1.0, 0.0, 0.1, 0.35, 0.35, 0.3, 0.9, 0.0, 0.35, 0.7, 0.2, 0.35, 0.0)          # straight segments on one side of each knot
CHROMA_A = (1.0, 0.0, 0.0, 0.35, 0.35, 0.5, 1.0, 0.35, 0.35, 1.0, 0.3, 0.35, 0.35)
LIGHT_A = (1.0, 0.0, 0.2, 0.35, 0.35, 0.4, 1.0, 0.3, 0.3, 1.0, 0.0, 0.35, 0.35)
LIGHT_B = (1.0, 0.0, 1.3, 0.35, 0.35, 0.6, -0.2, 0.35, 0.35, 1.0, 1.1, 0.35, 0.35)    # leaves [0, 1]: both sides of the LIM01 behind the blur
IDENTITY = (1.0, 0.0, 0.5, 0.35, 0.35, 1.0, 0.5, 0.35, 0.35)                          # FlatCurve's constructor: FCT_Empty, getVal = 0.5
LINEAR = (0.0,)                                                                       # FCT_Linear: absent
EMPTY = ()                                                                            # absent

MASK_DEFAULTS = dict(parametric_enabled=False, hue=DEFAULT_HUE, chromaticity=DEFAULT_CL, lightness=DEFAULT_CL, lightness_detail=0,
                     contrast_threshold=0, blur=0.0, area=None, posterization=0, smoothing=0, inverted=False, opacity=100,
                     deltae_enabled=False, drawn_enabled=False, external_enabled=False, linked_enabled=False, curve_is_identity=True,
                     show_mask=False)


def mask(**kw):
    """one region: Mask's defaults with the given fields replaced (`area`: an H x W float32 array)"""
    assert set(kw) <= set(MASK_DEFAULTS), sorted(set(kw) - set(MASK_DEFAULTS))
    m = dict(MASK_DEFAULTS)
    m.update(kw)
    return m


def _mask_array(masks):
    arr = (Mask * max(len(masks), 1))()
    keep = []
    for k, m in enumerate(masks):
        a = arr[k]
        for name in ("hue", "chromaticity", "lightness"):
            buf = (C.c_double * max(len(m[name]), 1))(*[float(v) for v in m[name]])
            keep.append(buf)
            setattr(a, name, C.cast(buf, _dp))
            setattr(a, "n" + name, len(m[name]))
        if m["area"] is not None:
            ar = np.ascontiguousarray(m["area"], dtype=np.float32)
            keep.append(ar)
            a.area = ar.ctypes.data_as(_fp)
        a.blur = float(m["blur"])
        for name in ("lightness_detail", "contrast_threshold", "posterization", "smoothing", "opacity"):
            setattr(a, name, int(m[name]))
        for name in ("parametric_enabled", "inverted", "deltae_enabled", "drawn_enabled", "external_enabled", "linked_enabled",
                     "curve_is_identity", "show_mask"):
            setattr(a, name, 1 if m[name] else 0)
    return arr, keep


def generate(img, mode, masks, want_L=True, want_ab=False, full_w=-1, full_h=-1, scale=1.0, ws=None, always_ll=False):
    """generateMasks on three H x W planes -> (return code, L planes or None, ab planes or None, [Info], counts dict)"""
    ws = oracle_lib.REC2020_WS_D if ws is None else ws
    planes = [np.ascontiguousarray(a, dtype=np.float32) for a in img]
    h, w = planes[0].shape
    n = len(masks)
    arr, keep = _mask_array(masks)
    L = np.full((n, h, w), np.nan, np.float32) if want_L else None
    ab = np.full((n, h, w), np.nan, np.float32) if want_ab else None
    wsd = (C.c_double * 9)(*np.asarray(ws, np.float64).ravel())
    info, cn = (Info * max(n, 1))(), Counts()
    rc = checker().mk_ref_generate(*[a.ctypes.data_as(_fp) for a in planes], w, h, int(mode), wsd, arr, n, int(full_w), int(full_h),
                                   C.c_double(float(scale)), L.ctypes.data_as(_fp) if want_L else None,
                                   ab.ctypes.data_as(_fp) if want_ab else None, 1 if always_ll else 0, info, C.byref(cn))
    del keep
    return rc, L, ab, list(info)[:n], cn.as_dict()


def scene(w, h, seed=1, lab=False):
    """Three planes in RGB mode (or their Imagefloat LAB form): a hue wheel around the centre (every Lab hue, saturation rising with the
    radius) modulated by art_amd.synth's frame, with a block above 65535 (l > 1), a block of out-of-gamut pixels (one channel negative, the
    others large) and a block of negative pixels (l < 0)."""
    tex = synth.bayer_frame(w, h, seed=seed).astype(np.float64) / 65535.0
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ang = np.arctan2((yy - (h - 1) / 2.0) / max(h, 2), (xx - (w - 1) / 2.0) / max(w, 2))
    rad = np.hypot((yy - (h - 1) / 2.0) / (h / 2.0), (xx - (w - 1) / 2.0) / (w / 2.0))
    sat = np.clip(rad, 0.0, 1.0)
    val = 0.15 + 0.85 * tex
    rgb = []
    for k in range(3):
        c = 0.5 + 0.5 * np.cos(ang - 2.0 * np.pi * k / 3.0)
        rgb.append(val * ((1.0 - sat) + sat * c) * 52000.0)
    by, bx = slice(h // 8, h // 8 + max(h // 6, 3)), slice(w // 10, w // 10 + max(w // 8, 5))
    for c in rgb:
        c[by, bx] = c[by, bx] * 2.5 + 40000.0                               # l > 1
    oy, ox = slice(h // 2, h // 2 + max(h // 6, 3)), slice(w // 2 + w // 8, w // 2 + w // 8 + max(w // 8, 5))
    rgb[0][oy, ox] = -9000.0 - 3000.0 * tex[oy, ox]                          # out of gamut
    rgb[1][oy, ox] = 60000.0
    rgb[2][oy, ox] = 90000.0 * tex[oy, ox]
    ny, nx = slice(h - max(h // 5, 4), h - 1), slice(w // 5, w // 5 + max(w // 8, 5))
    for k, c in enumerate(rgb):
        c[ny, nx] = -400.0 * (k + 1) - 2000.0 * tex[ny, nx]                  # l < 0
    img = [c.astype(np.float32) for c in rgb]
    if lab:
        img = oracle_lib.image_rgb_to_lab(img, oracle_lib.REC2020_WS_D)
    return [np.ascontiguousarray(a, dtype=np.float32) for a in img]


def area_plane(w, h):
    """what generate_area_mask hands over: a feathered ellipse with exact zeros outside and exact ones inside"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.hypot((yy - 0.45 * h) / (0.4 * h), (xx - 0.55 * w) / (0.45 * w))
    return np.clip(2.0 - 2.0 * d, 0.0, 1.0).astype(np.float32)


# The cases of the GPU comparison (tests/test_gpu_masks.py); tests/test_masks_checker.py shows from the checker's counters that they take
# every branch.  name: dict(size=(w, h), lab, want=(L, ab), scale, full=(full_w, full_h), masks=[mask(...), ...]); `area` = True stands for
# area_plane(w, h).
_P = dict(parametric_enabled=True)
CASES = {
    # 67 x 45: odd, w % 4 == 3; one region with three curves is 72 KB of polylines (the launch raises its LDS limit)
    "67x45-rgb-L-three-curves-ld50": dict(size=(67, 45), lab=False, want=(True, False), scale=1.0, full=(-1, -1),
                                          masks=[mask(**_P, hue=HUE_A, chromaticity=CHROMA_A, lightness=LIGHT_A, lightness_detail=50)]),
    "67x45-lab-ab-blur-5": dict(size=(67, 45), lab=True, want=(False, True), scale=1.0, full=(-1, -1),
                                masks=[mask(**_P, hue=HUE_B, chromaticity=CHROMA_A, blur=-5.0)]),
    # a region without curves beside regions with one; blur 3, blur below -10 (none), inverted, opacity 40
    "67x45-rgb-both-three-regions": dict(size=(67, 45), lab=False, want=(True, True), scale=1.0, full=(-1, -1),
                                         masks=[mask(**_P, hue=HUE_A, blur=3.0), mask(**_P),
                                                mask(**_P, lightness=LIGHT_B, lightness_detail=100, blur=-20.0, inverted=True, opacity=40)]),
    "67x45-rgb-L-no-mask": dict(size=(67, 45), lab=False, want=(True, True), scale=1.0, full=(-1, -1),
                                masks=[mask(**_P), mask(hue=HUE_A, lightness=LIGHT_A)]),            # (curves of a disabled parametric mask do not count)
    "67x45-lab-L-absent-curves": dict(size=(67, 45), lab=True, want=(True, False), scale=1.0, full=(-1, -1),
                                      masks=[mask(**_P, hue=EMPTY, chromaticity=LINEAR, lightness=DEFAULT_CL, opacity=70),
                                             mask(**_P, hue=IDENTITY, chromaticity=CHROMA_A)]),
    # five regions: two launches of the fused pass (four regions each at most, 144 KB of polylines each at most)
    "67x45-rgb-ab-five-regions": dict(size=(67, 45), lab=False, want=(False, True), scale=2.0, full=(400, 300),
                                      masks=[mask(**_P, hue=HUE_A, chromaticity=CHROMA_A, lightness=LIGHT_A), mask(**_P, hue=HUE_B),
                                             mask(**_P, chromaticity=CHROMA_A, lightness=LIGHT_B, blur=1.0),
                                             mask(**_P, hue=HUE_B, chromaticity=CHROMA_A, lightness=LIGHT_A, inverted=True),
                                             mask(**_P, lightness=LIGHT_A, opacity=40)]),
    "256x131-rgb-L-ld0-ld100": dict(size=(256, 131), lab=False, want=(True, False), scale=1.0, full=(1024, 524),
                                    masks=[mask(**_P, lightness=LIGHT_A, lightness_detail=0), mask(**_P, hue=HUE_A, lightness=LIGHT_B, lightness_detail=100, blur=-5.0)]),
    "256x131-lab-both-threshold+30-area": dict(size=(256, 131), lab=True, want=(True, True), scale=1.0, full=(-1, -1),
                                               masks=[mask(**_P, hue=HUE_A, contrast_threshold=30, area=True)]),
    "256x131-rgb-L-threshold-30-no-mask": dict(size=(256, 131), lab=False, want=(True, False), scale=2.0, full=(-1, -1),
                                               masks=[mask(**_P, contrast_threshold=-30, blur=4.0)]),
    "256x131-rgb-L-posterize": dict(size=(256, 131), lab=False, want=(True, False), scale=1.0, full=(2560, 1310),
                                    masks=[mask(**_P, chromaticity=CHROMA_A, posterization=1), mask(**_P, hue=HUE_A, posterization=1, smoothing=60),
                                           mask(**_P, lightness=LIGHT_A, lightness_detail=50, posterization=6, inverted=True),
                                           mask(**_P, hue=HUE_B, posterization=6, smoothing=60, opacity=40, area=True)]),
    # just above 1920: the contrast threshold works on the rescaled guide (1919 x 47)
    "1930x48-rgb-L-threshold-rescaled": dict(size=(1930, 48), lab=False, want=(True, False), scale=1.0, full=(-1, -1),
                                             masks=[mask(**_P, hue=HUE_A, contrast_threshold=30), mask(**_P, contrast_threshold=-30, blur=3.0)]),
}
_CACHE = {}


def case(name):
    """(input planes, mode, masks with their area arrays, keyword arguments of generate(), the checker's L planes, ab planes, [Info] and
    counts), computed once and read-only"""
    if name not in _CACHE:
        c = CASES[name]
        w, h = c["size"]
        img = scene(w, h, seed=len(name), lab=c["lab"])
        masks = []
        for m in c["masks"]:
            m = dict(m)
            if m["area"] is True:
                m["area"] = area_plane(w, h)
                m["area"].setflags(write=False)
            masks.append(m)
        kw = dict(want_L=c["want"][0], want_ab=c["want"][1], full_w=c["full"][0], full_h=c["full"][1], scale=c["scale"])
        mode = MODE_LAB if c["lab"] else MODE_RGB
        rc, L, ab, info, counts = generate(img, mode, masks, **kw)
        assert rc == 0, (name, rc)
        for a in img + [x for x in (L, ab) if x is not None]:
            a.setflags(write=False)
        _CACHE[name] = (img, mode, masks, kw, L, ab, info, counts)
    return _CACHE[name]
