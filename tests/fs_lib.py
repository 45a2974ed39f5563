"""Film simulation: the CPU checker (tests/emul/filmsim_ref.cc: CLUTApplication's HaldCLUT path and HaldCLUT::getRGB restated serially around
the oracle's two LUTf lookups), the tables, the scenes and the cases the tests use.  Test infrastructure only; nothing is read from a file."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
SRC = os.path.join(HERE, "emul", "filmsim_ref.cc")
SO = os.path.join(HERE, "emul", "libfilmsim_ref.so")
_fp = C.POINTER(C.c_float)
_LIB = None

COUNTERS = ("body", "tail", "below_zero", "above_max", "at_max", "frac_one", "cell_first_r", "cell_first_g", "cell_first_b",
            "cell_last_r", "cell_last_g", "cell_last_b", "igamma_below", "igamma_above")
# With a strength in [0, 1] the inverse table is never entered outside [0, 65535] by the scenes here.  Below zero it cannot be: the table's
# values, the encoded input and every weight are >= 0.  Above 65535 it could be if a * b + (1 - a) * c of two corners at 65535 rounded upwards,
# but the position inside a cell has few significant bits (it is x * flevel_minus_one minus an integer: a multiple of 2^-22 at level 4, of
# 2^-17 at level 256), the two products' rounding errors then cancel, and the strengths 1, 0.35 and 0 do not round upwards at 65535 either
# (measured: no such lookup in 1.8 million pixels of scenes full of saturated highlights).  So the branch gets cases of its own, OVERDRIVE:
# a strength of 1.5, which the ABI takes like any other finite float, leaves the range on both sides.


class Params(C.Structure):
    """fs_ref_params, the layout of artgpu_film_simulation_params"""
    _fields_ = [("strength", C.c_float), ("same_profile", C.c_int32), ("work_to_xyz", C.c_double * 9), ("xyz_to_clut", C.c_double * 9),
                ("clut_to_xyz", C.c_double * 9), ("xyz_to_work", C.c_double * 9)]


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
        _LIB.fs_ref_tables.restype = None
    return _LIB


# the working profile is Rec2020 (the matrices the other tools' tests use); the CLUT's is sRGB: ICCStore's D50-adapted sRGB matrix and its inverse,
# rounded as ART's iccmatrices.h prints them
SRGB_XYZ = np.array([[0.4360747, 0.3850649, 0.1430804], [0.2225045, 0.7168786, 0.0606169], [0.0139322, 0.0971045, 0.7141733]], dtype=np.float64)
XYZ_SRGB = np.array([[3.1338561, -1.6168667, -0.4906146], [-0.9787684, 1.9161415, 0.0334540], [0.0719453, -0.2289914, 1.4052427]], dtype=np.float64)


def params(strength=1.0, same_profile=True):
    p = Params()
    p.strength = float(strength); p.same_profile = int(bool(same_profile))
    if not same_profile:
        for name, m in (("work_to_xyz", oracle_lib.REC2020_WS_D), ("xyz_to_clut", XYZ_SRGB), ("clut_to_xyz", SRGB_XYZ), ("xyz_to_work", oracle_lib.REC2020_IWS_D)):
            getattr(p, name)[:] = [float(v) for v in np.asarray(m, np.float64).reshape(9)]
    return p


def tables():
    """(gamma2curve, igammatab_srgb) as Color::init builds them"""
    g, ig = np.empty(65536, np.float32), np.empty(65536, np.float32)
    checker().fs_ref_tables(g.ctypes.data_as(_fp), ig.ctypes.data_as(_fp))
    return g, ig


def film_simulation(img, table, level, p, want_cells=False):
    """CLUTApplication::operator() on copies of three H x W planes.  Returns (planes, counts dict[, cells (H, W, 3)])"""
    out = [np.array(a, dtype=np.float32, order="C") for a in img]
    h, w = out[0].shape
    table = np.ascontiguousarray(table)
    assert table.dtype == np.uint16 and table.shape[0] == level ** 3 and table.shape[1] in (3, 4)
    cn = Counts()
    cells = np.zeros((h, w, 3), np.int32) if want_cells else None
    rc = checker().fs_ref_tool(*[a.ctypes.data_as(_fp) for a in out], w, h, table.ctypes.data_as(C.POINTER(C.c_uint16)), int(level), int(table.shape[1]),
                               C.byref(p), C.byref(cn), cells.ctypes.data_as(C.POINTER(C.c_int32)) if want_cells else None)
    assert rc == 0, rc
    return (out, cn.as_dict(), cells) if want_cells else (out, cn.as_dict())


# ---------------------------------------------------------------------------------------------------------------------------------------
# tables: (level^3, 3) uint16, red fastest
# ---------------------------------------------------------------------------------------------------------------------------------------
KINDS = ("identity", "random", "look")
_TABLES = {}


def _axes(level):
    v = np.arange(level, dtype=np.float64) / (level - 1)
    b, g, r = np.meshgrid(v, v, v, indexing="ij")            # red fastest
    return r.ravel(), g.ravel(), b.ravel()


def clut(kind, level):
    """identity: the entry's own position; random: uniform uint16 with the eight corners of the last cell at 65535 (a cell that is flat at the
    top of the range); look: the identity through a per-channel curve that
    saturates in the highlights plus a term that mixes the other two channels in.  Cached, read-only."""
    key = (kind, level)
    if key not in _TABLES:
        r, g, b = _axes(level)
        if kind == "identity":
            t = np.stack([r, g, b], -1)
        elif kind == "random":
            rng = np.random.default_rng(1000 + level)
            t = rng.integers(0, 65536, (level ** 3, 3)).astype(np.float64) / 65535.0
            top = (r >= (level - 2) / (level - 1) - 1e-9) & (g >= (level - 2) / (level - 1) - 1e-9) & (b >= (level - 2) / (level - 1) - 1e-9)
            t[top] = 1.0
        elif kind == "look":
            t = np.stack([1.30 * r ** 0.80 + 0.06 * (g - b), 1.22 * g ** 0.90 + 0.05 * (b - r), 1.18 * b ** 1.10 + 0.04 * (r - g)], -1)
        else:
            raise KeyError(kind)
        t = np.rint(np.clip(t, 0.0, 1.0) * 65535.0).astype(np.uint16)
        t.setflags(write=False)
        _TABLES[key] = t
    return _TABLES[key]


def rgbx(table):
    """the same table with four values per entry, the fourth anything but zero"""
    t = np.empty((table.shape[0], 4), np.uint16)
    t[:, :3] = table
    t[:, 3] = (np.arange(table.shape[0]) * 40503 + 12345) & 0xFFFF
    return t


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------
def scene(w, h, seed=1):
    """three NaN-free planes: a smooth ramp with noise over the whole range; blocks of negative values, of values up to 1.5 x 65535, of exactly
    65535, of exactly 0 and of highlights in 60000 .. 65535 (the last cell of every level).  The blocks scale with the plane; on planes too
    small for them the later ones overwrite the earlier."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 200.0 + 64000.0 * (xx / max(w - 1, 1)) * (0.25 + 0.75 * yy / max(h - 1, 1))
    img = [(base * f + rng.normal(0.0, 700.0, (h, w))).astype(np.float32) for f in (1.0, 0.85, 0.6)]
    bw, bh = min(max(w // 6, 2), w), min(max(h // 4, 2), h)

    def block(ix, iy):
        x0, y0 = max(min(ix * (bw + 1) + 1, w - bw), 0), max(min(iy * (bh + 1) + 1, h - bh), 0)
        return slice(y0, y0 + bh), slice(x0, x0 + bw)

    fills = (lambda s: -rng.uniform(1.0, 900.0, s), lambda s: rng.uniform(1.0, 1.5, s) * 65535.0, lambda s: np.full(s, 65535.0),
             lambda s: np.zeros(s), lambda s: rng.uniform(60000.0, 65535.0, s))
    for k, fill in enumerate(fills):
        sy, sx = block(k % 3, k // 3)
        for c in range(3):
            img[c][sy, sx] = fill(img[c][sy, sx].shape).astype(np.float32)
    # the last columns (the scalar tail where w % 4 != 0) see the extremes too
    for c in range(3):
        col = img[c][:, w - 1]
        col[0::4] = 70000.0 + 1000.0 * c
        col[1::4] = -5.0 - c
    return img


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (9, 3), (1, 4), (5, 7), (48, 64), (41, 67), (45, 640))        # (h, w): 1x1, 3x9, 4x1, 7x5, 64x48, 67x41, 640x45 as width x height
LEVELS = (4, 9, 64)
BIG_LEVEL, BIG_SIZE = 144, (41, 67)
STRENGTHS = (1.0, 0.35, 0.0)
OVERDRIVE = ((41, 67, 9, "look", True, 1.5), (41, 67, 64, "random", False, 1.5), (7, 5, 4, "look", False, 1.5))     # case() arguments
_CACHE = {}


def case(h, w, level, kind, same_profile, strength):
    """(input planes, table, Params, the checker's planes, counts), computed once and read-only"""
    key = (h, w, level, kind, bool(same_profile), float(strength))
    if key not in _CACHE:
        img = scene(w, h, seed=7 + 13 * w + h)
        table = clut(kind, level)
        p = params(strength, same_profile)
        want, counts = film_simulation(img, table, level, p)
        for a in img + want:
            a.setflags(write=False)
        _CACHE[key] = (img, table, p, want, counts)
    return _CACHE[key]


def combos():
    """every (kind, same_profile, strength) a size and a level are run with"""
    return [(k, s, f) for k in KINDS for s in (True, False) for f in STRENGTHS]


def capi_params(p):
    """the checker's Params as capi.FilmSimulationParams (the same layout)"""
    from art_amd import capi
    return capi.FilmSimulationParams.from_buffer_copy(bytes(p))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what=""):
    """equality of float32 bit patterns"""
    for name, gp, wp in zip("rgb", got, want):
        bad = bits(gp) != bits(wp)
        assert not bad.any(), "%s plane %s: %d values differ, first at %s: %r != %r" % (
            what, name, int(bad.sum()), tuple(np.argwhere(bad)[0]), gp[tuple(np.argwhere(bad)[0])], wp[tuple(np.argwhere(bad)[0])])
