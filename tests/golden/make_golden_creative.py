"""Records tests/golden/creative.npz: what the graduated filter's and the vignette filter's factors are made of, from the reference's own sleef.h.

Runs only where the reference tree exists: oracle/Makefile.ref builds oracle/_ref/libartref.so from the reference headers where they lie, and
its ref_xsinf / ref_xcosf / ref_xcbrtf / ref_pow_F (oracle/ref_driver.cc) are the reference's scalar functions.  The file written holds numbers only:

  x_trig, sin_trig, cos_trig      4096 arguments spread over [-10, 10] and the reference's xsinf / xcosf of them;
  pow_a, pow_b, pow_F             arguments black-and-white's gamma tables hand to pow_F (i / 65535.f and a gamma) and the reference's values;
  case_<k>                        the parameters of case k as one float64 row (the order of FIELDS below);
  sinargs_<k>, sin_<k>, cosargs_<k>, cos_<k>
                                  what the ramp branches of case k hand to xsinf / xcosf, in raster order (the gradient ahead of the vignette within
                                  a pixel), and the reference's values;
  cbrtargs_<k>, cbrt_<k>          likewise normn's degree-6 branch and xcbrtf;
  gfac_<k>, vfac_<k>              the two factor planes (1.0 where a tool does not run).

The planes are computed HERE, in numpy one operation at a time, float32 / float64 as iptransform.cc declares each variable (L677-983), with the
recorded values standing in for the sleef calls and libm's powf / cos / tan / fmod / pow for the derived parameters: no code is shared with
tests/emul/creative_ref.cc, whose leaves and factor planes tests/test_creative_checker.py compares with these.
"""
import ctypes as C
import ctypes.util
import math
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "creative.npz")
F, D = np.float32, np.float64

FIELDS = ("w", "h", "g_on", "g_degree", "g_feather", "g_strength", "g_cx", "g_cy", "v_on", "v_strength", "v_feather", "v_roundness", "v_cx", "v_cy",
          "crop_on", "crop_x", "crop_y", "crop_w", "crop_h", "off_x", "off_y", "full_w", "full_h", "scale")


def case(w, h, g=None, v=None, crop=None, off=(0, 0), full=(-1, -1), scale=1.0):
    g_, v_, c_ = g or (0.0, 25, 0.6, 0, 0), v or (0.6, 50, 50, 0, 0), crop or (0, 0, 0, 0)
    return dict(zip(FIELDS, (w, h, int(g is not None), *g_, int(v is not None), *v_, int(crop is not None), *c_, *off, *full, scale)))


# small frames that reach every ramp: the snapped, the plain and the transposed gradient in both forms; every super-ellipse degree, the plain
# ellipse and the circle-wards one, portrait and landscape, strength 6 (scale 0) and a brightening vignette; a window of a larger picture; a crop
# at scale 2 with its fade; both tools
CASES = (case(13, 9, g=(0, 60, 2.0, 0, 0)), case(13, 9, g=(0.05, 100, -1.5, 20, -10)), case(9, 13, g=(45, 40, 2.0, 0, 0)), case(13, 9, g=(135, 80, -1.5, -30, 20)),
         case(12, 10, g=(270, 50, 1.0, 10, 10)), case(11, 7, g=(-30, 100, 0.7, 0, 0)), case(11, 7, g=(400, 25, -0.4, 100, -60)),
         case(13, 9, v=(0.6, 50, 0, 0, 0)), case(13, 9, v=(6.0, 100, 20, 10, -10)), case(9, 13, v=(-2.0, 50, 49, 0, 0)), case(13, 9, v=(0.6, 0, 50, 0, 0)),
         case(9, 13, v=(1.0, 100, 51, -20, 30)), case(12, 12, v=(-2.0, 50, 100, 0, 0)), case(13, 9, v=(0.6, 50, 35, 0, 0)),
         case(15, 11, g=(-30, 25, 2.0, 20, -10), off=(13, 7), full=(60, 40)), case(23, 15, v=(0.6, 50, 20, 0, 0), crop=(14, 10, 20, 12), scale=2.0),
         case(13, 9, g=(30, 40, 1.2, 10, -20), v=(1.5, 60, 30, -20, 10)))

RT_PI = 3.14159265358979323846
RT_PI_F_2 = F(1.57079632679489661923)


def load_ref():
    if not os.path.isdir("/root/reference/rtengine"):
        sys.exit("the reference tree is not here: the fixture is recorded where it is")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "-f", "Makefile.ref"])
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libartref.so"))
    fp = C.POINTER(C.c_float)
    for n in ("ref_xsinf", "ref_xcosf", "ref_xcbrtf"):
        getattr(lib, n).restype = None
        getattr(lib, n).argtypes = [fp, fp, C.c_size_t]
    lib.ref_pow_F.restype = None
    lib.ref_pow_F.argtypes = [fp, fp, fp, C.c_size_t]

    def call1(name):
        def f(x):
            x = np.ascontiguousarray(x, F).reshape(-1)
            y = np.empty_like(x)
            getattr(lib, name)(x.ctypes.data_as(fp), y.ctypes.data_as(fp), x.size)
            return y
        return f

    def pow_F(a, b):
        a, b = np.ascontiguousarray(a, F).reshape(-1), np.ascontiguousarray(b, F).reshape(-1)
        y = np.empty_like(a)
        lib.ref_pow_F(a.ctypes.data_as(fp), b.ctypes.data_as(fp), y.ctypes.data_as(fp), a.size)
        return y
    return call1("ref_xsinf"), call1("ref_xcosf"), call1("ref_xcbrtf"), pow_F


LIBM = C.CDLL(ctypes.util.find_library("m"))
LIBM.powf.restype = C.c_float
LIBM.powf.argtypes = [C.c_float, C.c_float]


def powf(a, b):
    return F(LIBM.powf(float(F(a)), float(F(b))))


def trunc(v):
    return int(v)            # float -> int conversion truncates towards zero


class Rec:
    """the sleef calls of one case: arguments in call order and the reference's values"""

    def __init__(self, fns):
        self.fn = dict(zip(("sin", "cos", "cbrt"), fns))
        self.args = {"sin": [], "cos": [], "cbrt": []}
        self.vals = {"sin": [], "cos": [], "cbrt": []}

    def __call__(self, which, x):
        x = F(x)
        y = F(self.fn[which](np.array([x], F))[0])
        self.args[which].append(x)
        self.vals[which].append(y)
        return y


def pow3(x):
    return F(F(x * x) * x)


def pow4(x):
    return F(F(x * x) * F(x * x))


def normn(a, b, n, rec):
    a, b = F(a), F(b)
    if n == 2:
        return F(np.sqrt(F(F(a * a) + F(b * b))))
    if n == 4:
        return F(np.sqrt(F(np.sqrt(F(pow4(a) + pow4(b))))))
    if n == 6:
        return F(np.sqrt(rec("cbrt", F(F(pow3(a) * pow3(a)) + F(pow3(b) * pow3(b))))))
    if n == 8:
        return F(np.sqrt(F(np.sqrt(F(np.sqrt(F(F(pow4(a) * pow4(a)) + F(pow4(b) * pow4(b)))))))))
    raise AssertionError(n)


def grad_params(oW, oH, c):
    """calcGradientParams (L677-758): doubles are Python floats, the struct's floats are np.float32"""
    w, h = oW, oH
    stops = float(c["g_strength"])
    span = c["g_feather"] / 100.0
    cx = c["g_cx"] / 200.0 + 0.5
    cy = c["g_cy"] / 200.0 + 0.5
    ang = float(c["g_degree"]) / 180.0 * RT_PI
    ang = math.fmod(ang, 2 * RT_PI)
    if ang < 0.0:
        ang += 2.0 * RT_PI
    gp = dict(bright_top=False, transpose=False, angle_is_zero=False, h=h)
    if abs(math.cos(ang)) < 0.707:
        gp["transpose"] = True
        ang += 0.5 * RT_PI
        cx, cy = 1.0 - cy, cx
    ang = math.fmod(ang, 2 * RT_PI)
    if 0.5 * RT_PI < ang < RT_PI:
        ang += RT_PI
        gp["bright_top"] = True
    elif RT_PI <= ang < 1.5 * RT_PI:
        ang -= RT_PI
        gp["bright_top"] = True
    if abs(ang) < 0.001 or abs(ang - 2 * RT_PI) < 0.001:
        ang = 0.0
        gp["angle_is_zero"] = True
    if gp["transpose"]:
        gp["bright_top"] = not gp["bright_top"]
        w, h = h, w
    gp["scale"] = F(1.0 / math.pow(2.0, stops))
    gp["topmul"], gp["botmul"] = (F(1.0), gp["scale"]) if gp["bright_top"] else (gp["scale"], F(1.0))
    gp["ta"] = F(math.tan(ang))
    gp["xc"] = F(w * cx)
    gp["yc"] = F(h * cy)
    hyp = F(np.sqrt(F(F(F(h) * F(h)) + F(F(w) * F(w)))))                    # sqrt of a float: the float overload
    gp["ys"] = F(float(hyp) * (span / math.cos(ang)))
    gp["ys_inv"] = F(1.0 / float(gp["ys"]))
    gp["top_edge_0"] = F(float(gp["yc"]) - float(gp["ys"]) / 2.0)
    if float(gp["ys"]) < 1.0 / h:
        gp["ys_inv"] = F(0)
        gp["ys"] = F(0)
    return gp


def grad_factor(gp, x, y, rec):
    """calcGradientFactor (L761-812)"""
    gy = x if gp["transpose"] else y
    if gp["angle_is_zero"]:
        top_edge = gp["top_edge_0"]
    else:
        gx = gp["h"] - y - 1 if gp["transpose"] else x
        top_edge = F(gp["top_edge_0"] - F(gp["ta"] * F(F(gx) - gp["xc"])))
    if F(gy) < top_edge:
        return gp["topmul"]
    if F(gy) >= F(top_edge + gp["ys"]):
        return gp["botmul"]
    val = F(F(F(gy) - top_edge) * gp["ys_inv"])
    if gp["bright_top"]:
        val = F(F(1.0) - val)
    val = F(val * RT_PI_F_2)
    if gp["scale"] < F(1.0):
        val = pow3(rec("sin", val))
    else:
        val = F(F(1.0) - pow3(rec("cos", val)))
    return F(float(gp["scale"]) + float(val) * (1.0 - float(gp["scale"])))      # evaluated in double, returned as float


def pcv_params(fW, fH, oW, oH, c):
    """calcPCVignetteParams (L828-895)"""
    p = {}
    roundness = c["v_roundness"] / 100.0
    p["feather"] = F(c["v_feather"] / 100.0)
    if c["crop_on"]:
        sW, sH = F(F(oW) / F(fW)), F(F(oH) / F(fH))
        p["ew"], p["eh"] = trunc(F(F(c["crop_w"]) * sW)), trunc(F(F(c["crop_h"]) * sH))
        p["x1"], p["y1"] = trunc(F(F(c["crop_x"]) * sW)), trunc(F(F(c["crop_y"]) * sH))
    else:
        p["ew"], p["eh"], p["x1"], p["y1"] = oW, oH, 0, 0
    dW = F(F(F(c["v_cx"]) / F(200.0)) * F(p["ew"]))
    dH = F(F(F(c["v_cy"]) / F(200.0)) * F(p["eh"]))
    p["ex"] = trunc(F(F(p["x1"]) + dW))
    p["ey"] = trunc(F(F(p["y1"]) + dH))
    p["x2"] = trunc(F(F(p["x1"] + p["ew"]) + F(abs(dW))))
    p["y2"] = trunc(F(F(p["y1"] + p["eh"]) + F(abs(dH))))
    p["fadeout_mul"] = F(1.0 / (0.05 * float(F(np.sqrt(F(oW * oW + oH * oH))))))
    short_side, long_side = F(min(p["ew"], p["eh"])), F(max(p["ew"], p["eh"]))
    p["sep"], p["sepmix"] = 2, F(0)
    p["oe_a"] = F(math.sqrt(2.0) * float(long_side) * 0.5)
    p["oe_b"] = F(F(p["oe_a"] * short_side) / long_side)
    p["ie_mul"] = F((1.0 / math.sqrt(2.0)) * (1.0 - float(p["feather"])))
    p["super"] = False
    p["portrait"] = p["ew"] < p["eh"]
    if roundness < 0.5:
        p["super"] = True
        sepf = F(F(2) + F(F(4) * powf(1.0 - 2 * roundness, 1.3)))
        p["sep"] = trunc(sepf) & ~1
        p["sepmix"] = F(float(F(sepf - F(p["sep"]))) * 0.5)
        for name, n in (("1", p["sep"]), ("2", p["sep"] + 2)):
            root = powf(2.0, 1.0 / n)
            p["oe%s_a" % name] = F(float(F(root * long_side)) * 0.5)
            p["oe%s_b" % name] = F(F(p["oe%s_a" % name] * short_side) / long_side)
            p["ie%s_mul" % name] = F((1.0 / float(root)) * (1.0 - float(p["feather"])))
    if roundness > 0.5:
        rad = F(float(F(np.sqrt(F(p["ew"] * p["ew"] + p["eh"] * p["eh"])))) / 2.0)
        diff_a, diff_b = F(rad - p["oe_a"]), F(rad - p["oe_b"])
        p["oe_a"] = F(float(p["oe_a"]) + float(F(diff_a * F(2))) * (roundness - 0.5))
        p["oe_b"] = F(float(p["oe_b"]) + float(F(diff_b * F(2))) * (roundness - 0.5))
    p["scale"] = powf(2, -float(c["v_strength"]))
    if float(c["v_strength"]) >= 6.0:
        p["scale"] = F(0.0)
    return p


def pcv_factor(p, x, y, rec):
    """calcPCVignetteFactor (L898-983)"""
    fo = F(1.0)
    if x < p["x1"] or x > p["x2"] or y < p["y1"] or y > p["y2"]:
        dist_x = max(p["x1"] - x if x < p["x1"] else x - p["x2"], 0)
        dist_y = max(p["y1"] - y if y < p["y1"] else y - p["y2"], 0)
        fo = F(F(np.sqrt(F(dist_x * dist_x + dist_y * dist_y))) * p["fadeout_mul"])
        if fo >= F(1.0):
            return F(1.0)
    a = F(abs(F(F(x - p["ex"]) - F(F(p["ew"]) * F(0.5)))))
    b = F(abs(F(F(y - p["ey"]) - F(F(p["eh"]) * F(0.5)))))
    if p["portrait"]:
        a, b = b, a
    dist = normn(a, b, 2, rec)
    cs, sn = (F(1.0), F(0.0)) if dist == F(0.0) else (F(a / dist), F(b / dist))
    if p["super"]:
        dist_oe1 = F(F(p["oe1_a"] * p["oe1_b"]) / normn(F(p["oe1_b"] * cs), F(p["oe1_a"] * sn), p["sep"], rec))
        dist_oe2 = F(F(p["oe2_a"] * p["oe2_b"]) / normn(F(p["oe2_b"] * cs), F(p["oe2_a"] * sn), p["sep"] + 2, rec))
        dist_ie1, dist_ie2 = F(p["ie1_mul"] * dist_oe1), F(p["ie2_mul"] * dist_oe2)
        one_m = F(F(1.0) - p["sepmix"])
        dist_oe = F(F(dist_oe1 * one_m) + F(dist_oe2 * p["sepmix"]))
        dist_ie = F(F(dist_ie1 * one_m) + F(dist_ie2 * p["sepmix"]))
    else:
        t1, t2 = F(p["oe_b"] * cs), F(p["oe_a"] * sn)
        dist_oe = F(F(p["oe_a"] * p["oe_b"]) / F(np.sqrt(F(F(t1 * t1) + F(t2 * t2)))))
        dist_ie = F(p["ie_mul"] * dist_oe)
    if dist <= dist_ie:
        return F(1.0)
    if dist >= dist_oe:
        val = p["scale"]
    else:
        val = F(F(RT_PI_F_2 * F(dist - dist_ie)) / F(dist_oe - dist_ie))
        if p["scale"] < F(1.0):
            val = pow4(rec("cos", val))
        else:
            val = F(F(1) - pow4(rec("sin", val)))
        val = F(p["scale"] + F(val * F(F(1.0) - p["scale"])))
    if fo < F(1.0):
        val = F(fo + F(val * F(F(1.0) - fo)))
    return val


def planes(c, fns):
    """creativeGradients (L1390-1405) and the loop of transformLuminanceOnly (L1018-1041) without the pixels: the two factor planes"""
    w, h = c["w"], c["h"]
    cw, ch = (w, h) if c["full_w"] < 0 else (c["full_w"], c["full_h"])
    fw, fh = trunc(cw * float(c["scale"])), trunc(ch * float(c["scale"]))
    g_on = bool(c["g_on"]) and abs(float(c["g_strength"])) > 1e-15
    v_on = bool(c["v_on"]) and abs(float(c["v_strength"])) > 1e-15
    gp = grad_params(cw, ch, c) if g_on else None
    pv = pcv_params(fw, fh, cw, ch, c) if v_on else None
    rec = Rec(fns)
    gfac, vfac = np.ones((h, w), F), np.ones((h, w), F)
    for y in range(h):
        for x in range(w):
            if g_on:
                gfac[y, x] = grad_factor(gp, c["off_x"] + x, c["off_y"] + y, rec)
            if v_on:
                vfac[y, x] = pcv_factor(pv, c["off_x"] + x, c["off_y"] + y, rec)
    return gfac, vfac, rec


def main():
    xsinf, xcosf, xcbrtf, pow_F = load_ref()
    rng = np.random.default_rng(20)
    x = np.sort(np.concatenate([np.linspace(-10.0, 10.0, 2048), rng.uniform(-10.0, 10.0, 2040), [0.0, -0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi, 1e-8, -1e-8]])).astype(F)
    out = {"x_trig": x, "sin_trig": xsinf(x), "cos_trig": xcosf(x)}
    idx = np.concatenate([np.arange(0, 65536, 257), [1, 2, 65534, 65535]]).astype(F)
    gam = np.array([1.0 - 20.0 / 125.0, 1.0 + 35.0 / 100.0, 1.0 - 60.0 / 125.0, 2.0, 0.2], F)
    pa = np.repeat(idx / F(65535.0), gam.size).astype(F)
    pb = np.tile(gam, idx.size).astype(F)
    out.update(pow_a=pa, pow_b=pb, pow_F=pow_F(pa, pb))
    for k, c in enumerate(CASES):
        gfac, vfac, rec = planes(c, (xsinf, xcosf, xcbrtf))
        out["case_%d" % k] = np.array([float(c[f]) for f in FIELDS], D)
        for which in ("sin", "cos", "cbrt"):
            out["%sargs_%d" % (which, k)] = np.array(rec.args[which], F)
            out["%s_%d" % (which, k)] = np.array(rec.vals[which], F)
        out["gfac_%d" % k], out["vfac_%d" % k] = gfac, vfac
        print("case %2d: %3d sin, %3d cos, %3d cbrt; factors %.4f .. %.4f / %.4f .. %.4f" % (
            k, len(rec.args["sin"]), len(rec.args["cos"]), len(rec.args["cbrt"]), gfac.min(), gfac.max(), vfac.min(), vfac.max()))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes, %d arrays)" % (OUT, os.path.getsize(OUT), len(out)))


if __name__ == "__main__":
    main()
