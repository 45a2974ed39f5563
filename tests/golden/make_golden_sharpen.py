"""Records tests/golden/gauss_divmult.npz: the GAUSS_DIV and GAUSS_MULT forms of the reference's gaussianBlur (rtengine/gauss.cc), from the
reference's own gauss.cc compiled where it lies, with the reference's Release flags (oracle/Makefile.ref's FLAGS).

Runs only where the reference tree exists (ART_REFERENCE, default /root/reference/rtengine).  Nothing of the reference and nothing compiled
from it lands in the repository: the build happens in a temporary directory, the file written holds planes of numbers only.

gauss.cc compiles as it is, but boxblur.h pulls StopWatch.h and with it glibmm.  So the build directory is a directory of links to the
reference's headers and gauss.cc with ONE stand-in of ours, a StopWatch.h whose BENCHFUN / BENCHFUNMICRO are empty.  The driver (ours as well)
calls gaussianBlur inside an `omp parallel` region, as deconvsharpening does (ipsharpen.cc:198-204).

For sigma in SIGMAS and W x H in SIZES the file holds  d_<sigma>_<W>x<H> (DIV) and m_<sigma>_<W>x<H> (MULT, the prior dst being dst0_<W>x<H>)
for the inputs src_<W>x<H> / div_<W>x<H>, and for the 5x5 / 7x7 regimes k_<sigma>: the kernel coefficients this machine's libm gives
(c21 c20 c11 c10 c00, or c31 c30 c22 c21 c20 c11 c10 c00), so that a libm difference is told apart from a stencil difference.
"""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("ART_REFERENCE", "/root/reference/rtengine")
OUT = os.path.join(HERE, "gauss_divmult.npz")

SIGMAS = (0.22, 0.45, 0.6, 0.75, 0.84, 1.0, 1.15, 1.6, 2.5)
SIZES = ((8, 8), (23, 9), (67, 41))
GAUSS_STANDARD, GAUSS_MULT, GAUSS_DIV = 0, 1, 2

DRIVER = r"""
#include "gauss.h"
#include <cmath>
#include <vector>
extern "C" void gd_blur(float *src, float *dst, float *div, int W, int H, double sigma, int type)
{
    std::vector<float *> s(H), d(H), v(H);
    for (int i = 0; i < H; ++i) { s[i] = src + (size_t)i * W; d[i] = dst + (size_t)i * W; v[i] = div ? div + (size_t)i * W : nullptr; }
#pragma omp parallel
    {
        gaussianBlur(s.data(), d.data(), W, H, sigma, nullptr, (eGaussType)type, div ? v.data() : nullptr);
    }
}
// the normalised (2R+1)^2 kernel of the 5x5 / 7x7 forms: exp in double, sum in float, row-major; limit = 0.84 / 1.15
extern "C" void gd_kernel(float sigma, int R, double limit, float *out /* (2R+1)^2 */)
{
    const double temp = -2.f * (sigma * sigma);
    const int n = 2 * R + 1;
    float sum = 0.f;
    for (int i = -R; i <= R; ++i)
        for (int j = -R; j <= R; ++j) {
            float &k = out[(i + R) * n + j + R];
            if ((double)(i * i + j * j) <= (3.0 * limit) * (3.0 * limit)) { k = std::exp((i * i + j * j) / temp); sum += k; }
            else k = 0.f;
        }
    for (int i = 0; i < n * n; ++i) out[i] /= sum;
}
"""


def ref_flags():
    text = open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "Makefile.ref")).read()
    return re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1).split()


def build(tmp):
    shadow = os.path.join(tmp, "shadow")
    os.mkdir(shadow)
    for name in os.listdir(REF):
        if name.endswith(".h") and name != "StopWatch.h":
            os.symlink(os.path.join(REF, name), os.path.join(shadow, name))
    os.symlink(os.path.join(REF, "gauss.cc"), os.path.join(shadow, "gauss.cc"))
    with open(os.path.join(shadow, "StopWatch.h"), "w") as f:
        f.write("#pragma once\n#define BENCHFUN\n#define BENCHFUNMICRO\n")
    with open(os.path.join(tmp, "driver.cc"), "w") as f:
        f.write(DRIVER)
    so = os.path.join(tmp, "libgd.so")
    subprocess.check_call(["g++"] + ref_flags() + ["-I" + shadow, "-shared", "-o", so, os.path.join(tmp, "driver.cc"), os.path.join(shadow, "gauss.cc")])
    return C.CDLL(so)


def inputs(w, h):
    """src: what a blur reads (an estimate around 1000 .. 70000 with a block of zeros, a few negatives and a value above 65535);
    div: the luminance the DIV form divides (zeros, negatives -- also in the last three rows -- and a value above 65535); dst0: the estimate the MULT form multiplies"""
    rng = np.random.default_rng(1000 * w + h)
    src = rng.uniform(900.0, 40000.0, (h, w)).astype(np.float32)
    src[h // 2:h // 2 + 2, w // 3:w // 3 + 3] = 0.0
    src[1, 2] = -350.0
    src[h - 2, w - 4] = -0.5
    src[3, w - 2] = 70000.0
    src[h - 1, 0] = 0.0
    div = rng.uniform(0.0, 50000.0, (h, w)).astype(np.float32)
    div[0, 1] = 0.0
    div[h // 2, w // 2] = -20.0
    div[2, 3] = 66000.0
    # negative divisors in the last three rows, where gaussVerticalSsediv's 8-column groups carry no max(.., 0): one in a column of those
    # groups, one in the last column (a scalar tail column unless W is a multiple of 8), and one in a row above for contrast
    div[h - 1, 1] = -30.0
    div[h - 2, w - 1] = -40.0
    div[h - 3, 5] = -50.0
    div[h - 4, 6] = -60.0
    dst0 = rng.uniform(0.0, 3.0, (h, w)).astype(np.float32)
    dst0[4, 4] = 0.0
    dst0[h - 3, 1] = 70000.0
    dst0[5, w - 1] = -1.5
    return src, div, dst0


def key(sigma, w, h):
    return f"{sigma:g}_{w}x{h}"


def main():
    if not os.path.isdir(REF):
        sys.exit(f"{REF}: no reference tree here")
    fp = C.POINTER(C.c_float)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        lib.gd_blur.argtypes = [fp, fp, fp, C.c_int, C.c_int, C.c_double, C.c_int]
        lib.gd_kernel.argtypes = [C.c_float, C.c_int, C.c_double, fp]
        for w, h in SIZES:
            src, div, dst0 = inputs(w, h)
            out[f"src_{w}x{h}"], out[f"div_{w}x{h}"], out[f"dst0_{w}x{h}"] = src, div, dst0
            for sigma in SIGMAS:
                s, d = src.copy(), np.full((h, w), np.nan, np.float32)
                lib.gd_blur(s.ctypes.data_as(fp), d.ctypes.data_as(fp), div.ctypes.data_as(fp), w, h, sigma, GAUSS_DIV)
                out["d_" + key(sigma, w, h)] = d
                s, m = src.copy(), dst0.copy()
                lib.gd_blur(s.ctypes.data_as(fp), m.ctypes.data_as(fp), None, w, h, sigma, GAUSS_MULT)
                out["m_" + key(sigma, w, h)] = m
        for sigma in SIGMAS:
            if 0.6 <= sigma <= 1.15:
                R, limit = (2, 0.84) if sigma <= 0.84 else (3, 1.15)
                k = np.zeros((2 * R + 1, 2 * R + 1), np.float32)
                lib.gd_kernel(sigma, R, limit, k.ctypes.data_as(fp))
                out[f"k_{sigma:g}"] = (np.array([k[0, 1], k[0, 2], k[1, 1], k[1, 2], k[2, 2]]) if R == 2 else
                                       np.array([k[0, 2], k[0, 3], k[1, 1], k[1, 2], k[1, 3], k[2, 2], k[2, 3], k[3, 3]])).astype(np.float32)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
