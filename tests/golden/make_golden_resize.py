"""Records tests/golden/lanczos.npz: what the Lanczos weights of the Resize tool are made of, from the reference's own sleef.h.

Runs only where the reference tree exists: oracle/Makefile.ref builds oracle/_ref/libartref.so from the reference headers where they lie, and
its ref_xsinf (oracle/ref_driver.cc) is the reference's scalar xsinf.  The file written holds numbers only:

  x_<case>, sin_<case>   the arguments Lanc hands to xsinf for the case's destination positions, in call order (for every tap in the sinc
                         branch: pi * z, then pi * z / 3), and ref_xsinf of them;
  w_<case>, lo_<case>, hi_<case>
                         the normalised weight rows (n x support, zeros behind a row's taps) and tap ranges.  They are computed HERE, in numpy
                         float32 one operation at a time from the formulas of ipresize.cc:83-109 with sin_<case> standing in for xsinf: no
                         code is shared with tests/emul/resize_ref.cc, whose xsinf and weights tests/test_resize_checker.py compares with these.

<case> = <source length>_<destination length>_<scale as %.9g>.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "lanczos.npz")
F = np.float32

# (source length, destination length, scale): the GPU tests' widths and heights at their scales; a destination two and five longer than the scale implies (the
# latter has positions without taps), and 1/7, where float rounding puts taps into Lanc's zero branch
CASES = ((67, 34, 0.5), (45, 15, 1 / 3), (131, 48, 0.37), (70, 56, 0.8), (131, 16, 1 / 8), (67, 10, 1 / 8), (23, 35, 1.5), (17, 34, 2.0), (23, 92, 4.0),
         (67, 36, 0.5), (67, 39, 0.5), (67, 10, 1 / 7), (3, 1, 0.4), (1, 1, 0.7))


def case_name(n_src, n_dst, scale):
    return "%d_%d_%.9g" % (n_src, n_dst, float(F(scale)))


def taps(n_src, n_dst, scale):
    """per destination position: (x0, first, last), float32 arithmetic as in the reference"""
    scale = F(scale)
    delta, a, sc = F(1.0) / scale, F(3.0), min(scale, F(1.0))
    out = []
    for j in range(n_dst):
        x0 = (F(j) + F(0.5)) * delta - F(0.5)
        first = max(0, int(np.floor(x0 - a / sc)) + 1)
        last = min(n_src, int(np.floor(x0 + a / sc)) + 1)
        out.append((x0, first, last))
    return out, a, sc


def sinc_args(n_src, n_dst, scale):
    """the arguments of xsinf, in call order"""
    rows, a, sc = taps(n_src, n_dst, scale)
    args = []
    for x0, first, last in rows:
        for jj in range(first, last):
            z = sc * (x0 - F(jj))
            if z * z < F(1e-6) or z * z > a * a:
                continue
            x = F(np.pi) * z
            args += [x, x / a]
    return np.array(args, F)


def weight_rows(n_src, n_dst, scale, sines):
    rows, a, sc = taps(n_src, n_dst, scale)
    support = int(F(2.0) * a / sc) + 1
    w = np.zeros((n_dst, support), F)
    lo, hi = np.zeros(n_dst, np.int32), np.zeros(n_dst, np.int32)
    it = iter(sines)
    for j, (x0, first, last) in enumerate(rows):
        lo[j], hi[j] = first, last
        ws = F(0.0)
        for jj in range(first, last):
            z = sc * (x0 - F(jj))
            if z * z < F(1e-6):
                v = F(1.0)
            elif z * z > a * a:
                v = F(0.0)
            else:
                x = F(np.pi) * z
                v = a * F(next(it)) * F(next(it)) / (x * x)
            w[j, jj - first] = v
            ws = ws + v
        with np.errstate(all="ignore"):
            for k in range(max(last - first, 0)):
                w[j, k] = w[j, k] / ws
    assert next(it, None) is None
    return w, lo, hi


def main():
    if not os.path.isdir("/root/reference/rtengine") and not os.environ.get("ART_REFERENCE"):
        sys.exit("no reference tree here")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "-f", "Makefile.ref"])
    R = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libartref.so"))
    fp = C.POINTER(C.c_float)
    out = {}
    for n_src, n_dst, scale in CASES:
        name = case_name(n_src, n_dst, scale)
        x = sinc_args(n_src, n_dst, scale)
        y = np.empty_like(x)
        R.ref_xsinf(x.ctypes.data_as(fp), y.ctypes.data_as(fp), C.c_size_t(x.size))
        w, lo, hi = weight_rows(n_src, n_dst, scale, y)
        out["x_" + name], out["sin_" + name], out["w_" + name], out["lo_" + name], out["hi_" + name] = x, y, w, lo, hi
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
