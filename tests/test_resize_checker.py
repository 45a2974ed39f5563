"""CPU: the Resize tool's checker (tests/rs_lib.py, tests/emul/resize_ref.cc) against the fixture recorded from the reference's own xsinf
(tests/golden/lanczos.npz), against the library's host function artgpu_resize_scale, against a float64 model that shares no code with it, and
the branches its scenes take."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from art_amd import capi
import rs_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (0.5, 1 / 3, 0.37, 0.8, 1 / 8, 1.5, 2.0, 4.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _golden_cases():
    g = np.load(rs_lib.GOLDEN)
    names = sorted(k[2:] for k in g.files if k.startswith("x_"))
    assert len(names) >= 10
    return g, names


def test_checker_xsinf_equals_the_reference_header():
    """xsinf on every argument Lanc produces for the fixture's cases (pi * z and pi * z / 3 for every tap of the sinc branch), bit for bit"""
    g, names = _golden_cases()
    total = 0
    for n in names:
        x, want = g["x_" + n], g["sin_" + n]
        got = rs_lib.xsinf(x)
        assert np.array_equal(_bits(got), _bits(want)), (n, int((_bits(got) != _bits(want)).sum()))
        total += x.size
    assert total > 3000


def test_checker_weights_equal_the_fixture():
    """the normalised weight rows, the tap ranges and the order xsinf is called in"""
    g, names = _golden_cases()
    for n in names:
        n_src, n_dst, scale = n.split("_")
        w, lo, hi, args = rs_lib.weights(int(n_dst), int(n_src), np.float32(float(scale)), want_args=True)
        assert np.array_equal(_bits(args), _bits(g["x_" + n])), n
        assert np.array_equal(lo, g["lo_" + n]) and np.array_equal(hi, g["hi_" + n]), n
        assert w.shape == g["w_" + n].shape and np.array_equal(_bits(w), _bits(g["w_" + n])), (n, int((_bits(w) != _bits(g["w_" + n])).sum()))
        taps = hi - lo
        full = taps > 0
        assert np.allclose(w[full].sum(1), 1.0, atol=1e-5), n


def test_resize_scale_equals_the_checker():
    """artgpu_resize_scale against the checker's resizeScale over dataspec x sizes x scales, with the 1e-5 rule and the upscaling rule"""
    sizes = ((8192, 5464), (5464, 8192), (67, 45), (131, 70), (23, 17), (1, 1), (6000, 4000))
    scales = (0.5, 0.25, 1 / 3, 0.37, 0.8, 1 / 8, 1.5, 2.0, 4.0, 1.0, 1.0 + 1e-5, 1.0 + 0.9e-5, 1.0 - 1e-5, 1.0 + 1.1e-5, 1.0 - 1.1e-5, 0.999, 1e-4)
    boxes = ((2048, 2048), (900, 900), (1920, 1080), (100, 3000), (10000, 10000), (8192, 5464), (8193, 5465), (1, 1))
    n = same = resized = 0
    for fw, fh in sizes:
        cases = [rs_lib.params(0, scale=s) for s in scales]
        for bw, bh in boxes:
            for up in (False, True):
                cases += [rs_lib.params(ds, width=bw, height=bh, allow_upscaling=up) for ds in (1, 2, 3)]
        cases += [rs_lib.params(0, scale=0.5, enabled=False), None, rs_lib.params(7, scale=0.3)]
        for p in cases:
            want = rs_lib.resize_scale(p, fw, fh)
            got = capi.resize_scale(None if p is None else rs_lib.capi_params(p), fw, fh)
            assert got[:2] == want[:2] and _bits(got[2]) == _bits(want[2]), (fw, fh, p and bytes(p), got, want)
            n += 1
            same += want[2] == 1.0
            resized += want[2] != 1.0
            if want[2] == 1.0:
                assert want[:2] == (fw, fh)
    assert n > 400 and same > 50 and resized > 300
    # the 1e-5 rule, both sides; the fit box never upscales unless allowed
    assert rs_lib.resize_scale(rs_lib.params(0, scale=1.0 + 0.9e-5), 8192, 5464) == (8192, 5464, 1.0)
    assert rs_lib.resize_scale(rs_lib.params(0, scale=1.0 + 1.1e-5), 8192, 5464)[2] != 1.0
    assert rs_lib.resize_scale(rs_lib.params(3, width=10000, height=10000), 67, 45) == (67, 45, 1.0)
    assert rs_lib.resize_scale(rs_lib.params(3, width=10000, height=10000, allow_upscaling=True), 67, 45)[2] > 1.0
    assert rs_lib.resize_scale(rs_lib.params(3, width=2048, height=2048), 8192, 5464)[:2] == (2048, 1366)


def test_abi_declared_bound_exported(tmp_path):
    src = open(os.path.join(ROOT, "include", "artgpu.h")).read()
    for sym in ("artgpu_resize_lanczos", "artgpu_resize_scale", "artgpu_set_pipeline_resize"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, src), sym
        assert sym in capi.EXPORTS and hasattr(capi.LIB, sym) and getattr(capi.LIB, sym).argtypes is not None, sym
    for m in ("resize_lanczos", "resize_scale", "set_pipeline_resize"):
        assert hasattr(capi.Context, m), m
    assert re.search(r"#define\s+ARTGPU_RESIZE_PLANES\s+0\b", src) and re.search(r"#define\s+ARTGPU_RESIZE_RGB\s+1\b", src)
    assert (capi.RESIZE_PLANES, capi.RESIZE_RGB) == (0, 1) == (rs_lib.PLANES, rs_lib.RGB)
    pf = [n for n, _ in capi.ResizeParams._fields_]
    exprs = ["sizeof(artgpu_resize_params)"] + [f"offsetof(artgpu_resize_params, {n})" for n in pf] + ["sizeof(artgpu_pipeline_params)"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "artgpu.h"\nint main(void){' +
                     "".join(f'printf("%zu\\n", (size_t)({e}));' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(capi.ResizeParams)] + [getattr(capi.ResizeParams, n).offset for n in pf] + [C.sizeof(capi.PipelineParams)]
    assert got == want, list(zip(exprs, got, want))
    assert got[0] == 32 and got[1:7] == [0, 4, 8, 16, 20, 24]
    # the checker's structure is the library's
    assert C.sizeof(rs_lib.Params) == C.sizeof(capi.ResizeParams) == rs_lib.checker().rs_ref_sizes(0)
    assert [(n, getattr(rs_lib.Params, n).offset) for n, _ in rs_lib.Params._fields_] == [(n, getattr(capi.ResizeParams, n).offset) for n in pf]
    assert C.sizeof(rs_lib.Counts) == rs_lib.checker().rs_ref_sizes(1)


def test_null_context_calls_return_an_error():
    one = [np.zeros((1, 1), np.float32) for _ in range(3)]
    src, dst = capi.host_rgb(one), capi.host_rgb([a.copy() for a in one])
    assert capi.LIB.artgpu_resize_lanczos(None, C.byref(src), C.byref(dst), C.c_float(0.5), 0, None, None) == -1
    assert capi.LIB.artgpu_resize_lanczos(None, None, None, C.c_float(0.5), 0, None, None) == -1
    assert capi.LIB.artgpu_set_pipeline_resize(None, None) == -1
    p = capi.resize_params(0, scale=0.5)
    assert capi.LIB.artgpu_set_pipeline_resize(None, C.byref(p)) == -1
    imw, imh, sc = C.c_int(), C.c_int(), C.c_float()
    assert capi.LIB.artgpu_resize_scale(C.byref(p), 10, 10, None, C.byref(imh), C.byref(sc)) == -1
    assert capi.LIB.artgpu_resize_scale(None, 10, 12, C.byref(imw), C.byref(imh), C.byref(sc)) == 0 and (imw.value, imh.value, sc.value) == (10, 12, 1.0)


# the scenes of tests/test_gpu_resize.py: (w, h, dw, dh, scale)
def _scene_set():
    out = [(1, 1, 1, 1, 0.7), (3, 2, 1, 1, 0.4)]
    for w, h in ((67, 45), (131, 70)):
        out += [(w, h) + rs_lib.dst_size(w, h, s) + (s,) for s in SCALES[:5]]
    out += [(23, 17) + rs_lib.dst_size(23, 17, s) + (s,) for s in SCALES[5:]]
    w, h, s = 67, 45, 0.5
    dw, dh = rs_lib.dst_size(w, h, s)
    out += [(w, h, dw + 1, dh + 1, s), (w, h, dw + 2, dh + 2, s), (23, 17, 48, 36, 2.0)]
    # At 0.5 the taps reach three destination pixels past the source's edge, so one and two pixels more only cut the ranges.  Four and five
    # more give positions without a tap; at 1/7 float rounding puts a few taps of full ranges into Lanc's zero branch
    out += [(w, h, dw + 4, dh + 4, s), (w, h, dw + 5, dh + 5, s), (67, 45) + rs_lib.dst_size(67, 45, 1 / 7) + (1 / 7,)]
    return out


def test_scenes_take_every_branch():
    """every counter of the checker is non-zero over the scene set: taps cut at each of the four borders, destination rows and columns without
    a tap (they are 0.0f), Lanc's three branches"""
    total = {n: 0 for n in rs_lib.COUNTERS}
    for w, h, dw, dh, s in _scene_set():
        img, want, counts = rs_lib.case(w, h, dw, dh, s)
        for k, v in counts.items():
            total[k] += v
        if counts["empty_cols"]:
            assert all((a[:, -counts["empty_cols"]:] == 0).all() for a in want)
        if counts["empty_rows"]:
            assert all((a[-counts["empty_rows"]:] == 0).all() for a in want)
    print("resize branch counters:", total)
    for n in rs_lib.COUNTERS:
        assert total[n] > 0, n


# -------------------------------------------------------------------------------------------------------------------------------------------
# a float64 model: analytic sin, double sums, one matrix product per direction
# -------------------------------------------------------------------------------------------------------------------------------------------
def _model_matrix(n_src, n_dst, scale):
    scale = float(np.float32(scale))
    delta, sc = 1.0 / scale, min(scale, 1.0)
    M = np.zeros((n_dst, n_src))
    for j in range(n_dst):
        x0 = (j + 0.5) * delta - 0.5
        jj = np.arange(max(0, int(np.floor(x0 - 3.0 / sc)) + 1), min(n_src, int(np.floor(x0 + 3.0 / sc)) + 1))
        if jj.size == 0:
            continue
        z = np.pi * sc * (x0 - jj)
        with np.errstate(all="ignore"):
            v = np.where(np.abs(z) < 1e-9, 1.0, 3.0 * np.sin(z) * np.sin(z / 3.0) / (z * z))
        M[j, jj] = v / v.sum()
    return M


# Largest |checker - model| / (|Mv| |src| |Mh|^T) -- the error relative to the sum of the taps' magnitudes, which is what float rounding of a sum
# with negative lobes is proportional to; relative to the result itself it is unbounded wherever the lobes cancel -- over the NaN-free scenes
# of _scene_set() in the families plain, scaled_frac and dark_offset, measured on the CPU (the test prints the current value).
MODEL_MEASURED = 3.311e-06     # at 131 x 70 -> 48 x 26, scale 0.37, family dark_offset
MODEL_BOUND = 2 * MODEL_MEASURED


def test_float64_model_agrees_with_the_checker():
    """MODEL_MEASURED = 3.311e-06 relative to the taps' magnitudes; asserted at twice that: the margin is for the scenes, not for slack"""
    worst, worst_at = 0.0, None
    for w, h, dw, dh, s in _scene_set():
        Mv, Mh = _model_matrix(h, dh, s), _model_matrix(w, dw, s)
        for fam in ("plain", "scaled_frac", "dark_offset"):
            img, want, _ = rs_lib.case(w, h, dw, dh, s, rs_lib.PLANES, fam)
            for gp, sp in zip(want, img):
                m = Mv @ np.asarray(sp, np.float64) @ Mh.T
                mag = np.abs(Mv) @ np.abs(np.asarray(sp, np.float64)) @ np.abs(Mh).T
                err = np.abs(np.asarray(gp, np.float64) - m)
                assert (err[mag == 0] == 0).all()
                dev = float((err[mag > 0] / mag[mag > 0]).max()) if (mag > 0).any() else 0.0
                if dev > worst:
                    worst, worst_at = dev, (w, h, dw, dh, s, fam)
    print("float64 model: largest deviation %.3e of the taps' magnitudes at %s (bound %.3e)" % (worst, worst_at, MODEL_BOUND))
    assert worst <= MODEL_BOUND
