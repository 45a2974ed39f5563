"""GPU: artgpu_clut_create / artgpu_film_simulation / artgpu_set_pipeline_film_simulation (ImProcFunctions::filmSimulation with a HaldCLUT:
clutstore.cc:178-288, 1063-1112, 1464-1615) against the CPU checker (tests/fs_lib.py: tests/emul/filmsim_ref.cc around the oracle's LUTf lookups).

Every pixel is compared as a bit pattern.  The inputs are NaN-free: that is the tool's contract.  The cases and the branches they take are
listed in fs_lib and checked from the checker's counters in test_filmsim_checker.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from art_amd import capi, synth
import fs_lib
import layout_lib
import lc_lib
from test_gpu_cli import MAT, MUL, run_cli, tone_lut
from test_gpu_pipeline import _lut, _params

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cluts(gpu_ctx):
    """handles by (kind, level, channels), uploaded once and released before the session's context goes"""
    made = {}

    def get(kind, level, channels=3):
        key = (kind, level, channels)
        if key not in made:
            t = fs_lib.clut(kind, level)
            made[key] = gpu_ctx.clut(fs_lib.rgbx(t) if channels == 4 else t, level)
        return made[key]

    yield get
    gpu_ctx.synchronize()
    for h in made.values():
        h.close()


def _device_tool(ctx, img, clut, p):
    d = [torch.from_numpy(np.array(a, dtype=np.float32)).to("cuda:0") for a in img]
    ctx.film_simulation(capi.RGB(*[capi.device_plane(t) for t in d]), clut, fs_lib.capi_params(p))
    ctx.synchronize()
    return [t.cpu().numpy() for t in d]


@pytest.mark.parametrize("level", fs_lib.LEVELS)
@pytest.mark.parametrize("size", fs_lib.SIZES, ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_planes_equal_the_checker(gpu_ctx, cluts, size, level):
    """dense device planes: the three tables x both same_profile values x strengths 1, 0.35 and 0"""
    h, w = size
    for kind, same, strength in fs_lib.combos():
        img, _, p, want, _ = fs_lib.case(h, w, level, kind, same, strength)
        got = _device_tool(gpu_ctx, img, cluts(kind, level), p)
        fs_lib.assert_same(got, want, f"{w}x{h} level {level} {kind} same_profile {same} strength {strength}")


def test_level_144_and_strengths_beyond_one(gpu_ctx, cluts):
    """a level-12 file (144 entries per axis, 24 MB on the device) once; the OVERDRIVE cases, whose blend leaves 0 .. 65535 on both sides, so
    that the inverse table extrapolates"""
    h, w = fs_lib.BIG_SIZE
    for kind, same, strength in (("look", False, 0.35), ("random", True, 1.0), ("identity", True, 1.0)):
        img, _, p, want, _ = fs_lib.case(h, w, fs_lib.BIG_LEVEL, kind, same, strength)
        c = gpu_ctx.clut(fs_lib.clut(kind, fs_lib.BIG_LEVEL), fs_lib.BIG_LEVEL)
        try:
            fs_lib.assert_same(_device_tool(gpu_ctx, img, c, p), want, f"level 144 {kind}")
        finally:
            c.close()
    for args in fs_lib.OVERDRIVE:
        img, _, p, want, counts = fs_lib.case(*args)
        assert counts["igamma_above"] > 0
        fs_lib.assert_same(_device_tool(gpu_ctx, img, cluts(args[3], args[2]), p), want, f"overdrive {args}")


@pytest.mark.parametrize("level", fs_lib.LEVELS)
def test_three_and_four_channels_give_the_same_bits(gpu_ctx, cluts, level):
    for kind, same, strength in (("random", False, 0.35), ("look", True, 1.0)):
        img, _, p, want, _ = fs_lib.case(41, 67, level, kind, same, strength)
        fs_lib.assert_same(_device_tool(gpu_ctx, img, cluts(kind, level, 4), p), want, f"RGBX table, level {level} {kind}")


@pytest.mark.parametrize("size", [(1, 1), (9, 3), (5, 7), (41, 67)], ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_host_planes_give_the_same_bits(gpu_ctx, cluts, size):
    h, w = size
    for kind, same, strength in (("random", False, 0.35), ("look", True, 1.0), ("identity", False, 0.0)):
        img, _, p, want, _ = fs_lib.case(h, w, 9, kind, same, strength)
        host = [np.array(a, dtype=np.float32) for a in img]
        gpu_ctx.film_simulation(capi.host_rgb(host), cluts(kind, 9), fs_lib.capi_params(p))
        fs_lib.assert_same(host, want, f"{w}x{h} {kind} (host planes)")


@pytest.mark.parametrize("layout", list(layout_lib.LAYOUTS))
@pytest.mark.parametrize("size", [(9, 3), (5, 7), (41, 67), (48, 64)], ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_padded_and_shifted_device_planes(gpu_ctx, cluts, size, layout):
    """row-padded, offset device planes: the groups of four are counted from column 0 of the row whatever the stride or the start's
    alignment, and every word outside the window still holds the poison"""
    h, w = size
    for kind, same, strength, level in (("random", False, 0.35, 64), ("look", False, 1.0, 9), ("look", True, 0.35, 4)):
        img, _, p, want, _ = fs_lib.case(h, w, level, kind, same, strength)
        ar = layout_lib.arena(layout_lib.LAYOUTS[layout], img)
        gpu_ctx.film_simulation(ar.rgb, cluts(kind, level), fs_lib.capi_params(p))
        gpu_ctx.synchronize()
        fs_lib.assert_same(layout_lib.check(ar, f"{w}x{h} {layout}"), want, f"{w}x{h} level {level} {kind}, layout {layout}")


def test_bad_levels_handles_and_strengths_are_refused(gpu_ctx, cluts):
    table = np.zeros((8, 3), np.uint16)
    for level in (5, 3, 1, 289):
        with pytest.raises(capi.ArtGpuError, match=r"^\[-1\].*level"):
            gpu_ctx.clut(table, level)
    h = C.c_void_p(1)
    assert capi.LIB.artgpu_clut_create(gpu_ctx._h, table.ctypes.data_as(C.POINTER(C.c_uint16)), 2 * 2, 5, C.byref(h)) == -1 and not h.value
    img, _, p, _, _ = fs_lib.case(41, 67, 9, "look", True, 1.0)
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in img]
    rgb = capi.RGB(*[capi.device_plane(t) for t in d])
    not_a_handle = C.create_string_buffer(64)
    cp = fs_lib.capi_params(p)
    assert capi.LIB.artgpu_film_simulation(gpu_ctx._h, C.byref(rgb), C.cast(not_a_handle, C.c_void_p), C.byref(cp)) == -1
    assert capi.LIB.artgpu_film_simulation(gpu_ctx._h, C.byref(rgb), None, C.byref(cp)) == -1
    assert capi.LIB.artgpu_set_pipeline_film_simulation(gpu_ctx._h, C.cast(not_a_handle, C.c_void_p), C.byref(cp), 0) == -1
    for bad in (float("nan"), float("inf")):
        with pytest.raises(capi.ArtGpuError, match=r"^\[-1\].*strength"):
            gpu_ctx.film_simulation(rgb, cluts("look", 9), capi.film_simulation_params(strength=bad))
    gpu_ctx.synchronize()
    assert all(np.array_equal(_bits(t.cpu().numpy()), _bits(a)) for t, a in zip(d, img))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the per-frame pipe
# ---------------------------------------------------------------------------------------------------------------------------------------
W, H = 416, 288
PIPE_KIND, PIPE_LEVEL = "look", 64


def _pipe_fs():
    p = fs_lib.params(0.35, False)
    return fs_lib.capi_params(p)


def _pipeline(ctx, raw, p):
    h, w = raw.shape
    b = p.border
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    ctx.synchronize()
    return [t.cpu().numpy() for t in d_img]


def _tools(ctx, frame, steps):
    """entry points one by one on a device copy of `frame`: steps is a list of callables taking the RGB image"""
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in frame]
    img = capi.RGB(*[capi.device_plane(t) for t in d])
    for s in steps:
        s(img)
    ctx.synchronize()
    return [t.cpu().numpy() for t in d]


def _same(got, want, what):
    assert all(np.isfinite(g).all() for g in got), what
    fs_lib.assert_same(got, want, what)


def test_pipeline_ahead_of_the_tone_curve_set_and_cleared(gpu_ctx, cluts):
    """pipeline_run with the setting equals the pipe up to texture boost, the tool, the tone curve; NULL turns it off again: the frame is the one
    of a context that never had the setting"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=81, noise=1500)
    lut = _lut()
    p = _params(lut, 0)
    never = _pipeline(gpu_ctx, raw, p)
    p.tone_enabled = 0
    upto = _pipeline(gpu_ctx, raw, p)
    p.tone_enabled = 1
    clut, fp = cluts(PIPE_KIND, PIPE_LEVEL), _pipe_fs()
    try:
        gpu_ctx.set_pipeline_film_simulation(clut, fp, after_tone_curve=False)
        got = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_film_simulation(None)
    want = _tools(gpu_ctx, upto, [lambda i: gpu_ctx.film_simulation(i, clut, fp), lambda i: gpu_ctx.tone_curve(i, lut, 1.0, True)])
    _same(got, want, "pipe, ahead of the tone curve")
    assert not np.array_equal(got[1], never[1])
    again = _pipeline(gpu_ctx, raw, p)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, never)), "NULL turns the tool off again"


def test_pipeline_behind_the_tone_curve_ahead_of_local_contrast(gpu_ctx, cluts):
    """after_tone_curve: the pipe up to and including the tone curve, the tool, local contrast (setMode(LAB), the L plane, back)"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=82, noise=1500)
    lut = _lut()
    p = _params(lut, 0)
    upto = _pipeline(gpu_ctx, raw, p)
    curve = lc_lib.curve_lut(lc_lib.BOOST_CURVE_POINTS)
    lc_arr, keep = capi.local_contrast_regions([(60.0, curve, None)])
    p.local_contrast_enabled = 1; p.local_contrast_nregions = 1; p.local_contrast_regions = lc_arr
    clut, fp = cluts(PIPE_KIND, PIPE_LEVEL), _pipe_fs()
    try:
        gpu_ctx.set_pipeline_film_simulation(clut, fp, after_tone_curve=True)
        got = _pipeline(gpu_ctx, raw, p)
        gpu_ctx.set_pipeline_film_simulation(clut, fp, after_tone_curve=False)
        ahead = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_film_simulation(None)
    ws, iws = [float(v) for v in p.ws], [float(v) for v in p.iws]
    want = _tools(gpu_ctx, upto, [lambda i: gpu_ctx.film_simulation(i, clut, fp), lambda i: gpu_ctx.rgb_to_lab(i, ws),
                                  lambda i: gpu_ctx.local_contrast(i.g, [(60.0, curve, None)], 1.0), lambda i: gpu_ctx.lab_to_rgb(i, iws)])
    _same(got, want, "pipe, behind the tone curve")
    assert not np.array_equal(got[1], ahead[1])
    del keep


def test_a_set_handle_may_be_destroyed_and_another_context_may_use_a_handle(gpu_ctx):
    """the setting keeps its own reference; the handle belongs to the device, not to the context that made it"""
    img, table, p, want, _ = fs_lib.case(41, 67, 9, "look", False, 0.35)
    other = capi.Context(0)
    try:
        c = other.clut(table, 9)
        fs_lib.assert_same(_device_tool(gpu_ctx, img, c, p), want, "a handle made by another context")
        raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=83, noise=1500)
        lut = _lut()
        pp = _params(lut, 0)
        fp = fs_lib.capi_params(p)
        other.set_pipeline_film_simulation(c, fp)
        a = _pipeline(other, raw, pp)
        c.close()                                                     # the caller's reference goes, the setting's stays
        b = _pipeline(other, raw, pp)
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
        other.set_pipeline_film_simulation(None)
        off = _pipeline(other, raw, pp)
        assert not np.array_equal(off[1], a[1])
    finally:
        other.close()


def test_batch_of_two_frames_on_two_lanes():
    lut = _lut()
    p = _params(lut, 0)
    raws = [synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=s, noise=1500) for s in (84, 85)]
    ctx = capi.Context(0)
    try:
        clut, fp = ctx.clut(fs_lib.clut(PIPE_KIND, PIPE_LEVEL), PIPE_LEVEL), _pipe_fs()
        ctx.set_pipeline_film_simulation(clut, fp)
        one = [_pipeline(ctx, r, p) for r in raws]
        ctx.set_batch_lanes(2)
        outs = [[np.zeros((H - 8, W - 8), np.float32) for _ in range(3)] for _ in raws]
        ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
        for wnt, o in zip(one, outs):
            _same(o, wnt, "batch lane")
        assert not np.array_equal(outs[0][1], outs[1][1])
        ctx.set_pipeline_film_simulation(None)
        off = _pipeline(ctx, raws[0], p)
        assert not np.array_equal(off[1], one[0][1])
        clut.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# artgpu-cli
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_cli_film_simulation_through_stage_3(gpu_ctx, cluts, tmp_path):
    """artgpu-cli --film-simulation (ImProcFunctions::process(STAGE_3) -> ImProcFunctions::filmSimulation in the C++ mirror, behind the tone
    curve with the fourth value set) equals the same stages called one by one"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=86, noise=1200)
    path = tmp_path / "look.u16"
    fs_lib.clut("look", 9).astype("<u2").tofile(path)
    _, without = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3"])
    _, got = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--film-simulation", f"{path},9,35,1"])
    assert not np.array_equal(got, without)
    h, w = raw.shape
    b = 4
    d_raw = torch.from_numpy(raw).to("cuda:0")
    dem = [torch.empty((h, w), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    planes = capi.RGB(*[capi.device_plane(t) for t in dem])
    gpu_ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), synth.FILTERS_RGGB, 1.0, b, planes)
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    gpu_ctx.get_image(planes, b, b, MUL, True, None, img)
    gpu_ctx.convert_color_space(img, MAT)
    gpu_ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    gpu_ctx.tone_curve(img, tone_lut(), 1.0, True)
    gpu_ctx.film_simulation(img, cluts("look", 9), capi.film_simulation_params(strength=float(np.float32(35) / np.float32(100))))
    gpu_ctx.synchronize()
    want = np.stack([np.rint(np.clip(t.cpu().numpy(), 0, 65535)).astype(np.uint16) for t in d_img], axis=-1)
    assert np.array_equal(got, want)
