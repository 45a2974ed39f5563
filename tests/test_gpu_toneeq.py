"""GPU: artgpu_tone_equalizer / artgpu_set_pipeline_tone_equalizer (ImProcFunctions::toneEqualizer, iptoneequalizer.cc:69-371) against the CPU
checker (tests/te_lib.py: tests/emul/toneeq_ref.cc around the oracle's guided filter, sleef forms and LUTf lookups).

Every pixel and every field of artgpu_tone_equalizer_info is compared as a bit pattern.  The inputs are NaN-free: that is the tool's contract.
The cases and the branches they take are listed in te_lib.CASES and checked from the checker's counters in test_toneeq_checker.py."""
import numpy as np
import pytest
import torch

from art_amd import capi, synth
import layout_lib
import oracle_lib as O
import te_lib
from test_gpu_cli import MAT, MUL, run_cli, tone_lut
from test_gpu_pipeline import _lut, _params

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _device_tool(ctx, img, p, scale=1.0):
    d = [torch.from_numpy(np.array(a, dtype=np.float32)).to("cuda:0") for a in img]
    info = ctx.tone_equalizer(capi.RGB(*[capi.device_plane(t) for t in d]), te_lib.capi_params(p), O.REC2020_WS_D, scale, want_info=True)
    ctx.synchronize()
    return [t.cpu().numpy() for t in d], info


@pytest.mark.parametrize("name", list(te_lib.CASES))
def test_planes_and_info_equal_the_checker(gpu_ctx, name):
    """dense device planes, the default form of the group-of-four rule"""
    img, p, scale, want, want_info, _ = te_lib.case(name)
    got, info = _device_tool(gpu_ctx, img, p, scale)
    print(f"tone equalizer {name}: filters {info.filters}, radius {list(info.radius)}, subsampling {list(info.subsampling)}, box radius {list(info.box_radius)}")
    assert te_lib.info_fields(info) == te_lib.info_fields(want_info)
    te_lib.assert_same(got, want, name)


@pytest.mark.parametrize("name", ["3x9-reg0", "37x29-reg0", "64x48-reg0", "67x41-reg0-pivot0-mixed", "67x41-reg1-pivot2.55", "640x45-reg4"])
def test_both_forms_of_the_group_rule_give_the_same_bits(name):
    """one thread per group of four columns (option te_group_thread) and one pixel per lane with the ballot: the same bits as the checker"""
    img, p, scale, want, _, _ = te_lib.case(name)
    ctx = capi.Context(0)
    try:
        for form in (1, 0):
            ctx.set_option("te_group_thread", form)
            got, _ = _device_tool(ctx, img, p, scale)
            te_lib.assert_same(got, want, f"{name}, te_group_thread {form}")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["64x48-reg2", "64x48-reg4", "640x45-reg4", "130x97-scale2-reg3", "724x720-reg4"])
def test_last_filter_upsample_in_its_own_pass_or_in_the_apply_pass(name):
    """the last regularising filter's pointwise pass as gf_finish_plain (option te_fuse_upsample 0) or inside te_apply (the default), in both
    forms of the group rule: the same bits as the checker"""
    img, p, scale, want, _, _ = te_lib.case(name)
    ctx = capi.Context(0)
    try:
        for fuse, form in ((0, 0), (0, 1), (1, 1), (1, 0)):
            ctx.set_option("te_fuse_upsample", fuse)
            ctx.set_option("te_group_thread", form)
            assert (ctx.get_option("te_fuse_upsample"), ctx.get_option("te_group_thread")) == (fuse, form)
            got, _ = _device_tool(ctx, img, p, scale)
            te_lib.assert_same(got, want, f"{name}, te_fuse_upsample {fuse}, te_group_thread {form}")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", te_lib.HOST_CASES)
def test_host_planes_give_the_same_bits(gpu_ctx, name):
    img, p, scale, want, _, _ = te_lib.case(name)
    host = [np.array(a, dtype=np.float32) for a in img]
    gpu_ctx.tone_equalizer(capi.host_rgb(host), te_lib.capi_params(p), O.REC2020_WS_D, scale)
    te_lib.assert_same(host, want, name + " (host planes)")


@pytest.mark.parametrize("layout", list(layout_lib.LAYOUTS))
@pytest.mark.parametrize("name", te_lib.LAYOUT_CASES)
def test_padded_and_shifted_device_planes(gpu_ctx, name, layout):
    """row-padded, offset device planes at widths that are no multiple of 4: the groups are counted from column 0 of the row whatever the
    stride or the start's alignment, and every word outside the window still holds the poison"""
    img, p, scale, want, want_info, _ = te_lib.case(name)
    for form in (0, 1):
        ar = layout_lib.arena(layout_lib.LAYOUTS[layout], img)
        gpu_ctx.set_option("te_group_thread", form)
        try:
            info = gpu_ctx.tone_equalizer(ar.rgb, te_lib.capi_params(p), O.REC2020_WS_D, scale, want_info=True)
        finally:
            gpu_ctx.set_option("te_group_thread", 0)
        gpu_ctx.synchronize()
        assert te_lib.info_fields(info) == te_lib.info_fields(want_info)
        te_lib.assert_same(layout_lib.check(ar, f"{name} {layout}"), want, f"{name}, layout {layout}, te_group_thread {form}")


def test_same_call_twice_same_bits_and_the_scratch_returns(gpu_ctx):
    """the table is uploaded once per band setting and again after the scratch was given back"""
    img, p, scale, want, _, _ = te_lib.case("64x48-reg4")
    gpu_ctx.trim_scratch()
    base = gpu_ctx.scratch_bytes()
    a, _ = _device_tool(gpu_ctx, img, p, scale)
    assert gpu_ctx.scratch_bytes() > base
    b, _ = _device_tool(gpu_ctx, img, p, scale)
    gpu_ctx.trim_scratch()
    assert gpu_ctx.scratch_bytes() == base
    c, _ = _device_tool(gpu_ctx, img, p, scale)
    for got in (a, b, c):
        te_lib.assert_same(got, want, "64x48-reg4 again")
    img2, p2, scale2, want2, _, _ = te_lib.case("67x41-reg0-pivot0-plus100")             # other bands: the table is rebuilt
    te_lib.assert_same(_device_tool(gpu_ctx, img2, p2, scale2)[0], want2, "other bands")


@pytest.mark.parametrize("name", list(te_lib.UNSUPPORTED))
def test_unsupported_cases_leave_the_image_alone(gpu_ctx, name):
    w, h, scale, kw = te_lib.UNSUPPORTED[name]
    img = te_lib.scene(w, h, seed=13)
    p = te_lib.params(**kw)
    assert te_lib.tone_equalizer(img, p, scale=scale) is None
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in img]
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        gpu_ctx.tone_equalizer(capi.RGB(*[capi.device_plane(t) for t in d]), te_lib.capi_params(p), O.REC2020_WS_D, scale, want_info=True)
    gpu_ctx.synchronize()
    assert all(np.array_equal(_bits(t.cpu().numpy()), _bits(a)) for t, a in zip(d, img))
    host = [np.array(a) for a in img]
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        gpu_ctx.tone_equalizer(capi.host_rgb(host), te_lib.capi_params(p), O.REC2020_WS_D, scale)
    assert all(np.array_equal(_bits(x), _bits(a)) for x, a in zip(host, img))


def test_disabled_leaves_the_image_alone_and_one_pixel_runs(gpu_ctx):
    img = te_lib.scene(67, 41, seed=13)
    got, _ = _device_tool(gpu_ctx, img, te_lib.params(te_lib.MIXED, 4, -4.0, enabled=False))
    assert all(np.array_equal(_bits(g), _bits(a)) for g, a in zip(got, img))
    got, _ = _device_tool(gpu_ctx, img, te_lib.params(te_lib.MIXED, 5, -4.0, enabled=False, show_colormap=True))     # nothing is looked at
    assert all(np.array_equal(_bits(g), _bits(a)) for g, a in zip(got, img))
    one = [np.full((1, 1), v, np.float32) for v in (30000.0, 20000.0, 10000.0)]
    p = te_lib.params(te_lib.MIXED, 0, -4.0)
    want, _, _ = te_lib.tone_equalizer(one, p)
    te_lib.assert_same(_device_tool(gpu_ctx, one, p)[0], want, "1 x 1")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the per-frame pipe
# ---------------------------------------------------------------------------------------------------------------------------------------
W, H = 416, 288
PIPE_TE = dict(bands=(40, -25, 10, 60, -80), regularization=4, pivot=-4.0)


def _pipeline(ctx, raw, p):
    h, w = raw.shape
    b = p.border
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    ctx.synchronize()
    return [t.cpu().numpy() for t in d_img]


def _stages(ctx, frame, exposure=False, te=None, sharpen=None):
    """the entry points one by one on a device copy of `frame`, in the pipe's order: exposure, tone equalizer, sharpening"""
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in frame]
    img = capi.RGB(*[capi.device_plane(t) for t in d])
    if exposure:
        ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    if te is not None:
        ctx.tone_equalizer(img, te, O.REC2020_WS_D, 1.0)
    if sharpen is not None:
        ctx.sharpening(img, sharpen, O.REC2020_WS_D, 1.0)
    ctx.synchronize()
    return [t.cpu().numpy() for t in d]


def _same(got, want, what):
    assert all(np.isfinite(g).all() for g in got), what
    te_lib.assert_same(got, want, what)


@pytest.mark.parametrize("sharpen", [False, True])
def test_pipeline_behind_the_denoise_fused_exposure(gpu_ctx, sharpen):
    """the exposure runs inside the denoise tool's last pass; the tool behind it, [the sharpening behind the tool]; NULL turns it off again"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=61, noise=1500)
    p = _params(_lut(), 0)
    p.tone_enabled = 0
    plain = _pipeline(gpu_ctx, raw, p)                                # demosaic, getImage, denoise with the exposure fused in
    sp = capi.sharpening_params(deconvradius=0.9)
    if sharpen:
        p.sharpening_enabled = 1; p.sharpening = sp; p.sharpening_auto_radius = 0
    without = _pipeline(gpu_ctx, raw, p)
    te = capi.tone_equalizer_params(**PIPE_TE)
    try:
        gpu_ctx.set_pipeline_tone_equalizer(te)
        got = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_tone_equalizer(None)
    _same(got, _stages(gpu_ctx, plain, te=te, sharpen=sp if sharpen else None), f"pipe, fused exposure, sharpening {sharpen}")
    assert not np.array_equal(got[1], without[1])
    again = _pipeline(gpu_ctx, raw, p)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, without)), "NULL turns the tool off again"


@pytest.mark.parametrize("sharpen", [False, True])
def test_pipeline_behind_dehaze_and_its_own_exposure(gpu_ctx, sharpen):
    """dehaze sits between the denoise tool and the exposure: the exposure is its own call, the tool follows it"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=62, noise=1500)
    p = _params(_lut(), 0)
    p.tone_enabled = 0; p.denoise_enabled = 0; p.exposure_enabled = 0
    dh, keep_dh = capi.dehaze_params(depth=50)
    p.dehaze_enabled = 1; p.dehaze = dh
    base = _pipeline(gpu_ctx, raw, p)                                 # demosaic, getImage, dehaze
    p.exposure_enabled = 1
    sp = capi.sharpening_params(deconvradius=0.9)
    if sharpen:
        p.sharpening_enabled = 1; p.sharpening = sp; p.sharpening_auto_radius = 0
    te = capi.tone_equalizer_params(bands=(-70, 35, -15, -50, 90), regularization=2, pivot=-4.0)
    try:
        gpu_ctx.set_pipeline_tone_equalizer(te)
        got = _pipeline(gpu_ctx, raw, p)
        # a disabled setting is a setting that does nothing
        off = capi.tone_equalizer_params(bands=(-70, 35, -15, -50, 90), regularization=7, enabled=False)
        gpu_ctx.set_pipeline_tone_equalizer(off)
        untouched = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_tone_equalizer(None)
    _same(got, _stages(gpu_ctx, base, exposure=True, te=te, sharpen=sp if sharpen else None), f"pipe, behind dehaze, sharpening {sharpen}")
    _same(untouched, _stages(gpu_ctx, base, exposure=True, sharpen=sp if sharpen else None), "pipe, enabled == 0")
    del keep_dh


def test_pipeline_refuses_what_the_tool_does_not_support_before_any_stage(gpu_ctx):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=63, noise=1500)
    p = _params(_lut(), 0)
    out = [torch.full((H - 8, W - 8), 7.0, device="cuda:0") for _ in range(3)]
    for kw, scale in ((dict(show_colormap=True), 1.0), (dict(regularization=5), 1.0), (dict(regularization=2), 400.0)):
        p.scale = scale
        try:
            gpu_ctx.set_pipeline_tone_equalizer(capi.tone_equalizer_params(**dict(PIPE_TE, **kw)))
            with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
                gpu_ctx.pipeline_run(capi.device_plane(torch.from_numpy(raw).to("cuda:0")), p, capi.RGB(*[capi.device_plane(t) for t in out]))
        finally:
            gpu_ctx.set_pipeline_tone_equalizer(None)
        gpu_ctx.synchronize()
        assert all(bool((t == 7.0).all()) for t in out)


def test_batch_of_two_frames_on_two_lanes():
    p = _params(_lut(), 0)
    p.tone_enabled = 0
    raws = [synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=s, noise=1500) for s in (64, 65)]
    ctx = capi.Context(0)
    te = capi.tone_equalizer_params(**PIPE_TE)
    plain = [_pipeline(ctx, r, p) for r in raws]
    want = [_stages(ctx, pl, te=te) for pl in plain]
    ctx.set_batch_lanes(2)
    ctx.set_pipeline_tone_equalizer(te)
    outs = [[np.zeros((H - 8, W - 8), np.float32) for _ in range(3)] for _ in raws]
    ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
    for wnt, o in zip(want, outs):
        _same(o, wnt, "batch lane")
    assert not np.array_equal(outs[0][1], outs[1][1])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# artgpu-cli
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_cli_tone_equalizer_through_stage_1(gpu_ctx, tmp_path):
    """artgpu-cli --tone-equalizer (ImProcFunctions::process(STAGE_1) -> ImProcFunctions::toneEqualizer in the C++ mirror, behind exposure) equals the
    same stages called one by one"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=66, noise=1200)
    _, without = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3"])
    _, got = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--tone-equalizer", "40,-25,10,60,-80,3,-4"])
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
    gpu_ctx.tone_equalizer(img, capi.tone_equalizer_params((40, -25, 10, 60, -80), 3, -4.0), O.REC2020_WS_D, 1.0)
    gpu_ctx.tone_curve(img, tone_lut(), 1.0, True)
    gpu_ctx.synchronize()
    want = np.stack([np.rint(np.clip(t.cpu().numpy(), 0, 65535)).astype(np.uint16) for t in d_img], axis=-1)
    assert np.array_equal(got, want)
