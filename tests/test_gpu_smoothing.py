"""GPU: artgpu_smoothing / artgpu_set_pipeline_smoothing (ImProcFunctions::guidedSmoothing, ipsmoothing.cc:902-1073, modes GUIDED and NLMEANS)
against the CPU checker (tests/sm_lib.py: tests/emul/smoothing_ref.cc around the oracle's guided filter, NL-means, log forms and YUV forms).

Every pixel and every field of artgpu_smoothing_info is compared as a bit pattern.  The inputs are NaN-free: that is the tool's contract.  The
cases and the branches they take are listed in sm_lib.CASES and checked from the checker's counters in test_smoothing_checker.py."""
import json
import subprocess

import numpy as np
import pytest
import torch

from art_amd import capi, synth
import mk_lib
import oracle_lib as O
import sm_lib
from test_gpu_cli import CLI, MAT, MUL, read_ppm16, run_cli, tone_lut
from test_gpu_pipeline import _lut, _params

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _capi_regions(regions, device_masks, w, h, keep):
    """sm_lib region dicts (mask arrays) -> capi region dicts (Planes); one array used twice becomes one Plane used twice"""
    planes = {}

    def plane(m):
        if m is None:
            return None
        if id(m) not in planes:
            if device_masks:
                mb = torch.full((h, w + 5), float("nan"), dtype=torch.float32, device="cuda:0")
                mb[:, :w].copy_(torch.from_numpy(np.array(m)))
                keep.append(mb)
                planes[id(m)] = capi.device_plane(mb[:, :w])
            else:
                hm = np.array(m, dtype=np.float32)
                keep.append(hm)
                planes[id(m)] = capi.host_plane(hm)
        return planes[id(m)]

    return [dict(r, mask=plane(r.get("mask"))) for r in regions]


def _device_tool(ctx, img, regions, scale=1.0, stride_pad=0, device_masks=False, want_info=True):
    h, w = img[0].shape
    buf = torch.full((3, h, w + stride_pad), float("nan"), dtype=torch.float32, device="cuda:0")
    views = [buf[c, :, :w] for c in range(3)]
    for v, a in zip(views, img):
        v.copy_(torch.from_numpy(np.array(a, dtype=np.float32)))
    keep = []
    info = ctx.smoothing(capi.RGB(*[capi.device_plane(v) for v in views]), _capi_regions(regions, device_masks, w, h, keep), O.REC2020_WS_D, scale,
                         want_info=want_info)
    ctx.synchronize()
    del keep
    if stride_pad:
        assert bool(torch.isnan(buf[:, :, w:]).all()), "wrote past the row"
    return [v.cpu().numpy() for v in views], info


def _host_tool(ctx, img, regions, scale=1.0):
    host = [np.array(a, dtype=np.float32) for a in img]
    h, w = host[0].shape
    keep = []
    ctx.smoothing(capi.host_rgb(host), _capi_regions(regions, False, w, h, keep), O.REC2020_WS_D, scale)
    return host


@pytest.mark.parametrize("name", list(sm_lib.CASES))
def test_planes_and_info_equal_the_checker(gpu_ctx, name):
    """device-resident image (padded rows for STRIDED_CASES) with host masks, or device masks with padded rows (DEVICE_MASK_CASES)"""
    img, regions, scale, want, want_info, _ = sm_lib.case(name)
    got, info = _device_tool(gpu_ctx, img, regions, scale, stride_pad=7 if name in sm_lib.STRIDED_CASES else 0, device_masks=name in sm_lib.DEVICE_MASK_CASES)
    print(f"smoothing {name}: info {[sm_lib.info_fields(i) for i in info]}")
    assert [sm_lib.info_fields(i) for i in info] == [sm_lib.info_fields(i) for i in want_info]
    sm_lib.assert_same(got, want, name)


@pytest.mark.parametrize("name", ["130x97-regions", "67x41-guided-C-r3-it3", "67x41-no-regions"])
def test_host_planes_give_the_same_bits(gpu_ctx, name):
    img, regions, scale, want, _, _ = sm_lib.case(name)
    sm_lib.assert_same(_host_tool(gpu_ctx, img, regions, scale), want, name + " (host planes)")


def test_same_call_twice_same_bits_and_the_scratch_returns(gpu_ctx):
    img, regions, scale, *_ = sm_lib.case("130x97-regions")
    gpu_ctx.trim_scratch()
    base = gpu_ctx.scratch_bytes()
    a, ia = _device_tool(gpu_ctx, img, regions, scale)
    assert gpu_ctx.scratch_bytes() > base
    b, ib = _device_tool(gpu_ctx, img, regions, scale, stride_pad=9, device_masks=True)
    assert [bytes(x) for x in ia] == [bytes(x) for x in ib]
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, b))
    gpu_ctx.trim_scratch()
    assert gpu_ctx.scratch_bytes() == base


def test_one_host_mask_shared_by_two_regions(gpu_ctx):
    """two regions share one host mask and a third has its own: two planes are staged, the shared one is read through two entries; the same
    bits and the same info per region as with three separate device masks"""
    w, h = 67, 41
    img = sm_lib.scene(w, h, seed=12)
    shared, own = sm_lib.mask("between", w, h), sm_lib.mask("corners2", w, h)
    fields = [dict(mode=sm_lib.GUIDED, channel=sm_lib.L, radius=2), dict(mode=sm_lib.GUIDED, channel=sm_lib.CH, radius=1, epsilon=2),
              dict(mode=sm_lib.GUIDED, channel=sm_lib.LC, radius=3)]
    a, ia = _device_tool(gpu_ctx, img, [dict(f, mask=m) for f, m in zip(fields, (shared, shared, own))])
    b, ib = _device_tool(gpu_ctx, img, [dict(f, mask=m) for f, m in zip(fields, (shared.copy(), shared.copy(), own.copy()))], device_masks=True)
    assert len(ia) == len(ib) == 3
    for i, (x, y) in enumerate(zip(ia, ib)):
        assert sm_lib.info_fields(x) == sm_lib.info_fields(y), f"region {i}"
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, b))
    assert any(not np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, img)), "the regions changed nothing"


@pytest.mark.parametrize("name", list(sm_lib.UNSUPPORTED))
def test_unsupported_cases_leave_the_image_alone(gpu_ctx, name):
    w, h, regs = sm_lib.UNSUPPORTED[name]
    big = w > 1000
    img = [np.full((h, w), 1000.0 + c, np.float32) for c in range(3)] if big else sm_lib.scene(w, h, seed=13)
    regions = [dict(r, mask=sm_lib.mask(k, w, h)) for r, k in regs]
    assert sm_lib.smoothing(img, regions) is None
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in img]
    keep = []
    with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
        gpu_ctx.smoothing(capi.RGB(*[capi.device_plane(t) for t in d]), _capi_regions(regions, False, w, h, keep), O.REC2020_WS_D, 1.0, want_info=True)
    gpu_ctx.synchronize()
    assert all(np.array_equal(_bits(t.cpu().numpy()), _bits(a)) for t, a in zip(d, img))
    if not big:
        host = [np.array(a) for a in img]
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
            gpu_ctx.smoothing(capi.host_rgb(host), _capi_regions(regions, True, w, h, keep), O.REC2020_WS_D, 1.0)
        assert all(np.array_equal(_bits(x), _bits(a)) for x, a in zip(host, img))


def test_bad_arguments_are_einval(gpu_ctx):
    img = sm_lib.scene(67, 41, seed=13)
    wrong = np.ones((41, 66), np.float32)
    for regions, scale in (([dict(radius=2, mask=capi.host_plane(wrong))], 1.0), ([dict(mode=9)], 1.0), ([dict(channel=3)], 1.0), ([dict(radius=2)], 0.0)):
        with pytest.raises(capi.ArtGpuError, match=r"^\[-1\]"):
            gpu_ctx.smoothing(capi.host_rgb([np.array(a) for a in img]), regions, O.REC2020_WS_D, scale)
    assert capi.LIB.artgpu_set_pipeline_smoothing(gpu_ctx._h, None, 2, None) == -1
    assert capi.LIB.artgpu_set_pipeline_smoothing(gpu_ctx._h, None, -1, None) == -1


def test_denoise_guided_smoothing_keeps_its_bits(gpu_ctx):
    """artgpu_denoise_guided_smoothing shares the statistics kernels with the tool: one case here, tests/test_gpu_guided.py has the rest"""
    img = sm_lib.scene(130, 97, seed=21)
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in img]
    gpu_ctx.denoise_guided_smoothing(capi.RGB(*[capi.device_plane(t) for t in d]), O.REC2020_WS_D, radius=3, scale=1.0)
    gpu_ctx.synchronize()
    sm_lib.assert_same([t.cpu().numpy() for t in d], O.guided_smoothing(img, radius=3, scale=1.0), "denoise_guided_smoothing")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the per-frame pipe
# ---------------------------------------------------------------------------------------------------------------------------------------
W, H = 392, 296
PIPE_REGIONS = [dict(mode=sm_lib.GUIDED, channel=sm_lib.CH, radius=3, epsilon=1, iterations=2), dict(mode=sm_lib.NLMEANS, channel=sm_lib.L, nlstrength=40, nldetail=60)]
GEN_MASKS = [mk_lib.mask(parametric_enabled=True, hue=mk_lib.HUE_A, chromaticity=mk_lib.CHROMA_A, lightness=mk_lib.LIGHT_A, blur=2.0),
             mk_lib.mask(parametric_enabled=True, lightness=mk_lib.LIGHT_A, inverted=True, opacity=60)]
CC_REGIONS = [dict(mode=capi.CC_RGB, slope=(1.15, 0.9, 1.05), offset=(0.04, -0.3, 0.03), power=(1.2, 0.85, 1.1))]


def _capi_masks(masks):
    return [{k: v for k, v in m.items() if not (k == "area" and v is None)} for m in masks]


def _pipeline(ctx, raw, p):
    h, w = raw.shape
    b = p.border
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    ctx.synchronize()
    return [t.cpu().numpy() for t in d_img]


def _pipe_params():
    """demosaic, getImage, exposure: everything behind the STAGE_2 tools off, so that the frame ahead of the tool is what a run without it returns"""
    p = _params(_lut(), 0)
    p.denoise_enabled = 0
    p.tone_enabled = 0
    return p


def _stages(ctx, frame, cc=None, sm=None, sm_masks=None, tb=None):
    """the tools called one by one on a device copy of `frame`: colour correction (ending in RGB mode), [generate_masks,] smoothing, texture boost"""
    h, w = frame[0].shape
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in frame]
    img = capi.RGB(*[capi.device_plane(t) for t in d])
    keep = []
    if cc is not None:
        ctx.color_correction(img, cc, O.REC2020_WS_D, O.REC2020_IWS_D, True)
    if sm is not None:
        regions = sm
        if sm_masks is not None:
            dL = torch.full((len(sm), h, w), float("nan"), device="cuda:0")
            Lp = [capi.device_plane(dL[i]) for i in range(len(sm))]
            ctx.generate_masks(img, capi.MASKS_MODE_RGB, O.REC2020_WS_D, _capi_masks(sm_masks), full_w=w, full_h=h, scale=1.0, Lmask=Lp)
            regions = [dict(r, mask=Lp[i]) for i, r in enumerate(sm)]
            keep.append(dL)
        ctx.smoothing(img, regions, O.REC2020_WS_D, 1.0)
    if tb is not None:
        ctx.texture_boost(img, tb, O.REC2020_WS_D, 1.0, True, True)
    ctx.synchronize()
    del keep
    return [t.cpu().numpy() for t in d]


def _same(got, want, what):
    assert all(np.isfinite(g).all() for g in got), what
    sm_lib.assert_same(got, want, what)


def test_pipeline_setting_with_caller_planes_set_and_cleared(gpu_ctx):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=41, noise=1500)
    p = _pipe_params()
    plain = _pipeline(gpu_ctx, raw, p)
    w, h = W - 8, H - 8
    m = sm_lib.mask("between", w, h)
    box = np.zeros((h, w), np.float32); box[40:140, 60:200] = 0.8
    regions = [dict(PIPE_REGIONS[0], mask=m), dict(PIPE_REGIONS[1], mask=box)]
    keep = []
    try:
        gpu_ctx.set_pipeline_smoothing(_capi_regions(regions, True, w, h, keep))
        got = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_smoothing(None)
    keep2 = []
    _same(got, _stages(gpu_ctx, plain, sm=_capi_regions(regions, True, w, h, keep2)), "pipe, caller planes")
    assert not np.array_equal(got[1], plain[1])
    again = _pipeline(gpu_ctx, raw, p)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, plain)), "clearing the setting restores the frame"


def test_pipeline_generates_the_masks(gpu_ctx):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=42, noise=1500)
    p = _pipe_params()
    plain = _pipeline(gpu_ctx, raw, p)
    try:
        gpu_ctx.set_pipeline_smoothing(PIPE_REGIONS, _capi_masks(GEN_MASKS))
        got = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_smoothing(None)
    _same(got, _stages(gpu_ctx, plain, sm=PIPE_REGIONS, sm_masks=GEN_MASKS), "pipe, generated masks")
    assert not np.array_equal(got[1], plain[1])


def test_pipeline_with_texture_boost_behind(gpu_ctx):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=43, noise=1500)
    p = _pipe_params()
    plain = _pipeline(gpu_ctx, raw, p)
    arr, keep = capi.texture_boost_regions([(1.0, 0.2, 1, None)])
    p.texture_boost_enabled = 1; p.texture_boost_nregions = 1; p.texture_boost_regions = arr
    tb_only = _pipeline(gpu_ctx, raw, p)
    try:
        gpu_ctx.set_pipeline_smoothing(PIPE_REGIONS[:1])
        got = _pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_smoothing(None)
    _same(got, _stages(gpu_ctx, plain, sm=PIPE_REGIONS[:1], tb=[(1.0, 0.2, 1, None)]), "pipe, texture boost behind")
    assert not np.array_equal(got[1], tb_only[1])
    del keep


def test_pipeline_behind_colour_correction(gpu_ctx):
    """colour correction then ends in RGB mode, also with texture boost behind the two; pipe-generated smoothing masks behind colour
    correction are refused before any stage runs"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=44, noise=1500)
    p = _pipe_params()
    plain = _pipeline(gpu_ctx, raw, p)
    w, h = W - 8, H - 8
    regions = [dict(PIPE_REGIONS[0], mask=sm_lib.mask("between", w, h))]
    keep, keep2 = [], []
    try:
        gpu_ctx.set_pipeline_color_correction(CC_REGIONS)
        gpu_ctx.set_pipeline_smoothing(_capi_regions(regions, True, w, h, keep))
        got = _pipeline(gpu_ctx, raw, p)
        arr, keep3 = capi.texture_boost_regions([(1.0, 0.2, 1, None)])
        p.texture_boost_enabled = 1; p.texture_boost_nregions = 1; p.texture_boost_regions = arr
        got_tb = _pipeline(gpu_ctx, raw, p)
        p.texture_boost_enabled = 0
        gpu_ctx.set_pipeline_smoothing(PIPE_REGIONS, _capi_masks(GEN_MASKS))
        out = [torch.full((h, w), 7.0, device="cuda:0") for _ in range(3)]
        with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
            gpu_ctx.pipeline_run(capi.device_plane(torch.from_numpy(raw).to("cuda:0")), p, capi.RGB(*[capi.device_plane(t) for t in out]))
        gpu_ctx.synchronize()
        assert all(bool((t == 7.0).all()) for t in out), "refused before any stage wrote the output"
    finally:
        gpu_ctx.set_pipeline_smoothing(None)
        gpu_ctx.set_pipeline_color_correction(None)
    sm = _capi_regions(regions, True, w, h, keep2)
    _same(got, _stages(gpu_ctx, plain, cc=CC_REGIONS, sm=sm), "pipe, colour correction ahead")
    _same(got_tb, _stages(gpu_ctx, plain, cc=CC_REGIONS, sm=sm, tb=[(1.0, 0.2, 1, None)]), "pipe, colour correction ahead, texture boost behind")
    del keep3


def test_pipeline_refuses_unsupported_regions_before_any_stage(gpu_ctx):
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=44, noise=1500)
    p = _pipe_params()
    out = [torch.full((H - 8, W - 8), 7.0, device="cuda:0") for _ in range(3)]
    for regions in ([dict(mode=sm_lib.WAVELETS)], [dict(radius=3, iterations=0)], [dict(radius=3), dict(mode=sm_lib.GAUSSIAN, sigma=2.0)]):
        try:
            gpu_ctx.set_pipeline_smoothing(regions)
            with pytest.raises(capi.ArtGpuError, match=r"^\[-4\]"):
                gpu_ctx.pipeline_run(capi.device_plane(torch.from_numpy(raw).to("cuda:0")), p, capi.RGB(*[capi.device_plane(t) for t in out]))
        finally:
            gpu_ctx.set_pipeline_smoothing(None)
        gpu_ctx.synchronize()
        assert all(bool((t == 7.0).all()) for t in out)


def test_batch_of_two_frames_on_two_lanes():
    p = _pipe_params()
    raws = [synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=s, noise=1500) for s in (45, 46)]
    ctx = capi.Context(0)
    plain = [_pipeline(ctx, r, p) for r in raws]
    want = [_stages(ctx, pl, sm=PIPE_REGIONS) for pl in plain]
    ctx.set_batch_lanes(2)
    ctx.set_pipeline_smoothing(PIPE_REGIONS)
    outs = [[np.zeros((H - 8, W - 8), np.float32) for _ in range(3)] for _ in raws]
    ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
    for wnt, o in zip(want, outs):
        _same(o, wnt, "batch lane")
    assert not np.array_equal(outs[0][1], outs[1][1])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# artgpu-cli
# ---------------------------------------------------------------------------------------------------------------------------------------
CLI_FLAG = "guided,c,3,1,2"
CLI_REGION = dict(mode=sm_lib.GUIDED, channel=sm_lib.CH, radius=3, epsilon=1, iterations=2)
CLI_FLAG_NLM = "nlmeans,l,40,60,1"
CLI_REGION_NLM = dict(mode=sm_lib.NLMEANS, channel=sm_lib.L, nlstrength=40, nldetail=60)


def _cli_stages(ctx, raw, regions, convert=True):
    h, w = raw.shape
    b = 4
    d_raw = torch.from_numpy(raw).to("cuda:0")
    dem = [torch.empty((h, w), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    planes = capi.RGB(*[capi.device_plane(t) for t in dem])
    ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), synth.FILTERS_RGGB, 1.0, b, planes)
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    if convert:
        ctx.get_image(planes, b, b, MUL, True, None, img)
        ctx.convert_color_space(img, MAT)
    else:
        ctx.get_image(planes, b, b, MUL, True, MAT, img)
    ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    if regions is not None:
        ctx.smoothing(img, regions, O.REC2020_WS_D, 1.0)
    ctx.tone_curve(img, tone_lut() if convert else _lut(), 1.0, True)
    ctx.synchronize()
    return [t.cpu().numpy() for t in d_img]


def test_cli_smoothing_through_stage_2(gpu_ctx, tmp_path):
    """artgpu-cli --smoothing (ImProcFunctions::process(STAGE_2) -> ImProcFunctions::guidedSmoothing in the C++ mirror, behind colorCorrection)
    equals the same stages called one by one"""
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=42, noise=1200)
    _, without = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3"])
    for flag, region in ((CLI_FLAG, CLI_REGION), (CLI_FLAG_NLM, CLI_REGION_NLM)):
        _, got = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--smoothing", flag])
        assert not np.array_equal(got, without)
        planes = _cli_stages(gpu_ctx, raw, [region])
        want = np.stack([np.rint(np.clip(t, 0, 65535)).astype(np.uint16) for t in planes], axis=-1)
        assert np.array_equal(got, want), flag
    # with a generated mask the result differs from the unmasked one
    _, masked = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", "--smoothing", CLI_FLAG_NLM, "--smoothing-mask", "0.2,0.7"])
    assert not np.array_equal(masked, got) and not np.array_equal(masked, without)


def test_cli_batch_queue_with_smoothing(gpu_ctx, tmp_path):
    w, h, black = W, H, 64.0
    frames = [np.clip(synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=50 + k, noise=1500), 0, 65535).astype(np.uint16) for k in range(2)]
    names = []
    for k, f in enumerate(frames):
        n = tmp_path / f"f{k}.u16"
        f.astype("<u2").tofile(n)
        names.append(str(n))
    res = subprocess.run([CLI, "--batch", ",".join(names), "--width", str(w), "--height", str(h), "--lanes", "2", "--black", str(black),
                          "--expcomp", "0.3", "--smoothing", CLI_FLAG, "--out", str(tmp_path / "o")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    assert json.loads(res.stdout.strip().splitlines()[-1])["frames"] == 2
    for k, f in enumerate(frames):
        raw = np.maximum(f.astype(np.float32) - np.float32(black), np.float32(0.0))          # scaleColors with scale_mul 1
        want = O.get_scanlines(_cli_stages(gpu_ctx, raw, [CLI_REGION], convert=False), 16, False)
        got = read_ppm16(tmp_path / f"o.{k}.ppm")
        assert np.array_equal(got, want), (k, int((got != want).sum()))
        plain = O.get_scanlines(_cli_stages(gpu_ctx, raw, None, convert=False), 16, False)
        assert not np.array_equal(got, plain)
