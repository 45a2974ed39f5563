"""GPU: artgpu_pipeline_run / artgpu_batch_run chain the same stages as the individual entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as O
from art_amd import capi, synth

pytestmark = pytest.mark.gpu
MUL = (2.1374, 1.0, 1.5918)
MAT = np.array([[0.6325, 0.2312, 0.0921], [0.2198, 0.7712, 0.0090], [0.0166, 0.0713, 0.7514]])


def _lut():
    x = np.arange(65536, dtype=np.float64) / 65535.0
    return ((1.0 - np.cos(np.pi * x ** 0.7)) / 2.0 * 65535.0).astype(np.float32)


def _params(lut, tone_mode, xtrans=False):
    p = capi.PipelineParams()
    p.sensor = 1 if xtrans else 0
    p.bayer_method = capi.BAYER_AMAZE; p.filters = synth.FILTERS_RGGB; p.initial_gain = 1.0
    p.xtrans_passes = 3
    p.xtrans[:] = [int(v) for v in synth.XTRANS_FUJI.reshape(36)]
    p.rgb_cam[:] = [float(v) for v in synth.XTRANS_RGB_CAM.reshape(12)]
    p.border = 7 if xtrans else 4
    p.mul[:] = MUL; p.do_clip = 1; p.has_cam_to_work = 1
    p.cam_to_work[:] = [float(v) for v in MAT.reshape(9)]
    p.ws[:] = [float(v) for v in O.REC2020_WS_D.reshape(9)]
    p.iws[:] = [float(v) for v in O.REC2020_IWS_D.reshape(9)]
    p.denoise_enabled = 1
    p.denoise = capi.DenoiseToolParams(capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0), 0, 3, 0, 80)
    p.exposure_enabled = 1; p.expcomp = 0.3; p.black = 0.0
    p.tone_enabled = 1; p.tone_mode = tone_mode
    p.tone_lut = lut.ctypes.data_as(C.POINTER(C.c_float)); p.white_point = 1.0
    p.to_out[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]; p.to_work[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    p.scale = 1.0
    return p


@pytest.mark.parametrize("tone_mode,xtrans", [(0, False), (1, False), (0, True)])
def test_pipeline_run_equals_stage_by_stage(gpu_ctx, tone_mode, xtrans):
    w, h = 520, 392
    raw = synth.xtrans_frame(w, h, seed=2, noise=2048) if xtrans else synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=2, noise=2048)
    b = 7 if xtrans else 4
    lut = _lut()
    p = _params(lut, tone_mode, xtrans)
    got = [np.zeros((h - 2 * b, w - 2 * b), np.float32) for _ in range(3)]
    gpu_ctx.pipeline_run(capi.host_plane(raw), p, capi.host_rgb(got))
    # the same chain through the individual entry points, frame resident on the device
    d_raw = torch.from_numpy(raw).cuda()
    d_dem = [torch.empty((h, w), dtype=torch.float32, device="cuda") for _ in range(3)]
    dem = capi.RGB(*[capi.device_plane(t) for t in d_dem])
    if xtrans:
        gpu_ctx.demosaic_xtrans(3, True, capi.device_plane(d_raw), synth.XTRANS_FUJI, synth.XTRANS_RGB_CAM, dem)
    else:
        gpu_ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), synth.FILTERS_RGGB, 1.0, 4, dem)
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    gpu_ctx.get_image(dem, b, b, MUL, True, MAT, img)
    curve, _ = capi.noise_curve_lut()
    gpu_ctx.improc_denoise(img, p.denoise, O.REC2020_WS_D, ecomp=0.3, calclum_mat=MAT, noise_c_curve=curve, iws=O.REC2020_IWS_D)
    gpu_ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    if tone_mode == 1:
        gpu_ctx.tone_curve_neutral(img, lut, 1.0, O.REC2020_WS_D, O.REC2020_IWS_D)
    else:
        gpu_ctx.tone_curve(img, lut, 1.0, True)
    gpu_ctx.synchronize()
    for g, t in zip(got, d_img):
        assert np.array_equal(g.view(np.uint32), t.cpu().numpy().view(np.uint32))


def test_batch_run_two_frames(gpu_ctx):
    w, h = 392, 296
    lut = _lut()
    p = _params(lut, 0)
    raws = [synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=s, noise=1500) for s in (5, 6)]
    outs = [[np.zeros((h - 8, w - 8), np.float32) for _ in range(3)] for _ in raws]
    gpu_ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
    for r, o in zip(raws, outs):
        single = [np.zeros((h - 8, w - 8), np.float32) for _ in range(3)]
        gpu_ctx.pipeline_run(capi.host_plane(r), p, capi.host_rgb(single))
        for a, s in zip(o, single):
            assert np.array_equal(a.view(np.uint32), s.view(np.uint32)) and a.max() > 0
    assert not np.array_equal(outs[0][1], outs[1][1])


def test_batch_gives_scratch_back_before_much_smaller_frames():
    """round-5 review, weak point 10: a context's scratch only grows, and a batch that goes on with much smaller frames kept the large frame's
    pools.  artgpu_batch_run trims a lane when this frame and its next one have less than half the pixels the pools were grown for; a batch
    that alternates sizes keeps them.  Same bits either way."""
    lut = _lut()
    p = _params(lut, 0)
    big, small = (1000, 760), (392, 296)

    def frames(sizes, seed0):
        raws = [synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=seed0 + i, noise=1500) for i, (w, h) in enumerate(sizes)]
        outs = [[np.zeros((h - 8, w - 8), np.float32) for _ in range(3)] for (w, h) in sizes]
        return raws, outs
    ctx = capi.Context(0)
    raws, outs = frames([big], 20)
    ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
    held_big = ctx.scratch_bytes()
    # big, small, small: the pools go back before the first small frame
    raws, outs = frames([big, small, small], 30)
    ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
    held_small = ctx.scratch_bytes()
    assert held_small < held_big / 2, (held_small, held_big)
    ref = capi.Context(0)
    for r, o in zip(raws, outs):
        single = [np.zeros_like(o[0]) for _ in range(3)]
        ref.pipeline_run(capi.host_plane(r), p, capi.host_rgb(single))
        for a, s_ in zip(o, single):
            assert np.array_equal(a.view(np.uint32), s_.view(np.uint32))
    # big, small, big, small: alternating sizes keep the pools (no trim: the lane's next frame is large again)
    raws, outs = frames([big, small, big, small], 40)
    ctx.batch_run([capi.host_plane(r) for r in raws[:1]], p, [capi.host_rgb(o) for o in outs[:1]])
    held_big2 = ctx.scratch_bytes()
    assert held_big2 > 2 * held_small
    ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
    assert ctx.scratch_bytes() >= held_big2
    del ctx, ref


def test_pipeline_automatic_chroma_equals_explicit_compute_params(gpu_ctx):
    """chrominance_method AUTOMATIC inside artgpu_pipeline_run = denoiseComputeParams on the demosaiced planes, then the same
    stages with the estimated values (simpleprocess.cc:254-256,311-315)."""
    w, h = 520, 392
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=9, noise=2600)
    lut = _lut()
    p = _params(lut, 0)
    p.denoise.dn.chrominance_method = 1
    p.denoise.dn.chrominance = 0.0
    p.chrominance_auto_factor = 1.5
    got = [np.zeros((h - 8, w - 8), np.float32) for _ in range(3)]
    gpu_ctx.pipeline_run(capi.host_plane(raw), p, capi.host_rgb(got))
    d_raw = torch.from_numpy(raw).cuda()
    d_dem = [torch.empty((h, w), dtype=torch.float32, device="cuda") for _ in range(3)]
    dem = capi.RGB(*[capi.device_plane(t) for t in d_dem])
    gpu_ctx.demosaic_bayer(capi.BAYER_AMAZE, capi.device_plane(d_raw), synth.FILTERS_RGGB, 1.0, 4, dem)
    dn = capi.DenoiseParams(40.0, 50.0, 0, 0.0, 0.0, 0.0, 1.7, 0, 0, 1)
    st = gpu_ctx.denoise_compute_params(dem, 4, MUL, True, MAT, O.REC2020_WS_D, dn, auto_factor=1.5)
    assert st.valid == 1 and dn.chrominance > 0
    # the oracle agrees on the estimate
    ref = O.denoise_compute_params([t.cpu().numpy() for t in d_dem], 4, MUL, True, MAT, O.REC2020_WS_D)
    assert np.float32(st.chrominance) == ref[0][0] and np.float32(st.chrominance_red_green) == ref[0][1]
    d_img = [torch.empty((h - 8, w - 8), dtype=torch.float32, device="cuda") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    gpu_ctx.get_image(dem, 4, 4, MUL, True, MAT, img)
    curve, _ = capi.noise_curve_lut()
    tp = capi.DenoiseToolParams(dn, 0, 3, 0, 80)
    gpu_ctx.improc_denoise(img, tp, O.REC2020_WS_D, ecomp=0.3, calclum_mat=MAT, noise_c_curve=curve, iws=O.REC2020_IWS_D)
    gpu_ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    gpu_ctx.tone_curve(img, lut, 1.0, True)
    gpu_ctx.synchronize()
    for g, t in zip(got, d_img):
        assert np.array_equal(g.view(np.uint32), t.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("lanes", [2, 3])
def test_batch_lanes_give_the_same_bits(lanes):
    """artgpu_set_batch_lanes: frames in flight on sibling contexts / streams / host threads; results identical to one-by-one."""
    w, h = 392, 296
    lut = _lut()
    p = _params(lut, 1)
    seeds = (11, 12, 13, 14, 15)
    raws = [synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=s, noise=1500) for s in seeds]
    ctx = capi.Context(0)
    try:
        ref = [[np.zeros((h - 8, w - 8), np.float32) for _ in range(3)] for _ in raws]
        ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in ref])
        ctx.set_batch_lanes(lanes)
        for _ in range(2):          # twice: the lanes are created once and reused
            outs = [[np.zeros((h - 8, w - 8), np.float32) for _ in range(3)] for _ in raws]
            ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
            for o, r in zip(outs, ref):
                for a, b in zip(o, r):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and a.max() > 0
        # device-resident frames too
        d_raws = [torch.from_numpy(r).cuda() for r in raws]
        d_outs = [[torch.zeros((h - 8, w - 8), dtype=torch.float32, device="cuda") for _ in range(3)] for _ in raws]
        torch.cuda.synchronize()
        ctx.batch_run([capi.device_plane(t) for t in d_raws], p, [capi.RGB(*[capi.device_plane(t) for t in o]) for o in d_outs])
        ctx.synchronize()
        for o, r in zip(d_outs, ref):
            for a, b in zip(o, r):
                assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32))
        with pytest.raises(capi.ArtGpuError):
            ctx.set_batch_lanes(0)
    finally:
        ctx.close()


def test_batch_lanes_inherit_the_context_settings():
    """The lanes are the context as far as the caller can tell: a curve tail above 65535 (artgpu_set_curve_tail) and the options apply to
    every frame whichever lane runs it -- with white_point > 1 and bright frames the output of a lane that missed the setting would differ
    (or the call would fail: the default tail kind refuses white_point > 1)."""
    w, h = 392, 296
    lut = _lut()
    p = _params(lut, 0)
    p.white_point = 1.6
    raws = [np.minimum(synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=s, noise=1500) * np.float32(1.7), np.float32(65535.0)) for s in (21, 22, 23, 24, 25, 26, 27)]
    ctx = capi.Context(0)
    try:
        ctx.set_curve_tail(1, 0.93)
        ctx.set_option("lut_lds", 0)
        ref = [[np.zeros((h - 8, w - 8), np.float32) for _ in range(3)] for _ in raws]
        ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in ref])
        ctx.set_batch_lanes(3)
        outs = [[np.zeros((h - 8, w - 8), np.float32) for _ in range(3)] for _ in raws]
        ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
        for o, r in zip(outs, ref):
            for a, b in zip(o, r):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and a.max() > 0
        # the setting changes between calls: the lanes follow
        ctx.set_curve_tail(2, 1.0)
        ctx.set_batch_lanes(1)
        ref2 = [[np.zeros((h - 8, w - 8), np.float32) for _ in range(3)] for _ in raws]
        ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in ref2])
        ctx.set_batch_lanes(3)
        outs2 = [[np.zeros((h - 8, w - 8), np.float32) for _ in range(3)] for _ in raws]
        ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs2])
        for o, r in zip(outs2, ref2):
            for a, b in zip(o, r):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert any((a != b).any() for o, r in zip(ref, ref2) for a, b in zip(o, r))        # the tail does show in these frames
    finally:
        ctx.close()


def test_batch_complete_over_rccl(gpu_ctx):
    """artgpu_batch_complete: the completion all-gather of a multi-GPU batch over the caller's RCCL communicator.  One GPU here, so the
    communicator has one rank (created through librccl's C API the way a host application would); the two-rank exchange itself is
    RCCL's, the N > 1 bookkeeping of bench.py is covered on CPU by tests/test_multiproc.py."""
    import ctypes as C
    rec = [0, 3, 0, 0x1234567890ABCDEF - (1 << 64) if 0x1234567890ABCDEF >= (1 << 63) else 0x1234567890ABCDEF, 16424, 0, 0, 0]
    assert gpu_ctx.batch_complete(rec) == [rec]                       # no communicator: single rank
    with pytest.raises(capi.ArtGpuError):
        gpu_ctx.batch_complete(rec, nranks=2)                         # two ranks need one
    try:
        rccl = C.CDLL("librccl.so.1")
    except OSError:
        rccl = C.CDLL("/opt/rocm/lib/librccl.so.1")

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_char * 128)]
    uid = UniqueId()
    assert rccl.ncclGetUniqueId(C.byref(uid)) == 0
    comm = C.c_void_p()
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    assert rccl.ncclCommInitRank(C.byref(comm), 1, uid, 0) == 0
    try:
        assert gpu_ctx.batch_complete(rec, nranks=1, rccl_comm=comm) == [rec]
        rec2 = [0, 5, 0, -7, 99, 1, 2, 3]
        assert gpu_ctx.batch_complete(rec2, nranks=1, rccl_comm=comm) == [rec2]
    finally:
        rccl.ncclCommDestroy.argtypes = [C.c_void_p]
        rccl.ncclCommDestroy(comm)


def test_progress_callback_and_roctx_ranges(gpu_ctx):
    """artgpu_set_progress_callback (rtengine::ProgressListener): every stage-level entry point reports (name of the reference function,
    0.0) when it starts and (name, 1.0) when it returns, nested the way the reference's call tree is; with the "roctx" option the same
    names label roctx ranges (must not change any result)."""
    w, h, filt = 330, 270, synth.FILTERS_RGGB
    raw = synth.bayer_frame(w, h, filt, seed=5)
    ref = gpu_ctx.demosaic_bayer_host(capi.BAYER_RCD, raw, filt, 1.0, 4)
    events = []
    gpu_ctx.set_progress_callback(lambda stage, frac: events.append((stage, frac)))
    gpu_ctx.set_option("roctx", 1)
    try:
        got = gpu_ctx.demosaic_bayer_host(capi.BAYER_RCD, raw, filt, 1.0, 4)
    finally:
        gpu_ctx.set_progress_callback(None)
        gpu_ctx.set_option("roctx", 0)
    assert events == [("RawImageSource::demosaic (Bayer)", 0.0), ("RawImageSource::demosaic (Bayer)", 1.0)]
    for a, b in zip(got, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    n = len(events)
    gpu_ctx.demosaic_bayer_host(capi.BAYER_RCD, raw, filt, 1.0, 4)
    assert len(events) == n                                       # removed


def all_tools_pipe_against_the_tools_one_by_one(gpu_ctx, raw):
    """the body of test_pipeline_all_tools_equal_the_tools_one_by_one for a 392 x 296 RGGB frame `raw` (tests/test_gpu_tool_domains.py hands it
    value-domain families)"""
    import lc_lib
    import mk_lib
    import sm_lib
    import tb_lib
    import test_gpu_colorcorrection as CC
    import test_gpu_masks as MK
    import test_gpu_smoothing as SM
    H, W = raw.shape
    w, h = W - 8, H - 8
    WS, IWS = O.REC2020_WS_D, O.REC2020_IWS_D
    lut = _lut()
    p = _params(lut, 0)
    p.denoise_enabled = 0; p.exposure_enabled = 0; p.tone_enabled = 0
    base = SM._pipeline(gpu_ctx, raw, p)                           # demosaic + getImage
    dh, keep_dh = capi.dehaze_params(depth=50)
    sp = capi.sharpening_params(deconvradius=0.9)
    keep = []
    mask = tb_lib.smooth_mask(w, h)
    box = np.zeros((h, w), np.float32); box[40:140, 60:200] = 0.8
    cc = CC._capi_regions([dict(CC.PIPE_REGIONS[0], lmask=mask, abmask=mask), dict(CC.PIPE_REGIONS[1])], True, w, h, keep)
    sm = SM._capi_regions([dict(SM.PIPE_REGIONS[0], mask=sm_lib.mask("between", w, h)), dict(SM.PIPE_REGIONS[1], mask=box)], True, w, h, keep)
    tb_masks, lc_masks = SM._capi_masks(MK.TB_MASKS), SM._capi_masks(MK.LC_MASKS)
    lc_curve = lc_lib.curve_lut(lc_lib.BOOST_CURVE_POINTS)
    tb_arr, keep_tb = capi.texture_boost_regions([r + (None,) for r in MK.TB_REGIONS])
    lc_arr, keep_lc = capi.local_contrast_regions([(60.0, lc_curve, None)])
    p.exposure_enabled = 1; p.tone_enabled = 1
    p.dehaze_enabled = 1; p.dehaze = dh
    p.sharpening_enabled = 1; p.sharpening = sp; p.sharpening_auto_radius = 0
    p.texture_boost_enabled = 1; p.texture_boost_nregions = len(MK.TB_REGIONS); p.texture_boost_regions = tb_arr
    p.local_contrast_enabled = 1; p.local_contrast_nregions = 1; p.local_contrast_regions = lc_arr
    try:
        gpu_ctx.set_pipeline_color_correction(cc)
        gpu_ctx.set_pipeline_smoothing(sm)
        gpu_ctx.set_pipeline_masks(lc_masks, tb_masks)
        got = SM._pipeline(gpu_ctx, raw, p)
    finally:
        gpu_ctx.set_pipeline_masks(None, None)
        gpu_ctx.set_pipeline_smoothing(None)
        gpu_ctx.set_pipeline_color_correction(None)
    d = [torch.from_numpy(np.array(a)).to("cuda:0") for a in base]
    img = capi.RGB(*[capi.device_plane(t) for t in d])
    gpu_ctx.dehaze(img, dh, WS, 1.0)
    gpu_ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0)
    gpu_ctx.sharpening(img, sp, WS, 1.0)
    gpu_ctx.color_correction(img, cc, WS, IWS, True)
    gpu_ctx.smoothing(img, sm, WS, 1.0)
    t_tb, mp = MK._generated(gpu_ctx, img, mk_lib.MODE_RGB, tb_masks, w, h)
    gpu_ctx.texture_boost(img, [r + (m,) for r, m in zip(MK.TB_REGIONS, mp)], WS, 1.0, True, True)
    gpu_ctx.tone_curve(img, lut, 1.0, True)
    gpu_ctx.rgb_to_lab(img, WS)
    t_lc, mp = MK._generated(gpu_ctx, img, mk_lib.MODE_LAB, lc_masks, w, h)
    gpu_ctx.local_contrast(img.g, [(60.0, lc_curve, mp[0])])
    gpu_ctx.lab_to_rgb(img, IWS)
    gpu_ctx.synchronize()
    want = [t.cpu().numpy() for t in d]
    assert all(np.isfinite(g).all() for g in got)
    for name, g, wnt in zip("rgb", got, want):
        nbad = int((g.view(np.uint32) != wnt.view(np.uint32)).sum())
        print(f"all tools, plane {name}: {nbad} values differ")
        assert nbad == 0, (name, nbad)
    assert not np.array_equal(got[1], base[1])
    del keep, keep_dh, keep_tb, keep_lc, t_tb, t_lc


def test_pipeline_all_tools_equal_the_tools_one_by_one(gpu_ctx):
    """Dehaze, sharpening with a fixed radius, colour correction and smoothing (GUIDED and NLMEANS) with caller planes, texture boost with
    pipe-generated masks (legal behind colour correction because smoothing sits in between), the standard tone curve and local contrast with
    pipe-generated masks in ONE frame, against the same tools called through their own entry points, in pipe order, on what a run with all of
    them off returns.  No other test has more than three of them on at once, which is where the walk over the colour modes and the mask slot
    that texture boost and local contrast share can go wrong.  Both sides are this build's kernels in the same order: float32 bit patterns,
    no tolerance."""
    all_tools_pipe_against_the_tools_one_by_one(gpu_ctx, synth.bayer_frame(392, 296, synth.FILTERS_RGGB, seed=71, noise=1500))


def test_batch_lanes_inherit_the_pipe_settings_and_an_option():
    """What a lane inherits is one block of the context: an option (lut_lds 0), a curve tail and the colour-correction and smoothing settings
    of the pipe together.  Five frames on one lane and on three lanes give the same bits, and the settings do show in these frames."""
    import test_gpu_colorcorrection as CC
    import test_gpu_smoothing as SM
    w, h = 392, 296
    lut = _lut()
    p = _params(lut, 0)
    p.denoise_enabled = 0
    p.white_point = 1.6
    raws = [np.minimum(synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=s, noise=1500) * np.float32(1.7), np.float32(65535.0)) for s in (51, 52, 53, 54, 55)]

    def run(ctx):
        outs = [[np.zeros((h - 8, w - 8), np.float32) for _ in range(3)] for _ in raws]
        ctx.batch_run([capi.host_plane(r) for r in raws], p, [capi.host_rgb(o) for o in outs])
        return outs
    ctx = capi.Context(0)
    try:
        ctx.set_option("lut_lds", 0)
        ctx.set_curve_tail(1, 0.93)
        ctx.set_pipeline_color_correction(CC.PIPE_REGIONS[1:])
        ctx.set_pipeline_smoothing(SM.PIPE_REGIONS[:1])
        one = run(ctx)
        ctx.set_batch_lanes(3)
        three = run(ctx)
        for o, r in zip(three, one):
            for a, b in zip(o, r):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and a.max() > 0
        # cleared (the tail: identity -- the default kind refuses white_point > 1): the lanes follow, and the frames differ
        ctx.set_option("lut_lds", 1)
        ctx.set_curve_tail(2, 1.0)
        ctx.set_pipeline_color_correction(None)
        ctx.set_pipeline_smoothing(None)
        cleared = run(ctx)
        ctx.set_batch_lanes(1)
        for o, r in zip(cleared, run(ctx)):
            for a, b in zip(o, r):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert all((o[1] != r[1]).any() for o, r in zip(cleared, one))
    finally:
        ctx.close()


def _progress_frame(kind):
    """(raw, params, image width, image height) of the three frames test_pipeline_progress_sequence walks"""
    lut = _lut()
    if kind == "xtrans-denoise-dehaze":        # the dehaze sits between the tool and the exposure: the exposure runs on its own
        W, H, b = 142, 128, 7
        raw = synth.xtrans_frame(W, H, seed=4, noise=1500)
        p = _params(lut, 0, xtrans=True)
        dh, keep = capi.dehaze_params(depth=50)
        p.dehaze_enabled = 1; p.dehaze = dh
        return raw, p, W - 2 * b, H - 2 * b, (lut, keep)
    W, H, b = 138, 122, 4                       # the image is 130 x 114: a width that is no multiple of 4
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=4, noise=1500)
    p = _params(lut, 1 if kind == "bayer-neutral" else 0)
    p.bayer_method = capi.BAYER_RCD
    if kind == "bayer-neutral":
        p.denoise_enabled = 0
    else:
        p.denoise = capi.DenoiseToolParams(capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 0, 0), 1, 3, 50, 80)
    return raw, p, W - 2 * b, H - 2 * b, (lut,)


def _scope(name):
    return [(name, 0.0), (name, 1.0)]


_FRAME = "ImageProcessor (stage_init .. stage_finish)"
# recorded with the driver that reached these stages through their public entry points
PROGRESS_EVENTS = {
    "bayer-denoise-smoothing-std": [(_FRAME, 0.0)] + _scope("RawImageSource::demosaic (Bayer)") + [("ImProcFunctions::denoise", 0.0)] + _scope("denoise::RGB_denoise")
                                   + _scope("denoise::denoiseGuidedSmoothing") + _scope("denoise::NLMeans") + [("ImProcFunctions::denoise", 1.0)]
                                   + _scope("ImProcFunctions::toneCurve") + [(_FRAME, 1.0)],
    "bayer-neutral": [(_FRAME, 0.0)] + _scope("RawImageSource::demosaic (Bayer)") + _scope("RawImageSource::getImage") + _scope("ImProcFunctions::expcomp")
                     + _scope("ImProcFunctions::toneCurve (NEUTRAL)") + [(_FRAME, 1.0)],
    "xtrans-denoise-dehaze": [(_FRAME, 0.0)] + _scope("RawImageSource::xtrans_interpolate") + [("ImProcFunctions::denoise", 0.0)] + _scope("denoise::RGB_denoise")
                             + [("ImProcFunctions::denoise", 1.0)] + _scope("ImProcFunctions::expcomp") + _scope("ImProcFunctions::toneCurve") + [(_FRAME, 1.0)],
}


@pytest.mark.parametrize("kind", sorted(PROGRESS_EVENTS))
def test_pipeline_progress_sequence(kind):
    """The full (name, fraction) list one artgpu_pipeline_run reports to the progress listener.  The raw stages, the denoise tool with what
    it runs inside, getImage, the exposure and the tone curves report; the tools that came later are silent inside a frame."""
    raw, p, w, h, keep = _progress_frame(kind)
    events = []
    ctx = capi.Context(0)
    try:
        d_raw = torch.from_numpy(raw).cuda()
        d_out = [torch.zeros((h, w), dtype=torch.float32, device="cuda") for _ in range(3)]
        ctx.set_progress_callback(lambda stage, frac: events.append((stage, frac)))
        ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_out]))
        ctx.synchronize()
    finally:
        ctx.set_progress_callback(None)
        ctx.close()
    print(kind, events)
    assert events == PROGRESS_EVENTS[kind]
    assert all(bool(torch.isfinite(t).all()) and float(t.max()) > 0 for t in d_out)
    del keep


def _neutral_null_lut(ctx, img):
    st = capi.NeutralState()
    st.ws[:] = [float(v) for v in O.REC2020_WS_D.reshape(9)]
    st.iws[:] = [float(v) for v in O.REC2020_IWS_D.reshape(9)]
    ctx._chk(capi.LIB.artgpu_tone_curve_neutral(ctx._h, C.byref(img), None, 1.0, C.byref(st)))


def _set(p, **kw):
    for k, v in kw.items():
        obj, names = p, k.split("__")
        for n in names[:-1]:
            obj = getattr(obj, n)
        setattr(obj, names[-1], v)


# name -> (raw size, what the frame's parameters get, the stand-alone call that refuses the same arguments: (ctx, raw plane, demosaiced
# planes of the raw's size, image of the frame's size, lut) -> raises)
REFUSALS = {
    "tone-mode-2": ((72, 68), dict(tone_mode=2), lambda c, raw, dem, img, lut: c.tone_curve(img, lut, 1.0, True, mode=2)),
    "white-point-default-tail": ((72, 68), dict(white_point=1.5), lambda c, raw, dem, img, lut: c.tone_curve(img, lut, 1.5, True)),
    "neutral-null-lut": ((72, 68), dict(tone_mode=1, tone_lut=None), lambda c, raw, dem, img, lut: _neutral_null_lut(c, img)),
    "denoise-color-space-2": ((72, 68), dict(denoise__dn__color_space=2),
                              lambda c, raw, dem, img, lut: c.rgb_denoise(img, capi.DenoiseParams(40.0, 50.0, 0, 15.0, 0.0, 0.0, 1.7, 0, 2, 0), O.REC2020_WS_D)),
    "smoothing-radius-over-scale": ((72, 68), dict(denoise__smoothing_enabled=1, denoise__guided_chroma_radius=1, scale=4.0),
                                    lambda c, raw, dem, img, lut: c.denoise_guided_smoothing(img, O.REC2020_WS_D, 1, 4.0)),
    "bayer-method-99": ((72, 68), dict(bayer_method=99), lambda c, raw, dem, img, lut: c.demosaic_bayer(99, raw, synth.FILTERS_RGGB, 1.0, 4, dem)),
    "initial-gain-0": ((72, 68), dict(initial_gain=0.0), lambda c, raw, dem, img, lut: c.demosaic_bayer(capi.BAYER_AMAZE, raw, synth.FILTERS_RGGB, 0.0, 4, dem)),
    "raw-60x72": ((60, 72), {}, lambda c, raw, dem, img, lut: c.demosaic_bayer(capi.BAYER_AMAZE, raw, synth.FILTERS_RGGB, 1.0, 4, dem)),
    "automatic-chroma-96x96": ((104, 104), dict(denoise__dn__chrominance_method=1),
                               lambda c, raw, dem, img, lut: c.denoise_compute_params(dem, 4, MUL, True, MAT, O.REC2020_WS_D, capi.DenoiseParams(40.0, 50.0, 0, 0.0, 0.0, 0.0, 1.7, 0, 0, 1))),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refused_frame_leaves_output_alone(case):
    """What the demosaicers, denoiseComputeParams, the denoise tool and the tone curves do not support fails the frame before any stage has
    run: the output planes, on the host or on the device, keep every bit, and the message is the stand-alone entry point's."""
    (W, H), changes, standalone = REFUSALS[case]
    b, sentinel = 4, np.float32(-7.25)
    w, h = W - 2 * b, H - 2 * b
    lut = _lut()
    p = _params(lut, 0)
    _set(p, **changes)
    raw = synth.bayer_frame(W, H, synth.FILTERS_RGGB, seed=8, noise=1500)
    ctx = capi.Context(0)
    try:
        d_raw = torch.from_numpy(raw).cuda()
        d_dem = [torch.zeros((H, W), dtype=torch.float32, device="cuda") for _ in range(3)]
        d_img = [torch.full((h, w), 1000.0, dtype=torch.float32, device="cuda") for _ in range(3)]
        with pytest.raises(capi.ArtGpuError) as alone:
            standalone(ctx, capi.device_plane(d_raw), capi.RGB(*[capi.device_plane(t) for t in d_dem]), capi.RGB(*[capi.device_plane(t) for t in d_img]), lut)
        host = [np.full((h, w), sentinel, np.float32) for _ in range(3)]
        dev = [torch.full((h, w), float(sentinel), dtype=torch.float32, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        for where, out in (("host", capi.host_rgb(host)), ("device", capi.RGB(*[capi.device_plane(t) for t in dev]))):
            with pytest.raises(capi.ArtGpuError) as frame:
                ctx.pipeline_run(capi.device_plane(d_raw), p, out)
            ctx.synchronize()
            print(case, where, frame.value)
            assert str(frame.value) == str(alone.value), where
        for a, t in zip(host, dev):
            assert (a.view(np.uint32) == sentinel.view(np.uint32)).all(), "host output written"
            assert (t.cpu().numpy().view(np.uint32) == sentinel.view(np.uint32)).all(), "device output written"
    finally:
        ctx.close()
