"""GPU: the raw CA correction inside the per-frame pipe (artgpu_pipeline_params.ca_enabled / .ca): artgpu_pipeline_run,
artgpu_batch_run and artgpu_batch_run_io give the bits of artgpu_raw_ca_correct followed by the pipe without it, never write the
caller's raw, and leave X-Trans frames alone (the reference skips CA there)."""
import numpy as np
import pytest
import torch

from art_amd import capi, synth
import ca_lib
from test_gpu_pipeline import _lut, _params
from test_gpu_batch_io import BLACK, SCALE, OUTM, _chain, _out_array, _sensor, _trc

pytestmark = pytest.mark.gpu
CA = capi.CaParams(1, 2, 0.0, 0.0, 1)


def _with_ca(p, ca=CA):
    p.ca_enabled = 1
    p.ca = ca
    return p


def _run(ctx, raw, p):
    h, w = raw.shape
    b = p.border
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx.pipeline_run(capi.device_plane(d_raw), p, capi.RGB(*[capi.device_plane(t) for t in d_img]))
    ctx.synchronize()
    return d_raw.cpu().numpy(), [t.cpu().numpy() for t in d_img]


@pytest.mark.parametrize("ca", [CA, capi.CaParams(0, 1, 0.6, -0.4, 0), capi.CaParams(1, 1, 0.0, 0.0, 0)], ids=["auto2", "manual", "auto1"])
def test_pipeline_run_equals_ca_then_pipeline(gpu_ctx, ca):
    lut = _lut()
    raw = ca_lib.lateral_ca_frame(640, 480, synth.FILTERS_RGGB)
    raw_after, got = _run(gpu_ctx, raw, _with_ca(_params(lut, 0), ca))
    assert np.array_equal(raw_after.view(np.uint32), raw.view(np.uint32)), "pipeline_run wrote the caller's raw"
    d = torch.from_numpy(raw).to("cuda:0")
    gpu_ctx.raw_ca_correct(capi.device_plane(d), synth.FILTERS_RGGB, ca)
    corrected = d.cpu().numpy()
    assert not np.array_equal(corrected, raw)
    _, want = _run(gpu_ctx, corrected, _params(lut, 0))
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))


def test_pipeline_ca_disabled_and_below_threshold_is_the_old_pipe(gpu_ctx):
    lut = _lut()
    raw = ca_lib.lateral_ca_frame(640, 480, synth.FILTERS_RGGB)
    _, want = _run(gpu_ctx, raw, _params(lut, 0))
    for p in (_with_ca(_params(lut, 0), capi.CaParams(0, 2, 0.0005, -0.001, 1)), _params(lut, 0)):
        _, got = _run(gpu_ctx, raw, p)
        for g, w in zip(got, want):
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32))


def test_batch_run_host_planes(gpu_ctx):
    lut = _lut()
    p = _with_ca(_params(lut, 0))
    raws = [ca_lib.lateral_ca_frame(640, 480, synth.FILTERS_RGGB, seed=s) for s in (3, 4)]
    b = p.border
    outs = [[np.zeros((480 - 2 * b, 640 - 2 * b), np.float32) for _ in range(3)] for _ in raws]
    copies = [r.copy() for r in raws]
    gpu_ctx.batch_run([capi.host_plane(r) for r in copies], p, [capi.RGB(*[capi.host_plane(a) for a in o]) for o in outs])
    for r, c, o in zip(raws, copies, outs):
        assert np.array_equal(r, c)
        _, want = _run(gpu_ctx, r, p)
        for g, w in zip(o, want):
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32))


def _ca_chain(ctx, sensor, p, b, fmt, matrix, trc):
    """scale_colors -> raw_ca_correct -> pipeline_run (no CA) -> rgb2out_matrix -> get_scanlines"""
    h, w = sensor.shape
    d_cfa = torch.empty((h, w), dtype=torch.float32, device="cuda")
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    chmax = ctx.scale_colors(sensor, synth.FILTERS_RGGB, None, BLACK, SCALE, capi.device_plane(d_cfa))
    ctx.raw_ca_correct(capi.device_plane(d_cfa), synth.FILTERS_RGGB, p.ca)
    q = _params(_LUT, 0)
    ctx.pipeline_run(capi.device_plane(d_cfa), q, img)
    if matrix is not None:
        ctx.rgb2out_matrix(img, img, matrix, trc is None, trc)
    return ctx.get_scanlines(img, fmt[0], fmt[1]), chmax


_LUT = _lut()


@pytest.mark.parametrize("lanes", [1, 2])
def test_batch_run_io_with_ca(gpu_ctx, lanes):
    w, h, b = 640, 480, 4
    p = _with_ca(_params(_LUT, 0))
    trc = _trc()
    fmt = (16, False)
    sensors = [np.clip(ca_lib.lateral_ca_frame(w, h, synth.FILTERS_RGGB, seed=20 + k), 0, 65535).astype(np.uint16) for k in range(3)]
    want = [_ca_chain(gpu_ctx, s, p, b, fmt, OUTM, trc) for s in sensors]
    outs = [_out_array(h, w, b, fmt) for _ in sensors]
    gpu_ctx.set_batch_lanes(lanes)
    try:
        res = gpu_ctx.batch_run_io([capi.sensor_frame(s, BLACK, SCALE) for s in sensors], p,
                                   [capi.scanline_frame(o, OUTM, trc) for o in outs])
    finally:
        gpu_ctx.set_batch_lanes(1)
    plain = _chain(gpu_ctx, sensors[0], _params(_LUT, 0), b, fmt, OUTM, trc)[0]
    assert not np.array_equal(plain.view(np.uint8), want[0][0].view(np.uint8)), "CA changed nothing"
    for k, (o, (scan, chmax)) in enumerate(zip(outs, want)):
        assert res[k].status == 0
        assert [float(v) for v in res[k].chmax] == chmax, k
        assert np.array_equal(o.view(np.uint8), scan.view(np.uint8)), k


def test_xtrans_frame_ignores_ca(gpu_ctx):
    lut = _lut()
    raw = np.clip(synth.xtrans_frame(420, 300, seed=2, noise=1800), 0, 65535).astype(np.float32)
    _, want = _run(gpu_ctx, raw, _params(lut, 0, xtrans=True))
    _, got = _run(gpu_ctx, raw, _with_ca(_params(lut, 0, xtrans=True)))
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
