"""GPU: artgpu_batch_run_io (sensor data in, writers' scanlines out, a frame's copies beside its neighbours' kernels) returns the bits of the
chain it stands for -- artgpu_scale_colors -> artgpu_pipeline_run -> artgpu_rgb2out_matrix -> artgpu_get_scanlines, one frame after the
other -- whatever the number of lanes, the scanline format, the residency of the buffers (the same for a whole batch or another for every
frame) and the mix of frame sizes; and after a batch that failed, every frame's status says whether that frame can be used."""
import ctypes as C

import numpy as np
import pytest
import torch

from art_amd import capi, synth
from test_gpu_pipeline import _lut, _params

pytestmark = pytest.mark.gpu
BLACK = (64.0, 60.0, 68.0, 62.0)
SCALE = (1.02, 1.0, 0.98, 1.01)
OUTM = np.array([[0.90, 0.06, 0.04], [0.05, 0.90, 0.05], [0.03, 0.07, 0.90]], np.float32)
EINVAL, EUNSUPPORTED = -1, -4       # ARTGPU_EINVAL, ARTGPU_EUNSUPPORTED (include/artgpu.h)
PATTERN16 = 0xA5A5                  # what the tests of refused frames fill the scanline buffers with


def _sensor(w, h, seed, xtrans=False):
    f = synth.xtrans_frame(w, h, seed=seed, noise=1800) if xtrans else synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=seed, noise=1800)
    return np.clip(f, 0, 65535).astype(np.uint16)


def _trc(n=4096):
    x = np.arange(n, dtype=np.float64) / (n - 1)
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * x ** (1 / 2.4) - 0.055).astype(np.float32)


def _chain(ctx, sensor, p, b, fmt, matrix, trc, xtrans=False):
    """one frame through the four entry points, everything in between resident on the device"""
    h, w = sensor.shape
    d_cfa = torch.empty((h, w), dtype=torch.float32, device="cuda")
    d_img = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda") for _ in range(3)]
    img = capi.RGB(*[capi.device_plane(t) for t in d_img])
    chmax = ctx.scale_colors(sensor, synth.FILTERS_RGGB, synth.XTRANS_FUJI if xtrans else None, BLACK, SCALE, capi.device_plane(d_cfa))
    ctx.pipeline_run(capi.device_plane(d_cfa), p, img)
    if matrix is not None:
        ctx.rgb2out_matrix(img, img, matrix, trc is None, trc)
    bps, is_float = fmt
    return ctx.get_scanlines(img, bps, is_float), chmax


def _out_array(h, w, b, fmt):
    bps, is_float = fmt
    dt = np.float32 if bps == 32 else (np.uint8 if bps == 8 else np.uint16)
    return np.zeros((h - 2 * b, w - 2 * b, 3), dt)


@pytest.mark.parametrize("lanes", [1, 2, 3])
@pytest.mark.parametrize("fmt,use_matrix,use_trc", [((16, False), True, True), ((8, False), True, False), ((32, True), False, False), ((16, True), True, False)])
def test_batch_run_io_same_bits_as_the_four_calls(gpu_ctx, lanes, fmt, use_matrix, use_trc):
    w, h, b = 520, 392, 4
    lut = _lut()
    p = _params(lut, 0)
    trc = _trc() if use_trc else None
    matrix = OUTM if use_matrix else None
    sensors = [_sensor(w, h, 11 + k) for k in range(5)]
    want = [_chain(gpu_ctx, s, p, b, fmt, matrix, trc) for s in sensors]
    outs = [_out_array(h, w, b, fmt) for _ in sensors]
    gpu_ctx.set_batch_lanes(lanes)
    try:
        res = gpu_ctx.batch_run_io([capi.sensor_frame(s, BLACK, SCALE) for s in sensors], p,
                                   [capi.scanline_frame(o, matrix, trc, is_float=fmt[1]) for o in outs])
    finally:
        gpu_ctx.set_batch_lanes(1)
    for k, (o, (scan, chmax)) in enumerate(zip(outs, want)):
        assert res[k].status == 0
        assert [float(v) for v in res[k].chmax] == chmax, k
        assert np.array_equal(o.view(np.uint8), scan.view(np.uint8)), k


def test_batch_run_io_frames_of_different_sizes_and_a_repeat(gpu_ctx):
    """the staging slots are regrown between frames while other frames' copies are in flight; a second batch on the same context reuses them"""
    b = 4
    lut = _lut()
    p = _params(lut, 0)
    sizes = [(392, 296), (648, 488), (392, 296), (520, 392), (648, 488), (264, 200)]
    sensors = [_sensor(w, h, 30 + k) for k, (w, h) in enumerate(sizes)]
    fmt = (16, False)
    want = [_chain(gpu_ctx, s, p, b, fmt, OUTM, None) for s in sensors]
    gpu_ctx.set_batch_lanes(2)
    try:
        for rep in range(2):
            outs = [_out_array(s.shape[0], s.shape[1], b, fmt) for s in sensors]
            ins = list(sensors)
            if rep:       # pitched buffers on both sides of every other frame (rows of a larger allocation)
                for k in range(0, len(sensors), 2):
                    hh, ww = sensors[k].shape
                    wide = np.zeros((hh, ww + 9), np.uint16); wide[:, :ww] = sensors[k]; ins[k] = wide[:, :ww]
                    outs[k] = np.zeros((hh - 2 * b, ww - 2 * b + 5, 3), np.uint16)[:, :ww - 2 * b, :]
            gpu_ctx.batch_run_io([capi.sensor_frame(s, BLACK, SCALE) for s in ins], p, [capi.scanline_frame(o, OUTM) for o in outs])
            for k, (o, (scan, _)) in enumerate(zip(outs, want)):
                assert np.array_equal(o, scan), k
    finally:
        gpu_ctx.set_batch_lanes(1)


def test_batch_run_io_device_buffers_and_pinned_host_buffers(gpu_ctx):
    w, h, b = 520, 392, 4
    lut = _lut()
    p = _params(lut, 0)
    fmt = (16, False)
    sensors = [_sensor(w, h, 50 + k) for k in range(4)]
    want = [_chain(gpu_ctx, s, p, b, fmt, OUTM, None)[0] for s in sensors]
    # pinned host memory on both sides
    pin_in = [torch.from_numpy(s.view(np.int16)).pin_memory() for s in sensors]
    pin_out = [torch.zeros((h - 2 * b, w - 2 * b, 3), dtype=torch.int16).pin_memory() for _ in sensors]
    gpu_ctx.set_batch_lanes(2)
    try:
        # (pinned scanline buffers: written by the download stream's own kernel, option io_direct workgroups; 0: staged and copied by the runtime)
        for direct in (32, 3, 0):
            gpu_ctx.set_option("io_direct", direct)
            for t in pin_out:
                t.zero_()
            gpu_ctx.batch_run_io([capi.sensor_frame(t.numpy().view(np.uint16), BLACK, SCALE) for t in pin_in], p,
                                 [capi.scanline_frame(t.numpy().view(np.uint16), OUTM) for t in pin_out])
            for t, scan in zip(pin_out, want):
                assert np.array_equal(t.numpy().view(np.uint16), scan), direct
        gpu_ctx.set_option("io_direct", -1)
        # device memory on both sides: no copies at all
        d_in = [t.cuda() for t in pin_in]
        d_out = [torch.zeros((h - 2 * b, w - 2 * b, 3), dtype=torch.int16, device="cuda") for _ in sensors]
        torch.cuda.synchronize()
        ins = []
        outs = []
        for t, o in zip(d_in, d_out):
            f = capi.SensorFrame(t.data_ptr(), w, h, w * 2, 1, 1, (C.c_float * 4)(*BLACK), (C.c_float * 4)(*SCALE))
            ins.append(f)
            g = capi.scanline_frame(np.zeros((1, 1, 3), np.uint16), OUTM)
            g.scanlines = o.data_ptr(); g.row_stride_bytes = (w - 2 * b) * 6; g.on_device = 1
            outs.append(g)
        gpu_ctx.batch_run_io(ins, p, outs)
        for o, scan in zip(d_out, want):
            assert np.array_equal(o.cpu().numpy().view(np.uint16), scan)
    finally:
        gpu_ctx.set_batch_lanes(1)


@pytest.mark.parametrize("fmt", [(8, False), (16, True), (32, True)])
@pytest.mark.parametrize("w,h", [(520, 392), (1100, 264)])
def test_batch_run_io_pinned_scanlines_every_format(gpu_ctx, fmt, w, h):
    """the direct-to-host kernel: rows whose byte length is no multiple of 16, chunks shorter than 512 pixels, padded row strides"""
    b = 4
    lut = _lut()
    p = _params(lut, 0)
    sensors = [_sensor(w, h, 60 + k) for k in range(3)]
    want = [_chain(gpu_ctx, s, p, b, fmt, OUTM, None)[0] for s in sensors]
    bps = fmt[0]
    iw, ih = w - 2 * b, h - 2 * b
    pitch = ((iw * 3 * (bps // 8) + 15) // 16) * 16 + 32           # 16-byte aligned rows, padded
    pins = [torch.zeros((ih, pitch), dtype=torch.uint8).pin_memory() for _ in sensors]
    frames = []
    for t in pins:
        f = capi.scanline_frame(np.zeros((1, 1, 3), np.float32 if bps == 32 else (np.uint8 if bps == 8 else np.uint16)), OUTM, is_float=fmt[1])
        f.scanlines = t.data_ptr(); f.row_stride_bytes = pitch
        frames.append(f)
    gpu_ctx.set_batch_lanes(2)
    gpu_ctx.set_option("io_direct", 5)
    try:
        gpu_ctx.batch_run_io([capi.sensor_frame(s, BLACK, SCALE) for s in sensors], p, frames)
    finally:
        gpu_ctx.set_batch_lanes(1)
        gpu_ctx.set_option("io_direct", -1)
    for t, scan in zip(pins, want):
        got = t.numpy()[:, :iw * 3 * (bps // 8)]
        assert np.array_equal(got, scan.reshape(ih, -1).view(np.uint8))
        assert not t.numpy()[:, iw * 3 * (bps // 8):].any()        # the padding stays untouched


def test_batch_run_io_xtrans(gpu_ctx):
    w, h, b = 520, 392, 7
    lut = _lut()
    p = _params(lut, 0, xtrans=True)
    fmt = (16, False)
    sensors = [_sensor(w, h, 70 + k, xtrans=True) for k in range(3)]
    want = [_chain(gpu_ctx, s, p, b, fmt, OUTM, None, xtrans=True)[0] for s in sensors]
    outs = [_out_array(h, w, b, fmt) for _ in sensors]
    gpu_ctx.set_batch_lanes(2)
    try:
        gpu_ctx.batch_run_io([capi.sensor_frame(s, BLACK, SCALE) for s in sensors], p, [capi.scanline_frame(o, OUTM) for o in outs])
    finally:
        gpu_ctx.set_batch_lanes(1)
    for o, scan in zip(outs, want):
        assert np.array_equal(o, scan)


def test_batch_run_io_reports_what_rgb2out_cannot_do_and_bad_arguments(gpu_ctx):
    w, h, b = 392, 296, 4
    lut = _lut()
    p = _params(lut, 0)
    sensors = [_sensor(w, h, 90 + k) for k in range(2)]
    outs = [_out_array(h, w, b, (16, False)) for _ in sensors]
    trc = _trc()
    ins = (capi.SensorFrame * 2)(*[capi.sensor_frame(s, BLACK, SCALE) for s in sensors])
    # values above 1 behind a matrix that amplifies, with a non-linear TRC: the frame says so, the call returns the code
    big = 3.0 * np.eye(3, dtype=np.float32)
    fr = (capi.ScanlineFrame * 2)(capi.scanline_frame(outs[0], OUTM, trc), capi.scanline_frame(outs[1], big, trc))
    rc = capi.LIB.artgpu_batch_run_io(gpu_ctx._h, 2, ins, C.byref(p), fr)
    assert rc == -4      # ARTGPU_EUNSUPPORTED
    assert fr[0].status == 0 and fr[1].status == rc
    assert b"ARTOutputProfile::eval" in capi.LIB.artgpu_last_error(gpu_ctx._h)
    want0 = _chain(gpu_ctx, sensors[0], p, b, (16, False), OUTM, trc)[0]
    assert np.array_equal(outs[0], want0)
    # arguments: the call says what was wrong, and every frame says whether it can be used (frame 0 ran to its end before frame 1 was refused)
    want_lin = _chain(gpu_ctx, sensors[0], p, b, (16, False), OUTM, None)
    bad = (capi.ScanlineFrame * 2)(capi.scanline_frame(outs[0], OUTM), capi.scanline_frame(outs[1], OUTM))
    for field, value, restore in (("bps", 12, 16), ("row_stride_bytes", 10, bad[1].row_stride_bytes)):
        setattr(bad[1], field, value)
        outs[0][:] = PATTERN16; outs[1][:] = PATTERN16
        assert capi.LIB.artgpu_batch_run_io(gpu_ctx._h, 2, ins, C.byref(p), bad) == EINVAL, field
        assert bad[0].status == 0 and [float(v) for v in bad[0].chmax] == want_lin[1], field
        assert np.array_equal(outs[0], want_lin[0]), field
        assert bad[1].status == EINVAL and [float(v) for v in bad[1].chmax] == [0.0] * 4, field
        assert (outs[1] == PATTERN16).all(), field
        setattr(bad[1], field, restore)
    assert capi.LIB.artgpu_batch_run_io(gpu_ctx._h, 2, None, C.byref(p), bad) != 0
    assert capi.LIB.artgpu_batch_run_io(gpu_ctx._h, 0, None, None, None) == 0
    # the context is usable afterwards
    ok = (capi.ScanlineFrame * 2)(capi.scanline_frame(outs[0], OUTM, trc), capi.scanline_frame(outs[1], OUTM, trc))
    assert capi.LIB.artgpu_batch_run_io(gpu_ctx._h, 2, ins, C.byref(p), ok) == 0
    assert np.array_equal(outs[0], want0)


# ---------------------------------------------------------------------------------------------
# frames of different residency in one batch; what a frame's status says after a lane has failed
# ---------------------------------------------------------------------------------------------

_WANT = {}
_TONE_LUT = _lut()       # (PipelineParams only points at its tone table: the array has to outlive every call that uses the parameters)


def _pipe_params():
    return _params(_TONE_LUT, 0)



def _wanted(ctx, sizes, seed0, matrix=OUTM, trc=None, b=4):
    """the sensors of one case and what the four calls make of them: (scanlines, chmax) per frame, computed once per session and left unchanged"""
    key = (tuple(sizes), seed0, trc is not None)
    if key not in _WANT:
        sensors = [_sensor(w, h, seed0 + k) for k, (w, h) in enumerate(sizes)]
        for s in sensors:
            s.setflags(write=False)
        want = [_chain(ctx, s, _pipe_params(), b, (16, False), matrix, trc) for s in sensors]
        for scan, _ in want:
            scan.setflags(write=False)
        _WANT[key] = (sensors, want)
    return _WANT[key]


class _Frame:
    """one frame's buffers of the given residency -- input: device / pinned / pageable; output: device / pinned / pinned-unaligned / pageable --
    as 16-bit scanlines, every output byte (and eight bytes either side of it) pre-filled with 0xA5"""

    def __init__(self, sensor, kin, kout, b=4):
        h, w = sensor.shape
        self.ih, self.iw = h - 2 * b, w - 2 * b
        if kin == "device":
            self.src = torch.from_numpy(sensor.view(np.int16).copy()).cuda()
            self.inp = capi.SensorFrame(self.src.data_ptr(), w, h, w * 2, 1, 1, (C.c_float * 4)(*BLACK), (C.c_float * 4)(*SCALE))
        else:
            self.src = torch.from_numpy(sensor.view(np.int16).copy())
            if kin == "pinned":
                self.src = self.src.pin_memory()
            self.inp = capi.sensor_frame(self.src.numpy().view(np.uint16), BLACK, SCALE)
        n = self.ih * self.iw * 6
        self.dst = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device="cuda" if kout == "device" else "cpu")
        if kout.startswith("pinned"):
            self.dst = self.dst.pin_memory()
        assert self.dst.data_ptr() % 16 == 0
        # the scanlines start 16 bytes into the allocation, or 8: rows that are not 16-byte aligned cannot be written by the download
        # stream's kernel and are staged and copied whatever io_direct says (io_frame: host_dev)
        self.off = 8 if kout == "pinned-unaligned" else 0
        self.out = capi.scanline_frame(np.zeros((1, 1, 3), np.uint16), OUTM)
        self.out.scanlines = self.dst.data_ptr() + self.off
        self.out.row_stride_bytes = self.iw * 6
        self.out.on_device = 1 if kout == "device" else 0

    def raw(self):
        return self.dst.cpu().numpy()

    def scanlines(self):
        return self.raw()[self.off:self.off + self.ih * self.iw * 6].view(np.uint16).reshape(self.ih, self.iw, 3)

    def untouched(self):
        return bool((self.raw() == 0xA5).all())

    def margins_untouched(self):
        raw = self.raw()
        return bool((raw[:self.off] == 0xA5).all() and (raw[self.off + self.ih * self.iw * 6:] == 0xA5).all())


# (input, output) by turn, one row per lane.  Turns i - 2 and i share a staging slot and a working image; "P>" is a pinned buffer the
# download stream's kernel may write directly, "P~" a pinned buffer whose rows are not 16-byte aligned (always staged and copied).
_D, _P, _U, _G = "device", "pinned", "pinned-unaligned", "pageable"
MIXED = {
    # one lane, eight turns.  Outputs, slot 0: direct -> device -> direct (both orders) -> pageable; slot 1: staged -> device -> pageable ->
    # direct.  Inputs, slot 0: pinned, device, pinned (a device input between pinned ones), pageable; turn by turn the same around turn 2
    1: [[(_P, _P), (_P, _U), (_D, _D), (_P, _D), (_P, _P), (_G, _G), (_G, _G), (_D, _P)]],
    # two lanes, four turns each (two pairs per lane, so the sequences are spread over the lanes).  Lane 0: direct -> device and staged ->
    # device, a device input between pinned ones.  Lane 1: device -> direct and pageable -> direct, a pageable input first
    2: [[(_P, _P), (_D, _U), (_P, _D), (_G, _D)],
        [(_G, _D), (_P, _G), (_D, _P), (_P, _P)]],
}


@pytest.mark.parametrize("io_direct", [3, 0])
@pytest.mark.parametrize("lanes", [1, 2])
def test_batch_run_io_mixed_residency_same_bits_as_the_four_calls(gpu_ctx, lanes, io_direct):
    """Frames of every residency in ONE batch, laid out so that each lane sees, two turns apart (same staging slot, same working image): a
    direct download then a device output, the reverse, a staged download then a device output, pageable buffers before and after the
    others; and a device input between pinned ones.  With io_direct = 0 every pinned download is staged.

    What this shows: for every kind of frame, beside every other kind, the right slot, stream and buffer are picked -- a wrong slot, a
    copy left out or a copy to the wrong place gives other bytes (the frames differ) or leaves the 0xA5 fill.  What it cannot show: the
    ORDER between the download of turn i - 2 and the kernels of turn i.  A frame of this size is read in microseconds, a missing wait
    would all but never flip a bit here; tests/test_batch_io_schedule.py is the argument for the ordering (it found the wait io_frame used
    to leave out in front of device outputs)."""
    w, h, b = 520, 392, 4
    sensors, want = _wanted(gpu_ctx, [(w, h)] * 8, 140)
    p = _pipe_params()
    kinds = [MIXED[lanes][f % lanes][f // lanes] for f in range(8)]
    outk = [[k[1] for k in lane] for lane in MIXED[lanes]]
    pairs = {(lane[i - 2], lane[i]) for lane in outk for i in range(2, len(lane))}
    assert {(_P, _D), (_D, _P), (_U, _D)} <= pairs and any(_G in pr for pr in pairs)      # the layout is what the docstring says
    assert any(lane[i - 1][0] == _P and lane[i][0] == _D and lane[i + 1][0] == _P for lane in MIXED[lanes] for i in range(1, len(lane) - 1))
    frames = [_Frame(s, kin, kout, b) for s, (kin, kout) in zip(sensors, kinds)]
    torch.cuda.synchronize()
    gpu_ctx.set_batch_lanes(lanes)
    gpu_ctx.set_option("io_direct", io_direct)
    try:
        res = gpu_ctx.batch_run_io([f.inp for f in frames], p, [f.out for f in frames])
    finally:
        gpu_ctx.set_batch_lanes(1)
        gpu_ctx.set_option("io_direct", -1)
    for k, (f, (scan, chmax)) in enumerate(zip(frames, want)):
        assert res[k].status == 0, (k, kinds[k])
        assert [float(v) for v in res[k].chmax] == chmax, (k, kinds[k])
        assert np.array_equal(f.scanlines(), scan), (k, kinds[k])
        assert f.margins_untouched(), (k, kinds[k])


def test_batch_run_io_pinned_direct_download_with_frames_of_different_sizes(gpu_ctx):
    """the working images and the upload slots are regrown between frames while the download stream's kernel still reads the other set"""
    sizes = [(392, 296), (648, 488), (392, 296), (520, 392), (648, 488), (264, 200)]
    sensors, want = _wanted(gpu_ctx, sizes, 30)
    p = _pipe_params()
    gpu_ctx.set_batch_lanes(2)
    gpu_ctx.set_option("io_direct", 5)
    try:
        for rep in range(2):
            frames = [_Frame(s, _P, _P) for s in sensors]
            res = gpu_ctx.batch_run_io([f.inp for f in frames], p, [f.out for f in frames])
            for k, (f, (scan, chmax)) in enumerate(zip(frames, want)):
                assert res[k].status == 0 and [float(v) for v in res[k].chmax] == chmax, (rep, k)
                assert np.array_equal(f.scanlines(), scan), (rep, k)
                assert f.margins_untouched(), (rep, k)
    finally:
        gpu_ctx.set_batch_lanes(1)
        gpu_ctx.set_option("io_direct", -1)


STATUS_SIZES = [(392, 296)] * 5


def _status_batch(ctx, lanes, frames, p):
    ctx.set_batch_lanes(lanes)
    try:
        return ctx.batch_run_io([f.inp for f in frames], p, [f.out for f in frames], check=False)
    finally:
        ctx.set_batch_lanes(1)


def _complete(res, frame, want_k):
    return res.status == 0 and [float(v) for v in res.chmax] == want_k[1] and np.array_equal(frame.scanlines(), want_k[0])


def _refused(res, frame, code):
    return res.status == code and [float(v) for v in res.chmax] == [0.0] * 4 and frame.untouched()


@pytest.mark.parametrize("lanes", [1, 2])
def test_batch_run_io_a_refused_frame_fails_its_turn_and_the_lane_behind_it(gpu_ctx, lanes):
    """frame 2 asks for 12-bit scanlines, which the argument checks refuse before anything of it is queued: the lane stops there, what it had
    queued before runs to its end and says so, and the other lane never hears of it"""
    sensors, want = _wanted(gpu_ctx, STATUS_SIZES, 160)
    p = _pipe_params()
    frames = [_Frame(s, _G, _G) for s in sensors]
    frames[2].out.bps = 12
    rc, res = _status_batch(gpu_ctx, lanes, frames, p)
    assert rc == EINVAL
    assert b"bps 12" in capi.LIB.artgpu_last_error(gpu_ctx._h)
    for k in range(5):
        stopped = k % lanes == 2 % lanes and k >= 2          # frame 2's lane, from frame 2 on
        if stopped:
            assert _refused(res[k], frames[k], EINVAL), (k, res[k].status, list(res[k].chmax))
        else:
            assert _complete(res[k], frames[k], want[k]), (k, res[k].status, list(res[k].chmax))


@pytest.mark.parametrize("lanes", [1, 2])
def test_batch_run_io_a_batch_the_plan_refuses_leaves_no_frame_that_looks_done(gpu_ctx, lanes):
    sensors, want = _wanted(gpu_ctx, STATUS_SIZES, 160)
    p = _pipe_params()
    frames = [_Frame(s, _G, _G) for s in sensors]
    try:
        gpu_ctx.set_pipeline_tone_equalizer(capi.tone_equalizer_params(bands=(40, -25, 10, 60, -80), regularization=5, pivot=-4.0))
        rc, res = _status_batch(gpu_ctx, lanes, frames, p)
    finally:
        gpu_ctx.set_pipeline_tone_equalizer(None)
    assert rc == EUNSUPPORTED
    for k in range(5):
        assert _refused(res[k], frames[k], EUNSUPPORTED), (k, res[k].status, list(res[k].chmax))
    # the same context, the same buffers, a batch that is fine
    rc, res = _status_batch(gpu_ctx, lanes, frames, p)
    assert rc == 0
    for k in range(5):
        assert _complete(res[k], frames[k], want[k]), (k, res[k].status, list(res[k].chmax))


@pytest.mark.parametrize("lanes", [1, 2])
def test_batch_run_io_rgb2out_report_survives_a_later_failure_of_its_lane(gpu_ctx, lanes):
    """frame 1 has values above 1 behind a non-linear TRC (complete but for those pixels, ARTGPU_EUNSUPPORTED), frame 3 -- the same lane with
    one lane or two -- is refused: frame 1's own report stands, frame 3 and what follows it on the lane carry the lane's code"""
    trc = _trc()
    sensors, want = _wanted(gpu_ctx, STATUS_SIZES, 160, trc=trc)
    p = _pipe_params()
    frames = [_Frame(s, _G, _G) for s in sensors]
    for f in frames:
        f.out.trc_linear = 0
        f.out.trc_lut = trc.ctypes.data_as(C.POINTER(C.c_float)); f.out.trc_lutsz = trc.size
    frames[1].out.out_matrix[:] = [float(v) for v in (3.0 * np.eye(3, dtype=np.float32)).reshape(9)]
    frames[3].out.bps = 12
    rc, res = _status_batch(gpu_ctx, lanes, frames, p)
    assert rc == EINVAL                                        # (the lane's own error comes before a frame's report)
    assert res[1].status == EUNSUPPORTED and [float(v) for v in res[1].chmax] == want[1][1]
    rows = frames[1].scanlines()
    assert not (rows == PATTERN16).all(axis=(1, 2)).any() and frames[1].margins_untouched()      # every row was written
    assert _refused(res[3], frames[3], EINVAL)
    for k in (0, 2, 4):
        if lanes == 1 and k == 4:
            assert _refused(res[k], frames[k], EINVAL), (k, res[k].status)
        else:
            assert _complete(res[k], frames[k], want[k]), (k, res[k].status, list(res[k].chmax))


def test_batch_run_io_leaves_the_callers_cu_reserve_alone(gpu_ctx):
    """the option only sizes the persistent grids: the bits are the chain's with it, and a batch (which reserves CUs for its own direct
    downloads while it runs) hands it back as the caller set it"""
    sensors, want = _wanted(gpu_ctx, STATUS_SIZES, 160)
    p = _pipe_params()
    assert gpu_ctx.get_option("cu_reserve") == 0 and gpu_ctx.get_option("io_direct") == -1
    try:
        gpu_ctx.set_option("cu_reserve", 5)
        gpu_ctx.set_option("io_direct", 3)
        gpu_ctx.set_batch_lanes(2)
        assert gpu_ctx.get_option("io_direct") == 3
        for kind in (_P, _G):          # pinned: direct download, the batch reserves CUs of its own; pageable: it reserves none
            frames = [_Frame(s, kind, kind) for s in sensors]
            res = gpu_ctx.batch_run_io([f.inp for f in frames], p, [f.out for f in frames])
            assert gpu_ctx.get_option("cu_reserve") == 5, kind
            for k in range(5):
                assert _complete(res[k], frames[k], want[k]), (kind, k)
    finally:
        gpu_ctx.set_batch_lanes(1)
        gpu_ctx.set_option("cu_reserve", 0)
        gpu_ctx.set_option("io_direct", -1)
