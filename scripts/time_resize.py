"""Time artgpu_resize_lanczos on a device-resident 45 MP image (8192 x 5464) at the Resize tool's usual settings -- scale 0.5, scale 0.25 and
"fit the 2048 box" -- in both modes: warm-up, then the median of --reps calls, event-timed on the context's stream.  ARTGPU_RESIZE_RGB
includes the two mode switches (rgb_to_lab at full size, lab_to_rgb on the small image); its source is copied back before every call.
Beside the times: the bytes the resampler has to move (the source planes once, the destination planes once) and the time they take at
the device-copy rate measured the way `bench.py --full` measures its device_copy_gbs.  One JSON line per setting.
With --default-only: only the PLANES call (kernel traces, counter runs).
With --io instead: artgpu_batch_run_io on pinned host buffers, uint16 sensor frames in and 16-bit scanlines out (the host_buffers
configuration), --frames frames on --lanes lanes, with the setting off (full size) and at --io-scale, alternating; one JSON line.
The script ends itself after --timeout seconds."""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from art_amd import capi, synth  # noqa: E402
import oracle_lib as O  # noqa: E402


def copy_rate_gbs(w, h):
    nb = w * h * 4
    src = torch.empty(nb, dtype=torch.float32, device="cuda:0").normal_()
    dst = torch.empty_like(src)
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    for _ in range(2):
        dst.copy_(src)
    ev[0].record()
    for _ in range(5):
        dst.copy_(src)
    ev[1].record()
    torch.cuda.synchronize()
    return 5 * 2 * nb * 4 / 1e9 / (ev[0].elapsed_time(ev[1]) / 1e3)


def stat(v):
    return {"ms_median": round(float(np.median(v)), 3), "ms_min": round(float(np.min(v)), 3), "ms_max": round(float(np.max(v)), 3)}


def io(args):
    from test_gpu_pipeline import _lut, _params
    w, h = args.width, args.height
    lut = _lut()
    pp = _params(lut, 0)
    b = pp.border
    par = capi.resize_params(dataspec=0, scale=args.io_scale)
    imw, imh, _ = capi.resize_scale(par, w - 2 * b, h - 2 * b)
    sensor = np.clip(synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=1, noise=1500), 0, 65535).astype(np.uint16)
    ins = [torch.empty((h, w), dtype=torch.int16).pin_memory() for _ in range(args.frames)]
    for t in ins:
        t.numpy().view(np.uint16)[:] = sensor
    outs = {"off": [torch.zeros((h - 2 * b, w - 2 * b, 3), dtype=torch.int16).pin_memory() for _ in range(args.frames)],
            "resize": [torch.zeros((imh, imw, 3), dtype=torch.int16).pin_memory() for _ in range(args.frames)]}
    ctx = capi.Context(0)
    ctx.set_batch_lanes(args.lanes)
    black, mul = (64.0, 60.0, 68.0, 62.0), (1.02, 1.0, 0.98, 1.01)
    times = {"off": [], "resize": []}
    for rep in range(args.warmup + args.reps):
        for name in times:
            ctx.set_pipeline_resize(par if name == "resize" else None)
            frames_in = [capi.sensor_frame(t.numpy().view(np.uint16), black, mul) for t in ins]
            frames_out = [capi.scanline_frame(t.numpy().view(np.uint16), None, None) for t in outs[name]]
            t0 = time.perf_counter()
            ctx.batch_run_io(frames_in, pp, frames_out)
            ms = (time.perf_counter() - t0) * 1e3 / args.frames
            if rep >= args.warmup:
                times[name].append(ms)
    ctx.set_pipeline_resize(None)
    line = {"w": w, "h": h, "frames": args.frames, "lanes": args.lanes, "scale": args.io_scale, "out": [imw, imh], "reps": args.reps,
            "host_mb_per_frame_off": round((w * h * 2 + (w - 2 * b) * (h - 2 * b) * 6) / 1e6, 1), "host_mb_per_frame_resize": round((w * h * 2 + imw * imh * 6) / 1e6, 1)}
    for name, v in times.items():
        line["ms_per_frame_" + name] = stat(v)
    print(json.dumps(line), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=5464)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--default-only", action="store_true", help="time only the PLANES call (kernel traces, counter runs)")
    ap.add_argument("--io", action="store_true", help="time artgpu_batch_run_io on pinned host buffers with the setting off and on")
    ap.add_argument("--io-scale", type=float, default=0.25)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
    signal.alarm(args.timeout)
    w, h = args.width, args.height
    if args.io:
        return io(args)
    # a tile of the tests' scene repeated over the frame
    import rs_lib
    tile = rs_lib.scene(1024, 683, "scaled_frac")
    src = [torch.from_numpy(np.ascontiguousarray(np.tile(t, (h // 683 + 1, w // 1024 + 1))[:h, :w])).to("cuda:0") for t in tile]
    work = [torch.empty_like(s) for s in src]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    img = capi.RGB(*[capi.device_plane(t) for t in work])
    gbs = copy_rate_gbs(w, h)

    def timed(fn):
        with torch.cuda.stream(stream):
            for d, s in zip(work, src):
                d.copy_(s)
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            fn()
            t1.record(stream)
        stream.synchronize()
        return t0.elapsed_time(t1)

    settings = (("scale 0.5", capi.resize_params(dataspec=0, scale=0.5)), ("scale 0.25", capi.resize_params(dataspec=0, scale=0.25)),
                ("fit 2048", capi.resize_params(dataspec=3, width=2048, height=2048)))
    for name, par in settings:
        imw, imh, scale = capi.resize_scale(par, w, h)
        out = [torch.empty((imh, imw), dtype=torch.float32, device="cuda:0") for _ in range(3)]
        dst = capi.RGB(*[capi.device_plane(t) for t in out])
        planes, rgb = [], []
        for rep in range(args.warmup + args.reps):
            ms = timed(lambda: ctx.resize_lanczos(img, dst, scale, capi.RESIZE_PLANES))
            if rep >= args.warmup:
                planes.append(ms)
            if not args.default_only:
                ms = timed(lambda: ctx.resize_lanczos(img, dst, scale, capi.RESIZE_RGB, O.REC2020_WS_D, O.REC2020_IWS_D))
                if rep >= args.warmup:
                    rgb.append(ms)
        ms = float(np.median(planes))
        nbytes = 12.0 * (w * h + imw * imh)
        at_copy = nbytes / 1e9 / gbs * 1e3
        line = {"w": w, "h": h, "setting": name, "scale": float(scale), "out": [imw, imh], "reps": args.reps, **stat(planes),
                "compulsory_mb": round(nbytes / 1e6, 1), "device_copy_gbs": round(gbs, 1), "ms_at_copy_rate": round(at_copy, 3),
                "ratio_to_copy_rate": round(ms / at_copy, 2), "achieved_gbs": round(nbytes / 1e9 / (ms / 1e3), 1)}
        if rgb:
            line["rgb_mode"] = stat(rgb)
        print(json.dumps(line), flush=True)
    ctx.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
