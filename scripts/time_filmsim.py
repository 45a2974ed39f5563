"""Time artgpu_film_simulation on a device-resident 45 MP image (8192 x 5464) with the tests' "look" table at the levels given by --levels
(default 64,144: a level-8 and a level-12 HaldCLUT file) and both same_profile values: warm-up, then the median of --reps calls, event-timed on
the context's stream.  Timed in the same run, alternating, so that every form sees the same clocks:
  - artgpu_tone_curve (tone_std) on the same planes: the nearest existing pass, one table lookup per channel (a yardstick, not a gate);
  - with --random, the same call with the random table: neighbouring pixels still hit neighbouring cells, the values differ.
Beside the times: the 24 B/px the pass has to move (three planes in, three out) and the time those bytes take at the device-copy rate measured
the way `bench.py --full` measures its device_copy_gbs.  One JSON line per level and same_profile value.
With --pipe instead: artgpu_pipeline_run on a device-resident 45 MP Bayer frame with the parameters of tests/test_gpu_pipeline.py (AMaZE, the
denoise tool with the exposure fused in, the standard tone curve) with the setting off, ahead of the tone curve and behind it, alternating; one
JSON line per level.
The script ends itself after --timeout seconds."""
import argparse
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from art_amd import capi  # noqa: E402
import fs_lib  # noqa: E402


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


def pipe(args):
    from art_amd import synth
    from test_gpu_pipeline import _lut, _params
    w, h = args.width, args.height
    lut = _lut()
    pp = _params(lut, 0)
    b = pp.border
    raw = torch.from_numpy(synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=1, noise=1500)).to("cuda:0")
    out = [torch.empty((h - 2 * b, w - 2 * b), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    rawp, img = capi.device_plane(raw), capi.RGB(*[capi.device_plane(t) for t in out])

    def frame():
        with torch.cuda.stream(stream):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            ctx.pipeline_run(rawp, pp, img)
            t1.record(stream)
        stream.synchronize()
        return t0.elapsed_time(t1)

    for level in [int(v) for v in args.levels.split(",")]:
        look = ctx.clut(fs_lib.clut("look", level), level)
        p = fs_lib.capi_params(fs_lib.params(args.strength, False))
        times = {"off": [], "ahead": [], "behind": []}
        for rep in range(args.warmup + args.reps):
            for name in times:
                if name == "off":
                    ctx.set_pipeline_film_simulation(None)
                else:
                    ctx.set_pipeline_film_simulation(look, p, after_tone_curve=name == "behind")
                ms = frame()
                if rep >= args.warmup:
                    times[name].append(ms)
        ctx.set_pipeline_film_simulation(None)
        line = {"w": w, "h": h, "level": level, "same_profile": 0, "reps": args.reps}
        for name, v in times.items():
            line["frame_ms_" + name] = {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}
        print(json.dumps(line), flush=True)
        ctx.synchronize()
        look.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=5464)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--levels", default="64,144")
    ap.add_argument("--strength", type=float, default=1.0)
    ap.add_argument("--random", action="store_true", help="also time the random table")
    ap.add_argument("--default-only", action="store_true", help="time only the tool (kernel traces, counter runs)")
    ap.add_argument("--pipe", action="store_true", help="time artgpu_pipeline_run with the setting off / ahead of / behind the tone curve")
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
    signal.alarm(args.timeout)
    w, h = args.width, args.height
    if args.pipe:
        return pipe(args)
    # a tile of the tests' scene repeated over the frame
    tile = fs_lib.scene(1024, 683, seed=9)
    src = [torch.from_numpy(np.ascontiguousarray(np.tile(t, (h // 683 + 1, w // 1024 + 1))[:h, :w])).to("cuda:0") for t in tile]
    work = [torch.empty_like(s) for s in src]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    img = capi.RGB(*[capi.device_plane(t) for t in work])
    gbs = copy_rate_gbs(w, h)
    x = np.arange(65536, dtype=np.float64) / 65535.0
    tone = ((1.0 - np.cos(np.pi * x ** 0.7)) / 2.0 * 65535.0).astype(np.float32)

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

    def stat(v):
        return {"ms_median": round(float(np.median(v)), 3), "ms_min": round(float(np.min(v)), 3), "ms_max": round(float(np.max(v)), 3)}

    for level in [int(v) for v in args.levels.split(",")]:
        look = ctx.clut(fs_lib.clut("look", level), level)
        rnd = ctx.clut(fs_lib.clut("random", level), level) if args.random and not args.default_only else None
        for same in (True, False):
            p = fs_lib.capi_params(fs_lib.params(args.strength, same))
            tool, random_table, tone_std = [], [], []
            for rep in range(args.warmup + args.reps):
                ms = timed(lambda: ctx.film_simulation(img, look, p))
                if rep >= args.warmup:
                    tool.append(ms)
                if rnd is not None:
                    ms = timed(lambda: ctx.film_simulation(img, rnd, p))
                    if rep >= args.warmup:
                        random_table.append(ms)
                if not args.default_only:
                    ms = timed(lambda: ctx.tone_curve(img, tone, 1.0, True))
                    if rep >= args.warmup:
                        tone_std.append(ms)
            ms = float(np.median(tool))
            nbytes = 24.0 * w * h
            at_copy = nbytes / 1e9 / gbs * 1e3
            line = {"w": w, "h": h, "level": level, "clut_mb": round((level ** 3 + 1) * 8 / 1e6, 1), "same_profile": int(same), "strength": args.strength,
                    "reps": args.reps, **stat(tool), "device_copy_gbs": round(gbs, 1), "ms_at_copy_rate": round(at_copy, 3),
                    "ratio_to_copy_rate": round(ms / at_copy, 2), "achieved_gbs": round(nbytes / 1e9 / (ms / 1e3), 1)}
            if random_table:
                line["random_table"] = stat(random_table)
            if tone_std:
                line["tone_std_same_planes"] = dict(stat(tone_std), ratio=round(ms / float(np.median(tone_std)), 2))
            print(json.dumps(line), flush=True)
        ctx.synchronize()
        look.close()
        if rnd is not None:
            rnd.close()
    ctx.close()


if __name__ == "__main__":
    main()
