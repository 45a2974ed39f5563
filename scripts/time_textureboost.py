"""Time artgpu_texture_boost_plane on a device-resident 45 MP Y plane (8192 x 5464), one region at iterations 1, for the three paths of the
tool: detail threshold 0.2 (the default: 7 x 7 convolution), 1.0 (guided, rescaled 1.14x) and 2.0 (guided, not rescaled).  Warm-up, then the
median of --reps calls, event-timed on the context's stream (the call has no host wait without `info`).
Beside each time: the bytes the call moves, derived from the kernels as built, and the time those bytes would take at
the device-copy rate measured the way `bench.py --full` measures its device_copy_gbs (a device-to-device copy, read + write bytes).
One JSON line per threshold.  The script ends itself after --timeout seconds."""
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
import tb_lib  # noqa: E402


def gf_subsampling(w, h, r):
    """calculate_subsampling (guidedfilter.cc:58-75)"""
    if r == 1 or max(w, h) <= 600:
        return 1
    return next(s for s in range(5, 0, -1) if r % s == 0)


def traffic_bytes(W, H, info, iterations=1):
    """bytes per call, by step: every kernel's reads and writes counted once (the bilinear reads of the statistics grids and the
    convolution's halo are cache hits after the first)"""
    P, Pw = W * H * 4, info.work_w * info.work_h * 4
    w, h = info.work_w, info.work_h
    blur = 4                                                   # a box blur of one plane: row pass in + out, column pass in + out
    s2 = gf_subsampling(w, h, 4 * info.radius)
    l2 = (w // s2) * (h // s2) * 4
    stats = lambda l: Pw + 2 * l + 2 * blur * l + 4 * l + 2 * blur * l        # subsample, two blurs, a / b in place, two blurs
    steps = {"prepare": P + 2 * Pw}
    if info.isguided:
        s1 = gf_subsampling(w, h, info.radius)
        l1 = (w // s1) * (h // s1) * 4
        steps["first_filter"] = iterations * (stats(l1) + 2 * Pw + 2 * l1)    # mid is stored: the next filter and the combine pass read it
    else:
        s1 = 0
        steps["convolution"] = iterations * 2 * Pw
    steps["second_filter_stats"] = iterations * stats(l2)
    last_write = Pw if info.rescaled else P
    steps["combine"] = (iterations - 1) * (3 * Pw + 2 * l2) + 2 * Pw + 2 * l2 + last_write      # base is evaluated, not stored
    if info.rescaled:
        steps["downscale"] = Pw + P
    steps["total"] = sum(steps.values())
    return {"subsampling": [s1, s2]}, steps


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=5464)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--thresholds", default="0.2,1.0,2.0")
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    signal.alarm(args.timeout)
    w, h = args.width, args.height
    # a tile of the tests' textured plane repeated over the frame
    tile = tb_lib.textured_plane(1024, 683, seed=9)
    src = torch.from_numpy(np.ascontiguousarray(np.tile(tile, (h // 683 + 1, w // 1024 + 1))[:h, :w])).to("cuda:0")
    work = torch.empty_like(src)
    gbs = copy_rate_gbs(w, h)
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    Y = capi.device_plane(work)
    for thr in [float(t) for t in args.thresholds.split(",")]:
        with torch.cuda.stream(stream):
            work.copy_(src)
            info = ctx.texture_boost_plane(Y, 1.0, thr, 1, 1.0, True, want_info=True)
        times = []
        for rep in range(args.warmup + args.reps):
            with torch.cuda.stream(stream):
                work.copy_(src)
                t0 = torch.cuda.Event(enable_timing=True)
                t1 = torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                ctx.texture_boost_plane(Y, 1.0, thr, 1, 1.0, True)
                t1.record(stream)
            stream.synchronize()
            if rep >= args.warmup:
                times.append(t0.elapsed_time(t1))
        shape, tb = traffic_bytes(w, h, info)
        ms = float(np.median(times))
        print(json.dumps({"w": w, "h": h, "detail_threshold": thr, "isguided": int(info.isguided), "rescaled": int(info.rescaled), "radius": int(info.radius),
                          "kernel_size": int(info.kernel_size), "work": [int(info.work_w), int(info.work_h)], **shape, "reps": args.reps,
                          "ms_median": round(ms, 3), "ms_min": round(float(np.min(times)), 3), "ms_max": round(float(np.max(times)), 3), "bytes": tb,
                          "device_copy_gbs": round(gbs, 1), "ms_at_copy_rate": {k: round(v / 1e9 / gbs * 1e3, 3) for k, v in tb.items()},
                          "ratio_to_copy_rate": round(ms / (tb["total"] / 1e9 / gbs * 1e3), 2),
                          "achieved_gbs": round(tb["total"] / 1e9 / (ms / 1e3), 1), "scratch_bytes": ctx.scratch_bytes()}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
