"""Time artgpu_tone_equalizer on a device-resident 45 MP image (8192 x 5464) at the regularization levels given by --levels (default 0,1,4,2:
no filter; the detail filter; detail + one regularising filter, the tool's default; all three): warm-up, then the median of --reps calls,
event-timed on the context's stream (no info is asked for: the call does not wait for the host).
Timed in the same run, alternating, so that all forms see the same clocks:
  - both forms of the group-of-four rule (option te_group_thread 0: one pixel per lane and a ballot; 1: one thread per group);
  - with a regularising filter, its last pointwise pass inside te_apply or as a pass of its own (option te_fuse_upsample 1 / 0);
  - at level 0, artgpu_exposure on the same planes: it moves the same bytes with less arithmetic (a yardstick, not a gate).
Beside the times: the planes the call reads and writes, derived from the kernels as built, against the minimum, and the time
those bytes would take at the device-copy rate measured the way `bench.py --full` measures its device_copy_gbs.  One JSON line per level.
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
import oracle_lib  # noqa: E402
import te_lib  # noqa: E402


def subsampling(w, h, r):
    """calculate_subsampling (guidedfilter.cc:58-75)"""
    if r == 1 or max(w, h) <= 600:
        return 1
    for s in range(5, 0, -1):
        if r % s == 0:
            return s
    return max(2, min(r // 2, 4))


def traffic_planes(w, h, level, scale=1.0, fuse=True):
    """full-size planes (P = w * h * 4 bytes) per call, by pass: every kernel's reads and writes counted once.  The statistics of a guided
    filter live on a (w / s) x (h / s) grid: its subsample pass reads two rows of every s of the one or two planes it samples, and its
    kernels and box blurs move grid planes, counted as 1 / s^2 of a plane each (4 in / 4 out subsample, 4 x 4 blur, 6 ab, 2 x 4 blur)."""
    if level == 0:
        return {"te_direct": 6.0, "total": 6.0, "minimum": 6.0}

    def stats(r, planes_sampled):
        s = subsampling(w, h, r)
        sample = planes_sampled * (min(2.0 / s, 1.0) if s > 1 else 1.0)
        return sample + (4 + 16 + 6 + 8) / float(s * s)

    post = level > 1
    steps = {"te_prepare": 4.0, "detail_stats": stats(int(5.0 / scale + 0.5), 1), "te_detail_finish": 3.0 if post else 2.0}
    if post:
        r = int(350.0 / scale)
        reg = 5 - min(level, 4)
        steps["regularise_1_stats"] = stats(r, 2)
        if reg > 1:
            steps["regularise_1_finish"] = 2.0
            steps["regularise_2_stats"] = stats(r * (reg - 1), 2)
        if not fuse:
            steps["regularise_last_finish"] = 2.0
    steps["te_apply"] = 7.0
    steps["total"] = sum(steps.values())
    steps["minimum"] = 4.0 + 7.0                     # 3P in + P out, the filters (not counted), then 4P in + 3P out
    return {k: round(v, 3) for k, v in steps.items()}


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
    ap.add_argument("--levels", default="0,1,4,2")
    ap.add_argument("--pivot", type=float, default=-4.0)
    ap.add_argument("--default-only", action="store_true", help="time only the default forms (kernel traces of the default path)")
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
    signal.alarm(args.timeout)
    w, h = args.width, args.height
    # a tile of the tests' scene repeated over the frame
    tile = te_lib.scene(1024, 683, seed=9)
    src = [torch.from_numpy(np.ascontiguousarray(np.tile(t, (h // 683 + 1, w // 1024 + 1))[:h, :w])).to("cuda:0") for t in tile]
    work = [torch.empty_like(s) for s in src]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    img = capi.RGB(*[capi.device_plane(t) for t in work])
    gbs = copy_rate_gbs(w, h)
    P = w * h * 4

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
        params = capi.tone_equalizer_params((40, -25, 10, 60, -80), level, args.pivot)
        forms = [(0, 1)] if args.default_only else ([(0, 1), (1, 1)] + ([(0, 0)] if level > 1 else []))      # (te_group_thread, te_fuse_upsample)
        times = {f: [] for f in forms}
        exposure = []
        for rep in range(args.warmup + args.reps):
            for f in forms:
                ctx.set_option("te_group_thread", f[0])
                ctx.set_option("te_fuse_upsample", f[1])
                ms = timed(lambda: ctx.tone_equalizer(img, params, oracle_lib.REC2020_WS_D, 1.0))
                if rep >= args.warmup:
                    times[f].append(ms)
            if level == 0 and not args.default_only:
                ms = timed(lambda: ctx.exposure(img, float(np.float32(2.0 ** 0.3)), 0.0))
                if rep >= args.warmup:
                    exposure.append(ms)
        ctx.set_option("te_group_thread", 0)
        ctx.set_option("te_fuse_upsample", 1)
        tp = traffic_planes(w, h, level)
        ms = float(np.median(times[(0, 1)]))
        at_copy = tp["total"] * P / 1e9 / gbs * 1e3
        line = {"w": w, "h": h, "regularization": level, "pivot": args.pivot, "reps": args.reps, **stat(times[(0, 1)]), "planes": tp,
                "device_copy_gbs": round(gbs, 1), "ms_at_copy_rate": round(at_copy, 3), "ratio_to_copy_rate": round(ms / at_copy, 2),
                "achieved_gbs": round(tp["total"] * P / 1e9 / (ms / 1e3), 1), "scratch_bytes": ctx.scratch_bytes()}
        if (1, 1) in times:
            line["group_thread_form"] = stat(times[(1, 1)])
        if (0, 0) in times:
            line["upsample_in_its_own_pass"] = dict(stat(times[(0, 0)]), planes_total=traffic_planes(w, h, level, fuse=False)["total"])
        if exposure:
            line["exposure_same_planes"] = dict(stat(exposure), ratio=round(ms / float(np.median(exposure)), 2))
        print(json.dumps(line), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
