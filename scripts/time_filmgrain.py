"""Time film grain on a device-resident 45 MP image (8256 x 5504): artgpu_add_noise per region for kernel sizes 3 / 5 / 7 (coarseness 0 / 30 /
100 at scale 1) and channels L / LC, and artgpu_film_grain at its defaults with colour off and on.  Warm-up, then the median of --reps calls,
event-timed on the context's stream: a call's time holds the host's table construction, the table's upload, the region kernel and (add_noise,
or an odd number of regions) the copy back into the image.  The region kernel alone is read from a kernel trace of this script
(rocprofv3 --kernel-trace --stats, a run of its own, with --trace-only: one call per setting).
Beside the times: the bytes a region has to move (12 B/px read, 12 B/px written) at the device-copy rate measured in the same process the way
`bench.py --full` measures its device_copy_gbs.  One JSON line per setting.  The script ends itself after --timeout seconds."""
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
import fg_lib  # noqa: E402


def copy_rate_gbs(w, h):
    nb = w * h * 3
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=8256)
    ap.add_argument("--height", type=int, default=5504)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-only", action="store_true", help="one call per setting and no copy-rate measurement (kernel traces, counter runs)")
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
    signal.alarm(args.timeout)
    w, h = args.width, args.height
    if args.trace_only:
        args.reps, args.warmup = 1, 0
    tile = fg_lib.scene(1032, 688, "wild")
    src = [torch.from_numpy(np.ascontiguousarray(np.tile(t, (h // 688 + 1, w // 1032 + 1))[:h, :w])).to("cuda:0") for t in tile]
    work = [torch.empty_like(s) for s in src]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    img = capi.RGB(*[capi.device_plane(t) for t in work])
    gbs = None if args.trace_only else copy_rate_gbs(w, h)
    region_bytes = 24.0 * w * h

    def timed(fn):
        with torch.cuda.stream(stream):
            for d, s in zip(work, src):
                d.copy_(s)
            stream.synchronize()
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            fn()
            t1.record(stream)
        stream.synchronize()
        return t0.elapsed_time(t1)

    def report(name, fn, regions, extra):
        v = []
        for rep in range(args.warmup + args.reps):
            ms = timed(fn)
            if rep >= args.warmup:
                v.append(ms)
        line = {"w": w, "h": h, "setting": name, "regions": regions, "reps": args.reps, **stat(v), **extra}
        if gbs is not None:
            at_copy = regions * region_bytes / 1e9 / gbs * 1e3
            line.update({"compulsory_mb": round(regions * region_bytes / 1e6, 1), "device_copy_gbs": round(gbs, 1), "ms_at_copy_rate": round(at_copy, 3),
                         "call_ratio_to_copy_rate": round(float(np.median(v)) / at_copy, 2)})
        print(json.dumps(line), flush=True)

    for channel, cname in ((fg_lib.L, "L"), (fg_lib.LC, "LC")):
        for coarseness, sz in ((0, 3), (30, 5), (100, 7)):
            report(f"add_noise {cname} sz {sz}", lambda: ctx.add_noise(img, 50, coarseness, channel, fg_lib.WS), 1, {"channel": cname, "sz": sz})
    for color in (False, True):
        p = capi.film_grain_params(400, 50, color)
        report(f"film_grain defaults colour {int(color)}", lambda: ctx.film_grain(img, p, fg_lib.WS), 4 if color else 3, {})
    ctx.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
