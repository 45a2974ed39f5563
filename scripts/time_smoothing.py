"""Time artgpu_smoothing on a device-resident 45 MP image (8192 x 5464): GUIDED L, C and LC at radius 3 and radius 20 on the full frame (no
mask), GUIDED LC on a quarter-frame crop (a device mask that is positive inside a 4096 x 2732 box), NLMEANS L and LC at strength 50, one
iteration, full frame.  Beside them, in the same process: artgpu_denoise_guided_smoothing at radius 3 (what GUIDED C is set against) and
artgpu_nlmeans on one normalised plane (what NLMEANS L is set against).  Two warm-up calls, then HIP events around each of --reps calls:
median, min and max.
Beside each time: the bytes the tool's own passes move, derived from the kernels as built (DESIGN.md section 26 has the sums; `s` is the
guided filter's subsampling, 3 at radius 3 and 5 at radius 20 on this frame), and the time those bytes would take at the device-copy rate
measured in the same process the way `bench.py --full` measures its device_copy_gbs.  NL-means' own traffic is not in `bytes` (the plane
filter is artgpu_nlmeans' code; its figure is the separate line).
One JSON line per configuration.  The script ends itself after --timeout seconds."""
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
import oracle_lib as O  # noqa: E402
import tb_lib  # noqa: E402


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


def guided_bytes_per_px(channel, s):
    """one iteration on a full-frame region with both normalise passes fused, per working pixel"""
    if channel == "lc":
        return 60.0 + 336.0 / (s * s)
    return 80.0 + 400.0 / (s * s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=5464)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    signal.alarm(args.timeout)
    w, h = args.width, args.height
    npx = w * h
    tiles = tb_lib.rgb_scene(1024, 683, seed=9)
    src = [torch.from_numpy(np.ascontiguousarray(np.tile(t, (h // 683 + 1, w // 1024 + 1))[:h, :w])).to("cuda:0") for t in tiles]
    work = [torch.empty_like(s) for s in src]
    gbs = copy_rate_gbs(w, h)
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    img = capi.RGB(*[capi.device_plane(t) for t in work])
    bw, bh = w // 2, h // 2
    crop = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
    crop[h // 4:h // 4 + bh, w // 4:w // 4 + bw] = 0.75
    crop_plane = capi.device_plane(crop)

    def sub(radius):
        return 1 if max(w, h) <= 600 or radius == 1 else next((s for s in (5, 4, 3, 2, 1) if radius % s == 0))

    configs = []
    for radius in (3, 20):
        for ch in ("l", "c", "lc"):
            configs.append(("guided-%s-r%d" % (ch, radius), [dict(mode="guided", channel=ch, radius=radius)], npx * guided_bytes_per_px(ch, sub(radius))))
    # cropped: the box pass reads the mask (4 B/px of the frame), neither normalise pass is fused (2 x 24 B/px of the frame), the region's passes and
    # its mask on the quarter
    configs.append(("guided-lc-r3-quarter-crop", [dict(mode="guided", channel="lc", radius=3, mask=crop_plane)],
                    npx * (4 + 48) + bw * bh * (guided_bytes_per_px("lc", sub(3)) + 4)))
    configs.append(("nlmeans-l-s50", [dict(mode="nlmeans", channel="l", nlstrength=50)], npx * 44.0))
    configs.append(("nlmeans-lc-s50", [dict(mode="nlmeans", channel="lc", nlstrength=50)], npx * 60.0))
    configs.append(("denoise_guided_smoothing-r3", None, npx * (68.0 + 400.0 / 9.0)))
    configs.append(("nlmeans-plane-s50", None, None))
    plane = torch.empty((h, w), dtype=torch.float32, device="cuda:0")

    def call(name, regions):
        if name == "denoise_guided_smoothing-r3":
            ctx.denoise_guided_smoothing(img, O.REC2020_WS_D, radius=3, scale=1.0)
        elif name == "nlmeans-plane-s50":
            ctx.nlmeans(capi.device_plane(plane), strength=50, detail=50, scale=1.0, normcoeff=1.0)
        else:
            ctx.smoothing(img, regions, O.REC2020_WS_D, 1.0)

    for name, regions, nbytes in configs:
        if args.only and name not in args.only.split(","):
            continue
        times = []
        for rep in range(args.warmup + args.reps):
            with torch.cuda.stream(stream):
                for d, s in zip(work, src):
                    d.copy_(s)
                plane.copy_(src[1])
                plane.mul_(1.0 / 65535.0)
                t0 = torch.cuda.Event(enable_timing=True)
                t1 = torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                call(name, regions)
                t1.record(stream)
            stream.synchronize()
            if rep >= args.warmup:
                times.append(t0.elapsed_time(t1))
        ms = float(np.median(times))
        rec = {"w": w, "h": h, "config": name, "reps": args.reps, "ms_median": round(ms, 3), "ms_min": round(float(np.min(times)), 3),
               "ms_max": round(float(np.max(times)), 3), "device_copy_gbs": round(gbs, 1), "scratch_bytes": ctx.scratch_bytes()}
        if nbytes is not None:
            at_copy = nbytes / 1e9 / gbs * 1e3
            rec.update({"bytes": int(nbytes), "bytes_per_px": round(nbytes / npx, 1), "ms_at_copy_rate": round(at_copy, 3),
                        "ratio_to_copy_rate": round(ms / at_copy, 2), "achieved_gbs": round(nbytes / 1e9 / (ms / 1e3), 1)})
        print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
