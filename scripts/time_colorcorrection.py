"""Time artgpu_color_correction on a device-resident 45 MP image (8192 x 5464) for one and three regions in the JZAZBZ, RGB and HSL modes
(HSL once without and once with a hue shift: only the latter carries the double-precision rgb2hsl / hsl2rgb), every region with its own
device-resident Lmask and abmask planes.  Warm-up, then the median of --reps calls, event-timed on the context's stream (the call has no host
wait without `info`).
Beside each time: the bytes the call moves, derived from the kernel as built (one pass: 24 B/px for the image and 8 B/px per region for the
two masks; a region list that mixes Jzazbz with an HSL hue shift or holds more than four regions is further passes of 24 B/px), and the time
those bytes would take at the device-copy rate measured in the same process the way `bench.py --full` measures its device_copy_gbs.
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

SOP = dict(slope=(1.15, 0.9, 1.05), offset=(0.04, -0.02, 0.03), power=(1.2, 0.85, 1.1))
MODES = {
    "jzazbz": dict(mode="jzazbz", a=0.35, b=-0.2, in_saturation=25.0, out_saturation=-30.0, **SOP),
    "rgb": dict(mode="rgb", pivot=(0.8, 1.2, 0.6), compression=(0.4, 0.2, 0.7), in_saturation=25.0, **SOP),
    "hsl": dict(mode="hsl", hue=(30.0, 200.0, 310.0), sat=(40.0, 25.0, 60.0), factor=(10.0, -15.0, 20.0)),
    "hsl_hueshift": dict(mode="hsl", hue=(30.0, 200.0, 310.0), sat=(40.0, 25.0, 60.0), factor=(10.0, -15.0, 20.0), hueshift=20.0),
}


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
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--regions", default="1,3")
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    signal.alarm(args.timeout)
    w, h = args.width, args.height
    # a tile of the tests' scene repeated over the frame; the masks are the tests' smooth ramp and its mirror (exact zeros and ones in both)
    tiles = tb_lib.rgb_scene(1024, 683, seed=9)
    src = [torch.from_numpy(np.ascontiguousarray(np.tile(t, (h // 683 + 1, w // 1024 + 1))[:h, :w])).to("cuda:0") for t in tiles]
    work = [torch.empty_like(s) for s in src]
    ramp = torch.from_numpy(tb_lib.smooth_mask(w, h)).to("cuda:0")
    masks = [ramp, torch.flip(ramp, dims=(1,)).contiguous()]
    gbs = copy_rate_gbs(w, h)
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    img = capi.RGB(*[capi.device_plane(t) for t in work])
    for mode in args.modes.split(","):
        for n in [int(v) for v in args.regions.split(",")]:
            planes = [[m.clone() for m in masks] for _ in range(n)]           # 2 n planes of their own: nothing is shared between regions
            regions = [dict(MODES[mode], lmask=capi.device_plane(p[0]), abmask=capi.device_plane(p[1])) for p in planes]
            with torch.cuda.stream(stream):
                for d, s in zip(work, src):
                    d.copy_(s)
                info = ctx.color_correction(img, regions, O.REC2020_WS_D, O.REC2020_IWS_D, True, want_info=True)
            times = []
            for rep in range(args.warmup + args.reps):
                with torch.cuda.stream(stream):
                    for d, s in zip(work, src):
                        d.copy_(s)
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    ctx.color_correction(img, regions, O.REC2020_WS_D, O.REC2020_IWS_D, True)
                    t1.record(stream)
                stream.synchronize()
                if rep >= args.warmup:
                    times.append(t0.elapsed_time(t1))
            nbytes = w * h * (24 + 8 * n)
            ms = float(np.median(times))
            at_copy = nbytes / 1e9 / gbs * 1e3
            print(json.dumps({"w": w, "h": h, "mode": mode, "regions": n, "launches": 1, "reps": args.reps, "ms_median": round(ms, 3),
                              "ms_min": round(float(np.min(times)), 3), "ms_max": round(float(np.max(times)), 3), "bytes": nbytes,
                              "bytes_per_px": 24 + 8 * n, "device_copy_gbs": round(gbs, 1), "ms_at_copy_rate": round(at_copy, 3),
                              "ratio_to_copy_rate": round(ms / at_copy, 2), "achieved_gbs": round(nbytes / 1e9 / (ms / 1e3), 1),
                              "oor_pixels": int(info[0].oor_pixels), "scratch_bytes": ctx.scratch_bytes()}), flush=True)
            del planes, regions
    ctx.close()


if __name__ == "__main__":
    main()
