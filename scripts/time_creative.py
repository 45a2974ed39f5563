"""Time the creative-gradients, soft-light and black-and-white kernels on a device-resident 8192 x 5464 image, and in the same process
artgpu_exposure, an in-place pass of the same 24 B/px, as the yardstick.  Warm-up, then --reps calls of each setting, event-timed on the
context's stream, the settings taking turns (round robin) so that a drift of the clocks meets all of them alike.  A call is one launch; the
tables of soft light and black-and-white are built and uploaded by the warm-up calls.
The expectation this checks: every setting is bound by its 24 B/px, i.e. its median lies within the exposure pass's own spread (its slowest
repeat over its median, in this run) of the exposure pass's median.  One JSON line per setting: ms_median / ms_min / ms_max, the achieved
GB/s, the ratio to the yardstick's median and whether that is inside the margin.  With --trace-only: one call per setting and no timing
(a kernel trace or a counter run of its own).  The script ends itself after --timeout seconds."""
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

WS = [0.6369580483012914, 0.14461690358620832, 0.1688809751641721, 0.2627002120112671, 0.6779980715188708, 0.05930171646986196,
      0.0, 0.028072693049087428, 1.060985057710791]      # Rec2020 -> XYZ (D65): row 1 is what the colour cast's setMode(YUV) reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=5464)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated setting names (counter runs of single kernels)")
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
    signal.alarm(args.timeout)
    w, h = args.width, args.height
    if args.trace_only:
        args.reps, args.warmup = 1, 0
    # linear scene data: most of it in the lower half of the tables, some super-white, a few negatives
    g = torch.Generator(device="cuda:0").manual_seed(3)
    src = [(torch.rand((h, w), device="cuda:0", generator=g) ** 2.2 * 70000.0 - 200.0) for _ in range(3)]
    work = [torch.empty_like(s) for s in src]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    img = capi.RGB(*[capi.device_plane(t) for t in work])
    x = np.arange(65536, dtype=np.float64) / 65535.0
    sat = np.sin(np.pi * x) ** 2
    ul, vl = (65535.0 * x ** 0.8 * 0.11 * sat).astype(np.float32), (65535.0 * x ** 0.8 * -0.07 * sat).astype(np.float32)
    grad = capi.creative_gradients_params(gradient=(30, 40, 1.2, 10, -20))
    grad_full = capi.creative_gradients_params(gradient=(30, 100, 1.2, 0, 0))                    # feather 100: nearly every pixel on the ramp
    pcv = capi.creative_gradients_params(pcvignette=(1.5, 60, 50, -20, 10))
    pcv_super = capi.creative_gradients_params(pcvignette=(1.5, 100, 20, 0, 0))                  # super-ellipses of degree 4 and 6, feather 100
    both = capi.creative_gradients_params(gradient=(30, 100, 1.2, 0, 0), pcvignette=(1.5, 100, 20, 0, 0))
    sl = capi.soft_light_params(40)
    bw, k0 = capi.black_and_white_params("Landscape", "Orange", (40, 30, 25))
    bwg, k1 = capi.black_and_white_params("Landscape", "Orange", (40, 30, 25), (20, -35, 60))
    bwc, k2 = capi.black_and_white_params("Landscape", "Orange", (40, 30, 25), (20, -35, 60), cast=(30, 40), ulut=ul, vlut=vl)
    settings = [("exposure (yardstick)", lambda: ctx.exposure(img, 1.23, 10.0)),
                ("gradient", lambda: ctx.creative_gradients(img, grad)), ("gradient, feather 100", lambda: ctx.creative_gradients(img, grad_full)),
                ("vignette", lambda: ctx.creative_gradients(img, pcv)), ("vignette, super-ellipse", lambda: ctx.creative_gradients(img, pcv_super)),
                ("gradient + vignette", lambda: ctx.creative_gradients(img, both)),
                ("soft light", lambda: ctx.soft_light(img, sl)),
                ("black and white", lambda: ctx.black_and_white(img, bw)), ("black and white, gamma", lambda: ctx.black_and_white(img, bwg)),
                ("black and white, gamma + cast", lambda: ctx.black_and_white(img, bwc, WS))]
    if args.only:
        settings = [s for s in settings if s[0] in args.only.split(",")]

    def timed(fn):
        with torch.cuda.stream(stream):
            for d, s in zip(work, src):
                d.copy_(s)
            stream.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            fn()
            t1.record(stream)
        stream.synchronize()
        return t0.elapsed_time(t1)

    times = {name: [] for name, _ in settings}
    for rep in range(args.warmup + args.reps):
        for name, fn in settings:
            ms = timed(fn)
            if rep >= args.warmup:
                times[name].append(ms)
    if args.trace_only:
        ctx.close()
        return
    nbytes = 24.0 * w * h
    yard = times.get("exposure (yardstick)")
    y_med = float(np.median(yard)) if yard else None
    margin = float(np.max(yard)) / y_med if yard else None
    for name, _ in settings:
        v = times[name]
        med = float(np.median(v))
        line = {"w": w, "h": h, "setting": name, "reps": args.reps, "ms_median": round(med, 4), "ms_min": round(float(np.min(v)), 4), "ms_max": round(float(np.max(v)), 4),
                "gbs_at_24_b_px": round(nbytes / 1e9 / (med / 1e3), 1)}
        if y_med:
            line.update({"ratio_to_exposure": round(med / y_med, 3), "exposure_spread_margin": round(margin, 3), "inside_margin": bool(med / y_med <= margin)})
        print(json.dumps(line), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
