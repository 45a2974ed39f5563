"""Time artgpu_local_contrast on a device-resident 45 MP L plane (8192 x 5464), one region: warm-up, then the median of --reps calls,
event-timed on the context's stream (the call's one host wait per region lies inside the interval).  Beside the time: the bytes the
call moves, derived from the band count (local contrast section), and the time those bytes would take at the device-copy
rate measured the way `bench.py --full` measures its device_copy_gbs (a 716 MB device-to-device copy, read + write bytes).  One JSON
line.  The script ends itself after --timeout seconds."""
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
import lc_lib  # noqa: E402


def traffic_bytes(w, h, contrast_on=True):
    """bytes per region, by phase: every kernel's reads and writes counted once (stencil re-reads are cache hits)"""
    nl = lc_lib.levels(w, h)
    full = w * h * 4
    band = ((w + 1) // 2) * ((h + 1) // 2) * 4
    nb = 3 * nl
    decompose = full + 4 * band + (nl - 1) * 5 * band            # level 0: plane in, 4 bands out; Haar level: 1 in, 4 out
    stats_remap = 4 * nb * band + (3 * band if contrast_on else 0)   # bands: average, variance, remap reads + one write; coeff0: 2 reads + 1 write
    reconstruct = (nl - 1) * 5 * band + 4 * band + full          # Haar level: 4 in, 1 out; level 0: 4 bands in, plane out
    blend = 3 * full                                             # L_new and l in, L out
    return {"levels": nl, "decompose": decompose, "stats_remap": stats_remap, "reconstruct": reconstruct, "blend": blend,
            "total": decompose + stats_remap + reconstruct + blend}


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
    ap.add_argument("--contrast", type=float, default=40.0)
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    signal.alarm(args.timeout)
    w, h = args.width, args.height
    rng = np.random.default_rng(5)
    # a tile of the tests' plane repeated over the frame, with fresh noise (building the full-size plane from sines takes a minute)
    tile = lc_lib.l_plane(1024, 683, seed=9, noise=0.0)
    src = np.tile(tile, (h // 683 + 1, w // 1024 + 1))[:h, :w] + rng.normal(0.0, 300.0, (h, w)).astype(np.float32)
    src = torch.from_numpy(np.clip(src, 0.0, 32768.0).astype(np.float32)).to("cuda:0")
    work = torch.empty_like(src)
    curve = lc_lib.curve_lut(lc_lib.BOOST_CURVE_POINTS)
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    plane = capi.device_plane(work)
    times = []
    for rep in range(args.warmup + args.reps):
        with torch.cuda.stream(stream):
            work.copy_(src)
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            ctx.local_contrast(plane, [(args.contrast, curve, None)])
            t1.record(stream)
        stream.synchronize()
        if rep >= args.warmup:
            times.append(t0.elapsed_time(t1))
    tb = traffic_bytes(w, h, args.contrast != 0)
    gbs = copy_rate_gbs(w, h)
    ms = float(np.median(times))
    print(json.dumps({"w": w, "h": h, "levels": tb["levels"], "contrast": args.contrast, "reps": args.reps, "ms_median": round(ms, 3),
                      "ms_min": round(float(np.min(times)), 3), "ms_max": round(float(np.max(times)), 3),
                      "bytes": {k: v for k, v in tb.items() if k != "levels"}, "device_copy_gbs": round(gbs, 1),
                      "ms_at_copy_rate": {k: round(v / 1e9 / gbs * 1e3, 3) for k, v in tb.items() if k != "levels"},
                      "achieved_gbs": round(tb["total"] / 1e9 / (ms / 1e3), 1), "scratch_bytes": ctx.scratch_bytes()}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
