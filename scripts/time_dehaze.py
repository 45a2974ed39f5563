"""Time artgpu_dehaze on a device-resident 45 MP image (8192 x 5464) with the default DehazeParams: warm-up, then the median of --reps
calls, event-timed on the context's stream (the call's one host wait, the ambient estimate on the thumbnail, lies inside the interval).
Beside the time: the bytes the call moves, derived from the kernels as built (dehaze section), and the time those bytes would
take at the device-copy rate measured the way `bench.py --full` measures its device_copy_gbs (a 716 MB device-to-device copy, read +
write bytes).  One JSON line.  The script ends itself after --timeout seconds."""
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
import dh_lib  # noqa: E402
import oracle_lib  # noqa: E402


def gf_subsampling(w, h, r):
    """calculate_subsampling (guidedfilter.cc:58-75)"""
    if r == 1 or max(w, h) <= 600:
        return 1
    for s in range(5, 0, -1):
        if r % s == 0:
            return s
    return min(max(r // 2, 2), 4)


def traffic_bytes(w, h, scale=1.0, blackpoint=0):
    """bytes per call, by step: every kernel's reads and writes counted once (the bilinear reads of the statistics grids are cache hits
    after the first; the thumbnail, the state block and the strength table are below a megabyte)"""
    P = w * h * 4
    r1 = max(int(5 / scale), 2)
    s1 = gf_subsampling(w, h, r1)
    patch = max(max(w, h) // 600, 2)
    s2 = gf_subsampling(w, h, 4 * patch)
    l1, l2 = (w // s1) * (h // s1) * 4, (w // s2) * (h // s2) * 4
    blur = 4                                                   # a box blur of one plane: row pass in + out, column pass in + out
    steps = {
        "max": 3 * P,
        "normalise": 6 * P,                                    # (a black point adds the thumbnail's kernels only)
        "self_guided_x3": 3 * P + 6 * l1 + 2 * 6 * blur * l1 + 12 * l1,   # image in, six grid planes out; two rounds of six blurs; a / b in place
        "dark_channel": 3 * P + 6 * l1 + P // (patch * patch),            # the three q planes are evaluated, not stored
        "transmission": 4 * P,
        "last_guided": 2 * P + 4 * l2 + (4 + 2) * blur * l2 + 6 * l2,
        "recovery": 6 * P + 2 * l2,                            # t evaluated from mean a / mean b; restore in the same pass
    }
    steps["total"] = sum(steps.values())
    return {"patch": patch, "subsampling": [s1, s2]}, steps


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
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    signal.alarm(args.timeout)
    w, h = args.width, args.height
    # a tile of the tests' hazy scene repeated over the frame (building the full-size scene from sines takes a minute)
    tile = dh_lib.hazy_scene(1024, 683, seed=9)
    src = [torch.from_numpy(np.ascontiguousarray(np.tile(t, (h // 683 + 1, w // 1024 + 1))[:h, :w])).to("cuda:0") for t in tile]
    work = [torch.empty_like(s) for s in src]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    img = capi.RGB(*[capi.device_plane(t) for t in work])
    params, keep = capi.dehaze_params()
    times, info = [], None
    for rep in range(args.warmup + args.reps):
        with torch.cuda.stream(stream):
            for d, s in zip(work, src):
                d.copy_(s)
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            info = ctx.dehaze(img, params, oracle_lib.REC2020_WS_D, 1.0, want_info=True)
            t1.record(stream)
        stream.synchronize()
        if rep >= args.warmup:
            times.append(t0.elapsed_time(t1))
    shape, tb = traffic_bytes(w, h)
    gbs = copy_rate_gbs(w, h)
    ms = float(np.median(times))
    print(json.dumps({"w": w, "h": h, **shape, "haze_detected": int(info.haze_detected), "reps": args.reps, "ms_median": round(ms, 3),
                      "ms_min": round(float(np.min(times)), 3), "ms_max": round(float(np.max(times)), 3), "bytes": tb,
                      "device_copy_gbs": round(gbs, 1), "ms_at_copy_rate": {k: round(v / 1e9 / gbs * 1e3, 3) for k, v in tb.items()},
                      "ratio_to_copy_rate": round(ms / (tb["total"] / 1e9 / gbs * 1e3), 2),
                      "achieved_gbs": round(tb["total"] / 1e9 / (ms / 1e3), 1), "scratch_bytes": ctx.scratch_bytes()}), flush=True)
    del keep
    ctx.close()


if __name__ == "__main__":
    main()
