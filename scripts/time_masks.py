"""Time artgpu_generate_masks on a device-resident 45 MP image (8192 x 5464, RGB mode): one region with three curves, blur 0, L mask only --
what a regional tool asks for.  Warm-up, then the median of --reps calls, event-timed on the context's stream (the call has no host wait for
device planes).  Beside the time: what uploading the same fp32 plane from pinned host memory costs, measured in the same process (the
alternative the adapter has today: generateMasks on the CPU, then one upload per region).
The per-kernel split comes from a run of its own under `rocprofv3 --kernel-trace --stats -- python scripts/time_masks.py --reps 3`; with
--stats-csv FILE the script reads that run's kernel statistics instead and prints each kernel's share.
One JSON line.  The script ends itself after --timeout seconds."""
import argparse
import csv
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def kernel_shares(path):
    """rocprofv3's kernel_stats.csv -> total time by group of kernels (ns) and each group's share"""
    groups = {"guided filters": ("gf_", "hblur", "vblur"), "fused pass": ("mk_fused",), "lightness-detail prepare": ("mk_ll",), "tail": ("mk_tail",),
              "copies": ("copy", "Copy", "fill", "Fill")}
    tot, rows = {}, []
    for row in csv.DictReader(open(path)):
        name, ns = row["Name"], float(row["TotalDurationNs"])
        rows.append((name, int(row["Calls"]), ns))
        g = next((g for g, keys in groups.items() if any(k in name for k in keys)), "other")
        tot[g] = tot.get(g, 0.0) + ns
    s = sum(tot.values())
    return {"kernels": [{"name": n[:80], "calls": c, "total_ms": round(ns / 1e6, 3)} for n, c, ns in sorted(rows, key=lambda r: -r[2])[:12]],
            "group_ms": {g: round(v / 1e6, 3) for g, v in tot.items()}, "group_share": {g: round(v / s, 3) for g, v in tot.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=5464)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--stats-csv", default=None)
    args = ap.parse_args()
    if args.stats_csv:
        print(json.dumps(kernel_shares(args.stats_csv)))
        return
    signal.alarm(args.timeout)
    import torch
    from art_amd import capi
    import mk_lib
    import oracle_lib as O

    w, h = args.width, args.height
    tile = mk_lib.scene(1024, 683, seed=9)                      # the tests' hue wheel, repeated over the frame
    img_t = torch.stack([torch.from_numpy(np.ascontiguousarray(np.tile(t, (h // 683 + 1, w // 1024 + 1))[:h, :w])) for t in tile]).to("cuda:0")
    out = torch.empty((1, h, w), dtype=torch.float32, device="cuda:0")
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    image = capi.RGB(*[capi.device_plane(img_t[c]) for c in range(3)])
    masks = [mk_lib.mask(parametric_enabled=True, hue=mk_lib.HUE_A, chromaticity=mk_lib.CHROMA_A, lightness=mk_lib.LIGHT_A, lightness_detail=50)]
    planes = [capi.device_plane(out[0])]
    info, times = None, []
    for rep in range(args.warmup + args.reps):
        with torch.cuda.stream(stream):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            info = ctx.generate_masks(image, mk_lib.MODE_RGB, O.REC2020_WS_D, masks, w, h, 1.0, planes, None, want_info=True)
            t1.record(stream)
        stream.synchronize()
        if rep >= args.warmup:
            times.append(t0.elapsed_time(t1))
    # the same plane uploaded from pinned host memory
    host = torch.empty((h, w), dtype=torch.float32).pin_memory()
    up = []
    for rep in range(args.warmup + args.reps):
        with torch.cuda.stream(stream):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            out[0].copy_(host, non_blocking=True)
            t1.record(stream)
        stream.synchronize()
        if rep >= args.warmup:
            up.append(t0.elapsed_time(t1))
    ms, ums = float(np.median(times)), float(np.median(up))
    P = w * h * 4
    print(json.dumps({"w": w, "h": h, "regions": 1, "curves": 3, "blur": 0, "lmask_only": True, "info": dict(zip(mk_lib.INFO_FIELDS, mk_lib.info_fields(info[0]))),
                      "reps": args.reps, "ms_median": round(ms, 3), "ms_min": round(float(np.min(times)), 3), "ms_max": round(float(np.max(times)), 3),
                      "plane_bytes": P, "upload_ms_median": round(ums, 3), "upload_gbs": round(P / 1e9 / (ums / 1e3), 1),
                      "ratio_to_upload": round(ms / ums, 2), "scratch_bytes": ctx.scratch_bytes()}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
