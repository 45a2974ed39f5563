"""Time artgpu_sharpening on a device-resident 45 MP image (8192 x 5464) with Sharpening.arp's values (rld, contrast 20, amount 100) at the
deconvolution radii given by --sigmas (default 0.75: the 5x5 regime, one fused kernel per iteration; 1.6: the recursive gaussian): warm-up,
then the median of --reps calls, event-timed on the context's stream (no info is asked for: the call does not wait for the host).
For the stencil regimes the two-kernels-per-iteration form (option sharpen_fused 0: DIV, MULT, check_stop as three launches) is timed in the
same run, alternating with the fused kernel, so the line says what the fusion bought.
Beside the times: the bytes the call moves, derived from the kernels as built, and the time those bytes would take at
the device-copy rate measured the way `bench.py --full` measures its device_copy_gbs.  One JSON line per sigma.  The script ends itself after
--timeout seconds."""
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
import sh_lib  # noqa: E402


def traffic_bytes(w, h, sigma, fused=True):
    """bytes per call, by step: every kernel's reads and writes counted once (a stencil's neighbours and a tile's halo are cache hits)"""
    P = w * h * 4
    B = w * h
    gauss = 8 * P                                      # the shared recursive gaussian, in place: each direction forward (in, tmp out) and backward (tmp in, out)
    if sigma < 0.25:
        it = 0                                         # the blur is a copy: one check_stop pass in all (3 P)
    elif sigma <= 1.15:
        it = 4 * P if fused else 9 * P                 # fused: estimate in, l, out in, estimate out; else DIV 3 P, MULT 3 P, check_stop 3 P
    else:
        it = 2 * P + gauss + 3 * P + gauss + 5 * P     # copy, blur, DIV step, blur, MULT + check_stop
    steps = {
        "luminance": 4 * P,
        "blend_mask": 2 * P + gauss,
        "mark_impulse": 2 * P + gauss + 3 * P + P + B,
        "copy_Y": 2 * P,
        "rl_init": 4 * P,
        "rl_iterations": 20 * it if it else 3 * P,
        "rl_final": 5 * P + B,
        "multiply": 8 * P,
    }
    steps["total"] = sum(steps.values())
    return steps


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
    ap.add_argument("--sigmas", default="0.75,1.6")
    ap.add_argument("--no-unfused", action="store_true", help="do not time the two-kernel form (kernel traces of the default path)")
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
    signal.alarm(args.timeout)
    w, h = args.width, args.height
    # a tile of the tests' edge scene repeated over the frame
    tile = sh_lib.edge_scene(1024, 683, seed=9)
    src = [torch.from_numpy(np.ascontiguousarray(np.tile(t, (h // 683 + 1, w // 1024 + 1))[:h, :w])).to("cuda:0") for t in tile]
    work = [torch.empty_like(s) for s in src]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    img = capi.RGB(*[capi.device_plane(t) for t in work])
    gbs = copy_rate_gbs(w, h)
    for sigma in [float(v) for v in args.sigmas.split(",")]:
        params = capi.sharpening_params(deconvradius=sigma)
        forms = [1] if (args.no_unfused or not 0.25 <= sigma <= 1.15) else [1, 0]
        times = {f: [] for f in forms}
        for rep in range(args.warmup + args.reps):
            for f in forms:                                        # alternating: both forms see the same clocks
                ctx.set_option("sharpen_fused", f)
                with torch.cuda.stream(stream):
                    for d, s in zip(work, src):
                        d.copy_(s)
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    ctx.sharpening(img, params, oracle_lib.REC2020_WS_D, 1.0)
                    t1.record(stream)
                stream.synchronize()
                if rep >= args.warmup:
                    times[f].append(t0.elapsed_time(t1))
        ctx.set_option("sharpen_fused", 1)
        tb = traffic_bytes(w, h, sigma, True)
        ms = float(np.median(times[1]))
        line = {"w": w, "h": h, "sigma": sigma, "reps": args.reps, "ms_median": round(ms, 3), "ms_min": round(float(np.min(times[1])), 3),
                "ms_max": round(float(np.max(times[1])), 3), "bytes": tb, "device_copy_gbs": round(gbs, 1),
                "ms_at_copy_rate": round(tb["total"] / 1e9 / gbs * 1e3, 3), "ratio_to_copy_rate": round(ms / (tb["total"] / 1e9 / gbs * 1e3), 2),
                "achieved_gbs": round(tb["total"] / 1e9 / (ms / 1e3), 1), "scratch_bytes": ctx.scratch_bytes()}
        if 0 in times:
            tu = traffic_bytes(w, h, sigma, False)
            mu = float(np.median(times[0]))
            line["two_kernel_form"] = {"ms_median": round(mu, 3), "ms_min": round(float(np.min(times[0])), 3), "ms_max": round(float(np.max(times[0])), 3),
                                       "bytes_total": tu["total"], "ratio_to_copy_rate": round(mu / (tu["total"] / 1e9 / gbs * 1e3), 2)}
        print(json.dumps(line), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
