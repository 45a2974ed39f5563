"""Times artgpu_impulse_denoise and artgpu_defringe on one 8256 x 5504 device image (45 MP) whose scene flags about 2 % of the pixels, next to
artgpu_exposure, an in-place pass of 24 B/px, as the yardstick in the same process.  Event-timed repeats after warm-up rounds, the settings taking
turns; one JSON line per setting on stdout (and into --out).  Per-kernel times come from running this under a kernel trace
(rocprofv3 --kernel-trace --stats -- python scripts/time_impulse_defringe.py --repeats 3).

    python scripts/time_impulse_defringe.py [--width 8256 --height 5504 --repeats 15 --warmup 3 --out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from art_amd import capi  # noqa: E402

WS = np.array([[0.6734241, 0.1656411, 0.1251286], [0.2790177, 0.6753402, 0.0456377], [-0.0019300, 0.0299784, 0.7973330]])
IWS = np.array([[1.6473376, -0.3935675, -0.2359961], [-0.6826036, 1.6475887, 0.0128190], [0.0296524, -0.0628993, 1.2531279]])


def scene(w, h, seed=1):
    """a smooth ramp with mild noise; 1 % of the pixels are salt and pepper (impulse noise) and purple discs of radius 2 .. 5 cover about 2 %
    (fringes), built on the device"""
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda:0", dtype=torch.float32), torch.arange(w, device="cuda:0", dtype=torch.float32), indexing="ij")
    planes = [9000.0 + 2000.0 * c + 1.1 * xx + 0.9 * yy + 25.0 * torch.randn((h, w), device="cuda:0", generator=g) for c in range(3)]
    hit = torch.rand((h, w), device="cuda:0", generator=g) < 0.01
    f = torch.where(torch.rand((h, w), device="cuda:0", generator=g) < 0.5, 4.0, 0.15)
    planes = [torch.where(hit, p * f, p) for p in planes]
    n = int(0.02 * w * h / 38.0)
    cx, cy = torch.rand(n, device="cuda:0", generator=g) * w, torch.rand(n, device="cuda:0", generator=g) * h
    r = 2.0 + 3.0 * torch.rand(n, device="cuda:0", generator=g)
    cx, cy, r = cx.cpu().numpy(), cy.cpu().numpy(), r.cpu().numpy()
    disc = torch.zeros((h, w), dtype=torch.bool, device="cuda:0")
    for k in range(n):
        x0, x1, y0, y1 = int(max(cx[k] - 6, 0)), int(min(cx[k] + 7, w)), int(max(cy[k] - 6, 0)), int(min(cy[k] + 7, h))
        sub = (yy[y0:y1, x0:x1] - float(cy[k])) ** 2 + (xx[y0:y1, x0:x1] - float(cx[k])) ** 2 <= float(r[k]) ** 2
        disc[y0:y1, x0:x1] |= sub
    col = (30000.0, 5000.0, 42000.0)
    return [torch.where(disc, torch.full_like(p, col[c]), p).contiguous() for c, p in enumerate(planes)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=8256)
    ap.add_argument("--height", type=int, default=5504)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--discs", type=int, default=1, help="0: no discs (a quick scene)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = a.width, a.height
    ctx = capi.Context(0)
    src = scene(w, h) if a.discs else [torch.rand((h, w), device="cuda:0") * 20000.0 + 5000.0 for _ in range(3)]
    work = [torch.empty_like(p) for p in src]
    rgb = capi.RGB(*[capi.device_plane(t) for t in work])
    settings = {"exposure (yardstick)": lambda: ctx.exposure(rgb, 1.1, 0.0),
                "rgb_to_lab + lab_to_rgb": lambda: (ctx.rgb_to_lab(rgb, WS), ctx.lab_to_rgb(rgb, IWS)),
                "impulse, thresh 50": lambda: ctx.impulse_denoise(rgb, capi.impulse_denoise_params(True, 50), WS, IWS, 1.0, True)}
    for radius in (0.5, 2.0, 5.0):
        settings[f"defringe, radius {radius}"] = (lambda r: lambda: ctx.defringe(rgb, capi.defringe_params(True, r, 13), WS, IWS, 1.0, True))(radius)
    times = {k: [] for k in settings}
    for rnd in range(a.warmup + a.repeats):
        for name, call in settings.items():
            for d, s in zip(work, src):
                d.copy_(s)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record()
            torch.cuda.synchronize()
            if rnd >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    for d, s in zip(work, src):
        d.copy_(s)
    shares = {"impulse": ctx.impulse_denoise(rgb, capi.impulse_denoise_params(True, 50), WS, IWS, 1.0, True, want_info=True).impulse_pixels / (w * h)}
    for radius in (0.5, 2.0, 5.0):
        for d, s in zip(work, src):
            d.copy_(s)
        shares[f"defringe {radius}"] = ctx.defringe(rgb, capi.defringe_params(True, radius, 13), WS, IWS, 1.0, True, want_info=True).corrected_pixels / (w * h)
    lines = [json.dumps({"setting": k, "w": w, "h": h, "ms_median": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v)), "repeats": len(v)})
             for k, v in times.items()] + [json.dumps({"flagged_share": shares})]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
