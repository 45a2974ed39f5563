"""Time artgpu_raw_ca_correct on a 45 MP CFA plane (8192 x 5464, device resident): auto with 1, 2 and 3 iterations, colour-shift guard
on and off.  One JSON line per configuration (median of --reps calls, event-timed on the context's stream).  Run it under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/ca_time.py` for the per-kernel split."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from art_amd import capi, synth  # noqa: E402
import ca_lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=5464)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    w, h, f = args.width, args.height, synth.FILTERS_RGGB
    raw = torch.from_numpy(ca_lib.lateral_ca_frame(w, h, f, k_red=0.0004, k_blue=-0.0003, seed=11)).to("cuda:0")
    work = torch.empty_like(raw)
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    plane = capi.device_plane(work)
    for it in (1, 2, 3):
        for guard in (1, 0):
            p = capi.CaParams(1, it, 0.0, 0.0, guard)
            times = []
            for rep in range(args.reps + 1):
                with torch.cuda.stream(stream):
                    work.copy_(raw)
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    ctx.raw_ca_correct(plane, f, p)
                    t1.record(stream)
                stream.synchronize()
                if rep:
                    times.append(t0.elapsed_time(t1))
            print(json.dumps({"w": w, "h": h, "iterations": it, "guard": guard, "ms_median": float(np.median(times)),
                              "ms_min": float(np.min(times)), "reps": args.reps}), flush=True)


if __name__ == "__main__":
    main()
