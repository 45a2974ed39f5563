#!/usr/bin/env python3
"""Static instruction counts per phase of the DCT block kernels, from the compiler's assembly:
    python scripts/detail_phase_counts.py [RAD]
compiles art_amd/csrc/detail.hip for gfx950 with -DDETAIL_PHASE_MARKS (an assembly comment at the start of every phase) and counts, per kernel
and phase, the instructions by the unit that issues them.  Static: the `factors` phases hold rolled loops (steady rows in groups of eight), so
their dynamic count is several times the figure; every other phase is straight-line code and runs once per block."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = "--offload-arch=gfx950 -Wno-unused-command-line-argument -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -DDETAIL_PHASE_MARKS -S --cuda-device-only".split()


def klass(m):
    if m.startswith("v_pk_"): return "valu_pk"
    if m.startswith("v_"): return "valu"
    if m.startswith(("s_load", "s_buffer_load")): return "smem"
    if m.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_branch", "s_cbranch", "s_endpgm")): return "ctl"
    if m.startswith("s_"): return "salu"
    if m.startswith("ds_"): return "lds"
    if m.startswith(("global_", "buffer_", "flat_", "scratch_")): return "vmem"
    return "other"


def main():
    rad = sys.argv[1] if len(sys.argv) > 1 else "3"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "detail.s")
        subprocess.check_call([hipcc, *FLAGS, "-o", out, os.path.join(ROOT, "art_amd", "csrc", "detail.hip")])
        text = open(out).read().splitlines()
    cols = ["valu", "valu_pk", "salu", "smem", "lds", "vmem", "ctl"]
    for kern in ("detail_blocks_kernel", "detail_blocks_trim_kernel"):
        sym = f"_ZN6artgpu{len(kern)}{kern}ILi{rad}EEEvNS_10DetailArgsE"
        start = next(i for i, l in enumerate(text) if l.startswith(sym + ":"))
        end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
        phase, counts, order = "prologue", collections.defaultdict(collections.Counter), ["prologue"]
        for line in text[start + 1:end]:
            line = line.strip()
            m = re.match(r";\s*detail-phase (\S+)", line)
            if m:
                phase = m.group(1)
                if phase not in order: order.append(phase)
                continue
            if not line or line.startswith((";", ".", "//")) or line.endswith(":"): continue
            counts[phase][klass(line.split()[0])] += 1
        print(f"{kern}<{rad}>")
        print("  %-16s" % "phase" + "".join("%9s" % c for c in cols))
        tot = collections.Counter()
        for ph in order:
            if ph == "end": continue
            tot.update(counts[ph])
            print("  %-16s" % ph + "".join("%9d" % counts[ph][c] for c in cols))
        print("  %-16s" % "all (static)" + "".join("%9d" % tot[c] for c in cols))


if __name__ == "__main__":
    main()
