"""bench.py --dump-outputs: what the last timed step computed, written so that two builds can be compared value for value."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
import oracle_lib as O
from art_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_small_planes_and_a_fixed_sample_of_large_ones(tmp_path):
    g = torch.Generator().manual_seed(1)
    small = torch.rand(288, 416, generator=g)
    big = {f"image_{c}": torch.rand(2048, 1100, generator=g) for c in "rgb"}
    bench.dump_outputs(str(tmp_path / "s"), {"demosaic_r": small}, 1)
    a = np.load(tmp_path / "s" / "demosaic_r.npy")
    assert a.dtype == np.float32 and np.array_equal(a, small.numpy())
    for d in ("b1", "b2"):
        bench.dump_outputs(str(tmp_path / d), big, 1)
    for c in "rgb":
        a, b = np.load(tmp_path / "b1" / f"image_{c}.npy"), np.load(tmp_path / "b2" / f"image_{c}.npy")
        assert a.shape == (1 << 20,) and np.array_equal(a, b)
        assert np.isin(a, big[f"image_{c}"].numpy()).all()
    # the budget holds for every file of a run, over lanes and ranks
    many = {f"lane{k}_image_{c}": torch.zeros(2048, 2048) for k in range(8) for c in "rgb"}
    bench.dump_outputs(str(tmp_path / "m"), many, 2)
    assert 2 * sum(os.path.getsize(tmp_path / "m" / f) for f in os.listdir(tmp_path / "m")) <= bench.DUMP_BYTES


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_demosaic_it_timed(tmp_path):
    w, h = 416, 288
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "amaze", "--width", str(w), "--height", str(h),
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and "roofline" not in line and "cpu_baseline" not in line
    raw = synth.bayer_frame(w, h, synth.FILTERS_RGGB, seed=0)
    for c, ref in zip("rgb", O.amaze(raw, synth.FILTERS_RGGB, 1.0, 4)):
        got = np.load(out / f"demosaic_{c}.npy")
        assert got.shape == (h, w) and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), c
