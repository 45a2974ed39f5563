"""GPU: artgpu-cli --ca (RawImageSource::CA_correct_RT in the C++ mirror, RAWParams' CA fields in BatchQueue) equals the library
chain: the CA checker's corrected CFA through the same front end without --ca (single frame), and scaleColors -> checker CA ->
the oracle's pipeline -> getScanline (batch queue)."""
import json
import subprocess

import numpy as np
import pytest

from art_amd import synth
import ca_lib
import oracle_lib as O
from test_gpu_cli import CLI, oracle_pipeline, read_ppm16, run_cli

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flags,kw", [(["--ca", "auto"], dict(autocorrect=True, iterations=2, avoid_colour_shift=True)),
                                      (["--ca", "auto,1", "--ca-keep-colourshift"], dict(autocorrect=True, iterations=1, avoid_colour_shift=False)),
                                      (["--ca", "manual,1.5,-6"], dict(autocorrect=False, red=1.5, blue=-6.0, avoid_colour_shift=True))],
                         ids=["auto", "auto1-keep", "manual"])
def test_cli_ca_equals_checker_then_cli(tmp_path, flags, kw):
    raw = ca_lib.lateral_ca_frame(640, 480, synth.FILTERS_RGGB)
    corrected, _ = ca_lib.ca_correct(raw, synth.FILTERS_RGGB, **kw)
    assert not np.array_equal(corrected, raw)
    _, got = run_cli(tmp_path, raw, "amaze", ["--expcomp", "0.3", *flags])
    _, want = run_cli(tmp_path, corrected, "amaze", ["--expcomp", "0.3"])
    assert np.array_equal(got, want)


def test_cli_batch_ca_auto(tmp_path):
    w, h, filt, b, black = 640, 480, synth.FILTERS_RGGB, 4, 64.0
    frames = [np.clip(ca_lib.lateral_ca_frame(w, h, filt, seed=30 + k), 0, 65535).astype(np.uint16) for k in range(2)]
    names = []
    for k, f in enumerate(frames):
        n = tmp_path / f"f{k}.u16"
        f.astype("<u2").tofile(n)
        names.append(str(n))
    res = subprocess.run([CLI, "--batch", ",".join(names), "--width", str(w), "--height", str(h), "--lanes", "2", "--black", str(black),
                          "--expcomp", "0.3", "--ca", "auto", "--out", str(tmp_path / "o")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    assert json.loads(res.stdout.strip().splitlines()[-1])["frames"] == 2
    for k, f in enumerate(frames):
        raw = np.maximum(f.astype(np.float32) - np.float32(black), np.float32(0.0))          # scaleColors with scale_mul 1
        corrected, _ = ca_lib.ca_correct(raw, filt, True, 2, avoid_colour_shift=True)
        want = O.get_scanlines(oracle_pipeline(corrected, filt, "amaze", b, expcomp=0.3), 16, False)
        plain = O.get_scanlines(oracle_pipeline(raw, filt, "amaze", b, expcomp=0.3), 16, False)
        got = read_ppm16(tmp_path / f"o.{k}.ppm")
        assert not np.array_equal(plain, want)
        assert np.array_equal(got, want), (k, int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max()))
