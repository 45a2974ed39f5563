"""GPU: artgpu_raw_ca_correct at 8192 x 5464 (45 MP), the default profile's settings (auto, 2 iterations, colour-shift guard on),
bit for bit against the CPU checker."""
import numpy as np
import pytest
import torch

from art_amd import capi, synth
import ca_lib

pytestmark = pytest.mark.gpu


def test_fullsize_default_profile():
    w, h, f = 8192, 5464, synth.FILTERS_RGGB
    raw = ca_lib.lateral_ca_frame(w, h, f, k_red=0.0004, k_blue=-0.0003, seed=11)
    want, wfit, info = ca_lib.ca_correct(raw, f, True, 2, avoid_colour_shift=True, want_info=True)
    assert info["processpasstwo"] and info["iterations_run"] == 2
    ctx = capi.Context(0)
    d = torch.from_numpy(raw).to("cuda:0")
    fit = ctx.raw_ca_correct(capi.device_plane(d), f, capi.CaParams(1, 2, 0.0, 0.0, 1), want_fit=True)
    ctx.synchronize()
    got = d.cpu().numpy()
    nbad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert nbad == 0, f"{nbad} values differ"
    assert np.array_equal(fit.view(np.uint64), wfit.view(np.uint64))
