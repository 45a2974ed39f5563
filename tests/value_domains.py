"""Frames outside the value domain of art_amd/synth.py::bayer_frame (integers in [0, 65535], one mid-grey scene): what rawData holds after
black subtraction (negatives), float gains (fractions, values above 65535 with clipping off), dead strips and blown skies (constant over whole
tiles), and the corners of fp32 itself (-0.0, subnormals, products that underflow or approach 1e21).  Every family is a function of ONE
bayer_frame (seed 3, noise 1500), computed in float64 and cast once, so it is the same on every host.  Test infrastructure, numpy only; the
fuzzers under scripts/ draw from here with --family."""
from __future__ import annotations

import numpy as np

from art_amd import synth

NAMES = ("dark_offset", "scaled_frac", "zero_and_sat_blocks", "all_zero", "constant", "tiny", "tiny2", "negzero", "huge", "mixed_zeros", "small")
_TINY_NORMAL = float(np.finfo(np.float32).tiny)      # 2^-126: below it (and above 0) a float32 is subnormal


def derive(name: str, base: np.ndarray) -> np.ndarray:
    """The family `name` of `base` (a frame of synth.bayer_frame's domain), float32."""
    b = np.asarray(base, dtype=np.float64)
    h, w = b.shape
    if name == "dark_offset":                # black-subtracted dark frame: ~63 % negatives, fractional, |v| < 600
        v = (b - 20000.0) * 0.013
    elif name == "scaled_frac":              # float gains: fractional, a few negatives, up to ~89 000
        v = b * 1.3718 - 511.37
    elif name == "zero_and_sat_blocks":      # dead strip / blown sky wider than a tile's reach, edges off the tile grids
        v = b.copy()
        v[h // 4:h // 2, w // 4:w // 2] = 0.0
        v[h // 2:3 * h // 4, w // 2:3 * w // 4] = 65535.0
    elif name == "all_zero":
        v = np.zeros_like(b)
    elif name == "constant":                 # zero variance in every window
        v = np.full_like(b, 12345.0)
    elif name == "tiny":                     # subnormal inputs at the dark end, all below 6.6e-37: subnormal differences and products
        v = b * 1e-41
    elif name == "tiny2":                    # normal inputs whose squares and products underflow
        v = b * 3e-24
    elif name == "negzero":                  # sign of zero, isolated zeros at full contrast
        v = np.where(np.random.default_rng(7).random((h, w)) < 0.3, -0.0, b)
    elif name == "mixed_zeros":              # zeros of BOTH signs side by side (30 % each): the only finite operands on which a min / max tie shows
        r = np.random.default_rng(7).random((h, w))
        v = np.where(r < 0.3, -0.0, np.where(r < 0.6, 0.0, b))
    elif name == "small":                    # between tiny2 and dark_offset, up to 1e-9: squares normal, fifth powers (the shrink update c x sf^2, sf ~ c^2) subnormal
        v = b * 1.5e-14
    elif name == "huge":                     # products near 1e21, far above every LUT
        v = b * 1e6
    else:
        raise KeyError(name)
    return np.ascontiguousarray(v.astype(np.float32))


def base_frame(w: int, h: int, filters: int, xtrans=None) -> np.ndarray:
    return synth.bayer_frame(w, h, filters, seed=3, noise=1500, xtrans=xtrans)


def family(name: str, w: int, h: int, filters: int, xtrans=None) -> np.ndarray:
    return derive(name, base_frame(w, h, filters, xtrans))


def families(w: int, h: int, filters: int, xtrans=None):
    """(name, float32 frame) for every family, all derived from one base frame."""
    base = base_frame(w, h, filters, xtrans)
    for name in NAMES:
        yield name, derive(name, base)


def describe(frame) -> dict:
    """What a frame (or any float32 array, a stage's output included) holds of the things bayer_frame never produces."""
    a = np.asarray(frame, dtype=np.float32)
    mag = np.abs(a)
    return {
        "n": int(a.size),
        "negatives": int((a < 0).sum()),
        "non_integers": int((a != np.floor(a)).sum()),
        "zeros": int((a == 0).sum()),                                   # both signs
        "neg_zeros": int(((a == 0) & np.signbit(a)).sum()),
        "subnormals": int(((mag > 0) & (mag < _TINY_NORMAL)).sum()),
        "min": float(a.min()),
        "max": float(a.max()),
    }


def report_mismatch(got, want, what: str, limit: int = 5):
    """None if the two float32 arrays agree in every bit; else the text of the failure: count, first coordinates, both values in hex (so that
    a zero's sign, a subnormal and a one-ulp difference can be told apart at a glance)."""
    g = np.ascontiguousarray(got, dtype=np.float32)
    w = np.ascontiguousarray(want, dtype=np.float32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    gu, wu = g.view(np.uint32), w.view(np.uint32)
    bad = gu != wu
    if not bad.any():
        return None
    rows = []
    for idx in np.argwhere(bad)[:limit]:
        i = tuple(int(v) for v in idx)
        rows.append(f"{i}: got {int(gu[i]):#010x} ({float(g[i])!r}) want {int(wu[i]):#010x} ({float(w[i])!r})")
    return f"{what}: {int(bad.sum())} of {bad.size} values differ; " + "; ".join(rows)
