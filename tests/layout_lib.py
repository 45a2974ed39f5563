"""Device images with padded rows, shifted starts and guard rows, for the tests that hand the library a caller's planes IN PLACE.

One channel of ART's PlanarRGBData<float> has a row stride of ceil16(W * 4) bytes (include/artgpu.h), so every width that is no multiple of
four gives a device-resident image rows longer than W.  An arena is one device tensor per plane whose every 32-bit word is first set to
POISON, a quiet NaN with a payload, written through an integer view so that the bits survive; the image is then copied into a window of it.
After the call, check() returns the window's contents and asserts that every word outside it still holds POISON bit for bit: the columns left
of the window (the shift), the columns right of it (the padding) and the guard rows above and below.  Because the poison is a NaN, a kernel
that reads a pad column or a guard row and lets it reach a result shows up in the comparison of the window; one that reads it and discards it
does not, which is fine.

Strides and shifts are multiples of the element size, and the arena always holds every address a kernel that ignored the stride (indexed
with w) or stored one element or one pair past the end of a row would touch: the tests are there to catch wrong values and stray writes, not
to make a kernel fault.  Test infrastructure, numpy and torch only; nothing here knows about the GPU beyond allocating on it."""
from __future__ import annotations

import numpy as np

from art_amd import capi

POISON = 0x7FC0BEEF
DEVICE = "cuda:0"
SHOW = 5


class Layout:
    """rows of w + pad + max(shifts) floats; plane k starts shifts[k] floats into its row; guard_rows full rows above and below each plane.
    pad None: the stride of PlanarRGBData, ceil16(w * 4) bytes (dense when w % 4 == 0).  The planes share the row stride, as the ABI requires,
    but not the alignment of their starts."""

    def __init__(self, pad, shifts=(0, 0, 0), guard_rows=2, name=""):
        self.pad, self.shifts, self.guard_rows, self.name = pad, tuple(int(s) for s in shifts), int(guard_rows), name
        assert self.guard_rows >= 1 and all(s >= 0 for s in self.shifts)

    def stride(self, w):
        pad = ((w * 4 + 15) // 16 * 16) // 4 - w if self.pad is None else self.pad
        return w + pad + max(self.shifts)

    def __repr__(self):
        return self.name or f"Layout({self.pad}, {self.shifts}, {self.guard_rows})"


LAYOUTS = {
    "planar16": Layout(None, (0, 0, 0), name="planar16"),     # the integration's layout
    "odd": Layout(1, (1, 1, 1), name="odd"),                  # starts on an odd float: nothing is 8-byte aligned (odd stride too when w is odd)
    "mixed": Layout(7, (0, 1, 2), name="mixed"),              # the planes disagree about alignment
    "even_off": Layout(6, (2, 2, 2), name="even_off"),        # 8-byte aligned starts that are not 16-byte aligned (even stride when w is even)
}
DENSE = Layout(0, (0, 0, 0), name="dense")


class Arena:
    """what arena() returns: .planes (capi.Plane per plane), .rgb (capi.RGB of the first three), .plane (the first); .bufs / .views are the
    device tensors behind them"""

    def __init__(self, layout, bufs, views, shape):
        self.layout, self.bufs, self.views, self.shape = layout, bufs, views, shape
        self.planes = [capi.device_plane(v) for v in views]

    @property
    def rgb(self):
        assert len(self.planes) >= 3
        return capi.RGB(*self.planes[:3])

    @property
    def plane(self):
        return self.planes[0]


def _shift(layout, k):
    return layout.shifts[k % len(layout.shifts)]


def arena(layout, planes):
    """one device tensor per plane of `planes` (float32 arrays of one shape, or a shape (h, w) to get three planes of poison only: an output)"""
    import torch
    if isinstance(planes, tuple) and len(planes) == 2 and all(isinstance(v, (int, np.integer)) for v in planes):
        h, w = planes
        planes = [None, None, None]
    else:
        planes = [np.array(p, dtype=np.float32, order="C") for p in planes]        # copies: the callers' arrays may be read-only
        h, w = planes[0].shape
        assert all(p.shape == (h, w) for p in planes)
    stride, g = layout.stride(w), layout.guard_rows
    bufs, views = [], []
    for k, p in enumerate(planes):
        words = torch.full((h + 2 * g, stride), POISON, dtype=torch.int32, device=DEVICE)
        buf = words.view(torch.float32)
        s = _shift(layout, k)
        view = buf[g:g + h, s:s + w]
        if p is not None:
            view.copy_(torch.from_numpy(p).to(DEVICE))
        bufs.append(buf)
        views.append(view)
    torch.cuda.synchronize()
    return Arena(layout, bufs, views, (h, w))


def contents(handle):
    """the windows as host arrays"""
    return [v.cpu().numpy().copy() for v in handle.views]


def stray(handle, what=""):
    """None if every word outside the windows still holds POISON; else the text of the failure: how many words changed and the first few
    (plane, row, col) in arena coordinates (the window starts at row guard_rows, column shifts[plane]) with what they hold now"""
    import torch
    h, w = handle.shape
    g = handle.layout.guard_rows
    total, rows = 0, []
    for k, buf in enumerate(handle.bufs):
        words = buf.view(torch.int32).cpu().numpy().view(np.uint32)
        s = _shift(handle.layout, k)
        bad = words != np.uint32(POISON)
        bad[g:g + h, s:s + w] = False
        n = int(bad.sum())
        total += n
        for idx in np.argwhere(bad)[:max(0, SHOW - len(rows))]:
            r, c = int(idx[0]), int(idx[1])
            rows.append(f"(plane {k}, row {r - g}, col {c - s}): {int(words[r, c]):#010x}")
    if not total:
        return None
    return f"{what}: {total} words outside the {w} x {h} window of layout {handle.layout!r} changed; " + "; ".join(rows)


def check(handle, what=""):
    """the windows' contents, after asserting that nothing outside them changed"""
    msg = stray(handle, what)
    assert msg is None, msg
    return contents(handle)


# ---- byte buffers (scanlines): the same idea with a byte pattern ----------------------------------------------------------------------------

BYTE_POISON = 0xA5


def byte_arena(h, rowb, stride, guard_rows=2):
    """a device byte buffer of h rows of `rowb` bytes, `stride` bytes apart, with guard rows above and below, every byte BYTE_POISON; the rows
    are buf[guard_rows:guard_rows + h]"""
    import torch
    assert stride >= rowb
    buf = torch.full(((h + 2 * guard_rows), stride), BYTE_POISON, dtype=torch.uint8, device=DEVICE)
    torch.cuda.synchronize()
    return buf


def byte_check(buf, h, rowb, guard_rows=2, what=""):
    """the h x rowb bytes of the window, after asserting that every other byte still holds BYTE_POISON"""
    a = buf.cpu().numpy()
    bad = a != BYTE_POISON
    bad[guard_rows:guard_rows + h, :rowb] = False
    assert not bad.any(), f"{what}: {int(bad.sum())} bytes outside the rows changed, first at {np.argwhere(bad)[:SHOW].tolist()}"
    return np.ascontiguousarray(a[guard_rows:guard_rows + h, :rowb])
