"""Scenes for the HSL equalizer and saturation / vibrance tests (CPU models and GPU comparisons).  Test infrastructure, numpy only."""
import numpy as np

from test_gpu_hsl import scene


def wild_scene(w, h, seed):
    """test_gpu_hsl.scene (smooth, every value >= 10, nothing above ~37 000) plus what that scene never holds.  The blocks sit at fractions of
    the frame so that 37 x 29 has all of them, each at least 3 x 2 pixels, none on a multiple of four columns:
      - achromatic (r == g == b, three levels): u and v are the rounding residue of Y alone; at level 0 they are exact zeros, xatan2f(0, 0)
      - negative in every channel: negative luminance, hue on the far side
      - 1.5 x 65535 in every channel, and in the red channel alone (chroma above 1 after normalizeFloatTo1)
      - exact zeros in every channel
      - single pixels with one negative channel, spread over the frame."""
    img = [p.copy() for p in scene(w, h, seed)]
    rng = np.random.default_rng(seed + 1000)
    bw, bh = max(3, w // 7), max(2, h // 8)

    def block(k):
        x0, y0 = 1 + (k % 3) * (w // 3), 1 + (k // 3) * (h // 3)
        return slice(y0, min(y0 + bh, h)), slice(x0, min(x0 + bw, w))

    grey = block(0)
    for p in img:
        p[grey] = img[1][grey]
    img[0][grey][:1] = img[1][grey][:1] = img[2][grey][:1] = 12345.0
    neg = block(1)
    for p in img:
        p[neg] = -0.25 * p[neg]
    white = block(2)
    for p in img:
        p[white] = np.float32(1.5 * 65535.0)
    red = block(3)
    img[0][red] = np.float32(1.5 * 65535.0)
    zero = block(4)
    for p in img:
        p[zero] = 0.0
    for k in range(max(6, w * h // 400)):
        yy, xx = int(rng.integers(0, h)), int(rng.integers(0, w))
        if not any(s[0].start <= yy < s[0].stop and s[1].start <= xx < s[1].stop for s in (grey, neg, white, red, zero)):
            img[k % 3][yy, xx] = np.float32(-rng.uniform(1.0, 9000.0))
    return img
