"""Float64 oracle of the pattern correction ("Pattern correction") and the
seeded generator of the raw detector patterns its tests use.  Plain numpy: a restatement of
the definition, not of the kernels."""
import functools

import numpy as np

MODES = {None: 0, "subtract": 1, "divide": 2}


def crop_offset(size, crop):
    """Source offset of the centre crop (crop <= size): round half to even."""
    return int(round((size - crop) / 2.0))


def taps64(sigma):
    """(one-sided float64 taps (r + 1,), r): exp(-i^2 / 2 sigma^2) / sum over -r..r."""
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi /= phi.sum()
    return phi[r:], r


def _blur_axis(a, taps, r, axis):
    """Correlation with the symmetric taps along one axis, border d c b a | a b c d."""
    n = a.shape[axis]
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    p = np.pad(a, pad, mode="symmetric")
    out = np.zeros_like(a, dtype=np.float64)
    for i in range(-r, r + 1):
        out += taps[abs(i)] * np.take(p, np.arange(r + i, r + i + n), axis=axis)
    return out


def blur(s, sigma, round_taps=False):
    """G_sigma * s over the last two axes, x (last axis) first, then y.  With round_taps the taps
    are the float32-rounded ones the device receives."""
    taps, r = taps64(sigma)
    if round_taps:
        taps = taps.astype(np.float32).astype(np.float64)
    s = np.asarray(s, dtype=np.float64)
    return _blur_axis(_blur_axis(s, taps, r, -1), taps, r, -2)


def correct(raw, size, static_bg=None, static_mode=None, sigma=None, dynamic_mode=None):
    """The definition on raw (B, H0, W0): returns a dict with out (B, 1, h, w) float64 and the
    intermediates s, b, d (B, h, w) the conditioning asserts look at."""
    raw = np.asarray(raw)
    B, H0, W0 = raw.shape
    h, w = size
    assert H0 >= h and W0 >= w
    t, l = crop_offset(H0, h), crop_offset(W0, w)
    v = raw[:, t:t + h, l:l + w].astype(np.float32)
    v = np.where(np.isfinite(v), v, np.float32(0)).astype(np.float64)
    sm = MODES[static_mode] if static_bg is not None else 0
    dm = MODES[dynamic_mode] if sigma is not None else 0
    s = v
    if sm:
        bg = np.asarray(static_bg, dtype=np.float32)[t:t + h, l:l + w].astype(np.float64)
        s = v - bg if sm == 1 else v / bg
    b = blur(s, sigma, round_taps=True) if dm else np.zeros_like(s)
    if dm == 1:
        d = s - b
    elif dm == 2:
        d = np.where(b == 0, 0.0, s / np.where(b == 0, 1.0, b))
    else:
        d = s
    lo = d.min(axis=(1, 2), keepdims=True)
    hi = d.max(axis=(1, 2), keepdims=True)
    span = np.where(hi == lo, 1.0, hi - lo)
    out = np.where(hi == lo, 0.0, (d - lo) / span)
    return dict(out=out[:, None], s=s, b=b, d=d, lo=lo.ravel(), hi=hi.ravel())


def assert_well_conditioned(ref, dynamic_divide):
    """What keeps the parity gate away from ill-conditioned cases: the rescale does not magnify
    rounding ((hi - lo) >= 0.1 max|d| per pattern), and a dynamic divide does not divide by a
    blur near zero (min|b| >= 0.25 max|s|)."""
    dmax = np.abs(ref["d"]).max(axis=(1, 2))
    assert ((ref["hi"] - ref["lo"]) >= 0.1 * dmax).all(), (ref["hi"] - ref["lo"], dmax)
    if dynamic_divide:
        bmin = np.abs(ref["b"]).min(axis=(1, 2))
        smax = np.abs(ref["s"]).max(axis=(1, 2))
        assert (bmin >= 0.25 * smax).all(), (bmin, smax)


@functools.lru_cache(maxsize=None)
def detector_patterns(B, h, w, seed=0):
    """(raw (B, h, w) uint8, bg (h, w) float64): a smooth background, two sets of bands and
    noise, like a raw detector pattern.  Read-only: shared between tests."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    bg = 120.0 + 80.0 * np.exp(-(((y - 0.47 * h) / (0.6 * h)) ** 2 + ((x - 0.53 * w) / (0.7 * w)) ** 2))
    bands = 12.0 * np.sin(0.4 * x + 0.2 * y) + 8.0 * np.sin(0.31 * y - 0.17 * x)
    raw = bg + bands + 3.0 * rng.standard_normal((B, h, w))
    raw = np.clip(raw, 0, 255).astype(np.uint8)
    raw.setflags(write=False)
    bg.setflags(write=False)
    return raw, bg


def static_background(bg, static_mode):
    """The static background of a test case: bg itself, half of it under subtract (so that s
    stays well away from 0)."""
    return (0.5 * bg if static_mode == "subtract" else bg).astype(np.float32)
