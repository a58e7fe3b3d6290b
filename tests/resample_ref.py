"""Float64 restatement of the detector resample ("Detector resampling"),
two independent evaluations of the same area mean, a float32 restatement of the device's fma
chains, and the seeded inputs the resample tests share.  Plain numpy: a restatement of the
definition, not of the kernel."""
import functools

import numpy as np

import correction_ref as C

# (H0, W0), roi or None (the default window), (h, w): the smallest shapes at which each mechanism
# of the kernel can go wrong (tests/test_gpu_resample.py says which)
PARITY_SHAPES = [
    ((60, 60), None, (16, 16)),
    ((50, 70), (3, 5, 45, 61), (12, 16)),
    ((128, 128), None, (16, 16)),
    ((39, 39), None, (32, 32)),
    ((31, 64), (0, 0, 31, 64), (8, 8)),
    ((129, 129), None, (128, 128)),
]
DTYPES = ("uint8", "float32", "float64")


def crop_offset(size, crop):
    return C.crop_offset(size, crop)


def default_roi(H0, W0, h, w):
    """The centred largest window of the output's aspect ratio."""
    g = int(np.gcd(h, w))
    m = min(H0 // (h // g), W0 // (w // g))
    rh, rw = m * (h // g), m * (w // g)
    return crop_offset(H0, rh), crop_offset(W0, rw), rh, rw


def overlap(R, O, rounded=True):
    """Dense (O, R) float64 overlap matrix of one axis: source pixel x overlaps output pixel j
    by max(0, min((j + 1) R, (x + 1) O) - max(j R, x O)) / O.  With `rounded` every quotient is
    the float32-rounded one the device receives."""
    j = np.arange(O, dtype=np.int64)[:, None]
    x = np.arange(R, dtype=np.int64)[None, :]
    num = np.minimum((j + 1) * R, (x + 1) * O) - np.maximum(j * R, x * O)
    wt = np.maximum(num, 0).astype(np.float64) / float(O)
    return wt.astype(np.float32).astype(np.float64) if rounded else wt


def load(raw, roi):
    """Step 1: the region as float32, non-finite -> 0, returned as float64."""
    t, l, rh, rw = roi
    v = np.asarray(raw)[..., t:t + rh, l:l + rw].astype(np.float32)
    return np.where(np.isfinite(v), v, np.float32(0)).astype(np.float64)


def denominator(roi, size, divisor=1.0):
    return np.float32((roi[2] / size[0]) * (roi[3] / size[1]) * float(divisor))


def resample(raw, roi, size, divisor=1.0, rounded=True):
    """The definition on raw (B, H0, W0): out (B, 1, h, w) float64.  `rounded`: the weights and
    the denominator are the float32 values of the contract; without it the exact area mean."""
    h, w = size
    u = load(raw, roi)
    wy, wx = overlap(roi[2], h, rounded), overlap(roi[3], w, rounded)
    s = wy @ u @ wx.T
    den = float(denominator(roi, size, divisor)) if rounded else \
        (roi[2] / h) * (roi[3] / w) * float(divisor)
    return (s / den)[:, None]


def resample_block_mean(raw, roi, size, divisor=1.0):
    """Integer factors only: reshape(h, k, w, l).mean."""
    h, w = size
    u = load(raw, roi)
    k, l = roi[2] // h, roi[3] // w
    assert k * h == roi[2] and l * w == roi[3]
    return u.reshape(u.shape[0], h, k, w, l).mean(axis=(2, 4))[:, None] / float(divisor)


def _cumulative(a, R, O, axis):
    """The integral of the piecewise-constant signal a (R pixels along `axis`) from 0 to the
    output pixel edges j R / O, j = 0 .. O: whole pixels from a running sum, the fraction of the
    pixel an edge falls into on top."""
    a = np.moveaxis(a, axis, -1)
    run = np.concatenate([np.zeros(a.shape[:-1] + (1,)), np.cumsum(a, axis=-1)], axis=-1)
    pad = np.concatenate([a, np.zeros(a.shape[:-1] + (1,))], axis=-1)
    e = np.arange(O + 1, dtype=np.int64) * R
    fl, frac = e // O, (e % O).astype(np.float64) / O
    return np.moveaxis(run[..., fl] + frac * pad[..., fl], -1, axis)


def resample_summed_area(raw, roi, size, divisor=1.0):
    """The same integral through a summed-area table: differences of the cumulative integral at
    the output pixel edges, over the output pixel's area in source pixels."""
    h, w = size
    u = load(raw, roi)
    f = _cumulative(_cumulative(u, roi[2], h, 1), roi[3], w, 2)
    box = f[:, 1:, 1:] - f[:, :-1, 1:] - f[:, 1:, :-1] + f[:, :-1, :-1]
    return (box / ((roi[2] / h) * (roi[3] / w) * float(divisor)))[:, None]


def _fma32(a, b, c):
    """float32 fma of float32 arrays: the product is exact in float64, the sum rounds to 53 bits
    and then to 24 (a double rounding only where the float64 sum is a float32 tie)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def resample_chain32(raw, roi, size, divisor, axis_tables):
    """The device's arithmetic in numpy float32: `axis_tables(R, O)` gives (start, weights) as
    latice.data_module.resample_axis does; x pass, y pass (fma chains from 0, taps ascending),
    one float32 division."""
    h, w = size
    u = load(raw, roi).astype(np.float32)
    ys, yw = axis_tables(roi[2], h)
    xs, xw = axis_tables(roi[3], w)
    r = np.zeros(u.shape[:2] + (w,), np.float32)
    for t in range(xw.shape[1]):
        r = _fma32(xw[None, None, :, t], u[:, :, xs + t], r)
    s = np.zeros((u.shape[0], h, w), np.float32)
    for t in range(yw.shape[1]):
        s = _fma32(yw[None, :, t, None], r[:, ys + t, :], s)
    return (s / denominator(roi, size, divisor))[:, None]


def gate(xtaps, ytaps, vmax, divisor=1.0):
    """max |out - ref| allowed: 2 (xtaps + ytaps + 4) 2^-24 max|v| / divisor.  Each fma rounds
    once against a partial sum no larger than the final one (weights and values are
    non-negative up to the sign of v); the weights, the denominator and the division round once
    each; the factor 2 covers the sum of the weights exceeding the denominator by rounding."""
    return 2.0 * (xtaps + ytaps + 4) * 2.0 ** -24 * float(vmax) / float(divisor)


@functools.lru_cache(maxsize=None)
def patterns(B, H0, W0, dtype="uint8", roi=None):
    """Seeded detector patterns (read-only): uint8 as correction_ref.detector_patterns makes
    them; float ones scaled by 1.37, with a NaN and an Inf inside `roi`."""
    raw, _ = C.detector_patterns(B, H0, W0, seed=H0 + 3 * W0)
    if dtype == "uint8":
        return raw
    raw = raw.astype(dtype) * np.asarray(1.37, dtype)
    t, l, rh, rw = roi if roi is not None else (0, 0, H0, W0)
    raw[0, t + rh // 3, l + rw // 2] = np.nan
    raw[B - 1, t + rh - 1, l] = np.inf
    raw.setflags(write=False)
    return raw
