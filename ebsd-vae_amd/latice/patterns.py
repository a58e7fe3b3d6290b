"""The device pattern stages between a raw scan and the encoder.  None of this has a counterpart
in the reference, whose one transform (`DPdataset.__getitem__`) `latice.data_module` mirrors.

    ingest_patterns / ingest_patterns_u8   the DPdataset transform of a whole batch in one
                                           launch (csrc/ingest.hip)
    correct_patterns(PatternCorrection)    static and dynamic background, per-pattern rescale
                                           (csrc/correct.hip); accumulate_patterns sums a scan
                                           into its mean pattern, the usual static background
    resample_patterns(DetectorResample)    detector binning, the exact area mean
                                           (csrc/resample.hip), in front of either ingest
    average_neighbour_patterns / _range    averaging over the scan grid (NeighbourAverage,
                                           csrc/neighbour.hip), between ingest and encoder
    nlpar_patterns / _weights / _range     non-local pattern averaging: the same window with
                                           weights from the pattern distances (NLPAR,
                                           csrc/nlpar.hip), in the averaging's place
    ScanIngest                             the per-scan plan `index_scan` runs every staged
                                           batch through: checks, route and intermediate once

Every entry point takes host or device patterns, checks shapes and sizes before anything touches
the device (`_batch`, `_stage`), uploads its tables once per (object, device) into the object's
`_device_state`, and raises where there is no ROCm device: no CPU fallback.
`latice.data_module` re-exports every public name here.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _native as N

_SRC_CODES = {torch.float64: 0, torch.float32: 1, torch.uint8: 2}   # src_dtype of the C entries


def _batch(raw, who: str, accept=_SRC_CODES, names: str = "uint8, float32 or float64"):
    """`raw` as a (B, H0, W0) tensor of an accepted dtype, where it lies (host or device); one
    (H0, W0) pattern is a batch of one."""
    t = torch.as_tensor(raw)
    if t.dtype not in accept:
        raise TypeError(f"{who} needs {names} patterns, got {t.dtype}")
    if t.ndim == 2:
        t = t.unsqueeze(0)
    if t.ndim != 3:
        raise ValueError(f"patterns must be (B, H, W), got {tuple(t.shape)}")
    return t


def _stage(t: torch.Tensor, who: str, device, h: int, w: int, out: torch.Tensor | None):
    """The last step in front of the library, after every size check: `out` is checked, the
    batch moves to `device`.  Returns (the contiguous device batch, out or a new (B, 1, h, w))."""
    B = t.shape[0]
    if out is not None and (out.numel() != B * h * w or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous ({B}, 1, {h}, {w}) tensor, got {tuple(out.shape)}")
    t = t.to(device, non_blocking=True).contiguous()
    if not t.is_cuda:
        raise RuntimeError(f"{who} needs a ROCm device (no CPU fallback)")
    if out is None:
        out = torch.empty(B, 1, h, w, dtype=torch.float32, device=t.device)
    return t, out


def ingest_patterns(raw, image_size=(128, 128), device="cuda", out: torch.Tensor | None = None):
    """Batched DPdataset transform on the device: raw (B, H0, W0) -> (B, 1, h, w) float32."""
    t = torch.as_tensor(raw)
    if t.dtype not in (torch.float64, torch.float32):
        t = t.to(torch.float64)   # data_module.py:132 casts every pattern to float64
    t = _batch(t, "ingest_patterns")
    h, w = image_size
    t, out = _stage(t, "ingest_patterns", device, h, w, out)
    B, H0, W0 = t.shape
    N.call("ebsdvae_ingest_patterns", t.data_ptr(), _SRC_CODES[t.dtype], B, H0, W0, h, w,
           N.ptr(out), N.stream(t.device))
    return out


def ingest_patterns_u8(raw, image_size=(128, 128), device="cuda", out: torch.Tensor | None = None):
    """The same transform for detector data that already is uint8: raw (B, H0, W0) uint8 ->
    (B, 1, h, w) float32 = float32(v) / 255 after the centre crop / zero pad, bit-identical to
    `ingest_patterns(raw / 255.0)`.  (`ingest_patterns` itself reads a uint8 array as raw
    values, as the reference's astype(float64) does, and clamps them to 1.)"""
    t = _batch(raw, "ingest_patterns_u8", (torch.uint8,), "uint8")
    h, w = image_size
    t, out = _stage(t, "ingest_patterns_u8", device, h, w, out)
    B, H0, W0 = t.shape
    N.call("ebsdvae_ingest_patterns_u8", t.data_ptr(), B, H0, W0, h, w, N.ptr(out),
           N.stream(t.device))
    return out


# ---------------------------------------------------------------- background correction
_MODES = {"subtract": 1, "divide": 2}
MAX_CORRECTED_SIDE = 256   # ebsdvae_correct_patterns' window limit per axis


def gaussian_taps(sigma: float) -> tuple[np.ndarray, int]:
    """One-sided taps of `scipy.ndimage.gaussian_filter(sigma, truncate=4.0)`: radius
    r = int(4 sigma + 0.5) and exp(-i^2 / 2 sigma^2) / sum over -r..r for i = 0..r, computed in
    float64 and rounded to float32.  Returns (taps (r + 1,) float32, r)."""
    sigma = float(sigma)
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise ValueError(f"sigma must be a positive finite number, got {sigma}")
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi /= phi.sum()
    return phi[r:].astype(np.float32), r


def _crop_offset(size: int, crop: int) -> int:
    """Source offset of the centre crop along one axis (crop <= size): round((size - crop) / 2),
    half to even, as torchvision's center_crop and csrc/crop.h."""
    return int(round((size - crop) / 2.0))


@dataclass(frozen=True, eq=False)
class PatternCorrection:
    """Background correction of raw detector patterns, applied by `correct_patterns` on the
    cropped window: static background (subtract or divide by the (H0, W0) pattern
    `static_background`, e.g. `DiffractionPatternIndexer.scan_background`), then dynamic
    background (subtract or divide by the pattern's own Gaussian blur of `dynamic_sigma` pixels,
    border "reflect", truncated at 4 sigma), then a rescale of every pattern to [0, 1].  A step
    whose parameter is None is skipped; the rescale always runs."""

    static_background: np.ndarray | None = None
    static_mode: str = "subtract"
    dynamic_sigma: float | None = None
    dynamic_mode: str = "subtract"
    # per device: the uploaded background and taps (filled by correct_patterns)
    _device_state: dict = field(default_factory=dict, init=False, repr=False)

    def __post_init__(self):
        for name in ("static_mode", "dynamic_mode"):
            if getattr(self, name) not in _MODES:
                raise ValueError(f"{name} must be 'subtract' or 'divide', got {getattr(self, name)!r}")
        if self.static_background is not None:
            bg = np.array(self.static_background, dtype=np.float32, order="C")   # a private copy
            if bg.ndim != 2:
                raise ValueError(f"static_background must be a 2-D (H0, W0) pattern, got shape {bg.shape}")
            if not np.isfinite(bg).all():
                raise ValueError("static_background holds non-finite values")
            bg.setflags(write=False)
            object.__setattr__(self, "static_background", bg)
        if self.dynamic_sigma is not None:
            sigma = float(self.dynamic_sigma)
            if not (sigma > 0.0 and math.isfinite(sigma)):
                raise ValueError(f"dynamic_sigma must be a positive finite number, got {self.dynamic_sigma}")
            object.__setattr__(self, "dynamic_sigma", sigma)

    @property
    def static_code(self) -> int:
        return 0 if self.static_background is None else _MODES[self.static_mode]

    @property
    def dynamic_code(self) -> int:
        return 0 if self.dynamic_sigma is None else _MODES[self.dynamic_mode]

    def check(self, H0: int, W0: int, h: int, w: int, resample: DetectorResample | None = None) -> None:
        """Everything that depends on the pattern and window sizes; raises ValueError.  The
        window of the (H0, W0) patterns that reaches the correction is the centre crop, or with
        a `resample` its region, binned to (h, w): the resample's own checks run first, the
        static background stays at detector shape (H0, W0) and, under "divide", must be positive
        inside the window, and `dynamic_sigma` is in pixels of the (h, w) patterns."""
        if resample is not None:
            resample.check(H0, W0, h, w)
            t, l, wh, ww = resample.window(H0, W0, h, w)
            inside, unit, side = "resampled region", " (in output pixels)", "output"
        else:
            if h > H0 or w > W0:
                raise ValueError(f"the ({h}, {w}) window does not fit ({H0}, {W0}) patterns "
                                 "(the corrected ingest crops, it does not pad)")
            if not (0 < h <= MAX_CORRECTED_SIDE and 0 < w <= MAX_CORRECTED_SIDE):
                raise ValueError(f"the window ({h}, {w}) must lie within "
                                 f"({MAX_CORRECTED_SIDE}, {MAX_CORRECTED_SIDE})")
            t, l, wh, ww = _crop_offset(H0, h), _crop_offset(W0, w), h, w
            inside, unit, side = "cropped window", "", "window"
        bg = self.static_background
        if bg is not None:
            if bg.shape != (H0, W0):
                raise ValueError(f"static_background is {bg.shape}, the patterns are ({H0}, {W0})")
            if self.static_mode == "divide" and not (bg[t:t + wh, l:l + ww] > 0).all():
                raise ValueError("static_mode 'divide' needs a background that is positive "
                                 f"everywhere inside the {inside}")
        if self.dynamic_sigma is not None:
            r = int(4.0 * self.dynamic_sigma + 0.5)
            if r > min(h, w):
                raise ValueError(f"dynamic_sigma={self.dynamic_sigma}{unit} gives a blur radius of "
                                 f"{r}, more than the {side}'s smaller side {min(h, w)}")

    def _on(self, device: torch.device):
        """(background, taps, radius) on `device`, uploaded on first use."""
        st = self._device_state.get(device)
        if st is None:
            bg = taps = None
            r = 0
            if self.static_background is not None:
                bg = torch.from_numpy(self.static_background.copy()).to(device)   # ours is read-only
            if self.dynamic_sigma is not None:
                t, r = gaussian_taps(self.dynamic_sigma)
                taps = torch.from_numpy(t).to(device)
            st = self._device_state[device] = (bg, taps, r)
        return st


def check_resampled_correction(correction: PatternCorrection, resample: DetectorResample,
                               H0: int, W0: int, h: int, w: int) -> None:
    """The size checks of `correct_patterns(..., resample=resample)`."""
    correction.check(H0, W0, h, w, resample)


# ---------------------------------------------------------------- detector resampling
MAX_RESAMPLED_SIDE = 256    # ebsdvae_resample_patterns' output limit per axis
MAX_RESAMPLE_FACTOR = 8     # ... and its largest region / output ratio per axis


def resample_axis(R: int, O: int) -> tuple[np.ndarray, np.ndarray]:
    """The area-mean tables of one axis: a region of R source pixels onto O output pixels,
    O <= R.  Source pixel x overlaps output pixel j by
    max(0, min((j + 1) R, (x + 1) O) - max(j R, x O)) / O output pixels: an integer numerator,
    the quotient taken in float64 and rounded to float32.  Returns (start (O,) int32, weights
    (O, T) float32): output j sums weights[j, t] * source[start[j] + t] over its T taps,
    T = the largest number of source pixels an output overlaps (at most ceil(R / O) + 1).  An
    output that overlaps fewer has zero weights behind them, or in front where the window would
    otherwise leave the region: every tap lies inside [0, R)."""
    R, O = int(R), int(O)
    if not 1 <= O <= R:
        raise ValueError(f"resample_axis: {R} source pixels onto {O} (downsampling only)")
    j = np.arange(O, dtype=np.int64)
    first = j * R // O                         # floor(j R / O)
    last = ((j + 1) * R + O - 1) // O          # ceil((j + 1) R / O), exclusive
    T = int((last - first).max())
    start = np.minimum(first, R - T)
    x = start[:, None] + np.arange(T, dtype=np.int64)[None, :]
    num = np.minimum((j[:, None] + 1) * R, (x + 1) * O) - np.maximum(j[:, None] * R, x * O)
    weights = (np.maximum(num, 0).astype(np.float64) / float(O)).astype(np.float32)
    return start.astype(np.int32), weights


@dataclass(frozen=True, eq=False)
class DetectorResample:
    """Binning of raw detector patterns to the model's input size, applied by
    `resample_patterns`, `correct_patterns(resample=...)` and `index_scan(resample=...)`: the
    exact area mean (a box filter with fractional pixel overlap) of the region `roi` =
    (top, left, height, width) of the (H0, W0) pattern on the (h, w) output grid, by a factor of
    1 to 8 per axis, independently.  `roi=None` takes the centred largest window of the output's
    aspect ratio: with g = gcd(h, w) and m = min(H0 // (h / g), W0 // (w / g)) the window
    (m h / g, m w / g), at the centre-crop offsets; for a square model the centred square of
    side min(H0, W0)."""

    roi: tuple | None = None
    # per (device, region size, output size): the uploaded tables (filled on first use)
    _device_state: dict = field(default_factory=dict, init=False, repr=False)

    def __post_init__(self):
        if self.roi is not None:
            try:
                roi = tuple(int(v) for v in self.roi)
            except (TypeError, ValueError):
                raise ValueError(f"roi must be (top, left, height, width), got {self.roi!r}") from None
            if len(roi) != 4:
                raise ValueError(f"roi must be (top, left, height, width), got {self.roi!r}")
            object.__setattr__(self, "roi", roi)

    def window(self, H0: int, W0: int, h: int, w: int) -> tuple[int, int, int, int]:
        """The region (top, left, height, width) of an (H0, W0) pattern that goes to (h, w)."""
        if self.roi is not None:
            return self.roi
        H0, W0, h, w = int(H0), int(W0), int(h), int(w)
        if min(H0, W0, h, w) < 1:
            raise ValueError(f"pattern ({H0}, {W0}) / output ({h}, {w}): sizes must be positive")
        g = math.gcd(h, w)
        m = min(H0 // (h // g), W0 // (w // g))
        rh, rw = m * (h // g), m * (w // g)
        return _crop_offset(H0, rh), _crop_offset(W0, rw), rh, rw

    def check(self, H0: int, W0: int, h: int, w: int) -> None:
        """Everything `ebsdvae_resample_patterns` refuses for these sizes; raises ValueError."""
        if not (0 < h <= MAX_RESAMPLED_SIDE and 0 < w <= MAX_RESAMPLED_SIDE):
            raise ValueError(f"the output ({h}, {w}) must lie within "
                             f"({MAX_RESAMPLED_SIDE}, {MAX_RESAMPLED_SIDE})")
        top, left, rh, rw = self.window(H0, W0, h, w)
        if top < 0 or left < 0 or rh < 1 or rw < 1 or top + rh > H0 or left + rw > W0:
            raise ValueError(f"the region {(top, left, rh, rw)} leaves the ({H0}, {W0}) patterns")
        if rh < h or rw < w:
            raise ValueError(f"a ({rh}, {rw}) region is smaller than the ({h}, {w}) output: "
                             "the resample bins down, it does not upsample")
        if rh > MAX_RESAMPLE_FACTOR * h or rw > MAX_RESAMPLE_FACTOR * w:
            raise ValueError(f"a ({rh}, {rw}) region onto ({h}, {w}) is a factor above "
                             f"{MAX_RESAMPLE_FACTOR}")

    def _on(self, device: torch.device, rh: int, rw: int, h: int, w: int):
        """(ystart, ywts, ytaps, xstart, xwts, xtaps) on `device`, built and uploaded once."""
        key = (device, rh, rw, h, w)
        st = self._device_state.get(key)
        if st is None:
            st = ()
            for R, O in ((rh, h), (rw, w)):
                start, wts = resample_axis(R, O)
                st += (torch.from_numpy(start).to(device), torch.from_numpy(wts).to(device),
                       wts.shape[1])
            self._device_state[key] = st
        return st


def resample_denominator(rh: int, rw: int, h: int, w: int, divisor: float = 1.0) -> np.float32:
    """float32((rh / h) (rw / w) divisor), computed in float64: what the weighted sum of a
    resampled pixel is divided by."""
    return np.float32((float(rh) / float(h)) * (float(rw) / float(w)) * float(divisor))


def _check_resample(resample) -> None:
    if not isinstance(resample, DetectorResample):
        raise TypeError(f"resample must be a DetectorResample, got {type(resample).__name__}")


def resample_patterns(raw, image_size=(128, 128), resample: DetectorResample | None = None,
                      divisor: float = 1.0, device="cuda", out: torch.Tensor | None = None):
    """Detector binning on the device: raw (B, H0, W0) or (H0, W0) patterns (uint8, float32 or
    float64, host or device) -> (B, 1, h, w) float32, the area mean of `resample`'s region
    (default: `DetectorResample()`, the centred largest window) on the (h, w) grid, divided by
    `divisor` (255 gives ToTensor's scale for uint8 data, what `ingest_patterns_u8` writes)
    (`ebsdvae_resample_patterns`, csrc/resample.hip).  Non-finite source values count as 0.
    Sizes are checked before anything touches the device; the tables are uploaded once per
    (resample, geometry, device).  No CPU fallback."""
    if resample is None:
        resample = DetectorResample()
    _check_resample(resample)
    t = _batch(raw, "resample_patterns")
    B, H0, W0 = t.shape
    h, w = (int(v) for v in image_size)
    resample.check(H0, W0, h, w)
    divisor = float(divisor)
    if not (divisor > 0.0 and math.isfinite(divisor)):
        raise ValueError(f"divisor must be a positive finite number, got {divisor}")
    t, out = _stage(t, "resample_patterns", device, h, w, out)
    top, left, rh, rw = resample.window(H0, W0, h, w)
    ys, yw, yt, xs, xw, xt = resample._on(t.device, rh, rw, h, w)
    N.call("ebsdvae_resample_patterns", t.data_ptr(), _SRC_CODES[t.dtype], B, H0, W0, top, left,
           rh, rw, h, w, ys.data_ptr(), N.ptr(yw), yt, xs.data_ptr(), N.ptr(xw), xt,
           float(resample_denominator(rh, rw, h, w, divisor)), N.ptr(out), N.stream(t.device))
    return out


def _resampled_background(correction: PatternCorrection, resample: DetectorResample,
                          device: torch.device, H0: int, W0: int, h: int, w: int):
    """The static background binned as the patterns are (float32, divisor 1), (h, w) on
    `device`; computed once per (correction, device, geometry).  None without a background."""
    if correction.static_background is None:
        return None
    key = ("resampled", device, resample.window(H0, W0, h, w), h, w)
    bg = correction._device_state.get(key)
    if bg is None:
        full = torch.from_numpy(correction.static_background.copy())[None]
        bg = resample_patterns(full, (h, w), resample, 1.0, device).view(h, w)
        correction._device_state[key] = bg
    return bg


def correct_patterns(raw, image_size=(128, 128), correction: PatternCorrection | None = None,
                     device="cuda", out: torch.Tensor | None = None,
                     resample: DetectorResample | None = None,
                     intermediate: torch.Tensor | None = None):
    """Background-corrected ingest on the device: raw (B, H0, W0) detector patterns (uint8,
    float32 or float64, host or device) -> (B, 1, h, w) float32 in [0, 1]: centre crop (no
    padding), `correction`'s static and dynamic steps, per-pattern rescale
    (`ebsdvae_correct_patterns`, csrc/correct.hip).  Float sources are raw intensities of any
    scale.  Shapes and sizes are checked before anything touches the device; the background and
    the taps are uploaded once per (correction, device).

    With `resample` (a `DetectorResample`) the patterns are binned to (h, w) first, in place of
    the crop: resample (`resample_patterns`, divisor 1, into a float32 intermediate), static,
    dynamic, rescale; the correction kernel's crop is then the identity.
    `correction.static_background` stays at detector shape (H0, W0) and is
    binned once through the same kernel; under "divide" it must be positive inside the region.
    `dynamic_sigma` is then in output pixels.  `intermediate` may supply the float32 buffer of
    at least B h w elements the binned patterns pass through."""
    if not isinstance(correction, PatternCorrection):
        raise TypeError(f"correction must be a PatternCorrection, got {type(correction).__name__}")
    if resample is not None:
        _check_resample(resample)
    t = _batch(raw, "correct_patterns")
    B, H0, W0 = t.shape
    h, w = (int(v) for v in image_size)
    correction.check(H0, W0, h, w, resample)
    t, out = _stage(t, "correct_patterns", device, h, w, out)
    if resample is not None:
        if intermediate is None:
            mid = torch.empty(B, 1, h, w, dtype=torch.float32, device=t.device)
        else:
            if not (intermediate.is_cuda and intermediate.dtype == torch.float32
                    and intermediate.is_contiguous() and intermediate.numel() >= B * h * w):
                raise ValueError(f"intermediate must be a contiguous float32 device tensor of at least "
                                 f"{B} ({h}, {w}) patterns, got {tuple(intermediate.shape)}")
            mid = intermediate.view(-1)[:B * h * w].view(B, 1, h, w)
        resample_patterns(t, (h, w), resample, 1.0, t.device, out=mid)
        bg = _resampled_background(correction, resample, t.device, H0, W0, h, w)
        _, taps, radius = correction._on(t.device)
        t, H0, W0 = mid, h, w     # what the correction kernel reads: the binned patterns
    else:
        bg, taps, radius = correction._on(t.device)
    nbytes = N.call("ebsdvae_correct_patterns_work", B, h, w)
    work = torch.empty(nbytes, dtype=torch.uint8, device=t.device) if nbytes else None
    N.call("ebsdvae_correct_patterns", t.data_ptr(), _SRC_CODES[t.dtype], B, H0, W0, h, w,
           N.ptr(bg), correction.static_code, N.ptr(taps), radius, correction.dynamic_code,
           N.ptr(out), work.data_ptr() if work is not None else None, N.stream(t.device))
    return out


def accumulate_patterns(raw: torch.Tensor, acc: torch.Tensor) -> torch.Tensor:
    """acc (H0, W0) float64 += the sum over a device batch raw (B, H0, W0) (uint8, float32 or
    float64), each pixel in batch order (`ebsdvae_accumulate_patterns`)."""
    if raw.dtype not in _SRC_CODES:
        raise TypeError(f"accumulate_patterns needs uint8, float32 or float64 patterns, got {raw.dtype}")
    if raw.ndim != 3 or tuple(acc.shape) != tuple(raw.shape[1:]) or acc.dtype != torch.float64:
        raise ValueError(f"patterns {tuple(raw.shape)} / accumulator {tuple(acc.shape)} {acc.dtype}: "
                         "need (B, H0, W0) and a float64 (H0, W0)")
    if not (raw.is_cuda and acc.is_cuda and raw.is_contiguous() and acc.is_contiguous()):
        raise RuntimeError("accumulate_patterns needs contiguous tensors on a ROCm device")
    B, H0, W0 = raw.shape
    N.call("ebsdvae_accumulate_patterns", raw.data_ptr(), _SRC_CODES[raw.dtype], B, H0, W0,
           acc.data_ptr(), N.stream(raw.device))
    return acc


class ScanIngest:
    """How one host scan's staged batches become transformed patterns: built once per scan from
    the source's (H0, W0), its staging dtype code (the C entries' src_dtype), the model's
    `image_size`, the device, the largest batch and the scan's `correction` and `resample`.
    Construction runs the type and size checks (nothing has touched the device when one
    raises), fixes `route` and allocates `intermediate`, the float32 buffer of `max_batch`
    patterns that binned float data or a binned corrected scan passes through; the other routes
    have none.  `plan(raw, out)` then runs one staged batch through the route:

        float             ingest_patterns                      the DPdataset transform
        u8                ingest_patterns_u8                   v / 255
        corrected         correct_patterns
        binned_u8         resample_patterns, divisor 255       straight to ToTensor's scale
        binned_float      resample_patterns -> intermediate -> ingest_patterns at equal size
                                                               (its clamp and truncation)
        binned_corrected  correct_patterns(resample=), binned through the intermediate"""

    def __init__(self, source_shape, code: int, image_size, device, max_batch: int,
                 correction: PatternCorrection | None = None,
                 resample: DetectorResample | None = None):
        if resample is not None:
            _check_resample(resample)
        if correction is not None and not isinstance(correction, PatternCorrection):
            raise TypeError(f"correction must be a PatternCorrection, got {type(correction).__name__}")
        (H0, W0), (h, w) = (int(v) for v in source_shape), (int(v) for v in image_size)
        if correction is not None:
            correction.check(H0, W0, h, w, resample)
        elif resample is not None:
            resample.check(H0, W0, h, w)
        size, dev, u8 = (h, w), device, code == _SRC_CODES[torch.uint8]
        self.route = ("binned_" if resample is not None else "") + \
            ("corrected" if correction is not None else "u8" if u8 else "float")
        self.needs_intermediate = self.route in ("binned_float", "binned_corrected")
        self.intermediate = mid = torch.empty(max_batch, 1, h, w, dtype=torch.float32, device=dev) \
            if self.needs_intermediate and max_batch > 0 else None

        def binned_float(raw, out):
            binned = mid.view(-1)[:raw.shape[0] * h * w].view(raw.shape[0], h, w)
            resample_patterns(raw, size, resample, 1.0, dev, out=binned)
            ingest_patterns(binned, size, dev, out=out)

        # plan(raw, out): one staged device batch raw (m, H0, W0), m <= max_batch -> out (m, 1, h, w)
        self.plan = {
            "float": lambda raw, out: ingest_patterns(raw, size, dev, out=out),
            "u8": lambda raw, out: ingest_patterns_u8(raw, size, dev, out=out),
            "corrected": lambda raw, out: correct_patterns(raw, size, correction, dev, out=out),
            "binned_u8": lambda raw, out: resample_patterns(raw, size, resample, 255.0, dev, out=out),
            "binned_float": binned_float,
            "binned_corrected": lambda raw, out: correct_patterns(
                raw, size, correction, dev, out=out, resample=resample, intermediate=mid),
        }[self.route]


# ---------------------------------------------------------------- neighbour pattern averaging
MAX_NEIGHBOUR_SIDE = 5   # ebsdvae_average_neighbours' window limit per axis
_WINDOWS = ("rectangular", "circular", "gaussian")


def _grid_and_window(scan_shape=None, window_shape=None):
    """(scan_shape, window_shape) as tuples of two ints, each checked where it is given: a grid
    of positive sides with fewer than 2^31 patterns, a window of odd sides of at most 5."""
    if scan_shape is not None:
        try:
            rows, cols = (int(v) for v in scan_shape)
        except (TypeError, ValueError):
            raise ValueError(f"scan_shape must be (rows, cols), got {scan_shape!r}") from None
        if rows < 1 or cols < 1 or rows * cols >= 1 << 31:
            raise ValueError(f"scan_shape {scan_shape!r}: rows and cols must be positive "
                             "(and rows * cols below 2^31)")
        scan_shape = (rows, cols)
    if window_shape is not None:
        try:
            ny, nx = (int(v) for v in window_shape)
        except (TypeError, ValueError):
            raise ValueError(f"window_shape must be two integers, got {window_shape!r}") from None
        for v in (ny, nx):
            if not (1 <= v <= MAX_NEIGHBOUR_SIDE and v % 2 == 1):
                raise ValueError(f"window_shape {window_shape!r}: sides must be odd and at most "
                                 f"{MAX_NEIGHBOUR_SIDE}")
        window_shape = (ny, nx)
    return scan_shape, window_shape


class _ScanStage:
    """What the records of the two scan-grid averagings share: each has a `scan_shape` =
    (rows, cols) and an odd-sided `window_shape`."""

    @property
    def half(self) -> tuple[int, int]:
        """(hr, hc): the window reaches hr scan rows and hc scan columns each way."""
        return self.window_shape[0] // 2, self.window_shape[1] // 2

    @property
    def schedule_half(self) -> tuple[int, int]:
        """The half widths of everything an output depends on: what the streaming schedule of
        `index_scan` keeps resident around a chunk."""
        return self.half

    @property
    def reach(self) -> int:
        """hr * cols + hc of `schedule_half`: how far, in flat scan index, the patterns lie that
        an output depends on."""
        hr, hc = self.schedule_half
        return hr * self.scan_shape[1] + hc

    def check(self, n: int) -> None:
        rows, cols = self.scan_shape
        if int(n) != rows * cols:
            raise ValueError(f"the scan has {n} patterns, scan_shape {self.scan_shape} needs "
                             f"{rows * cols}")


def neighbour_window(window: str = "circular", window_shape=(3, 3), std: float = 1.0) -> np.ndarray:
    """A named averaging window of odd shape (2 hr + 1, 2 hc + 1), at most 5 x 5, built in
    float64 over the offsets (a, b) from the centre and rounded to float32: "rectangular" all
    ones, "circular" 1 where a^2 + b^2 <= max(hr, hc)^2 (3 x 3: the five-point cross), "gaussian"
    exp(-(a^2 + b^2) / (2 std^2))."""
    if window not in _WINDOWS:
        raise ValueError(f"window must be one of {_WINDOWS}, got {window!r}")
    _, (ny, nx) = _grid_and_window(window_shape=window_shape)
    std = float(std)
    if not (std > 0.0 and math.isfinite(std)):
        raise ValueError(f"std must be a positive finite number, got {std}")
    hr, hc = ny // 2, nx // 2
    a, b = np.mgrid[-hr:hr + 1, -hc:hc + 1].astype(np.float64)
    r2 = a * a + b * b
    if window == "rectangular":
        wt = np.ones_like(r2)
    elif window == "circular":
        wt = (r2 <= float(max(hr, hc)) ** 2).astype(np.float64)
    else:
        wt = np.exp(-r2 / (2.0 * std * std))
    return wt.astype(np.float32)


@dataclass(frozen=True, eq=False)
class NeighbourAverage(_ScanStage):
    """Averaging of every transformed pattern with its neighbours on the scan grid
    (kikuchipy's `average_neighbour_patterns`), applied by `average_neighbour_patterns` and
    `index_scan(neighbour_average=...)`.  The scan's N = rows * cols patterns lie on the grid
    `scan_shape` = (rows, cols) in row-major order.  The window is the named one
    (`neighbour_window(window, window_shape, std)`) unless `weights`, an explicit odd-sided array
    of at most 5 x 5 finite non-negative weights with a positive centre, is given.  Neighbours
    off the grid are dropped and the remaining weights renormalise; the result is not rescaled."""

    scan_shape: tuple
    window: str = "circular"
    window_shape: tuple = (3, 3)
    std: float = 1.0
    weights: np.ndarray | None = None
    # per device: the uploaded weights (filled on first use)
    _device_state: dict = field(default_factory=dict, init=False, repr=False)

    def __post_init__(self):
        object.__setattr__(self, "scan_shape", _grid_and_window(self.scan_shape)[0])
        if self.weights is None:
            wt = neighbour_window(self.window, self.window_shape, self.std)
        else:
            wt = np.array(self.weights, dtype=np.float32, order="C")   # a private copy
            if wt.ndim != 2 or any(s % 2 == 0 or s > MAX_NEIGHBOUR_SIDE for s in wt.shape):
                raise ValueError(f"weights must be 2-D with odd sides of at most "
                                 f"{MAX_NEIGHBOUR_SIDE}, got shape {wt.shape}")
            if not np.isfinite(wt).all() or (wt < 0).any():
                raise ValueError("weights must be finite and non-negative")
        if not wt[wt.shape[0] // 2, wt.shape[1] // 2] > 0:
            raise ValueError("the centre weight must be positive")
        wt.setflags(write=False)
        object.__setattr__(self, "weights", wt)
        object.__setattr__(self, "window_shape", tuple(wt.shape))

    def _on(self, device: torch.device) -> torch.Tensor:
        """The weights on `device`, uploaded on first use."""
        wt = self._device_state.get(device)
        if wt is None:
            wt = self._device_state[device] = torch.from_numpy(self.weights.copy()).to(device)
        return wt


def _check_ring(ring, out, count: int, who: str, one_message: str | None = None):
    """The ring and `out` of a `*_range` call; returns (cap, h, w).  A ring that is no device
    tensor raises RuntimeError and one of the wrong dtype, shape or strides ValueError; with
    `one_message` both raise RuntimeError with that text."""
    on_device = torch.is_tensor(ring) and ring.is_cuda
    laid_out = on_device and (ring.dtype == torch.float32 and ring.dim() == 4
                              and ring.shape[1] == 1 and ring.is_contiguous())
    if not on_device or (one_message and not laid_out):
        raise RuntimeError(one_message or f"{who} needs a tensor on a ROCm device (no CPU fallback)")
    if not laid_out:
        raise ValueError(f"{who}: patterns must be a contiguous (N, 1, h, w) float32 tensor, got "
                         f"{tuple(ring.shape)} {ring.dtype}")
    cap, _, h, w = ring.shape
    if not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32
            and out.numel() >= count * h * w):
        raise ValueError(f"out must be a contiguous float32 device tensor of at least {count} "
                         f"({h}, {w}) patterns, got {tuple(out.shape)}")
    return cap, h, w


def _resident_scan(x, stage, kind: type, wanted: str, who: str) -> torch.Tensor:
    """The resident scan x (N, 1, h, w) of `who`, checked against its record `stage` (`wanted`
    says what it must be: a `kind`); returns x contiguous."""
    if not isinstance(stage, kind):
        raise TypeError(f"{wanted}, got {type(stage).__name__}")
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"{who} needs a tensor on a ROCm device (no CPU fallback)")
    if x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32:
        raise ValueError(f"patterns must be (N, 1, h, w) float32, got {tuple(x.shape)} {x.dtype}")
    stage.check(x.shape[0])
    return x.contiguous()


def _out_like(x: torch.Tensor, out: torch.Tensor | None) -> torch.Tensor:
    """`out` if it has the resident scan's shape, a new tensor of that shape without one."""
    if out is None:
        return torch.empty_like(x, memory_format=torch.contiguous_format)
    if out.shape != x.shape:
        raise ValueError(f"out must be a {tuple(x.shape)} tensor, got {tuple(out.shape)}")
    return out


def average_neighbour_range(ring: torch.Tensor, neighbour_average: NeighbourAverage, p0: int,
                            count: int, out: torch.Tensor) -> torch.Tensor:
    """out[:count] = the averaged patterns [p0, p0 + count) of the scan (`ebsdvae_average_neighbours`,
    csrc/neighbour.hip).  `ring` (cap, 1, h, w) float32 holds scan pattern q in slot q % cap and
    every on-grid neighbour of the range is resident; a resident scan is its own ring (cap = N).
    `out` is contiguous, holds at least `count` patterns and does not overlap `ring`."""
    cap, h, w = _check_ring(ring, out, count, "average_neighbour_range",
                            "average_neighbour_range needs a contiguous (cap, 1, h, w) float32 "
                            "tensor on a ROCm device (no CPU fallback)")
    hr, hc = neighbour_average.half
    rows, cols = neighbour_average.scan_shape
    N.call("ebsdvae_average_neighbours", N.ptr(ring), cap, rows, cols, int(p0), int(count),
           N.ptr(neighbour_average._on(ring.device)), hr, hc, h, w, N.ptr(out),
           N.stream(ring.device))
    return out


def average_neighbour_patterns(x: torch.Tensor, neighbour_average: NeighbourAverage,
                               out: torch.Tensor | None = None) -> torch.Tensor:
    """A resident scan of transformed patterns x (N, 1, h, w) float32 on the device (what
    `ingest_patterns`, `ingest_patterns_u8` or `correct_patterns` wrote) -> a new tensor of that
    shape in which every pattern is averaged with its neighbours on the scan grid."""
    x = _resident_scan(x, neighbour_average, NeighbourAverage,
                       "neighbour_average must be a NeighbourAverage", "average_neighbour_patterns")
    return average_neighbour_range(x, neighbour_average, 0, x.shape[0], _out_like(x, out))


# ---------------------------------------------------------------- non-local pattern averaging
def _positive(name: str, value) -> float:
    v = float(value)
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"{name} must be a positive finite number, got {value}")
    return v


@dataclass(frozen=True, eq=False)
class NLPAR(_ScanStage):
    """Non-local pattern averaging and re-weighting (Brewick, Wright and Rowenhorst,
    Ultramicroscopy 200, 2019), applied by `nlpar_patterns` and `index_scan(nlpar=...)`: every
    transformed pattern of the `scan_shape` = (rows, cols) grid becomes the weighted mean of the
    on-grid patterns of its `window_shape` window (odd sides of at most 5), each weighted by
    exp(-d / lam^2), d = max((D - n v) / (v sqrt(2 n)), 0), with D the squared distance of the
    two patterns over their n pixels and v the sum of their noise variances.  A variance is
    `sigma`^2, or with `sigma=None` estimated per pattern from its nearest of the 8 surrounding
    patterns, min D / (2 n), and not below `sigma_floor`^2.  With `dthresh` a neighbour whose
    d exceeds it is dropped.  The centre weight is 1; the result is not rescaled."""

    scan_shape: tuple
    window_shape: tuple = (3, 3)
    lam: float = 0.7
    sigma: float | None = None
    sigma_floor: float = 1e-3
    dthresh: float | None = None

    def __post_init__(self):
        scan_shape, window_shape = _grid_and_window(self.scan_shape, self.window_shape)
        object.__setattr__(self, "scan_shape", scan_shape)
        object.__setattr__(self, "window_shape", window_shape)
        object.__setattr__(self, "lam", _positive("lam", self.lam))
        object.__setattr__(self, "sigma_floor", _positive("sigma_floor", self.sigma_floor))
        if self.sigma is not None:
            object.__setattr__(self, "sigma", _positive("sigma", self.sigma))
        if self.dthresh is not None:
            dthresh = float(self.dthresh)
            if not (dthresh >= 0.0 and math.isfinite(dthresh)):
                raise ValueError(f"dthresh must be a non-negative finite number, got {self.dthresh}")
            object.__setattr__(self, "dthresh", dthresh)

    @property
    def schedule_half(self) -> tuple[int, int]:
        """`half` plus one each way: a pattern's weights depend on its neighbours' variances, and
        a variance on that neighbour's own 3 x 3 ring."""
        hr, hc = self.half
        return hr + 1, hc + 1


_WANT_NLPAR = "nlpar must be an NLPAR"


def _nlpar_weights_range(ring: torch.Tensor, nlpar: NLPAR, p0: int, count: int):
    """(weights (count, 2 hr + 1, 2 hc + 1), sigma (count,)) of the outputs [p0, p0 + count)
    out of a ring (`ebsdvae_nlpar_weights`); the scratch is stream-ordered and freed on return."""
    cap, _, h, w = ring.shape
    (hr, hc), (rows, cols) = nlpar.half, nlpar.scan_shape
    nbytes = N.call("ebsdvae_nlpar_work", rows, cols, int(count), hr, hc, h, w)
    if not nbytes:
        raise ValueError(f"nlpar: {count} outputs of ({h}, {w}) patterns on a {rows} x {cols} grid "
                         "are refused (h * w must be a multiple of 4 below 2^24)")
    with torch.cuda.device(ring.device):
        work = torch.empty(nbytes, dtype=torch.uint8, device=ring.device)
        weights = torch.empty(count, 2 * hr + 1, 2 * hc + 1, dtype=torch.float32, device=ring.device)
        sigma = torch.empty(count, dtype=torch.float32, device=ring.device)
    N.call("ebsdvae_nlpar_weights", N.ptr(ring), cap, rows, cols, int(p0), int(count), hr, hc, h, w,
           nlpar.lam, int(nlpar.sigma is not None), nlpar.sigma or 0.0, nlpar.sigma_floor,
           int(nlpar.dthresh is not None), nlpar.dthresh or 0.0, N.ptr(weights), N.ptr(sigma),
           work.data_ptr(), N.stream(ring.device))
    return weights, sigma


def nlpar_range(ring: torch.Tensor, nlpar: NLPAR, p0: int, count: int,
                out: torch.Tensor) -> torch.Tensor:
    """out[:count] = the NLPAR-averaged patterns [p0, p0 + count) of the scan (csrc/nlpar.hip).
    `ring` (cap, 1, h, w) float32 holds scan pattern q in slot q % cap, and every on-grid pattern
    within `nlpar.reach` of the range is resident; a resident scan is its own ring (cap = N).
    `out` is contiguous, holds at least `count` patterns and does not overlap `ring`."""
    if not isinstance(nlpar, NLPAR):
        raise TypeError(f"{_WANT_NLPAR}, got {type(nlpar).__name__}")
    cap, h, w = _check_ring(ring, out, count, "nlpar_range")
    if count == 0:
        return out
    weights, _ = _nlpar_weights_range(ring, nlpar, p0, count)
    (hr, hc), (rows, cols) = nlpar.half, nlpar.scan_shape
    N.call("ebsdvae_nlpar_average", N.ptr(ring), cap, rows, cols, int(p0), int(count),
           N.ptr(weights), hr, hc, h, w, N.ptr(out), N.stream(ring.device))
    return out


def nlpar_weights(x: torch.Tensor, nlpar: NLPAR):
    """The weights NLPAR gives a resident scan x (N, 1, h, w): (weights (N, 2 hr + 1, 2 hc + 1),
    sigma (N,)) as float32 device tensors.  weights[p] is the window of pattern p before the
    normalisation, centre 1: 1 / weights[p].sum() is the share that stays on the pattern itself,
    what one looks at to choose `lam`."""
    x = _resident_scan(x, nlpar, NLPAR, _WANT_NLPAR, "nlpar_weights")
    return _nlpar_weights_range(x, nlpar, 0, x.shape[0])


def nlpar_patterns(x: torch.Tensor, nlpar: NLPAR, out: torch.Tensor | None = None) -> torch.Tensor:
    """A resident scan of transformed patterns x (N, 1, h, w) float32 on the device -> a new
    tensor of that shape (or `out`) in which every pattern is the NLPAR mean of its window."""
    x = _resident_scan(x, nlpar, NLPAR, _WANT_NLPAR, "nlpar_patterns")
    return nlpar_range(x, nlpar, 0, x.shape[0], _out_like(x, out))
