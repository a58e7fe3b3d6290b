"""Drop-in `latice.data_module` (reference: latice/data_module.py) with the pattern transform
on the MI355X.

The reference converts one pattern at a time on CPU DataLoader workers
(`DPdataset.__getitem__`, data_module.py:122-133, through `create_default_transform`
:17-33: ToPILImage -> Grayscale -> CenterCrop -> ToTensor).  Here the same transform runs as
one HIP launch over a whole batch (`ebsdvae_ingest_patterns`, csrc/ingest.hip: float -> x255
-> uint8 cast, centre crop / zero pad, /255), fed from a memory-mapped .npy through pinned
host buffers that a background thread fills while the GPU works.

Same public names, constructor arguments and behaviour as the reference:

    create_default_transform(image_size)  -> callable: one (H, W) pattern -> (1, h, w) fp32
    DPdataset(path, rot_angles_path, image_size, transform)   data_module.py:36-133
    DPDataModule(path, rot_angles_path, image_size, val_data_ratio, batch_size, n_cpu,
                 seed, transform)                             data_module.py:136-261
        .setup(stage)   random_split(seed) for "fit", the whole set for "test" (:194-213)
        .train_dataloader() / .val_dataloader() / .test_dataloader()
            iterables of (patterns (B, 1, h, w) fp32 ON THE DEVICE, angles (B, 3) float64)
            with len() = number of batches, as torch DataLoaders of the reference's
            collated batches (callers' `data.to(device)` is then a no-op).

Beyond the reference: raw detector patterns are background-corrected on the device by
`correct_patterns(raw, image_size, PatternCorrection(...))` (static and dynamic background,
per-pattern rescale; csrc/correct.hip), the ingest `index_scan(correction=...)` uses, and
transformed patterns are averaged with their neighbours on the scan grid by
`average_neighbour_patterns(x, NeighbourAverage(...))` (csrc/neighbour.hip), the stage
`index_scan(neighbour_average=...)` puts between ingest and encoder.  Detector-size patterns
are binned to the model's input size in front of either ingest by
`resample_patterns(raw, image_size, DetectorResample(...))` (the exact area mean;
csrc/resample.hip), the stage `index_scan(resample=...)` and `correct_patterns(resample=...)` use.

Lightning is optional: DPDataModule subclasses `pl.LightningDataModule` when
pytorch_lightning is importable.  There is no CPU fallback: the transform runs on the ROCm
device or raises.  A user-supplied `transform` (any callable of the reference's kind) is
honoured per pattern, exactly as the reference applies it.
"""
from __future__ import annotations

import logging
import math
import threading
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import random_split

from . import _native as N

try:  # pragma: no cover - depends on the environment
    import pytorch_lightning as pl
    _DMBase = pl.LightningDataModule
except Exception:  # noqa: BLE001
    pl = None
    _DMBase = object

logger = logging.getLogger(__name__)

_DTYPES = {torch.float64: 0, torch.float32: 1}


def _default_device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
        else torch.device("cuda")


def ingest_patterns(raw, image_size=(128, 128), device="cuda", out: torch.Tensor | None = None):
    """Batched DPdataset transform on the device: raw (B, H0, W0) -> (B, 1, h, w) float32."""
    t = torch.as_tensor(raw)
    if t.dtype not in _DTYPES:
        t = t.to(torch.float64)   # data_module.py:132 casts every pattern to float64
    if t.ndim == 2:
        t = t.unsqueeze(0)
    if t.ndim != 3:
        raise ValueError(f"patterns must be (B, H, W), got {tuple(t.shape)}")
    t = t.to(device, non_blocking=True).contiguous()
    if not t.is_cuda:
        raise RuntimeError("ingest_patterns needs a ROCm device (no CPU fallback)")
    B, H0, W0 = t.shape
    h, w = image_size
    if out is None:
        out = torch.empty(B, 1, h, w, dtype=torch.float32, device=t.device)
    N.call("ebsdvae_ingest_patterns", t.data_ptr(), _DTYPES[t.dtype], B, H0, W0, h, w,
           N.ptr(out), N.stream(t.device))
    return out


def ingest_patterns_u8(raw, image_size=(128, 128), device="cuda", out: torch.Tensor | None = None):
    """The same transform for detector data that already is uint8: raw (B, H0, W0) uint8 ->
    (B, 1, h, w) float32 = float32(v) / 255 after the centre crop / zero pad, bit-identical to
    `ingest_patterns(raw / 255.0)`.  (`ingest_patterns` itself reads a uint8 array as raw
    values, as the reference's astype(float64) does, and clamps them to 1.)"""
    t = torch.as_tensor(raw)
    if t.dtype != torch.uint8:
        raise TypeError(f"ingest_patterns_u8 needs uint8 patterns, got {t.dtype}")
    if t.ndim == 2:
        t = t.unsqueeze(0)
    if t.ndim != 3:
        raise ValueError(f"patterns must be (B, H, W), got {tuple(t.shape)}")
    t = t.to(device, non_blocking=True).contiguous()
    if not t.is_cuda:
        raise RuntimeError("ingest_patterns_u8 needs a ROCm device (no CPU fallback)")
    B, H0, W0 = t.shape
    h, w = image_size
    if out is None:
        out = torch.empty(B, 1, h, w, dtype=torch.float32, device=t.device)
    elif out.numel() != B * h * w or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous ({B}, 1, {h}, {w}) tensor, got {tuple(out.shape)}")
    N.call("ebsdvae_ingest_patterns_u8", t.data_ptr(), B, H0, W0, h, w, N.ptr(out),
           N.stream(t.device))
    return out


# ---------------------------------------------------------------- background correction
_SRC_CODES = {torch.float64: 0, torch.float32: 1, torch.uint8: 2}   # src_dtype of the C entries
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

    def check(self, H0: int, W0: int, h: int, w: int) -> None:
        """Everything that depends on the pattern and window sizes; raises ValueError."""
        if h > H0 or w > W0:
            raise ValueError(f"the ({h}, {w}) window does not fit ({H0}, {W0}) patterns "
                             "(the corrected ingest crops, it does not pad)")
        if not (0 < h <= MAX_CORRECTED_SIDE and 0 < w <= MAX_CORRECTED_SIDE):
            raise ValueError(f"the window ({h}, {w}) must lie within "
                             f"({MAX_CORRECTED_SIDE}, {MAX_CORRECTED_SIDE})")
        bg = self.static_background
        if bg is not None:
            if bg.shape != (H0, W0):
                raise ValueError(f"static_background is {bg.shape}, the patterns are ({H0}, {W0})")
            if self.static_mode == "divide":
                t, l = _crop_offset(H0, h), _crop_offset(W0, w)
                if not (bg[t:t + h, l:l + w] > 0).all():
                    raise ValueError("static_mode 'divide' needs a background that is positive "
                                     "everywhere inside the cropped window")
        if self.dynamic_sigma is not None:
            r = int(4.0 * self.dynamic_sigma + 0.5)
            if r > min(h, w):
                raise ValueError(f"dynamic_sigma={self.dynamic_sigma} gives a blur radius of {r}, "
                                 f"more than the window's smaller side {min(h, w)}")

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
    elif not isinstance(resample, DetectorResample):
        raise TypeError(f"resample must be a DetectorResample, got {type(resample).__name__}")
    t = torch.as_tensor(raw)
    if t.dtype not in _SRC_CODES:
        raise TypeError(f"resample_patterns needs uint8, float32 or float64 patterns, got {t.dtype}")
    if t.ndim == 2:
        t = t.unsqueeze(0)
    if t.ndim != 3:
        raise ValueError(f"patterns must be (B, H, W), got {tuple(t.shape)}")
    B, H0, W0 = t.shape
    h, w = (int(v) for v in image_size)
    resample.check(H0, W0, h, w)
    divisor = float(divisor)
    if not (divisor > 0.0 and math.isfinite(divisor)):
        raise ValueError(f"divisor must be a positive finite number, got {divisor}")
    if out is not None and (out.numel() != B * h * w or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous ({B}, 1, {h}, {w}) tensor, got {tuple(out.shape)}")
    t = t.to(device, non_blocking=True).contiguous()
    if not t.is_cuda:
        raise RuntimeError("resample_patterns needs a ROCm device (no CPU fallback)")
    top, left, rh, rw = resample.window(H0, W0, h, w)
    ys, yw, yt, xs, xw, xt = resample._on(t.device, rh, rw, h, w)
    if out is None:
        out = torch.empty(B, 1, h, w, dtype=torch.float32, device=t.device)
    N.call("ebsdvae_resample_patterns", t.data_ptr(), _SRC_CODES[t.dtype], B, H0, W0, top, left,
           rh, rw, h, w, ys.data_ptr(), N.ptr(yw), yt, xs.data_ptr(), N.ptr(xw), xt,
           float(resample_denominator(rh, rw, h, w, divisor)), N.ptr(out), N.stream(t.device))
    return out


def check_resampled_correction(correction: PatternCorrection, resample: DetectorResample,
                               H0: int, W0: int, h: int, w: int) -> None:
    """The size checks of `correct_patterns(..., resample=resample)`: the resample's own, the
    correction's on the (h, w) patterns it then sees, and the static background, which stays at
    detector shape (H0, W0) and, under "divide", must be positive inside the region."""
    resample.check(H0, W0, h, w)
    bg = correction.static_background
    if bg is not None:
        if bg.shape != (H0, W0):
            raise ValueError(f"static_background is {bg.shape}, the patterns are ({H0}, {W0})")
        if correction.static_mode == "divide":
            t, l, rh, rw = resample.window(H0, W0, h, w)
            if not (bg[t:t + rh, l:l + rw] > 0).all():
                raise ValueError("static_mode 'divide' needs a background that is positive "
                                 "everywhere inside the resampled region")
    if correction.dynamic_sigma is not None:
        r = int(4.0 * correction.dynamic_sigma + 0.5)
        if r > min(h, w):
            raise ValueError(f"dynamic_sigma={correction.dynamic_sigma} (in output pixels) gives a "
                             f"blur radius of {r}, more than the output's smaller side {min(h, w)}")


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
    dynamic, rescale.  `correction.static_background` stays at detector shape (H0, W0) and is
    binned once through the same kernel; under "divide" it must be positive inside the region.
    `dynamic_sigma` is then in output pixels.  `intermediate` may supply the float32 buffer of
    at least B h w elements the binned patterns pass through."""
    if not isinstance(correction, PatternCorrection):
        raise TypeError(f"correction must be a PatternCorrection, got {type(correction).__name__}")
    if resample is not None:
        return _correct_resampled(raw, image_size, correction, device, out, resample, intermediate)
    t = torch.as_tensor(raw)
    if t.dtype not in _SRC_CODES:
        raise TypeError(f"correct_patterns needs uint8, float32 or float64 patterns, got {t.dtype}")
    if t.ndim == 2:
        t = t.unsqueeze(0)
    if t.ndim != 3:
        raise ValueError(f"patterns must be (B, H, W), got {tuple(t.shape)}")
    B, H0, W0 = t.shape
    h, w = (int(v) for v in image_size)
    correction.check(H0, W0, h, w)
    if out is not None and (out.numel() != B * h * w or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous ({B}, 1, {h}, {w}) tensor, got {tuple(out.shape)}")
    t = t.to(device, non_blocking=True).contiguous()
    if not t.is_cuda:
        raise RuntimeError("correct_patterns needs a ROCm device (no CPU fallback)")
    bg, taps, radius = correction._on(t.device)
    if out is None:
        out = torch.empty(B, 1, h, w, dtype=torch.float32, device=t.device)
    nbytes = N.call("ebsdvae_correct_patterns_work", B, h, w)
    work = torch.empty(nbytes, dtype=torch.uint8, device=t.device) if nbytes else None
    N.call("ebsdvae_correct_patterns", t.data_ptr(), _SRC_CODES[t.dtype], B, H0, W0, h, w,
           N.ptr(bg), correction.static_code, N.ptr(taps), radius, correction.dynamic_code,
           N.ptr(out), work.data_ptr() if work is not None else None, N.stream(t.device))
    return out


def _correct_resampled(raw, image_size, correction, device, out, resample, intermediate):
    """`correct_patterns` with a `DetectorResample`: bin to (h, w), then the correction kernel on
    the binned patterns (its crop is the identity) with the binned background."""
    if not isinstance(resample, DetectorResample):
        raise TypeError(f"resample must be a DetectorResample, got {type(resample).__name__}")
    t = torch.as_tensor(raw)
    if t.dtype not in _SRC_CODES:
        raise TypeError(f"correct_patterns needs uint8, float32 or float64 patterns, got {t.dtype}")
    if t.ndim == 2:
        t = t.unsqueeze(0)
    if t.ndim != 3:
        raise ValueError(f"patterns must be (B, H, W), got {tuple(t.shape)}")
    B, H0, W0 = t.shape
    h, w = (int(v) for v in image_size)
    check_resampled_correction(correction, resample, H0, W0, h, w)
    if out is not None and (out.numel() != B * h * w or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous ({B}, 1, {h}, {w}) tensor, got {tuple(out.shape)}")
    t = t.to(device, non_blocking=True).contiguous()
    if not t.is_cuda:
        raise RuntimeError("correct_patterns needs a ROCm device (no CPU fallback)")
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
    if out is None:
        out = torch.empty(B, 1, h, w, dtype=torch.float32, device=t.device)
    nbytes = N.call("ebsdvae_correct_patterns_work", B, h, w)
    work = torch.empty(nbytes, dtype=torch.uint8, device=t.device) if nbytes else None
    N.call("ebsdvae_correct_patterns", mid.data_ptr(), _SRC_CODES[torch.float32], B, h, w, h, w,
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


# ---------------------------------------------------------------- neighbour pattern averaging
MAX_NEIGHBOUR_SIDE = 5   # ebsdvae_average_neighbours' window limit per axis
_WINDOWS = ("rectangular", "circular", "gaussian")


def neighbour_window(window: str = "circular", window_shape=(3, 3), std: float = 1.0) -> np.ndarray:
    """A named averaging window of odd shape (2 hr + 1, 2 hc + 1), at most 5 x 5, built in
    float64 over the offsets (a, b) from the centre and rounded to float32: "rectangular" all
    ones, "circular" 1 where a^2 + b^2 <= max(hr, hc)^2 (3 x 3: the five-point cross), "gaussian"
    exp(-(a^2 + b^2) / (2 std^2))."""
    if window not in _WINDOWS:
        raise ValueError(f"window must be one of {_WINDOWS}, got {window!r}")
    try:
        ny, nx = (int(v) for v in window_shape)
    except (TypeError, ValueError):
        raise ValueError(f"window_shape must be two integers, got {window_shape!r}") from None
    for v in (ny, nx):
        if not (1 <= v <= MAX_NEIGHBOUR_SIDE and v % 2 == 1):
            raise ValueError(f"window_shape {window_shape!r}: sides must be odd and at most "
                             f"{MAX_NEIGHBOUR_SIDE}")
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
class NeighbourAverage:
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
        try:
            rows, cols = (int(v) for v in self.scan_shape)
        except (TypeError, ValueError):
            raise ValueError(f"scan_shape must be (rows, cols), got {self.scan_shape!r}") from None
        if rows < 1 or cols < 1 or rows * cols >= 1 << 31:
            raise ValueError(f"scan_shape {self.scan_shape!r}: rows and cols must be positive "
                             "(and rows * cols below 2^31)")
        object.__setattr__(self, "scan_shape", (rows, cols))
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

    @property
    def half(self) -> tuple[int, int]:
        """(hr, hc): the window reaches hr scan rows and hc scan columns each way."""
        return self.weights.shape[0] // 2, self.weights.shape[1] // 2

    @property
    def reach(self) -> int:
        """hr * cols + hc: how far, in flat scan index, a pattern's neighbours lie from it."""
        hr, hc = self.half
        return hr * self.scan_shape[1] + hc

    def check(self, n: int) -> None:
        rows, cols = self.scan_shape
        if int(n) != rows * cols:
            raise ValueError(f"the scan has {n} patterns, scan_shape {self.scan_shape} needs "
                             f"{rows * cols}")

    def _on(self, device: torch.device) -> torch.Tensor:
        """The weights on `device`, uploaded on first use."""
        wt = self._device_state.get(device)
        if wt is None:
            wt = self._device_state[device] = torch.from_numpy(self.weights.copy()).to(device)
        return wt


def average_neighbour_range(ring: torch.Tensor, neighbour_average: NeighbourAverage, p0: int,
                            count: int, out: torch.Tensor) -> torch.Tensor:
    """out[:count] = the averaged patterns [p0, p0 + count) of the scan (`ebsdvae_average_neighbours`,
    csrc/neighbour.hip).  `ring` (cap, 1, h, w) float32 holds scan pattern q in slot q % cap and
    every on-grid neighbour of the range is resident; a resident scan is its own ring (cap = N).
    `out` is contiguous, holds at least `count` patterns and does not overlap `ring`."""
    if not (ring.is_cuda and ring.dtype == torch.float32 and ring.dim() == 4 and ring.shape[1] == 1
            and ring.is_contiguous()):
        raise RuntimeError("average_neighbour_range needs a contiguous (cap, 1, h, w) float32 "
                           "tensor on a ROCm device (no CPU fallback)")
    cap, _, h, w = ring.shape
    if not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32
            and out.numel() >= count * h * w):
        raise ValueError(f"out must be a contiguous float32 device tensor of at least {count} "
                         f"({h}, {w}) patterns, got {tuple(out.shape)}")
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
    if not isinstance(neighbour_average, NeighbourAverage):
        raise TypeError("neighbour_average must be a NeighbourAverage, got "
                        f"{type(neighbour_average).__name__}")
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("average_neighbour_patterns needs a tensor on a ROCm device "
                           "(no CPU fallback)")
    if x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32:
        raise ValueError(f"patterns must be (N, 1, h, w) float32, got {tuple(x.shape)} {x.dtype}")
    neighbour_average.check(x.shape[0])
    if out is None:
        out = torch.empty_like(x, memory_format=torch.contiguous_format)
    elif out.shape != x.shape:
        raise ValueError(f"out must be a {tuple(x.shape)} tensor, got {tuple(out.shape)}")
    return average_neighbour_range(x.contiguous(), neighbour_average, 0, x.shape[0], out)


class PatternTransform:
    """What `create_default_transform(image_size)` returns (data_module.py:17-33): called on
    one pattern -- an (H, W) or (1, H, W) array or tensor -- it returns the (1, h, w) float32
    tensor torchvision's ToPILImage -> Grayscale -> CenterCrop -> ToTensor would, computed on
    the device.  `.batch(raw)` transforms a whole (B, H, W) stack in one launch."""

    def __init__(self, image_size, device=None):
        self.image_size = tuple(image_size) if not isinstance(image_size, int) else (image_size,) * 2
        self.device = torch.device(device) if device is not None else None

    def _dev(self):
        return self.device if self.device is not None else _default_device()

    def __call__(self, pattern):
        t = torch.as_tensor(pattern)
        if t.ndim == 3 and t.shape[0] == 1:
            t = t[0]
        if t.ndim != 2:
            raise ValueError(f"expected one (H, W) pattern, got {tuple(t.shape)}")
        return ingest_patterns(t, self.image_size, self._dev())[0]

    def batch(self, raw):
        return ingest_patterns(raw, self.image_size, self._dev())

    def __repr__(self):
        return f"PatternTransform(image_size={self.image_size}, device={self.device})"


def create_default_transform(image_size: tuple[int, int]) -> PatternTransform:
    """data_module.py:17-33 (ToPILImage -> Grayscale -> CenterCrop(image_size) -> ToTensor)."""
    return PatternTransform(image_size)


def parse_rotation_angles(rot_angles_path) -> np.ndarray:
    """data_module.py:87-116: skip two header lines, whitespace-split "z1 x z2" rows."""
    try:
        with open(rot_angles_path) as f:
            lines = f.readlines()[2:]
        rows = [[a for a in line.strip().split(" ") if a] for line in lines]
        return np.asarray(rows, dtype=float).reshape(-1, 3)
    except FileNotFoundError:
        logger.error(f"Rotation angles file not found: {rot_angles_path}")
        raise
    except Exception as e:  # noqa: BLE001
        raise ValueError(f"Failed to parse rotation angles file: {e}") from e


class DPdataset:
    """data_module.py:36-133.  The pattern file is memory-mapped (the reference loads it
    whole, :70); `rot_angles` is the same pandas DataFrame (z1, x, z2).  Indexing returns
    (transform(pattern) (1, h, w), angles (3,) float64) like the reference; `batch(indices)`
    returns a whole device batch from one pinned copy and one transform launch."""

    def __init__(self, path, rot_angles_path, image_size=(128, 128), transform=None,
                 device=None) -> None:
        path = Path(path)
        try:
            self.ebsp_dataset = np.load(path, mmap_mode="r")
            logger.info(f"Loaded diffraction pattern data from {path}")
        except Exception as e:  # noqa: BLE001
            raise ValueError("Only .npy data files are supported.") from e
        if len(self.ebsp_dataset.shape) != 3:
            raise ValueError("The input dataset should be 3D.")
        self._angles = parse_rotation_angles(rot_angles_path)
        self.image_size = tuple(image_size)
        self.transform = transform or create_default_transform(self.image_size)
        self.device = torch.device(device) if device is not None else None
        self._pinned = None
        self._pinned_free = None   # HIP event: the last device copy out of _pinned finished

    @property
    def rot_angles(self):
        import pandas as pd
        return pd.DataFrame(self._angles, columns=["z1", "x", "z2"])

    def __len__(self) -> int:
        return self.ebsp_dataset.shape[0]

    def __getitem__(self, idx: int):
        dp = np.asarray(self.ebsp_dataset[idx]).astype(np.float64)
        return self.transform(dp), self._angles[idx].copy()

    def _dev(self):
        return self.device if self.device is not None else _default_device()

    def load_raw(self, indices, out: torch.Tensor | None = None) -> torch.Tensor:
        """Raw patterns of `indices` (sorted runs read straight from the memmap) copied into
        the host tensor `out` (pinned) or a new one."""
        idx = np.asarray(indices, dtype=np.int64)
        raw = self.ebsp_dataset[idx]
        if raw.dtype not in (np.float64, np.float32):
            raw = raw.astype(np.float64)
        src = torch.from_numpy(np.ascontiguousarray(raw))
        if out is None:
            return src
        dst = out[: src.numel()].view(src.shape)
        dst.copy_(src)
        return dst

    def to_device(self, host_raw: torch.Tensor) -> torch.Tensor:
        """(B, H0, W0) raw host batch -> (B, 1, h, w) fp32 device batch (DPdataset transform)."""
        if isinstance(self.transform, PatternTransform):
            return ingest_patterns(host_raw, self.image_size, self._dev())
        # a user transform: applied per pattern, as the reference's __getitem__ does
        return torch.stack([torch.as_tensor(self.transform(p.numpy().astype(np.float64)))
                            for p in host_raw]).to(self._dev())

    def batch(self, indices):
        """(patterns (B, 1, h, w) fp32 on device, angles (B, 3) float64) for `indices`."""
        idx = np.asarray(indices, dtype=np.int64)
        shape = (len(idx),) + tuple(self.ebsp_dataset.shape[1:])
        n = int(np.prod(shape))
        dt = torch.float32 if self.ebsp_dataset.dtype == np.float32 else torch.float64
        if self._pinned_free is not None:
            self._pinned_free.synchronize()   # the async copy of the previous batch read it
        if self._pinned is None or self._pinned.numel() < n or self._pinned.dtype != dt:
            self._pinned = torch.empty(n, dtype=dt).pin_memory()
        x = self.to_device(self.load_raw(idx, self._pinned))
        self._pinned_free = torch.cuda.Event()
        self._pinned_free.record()
        return x, self._angles[idx]

    def iter_batches(self, batch_size: int):
        for s in range(0, len(self), batch_size):
            yield self.batch(np.arange(s, min(s + batch_size, len(self))))


class DeviceBatchLoader:
    """The DataLoader of the drop-in DPDataModule: batches of (patterns on the device,
    angles (B, 3) float64 tensor) over a subset of a DPdataset, in order or shuffled per
    epoch.  A background thread reads batch i+1 from the memmap into the second of two
    pinned buffers while batch i is copied and transformed on the device; a buffer is
    refilled only after the device copy out of it has completed (HIP event).

    Order, matching what the reference's `DataLoader(..., shuffle=...)` yields
    (latice/data_module.py:215-261):
      * one process: `DataLoader(shuffle=True)` draws its base seed and then RandomSampler's
        seed from torch's default generator and permutes with a generator seeded by the
        latter; the same draws happen here, so torch.manual_seed(s) gives the same epoch
        order as the reference's loader.
      * torch.distributed initialised with W > 1 ranks (Lightning DDP, which would inject a
        DistributedSampler): each rank takes its DistributedSampler share -- the permutation
        of a generator seeded with seed + epoch (seed = PL_GLOBAL_SEED, as Lightning passes
        it, else 0), padded by wrapping to a multiple of W, then every W-th index from the
        rank's offset -- so the ranks see disjoint batches that cover the epoch.
        `set_epoch(e)` (reached through `.sampler`, where Lightning looks for it) moves to
        epoch e.
    Every torch DataLoader iterator draws a base seed from the default generator when it is
    created -- in order or shuffled, one process or W ranks -- except that a loader with
    persistent workers (the reference's val/test loaders when n_cpu > 0) creates its
    iterator once and draws it on the first iteration only; `persistent` says which.  Both
    draws (base seed, then RandomSampler's) happen when iter() is called, as DataLoader's
    worker iterator prefetches at creation, so later epochs and the other loaders see the
    reference's generator state."""

    def __init__(self, dataset: DPdataset, indices, batch_size: int, shuffle: bool = False,
                 drop_last: bool = False, rank: int | None = None, world: int | None = None,
                 seed: int | None = None, persistent: bool = False):
        self.dataset = dataset
        self.persistent = bool(persistent)
        self._iterated = False
        self.indices = np.asarray(indices, dtype=np.int64)
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.drop_last = bool(drop_last)
        if world is None:
            import torch.distributed as dist
            inited = dist.is_available() and dist.is_initialized()
            world = dist.get_world_size() if inited else 1
            rank = dist.get_rank() if inited else 0
        self.rank, self.world = int(rank or 0), int(world)
        if not 0 <= self.rank < self.world:
            raise ValueError(f"rank {self.rank} outside a world of {self.world}")
        import os
        self.seed = int(os.environ.get("PL_GLOBAL_SEED", 0)) if seed is None else int(seed)
        self.epoch = 0

    @property
    def sampler(self):
        return self

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def _num_local(self) -> int:
        n = len(self.indices)
        return n if self.world == 1 else math.ceil(n / self.world)

    def __len__(self) -> int:
        n = self._num_local()
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def _order(self):
        n = len(self.indices)
        if not (self.persistent and self._iterated):
            torch.empty((), dtype=torch.int64).random_()   # the iterator's base seed
        self._iterated = True
        if self.world > 1:
            # torch.utils.data.DistributedSampler (shuffle, drop_last=False)
            if self.shuffle:
                g = torch.Generator()
                g.manual_seed(self.seed + self.epoch)
                pos = torch.randperm(n, generator=g).numpy()
            else:
                pos = np.arange(n)
            total = self._num_local() * self.world
            if total > n:
                pos = np.concatenate([pos] * (total // n) + [pos[: total % n]])
            return self.indices[pos[self.rank:total:self.world]]
        if not self.shuffle:
            return self.indices
        # after the base seed, RandomSampler.__iter__ draws its own seed
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        g = torch.Generator()
        g.manual_seed(seed)
        return self.indices[torch.randperm(n, generator=g).numpy()]

    def __iter__(self):
        # the generator draws happen here, at iter(), not at the first next()
        return self._batches(self._order())

    def _batches(self, order):
        nb = len(self)
        if nb == 0:
            return
        ds = self.dataset
        shape = tuple(ds.ebsp_dataset.shape[1:])
        dt = torch.float32 if ds.ebsp_dataset.dtype == np.float32 else torch.float64
        per = int(np.prod(shape))
        bufs = [torch.empty(self.batch_size * per, dtype=dt).pin_memory() for _ in range(2)]
        done = [None, None]            # HIP event: device copy out of bufs[k] finished
        ready = [threading.Event(), threading.Event()]
        staged = [None, None]
        err = []

        def fill(i):
            k = i & 1
            try:
                if done[k] is not None:
                    done[k].synchronize()
                sel = np.sort(order[i * self.batch_size:(i + 1) * self.batch_size])
                staged[k] = (ds.load_raw(sel, bufs[k]), sel)
            except Exception as e:  # noqa: BLE001
                err.append(e)
            ready[k].set()

        th = threading.Thread(target=fill, args=(0,), daemon=True)
        th.start()
        for i in range(nb):
            k = i & 1
            ready[k].wait()
            th.join()
            if err:
                raise err[0]
            ready[k].clear()
            host, sel = staged[k]
            x = ds.to_device(host)
            ev = torch.cuda.Event()
            ev.record()
            done[k] = ev
            if i + 1 < nb:
                th = threading.Thread(target=fill, args=(i + 1,), daemon=True)
                th.start()
            yield x, torch.from_numpy(ds._angles[sel])


class DPDataModule(_DMBase):
    """data_module.py:136-261: same arguments, split and loaders; the loaders yield device
    batches (DeviceBatchLoader).  `n_cpu` starts no worker processes (one transform launch
    per batch replaces them); it only decides, as in the reference, whether the val/test
    loaders are persistent, which changes their generator draws."""

    def __init__(self, path, rot_angles_path, image_size=(128, 128), val_data_ratio: float = 0.1,
                 batch_size: int = 32, n_cpu: int = 4, seed: int = 42, transform=None,
                 device=None):
        super().__init__()
        self.path = path
        self.rot_angles_path = rot_angles_path
        self.image_size = tuple(image_size)
        self.val_data_ratio = val_data_ratio
        self.batch_size = batch_size
        self.n_cpu = n_cpu
        self.seed = seed
        self.transform = transform or create_default_transform(self.image_size)
        torch.manual_seed(seed)          # data_module.py:184-186
        np.random.seed(seed)
        self.dataset_full = DPdataset(self.path, self.rot_angles_path, self.image_size,
                                      self.transform, device=device)

    def setup(self, stage: str | None = None) -> None:
        """data_module.py:192-213 (random_split with a generator seeded by `seed`)."""
        if stage == "fit" or stage is None:
            all_size = len(self.dataset_full)
            val_size = int(all_size * self.val_data_ratio)
            train_size = all_size - val_size
            logger.info(f"Splitting dataset: {train_size} training, {val_size} validation samples")
            self.dataset_train, self.dataset_val = random_split(
                self.dataset_full, [train_size, val_size],
                generator=torch.Generator().manual_seed(self.seed))
        if stage == "test":
            self.dataset_test = self.dataset_full
            logger.info(f"Test dataset prepared with {len(self.dataset_test)} samples")

    def _loader(self, subset, shuffle):
        idx = subset.indices if hasattr(subset, "indices") else np.arange(len(subset))
        # val/test: persistent_workers=n_cpu > 0 (data_module.py:245,260)
        return DeviceBatchLoader(self.dataset_full, idx, self.batch_size, shuffle=shuffle,
                                 persistent=not shuffle and self.n_cpu > 0)

    def train_dataloader(self) -> DeviceBatchLoader:
        """data_module.py:215-233 (with no validation split, the whole set)."""
        if self.val_data_ratio > 0.0:
            return self._loader(self.dataset_train, shuffle=True)
        idx = np.concatenate([np.asarray(self.dataset_train.indices), np.asarray(self.dataset_val.indices)])
        return DeviceBatchLoader(self.dataset_full, idx, self.batch_size, shuffle=True)

    def val_dataloader(self) -> DeviceBatchLoader:
        return self._loader(self.dataset_val, shuffle=False)

    def test_dataloader(self) -> DeviceBatchLoader:
        return self._loader(self.dataset_test, shuffle=False)
