"""Dictionary simulation on the MI355X: dictionary patterns projected from a master pattern, one
launch per batch in front of the encoder (`ebsdvae_simulate_patterns`, csrc/simulate.hip;
DESIGN.md section 14, "Dictionary simulation").  The reference has no such step: its dictionary
patterns are simulated elsewhere and read from a .npy file.

    MasterPattern(upper, lower=None)        the two square-Lambert hemispheres, arrays in
    DetectorGeometry(shape, pc, ...)        the detector pixels' directions in the sample frame
    simulate_patterns(master, orientations, detector)   -> (B, 1, h, w) float32 on the device

Conventions (include/ebsdvae.h states the arithmetic): `orientations` are Bunge angles phi1, Phi,
phi2 in degrees, read as the passive rotation sample -> crystal,
`scipy Rotation.from_euler("ZXZ", e, degrees=True).inv()`.  The orientation consensus of the
database reads the same stored triples as the reference does, extrinsic "zxz"; the database keeps
storing them untouched.  Master rows follow the Lambert Y, columns the Lambert X.  There is no
CPU fallback.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native as N

MIN_MASTER_SIDE = 3       # ebsdvae_simulate_patterns' limits on M
MAX_MASTER_SIDE = 4097
MAX_SIMULATED_SIDE = 256  # ... and on h, w

__all__ = ["MasterPattern", "DetectorGeometry", "simulate_patterns", "orientation_matrix",
           "check_orientations", "check_dictionary_request", "MIN_MASTER_SIDE",
           "MAX_MASTER_SIDE", "MAX_SIMULATED_SIDE"]


def orientation_matrix(euler) -> np.ndarray:
    """The Bunge passive matrix g (sample -> crystal) of (..., 3) angles phi1, Phi, phi2 in
    degrees, float64 (..., 3, 3): step (a) of the kernel before its rounding to float32."""
    e = np.asarray(euler, dtype=np.float64) * (math.pi / 180.0)
    c1, s1 = np.cos(e[..., 0]), np.sin(e[..., 0])
    c, s = np.cos(e[..., 1]), np.sin(e[..., 1])
    c2, s2 = np.cos(e[..., 2]), np.sin(e[..., 2])
    g = np.empty(e.shape[:-1] + (3, 3), dtype=np.float64)
    g[..., 0, 0] = c1 * c2 - s1 * s2 * c
    g[..., 0, 1] = s1 * c2 + c1 * s2 * c
    g[..., 0, 2] = s2 * s
    g[..., 1, 0] = -c1 * s2 - s1 * c2 * c
    g[..., 1, 1] = -s1 * s2 + c1 * c2 * c
    g[..., 1, 2] = c2 * s
    g[..., 2, 0] = s1 * s
    g[..., 2, 1] = -c1 * s
    g[..., 2, 2] = c
    return g


class MasterPattern:
    """A master pattern: the square-Lambert projections of the upper (z >= 0) and the lower
    hemisphere, numpy (M, M) arrays or one (2, M, M) array, M = 2n + 1 odd.  `lower=None`
    reuses `upper` (a centrosymmetric master).  Row r, column c of a hemisphere sits at the
    Lambert coordinates (X, Y) = ((c - n) / n, (r - n) / n).  Raises ValueError for arrays that
    are not square, of an even or unsupported side, of different sizes or not finite.  One
    float32 copy per device is made on first use."""

    def __init__(self, upper, lower=None):
        up = np.asarray(upper)
        if lower is None and up.ndim == 3:
            if up.shape[0] != 2:
                raise ValueError(f"a stacked master must be (2, M, M), got {up.shape}")
            up, lower = up[0], up[1]
        self.upper = self._check(up, "upper")
        self.lower = self.upper if lower is None else self._check(np.asarray(lower), "lower")
        if self.lower.shape != self.upper.shape:
            raise ValueError(f"the hemispheres differ in size: {self.upper.shape} and "
                             f"{self.lower.shape}")
        self._device_state: dict = {}

    @staticmethod
    def _check(a: np.ndarray, name: str) -> np.ndarray:
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError(f"{name} must be a square (M, M) array, got shape {a.shape}")
        M = a.shape[0]
        if M % 2 == 0 or not MIN_MASTER_SIDE <= M <= MAX_MASTER_SIDE:
            raise ValueError(f"{name}: the side M = {M} must be odd and within "
                             f"{MIN_MASTER_SIDE}..{MAX_MASTER_SIDE}")
        if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"{name} must be a real array, got {a.dtype}")
        a = np.array(a, dtype=np.float32, order="C")   # a private copy
        if not np.isfinite(a).all():
            raise ValueError(f"{name} holds non-finite values")
        a.setflags(write=False)
        return a

    @property
    def side(self) -> int:
        return self.upper.shape[0]

    @property
    def centrosymmetric(self) -> bool:
        return self.lower is self.upper

    def _on(self, device: torch.device):
        """(upper, lower) on `device`, uploaded on first use; one tensor twice when
        centrosymmetric."""
        st = self._device_state.get(device)
        if st is None:
            up = torch.from_numpy(self.upper.copy()).to(device)   # ours is read-only
            lo = up if self.centrosymmetric else torch.from_numpy(self.lower.copy()).to(device)
            st = self._device_state[device] = (up, lo)
        return st


class DetectorGeometry:
    """The directions of the detector pixels in the sample frame.  `shape` = (h, w) pixels (or
    one int), `pc` = (pcx, pcy, pcz) in the Bruker convention: pcx the fraction of the width from
    the left, pcy the fraction of the height from the top, pcz the detector distance divided by
    the height.  Angles in degrees.  For the centre of pixel (i, j):

        dx = ((j + 1/2) / w - pcx) (w / h)          dy = pcy - (i + 1/2) / h
        alpha = 90 - sample_tilt + tilt             omega = azimuthal
        Ls = -sin(omega) dx + pcz cos(omega)        Lc = cos(omega) dx + pcz sin(omega)
        v ~ (dy cos(alpha) + sin(alpha) Ls,  Lc,  -sin(alpha) dy + cos(alpha) Ls),  normalised

    This formula is the contract.  `directions` (an (h w, 3) or (h, w, 3) array, normalised on
    entry) replaces it for any other convention; pc and the angles are then not used."""

    def __init__(self, shape, pc=(0.5, 0.5, 0.5), sample_tilt: float = 70.0, tilt: float = 0.0,
                 azimuthal: float = 0.0, directions=None):
        try:
            shape = (int(shape),) * 2 if np.isscalar(shape) else tuple(int(v) for v in shape)
        except (TypeError, ValueError):
            raise ValueError(f"shape must be (h, w), got {shape!r}") from None
        if len(shape) != 2 or not all(1 <= v <= MAX_SIMULATED_SIDE for v in shape):
            raise ValueError(f"shape must be (h, w) within 1..{MAX_SIMULATED_SIDE}, got {shape}")
        self.shape = shape
        try:
            pc = tuple(float(v) for v in pc)
        except (TypeError, ValueError):
            raise ValueError(f"pc must be (pcx, pcy, pcz), got {pc!r}") from None
        if len(pc) != 3 or not all(math.isfinite(v) for v in pc) or not pc[2] > 0.0:
            raise ValueError(f"pc must be three finite numbers with pcz > 0, got {pc}")
        self.pc = pc
        self.sample_tilt, self.tilt, self.azimuthal = float(sample_tilt), float(tilt), float(azimuthal)
        if not all(math.isfinite(v) for v in (self.sample_tilt, self.tilt, self.azimuthal)):
            raise ValueError("sample_tilt, tilt and azimuthal must be finite")
        self._directions = None
        if directions is not None:
            d = np.array(directions, dtype=np.float64)
            h, w = shape
            if d.shape not in ((h * w, 3), (h, w, 3)):
                raise ValueError(f"directions must be ({h * w}, 3) or ({h}, {w}, 3), got {d.shape}")
            d = d.reshape(h * w, 3)
            norm = np.linalg.norm(d, axis=1, keepdims=True)
            if not (np.isfinite(d).all() and (norm > 0).all()):
                raise ValueError("directions must be finite and non-zero")
            self._directions = d / norm
        self._device_state: dict = {}

    def direction_cosines(self) -> np.ndarray:
        """(h w, 3) float64 unit vectors, row-major pixel order."""
        if self._directions is not None:
            return self._directions.copy()
        h, w = self.shape
        pcx, pcy, pcz = self.pc
        i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64),
                           indexing="ij")
        dx = ((j + 0.5) / w - pcx) * (w / h)
        dy = pcy - (i + 0.5) / h
        alpha = math.radians(90.0 - self.sample_tilt + self.tilt)
        omega = math.radians(self.azimuthal)
        ca, sa, cw, sw = math.cos(alpha), math.sin(alpha), math.cos(omega), math.sin(omega)
        Ls = -sw * dx + pcz * cw
        Lc = cw * dx + pcz * sw
        v = np.stack([dy * ca + sa * Ls, Lc, -sa * dy + ca * Ls], axis=-1).reshape(h * w, 3)
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def planar_directions(self) -> np.ndarray:
        """What the kernel reads: (3, h w) float32, the rounded direction cosines."""
        return np.ascontiguousarray(self.direction_cosines().T.astype(np.float32))

    def _on(self, device: torch.device) -> torch.Tensor:
        d = self._device_state.get(device)
        if d is None:
            d = self._device_state[device] = torch.from_numpy(self.planar_directions()).to(device)
        return d


def check_orientations(orientations, who: str = "simulate_patterns"):
    """`orientations` as a (B, 3) float64 array where it lies: a numpy array for host data, the
    tensor itself for a device tensor.  One (3,) triple is a batch of one.  ValueError for any
    other shape or dtype, and for host values that are not finite."""
    if torch.is_tensor(orientations):
        t = orientations
        if t.dtype != torch.float64:
            raise ValueError(f"{who}: orientations must be float64, got {t.dtype}")
        if t.ndim == 1:
            t = t.unsqueeze(0)
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError(f"{who}: orientations must be (B, 3), got {tuple(orientations.shape)}")
        if t.is_cuda:
            return t
        t = t.numpy()
    elif isinstance(orientations, np.ndarray):
        t = orientations
        if t.dtype != np.float64:
            raise ValueError(f"{who}: orientations must be float64, got {t.dtype}")
    else:
        try:
            t = np.asarray(orientations, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: orientations must be a (B, 3) float64 array") from None
    if t.ndim == 1:
        t = t[None]
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"{who}: orientations must be (B, 3), got {t.shape}")
    if not np.isfinite(t).all():
        raise ValueError(f"{who}: orientations hold non-finite angles")
    return np.ascontiguousarray(t)


def simulate_patterns(master: MasterPattern, orientations, detector: DetectorGeometry,
                      rescale: bool = True, device="cuda", out: torch.Tensor | None = None):
    """Dictionary patterns of `orientations` ((B, 3) float64 Bunge angles in degrees, host or
    device, or one (3,) triple) on `detector`, projected from `master`: (B, 1, h, w) float32 on
    the device, one launch.  `rescale` maps every pattern to [0, 1] (0 everywhere for a constant
    one); without it the interpolated master intensity is returned.  Shapes and dtypes are
    checked (ValueError) before anything touches the device; the master and the directions are
    uploaded once per device.  No CPU fallback."""
    if not isinstance(master, MasterPattern):
        raise ValueError(f"master must be a MasterPattern, got {type(master).__name__}")
    if not isinstance(detector, DetectorGeometry):
        raise ValueError(f"detector must be a DetectorGeometry, got {type(detector).__name__}")
    ori = check_orientations(orientations)
    B = ori.shape[0]
    h, w = detector.shape
    if out is not None and not (torch.is_tensor(out) and out.dtype == torch.float32
                                and out.numel() == B * h * w and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 ({B}, 1, {h}, {w}) tensor")
    if out is not None and not out.is_cuda:
        raise RuntimeError("simulate_patterns needs a ROCm device (no CPU fallback)")
    if torch.is_tensor(ori):
        dev = ori.device
        ori = ori.contiguous()
    else:
        dev = out.device if out is not None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("simulate_patterns needs a ROCm device (no CPU fallback)")
        ori = torch.from_numpy(ori).to(dev)
    if out is None:
        out = torch.empty(B, 1, h, w, dtype=torch.float32, device=dev)
    elif out.device != dev:
        raise ValueError(f"out is on {out.device}, the orientations on {dev}")
    up, lo = master._on(dev)
    dirs = detector._on(dev)
    N.call("ebsdvae_simulate_patterns", N.ptr(up), N.ptr(lo), master.side, N.ptr(dirs),
           ori.data_ptr(), B, h, w, int(bool(rescale)), N.ptr(out), N.stream(dev))
    return out


def check_dictionary_request(image_size, master, orientations, detector, batch_size, correction):
    """The checks of `DiffractionPatternIndexer.build_dictionary_from_master`, before anything
    touches a device; raises ValueError.  Returns (orientations (N, 3) float64 host array,
    detector, batch size)."""
    from .patterns import PatternCorrection
    if not isinstance(master, MasterPattern):
        raise ValueError(f"master must be a MasterPattern, got {type(master).__name__}")
    image_size = tuple(int(v) for v in image_size)
    if detector is None:
        detector = DetectorGeometry(image_size)
    if not isinstance(detector, DetectorGeometry):
        raise ValueError(f"detector must be a DetectorGeometry, got {type(detector).__name__}")
    if detector.shape != image_size:
        raise ValueError(f"the detector is {detector.shape}, the model reads {image_size} patterns")
    if torch.is_tensor(orientations) and orientations.is_cuda:
        raise ValueError("build_dictionary_from_master takes the orientation list as a host array "
                         "(the database keeps a host copy)")
    ori = check_orientations(orientations, "build_dictionary_from_master")
    if ori.shape[0] == 0:
        raise ValueError("build_dictionary_from_master needs at least one orientation")
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size={batch_size} must be at least 1")
    if correction is not None:
        if not isinstance(correction, PatternCorrection):
            raise ValueError("correction must be a PatternCorrection, got "
                             f"{type(correction).__name__}")
        if correction.static_background is not None:
            raise ValueError("a static_background belongs to a detector, not to simulated patterns: "
                             "build_dictionary_from_master takes the dynamic step and the rescale only")
        correction.check(image_size[0], image_size[1], image_size[0], image_size[1])
    return ori, detector, batch_size
