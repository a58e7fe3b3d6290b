"""Scan maps: what an indexed scan is looked at with, built on the device from the result rows
of `index_scan` (csrc/scan_maps.hip; the definitions are in include/ebsdvae.h and DESIGN.md
section 14, "Scan maps").

    ipf_colors                       inverse-pole-figure colours, the reference's `get_color_key`
                                     (latice/utils/utils.py:206-240) for a whole scan in one launch
    orientation_similarity_map       how many of a point's top-k dictionary rows its scan
                                     neighbours share (Marquardt et al. 2017)
    kernel_average_misorientation    the mean cubic disorientation to the scan neighbours
    ScanMaps                         which of them `index_scan(maps=...)` appends to its result

Only `ipf_colors` has a counterpart in the reference.  Every function takes a numpy array, which
is uploaded and whose map comes back as numpy, or a device tensor, whose map stays a device
tensor; shapes and dtypes are checked before anything touches the device, and there is no CPU
fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from latice import _native as N

__all__ = ["IPF_DIRECTIONS", "MAX_SIMILARITY_K", "ScanMaps", "ipf_colors",
           "orientation_similarity_map", "kernel_average_misorientation"]

IPF_DIRECTIONS = {"x": 0, "y": 1, "z": 2}     # the row of the rotation matrix: ipf_x / _y / _z
MAX_SIMILARITY_K = 64                         # candidates per point: one wave lane each
CONNECTIVITIES = (4, 8)
N_NUMPY = {torch.float64: np.float64, torch.int64: np.int64, torch.int32: np.int32}


def _scan_shape(scan_shape) -> tuple[int, int]:
    try:
        rows, cols = (int(v) for v in scan_shape)
    except (TypeError, ValueError):
        raise ValueError(f"scan_shape must be (rows, cols), got {scan_shape!r}") from None
    if rows < 1 or cols < 1 or rows * cols >= 1 << 31:
        raise ValueError(f"scan_shape {scan_shape!r}: rows and cols must be positive "
                         "(and rows * cols below 2^31)")
    return rows, cols


def _connectivity(connectivity) -> int:
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"connectivity must be 4 (cross) or 8 (square), got {connectivity!r}")
    return int(connectivity)


def _direction(direction) -> int:
    if direction not in IPF_DIRECTIONS:
        raise ValueError(f"direction must be one of 'x', 'y', 'z', got {direction!r}")
    return IPF_DIRECTIONS[direction]


def _max_angle(max_angle) -> float:
    v = math.inf if max_angle is None else float(max_angle)
    if math.isnan(v) or v < 0.0:
        raise ValueError(f"max_angle must be a non-negative number of degrees (inf or None keeps "
                         f"every neighbour), got {max_angle!r}")
    return v


def _grain_threshold(threshold) -> float:
    try:
        v = float(threshold)
    except (TypeError, ValueError):
        v = math.nan
    if not math.isfinite(v) or v < 0.0:
        raise ValueError(f"the grain threshold must be a finite, non-negative number of degrees, "
                         f"got {threshold!r}")
    return v


def _device_input(x, who: str, what: str, dtype: torch.dtype, kinds: str):
    """`x` as (is it a tensor, a tensor of `dtype`) after the dtype check; a numpy array stays on
    the host until every other check has passed.  A tensor must already be on the device."""
    if torch.is_tensor(x):
        if x.dtype != dtype:
            raise ValueError(f"{who}: {what} must be {dtype}, got {x.dtype}")
        if not x.is_cuda:
            raise ValueError(f"{who}: a tensor must be on a ROCm device (pass a numpy array to "
                             f"have it uploaded), got {x.device}")
        return True, x
    a = np.asarray(x)
    if a.dtype.kind not in kinds:
        raise ValueError(f"{who}: {what} must be a numeric array, got dtype {a.dtype}")
    return False, torch.from_numpy(np.ascontiguousarray(a, dtype=N_NUMPY[dtype]))


def _upload(t: torch.Tensor, who: str) -> torch.Tensor:
    if t.is_cuda:
        return t.contiguous()
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who} needs a ROCm device (no CPU fallback)")
    return t.to("cuda")


def _give_back(is_tensor: bool, out: torch.Tensor):
    return out if is_tensor else out.cpu().numpy()


def _euler_rows(orientations, who: str):
    is_tensor, t = _device_input(orientations, who, "orientations", torch.float64, "fiu")
    if t.dim() < 1 or t.shape[-1] != 3:
        raise ValueError(f"{who}: orientations must be (..., 3) ZXZ Euler degrees, got shape "
                         f"{tuple(t.shape)}")
    return is_tensor, t


def ipf_rows(euler: torch.Tensor, axis: int, out: torch.Tensor) -> torch.Tensor:
    """out (n, 3) uint8 = the IPF colours of the contiguous device rows euler (n, 3) float64
    (`ebsdvae_ipf_colors`) on the current stream."""
    if euler.shape[0] == 0:      # an empty tensor has no pointer to hand over
        return out
    N.call("ebsdvae_ipf_colors", euler.data_ptr(), euler.shape[0], axis, out.data_ptr(),
           N.stream(euler.device))
    return out


def similarity_rows(cand_idx: torch.Tensor, scan_shape, connectivity: int, normalize: bool,
                    out: torch.Tensor) -> torch.Tensor:
    """out (rows * cols,) float32 = the orientation similarity of the contiguous device rows
    cand_idx (rows * cols, k) int64 (`ebsdvae_orientation_similarity`) on the current stream."""
    N.call("ebsdvae_orientation_similarity", cand_idx.data_ptr(), cand_idx.shape[1],
           scan_shape[0], scan_shape[1], connectivity, int(bool(normalize)), out.data_ptr(),
           N.stream(cand_idx.device))
    return out


def misorientation_rows(euler: torch.Tensor, scan_shape, connectivity: int, max_angle: float,
                        out: torch.Tensor) -> torch.Tensor:
    """out (rows * cols,) float32 = the kernel average misorientation of the contiguous device
    rows euler (rows * cols, 3) float64 (`ebsdvae_kernel_misorientation`) on the current stream."""
    N.call("ebsdvae_kernel_misorientation", euler.data_ptr(), scan_shape[0], scan_shape[1],
           connectivity, float(max_angle), out.data_ptr(), N.stream(euler.device))
    return out


def ipf_colors(orientations, direction: str = "z"):
    """Inverse-pole-figure colours of `orientations` (..., 3), ZXZ Euler degrees (float64 for a
    tensor): (..., 3) uint8, equal to the reference's `get_color_key(orientations, "ipf_" +
    direction)` (the sample direction x, y or z in crystal coordinates, folded by the cubic group
    into the reference's colour sector).  A non-finite row gives (0, 0, 0)."""
    axis = _direction(direction)
    is_tensor, t = _euler_rows(orientations, "ipf_colors")
    e = _upload(t, "ipf_colors").reshape(-1, 3)
    with torch.cuda.device(e.device):
        out = torch.empty(e.shape[0], 3, dtype=torch.uint8, device=e.device)
        ipf_rows(e, axis, out)
    return _give_back(is_tensor, out.view(tuple(t.shape)))


def orientation_similarity_map(candidate_indices, scan_shape, connectivity: int = 4,
                               normalize: bool = False):
    """The orientation similarity map of a scan on the grid `scan_shape` = (rows, cols), row-major:
    `candidate_indices` (rows * cols, k) int64 are the top-k dictionary rows per point
    (`ScanIndexResult.candidate_indices`; entries < 0 count as none).  Per point, the number of
    its candidates that a neighbour's list holds too, averaged over the on-grid neighbours of
    the cross (`connectivity` 4) or the square (8), divided by k with `normalize`; 0 where there
    is no neighbour.  Returns (rows, cols) float32."""
    rows, cols = _scan_shape(scan_shape)
    connectivity = _connectivity(connectivity)
    is_tensor, t = _device_input(candidate_indices, "orientation_similarity_map",
                                 "candidate_indices", torch.int64, "iu")
    if t.dim() != 2 or t.shape[0] != rows * cols or not 1 <= t.shape[1] <= MAX_SIMILARITY_K:
        raise ValueError(f"orientation_similarity_map: candidate_indices must be ({rows * cols}, k) "
                         f"with 1 <= k <= {MAX_SIMILARITY_K} for scan_shape {(rows, cols)}, got "
                         f"shape {tuple(t.shape)}")
    c = _upload(t, "orientation_similarity_map")
    with torch.cuda.device(c.device):
        out = torch.empty(rows * cols, dtype=torch.float32, device=c.device)
        similarity_rows(c, (rows, cols), connectivity, normalize, out)
    return _give_back(is_tensor, out.view(rows, cols))


def kernel_average_misorientation(orientations, scan_shape, connectivity: int = 4,
                                  max_angle: float | None = 5.0):
    """The kernel average misorientation of a scan on the grid `scan_shape` = (rows, cols):
    `orientations` (rows * cols, 3) or (rows, cols, 3), ZXZ Euler degrees (float64 for a tensor).
    Per point, the mean cubic disorientation in degrees to the on-grid neighbours of the cross
    (`connectivity` 4) or the square (8) that lie within `max_angle` degrees of it (None or inf:
    all of them); 0 where none does, NaN where the point's own orientation is not finite, and a
    non-finite neighbour is skipped.  Returns (rows, cols) float32."""
    rows, cols = _scan_shape(scan_shape)
    connectivity = _connectivity(connectivity)
    max_angle = _max_angle(max_angle)
    is_tensor, t = _euler_rows(orientations, "kernel_average_misorientation")
    if tuple(t.shape) not in ((rows * cols, 3), (rows, cols, 3)):
        raise ValueError(f"kernel_average_misorientation: orientations must be ({rows * cols}, 3) "
                         f"or ({rows}, {cols}, 3) for scan_shape {(rows, cols)}, got shape "
                         f"{tuple(t.shape)}")
    e = _upload(t, "kernel_average_misorientation").reshape(-1, 3)
    with torch.cuda.device(e.device):
        out = torch.empty(rows * cols, dtype=torch.float32, device=e.device)
        misorientation_rows(e, (rows, cols), connectivity, max_angle, out)
    return _give_back(is_tensor, out.view(rows, cols))


@dataclass(frozen=True)
class ScanMaps:
    """The maps `index_scan(maps=...)` builds on the device once the last batch is queued, from
    the result rows of the whole scan, and returns as further fields of its `ScanIndexResult`.
    The scan's N = rows * cols patterns lie on the grid `scan_shape` = (rows, cols) in row-major
    order.  `ipf` names the sample directions ('x', 'y', 'z') to colour (`ipf_colors`; none:
    ()); `similarity` asks for `orientation_similarity_map` (divided by k with
    `similarity_normalize`), `kam` for `kernel_average_misorientation` within `kam_max_angle`
    degrees (None or inf: every neighbour); both use `connectivity` 4 or 8.  With `mask_failed`
    the colours of patterns without a consensus (`success` false) are (0, 0, 0).  `grains` asks
    for `segment_grains` (latice/index/grains.py) at `grain_threshold` degrees and the same
    `connectivity`, with every output, as `ScanIndexResult.grains`; with `grain_mask_failed` the
    patterns without a consensus are unusable points (grain id -1)."""

    scan_shape: tuple
    ipf: tuple = ("z",)
    similarity: bool = False
    similarity_normalize: bool = False
    kam: bool = False
    kam_max_angle: float | None = 5.0
    connectivity: int = 4
    mask_failed: bool = False
    grains: bool = False
    grain_threshold: float = 5.0
    grain_mask_failed: bool = False

    def __post_init__(self):
        object.__setattr__(self, "scan_shape", _scan_shape(self.scan_shape))
        try:
            ipf = tuple(self.ipf)      # a string names one direction per letter
        except TypeError:
            raise ValueError(f"ipf must name directions, e.g. ('z',), got {self.ipf!r}") from None
        for d in ipf:
            _direction(d)
        if len(set(ipf)) != len(ipf):
            raise ValueError(f"ipf names a direction twice: {ipf!r}")
        object.__setattr__(self, "ipf", ipf)
        object.__setattr__(self, "connectivity", _connectivity(self.connectivity))
        object.__setattr__(self, "kam_max_angle", _max_angle(self.kam_max_angle))
        object.__setattr__(self, "grain_threshold", _grain_threshold(self.grain_threshold))
        for name in ("similarity", "similarity_normalize", "kam", "mask_failed", "grains",
                     "grain_mask_failed"):
            object.__setattr__(self, name, bool(getattr(self, name)))

    def check(self, n: int) -> None:
        rows, cols = self.scan_shape
        if int(n) != rows * cols:
            raise ValueError(f"the scan has {n} patterns, scan_shape {self.scan_shape} needs "
                             f"{rows * cols}")
