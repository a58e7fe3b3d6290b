"""Grains of an indexed scan, built on the device (csrc/grains.hip; the definitions are in
include/ebsdvae.h and DESIGN.md section 14, "Grains").

    segment_grains    connected components of the scan grid under the cubic disorientation, and per
                      point its grain's id, mean orientation and orientation spread (GOS), its own
                      deviation from that mean (GROD) and whether it lies on a grain boundary
    GrainMap          those per-point arrays; `table()` derives the per-grain table on the host

`index_scan(maps=ScanMaps(..., grains=True))` appends the same to its result.  As the scan maps:
a numpy array is uploaded and numpy comes back, a device tensor stays on the device; shapes,
dtypes and values are checked before anything touches the device, and there is no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from latice import _native as N
from latice.index.maps import (_connectivity, _device_input, _euler_rows, _give_back,
                               _grain_threshold, _scan_shape, _upload)

__all__ = ["GrainMap", "segment_grains", "grain_rows"]


@dataclass
class GrainTable:
    """One row per grain, in grain id order."""
    sizes: np.ndarray                       # (G,) int64: points in the grain
    first_point: np.ndarray                 # (G,) int64: flat index of the grain's root
    mean_orientation: np.ndarray | None     # (G, 3) float64, ZXZ Euler degrees
    gos: np.ndarray | None                  # (G,) float32, degrees

    def __len__(self) -> int:
        return int(self.sizes.shape[0])


@dataclass
class GrainMap:
    """Per-point arrays on the (rows, cols) grid: numpy arrays, or device tensors where
    `segment_grains` was given one."""
    grain_id: object                        # (rows, cols) int32, -1 at unusable points
    grain_orientation: object = None        # (rows, cols, 3) float64: the grain's mean, ZXZ degrees
    gos: object = None                      # (rows, cols) float32: the grain's mean GROD
    grod: object = None                     # (rows, cols) float32: degrees from the grain's mean
    boundary: object = None                 # (rows, cols) uint8

    @property
    def n_grains(self) -> int:
        return int(self.grain_id.max()) + 1

    def table(self) -> GrainTable:
        """The per-grain table, derived on the host (a tensor's values are copied there)."""
        def host(a):
            if a is None:
                return None
            return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        ids = host(self.grain_id).reshape(-1)
        found, first = np.unique(ids, return_index=True)
        first = first[found >= 0].astype(np.int64)      # ids rank the grains by their first point
        sizes = np.bincount(ids[ids >= 0], minlength=len(first)).astype(np.int64)
        mean, gos = host(self.grain_orientation), host(self.gos)
        return GrainTable(sizes=sizes, first_point=first,
                          mean_orientation=None if mean is None else mean.reshape(-1, 3)[first],
                          gos=None if gos is None else gos.reshape(-1)[first])


def grain_rows(euler: torch.Tensor, valid: torch.Tensor | None, scan_shape, connectivity: int,
               threshold: float, grain_id: torch.Tensor, grain_euler: torch.Tensor | None = None,
               gos: torch.Tensor | None = None, grod: torch.Tensor | None = None,
               boundary: torch.Tensor | None = None, work: torch.Tensor | None = None) -> torch.Tensor:
    """`ebsdvae_segment_grains` of the contiguous device rows euler (rows * cols, 3) float64 (and
    valid (rows * cols,) int32) into the given outputs, on the current stream.  Returns the scratch
    (`work`, or a new tensor of `ebsdvae_grain_work` bytes): keep it until the stream is past."""
    rows, cols = scan_shape
    need = N.call("ebsdvae_grain_work", rows, cols)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=euler.device)
    elif work.numel() * work.element_size() < need:
        raise ValueError(f"grain_rows: work holds {work.numel() * work.element_size()} bytes, "
                         f"{need} are needed")

    def p(t):
        return None if t is None else t.data_ptr()
    N.call("ebsdvae_segment_grains", euler.data_ptr(), p(valid), rows, cols, connectivity,
           float(threshold), grain_id.data_ptr(), p(grain_euler), p(gos), p(grod), p(boundary),
           work.data_ptr(), N.stream(euler.device))
    return work


def segment_grains(orientations, scan_shape, threshold: float = 5.0, connectivity: int = 4,
                   valid=None, mean: bool = True, grod: bool = True,
                   boundary: bool = True) -> GrainMap:
    """The grains of a scan on the grid `scan_shape` = (rows, cols), row-major: `orientations`
    (rows * cols, 3) or (rows, cols, 3), ZXZ Euler degrees (float64 for a tensor).  A point is
    usable if its angles are finite and `valid` ((rows * cols,) or (rows, cols); int32 for a
    tensor; None: all) is non-zero there.  Usable neighbours of the cross (`connectivity` 4) or
    the square (8) whose cubic disorientation is at most `threshold` degrees are joined; grains
    are the connected components, numbered by their first point in row-major order, -1 at
    unusable points.  With `mean`, `grain_orientation` and `gos` are returned, with `grod` the
    per-point deviation, with `boundary` the boundary map; the ids are the same bits whichever
    are asked for.  Unusable points hold NaN (boundary: 0)."""
    rows, cols = _scan_shape(scan_shape)
    connectivity = _connectivity(connectivity)
    threshold = _grain_threshold(threshold)
    n = rows * cols
    is_tensor, t = _euler_rows(orientations, "segment_grains")
    if tuple(t.shape) not in ((n, 3), (rows, cols, 3)):
        raise ValueError(f"segment_grains: orientations must be ({n}, 3) or ({rows}, {cols}, 3) "
                         f"for scan_shape {(rows, cols)}, got shape {tuple(t.shape)}")
    v = None
    if valid is not None:
        v_tensor, v = _device_input(valid, "segment_grains", "valid", torch.int32, "biu")
        if v_tensor != is_tensor:
            raise ValueError("segment_grains: orientations and valid must both be numpy arrays or "
                             "both be device tensors")
        if tuple(v.shape) not in ((n,), (rows, cols)):
            raise ValueError(f"segment_grains: valid must be ({n},) or ({rows}, {cols}) for "
                             f"scan_shape {(rows, cols)}, got shape {tuple(v.shape)}")
    e = _upload(t, "segment_grains").reshape(-1, 3)
    with torch.cuda.device(e.device):
        if v is not None:
            v = _upload(v, "segment_grains").to(e.device).reshape(-1)
        dev = e.device
        ids = torch.empty(n, dtype=torch.int32, device=dev)
        g_euler = torch.empty(n, 3, dtype=torch.float64, device=dev) if mean else None
        g_gos = torch.empty(n, dtype=torch.float32, device=dev) if mean else None
        g_grod = torch.empty(n, dtype=torch.float32, device=dev) if grod else None
        g_edge = torch.empty(n, dtype=torch.uint8, device=dev) if boundary else None
        grain_rows(e, v, (rows, cols), connectivity, threshold, ids, g_euler, g_gos, g_grod, g_edge)

    def back(out, *tail):
        return None if out is None else _give_back(is_tensor, out.view(rows, cols, *tail))
    return GrainMap(grain_id=back(ids), grain_orientation=back(g_euler, 3), gos=back(g_gos),
                    grod=back(g_grod), boundary=back(g_edge))
