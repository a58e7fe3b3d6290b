"""Host side of `DiffractionPatternIndexer.index_scan`: the result record, the batching of
a scan into work items and the schedule of a neighbour-averaged scan through its device ring.
numpy only: nothing here touches the device or the HIP library.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path

import numpy as np

# staging dtype codes of a host scan: what the pinned buffers hold and which ingest kernel
# reads them (0 / 1 = ebsdvae_ingest_patterns' src_dtype, 2 = ebsdvae_ingest_patterns_u8)
SCAN_F64, SCAN_F32, SCAN_U8 = 0, 1, 2
SCAN_NUMPY_DTYPES = {SCAN_F64: np.float64, SCAN_F32: np.float32, SCAN_U8: np.uint8}


@dataclass
class ScanIndexResult:
    """One row per pattern of a scan, as plain numpy arrays."""
    orientations: np.ndarray            # (N, 3) float64: ZXZ Euler degrees, best per pattern
    success: np.ndarray                 # (N,) bool: a consensus was found
    scores: np.ndarray                  # (N,) float32: top-1 cosine similarity
    top_index: np.ndarray               # (N,) int64: dictionary row of the top match (-1: none)
    n_similar: np.ndarray               # (N,) int32: candidates within the threshold
    candidate_indices: np.ndarray | None = None   # (N, k) int64, best first
    candidate_scores: np.ndarray | None = None    # (N, k) float32
    # the scan maps of `index_scan(maps=ScanMaps(...))` on its (rows, cols) grid (latice/index/maps.py)
    ipf_colors: dict | None = None                # direction -> (rows, cols, 3) uint8
    orientation_similarity: np.ndarray | None = None   # (rows, cols) float32
    kam: np.ndarray | None = None                 # (rows, cols) float32, degrees
    grains: object | None = None                  # GrainMap (latice/index/grains.py) of numpy arrays

    def __len__(self) -> int:
        return int(self.success.shape[0])


def scan_dtype_code(dtype) -> int:
    """Staging code of a host scan's dtype.  float64, float32 and uint8 are staged as they
    are; any other dtype is staged as float64 raw values, as `ingest_patterns` reads it."""
    dt = np.dtype(dtype)
    if dt == np.float32:
        return SCAN_F32
    if dt == np.uint8:
        return SCAN_U8
    return SCAN_F64


def open_scan(patterns):
    """A path to a .npy file -> a read-only memmap; an array is returned as it is."""
    if isinstance(patterns, (str, Path)):
        path = Path(patterns)
        if path.suffix != ".npy":
            raise ValueError(f"Only .npy scan files are supported, got {path}")
        return np.load(path, mmap_mode="r")
    return patterns


def scan_batches(source: np.ndarray, batch_size: int) -> list[tuple[int, int, int]]:
    """Work items (start, stop, dtype code) that cover a host scan (N, H0, W0) in order,
    `batch_size` patterns each and a shorter tail."""
    if not isinstance(source, np.ndarray):
        raise TypeError(f"a host scan must be a numpy array or memmap, got {type(source).__name__}")
    if source.ndim != 3:
        raise ValueError(f"a host scan must be (N, H0, W0), got shape {tuple(source.shape)}")
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size={batch_size} must be at least 1")
    code = scan_dtype_code(source.dtype)
    n = source.shape[0]
    return [(s, min(s + batch_size, n), code) for s in range(0, n, batch_size)]


@dataclass(frozen=True)
class NeighbourStep:
    """One staged batch of a neighbour-averaged scan."""
    start: int                  # the batch: flat scan range [start, stop)
    stop: int
    ingest: tuple               # ((start, stop, slot), ...): sub-ranges and the ring slot each begins at
    ready: tuple                # ((start, stop), ...): output chunks that are complete after it


@dataclass(frozen=True)
class NeighbourSchedule:
    ring_cap: int               # patterns in the ring; scan pattern q lives in slot q % ring_cap
    steps: tuple


def neighbour_schedule(n: int, cols: int, hr: int, hc: int, batch_size: int) -> NeighbourSchedule:
    """How a host scan of n patterns on a grid of `cols` columns streams through a device ring
    of transformed patterns when each is averaged over a (2 hr + 1) x (2 hc + 1) window.

    A pattern's neighbours lie within reach = hr * cols + hc of its flat index.  The batches are
    those of `scan_batches`.  After the batch ending at e has been ingested, the outputs below
    e - reach are complete (all of them at e = n); they become ready in chunks of at most
    `batch_size`.  A ready chunk [a, b) reads the patterns [a - reach, b + reach) of the scan,
    the oldest of which is reach below the first output still to come, itself at most reach
    below the batch's start: a ring of batch_size + 2 reach slots (or n, if that is less) holds
    every pattern until its last reader has run.  A batch that passes the ring's end is
    ingested in two parts; every pattern is ingested once."""
    n, cols, hr, hc, batch_size = int(n), int(cols), int(hr), int(hc), int(batch_size)
    if n < 0 or cols < 1 or hr < 0 or hc < 0 or batch_size < 1:
        raise ValueError(f"neighbour_schedule: n={n} cols={cols} hr={hr} hc={hc} batch_size={batch_size}")
    reach = hr * cols + hc
    cap = max(1, min(n, batch_size + 2 * reach))
    steps, done = [], 0
    for s in range(0, n, batch_size):
        e = min(s + batch_size, n)
        slot = s % cap
        head = min(e - s, cap - slot)
        ingest = [(s, s + head, slot)]
        if s + head < e:
            ingest.append((s + head, e, 0))
        upto = n if e == n else max(done, e - reach)
        ready = [(a, min(a + batch_size, upto)) for a in range(done, upto, batch_size)]
        done = upto
        steps.append(NeighbourStep(s, e, tuple(ingest), tuple(ready)))
    return NeighbourSchedule(cap, tuple(steps))
