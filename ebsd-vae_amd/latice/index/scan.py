"""Host side of `DiffractionPatternIndexer.index_scan`: the result record and the batching of
a scan into work items.  numpy only: nothing here touches the device or the HIP library.
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
