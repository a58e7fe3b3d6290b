"""Float64 oracle of the neighbour pattern averaging ("Neighbour pattern
averaging") and the host simulation of its streaming schedule.  Plain numpy: a restatement of
the definition, not of the kernel."""
import functools

import numpy as np


def average(T, scan_shape, weights):
    """The definition on T (N, ...) with N = rows * cols patterns in row-major grid order and the
    (2 hr + 1, 2 hc + 1) window `weights` (the float32 values the device receives): every
    pattern becomes the weighted mean of its on-grid neighbours with a nonzero weight.  Whole
    shifted slabs of the grid are accumulated, in float64."""
    rows, cols = scan_shape
    T = np.asarray(T, dtype=np.float64)
    assert T.shape[0] == rows * cols
    W = np.asarray(weights, dtype=np.float32).astype(np.float64)
    hr, hc = W.shape[0] // 2, W.shape[1] // 2
    grid = T.reshape((rows, cols) + T.shape[1:])
    num = np.zeros_like(grid)
    den = np.zeros((rows, cols) + (1,) * (T.ndim - 1))
    for a in range(-hr, hr + 1):
        for b in range(-hc, hc + 1):
            wt = W[a + hr, b + hc]
            if wt == 0:
                continue
            # outputs (i, j) whose neighbour (i + a, j + b) is on the grid
            i0, i1 = max(0, -a), min(rows, rows - a)
            j0, j1 = max(0, -b), min(cols, cols - b)
            if i0 >= i1 or j0 >= j1:
                continue
            num[i0:i1, j0:j1] += wt * grid[i0 + a:i1 + a, j0 + b:j1 + b]
            den[i0:i1, j0:j1] += wt
    return (num / den).reshape(T.shape)


def brute_force(T, scan_shape, weights):
    """The same by a quadruple loop over (i, j, a, b), one pattern and one tap at a time."""
    rows, cols = scan_shape
    T = np.asarray(T, dtype=np.float64)
    W = np.asarray(weights, dtype=np.float32).astype(np.float64)
    hr, hc = W.shape[0] // 2, W.shape[1] // 2
    out = np.empty_like(T)
    for i in range(rows):
        for j in range(cols):
            num, den = np.zeros(T.shape[1:]), 0.0
            for a in range(-hr, hr + 1):
                for b in range(-hc, hc + 1):
                    wt = W[a + hr, b + hc]
                    if wt != 0 and 0 <= i + a < rows and 0 <= j + b < cols:
                        num = num + wt * T[(i + a) * cols + (j + b)]
                        den += wt
            out[i * cols + j] = num / den
    return out


def taps(weights):
    """Number of nonzero weights: what the parity gate 2 (taps + 1) 2^-24 counts."""
    return int(np.count_nonzero(np.asarray(weights)))


@functools.lru_cache(maxsize=None)
def patterns(n, h, w, seed=0):
    """(n, 1, h, w) uniform random float32 in [0, 1).  Read-only: shared between tests."""
    x = np.random.default_rng(seed).random((n, 1, h, w), dtype=np.float32)
    x.setflags(write=False)
    return x


def simulate(schedule, n, cols, hr, hc, batch):
    """Walk a `neighbour_schedule` as index_scan does, with the ring as an array of the flat
    index each slot holds, and assert what the streaming relies on: the batches cover the scan
    in order, every pattern is ingested once and averaged once, in order, every on-grid
    neighbour is in its slot (not yet overwritten) when an output reads it, no chunk exceeds the
    batch size and the ring stays within batch + 2 (hr cols + hc) patterns.  Returns the number
    of averaging chunks."""
    rows = -(-n // cols)
    cap = schedule.ring_cap
    assert 1 <= cap <= max(1, min(n, batch + 2 * (hr * cols + hc)))
    ring = np.full(cap, -1, dtype=np.int64)
    ingested = np.zeros(n, dtype=np.int64)
    averaged = np.zeros(n, dtype=np.int64)
    at, done, chunks = 0, 0, 0
    for step in schedule.steps:
        assert step.start == at and step.start < step.stop <= min(n, at + batch)
        at = step.stop
        cursor = step.start
        for a, b, slot in step.ingest:
            assert a == cursor and a < b and slot == a % cap and slot + (b - a) <= cap
            ring[slot:slot + b - a] = np.arange(a, b)
            ingested[a:b] += 1
            cursor = b
        assert cursor == step.stop
        for a, b in step.ready:
            assert a == done and a < b <= n and b - a <= batch
            chunks += 1
            for p in range(a, b):
                i, j = divmod(p, cols)
                for da in range(-hr, hr + 1):
                    for db in range(-hc, hc + 1):
                        if 0 <= i + da < rows and 0 <= j + db < cols:
                            q = (i + da) * cols + (j + db)
                            assert q < n and ring[q % cap] == q, (p, q, int(ring[q % cap]))
            averaged[a:b] += 1
            done = b
    assert at == n and done == n
    assert (ingested == 1).all() and (averaged == 1).all()
    return chunks
