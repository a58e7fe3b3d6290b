"""Oracle of the non-local pattern averaging ("Non-local pattern
averaging") and the two-grain scan its tests run on.  Plain numpy, written from the definition:
loops over patterns and window offsets, nothing of the kernels' structure.

`nlpar_ref(..., dtype=np.float64)` is the oracle.  `dtype=np.float32` is the float32 restatement:
the same formulas with every operation rounded to float32 (numpy's pairwise
`sum(dtype=float32)` for the distances), whose deviation from the oracle calibrates the gates of
tests/test_gpu_nlpar.py."""
import functools

import numpy as np


def nlpar_ref(T, rows, cols, hr, hc, lam=0.7, sigma=None, sigma_floor=1e-3, dthresh=None,
              dtype=np.float64):
    """T (N, ...) float32 patterns, N = rows * cols in row-major grid order.  Returns
    (sigma (N,), weights (N, 2 hr + 1, 2 hc + 1) float32, d (N, 2 hr + 1, 2 hc + 1), A):
    sigma and d in `dtype` (d is 0 at the centre and NaN off the grid), the weights rounded to
    float32 as the contract says, A = the weighted mean with those float32 weights, summed in
    `dtype`, a ascending then b ascending."""
    f = np.dtype(dtype).type
    T = np.asarray(T)
    N = rows * cols
    assert T.shape[0] == N and T.dtype == np.float32
    X = T.reshape(N, -1).astype(dtype)
    n = X.shape[1]

    def D(p, q):
        diff = X[p] - X[q]
        return np.sum(diff * diff, dtype=dtype)

    def on_grid(i, j):
        return 0 <= i < rows and 0 <= j < cols

    # noise variance per pattern
    s = np.empty(N, dtype=dtype)
    for p in range(N):
        i, j = divmod(p, cols)
        if sigma is not None:
            s[p] = f(float(sigma) ** 2)
            continue
        ring = [D(p, (i + a) * cols + j + b) for a in (-1, 0, 1) for b in (-1, 0, 1)
                if (a, b) != (0, 0) and on_grid(i + a, j + b)]
        floor2 = f(float(sigma_floor) ** 2)
        s[p] = max(min(ring) / f(2 * n), floor2) if ring else floor2

    NA, NB = 2 * hr + 1, 2 * hc + 1
    W = np.zeros((N, NA, NB), np.float32)
    d = np.full((N, NA, NB), np.nan, dtype=dtype)
    lam2, root = f(float(lam) ** 2), np.sqrt(f(2 * n))
    for p in range(N):
        i, j = divmod(p, cols)
        for a in range(-hr, hr + 1):
            for b in range(-hc, hc + 1):
                if (a, b) == (0, 0):
                    W[p, hr, hc], d[p, hr, hc] = 1.0, 0.0
                    continue
                if not on_grid(i + a, j + b):
                    continue
                q = (i + a) * cols + j + b
                v = s[p] + s[q]
                dd = max((D(p, q) - f(n) * v) / (v * root), f(0))
                wt = np.exp(-dd / lam2)
                if dthresh is not None and dd > f(dthresh):
                    wt = f(0)
                d[p, a + hr, b + hc] = dd
                W[p, a + hr, b + hc] = wt
    return np.sqrt(s), W, d, weighted_mean(T, rows, cols, W, dtype)


def weighted_mean(T, rows, cols, W, dtype=np.float64):
    """A[p] = sum W[p][a][b] T[q] / sum W[p][a][b] over the on-grid window of p, a ascending
    then b ascending, in `dtype`: the chain of the contract run on given float32 weights."""
    T = np.asarray(T)
    X = T.reshape(T.shape[0], -1).astype(dtype)
    W = np.asarray(W, np.float32).astype(dtype)
    hr, hc = W.shape[1] // 2, W.shape[2] // 2
    out = np.empty_like(X)
    for p in range(X.shape[0]):
        i, j = divmod(p, cols)
        num, den = np.zeros(X.shape[1], dtype=dtype), np.dtype(dtype).type(0)
        for a in range(-hr, hr + 1):
            for b in range(-hc, hc + 1):
                if 0 <= i + a < rows and 0 <= j + b < cols:
                    wt = W[p, a + hr, b + hc]
                    num = num + wt * X[(i + a) * cols + j + b]
                    den = den + wt
        out[p] = num / den
    return out.reshape(T.shape)


def _field(rng, h, w):
    """A standard-normal (h, w) field, box-filtered with a 5-tap mean along each axis, divided
    by its standard deviation."""
    x = rng.standard_normal((h, w))
    box = np.full(5, 0.2)
    x = np.apply_along_axis(lambda r: np.convolve(r, box, "same"), 0, x)
    x = np.apply_along_axis(lambda r: np.convolve(r, box, "same"), 1, x)
    return x / x.std()


@functools.lru_cache(maxsize=None)
def nlpar_scan(rows, cols, h, w, noise=0.05, drift=0.004, seed=0):
    """(rows * cols, 1, h, w) float32 in [0, 1]: two grains with a sharp boundary between the
    columns (cols + 1) // 2 - 1 and (cols + 1) // 2, a slow drift inside each and white noise
    of standard deviation `noise`, so that the weights cover every regime.  Read-only: shared
    between tests."""
    rng = np.random.default_rng(seed)
    S0, S1, B = _field(rng, h, w), _field(rng, h, w), _field(rng, h, w)
    grains = (0.5 + 0.15 * S0, 0.5 + 0.15 * S1)
    out = np.empty((rows * cols, 1, h, w), np.float32)
    for p in range(rows * cols):
        i, j = divmod(p, cols)
        g = 0 if j < (cols + 1) // 2 else 1
        out[p, 0] = np.clip(grains[g] + drift * (i + j) * B + noise * rng.standard_normal((h, w)),
                            0.0, 1.0).astype(np.float32)
    out.setflags(write=False)
    return out


# (rows, cols, h, w, hr, hc, lam): the four scans of the parity tests
CASES = [(5, 7, 32, 32, 1, 1, 0.9), (5, 7, 32, 32, 2, 2, 0.9), (4, 6, 48, 40, 2, 1, 0.7),
         (3, 4, 128, 128, 1, 2, 0.9)]
# the grids on which whole rows or columns of the window leave the grid, under 5 x 5
DEGENERATE = [(1, 1), (1, 9), (9, 1), (2, 2)]
DTHRESH = 2.0


@functools.lru_cache(maxsize=None)
def case(rows, cols, h, w, hr, hc, lam, dthresh=None):
    """(T, the oracle's (sigma, W, d, A), the float32 restatement's) of one scan; computed once."""
    T = nlpar_scan(rows, cols, h, w)
    want = nlpar_ref(T, rows, cols, hr, hc, lam, dthresh=dthresh)
    rest = nlpar_ref(T, rows, cols, hr, hc, lam, dthresh=dthresh, dtype=np.float32)
    for arr in want + rest:
        arr.setflags(write=False)
    return T, want, rest
