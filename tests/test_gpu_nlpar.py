"""Non-local pattern averaging on the device (csrc/nlpar.hip through
latice.data_module.nlpar_weights / nlpar_patterns / nlpar_range) and index_scan(nlpar=).

The oracle is tests/nlpar_ref.py in float64.  The gates are computed by the test from the
float32 restatement of the same input (the oracle's formulas with every operation rounded to
float32), with the project's 4 x margin, and never from what the kernels give:

    sigma     relative, 4 x the restatement's deviation, not below 4 * 2^-24 (three roundings
              after a double sum)
    weights   absolute, 4 x the restatement's max |dW|, not below 8 * 2^-24
    A         against the float64 chain run on the kernel's own weights: 2 (taps + 1) 2^-24, the
              derived gate of tests/test_gpu_neighbour_average.py
    A         against the full oracle: 2 taps gate_W + 2 (taps + 1) 2^-24 (the weight sum is at
              least 1, the values at most 1)

With `dthresh` a weight whose reference d lies within 1e-3 of the threshold is left out with its
pattern's outputs (at most 2 % may be; with these seeds none is).  Everything else is bitwise:
sigma, weights and outputs are functions of the transformed patterns, the grid and the
parameters alone."""
import functools

import numpy as np
import pytest
import torch

import neighbour_ref as NR
import nlpar_ref as R
from latice import _native as N
from latice.data_module import (NLPAR, NeighbourAverage, PatternCorrection,
                                average_neighbour_patterns, average_neighbour_range,
                                correct_patterns, ingest_patterns, ingest_patterns_u8,
                                nlpar_patterns, nlpar_range, nlpar_weights)
from latice.patterns import _nlpar_weights_range
from scan_stage_util import clustered_indexer, same_result

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# the four scans (one pixel block; a partial second block; the model's size, 16 blocks; both
# rectangular windows) and the degenerate grids under 5 x 5
PARITY_CASES = R.CASES + [(rows, cols, 32, 32, 2, 2, 0.9) for rows, cols in R.DEGENERATE]


def _nlpar(rows, cols, hr, hc, lam, **kw):
    return NLPAR((rows, cols), window_shape=(2 * hr + 1, 2 * hc + 1), lam=lam, **kw)


@functools.lru_cache(maxsize=None)
def _device(dev, rows, cols, h, w, hr, hc, lam, dthresh=None, sigma=None):
    """(sigma, weights, A) of one scan from the device, as numpy arrays; run once per case."""
    T = R.nlpar_scan(rows, cols, h, w)
    x = torch.tensor(T).to(dev)
    nl = _nlpar(rows, cols, hr, hc, lam, dthresh=dthresh, sigma=sigma)
    W, sigma_p = nlpar_weights(x, nl)
    A = nlpar_patterns(x, nl)
    assert W.shape == (rows * cols, 2 * hr + 1, 2 * hc + 1) and W.dtype == torch.float32 and W.is_cuda
    assert sigma_p.shape == (rows * cols,) and sigma_p.dtype == torch.float32
    assert A.shape == x.shape and A.dtype == torch.float32 and A.data_ptr() != x.data_ptr()
    assert x.cpu().numpy().tobytes() == T.tobytes()          # the source is left alone
    return sigma_p.cpu().numpy(), W.cpu().numpy(), A.cpu().numpy()


@pytest.mark.parametrize("dthresh", [None, R.DTHRESH], ids=["all", "dthresh"])
@pytest.mark.parametrize("rows,cols,h,w,hr,hc,lam", PARITY_CASES)
def test_parity(cuda, rows, cols, h, w, hr, hc, lam, dthresh):
    T, (sigma, W, d, A), (sigma32, W32, _, _) = R.case(rows, cols, h, w, hr, hc, lam, dthresh)
    got_sigma, got_W, got_A = _device(cuda, rows, cols, h, w, hr, hc, lam, dthresh)
    taps = (2 * hr + 1) * (2 * hc + 1)
    gate_sigma = max(4 * np.abs(sigma32 / sigma - 1).max(), 4 * U)
    gate_W = max(4 * np.abs(W32.astype(np.float64) - W).max(), 8 * U)
    # what is left out: weights whose reference d sits at the threshold, and their patterns
    near = np.zeros(W.shape, bool) if dthresh is None else np.abs(d - dthresh) < 1e-3
    keep = ~near.any(axis=(1, 2))
    assert near.mean() <= 0.02
    err_sigma = np.abs(got_sigma / sigma - 1).max()
    err_W = np.abs(got_W.astype(np.float64) - W)[~near].max()
    own = R.weighted_mean(T, rows, cols, got_W)              # the float64 chain on the kernel's weights
    err_own = np.abs(got_A - own).max()
    err_A = np.abs(got_A - A)[keep].max()
    gate_own = 2 * (taps + 1) * U
    gate_A = 2 * taps * gate_W + gate_own
    print(f"{rows}x{cols} at {h}x{w} window {2 * hr + 1}x{2 * hc + 1} dthresh {dthresh}: "
          f"sigma {err_sigma:.2e} (gate {gate_sigma:.2e}) W {err_W:.2e} (gate {gate_W:.2e}) "
          f"A own weights {err_own:.2e} (gate {gate_own:.2e}) A {err_A:.2e} (gate {gate_A:.2e}) "
          f"left out {int(near.sum())}")
    assert np.isfinite(got_A).all() and got_A.min() >= 0.0 and got_A.max() <= 1.0 + gate_own
    assert (got_W[:, hr, hc] == 1).all()                     # the centre weight is exactly 1
    assert (got_W[np.isnan(d)] == 0).all()                   # off-grid weights are exactly 0
    if dthresh is not None:
        far = ~near & ~np.isnan(d)
        assert (got_W[far & (d > dthresh)] == 0).all()
        assert (got_W[far & (d <= dthresh)] > 0).all()
    assert err_sigma <= gate_sigma, err_sigma
    assert err_W <= gate_W, err_W
    assert err_own <= gate_own, err_own
    assert err_A <= gate_A, err_A
    if rows * cols == 1:
        assert got_A.tobytes() == T.tobytes()                # a 1 x 1 scan is returned as it is
    elif dthresh is None and (rows, cols) not in R.DEGENERATE:
        assert np.abs(got_A - T).max() > 0.01                # it averaged something


@pytest.mark.parametrize("rows,cols,h,w,hr,hc,lam", PARITY_CASES)
def test_fixed_sigma_limits_are_bitwise(cuda, rows, cols, h, w, hr, hc, lam):
    T = R.nlpar_scan(rows, cols, h, w)
    # sigma = 1e-4: every off-centre weight is exactly 0 and the scan comes back
    sigma_p, W, A = _device(cuda, rows, cols, h, w, hr, hc, lam, None, 1e-4)
    centre = np.zeros(W.shape, bool)
    centre[:, hr, hc] = True
    assert (W[centre] == 1).all() and (W[~centre] == 0).all()
    assert A.tobytes() == T.tobytes()
    assert np.abs(sigma_p / 1e-4 - 1).max() <= 4 * U          # sqrtf(float32(sigma^2))
    # sigma = 10: every on-grid weight is exactly 1: the rectangular window of the fixed averaging
    sigma_p, W, A = _device(cuda, rows, cols, h, w, hr, hc, lam, None, 10.0)
    d = R.nlpar_ref(T, rows, cols, hr, hc, lam, sigma=10.0)[2]
    assert (W[~np.isnan(d)] == 1).all() and (W[np.isnan(d)] == 0).all()
    rect = NeighbourAverage((rows, cols), window="rectangular", window_shape=(2 * hr + 1, 2 * hc + 1))
    want = average_neighbour_patterns(torch.tensor(T).to(cuda), rect)
    assert A.tobytes() == want.cpu().numpy().tobytes()
    assert np.abs(sigma_p / 10.0 - 1).max() <= 4 * U


RANGE_SCAN = (6, 5, 48, 40)     # 30 patterns, two pixel blocks


@pytest.mark.parametrize("hr,hc,dthresh", [(1, 1, None), (2, 2, R.DTHRESH), (0, 2, None), (0, 0, None)])
def test_a_range_does_not_depend_on_the_call(cuda, hr, hc, dthresh):
    rows, cols, h, w = RANGE_SCAN
    T = R.nlpar_scan(*RANGE_SCAN)
    nl = _nlpar(rows, cols, hr, hc, 0.8, dthresh=dthresh)
    x = torch.tensor(T).to(cuda)
    whole = nlpar_patterns(x, nl).cpu().numpy()
    W, sigma = (t.cpu().numpy() for t in nlpar_weights(x, nl))
    assert nlpar_patterns(x, nl).cpu().numpy().tobytes() == whole.tobytes()     # two runs
    W2, sigma2 = (t.cpu().numpy() for t in nlpar_weights(x, nl))
    assert W2.tobytes() == W.tobytes() and sigma2.tobytes() == sigma.tobytes()
    for p0, count in ((0, 30), (0, 7), (7, 23), (11, 1), (29, 1), (4, 2), (13, 9)):
        out = torch.full((count + 1, 1, h, w), -7.0, device=cuda)
        assert nlpar_range(x, nl, p0, count, out) is out
        host = out.cpu().numpy()
        assert host[:count].tobytes() == whole[p0:p0 + count].tobytes(), (p0, count)
        assert (host[count:] == -7.0).all(), (p0, count)     # nothing past the range is written
        Wr, sr = _nlpar_weights_range(x, nl, p0, count)
        assert Wr.cpu().numpy().tobytes() == W[p0:p0 + count].tobytes(), (p0, count)
        assert sr.cpu().numpy().tobytes() == sigma[p0:p0 + count].tobytes(), (p0, count)


def test_ring_addressing(cuda):
    """A 27-slot ring filled by hand: outputs [13, 16) of a 6 x 5 scan under a 3 x 3 window read
    the patterns [1, 28) (reach' = 2 * 5 + 2), whose slots 1 .. 26 and then 0 wrap past the
    ring's end.  Every other slot holds NaN: a pattern read by mistake shows."""
    rows, cols, h, w = RANGE_SCAN
    T = R.nlpar_scan(*RANGE_SCAN)
    nl = _nlpar(rows, cols, 1, 1, 0.8)
    x = torch.tensor(T).to(cuda)
    whole = nlpar_patterns(x, nl).cpu().numpy()
    W, sigma = (t.cpu().numpy() for t in nlpar_weights(x, nl))
    cap = 27
    assert cap == 3 + 2 * nl.reach
    # the middle of the scan, then its first and last rows from rings that hold just what they read
    for p0, count, lo, hi in ((13, 3, 1, 28), (0, 3, 0, 15), (27, 3, 15, 30)):
        assert (lo, hi) == (max(0, p0 - nl.reach), min(30, p0 + count + nl.reach))
        ring = np.full((cap, 1, h, w), np.nan, np.float32)
        for q in range(lo, hi):
            ring[q % cap] = T[q]
        assert np.isnan(ring).any() == (hi - lo < cap)
        dev_ring = torch.from_numpy(ring).to(cuda)
        out = torch.full((count, 1, h, w), -7.0, device=cuda)
        nlpar_range(dev_ring, nl, p0, count, out)
        assert out.cpu().numpy().tobytes() == whole[p0:p0 + count].tobytes(), p0
        Wr, sr = _nlpar_weights_range(dev_ring, nl, p0, count)
        assert Wr.cpu().numpy().tobytes() == W[p0:p0 + count].tobytes(), p0
        assert sr.cpu().numpy().tobytes() == sigma[p0:p0 + count].tobytes(), p0
    with pytest.raises(RuntimeError, match="ring of 26"):
        nlpar_range(torch.zeros(26, 1, h, w, device=cuda), nl, 13, 3, out)


def _guarded(n, dev):
    """A float32 buffer of n values with a guard band of 64 behind it, all -7."""
    return torch.full((n + 64,), -7.0, device=dev)


def test_out_is_honoured_and_guard_bands_stay(cuda):
    rows, cols, h, w = RANGE_SCAN
    T = R.nlpar_scan(*RANGE_SCAN)
    nl = _nlpar(rows, cols, 2, 1, 0.8)
    x = torch.tensor(T).to(cuda)
    want = nlpar_patterns(x, nl)
    W, sigma = nlpar_weights(x, nl)
    out = torch.full((30, 1, h, w), -7.0, device=cuda)
    assert nlpar_patterns(x, nl, out=out) is out
    assert torch.equal(out, want)
    with pytest.raises(ValueError, match="out must be"):
        nlpar_patterns(x, nl, out=torch.empty(29, 1, h, w, device=cuda))
    with pytest.raises(ValueError, match="31 patterns"):
        nlpar_patterns(torch.zeros(31, 1, h, w, device=cuda), nl)
    # the C entries on guarded buffers: a range in the middle, every output and the scratch
    p0, count, (hr, hc) = 9, 8, nl.half
    nbytes = N.call("ebsdvae_nlpar_work", rows, cols, count, hr, hc, h, w)
    assert nbytes > 0 and nbytes % 4 == 0
    gw, gs, gd, gk = (_guarded(n, cuda) for n in (count * 15, count, count * h * w, nbytes // 4))
    st = N.stream(cuda)
    N.call("ebsdvae_nlpar_weights", N.ptr(x), 30, rows, cols, p0, count, hr, hc, h, w, nl.lam, 0, 0.0,
           nl.sigma_floor, 0, 0.0, N.ptr(gw), N.ptr(gs), N.ptr(gk), st)
    N.call("ebsdvae_nlpar_average", N.ptr(x), 30, rows, cols, p0, count, N.ptr(gw), hr, hc, h, w,
           N.ptr(gd), st)
    for name, buf, ref in (("weights", gw, W[p0:p0 + count]), ("sigma", gs, sigma[p0:p0 + count]),
                           ("patterns", gd, want[p0:p0 + count]), ("work", gk, None)):
        assert (buf[-64:] == -7.0).all(), name
        if ref is not None:
            assert torch.equal(buf[:-64], ref.reshape(-1)), name
    # a refused call writes nothing
    gw2 = _guarded(count * 15, cuda)
    with pytest.raises(RuntimeError, match="lam="):
        N.call("ebsdvae_nlpar_weights", N.ptr(x), 30, rows, cols, p0, count, hr, hc, h, w, 0.0, 0,
               0.0, nl.sigma_floor, 0, 0.0, N.ptr(gw2), N.ptr(gs), N.ptr(gk), st)
    assert (gw2 == -7.0).all()


# ---------------------------------------------------------------- the shared chain
# (rows, cols, h, w, window, window_shape, p0, count): count None is the whole scan; a window
# that is an array is explicit weights
SAME_CHAIN_CASES = [
    (5, 6, 16, 16, "circular", (3, 3), 0, None),
    (5, 6, 16, 16, "gaussian", (5, 5), 0, None),
    (5, 6, 16, 16, "rectangular", (3, 5), 0, None),
    (5, 6, 16, 16, "rectangular", (5, 3), 0, None),
    (5, 6, 16, 16, "rectangular", (1, 1), 0, None),
    (3, 11, 8, 12, "circular", (5, 5), 0, None),        # runs of 8 + 3 columns
    (1, 7, 16, 16, "rectangular", (5, 5), 0, None),     # line scans
    (7, 1, 16, 16, "rectangular", (5, 5), 0, None),
    (5, 6, 16, 16, "gaussian", (5, 5), 7, 16),          # both ends of the range clip a run
    # on-grid neighbour rows whose weights are all zero: the fixed averaging does not load them
    (5, 6, 16, 16, ((0, 0, 0), (1, 2, 0.5), (0, 0, 0)), (3, 3), 0, None),
    (5, 6, 16, 16, ((0, 3, 0), (0, 0, 0), (1, 2, 1), (0, 0, 0), (0, 0, 0)), (5, 3), 7, 16),
]


@pytest.mark.parametrize("rows,cols,h,w,window,shape,p0,count", SAME_CHAIN_CASES)
def test_average_with_fixed_weights_is_the_fixed_averaging(cuda, rows, cols, h, w, window, shape,
                                                           p0, count):
    """ebsdvae_nlpar_average with the per-output weights W[a][b] where the tap is on the grid
    and 0 where it is off gives the bytes of ebsdvae_average_neighbours with W: a dropped tap
    enters both chains as weight 0, and for finite patterns fma(0, t, s) == s."""
    count = rows * cols - p0 if count is None else count
    if isinstance(window, str):
        na = NeighbourAverage((rows, cols), window=window, window_shape=shape, std=1.0)
    else:
        na = NeighbourAverage((rows, cols), weights=np.array(window, np.float32))
    (hr, hc), W = na.half, na.weights
    assert W.shape == shape
    x = torch.from_numpy(NR.patterns(rows * cols, h, w, seed=rows * 100 + cols)).to(cuda)
    i, j = np.divmod(np.arange(p0, p0 + count), cols)
    per_output = np.zeros((count,) + W.shape, np.float32)
    for a in range(-hr, hr + 1):
        for b in range(-hc, hc + 1):
            on = (i + a >= 0) & (i + a < rows) & (j + b >= 0) & (j + b < cols)
            per_output[on, a + hr, b + hc] = W[a + hr, b + hc]
    want = torch.full((count + 1, 1, h, w), -7.0, device=cuda)
    average_neighbour_range(x, na, p0, count, want)
    got = torch.full((count + 1, 1, h, w), -7.0, device=cuda)
    N.call("ebsdvae_nlpar_average", N.ptr(x), rows * cols, rows, cols, p0, count,
           N.ptr(torch.from_numpy(per_output).to(cuda)), hr, hc, h, w, N.ptr(got), N.stream(cuda))
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert got.tobytes() == want.tobytes()
    assert (got[count:] == -7.0).all() and np.isfinite(got[:count]).all()
    if rows * cols > 1 and shape != (1, 1):
        assert np.abs(got[:count] - x.cpu().numpy()[p0:p0 + count]).max() > 0.01   # it averaged


# ---------------------------------------------------------------- index_scan
ROWS, COLS, SIDE = 6, 7, 140
NL_SCAN = dict(window_shape=(3, 5), lam=0.9)


@pytest.fixture(scope="module")
def indexer(cuda, tmp_path_factory):
    """The two-grain 6 x 7 scan as uint8 140 x 140 detector patterns and the clustered
    dictionary of tests/scan_stage_util.py around the latents of the scan as ingested and as
    NLPAR-averaged."""
    scan = np.round(R.nlpar_scan(ROWS, COLS, SIDE, SIDE)[:, 0] * 255.0).astype(np.uint8)
    nl = NLPAR((ROWS, COLS), **NL_SCAN)
    return clustered_indexer(cuda, tmp_path_factory.mktemp("nlpar"), scan,
                             lambda T: nlpar_patterns(T, nl), np.random.default_rng(23))


@pytest.mark.parametrize("corrected", [False, True], ids=["plain", "corrected"])
@pytest.mark.parametrize("staging", ["uint8", "float32"])
def test_streamed_index_scan_equals_the_resident_one(indexer, staging, corrected):
    ix, scan = indexer
    nl = NLPAR((ROWS, COLS), **NL_SCAN)
    kw = dict(top_n=10, orientation_threshold=2.0, min_required_matches=8, return_candidates=True)
    if staging == "float32":
        scan = scan.astype(np.float32) / np.float32(255.0)
    if corrected:
        c = PatternCorrection(dynamic_sigma=4.0, dynamic_mode="subtract")
        ckw = dict(correction=c)
        T = correct_patterns(scan, (128, 128), c)
    else:
        ckw = {}
        T = (ingest_patterns_u8 if staging == "uint8" else ingest_patterns)(scan, (128, 128))
    want = ix.index_scan(nlpar_patterns(T, nl), **kw)
    assert len(want) == ROWS * COLS
    for b in (7, 5, 64):                  # several batches and a wrapped ring; the scan in one batch
        got = ix.index_scan(scan, nlpar=nl, batch_size=b, **ckw, **kw)
        same_result(got, want, f"batch_size={b}")
    # a transformed tensor scan takes it too
    same_result(ix.index_scan(T, nlpar=nl, batch_size=7, **kw), want, "tensor scan")
    # it is not skipped: the scores differ from the plain scan's
    plain = ix.index_scan(scan, batch_size=7, **ckw, **kw)
    assert plain.scores.tobytes() != want.scores.tobytes()


def test_index_scan_argument_errors(indexer):
    ix, scan = indexer
    nl = NLPAR((ROWS, COLS), **NL_SCAN)
    with pytest.raises(ValueError, match="not both"):
        ix.index_scan(scan, nlpar=nl, neighbour_average=NeighbourAverage((ROWS, COLS)))
    with pytest.raises(TypeError, match="NLPAR"):
        ix.index_scan(scan, nlpar=(ROWS, COLS))
    with pytest.raises(ValueError, match="42 patterns"):
        ix.index_scan(scan, nlpar=NLPAR((5, 5)))
    with pytest.raises(ValueError, match="12 patterns"):
        ix.index_scan(ingest_patterns_u8(scan[:12], (128, 128)), nlpar=NLPAR((5, 5)))
