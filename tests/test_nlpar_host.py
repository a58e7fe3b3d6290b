"""Host side of the non-local pattern averaging: the validation of `latice.data_module.NLPAR`,
the oracle tests/nlpar_ref.py on the scans of the device tests (what it recovers, its two exact
limits, its degenerate grids), the streaming schedule under NLPAR's larger reach, simulated
without a device, and the C entries' refusals before any launch."""
import numpy as np
import pytest
import torch

import neighbour_ref as NR
import nlpar_ref as R
from latice.data_module import NLPAR, nlpar_patterns, nlpar_weights
from latice.index.scan import neighbour_schedule


# ---------------------------------------------------------------- the record
def test_nlpar_record():
    nl = NLPAR((6, 5))
    assert nl.scan_shape == (6, 5) and nl.window_shape == (3, 3) and nl.half == (1, 1)
    assert nl.reach == 2 * 5 + 2
    assert (nl.lam, nl.sigma, nl.sigma_floor, nl.dthresh) == (0.7, None, 1e-3, None)
    nl = NLPAR([4, 7], window_shape=[5, 3], lam=1, sigma=0.05, sigma_floor=1e-2, dthresh=0)
    assert nl.half == (2, 1) and nl.reach == 3 * 7 + 2 and nl.window_shape == (5, 3)
    assert (nl.lam, nl.sigma, nl.sigma_floor, nl.dthresh) == (1.0, 0.05, 0.01, 0.0)
    assert NLPAR((3, 3), window_shape=(1, 1)).reach == 3 + 1      # the ring of the noise estimate
    with pytest.raises(Exception):      # frozen
        nl.lam = 2.0
    nl.check(28)
    with pytest.raises(ValueError, match="5 patterns"):
        nl.check(5)


@pytest.mark.parametrize("kwargs", [
    dict(window_shape=(4, 3)),                       # an even side
    dict(window_shape=(3, 7)),                       # more than 5
    dict(window_shape=(3,)),
    dict(window_shape=(0, 3)),
    dict(lam=0.0), dict(lam=-1.0), dict(lam=float("nan")), dict(lam=float("inf")),
    dict(sigma=0.0), dict(sigma=-0.05), dict(sigma=float("nan")),
    dict(sigma_floor=0.0), dict(sigma_floor=-1e-3), dict(sigma_floor=float("inf")),
    dict(dthresh=-0.5), dict(dthresh=float("nan")),
])
def test_construction_errors(kwargs):
    with pytest.raises(ValueError):
        NLPAR((4, 4), **kwargs)


@pytest.mark.parametrize("scan_shape", [(0, 4), (4, -1), (4,), 12, (1 << 16, 1 << 15)])
def test_scan_shape_errors(scan_shape):
    with pytest.raises(ValueError):
        NLPAR(scan_shape)


def test_there_is_no_cpu_fallback():
    nl = NLPAR((2, 3))
    for fn in (nlpar_patterns, nlpar_weights):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(torch.zeros(6, 1, 16, 16), nl)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(np.zeros((6, 1, 16, 16), np.float32), nl)
        with pytest.raises(TypeError, match="NLPAR"):
            fn(torch.zeros(6, 1, 16, 16), (2, 3))


# ---------------------------------------------------------------- the oracle
def _off_centre(W, d, hr, hc):
    """Mask of the on-grid off-centre entries of a (N, NA, NB) array."""
    on = ~np.isnan(d)
    on[:, hr, hc] = False
    return on


@pytest.mark.parametrize("rows,cols,h,w,hr,hc,lam", R.CASES)
def test_oracle_covers_every_regime(rows, cols, h, w, hr, hc, lam):
    T, (sigma, W, d, A), (sigma32, W32, d32, A32) = R.case(rows, cols, h, w, hr, hc, lam)
    assert sigma.dtype == np.float64 and W.dtype == np.float32 and A.shape == T.shape
    assert np.abs(sigma / 0.05 - 1).max() <= 0.10            # the injected noise is recovered
    on = _off_centre(W, d, hr, hc)
    ww = W[on]
    for name, share in (("kept", (ww > 0.5).mean()), ("partial", ((ww > 0.05) & (ww <= 0.5)).mean()),
                        ("dropped", (ww < 1e-3).mean())):
        assert share >= 0.10, (name, share)
    assert (W[:, hr, hc] == 1).all() and (W[np.isnan(d)] == 0).all()
    assert np.abs(A - T).max() > 0.01                        # it averaged something
    # the float32 restatement stays close: what the device gates are scaled from
    assert np.abs(W32.astype(np.float64) - W).max() <= 1e-5
    assert np.abs(sigma32 / sigma - 1).max() <= 1e-6
    # with the threshold no distance sits at the cut, and both sides are populated
    _, (_, Wc, dc, _), _ = R.case(rows, cols, h, w, hr, hc, lam, R.DTHRESH)
    assert np.abs(dc[on] - R.DTHRESH).min() >= 7e-3
    assert 44 <= (dc[on] > R.DTHRESH).sum() <= 210 and 42 <= (dc[on] <= R.DTHRESH).sum() <= 306
    assert (Wc[on][dc[on] > R.DTHRESH] == 0).all()
    assert np.array_equal(Wc[on][dc[on] <= R.DTHRESH], ww[dc[on] <= R.DTHRESH])


@pytest.mark.parametrize("rows,cols,h,w,hr,hc,lam", R.CASES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fixed_sigma_limits_are_exact(rows, cols, h, w, hr, hc, lam, dtype):
    T = R.nlpar_scan(rows, cols, h, w)
    # sigma far below the noise: every off-centre weight underflows to 0, the scan comes back
    sigma, W, d, A = R.nlpar_ref(T, rows, cols, hr, hc, lam, sigma=1e-4, dtype=dtype)
    assert (W[_off_centre(W, d, hr, hc)] == 0).all()
    assert np.array_equal(A, T.astype(dtype))
    # sigma far above it: every d clamps to 0, every on-grid weight is 1: the rectangular window
    sigma, W, d, A = R.nlpar_ref(T, rows, cols, hr, hc, lam, sigma=10.0, dtype=dtype)
    assert (d[~np.isnan(d)] == 0).all() and (W[~np.isnan(d)] == 1).all()
    if dtype is np.float64:
        rect = NR.average(T, (rows, cols), np.ones((2 * hr + 1, 2 * hc + 1), np.float32))
        assert np.abs(A - rect).max() <= 4 * np.finfo(np.float64).eps


@pytest.mark.parametrize("rows,cols", R.DEGENERATE)
def test_oracle_on_degenerate_grids(rows, cols):
    T = R.nlpar_scan(rows, cols, 32, 32)
    sigma, W, d, A = R.nlpar_ref(T, rows, cols, 2, 2, 0.9)
    assert np.isfinite(A).all() and np.isfinite(sigma).all()
    i, j = np.divmod(np.arange(rows * cols), cols)
    for a in range(-2, 3):
        for b in range(-2, 3):
            on = (i + a >= 0) & (i + a < rows) & (j + b >= 0) & (j + b < cols)
            assert (W[~on, a + 2, b + 2] == 0).all() and np.isnan(d[~on, a + 2, b + 2]).all()
            assert not np.isnan(d[on, a + 2, b + 2]).any()
    if rows * cols == 1:
        assert sigma[0] == np.sqrt(1e-3 ** 2)                # no ring: the floor
        assert np.array_equal(A, T.astype(np.float64))       # a 1 x 1 scan is returned as it is
    else:
        assert np.abs(sigma / 0.05 - 1).max() <= 0.10
    _, W, _, A = R.nlpar_ref(T, rows, cols, 2, 2, 0.9, sigma=10.0)
    rect = NR.average(T, (rows, cols), np.ones((5, 5), np.float32))
    assert np.abs(A - rect).max() <= 4 * np.finfo(np.float64).eps


# ---------------------------------------------------------------- the schedule
SCHEDULE_CASES = [(42, 7, 1, 1, 7), (42, 7, 2, 2, 5), (42, 7, 1, 1, 64), (30, 5, 2, 1, 3),
                  (9, 9, 0, 2, 2), (9, 1, 2, 0, 2), (1, 1, 2, 2, 4), (4, 2, 2, 2, 1)]


@pytest.mark.parametrize("n,cols,hr,hc,batch", SCHEDULE_CASES)
def test_schedule_keeps_what_nlpar_reads(n, cols, hr, hc, batch):
    """index_scan(nlpar=) plans with neighbour_schedule(n, cols, hr + 1, hc + 1, batch).  A ready
    chunk [a, b) reads the on-grid patterns of the flat range [a - reach', b + reach'),
    reach' = (hr + 1) cols + (hc + 1): the distance windows of every centre within hr cols + hc
    of the chunk.  Walk the ring slot by slot: all of them are in their slots, not yet
    overwritten, when the chunk runs."""
    sched = neighbour_schedule(n, cols, hr + 1, hc + 1, batch)
    reach = NLPAR((-(-n // cols), cols), window_shape=(2 * hr + 1, 2 * hc + 1)).reach
    assert reach == (hr + 1) * cols + hc + 1
    cap = sched.ring_cap
    assert cap == min(n, batch + 2 * reach)
    ring = np.full(cap, -1, dtype=np.int64)
    done = 0
    for step in sched.steps:
        for a, b, slot in step.ingest:
            assert slot == a % cap and slot + (b - a) <= cap
            ring[slot:slot + b - a] = np.arange(a, b)
        for a, b in step.ready:
            assert a == done and a < b <= n and b - a <= batch
            q = np.arange(max(0, a - reach), min(n, b + reach))
            assert np.array_equal(ring[q % cap], q), (a, b)
            assert cap >= min(n, (b - a) + 2 * reach)        # what ebsdvae_nlpar_weights asks for
            done = b
    assert done == n
    # and the plain simulation of the widened window holds as it does for the fixed window
    NR.simulate(sched, n, cols, hr + 1, hc + 1, batch)


# ---------------------------------------------------------------- the C entries' validation
def _weights_call(ring_cap=30, rows=6, cols=5, p0=0, count=30, hr=1, hc=1, h=16, w=16, lam=0.7,
                  fixed=0, sigma=0.0, floor=1e-3, cut=0, dthresh=0.0, src=1, weights=1, sigma_out=1,
                  work=1):
    from latice import _native as N
    N.call("ebsdvae_nlpar_weights", src, ring_cap, rows, cols, p0, count, hr, hc, h, w, lam, fixed,
           sigma, floor, cut, dthresh, weights, sigma_out, work, None)


def _average_call(ring_cap=30, rows=6, cols=5, p0=0, count=30, hr=1, hc=1, h=16, w=16, src=1,
                  weights=1, dst=1):
    from latice import _native as N
    N.call("ebsdvae_nlpar_average", src, ring_cap, rows, cols, p0, count, weights, hr, hc, h, w,
           dst, None)


SHAPE_REFUSALS = [(dict(hr=3), "hr=3"), (dict(hc=3), "hc=3"), (dict(hr=-1), "hr=-1"),
                  (dict(h=2, w=3), r"h\*w = 6"), (dict(h=0), "multiple of 4"),
                  (dict(h=4096, w=4096), "below 2\\^24"),
                  (dict(rows=0), "grid 0 x 5"), (dict(rows=1 << 16, cols=1 << 15), "grid")]
RANGE_REFUSALS = [(dict(p0=26, count=5), "leaves the 6 x 5 grid"),
                  (dict(count=-1), "leaves the 6 x 5 grid"),
                  (dict(p0=31, count=0), "leaves the 6 x 5 grid"),
                  (dict(p0=-1, count=2), "leaves the 6 x 5 grid")]


def test_c_entries_reject_bad_arguments_before_any_launch():
    """Argument validation needs no device: the pointers are only compared with NULL."""
    for kwargs, message in SHAPE_REFUSALS + RANGE_REFUSALS + [
            (dict(ring_cap=26, p0=12, count=3), "ring of 26"),        # needs 3 + 2 * 12
            (dict(ring_cap=29), "ring of 29"),                        # needs the scan
            (dict(lam=0.0), "lam="), (dict(lam=-1.0), "lam="), (dict(lam=float("nan")), "lam="),
            (dict(fixed=1, sigma=0.0), "sigma=0"), (dict(fixed=1, sigma=-0.1), "sigma=-0.1"),
            (dict(floor=0.0), "sigma_floor=0"), (dict(floor=-1.0), "sigma_floor=-1"),
            (dict(cut=1, dthresh=-0.5), "dthresh=-0.5"),
            (dict(src=None), "null pointer"), (dict(weights=None), "null pointer"),
            (dict(work=None), "null pointer")]:
        with pytest.raises(RuntimeError, match=message):
            _weights_call(**kwargs)
    for kwargs, message in SHAPE_REFUSALS + RANGE_REFUSALS + [
            (dict(ring_cap=16, p0=12, count=5), "ring of 16"),        # needs 5 + 2 * 6
            (dict(ring_cap=29), "ring of 29"),
            (dict(src=None), "null pointer"), (dict(weights=None), "null pointer"),
            (dict(dst=None), "null pointer")]:
        with pytest.raises(RuntimeError, match=message):
            _average_call(**kwargs)
    # an empty range is valid and launches nothing; ignored values are not checked; sigma_out
    # is optional
    for call in (_weights_call, _average_call):
        call(count=0)
        call(p0=30, count=0)
    _weights_call(count=0, sigma=-1.0, dthresh=-1.0, sigma_out=None)
    _weights_call(count=0, ring_cap=27, p0=12)


def test_work_answers_zero_for_exactly_the_refused_shapes():
    from latice import _native as N

    def work(rows=6, cols=5, count=30, hr=1, hc=1, h=16, w=16):
        return N.call("ebsdvae_nlpar_work", rows, cols, count, hr, hc, h, w)

    for kwargs, _ in SHAPE_REFUSALS:
        assert work(**kwargs) == 0, kwargs
    assert work(count=-1) == 0 and work(count=31) == 0
    # accepted shapes: the partial distances of the centres (the outputs and hr cols + hc each
    # way, the scan at most), offsets of the window widened to 3 x 3, blocks of 1024 pixels,
    # one variance per centre, 16 bytes
    for kw, centres, offsets, blocks in [
            (dict(), 30, 9, 1), (dict(count=3), 15, 9, 1), (dict(count=0), 12, 9, 1),
            (dict(hr=0, hc=0, count=4), 4, 9, 1), (dict(hr=2, hc=1, count=1), 23, 15, 1),
            (dict(hr=2, hc=2, h=128, w=128), 30, 25, 16), (dict(hc=2, h=48, w=40, count=2), 16, 15, 2),
            (dict(rows=1, cols=1, count=1, hr=2, hc=2), 1, 25, 1)]:
        assert work(**kw) == centres * (offsets * blocks + 1) * 4 + 16, kw
