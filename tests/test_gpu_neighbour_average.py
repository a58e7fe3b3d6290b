"""Neighbour pattern averaging on the device (csrc/neighbour.hip through
latice.data_module.average_neighbour_patterns / average_neighbour_range) and
index_scan(neighbour_average=).

Parity gate against the float64 oracle tests/neighbour_ref.py: 2 (taps + 1) 2^-24 with taps the
number of nonzero weights.  It is derived, not measured: each fma of the chain and the weight sum
round once against a partial sum of at most sum(w), the division rounds once more, and the
values are at most 1.  Everything else is bitwise: a pattern's output is a function of the
transformed patterns, the window and the grid alone, so ranges, ring positions and the streamed
index_scan must reproduce the resident call's bytes."""
import functools

import numpy as np
import pytest
import torch

import neighbour_ref as R
from latice import _native as N
from latice.data_module import (NeighbourAverage, PatternCorrection, average_neighbour_patterns,
                                average_neighbour_range, correct_patterns, ingest_patterns_u8)
from scan_stage_util import clustered_indexer, same_result

pytestmark = pytest.mark.gpu

# (rows, cols, window, window_shape, h, w)
PARITY_CASES = [
    (5, 6, "circular", (3, 3), 16, 16),
    (5, 6, "gaussian", (5, 5), 16, 16),
    (5, 6, "rectangular", (3, 5), 16, 16),
    (5, 6, "rectangular", (5, 3), 16, 16),
    (2, 2, "rectangular", (5, 5), 16, 16),     # the window is larger than the grid
    (1, 7, "rectangular", (5, 5), 16, 16),     # line scans
    (7, 1, "rectangular", (5, 5), 16, 16),
    (1, 1, "circular", (5, 5), 16, 16),
    (3, 4, "gaussian", (5, 5), 128, 128),      # 16 pixel blocks per pattern
    (3, 11, "circular", (5, 5), 8, 12),        # 24 float4 per pattern, runs of 8 + 3 columns
]


def _gate(weights):
    return 2 * (R.taps(weights) + 1) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _case(rows, cols, window, shape, h, w):
    T = R.patterns(rows * cols, h, w, seed=rows * 100 + cols)
    na = NeighbourAverage((rows, cols), window=window, window_shape=shape, std=1.0)
    return T, na, R.average(T, (rows, cols), na.weights)


@pytest.mark.parametrize("rows,cols,window,shape,h,w", PARITY_CASES)
def test_parity(cuda, rows, cols, window, shape, h, w):
    T, na, want = _case(rows, cols, window, shape, h, w)
    x = torch.from_numpy(T).to(cuda)
    got = average_neighbour_patterns(x, na)
    assert got.shape == x.shape and got.dtype == torch.float32 and got.is_cuda
    assert got.data_ptr() != x.data_ptr()
    assert x.cpu().numpy().tobytes() == T.tobytes()          # the source is left alone
    got = got.cpu().numpy()
    err = np.abs(got - want).max()
    print(f"{rows}x{cols} {window} {shape} at {h}x{w}: taps {R.taps(na.weights)} "
          f"max err {err:.2e} gate {_gate(na.weights):.2e}")
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    assert err <= _gate(na.weights), err
    if rows * cols > 1:
        assert np.abs(got - T).max() > 0.01                  # it averaged something


def test_unit_weight_1x1_scan_is_returned_bit_for_bit(cuda):
    T = R.patterns(1, 16, 16, seed=9)
    for shape in ((1, 1), (3, 3), (5, 5)):
        na = NeighbourAverage((1, 1), window="rectangular", window_shape=shape)
        got = average_neighbour_patterns(torch.from_numpy(T).to(cuda), na)
        assert got.cpu().numpy().tobytes() == T.tobytes(), shape


def test_explicit_weights_and_out(cuda):
    wt = np.array([[0.0, 0.5, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 3.0]], np.float32)   # lopsided
    T = R.patterns(30, 16, 16, seed=2)
    na = NeighbourAverage((5, 6), weights=wt)
    x = torch.from_numpy(T).to(cuda)
    out = torch.full((30, 1, 16, 16), -7.0, device=cuda)
    assert average_neighbour_patterns(x, na, out=out) is out
    err = np.abs(out.cpu().numpy() - R.average(T, (5, 6), wt)).max()
    assert err <= _gate(wt), err
    assert len(na._device_state) == 1                        # uploaded once per device
    wdev = na._device_state[x.device]
    average_neighbour_patterns(x, na)
    assert na._device_state[x.device] is wdev
    with pytest.raises(ValueError, match="31 patterns"):
        average_neighbour_patterns(torch.zeros(31, 1, 16, 16, device=cuda), na)
    with pytest.raises(ValueError, match="out must be"):
        average_neighbour_patterns(x, na, out=torch.empty(29, 1, 16, 16, device=cuda))
    with pytest.raises(TypeError, match="NeighbourAverage"):
        average_neighbour_patterns(x, wt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        average_neighbour_patterns(torch.from_numpy(T), na)


def test_a_range_does_not_depend_on_the_call(cuda):
    T = R.patterns(30, 16, 16, seed=5)
    na = NeighbourAverage((6, 5), window="gaussian", window_shape=(5, 5), std=1.0)
    x = torch.from_numpy(T).to(cuda)
    whole = average_neighbour_patterns(x, na).cpu().numpy()
    for ranges in ([(0, 30)], [(0, 7), (7, 23)], [(11, 1)], [(29, 1)]):
        for p0, count in ranges:
            out = torch.full((count + 1, 1, 16, 16), -7.0, device=cuda)
            average_neighbour_range(x, na, p0, count, out)
            host = out.cpu().numpy()
            assert host[:count].tobytes() == whole[p0:p0 + count].tobytes(), (p0, count)
            assert (host[count:] == -7.0).all(), (p0, count)   # nothing past the range is written


def test_ring_addressing(cuda):
    """A 17-slot ring filled by hand: outputs [12, 17) of a 6 x 5 scan under a 3 x 3 window read
    the patterns [6, 23), whose slots 6 .. 16 and then 0 .. 5 wrap past the ring's end."""
    T = R.patterns(30, 16, 16, seed=6)
    na = NeighbourAverage((6, 5), window="rectangular", window_shape=(3, 3))
    whole = average_neighbour_patterns(torch.from_numpy(T).to(cuda), na).cpu().numpy()
    cap, p0, count = 17, 12, 5
    assert cap == count + 2 * na.reach
    ring = np.full((cap, 1, 16, 16), np.nan, np.float32)     # a slot read by mistake shows
    for q in range(p0 - na.reach, p0 + count + na.reach):
        ring[q % cap] = T[q]
    assert not np.isnan(ring).any()                          # exactly the 17 patterns needed
    out = torch.full((count, 1, 16, 16), -7.0, device=cuda)
    average_neighbour_range(torch.from_numpy(ring).to(cuda), na, p0, count, out)
    assert out.cpu().numpy().tobytes() == whole[p0:p0 + count].tobytes()
    # the scan's first and last rows from rings that hold just their neighbourhoods
    for p0, count, lo, hi in ((0, 5, 0, 11), (25, 5, 19, 30)):
        ring = np.full((cap, 1, 16, 16), np.nan, np.float32)
        for q in range(lo, hi):
            ring[q % cap] = T[q]
        out = torch.full((count, 1, 16, 16), -7.0, device=cuda)
        average_neighbour_range(torch.from_numpy(ring).to(cuda), na, p0, count, out)
        assert out.cpu().numpy().tobytes() == whole[p0:p0 + count].tobytes(), p0


def test_c_entry_error_returns(cuda):
    x = torch.zeros(30, 1, 16, 16, device=cuda)
    out = torch.zeros(30, 1, 16, 16, device=cuda)
    wt = torch.ones(49, device=cuda)
    st = N.stream(cuda)

    def call(ring_cap=30, rows=6, cols=5, p0=0, count=30, hr=1, hc=1, h=16, w=16, src=x, weights=wt,
             dst=out):
        N.call("ebsdvae_average_neighbours", N.ptr(src), ring_cap, rows, cols, p0, count,
               N.ptr(weights), hr, hc, h, w, N.ptr(dst), st)

    call()
    call(count=0)
    for kwargs, message in [(dict(hr=3), "hr=3"), (dict(hc=-1), "hc=-1"),
                            (dict(h=2, w=3), "h\\*w = 6"),
                            (dict(ring_cap=16, p0=12, count=5), "ring of 16"),   # needs 5 + 2 * 6
                            (dict(ring_cap=29), "ring of 29"),                   # needs the scan
                            (dict(p0=26, count=5), "leaves the 6 x 5 grid"),
                            (dict(count=-1), "leaves the 6 x 5 grid"),
                            (dict(p0=-1, count=2), "leaves the 6 x 5 grid"),
                            (dict(src=None), "null pointer"), (dict(weights=None), "null pointer"),
                            (dict(dst=None), "null pointer")]:
        with pytest.raises(RuntimeError, match=message):
            call(**kwargs)
    assert not out.cpu().numpy().any()                       # zeros in, zeros out, nothing else


# ---------------------------------------------------------------- index_scan
ROWS, COLS, SIDE = 6, 5, 140
NA_SCAN = dict(window="gaussian", window_shape=(5, 5), std=1.0)


@pytest.fixture(scope="module")
def indexer(cuda, tmp_path_factory):
    """A 6 x 5 scan of uint8 140 x 140 patterns and the clustered dictionary of
    tests/scan_stage_util.py, 60 clusters: a pattern's top match lies in another cluster with
    the averaging than without it."""
    rng = np.random.default_rng(17)
    scan = rng.integers(0, 256, (ROWS * COLS, SIDE, SIDE), dtype=np.uint8)
    na = NeighbourAverage((ROWS, COLS), **NA_SCAN)
    return clustered_indexer(cuda, tmp_path_factory.mktemp("neighbour"), scan,
                             lambda T: average_neighbour_patterns(T, na), rng)


@pytest.mark.parametrize("corrected", [False, True], ids=["plain", "corrected"])
def test_streamed_index_scan_equals_the_resident_one(indexer, corrected):
    ix, scan = indexer
    na = NeighbourAverage((ROWS, COLS), **NA_SCAN)
    kw = dict(top_n=10, orientation_threshold=2.0, min_required_matches=8, return_candidates=True)
    if corrected:
        c = PatternCorrection(dynamic_sigma=4.0, dynamic_mode="subtract")
        ckw = dict(correction=c)
        T = correct_patterns(scan, (128, 128), c)
    else:
        ckw = {}
        T = ingest_patterns_u8(scan, (128, 128))
    want = ix.index_scan(average_neighbour_patterns(T, na), **kw)
    assert len(want) == ROWS * COLS
    for b in (7, 5, 64):                  # several batches and a wrapped ring; the scan in one batch
        got = ix.index_scan(scan, neighbour_average=na, batch_size=b, **ckw, **kw)
        same_result(got, want, f"batch_size={b}")
    # a transformed tensor scan takes the averaging too, and a float scan the same ingest path
    same_result(ix.index_scan(T, neighbour_average=na, batch_size=7, **kw), want, "tensor scan")
    if not corrected:
        same_result(ix.index_scan(scan / 255.0, neighbour_average=na, batch_size=7, **kw), want,
                    "float64 scan")
    # the averaging is not skipped: it changes at least one pattern's top match
    plain = ix.index_scan(scan, batch_size=7, **ckw, **kw)
    assert (plain.top_index != want.top_index).any()
    assert plain.scores.tobytes() != want.scores.tobytes()


def test_index_scan_argument_errors(indexer):
    ix, scan = indexer
    with pytest.raises(TypeError, match="NeighbourAverage"):
        ix.index_scan(scan, neighbour_average=(ROWS, COLS))
    with pytest.raises(ValueError, match="30 patterns"):
        ix.index_scan(scan, neighbour_average=NeighbourAverage((5, 5)))
    with pytest.raises(ValueError, match="12 patterns"):
        ix.index_scan(ingest_patterns_u8(scan[:12], (128, 128)), neighbour_average=NeighbourAverage((5, 5)))
