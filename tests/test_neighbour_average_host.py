"""Host side of the neighbour pattern averaging: the window builders and the validation of
`latice.data_module.NeighbourAverage`, the float64 oracle tests/neighbour_ref.py against a
brute-force loop, and the streaming schedule `latice.index.scan.neighbour_schedule`, simulated
without a device."""
import numpy as np
import pytest
import torch

import neighbour_ref as R
from latice.data_module import (NeighbourAverage, average_neighbour_patterns, neighbour_window)
from latice.index.scan import neighbour_schedule, scan_batches

CROSS = np.array([[0, 1, 0],
                  [1, 1, 1],
                  [0, 1, 0]], np.float32)
DISC = np.array([[0, 0, 1, 0, 0],
                 [0, 1, 1, 1, 0],
                 [1, 1, 1, 1, 1],
                 [0, 1, 1, 1, 0],
                 [0, 0, 1, 0, 0]], np.float32)


def test_named_windows():
    w = neighbour_window("circular", (3, 3))
    assert w.dtype == np.float32 and np.array_equal(w, CROSS)
    w = neighbour_window("circular", (5, 5))
    assert np.array_equal(w, DISC) and w.sum() == 13
    w = neighbour_window("rectangular", (3, 5))
    assert w.shape == (3, 5) and w.dtype == np.float32 and (w == 1).all()
    for shape, std in (((5, 5), 1.0), ((3, 5), 0.7), ((1, 3), 2.5)):
        w = neighbour_window("gaussian", shape, std)
        hr, hc = shape[0] // 2, shape[1] // 2
        want = np.array([[np.exp(-(a * a + b * b) / (2.0 * std * std)) for b in range(-hc, hc + 1)]
                         for a in range(-hr, hr + 1)]).astype(np.float32)
        assert w.shape == shape and w.dtype == np.float32 and np.array_equal(w, want)
        assert w[hr, hc] == 1.0
    # a circular window of unequal sides takes the larger half width as its radius
    assert np.array_equal(neighbour_window("circular", (3, 5)),
                          np.array([[0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [0, 1, 1, 1, 0]], np.float32))


def test_neighbour_average_record():
    na = NeighbourAverage((6, 5))
    assert na.scan_shape == (6, 5) and na.half == (1, 1) and na.reach == 6
    assert np.array_equal(na.weights, CROSS) and not na.weights.flags.writeable
    na = NeighbourAverage([4, 7], window="gaussian", window_shape=(5, 3), std=2.0)
    assert na.half == (2, 1) and na.reach == 15 and na.window_shape == (5, 3)
    assert np.array_equal(na.weights, neighbour_window("gaussian", (5, 3), 2.0))
    # explicit weights override the named window, its shape and std
    wt = np.array([[0.0, 2.0, 0.5]])
    na = NeighbourAverage((2, 2), window="no such window", window_shape=(4, 4), std=-1.0, weights=wt)
    assert na.half == (0, 1) and na.window_shape == (1, 3)
    assert na.weights.dtype == np.float32 and np.array_equal(na.weights, wt.astype(np.float32))
    wt[0, 1] = 7.0                      # a private copy
    assert na.weights[0, 1] == 2.0
    with pytest.raises(Exception):      # frozen
        na.std = 2.0
    na.check(4)
    with pytest.raises(ValueError, match="5 patterns"):
        na.check(5)


@pytest.mark.parametrize("kwargs", [
    dict(window="triangular"),
    dict(window_shape=(4, 3)),                       # an even side
    dict(window_shape=(3, 7)),                       # more than 5
    dict(window_shape=(3,)),
    dict(window="gaussian", std=0.0),
    dict(window="gaussian", std=float("nan")),
    dict(window="gaussian", std=float("inf")),
    dict(weights=np.ones((2, 3))),                   # an even side
    dict(weights=np.ones((7, 1))),                   # more than 5
    dict(weights=np.ones(3)),                        # not 2-D
    dict(weights=np.array([[1.0, -1.0, 1.0]])),      # negative
    dict(weights=np.array([[1.0, 1.0, np.inf]])),    # not finite
    dict(weights=np.array([[np.nan, 1.0, 1.0]])),
    dict(weights=np.array([[1.0, 0.0, 1.0]])),       # centre 0
])
def test_construction_errors(kwargs):
    with pytest.raises(ValueError):
        NeighbourAverage((4, 4), **kwargs)


@pytest.mark.parametrize("scan_shape", [(0, 4), (4, -1), (4,), 12, (1 << 16, 1 << 15)])
def test_scan_shape_errors(scan_shape):
    with pytest.raises(ValueError):
        NeighbourAverage(scan_shape)


def test_there_is_no_cpu_fallback():
    na = NeighbourAverage((2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        average_neighbour_patterns(torch.zeros(6, 1, 16, 16), na)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        average_neighbour_patterns(np.zeros((6, 1, 16, 16), np.float32), na)
    with pytest.raises(TypeError, match="NeighbourAverage"):
        average_neighbour_patterns(torch.zeros(6, 1, 16, 16), CROSS)


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("weights", [CROSS, DISC, neighbour_window("gaussian", (5, 5), 1.0),
                                     neighbour_window("rectangular", (3, 5)),
                                     neighbour_window("rectangular", (5, 1)),
                                     np.array([[0.0, 0.25, 3.0]], np.float32)],
                         ids=["cross", "disc", "gauss5", "rect3x5", "rect5x1", "lopsided"])
def test_oracle_equals_a_brute_force_loop(weights):
    T = R.patterns(12, 4, 6, seed=3)
    got, want = R.average(T, (3, 4), weights), R.brute_force(T, (3, 4), weights)
    assert got.shape == T.shape and got.dtype == np.float64
    assert np.abs(got - want).max() <= 4 * np.finfo(np.float64).eps
    assert np.abs(got - T).max() > 0.01             # it averaged something


def test_oracle_edges():
    T = R.patterns(12, 4, 6, seed=3)
    # corner (0, 0) of a 3 x 4 grid under the cross: itself, its right and its lower neighbour
    got = R.average(T, (3, 4), CROSS)
    want = (T[0].astype(np.float64) + T[1] + T[4]) / 3.0
    assert np.abs(got[0] - want).max() <= 1e-15
    # a 1 x 1 scan is returned as it is, whatever the window
    one = R.patterns(1, 4, 6, seed=4)
    assert np.array_equal(R.average(one, (1, 1), DISC), one.astype(np.float64))
    # the float32 chain of the definition stays inside the parity gate of the device test
    acc, den = np.zeros(T.shape[1:], np.float32), np.float32(0)
    for q in (0, 1, 4):                             # unit weights: fma(1, t, acc) = acc + t
        acc, den = acc + T[q], den + np.float32(1)
    assert acc.dtype == np.float32
    assert np.abs((acc / den).astype(np.float64) - got[0]).max() <= 2 * (3 + 1) * 2.0 ** -24


@pytest.mark.parametrize("scan_shape,weights", [((3, 4), DISC), ((1, 5), CROSS), ((5, 1), DISC),
                                                ((2, 2), np.array([[0.3, 1.0, 2.0]], np.float32))])
def test_a_constant_scan_stays_constant(scan_shape, weights):
    n = scan_shape[0] * scan_shape[1]
    T = np.full((n, 1, 4, 4), 0.3125)
    assert np.array_equal(R.average(T, scan_shape, weights), T)
    ramp = np.broadcast_to(np.linspace(0.0, 1.0, 16).reshape(1, 1, 4, 4), (n, 1, 4, 4))
    assert np.abs(R.average(ramp, scan_shape, weights) - ramp).max() <= 1e-15


# ---------------------------------------------------------------- the schedule
SCHEDULE_CASES = [(30, 5, 1, 1, 7), (30, 5, 2, 2, 5), (30, 5, 1, 1, 64), (7, 7, 0, 2, 3),
                  (7, 1, 2, 0, 2), (1, 1, 1, 1, 4)]


@pytest.mark.parametrize("n,cols,hr,hc,batch", SCHEDULE_CASES)
def test_schedule_simulation(n, cols, hr, hc, batch):
    sched = neighbour_schedule(n, cols, hr, hc, batch)
    chunks = R.simulate(sched, n, cols, hr, hc, batch)
    reach = hr * cols + hc
    assert sched.ring_cap == min(n, batch + 2 * reach)
    # the steps are the staged batches of the scan, one for one
    items = scan_batches(np.zeros((n, 2, 2), np.uint8), batch)
    assert [(st.start, st.stop) for st in sched.steps] == [(s, e) for s, e, _ in items]
    # every output is ready as soon as its last neighbour has been ingested
    done = 0
    for st in sched.steps:
        done = st.ready[-1][1] if st.ready else done
        assert done == (n if st.stop == n else max(0, st.stop - reach))
    assert chunks >= -(-n // batch)


def test_schedule_examples():
    sched = neighbour_schedule(30, 5, 1, 1, 7)        # reach 6, ring 19
    assert sched.ring_cap == 19
    first, second, third = sched.steps[:3]
    assert first.ingest == ((0, 7, 0),) and first.ready == ((0, 1),)
    assert second.ingest == ((7, 14, 7),) and second.ready == ((1, 8),)
    assert third.ingest == ((14, 19, 14), (19, 21, 0)) and third.ready == ((8, 15),)
    assert sched.steps[-1].ingest == ((28, 30, 9),) and sched.steps[-1].ready == ((22, 29), (29, 30))
    # the whole scan in one batch: resident, one chunk
    sched = neighbour_schedule(30, 5, 1, 1, 64)
    assert sched.ring_cap == 30 and len(sched.steps) == 1
    assert sched.steps[0].ingest == ((0, 30, 0),) and sched.steps[0].ready == ((0, 30),)
    assert neighbour_schedule(0, 5, 1, 1, 4).steps == ()
    with pytest.raises(ValueError):
        neighbour_schedule(30, 5, 1, 1, 0)
    with pytest.raises(ValueError):
        neighbour_schedule(30, 0, 1, 1, 4)


# ---------------------------------------------------------------- the C entry's validation
def test_c_entry_rejects_bad_arguments_before_any_launch():
    """Argument validation needs no device: the pointers are only compared with NULL."""
    from latice import _native as N

    def call(ring_cap=30, rows=6, cols=5, p0=0, count=30, hr=1, hc=1, h=16, w=16, src=1, weights=1,
             dst=1):
        N.call("ebsdvae_average_neighbours", src, ring_cap, rows, cols, p0, count, weights, hr, hc,
               h, w, dst, None)

    for kwargs, message in [(dict(hr=3), "hr=3"), (dict(hc=3), "hc=3"), (dict(hr=-1), "hr=-1"),
                            (dict(h=2, w=3), r"h\*w = 6"), (dict(h=0), "multiple of 4"),
                            (dict(ring_cap=16, p0=12, count=5), "ring of 16"),
                            (dict(ring_cap=29), "ring of 29"),
                            (dict(p0=26, count=5), "leaves the 6 x 5 grid"),
                            (dict(count=-1), "leaves the 6 x 5 grid"),
                            (dict(p0=31, count=0), "leaves the 6 x 5 grid"),
                            (dict(rows=0), "grid 0 x 5"), (dict(rows=1 << 16, cols=1 << 15), "grid"),
                            (dict(src=None), "null pointer"), (dict(weights=None), "null pointer"),
                            (dict(dst=None), "null pointer")]:
        with pytest.raises(RuntimeError, match=message):
            call(**kwargs)
    call(count=0)                     # an empty range is valid and launches nothing
    call(p0=30, count=0)
