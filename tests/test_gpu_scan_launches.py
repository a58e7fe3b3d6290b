"""Which pattern-stage entry points a scan calls, in which order and on how many patterns:
`index_scan` and `scan_background` under a recorder of `latice._native.call`, for every route of
the scan's ingest plan (latice.patterns.ScanIngest) and both neighbour-averaged loops.  The
expected sequences are literal: they were recorded from the per-batch dispatch the plan replaced
and follow from `scan_batches` and `neighbour_schedule` by hand (12 patterns in batches of 5 on a
3 x 4 grid: batches (0, 5), (5, 10), (10, 12)).

The fixture is that of tests/test_gpu_resample.py: 12 uint8 patterns of 150 x 170, the seeded
128 x 128 model and a 64-row dictionary."""
import contextlib

import numpy as np
import pytest
import torch

import correction_ref as C
from latice import _native as N
from latice.data_module import DetectorResample, NeighbourAverage, PatternCorrection
from latice.index import faiss_db as F
from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig
from latice.model import VariationalAutoEncoderRawData
from latice.seeding import seeded_state_dict

pytestmark = pytest.mark.gpu

INGEST, INGEST_U8 = "ebsdvae_ingest_patterns", "ebsdvae_ingest_patterns_u8"
RESAMPLE, CORRECT = "ebsdvae_resample_patterns", "ebsdvae_correct_patterns"
AVERAGE, ACCUMULATE = "ebsdvae_average_neighbours", "ebsdvae_accumulate_patterns"
# position of the batch size B among each entry's arguments (include/ebsdvae.h)
B_ARG = {INGEST: 2, INGEST_U8: 1, RESAMPLE: 2, CORRECT: 2, ACCUMULATE: 2}
SRC_ARG, RESAMPLE_DST_ARG = 0, 18


@contextlib.contextmanager
def recording():
    """Every call of the six entries while the block runs, as (name, arguments)."""
    calls, real = [], N.call

    def call(name, *a):
        if name in B_ARG or name == AVERAGE:
            calls.append((name, a))
        return real(name, *a)

    N.call = call
    try:
        yield calls
    finally:
        N.call = real


def sequence(calls):
    """(entry, B) per call; (entry, p0, count) for the neighbour average, which has no B."""
    return [(name, a[4], a[5]) if name == AVERAGE else (name, a[B_ARG[name]]) for name, a in calls]


@pytest.fixture(scope="module")
def indexer(cuda, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("launches")
    m = VariationalAutoEncoderRawData(32, 16, 128)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0, 32, 16, 128).items()})
    rng = np.random.default_rng(5)
    db = F.FaissLatentVectorDatabase(F.FaissLatentVectorDatabaseConfig(dimension=16, device="cuda:0"))
    db.add_vectors(rng.standard_normal((64, 16)).astype(np.float32),
                   rng.uniform(0.0, 90.0, (64, 3)))
    cfg = IndexerConfig(pattern_path=tmp / "unused.npy", angles_path=tmp / "unused.txt",
                        batch_size=5, device="cuda", image_size=(128, 128))
    return DiffractionPatternIndexer(m.to(cuda), db=db, config=cfg)


@pytest.fixture(scope="module")
def scan():
    return C.detector_patterns(12, 150, 170, seed=77)


def _record(run):
    with recording() as calls:
        run()
    torch.cuda.synchronize()
    return calls


def test_plain_uint8(indexer, scan):
    calls = _record(lambda: indexer.index_scan(scan[0]))
    assert sequence(calls) == [(INGEST_U8, 5), (INGEST_U8, 5), (INGEST_U8, 2)]


def test_uint8_with_a_resample(indexer, scan):
    calls = _record(lambda: indexer.index_scan(scan[0], resample=DetectorResample()))
    assert sequence(calls) == [(RESAMPLE, 5), (RESAMPLE, 5), (RESAMPLE, 2)]


def test_float32_with_a_resample(indexer, scan):
    raw = scan[0].astype(np.float32) / np.float32(255)
    calls = _record(lambda: indexer.index_scan(raw, resample=DetectorResample()))
    assert sequence(calls) == [(RESAMPLE, 5), (INGEST, 5), (RESAMPLE, 5), (INGEST, 5),
                               (RESAMPLE, 2), (INGEST, 2)]
    # one intermediate for the whole scan: every batch is binned into it and ingested from it
    mids = {a[RESAMPLE_DST_ARG] for name, a in calls if name == RESAMPLE}
    assert len(mids) == 1 and mids == {a[SRC_ARG] for name, a in calls if name == INGEST}


def test_uint8_with_a_resample_and_a_correction(indexer, scan):
    raw, bg = scan
    c = PatternCorrection(static_background=C.static_background(bg, "subtract"),
                          static_mode="subtract", dynamic_sigma=2.0, dynamic_mode="divide")
    calls = _record(lambda: indexer.index_scan(raw, resample=DetectorResample(), correction=c))
    # the first batch also bins the static background, once, as one pattern
    assert sequence(calls) == [(RESAMPLE, 5), (RESAMPLE, 1), (CORRECT, 5), (RESAMPLE, 5), (CORRECT, 5),
                               (RESAMPLE, 2), (CORRECT, 2)]
    mids = {a[RESAMPLE_DST_ARG] for name, a in calls if name == RESAMPLE and a[B_ARG[name]] != 1}
    assert len(mids) == 1 and mids == {a[SRC_ARG] for name, a in calls if name == CORRECT}


def test_uint8_with_a_resample_and_a_neighbour_average(indexer, scan):
    # reach 5, a ring of all 12: nothing is complete after (0, 5), (0, 5) after (5, 10), the rest
    # after the last batch in chunks of at most 5
    calls = _record(lambda: indexer.index_scan(scan[0], resample=DetectorResample(),
                                               neighbour_average=NeighbourAverage((3, 4))))
    assert sequence(calls) == [(RESAMPLE, 5), (RESAMPLE, 5), (AVERAGE, 0, 5), (RESAMPLE, 2),
                               (AVERAGE, 5, 5), (AVERAGE, 10, 2)]


def test_a_batch_that_passes_the_rings_end(indexer, scan):
    # reach 1, a ring of 7 slots: the batch at 5 is ingested as (5, 7) and (7, 10)
    na = NeighbourAverage((3, 4), weights=np.ones((1, 3)))
    calls = _record(lambda: indexer.index_scan(scan[0], neighbour_average=na))
    assert sequence(calls) == [(INGEST_U8, 5), (AVERAGE, 0, 4), (INGEST_U8, 2), (INGEST_U8, 3),
                               (AVERAGE, 4, 5), (INGEST_U8, 2), (AVERAGE, 9, 3)]


def test_scan_background(indexer, scan):
    calls = _record(lambda: indexer.scan_background(scan[0]))
    assert sequence(calls) == [(ACCUMULATE, 5), (ACCUMULATE, 5), (ACCUMULATE, 2)]
