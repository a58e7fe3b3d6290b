"""Host-side batching of `DiffractionPatternIndexer.index_scan` (latice/index/scan.py): a scan
is cut into (start, stop, dtype code) work items.  numpy only: no GPU, no library load."""
import numpy as np
import pytest

from latice.index import scan as S


def _covers(items, n, batch):
    assert [i[0] for i in items] == list(range(0, n, batch))
    assert all(b - a == batch for a, b, _ in items[:-1])
    assert items[-1][1] == n and 0 < items[-1][1] - items[-1][0] <= batch
    assert all(items[i][1] == items[i + 1][0] for i in range(len(items) - 1))


@pytest.mark.parametrize("dtype,code", [(np.float64, S.SCAN_F64), (np.float32, S.SCAN_F32),
                                        (np.uint8, S.SCAN_U8)])
@pytest.mark.parametrize("n,batch", [(48, 16), (37, 16), (5, 16), (16, 16), (1, 1)])
def test_work_items_cover_the_scan(dtype, code, n, batch):
    src = np.zeros((n, 6, 5), dtype=dtype)
    items = S.scan_batches(src, batch)
    assert len(items) == -(-n // batch)
    _covers(items, n, batch)
    assert {c for _, _, c in items} == {code}
    assert S.SCAN_NUMPY_DTYPES[code] == dtype


def test_memmap_by_path(tmp_path):
    raw = np.arange(37 * 4 * 3, dtype=np.uint8).reshape(37, 4, 3)
    np.save(tmp_path / "scan.npy", raw)
    src = S.open_scan(tmp_path / "scan.npy")
    assert isinstance(src, np.memmap) and not src.flags.writeable
    items = S.scan_batches(src, 16)
    assert items == [(0, 16, S.SCAN_U8), (16, 32, S.SCAN_U8), (32, 37, S.SCAN_U8)]
    assert np.array_equal(np.concatenate([src[a:b] for a, b, _ in items]), raw)
    assert S.open_scan(str(tmp_path / "scan.npy")).shape == (37, 4, 3)
    assert S.open_scan(raw) is raw
    with pytest.raises(ValueError, match="npy"):
        S.open_scan(tmp_path / "scan.h5")


def test_other_dtypes_are_staged_as_float64():
    # what ingest_patterns does with them: raw values as float64
    for dt in (np.uint16, np.int32, np.float16, bool):
        assert S.scan_dtype_code(dt) == S.SCAN_F64
    assert S.scan_batches(np.zeros((3, 2, 2), np.uint16), 2) == [(0, 2, S.SCAN_F64), (2, 3, S.SCAN_F64)]


def test_empty_scan_has_no_work():
    assert S.scan_batches(np.zeros((0, 4, 4), np.uint8), 16) == []


@pytest.mark.parametrize("shape", [(8, 8), (4, 1, 8, 8)])
def test_rejects_scans_that_are_not_3d(shape):
    with pytest.raises(ValueError, match="N, H0, W0"):
        S.scan_batches(np.zeros(shape, np.float32), 16)


def test_rejects_bad_arguments():
    with pytest.raises(TypeError):
        S.scan_batches([[1.0]], 16)
    with pytest.raises(ValueError, match="batch_size"):
        S.scan_batches(np.zeros((3, 2, 2)), 0)


def test_result_record():
    r = S.ScanIndexResult(orientations=np.zeros((4, 3)), success=np.zeros(4, bool),
                          scores=np.zeros(4, np.float32), top_index=np.zeros(4, np.int64),
                          n_similar=np.zeros(4, np.int32))
    assert len(r) == 4 and r.candidate_indices is None and r.candidate_scores is None
