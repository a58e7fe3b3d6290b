"""The host side of the scan maps (latice/index/maps.py): the float64 reference tests/maps_ref.py
against the reference's recorded IPF colours and against hand-worked grids, the `ScanMaps` record,
the argument checks that come before any launch, and the new `ScanIndexResult` fields.  No GPU."""
import os

import numpy as np
import pytest
import torch

import maps_ref as M
from conftest import GOLDEN
from latice.index import (ScanMaps, ipf_colors, kernel_average_misorientation,
                          orientation_similarity_map)
from latice.index import maps as L
from latice.index.scan import ScanIndexResult


def ipf_gate(got, want):
    """The gate of the IPF colours, on the host and on the device: no colour channel differs by
    more than one level, and at most 0.5 % of the colours differ at all.  (A float32 port of the
    reference misses it: 0.1 % of its colours are off by up to 4 levels.)"""
    assert got.shape == want.shape and got.dtype == np.uint8
    diff = np.abs(got.astype(int) - want.astype(int)).reshape(-1, 3).max(axis=1)
    print(f"ipf: {len(diff)} colours, max level difference {diff.max(initial=0)}, "
          f"{(diff > 0).sum()} differ")
    assert diff.max(initial=0) <= 1
    assert (diff > 0).sum() <= 0.005 * len(diff)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "ipf_colors.npz"))
    assert g["euler"].shape == (1040, 3) and (g["euler"][1024:1032, 1] == 0).all()
    return g


@pytest.mark.parametrize("direction", ["x", "y", "z"])
def test_reference_ipf_matches_the_recorded_colours(golden, direction):
    ipf_gate(M.ipf(golden["euler"], direction), golden["ipf_" + direction])


def test_recorded_colours_cover_the_sector(golden):
    z = golden["ipf_z"]
    assert (z[1024:1032] == [255, 0, 0]).all()          # the exact [001] pole is red
    assert z[:, 0].max() == z[:, 1].max() == z[:, 2].max() == 255
    assert (z.max(axis=1) == 255).all()                 # every colour is normalised to its maximum
    assert M.ipf([[np.nan, 1.0, 2.0], [0.0, np.inf, 0.0]]).tolist() == [[0, 0, 0], [0, 0, 0]]


# top-3 rows on a 2 x 2 grid: (0,0) shares {2, 3} with (0,1) and {1} with (1,0); (1,1) shares {9}
# with (1,0) and nothing else; the -1 of (1,0) is no entry
CAND_2X2 = np.array([[1, 2, 3], [2, 3, 4], [1, -1, 9], [7, 8, 9]], np.int64)


def test_similarity_reference_on_hand_worked_grids():
    got = M.osm(CAND_2X2, (2, 2), 4)
    assert got.dtype == np.float32 and got.tolist() == [[1.5, 1.0], [1.0, 0.5]]
    assert np.array_equal(M.osm(CAND_2X2, (2, 2), 4, normalize=True),
                          np.array([[1.5, 1.0], [1.0, 0.5]], np.float32) / np.float32(3))
    third = np.float32(1) / np.float32(3)
    two_thirds = np.float32(2) / np.float32(3)
    assert np.array_equal(M.osm(CAND_2X2, (2, 2), 8),
                          np.array([[1.0, two_thirds], [two_thirds, third]], np.float32))
    # 1 x 3: a duplicated entry counts once per copy; a row of -1 shares nothing
    row = np.array([[5, 5], [5, 6], [-1, -1]], np.int64)
    for conn in (4, 8):
        assert M.osm(row, (1, 3), conn).tolist() == [[2.0, 0.5, 0.0]]
    assert M.osm(row[:1], (1, 1), 8).tolist() == [[0.0]]   # no neighbour


def test_misorientation_reference_on_hand_worked_grids():
    # rotations about z by 0, 2, 4 and 93 degrees: 93 is 3 under the cubic group's 90 degrees
    e = np.array([[0, 0, 0], [2, 0, 0], [0, 0, 4], [93, 0, 0]], np.float64)
    assert M.disorientation(e[0], e[3]) == pytest.approx(3.0, abs=1e-9)
    for got, want in [(M.kam(e, (2, 2), 4, 5.0), [[3.0, 1.5], [2.5, 1.0]]),
                      (M.kam(e, (2, 2), 4, 2.5), [[2.0, 1.5], [1.0, 1.0]]),
                      (M.kam(e, (2, 2), 8, np.inf), [[3.0, 5 / 3], [7 / 3, 5 / 3]]),
                      (M.kam(e, (2, 2), 8, 0.5), [[0.0, 0.0], [0.0, 0.0]])]:
        assert np.allclose(got, want, rtol=0, atol=1e-9), (got, want)
    # 1 x 3 with a non-finite middle: NaN there, skipped by its neighbours, which keep nothing
    row = np.array([[0, 0, 0], [np.nan, 0, 0], [0, 0, 1]], np.float64)
    got = M.kam(row, (1, 3), 4, 5.0)
    assert got[0, 0] == 0.0 and np.isnan(got[0, 1]) and got[0, 2] == 0.0


def test_scan_maps_record():
    m = ScanMaps((6, 7))
    assert m.scan_shape == (6, 7) and m.ipf == ("z",) and m.connectivity == 4
    assert not (m.similarity or m.similarity_normalize or m.kam or m.mask_failed)
    assert m.kam_max_angle == 5.0
    m.check(42)
    with pytest.raises(ValueError, match="42"):
        m.check(41)
    with pytest.raises(Exception):
        m.kam = True                                     # frozen
    full = ScanMaps([2, 3], ipf="xy", similarity=1, kam=True, kam_max_angle=None, connectivity=8)
    assert full.ipf == ("x", "y") and full.similarity is True and full.kam_max_angle == np.inf
    assert ScanMaps((1, 1), ipf=()).ipf == ()
    assert ScanMaps((1, 1), ipf="z").ipf == ("z",)
    for bad in [dict(scan_shape=(0, 4)), dict(scan_shape=(3,)), dict(scan_shape=5),
                dict(scan_shape=(1 << 16, 1 << 15)), dict(scan_shape=(2, 2), ipf=("w",)),
                dict(scan_shape=(2, 2), ipf=("z", "z")), dict(scan_shape=(2, 2), connectivity=6),
                dict(scan_shape=(2, 2), kam_max_angle=-1.0),
                dict(scan_shape=(2, 2), kam_max_angle=float("nan"))]:
        with pytest.raises(ValueError):
            ScanMaps(**bad)


def test_arguments_are_checked_before_any_launch(monkeypatch):
    def no_call(*a, **k):
        raise AssertionError("a refused argument reached the library")
    monkeypatch.setattr(L.N, "call", no_call)
    monkeypatch.setattr(L, "_upload", no_call)
    e, c = np.zeros((6, 3)), np.zeros((6, 4), np.int64)
    with pytest.raises(ValueError, match="direction"):
        ipf_colors(e, "w")
    for bad in (np.zeros((6, 2)), np.zeros(()), np.zeros((6, 3), bool), np.zeros((6, 3), complex),
                torch.zeros(6, 3, dtype=torch.float32), torch.zeros(6, 3, dtype=torch.float64)):
        with pytest.raises(ValueError):                  # shape, dtype, a tensor off the device
            ipf_colors(bad)
    for kw in [dict(candidate_indices=c, scan_shape=(2, 4)), dict(candidate_indices=c, scan_shape=(0, 6)),
               dict(candidate_indices=c, scan_shape=(2, 3), connectivity=5),
               dict(candidate_indices=c.astype(np.float64), scan_shape=(2, 3)),
               dict(candidate_indices=np.zeros((6, 65), np.int64), scan_shape=(2, 3)),
               dict(candidate_indices=np.zeros((6, 0), np.int64), scan_shape=(2, 3)),
               dict(candidate_indices=np.zeros(6, np.int64), scan_shape=(2, 3)),
               dict(candidate_indices=torch.zeros(6, 4, dtype=torch.int32), scan_shape=(2, 3)),
               dict(candidate_indices=torch.zeros(6, 4, dtype=torch.int64), scan_shape=(2, 3))]:
        with pytest.raises(ValueError):
            orientation_similarity_map(**kw)
    for kw in [dict(orientations=e, scan_shape=(2, 4)), dict(orientations=e, scan_shape=(2, 3), connectivity=0),
               dict(orientations=e, scan_shape=(2, 3), max_angle=-0.1),
               dict(orientations=e, scan_shape=(2, 3), max_angle=float("nan")),
               dict(orientations=e.reshape(3, 2, 3), scan_shape=(2, 3)),
               dict(orientations=np.zeros((6, 4)), scan_shape=(2, 3)),
               dict(orientations=torch.zeros(6, 3, dtype=torch.float64), scan_shape=(2, 3))]:
        with pytest.raises(ValueError):
            kernel_average_misorientation(**kw)


def test_scan_index_result_defaults():
    r = ScanIndexResult(orientations=np.zeros((2, 3)), success=np.zeros(2, bool),
                        scores=np.zeros(2, np.float32), top_index=np.zeros(2, np.int64),
                        n_similar=np.zeros(2, np.int32))
    assert r.ipf_colors is None and r.orientation_similarity is None and r.kam is None
    assert r.candidate_indices is None and len(r) == 2
