"""The grain reference tests/grains_ref.py on hand-worked cases, the inputs of the GPU cases
against their caps, `ScanMaps`' grain fields, `GrainMap.table()` and the result buffer's layout
with grains.  No GPU."""
import numpy as np
import pytest
import torch

import grains_ref as G
from latice.index import GrainMap, ScanMaps, segment_grains
from latice.index.dp_indexer import _result_buffer

HAND_2X2 = np.array([[0, 0, 0], [2, 0, 0], [0, 0, 4], [93, 0, 0]], np.float64)


def test_reference_on_a_hand_worked_2x2():
    # angles about z: 0, 2 | 4, 93 (= 3 under the cubic group).  The forward edges are 2 (right of
    # the first), 4 (below it), 1 and 1 degrees: threshold 1.5 joins the last three points
    e = HAND_2X2
    r = G.segment(e, (2, 2), 1.5, 4)
    assert r.grain_id.tolist() == [[0, 1], [1, 1]] and r.n_grains == 2
    assert r.boundary.tolist() == [[1, 1], [1, 0]]
    # grain 1 = 2, 4 and 3 degrees (93 projected onto the root): the mean is 3 about z
    assert np.allclose(G.rotation_angle_deg(r.grain_orientation[1, 1], [3, 0, 0]), 0, atol=1e-9)
    assert np.allclose(G.rotation_angle_deg(r.grain_orientation[0, 0], [0, 0, 0]), 0, atol=1e-9)
    assert np.allclose(r.grod, [[0, 1], [1, 0]], atol=1e-9)
    assert np.allclose(r.gos, [[0, 2 / 3], [2 / 3, 2 / 3]], atol=1e-9)
    assert abs(r.edge_margin - 0.5) < 1e-9
    assert G.segment(e, (2, 2), 1.5, 8).n_grains == 2      # the diagonals are 3 and 2 degrees
    assert G.segment(e, (2, 2), 2.5, 4).n_grains == 1
    assert G.segment(e, (2, 2), 0.5, 8).grain_id.tolist() == [[0, 1], [2, 3]]


def test_reference_joins_the_arms_of_a_u_in_the_last_row():
    ref = G.reference("u")
    lab = G.u_shape()
    assert ref.n_grains == 2
    assert (ref.grain_id[lab == 0] == 0).all() and (ref.grain_id[lab == 1] == 1).all()
    # without the last row the arms are two grains
    e, shape, conn, _, _ = G.case("u")
    cut = G.segment(e[:-12], (11, 12), G.THRESHOLD, conn)
    assert cut.n_grains == 3 and cut.grain_id[0, 0] != cut.grain_id[0, 11]


def test_reference_on_a_checkerboard():
    four, eight = G.reference("checker4"), G.reference("checker8")
    assert four.n_grains == 64 and four.grain_id.reshape(-1).tolist() == list(range(64))
    assert (four.boundary == 1).all() and np.nanmax(four.grod) < 1e-9
    assert eight.n_grains == 2 and (eight.grain_id == G.checkerboard()).all()
    assert (eight.boundary == 1).all()


def test_reference_masks_unusable_points():
    ref = G.reference("1x3_lone")
    assert ref.grain_id.tolist() == [[-1, 0, -1]] and ref.boundary.tolist() == [[0, 1, 0]]
    bad = G.reference("3x4_bad")
    assert [bad.grain_id.reshape(-1)[p] for p in (2, 5, 11)] == [-1, -1, -1]
    assert np.isnan(bad.grod.reshape(-1)[[2, 5, 11]]).all() and np.isnan(bad.gos).sum() == 3
    assert bad.boundary.reshape(-1)[[1, 3, 6]].tolist() == [1, 1, 1]      # against -1


@pytest.mark.parametrize("name", G.CASES)
def test_every_case_stays_inside_its_caps(name):
    ref = G.check_preconditions(name)
    if name == "chain":
        assert np.nanmax(ref.grod) > 9.0           # one grain although its ends are 20 degrees apart
    if name == "voronoi":
        assert ref.grain_id.size > 2 * G.SCAN_BLOCK and ref.n_grains > 100
    if name in ("1x65_two", "2x129_two"):
        ids = ref.grain_id.reshape(-1)                # the split lies inside a wave of 64 points
        assert int(np.flatnonzero(ids == 1)[0]) % 64 not in (0, 63) and ids[0] == 0


def test_scan_maps_validates_the_grain_fields():
    m = ScanMaps((3, 4))
    assert (m.grains, m.grain_threshold, m.grain_mask_failed) == (False, 5.0, False)
    m = ScanMaps((3, 4), grains=1, grain_threshold=2, grain_mask_failed=1)
    assert m.grains is True and m.grain_threshold == 2.0 and m.grain_mask_failed is True
    for bad in (-1.0, float("nan"), float("inf"), None, "wide"):
        with pytest.raises(ValueError, match="grain threshold"):
            ScanMaps((3, 4), grains=True, grain_threshold=bad)


def test_segment_grains_checks_before_the_device():
    e = np.zeros((12, 3))
    for kw in (dict(scan_shape=(3, 5)), dict(scan_shape=(3, 4), connectivity=6),
               dict(scan_shape=(3, 4), threshold=-1.0), dict(scan_shape=(3, 4), threshold=np.inf),
               dict(scan_shape=(3, 4), valid=np.ones(11)), dict(scan_shape=(0, 4)),
               dict(scan_shape=(3, 4), valid=torch.ones(12, dtype=torch.int32))):
        with pytest.raises(ValueError):
            segment_grains(e, **kw)
    with pytest.raises(ValueError, match="float64"):
        segment_grains(torch.zeros(12, 3), (3, 4))


def test_grain_table_on_hand_made_arrays():
    ids = np.array([[0, 0, 1], [-1, 1, 2]], np.int32)
    mean = np.arange(18, dtype=np.float64).reshape(2, 3, 3)
    gos = np.array([[.5, .5, 1.5], [np.nan, 1.5, 2.5]], np.float32)
    gm = GrainMap(grain_id=ids, grain_orientation=mean, gos=gos)
    t = gm.table()
    assert gm.n_grains == 3 and len(t) == 3
    assert t.sizes.dtype == np.int64 and t.sizes.tolist() == [2, 2, 1]
    assert t.first_point.tolist() == [0, 2, 5]
    assert t.mean_orientation.tolist() == [[0, 1, 2], [6, 7, 8], [15, 16, 17]]
    assert t.gos.tolist() == [0.5, 1.5, 2.5]
    lean = GrainMap(grain_id=torch.from_numpy(ids)).table()
    assert lean.sizes.tolist() == [2, 2, 1] and lean.mean_orientation is None and lean.gos is None
    none = GrainMap(grain_id=np.full((2, 2), -1, np.int32))
    assert none.n_grains == 0 and len(none.table()) == 0


@pytest.mark.parametrize("candidates", [False, True])
@pytest.mark.parametrize("n", [1, 7, 41])
def test_result_buffer_views_are_aligned_and_unchanged_without_grains(n, candidates):
    k = 3
    every = ScanMaps((1, n), ipf=("x", "z"), similarity=True, kam=True, grains=True)
    buf, layout, res, views = _result_buffer(n, k, candidates, "cpu", every)
    assert {"grain_id", "grain_orientation", "gos", "grod", "grain_boundary"} <= set(views)
    end = 0
    for name, dt, shape, offset, nbytes in layout:
        assert offset == end and offset % torch.empty((), dtype=dt).element_size() == 0, name
        end += nbytes
    assert views["grain_orientation"].dtype == torch.float64 and views["grain_id"].dtype == torch.int32
    assert views["grain_boundary"].shape == (n,) and views["grain_orientation"].shape == (n, 3)
    # without grains: the layout of the same maps is what it was, field by field
    off = ScanMaps((1, n), ipf=("x", "z"), similarity=True, kam=True)
    _, plain, _, plain_views = _result_buffer(n, k, candidates, "cpu", off)
    names = [f[0] for f in plain]
    want = ["best", "row"] + (["cand_idx"] if candidates else []) + ["score", "success", "n_similar"] \
        + (["cand_scores"] if candidates else []) + ["osm", "kam", "ipf_x", "ipf_z"]
    assert names == want and set(plain_views) == {"osm", "kam", "ipf_x", "ipf_z"}
    sizes = {"best": 24 * n, "row": 8 * n, "cand_idx": 8 * n * k, "score": 4 * n, "success": 4 * n,
             "n_similar": 4 * n, "cand_scores": 4 * n * k, "osm": 4 * n, "kam": 4 * n,
             "ipf_x": 3 * n, "ipf_z": 3 * n}
    end = 0
    for name, _, _, offset, nbytes in plain:
        assert (offset, nbytes) == (end, sizes[name]), name
        end += nbytes
    assert [f[0] for f in _result_buffer(n, k, candidates, "cpu", None)[1]] == want[:-4]
