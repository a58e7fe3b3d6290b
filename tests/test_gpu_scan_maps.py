"""The scan maps on the device (csrc/scan_maps.hip, latice/index/maps.py) against the float64
reference tests/maps_ref.py and the reference's recorded IPF colours, their refusals, and
`index_scan(maps=...)` against the direct functions on the same call's result rows."""
import functools
import os

import numpy as np
import pytest
import torch

import maps_ref as M
from conftest import GOLDEN
from latice import _native as N
from latice.data_module import NLPAR, ingest_patterns_u8
from latice.index import (ScanMaps, ipf_colors, kernel_average_misorientation,
                          orientation_similarity_map)
from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig
from latice.model import VariationalAutoEncoderRawData
from latice.seeding import seeded_state_dict
from test_scan_maps_host import CAND_2X2, ipf_gate

pytestmark = pytest.mark.gpu

GRIDS = [(1, 1), (1, 5), (5, 1), (3, 4), (7, 9)]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- IPF colours
@functools.lru_cache(maxsize=None)
def _random_euler(n):
    rng = np.random.default_rng(100 + n)
    return np.stack([rng.uniform(-180, 180, n), rng.uniform(0, 180, n), rng.uniform(-180, 180, n)], 1)


@pytest.mark.parametrize("direction", ["x", "y", "z"])
def test_ipf_matches_the_recorded_reference_colours(cuda, direction):
    g = np.load(os.path.join(GOLDEN, "ipf_colors.npz"))
    got = ipf_colors(g["euler"], direction)
    ipf_gate(got, g["ipf_" + direction])
    on_device = ipf_colors(torch.from_numpy(g["euler"]).to(cuda), direction)
    assert torch.is_tensor(on_device) and on_device.is_cuda
    assert _same_bits(on_device.cpu().numpy(), got)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_ipf_sizes_against_the_reference(cuda, n):
    e = _random_euler(n)
    for direction in "xyz":
        ipf_gate(ipf_colors(e, direction), M.ipf(e, direction))
    grid = ipf_colors(e.reshape(1, n, 3))              # leading dimensions are kept
    assert grid.shape == (1, n, 3) and _same_bits(grid.reshape(n, 3), ipf_colors(e))


def test_ipf_nan_rows_and_the_empty_call(cuda):
    e = _random_euler(65).copy()
    e[0, 0], e[7, 1], e[64, 2] = np.nan, np.inf, -np.inf
    got = ipf_colors(e, "y")
    assert (got[[0, 7, 64]] == 0).all()
    keep = np.ones(65, bool)
    keep[[0, 7, 64]] = False
    assert _same_bits(got[keep], ipf_colors(e[keep], "y"))   # a row's colour is its own
    assert (got[keep].max(axis=1) == 255).all()
    none = ipf_colors(np.zeros((0, 3)))
    assert none.shape == (0, 3) and none.dtype == np.uint8
    # n = 0 succeeds in the library too, whatever the pointers hold
    buf = torch.full((3,), 9, dtype=torch.uint8, device=cuda)
    N.call("ebsdvae_ipf_colors", buf.data_ptr(), 0, 2, buf.data_ptr(), N.stream(cuda))
    assert (buf.cpu().numpy() == 9).all()


# ---------------------------------------------------------------- orientation similarity
@functools.lru_cache(maxsize=None)
def _candidates(rows, cols, k):
    """Top-k rows such that neighbours share 0..k entries: every point draws its list from a pool
    that it shares with a varying number of its neighbours, some entries replaced by -1."""
    rng = np.random.default_rng(rows * 1000 + cols * 10 + k)
    n = rows * cols
    base = rng.permutation(4 * k + 8)[:k]                          # one list every point starts from
    cand = np.tile(base, (n, 1)).astype(np.int64)
    for p in range(n):
        m = int(rng.integers(0, k + 1))                            # entries of its own: 0 .. k
        cand[p, rng.permutation(k)[:m]] = 1000 + p * k + np.arange(m)
        if p % 3 == 1:
            cand[p, rng.integers(0, k)] = -1
        cand[p] = rng.permutation(cand[p])
    if n > 2:
        cand[2] = -1                                               # a point without any candidate
    return cand


@pytest.mark.parametrize("k", [1, 20, 64])
@pytest.mark.parametrize("rows,cols", GRIDS)
def test_similarity_is_the_reference_bit_for_bit(cuda, rows, cols, k):
    cand = _candidates(rows, cols, k)
    shared = set()
    for conn in (4, 8):
        for normalize in (False, True):
            want = M.osm(cand, (rows, cols), conn, normalize)
            got = orientation_similarity_map(cand, (rows, cols), conn, normalize)
            assert _same_bits(got, want), (conn, normalize, got, want)
            if not normalize:
                shared |= set(np.unique(want).tolist())
    if rows * cols > 1 and k > 1:
        assert len(shared) > 1                                     # the case is not degenerate
    dev = orientation_similarity_map(torch.from_numpy(cand).to(cuda), (rows, cols), 8, True)
    assert dev.is_cuda and _same_bits(dev.cpu().numpy(), M.osm(cand, (rows, cols), 8, True))


def test_similarity_hand_worked(cuda):
    assert orientation_similarity_map(CAND_2X2, (2, 2)).tolist() == [[1.5, 1.0], [1.0, 0.5]]
    full = np.tile(np.arange(64, dtype=np.int64), (12, 1))         # everything shared, k = 64
    assert (orientation_similarity_map(full, (3, 4), 8) == 64.0).all()
    assert (orientation_similarity_map(full, (3, 4), 8, normalize=True) == 1.0).all()


# ---------------------------------------------------------------- kernel average misorientation
@functools.lru_cache(maxsize=None)
def _grains(rows, cols):
    """A grid of a few grains: a base orientation plus at most 1 degree of noise per point, and
    inside each grain some points replaced by a cubic equivalent S q of their orientation."""
    from scipy.spatial.transform import Rotation as R
    rng = np.random.default_rng(rows * 100 + cols)
    bases = [R.random(random_state=int(rng.integers(1 << 30))) for _ in range(3)]
    e = np.empty((rows, cols, 3))
    for i in range(rows):
        for j in range(cols):
            grain = (i * 2 // max(rows, 2)) + (j * 2 // max(cols, 2))    # 0, 1 or 2
            axis = rng.standard_normal(3)
            noise = R.from_rotvec(np.radians(rng.uniform(0, 1.0)) * axis / np.linalg.norm(axis))
            rot = noise * bases[grain]
            if (i + 2 * j) % 3 == 1:
                rot = M.SYM[int(rng.integers(1, 24))] * rot
            e[i, j] = rot.as_euler("zxz", degrees=True)
    return e.reshape(-1, 3)


@pytest.mark.parametrize("rows,cols", GRIDS)
def test_misorientation_matches_the_reference(cuda, rows, cols):
    e = _grains(rows, cols)
    for conn in (4, 8):
        angles = M.neighbour_angles(e, (rows, cols), conn)
        flat = np.array([w for v in angles.values() for w in v])
        for max_angle in (5.0, np.inf):
            # no neighbour angle sits on the threshold, where an ulp decides
            assert not (np.abs(flat - max_angle) < 1e-6).any()
            want = M.kam(e, (rows, cols), conn, max_angle)
            got = kernel_average_misorientation(e, (rows, cols), conn, max_angle)
            assert got.dtype == np.float32 and got.shape == (rows, cols)
            err = np.abs(got.astype(np.float64) - want.astype(np.float32))
            print(f"kam {rows}x{cols} conn {conn} max {max_angle}: max err {err.max():.3e}")
            # both sides are float64: the output's float32 rounding dominates
            assert np.allclose(got, want.astype(np.float32), rtol=1e-6, atol=1e-9)
        if rows * cols > 1:
            # the symmetry reduction is in: within a grain the angles stay below 2 degrees although
            # a third of the points are cubic equivalents, and grain boundaries exceed 5 degrees
            assert flat.min() < 2.0
            assert (M.kam(e, (rows, cols), conn, 5.0) <= 2.0 + 1e-9).all()
    if (rows, cols) == (7, 9):
        assert (flat > 5.0).any()
        assert not np.array_equal(M.kam(e, (7, 9), 8, 5.0), M.kam(e, (7, 9), 8, np.inf))
    dev = kernel_average_misorientation(torch.from_numpy(e).to(cuda).view(rows, cols, 3), (rows, cols))
    assert dev.is_cuda and _same_bits(dev.cpu().numpy(),
                                      kernel_average_misorientation(e, (rows, cols)))


def test_misorientation_nan_centre_and_neighbour(cuda):
    e = _grains(3, 4).copy()
    e[5, 1] = np.nan                                               # (1, 1): an inner point
    e[11] = np.inf                                                 # (2, 3): a corner
    for conn in (4, 8):
        want = M.kam(e, (3, 4), conn, np.inf)
        got = kernel_average_misorientation(e, (3, 4), conn, None)
        assert np.isnan(got[1, 1]) and np.isnan(got[2, 3])
        assert np.isnan(got).sum() == 2
        assert np.allclose(got, want.astype(np.float32), rtol=1e-6, atol=1e-9, equal_nan=True)
    # a point whose every neighbour is non-finite keeps none: 0
    lone = np.full((3, 3), np.nan)
    lone[1] = [10.0, 20.0, 30.0]
    assert kernel_average_misorientation(lone, (1, 3)).tolist()[0][1] == 0.0


def test_misorientation_hand_worked(cuda):
    e = np.array([[0, 0, 0], [2, 0, 0], [0, 0, 4], [93, 0, 0]], np.float64)
    assert np.allclose(kernel_average_misorientation(e, (2, 2), 4, 5.0), [[3.0, 1.5], [2.5, 1.0]],
                       rtol=1e-6, atol=1e-9)
    assert np.allclose(kernel_average_misorientation(e, (2, 2), 4, 2.5), [[2.0, 1.5], [1.0, 1.0]],
                       rtol=1e-6, atol=1e-9)


# ---------------------------------------------------------------- refusals
def test_every_refusal_leaves_the_output_untouched(cuda):
    lib = N.load()
    n = 6
    e = torch.from_numpy(_random_euler(n)).to(cuda)
    c = torch.from_numpy(_candidates(2, 3, 4)).to(cuda)
    rgb = torch.full((n, 3), 77, dtype=torch.uint8, device=cuda)
    f = torch.full((n,), -7.0, dtype=torch.float32, device=cuda)
    E, C, RGB, F_ = e.data_ptr(), c.data_ptr(), rgb.data_ptr(), f.data_ptr()
    st = N.stream(cuda)
    inf, nan = float("inf"), float("nan")
    refused = [
        ("ebsdvae_ipf_colors", (None, n, 2, RGB, st)),
        ("ebsdvae_ipf_colors", (E, n, 2, None, st)),
        ("ebsdvae_ipf_colors", (E, -1, 2, RGB, st)),
        ("ebsdvae_ipf_colors", (E, n, -1, RGB, st)),
        ("ebsdvae_ipf_colors", (E, n, 3, RGB, st)),
        ("ebsdvae_orientation_similarity", (None, 4, 2, 3, 4, 0, F_, st)),
        ("ebsdvae_orientation_similarity", (C, 4, 2, 3, 4, 0, None, st)),
        ("ebsdvae_orientation_similarity", (C, 0, 2, 3, 4, 0, F_, st)),
        ("ebsdvae_orientation_similarity", (C, 65, 2, 3, 4, 0, F_, st)),
        ("ebsdvae_orientation_similarity", (C, 4, 0, 3, 4, 0, F_, st)),
        ("ebsdvae_orientation_similarity", (C, 4, 2, 0, 4, 0, F_, st)),
        ("ebsdvae_orientation_similarity", (C, 4, -2, -3, 4, 0, F_, st)),
        ("ebsdvae_orientation_similarity", (C, 4, 1 << 16, 1 << 15, 4, 0, F_, st)),
        ("ebsdvae_orientation_similarity", (C, 4, 2, 3, 6, 0, F_, st)),
        ("ebsdvae_orientation_similarity", (C, 4, 2, 3, 0, 0, F_, st)),
        ("ebsdvae_kernel_misorientation", (None, 2, 3, 4, 5.0, F_, st)),
        ("ebsdvae_kernel_misorientation", (E, 2, 3, 4, 5.0, None, st)),
        ("ebsdvae_kernel_misorientation", (E, 0, 3, 4, 5.0, F_, st)),
        ("ebsdvae_kernel_misorientation", (E, 2, 0, 4, 5.0, F_, st)),
        ("ebsdvae_kernel_misorientation", (E, 1 << 16, 1 << 15, 4, 5.0, F_, st)),
        ("ebsdvae_kernel_misorientation", (E, 2, 3, 5, 5.0, F_, st)),
        ("ebsdvae_kernel_misorientation", (E, 2, 3, 4, nan, F_, st)),
        ("ebsdvae_kernel_misorientation", (E, 2, 3, 4, -1.0, F_, st)),
        ("ebsdvae_kernel_misorientation", (E, 2, 3, 4, -inf, F_, st)),
    ]
    for name, args in refused:
        assert getattr(lib, name)(*args) != 0, (name, args)
        assert lib.ebsdvae_last_error(), name
        with pytest.raises(RuntimeError, match=name):
            N.call(name, *args)
    torch.cuda.synchronize()
    assert (rgb.cpu().numpy() == 77).all() and (f.cpu().numpy() == -7.0).all()
    # and the accepted forms of the same calls write every element
    N.call("ebsdvae_ipf_colors", E, n, 2, RGB, st)
    assert (rgb.cpu().numpy().max(axis=1) == 255).all()
    N.call("ebsdvae_kernel_misorientation", E, 2, 3, 4, inf, F_, st)
    assert (f.cpu().numpy() > 0).all()
    N.call("ebsdvae_orientation_similarity", C, 4, 2, 3, 4, 0, F_, st)
    assert (f.cpu().numpy() >= 0).all()


# ---------------------------------------------------------------- index_scan(maps=...)
ROWS, COLS = 6, 7
N_SCAN = ROWS * COLS
KW = dict(top_n=10, orientation_threshold=2.0, min_required_matches=8)


@pytest.fixture(scope="module")
def scan(cuda, tmp_path_factory):
    """The small model and dictionary of tests/test_gpu_scan_index.py on a 6 x 7 grid: 42
    patterns = 3 random base patterns x 14 near copies.  The angles of the first two groups
    scatter by 0.3 degrees around a centre, one copy per group behind a cubic symmetry operator;
    those of the third are unrelated, so its patterns (scan rows 4 and 5) find no consensus.  The
    dictionary is built from the same patterns."""
    from scipy.spatial.transform import Rotation as R
    tmp = tmp_path_factory.mktemp("scan_maps")
    rng = np.random.default_rng(22)
    raw, ang = [], []
    for c in range(3):
        base = rng.random((140, 140))
        centre = R.random(random_state=int(rng.integers(1 << 30)))
        for j in range(14):
            raw.append(np.clip(base + 1e-3 * rng.standard_normal((140, 140)), 0.0, 1.0))
            rot = R.from_rotvec(np.radians(0.3) * rng.standard_normal(3)) * centre
            if j == 5:
                rot = M.SYM[7 + c] * rot
            if c == 2:
                rot = R.random(random_state=int(rng.integers(1 << 30)))
            ang.append(rot.as_euler("zxz", degrees=True))
    raw, ang = np.array(raw), np.array(ang)
    np.save(tmp / "patterns.npy", raw)
    with open(tmp / "angles.txt", "w") as f:
        f.write(f"eu\n{N_SCAN}\n")
        for a in ang:
            f.write(" ".join(repr(float(v)) for v in a) + "\n")
    m = VariationalAutoEncoderRawData()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0).items()})
    cfg = IndexerConfig(pattern_path=tmp / "patterns.npy", angles_path=tmp / "angles.txt",
                        batch_size=16, device="cuda")
    ix = DiffractionPatternIndexer(m.to(cuda), config=cfg)
    ix.build_dictionary()
    return dict(ix=ix, raw_u8=np.round(raw * 255).astype(np.uint8))


ALL_MAPS = ScanMaps((ROWS, COLS), ipf=("x", "y", "z"), similarity=True, similarity_normalize=True,
                    kam=True, kam_max_angle=3.0, connectivity=8)
INDEX_FIELDS = ("orientations", "success", "scores", "top_index", "n_similar", "candidate_indices",
                "candidate_scores")


def _check_maps(r, maps):
    """Every map of the result equals the direct function on the same call's rows, bit for bit."""
    for d in maps.ipf:
        want = ipf_colors(r.orientations, d).reshape(ROWS, COLS, 3)
        if maps.mask_failed:
            want = want * r.success.reshape(ROWS, COLS, 1).astype(np.uint8)
        assert _same_bits(r.ipf_colors[d], want), d
    assert set(r.ipf_colors) == set(maps.ipf)
    if maps.similarity and r.candidate_indices is not None:
        assert _same_bits(r.orientation_similarity, orientation_similarity_map(
            r.candidate_indices, maps.scan_shape, maps.connectivity, maps.similarity_normalize))
    if maps.kam:
        assert _same_bits(r.kam, kernel_average_misorientation(
            r.orientations, maps.scan_shape, maps.connectivity, maps.kam_max_angle))


@pytest.mark.parametrize("form", ["host", "tensor"])
def test_index_scan_maps_equal_the_direct_functions(scan, form):
    ix, raw = scan["ix"], scan["raw_u8"]
    patterns = raw if form == "host" else ingest_patterns_u8(raw, (128, 128))
    plain = ix.index_scan(patterns, batch_size=5, return_candidates=True, **KW)
    assert plain.ipf_colors is None and plain.orientation_similarity is None and plain.kam is None
    assert plain.success.any() and not plain.success.all()
    results = []
    for batch in (5, 64):
        r = ix.index_scan(patterns, batch_size=batch, return_candidates=True, maps=ALL_MAPS, **KW)
        assert r.orientation_similarity.shape == (ROWS, COLS) and r.kam.dtype == np.float32
        assert r.ipf_colors["z"].shape == (ROWS, COLS, 3) and r.ipf_colors["z"].dtype == np.uint8
        _check_maps(r, ALL_MAPS)
        for name in INDEX_FIELDS:          # with maps=None the existing fields are the same bits
            assert _same_bits(getattr(r, name), getattr(plain, name)), (name, batch)
        results.append(r)
    a, b = results                         # and the maps do not depend on the batch size
    assert _same_bits(a.kam, b.kam) and _same_bits(a.orientation_similarity, b.orientation_similarity)
    assert all(_same_bits(a.ipf_colors[d], b.ipf_colors[d]) for d in "xyz")
    assert a.orientation_similarity.max() > 0 and (a.kam > 0).any()


def test_index_scan_masks_failed_rows_and_keeps_candidates_on_the_device(scan):
    ix, raw = scan["ix"], scan["raw_u8"]
    maps = ScanMaps((ROWS, COLS), similarity=True, mask_failed=True)
    with_rows = ix.index_scan(raw, batch_size=16, return_candidates=True, maps=maps, **KW)
    failed = ~with_rows.success.reshape(ROWS, COLS)
    assert failed.any() and not failed.all()
    _check_maps(with_rows, maps)
    unmasked = ipf_colors(with_rows.orientations).reshape(ROWS, COLS, 3)
    masked = with_rows.ipf_colors["z"]
    assert (masked[failed] == 0).all() and (unmasked[failed].max(axis=1) == 255).all()
    assert _same_bits(masked[~failed], unmasked[~failed])      # exactly the failed rows
    assert with_rows.kam is None
    # the similarity map without the candidate lists: the same map, no lists
    lean = ix.index_scan(raw, batch_size=16, maps=maps, **KW)
    assert lean.candidate_indices is None and lean.candidate_scores is None
    assert _same_bits(lean.orientation_similarity, with_rows.orientation_similarity)
    assert _same_bits(lean.ipf_colors["z"], masked)
    for name in INDEX_FIELDS[:5]:
        assert _same_bits(getattr(lean, name), getattr(with_rows, name)), name


def test_index_scan_refuses_a_wrong_grid_before_any_launch(scan, monkeypatch):
    ix, raw = scan["ix"], scan["raw_u8"]

    def no_call(name, *a):
        raise AssertionError(f"{name} was called for a refused scan")
    monkeypatch.setattr(N, "call", no_call)
    with pytest.raises(ValueError, match="42 patterns"):
        ix.index_scan(raw, maps=ScanMaps((6, 6)), **KW)
    with pytest.raises(ValueError, match="42 patterns"):
        ix.index_scan(torch.zeros(N_SCAN, 1, 128, 128, device="cuda"), maps=ScanMaps((7, 7)), **KW)
    with pytest.raises(ValueError, match="differs"):
        ix.index_scan(raw, nlpar=NLPAR((ROWS, COLS)), maps=ScanMaps((COLS, ROWS)), **KW)
    with pytest.raises(TypeError, match="ScanMaps"):
        ix.index_scan(raw, maps=(ROWS, COLS), **KW)
