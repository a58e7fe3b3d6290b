"""The grain segmentation on the device (csrc/grains.hip, latice/index/grains.py) against the
float64 reference tests/grains_ref.py, its reproducibility, its refusals, and
`index_scan(maps=ScanMaps(grains=True))` against `segment_grains` on the same call's rows."""
import numpy as np
import pytest
import torch

import grains_ref as G
import maps_ref as M
from latice import _native as N
from latice.data_module import ingest_patterns_u8
from latice.index import ScanMaps, segment_grains
from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig
from latice.index.grains import grain_rows
from latice.model import VariationalAutoEncoderRawData
from latice.seeding import seeded_state_dict

pytestmark = pytest.mark.gpu

SCAN_BLOCK = 4096       # points per block of the device's prefix sum (csrc/grains.hip kScanBlock)
FIELDS = ("grain_id", "grain_orientation", "gos", "grod", "boundary")


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_map(a, b, fields=FIELDS):
    return all(_same_bits(getattr(a, f), getattr(b, f)) for f in fields)


@pytest.mark.parametrize("name", G.CASES)
def test_grains_match_the_reference(cuda, name):
    """grain_id and boundary equal the reference; the grain mean lies within 1e-6 degrees of it as
    a rotation (fixed point 2^-31 rounds a component by <= 2^-32, about 5e-8 degrees); grod and gos
    within 1e-6 degrees absolute plus rtol 1e-6 of the reference rounded to float32."""
    ref = G.check_preconditions(name)
    e, shape, conn, valid, _ = G.case(name)
    if name == "voronoi":
        assert e.shape[0] > 2 * SCAN_BLOCK and G.SCAN_BLOCK == SCAN_BLOCK
    got = segment_grains(e, shape, G.THRESHOLD, conn, valid=valid)
    assert got.grain_id.dtype == np.int32 and got.boundary.dtype == np.uint8
    assert got.grod.dtype == np.float32 and got.gos.dtype == np.float32
    assert got.grain_orientation.dtype == np.float64 and got.grain_orientation.shape == shape + (3,)
    assert np.array_equal(got.grain_id, ref.grain_id), name
    assert np.array_equal(got.boundary, ref.boundary), name
    assert got.n_grains == ref.n_grains
    ok = ref.grain_id >= 0
    assert np.isnan(got.grod[~ok]).all() and np.isnan(got.gos[~ok]).all()
    assert np.isnan(got.grain_orientation[~ok]).all()
    mean_err = G.rotation_angle_deg(got.grain_orientation[ok], ref.grain_orientation[ok]).max()
    grod_err = np.abs(got.grod[ok].astype(np.float64) - ref.grod[ok].astype(np.float32)).max()
    gos_err = np.abs(got.gos[ok].astype(np.float64) - ref.gos[ok].astype(np.float32)).max()
    print(f"grains {name}: G {got.n_grains} mean err {mean_err:.3e} deg, grod err {grod_err:.3e}, "
          f"gos err {gos_err:.3e}")
    assert mean_err <= 1e-6
    assert np.allclose(got.grod[ok], ref.grod[ok].astype(np.float32), rtol=1e-6, atol=1e-6)
    assert np.allclose(got.gos[ok], ref.gos[ok].astype(np.float32), rtol=1e-6, atol=1e-6)
    # the per-grain table agrees with the map
    t = got.table()
    assert len(t) == ref.n_grains and t.sizes.sum() == ok.sum()
    assert np.array_equal(got.grain_id.reshape(-1)[t.first_point], np.arange(len(t)))


def test_hand_worked_2x2(cuda):
    e = np.array([[0, 0, 0], [2, 0, 0], [0, 0, 4], [93, 0, 0]], np.float64)
    got = segment_grains(e, (2, 2), threshold=1.5)
    assert got.grain_id.tolist() == [[0, 1], [1, 1]] and got.boundary.tolist() == [[1, 1], [1, 0]]
    assert np.allclose(got.grod, [[0, 1], [1, 0]], atol=1e-6)
    assert np.allclose(got.gos, [[0, 2 / 3], [2 / 3, 2 / 3]], atol=1e-6)
    assert segment_grains(e, (2, 2), threshold=2.5).n_grains == 1
    assert segment_grains(e, (2, 2), threshold=0.5, connectivity=8).grain_id.tolist() == [[0, 1], [2, 3]]


@pytest.mark.parametrize("name", ["7x9_bad", "2x129_two", "spirals", "voronoi"])
def test_grains_are_the_same_bits_on_every_run(cuda, name):
    e, shape, conn, valid, _ = G.case(name)
    first = segment_grains(e, shape, G.THRESHOLD, conn, valid=valid)
    assert _same_map(first, segment_grains(e, shape, G.THRESHOLD, conn, valid=valid))
    # the device-tensor form: device tensors, the same bits
    et = torch.from_numpy(e).to(cuda)
    vt = None if valid is None else torch.from_numpy(valid).to(cuda)
    dev = segment_grains(et.view(shape + (3,)), shape, G.THRESHOLD, conn, valid=vt)
    for f in FIELDS:
        assert torch.is_tensor(getattr(dev, f)) and getattr(dev, f).is_cuda
        assert _same_bits(getattr(dev, f).cpu().numpy(), getattr(first, f)), f
    assert dev.n_grains == first.n_grains and dev.table().sizes.tolist() == first.table().sizes.tolist()
    # a scratch full of 0xFF bytes changes nothing
    n = e.shape[0]
    out = dict(grain_id=torch.empty(n, dtype=torch.int32, device=cuda),
               grain_euler=torch.empty(n, 3, dtype=torch.float64, device=cuda),
               gos=torch.empty(n, dtype=torch.float32, device=cuda),
               grod=torch.empty(n, dtype=torch.float32, device=cuda),
               boundary=torch.empty(n, dtype=torch.uint8, device=cuda))
    work = torch.full((N.call("ebsdvae_grain_work", *shape),), 0xFF, dtype=torch.uint8, device=cuda)
    grain_rows(et, vt, shape, conn, G.THRESHOLD, work=work, **out)
    for f, key in zip(FIELDS, ("grain_id", "grain_euler", "gos", "grod", "boundary")):
        assert out[key].cpu().numpy().tobytes() == getattr(first, f).tobytes(), f
    # optional outputs off: the ids are the same bits, and gos does not need grod
    lean = segment_grains(e, shape, G.THRESHOLD, conn, valid=valid, mean=False, grod=False,
                          boundary=False)
    assert _same_bits(lean.grain_id, first.grain_id)
    assert lean.grain_orientation is None and lean.gos is None and lean.grod is None and lean.boundary is None
    no_grod = segment_grains(e, shape, G.THRESHOLD, conn, valid=valid, grod=False)
    assert no_grod.grod is None and _same_map(no_grod, first, ("grain_id", "grain_orientation", "gos", "boundary"))
    only_grod = segment_grains(e, shape, G.THRESHOLD, conn, valid=valid, mean=False, boundary=False)
    assert _same_map(only_grod, first, ("grain_id", "grod"))


def test_every_refusal_leaves_the_outputs_untouched(cuda):
    lib = N.load()
    n = 6
    e = torch.from_numpy(G.case("3x4")[0][:n].copy()).to(cuda)
    ids = torch.full((n,), 77, dtype=torch.int32, device=cuda)
    ge = torch.full((n, 3), -7.0, dtype=torch.float64, device=cuda)
    f1 = torch.full((n,), -7.0, dtype=torch.float32, device=cuda)
    f2 = torch.full((n,), -7.0, dtype=torch.float32, device=cuda)
    bd = torch.full((n,), 77, dtype=torch.uint8, device=cuda)
    assert N.call("ebsdvae_grain_work", 2, 3) > 0
    for rows, cols in ((0, 3), (2, 0), (-2, -3), (1 << 16, 1 << 15)):
        assert N.call("ebsdvae_grain_work", rows, cols) == 0
    work = torch.zeros(N.call("ebsdvae_grain_work", 2, 3) + 8, dtype=torch.uint8, device=cuda)
    E, I_, GE, F1, F2, B, W = (t.data_ptr() for t in (e, ids, ge, f1, f2, bd, work))
    st = N.stream(cuda)
    inf, nan = float("inf"), float("nan")
    name = "ebsdvae_segment_grains"
    refused = [
        (None, None, 2, 3, 4, 5.0, I_, GE, F1, F2, B, W, st),
        (E, None, 2, 3, 4, 5.0, None, GE, F1, F2, B, W, st),
        (E, None, 2, 3, 4, 5.0, I_, GE, F1, F2, B, None, st),
        (E, None, 2, 3, 4, 5.0, I_, GE, F1, F2, B, W + 4, st),
        (E, None, 0, 3, 4, 5.0, I_, GE, F1, F2, B, W, st),
        (E, None, 2, 0, 4, 5.0, I_, GE, F1, F2, B, W, st),
        (E, None, -2, -3, 4, 5.0, I_, GE, F1, F2, B, W, st),
        (E, None, 1 << 16, 1 << 15, 4, 5.0, I_, GE, F1, F2, B, W, st),
        (E, None, 2, 3, 6, 5.0, I_, GE, F1, F2, B, W, st),
        (E, None, 2, 3, 0, 5.0, I_, GE, F1, F2, B, W, st),
        (E, None, 2, 3, 4, nan, I_, GE, F1, F2, B, W, st),
        (E, None, 2, 3, 4, -1.0, I_, GE, F1, F2, B, W, st),
        (E, None, 2, 3, 4, inf, I_, GE, F1, F2, B, W, st),
        (E, None, 2, 3, 4, -inf, I_, GE, F1, F2, B, W, st),
    ]
    for args in refused:
        assert getattr(lib, name)(*args) != 0, args
        assert lib.ebsdvae_last_error(), args
        with pytest.raises(RuntimeError, match=name):
            N.call(name, *args)
    torch.cuda.synchronize()
    assert (ids.cpu().numpy() == 77).all() and (bd.cpu().numpy() == 77).all()
    assert (ge.cpu().numpy() == -7.0).all() and (f1.cpu().numpy() == -7.0).all()
    assert (f2.cpu().numpy() == -7.0).all()
    # and the accepted form of the same call writes every element
    N.call(name, E, None, 2, 3, 4, 5.0, I_, GE, F1, F2, B, W, st)
    assert (ids.cpu().numpy() >= 0).all() and (bd.cpu().numpy() <= 1).all()
    assert (f1.cpu().numpy() >= 0).all() and (f2.cpu().numpy() >= 0).all()
    assert (ge.cpu().numpy() != -7.0).all()


# ---------------------------------------------------------------- index_scan(maps=ScanMaps(grains=True))
ROWS, COLS = 6, 7
N_SCAN = ROWS * COLS
KW = dict(top_n=10, orientation_threshold=2.0, min_required_matches=8)
INDEX_FIELDS = ("orientations", "success", "scores", "top_index", "n_similar", "candidate_indices",
                "candidate_scores")


@pytest.fixture(scope="module")
def scan(cuda, tmp_path_factory):
    """The recipe of tests/test_gpu_scan_maps.py: 42 patterns = 3 random base patterns x 14 near
    copies on a 6 x 7 grid.  The angles of the first two groups scatter by 0.3 degrees around a
    centre, one copy per group behind a cubic operator; those of the third are unrelated, so its
    patterns (scan rows 4 and 5) find no consensus.  The dictionary is the same patterns."""
    from scipy.spatial.transform import Rotation as R
    tmp = tmp_path_factory.mktemp("scan_grains")
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


OLD_MAPS = dict(ipf=("x", "z"), similarity=True, kam=True, kam_max_angle=3.0, connectivity=8)


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("form", ["host", "tensor"])
def test_index_scan_grains_equal_segment_grains(scan, form, mask):
    ix, raw = scan["ix"], scan["raw_u8"]
    patterns = raw if form == "host" else ingest_patterns_u8(raw, (128, 128))
    without = ix.index_scan(patterns, batch_size=5, return_candidates=True,
                            maps=ScanMaps((ROWS, COLS), **OLD_MAPS), **KW)
    assert without.grains is None
    maps = ScanMaps((ROWS, COLS), grains=True, grain_threshold=4.0, grain_mask_failed=mask, **OLD_MAPS)
    results = []
    for batch in (5, 64):
        r = ix.index_scan(patterns, batch_size=batch, return_candidates=True, maps=maps, **KW)
        want = segment_grains(r.orientations, (ROWS, COLS), 4.0, 8,
                              valid=r.success if mask else None)
        assert _same_map(r.grains, want), (form, mask, batch)
        assert r.grains.grain_id.shape == (ROWS, COLS) and r.grains.n_grains >= 2
        for name in INDEX_FIELDS:          # the existing fields and maps are the same bits
            assert _same_bits(getattr(r, name), getattr(without, name)), (name, batch)
        assert _same_bits(r.kam, without.kam)
        assert _same_bits(r.orientation_similarity, without.orientation_similarity)
        assert all(_same_bits(r.ipf_colors[d], without.ipf_colors[d]) for d in "xz")
        failed = ~r.success.reshape(ROWS, COLS)
        assert failed.any() and not failed.all()
        if mask:
            assert (r.grains.grain_id[failed] == -1).all() and (r.grains.grain_id[~failed] >= 0).all()
            assert np.isnan(r.grains.grod[failed]).all()
        else:
            assert (r.grains.grain_id >= 0).all()
        results.append(r)
    assert _same_map(results[0].grains, results[1].grains)     # whatever the batch size


def test_index_scan_refuses_a_wrong_grid_before_any_launch(scan, monkeypatch):
    ix, raw = scan["ix"], scan["raw_u8"]

    def no_call(name, *a):
        raise AssertionError(f"{name} was called for a refused scan")
    monkeypatch.setattr(N, "call", no_call)
    with pytest.raises(ValueError, match="42 patterns"):
        ix.index_scan(raw, maps=ScanMaps((6, 6), grains=True), **KW)
    with pytest.raises(ValueError, match="42 patterns"):
        ix.index_scan(torch.zeros(N_SCAN, 1, 128, 128, device="cuda"),
                      maps=ScanMaps((7, 7), grains=True), **KW)
