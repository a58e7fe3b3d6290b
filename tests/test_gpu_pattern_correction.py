"""Background-corrected pattern ingest on the device (csrc/correct.hip through
latice.data_module.correct_patterns), the scan-mean background
(DiffractionPatternIndexer.scan_background) and index_scan(correction=).

Parity gate: max |out - oracle| <= 2e-5 on outputs in [0, 1], the kernel-level gate of
DESIGN.md section 4, against the float64 oracle tests/correction_ref.py.  numpy float32
against that oracle on exactly these inputs gives at most 2.9e-6.  The oracle's conditioning is
asserted before every comparison (correction_ref.assert_well_conditioned), so the gate never
covers a case where the rescale or a divide magnifies rounding."""
import functools

import numpy as np
import pytest
import torch

import correction_ref as R
from latice.data_module import PatternCorrection, correct_patterns
from latice.index import faiss_db as F
from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig
from latice.model import VariationalAutoEncoderRawData
from latice.seeding import seeded_state_dict

pytestmark = pytest.mark.gpu

GATE = 2e-5
MODES = (None, "subtract", "divide")
ALL_PAIRS = [(s, d) for s in MODES for d in MODES]
THREE_PAIRS = [(None, "subtract"), ("divide", "divide"), ("subtract", "divide")]


def _correction(bg, static_mode, sigma, dynamic_mode):
    return PatternCorrection(
        static_background=None if static_mode is None else R.static_background(bg, static_mode),
        static_mode=static_mode or "subtract",
        dynamic_sigma=None if dynamic_mode is None else sigma,
        dynamic_mode=dynamic_mode or "subtract")


@functools.lru_cache(maxsize=None)
def _oracle(B, H0, W0, side, static_mode, sigma, dynamic_mode, dtype="uint8"):
    raw, bg = R.detector_patterns(B, H0, W0, seed=H0 + side)
    if dtype != "uint8":
        raw = raw.astype(dtype)
        t, l = R.crop_offset(H0, side), R.crop_offset(W0, side)
        raw[0, t + 10, l + 12] = np.nan          # both inside the window
        raw[B - 1, t + side - 1, l] = np.inf
        raw.setflags(write=False)
    sbg = None if static_mode is None else R.static_background(bg, static_mode)
    ref = R.correct(raw, (side, side), sbg, static_mode, None if dynamic_mode is None else sigma,
                    dynamic_mode)
    R.assert_well_conditioned(ref, dynamic_mode == "divide")
    return raw, bg, ref["out"]


def _check_parity(B, H0, W0, side, static_mode, sigma, dynamic_mode, dtype="uint8"):
    raw, bg, want = _oracle(B, H0, W0, side, static_mode, sigma, dynamic_mode, dtype)
    got = correct_patterns(raw, (side, side), _correction(bg, static_mode, sigma, dynamic_mode))
    assert got.shape == (B, 1, side, side) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy()
    err = np.abs(got - want).max()
    print(f"{dtype} {H0}x{W0}->{side} static={static_mode} dynamic={dynamic_mode} sigma={sigma}: "
          f"max err {err:.2e}")
    assert np.isfinite(got).all()
    per = got.reshape(B, -1)
    assert (per.min(1) == 0.0).all() and (per.max(1) == 1.0).all()   # in [0, 1], both attained
    assert err <= GATE, err


@pytest.mark.parametrize("sigma", [2.0, 15.9])      # 15.9: radius 64 = the window, maximal reflect
@pytest.mark.parametrize("static_mode,dynamic_mode", ALL_PAIRS)
def test_parity_64_every_mode_pair(cuda, static_mode, dynamic_mode, sigma):
    # 70 -> 64: offset 3; 66 -> 64: offset 1 (the 69 x 67 case below has the half-way ties)
    _check_parity(3, 70, 66, 64, static_mode, sigma, dynamic_mode)


def test_parity_64_half_to_even_offsets(cuda):
    # 69 -> 64: 2.5 -> 2; 67 -> 64: 1.5 -> 2
    _check_parity(3, 69, 67, 64, "divide", 2.0, "subtract")


@pytest.mark.parametrize("static_mode,dynamic_mode", THREE_PAIRS)
def test_parity_128(cuda, static_mode, dynamic_mode):
    _check_parity(2, 140, 140, 128, static_mode, 16.0, dynamic_mode)


@pytest.mark.parametrize("static_mode,dynamic_mode", THREE_PAIRS + [("divide", None)])
def test_parity_256_phased_path(cuda, static_mode, dynamic_mode):
    _check_parity(2, 256, 256, 256, static_mode, 8.0, dynamic_mode)


def test_parity_phased_path_with_partial_bands(cuda):
    # 160 x 160: row bands 64 + 64 + 32, column bands likewise
    _check_parity(2, 163, 161, 160, "subtract", 4.0, "divide")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("static_mode,dynamic_mode", [(None, "subtract"), ("divide", "divide")])
def test_parity_float_sources_with_non_finite_values(cuda, dtype, static_mode, dynamic_mode):
    _check_parity(3, 70, 66, 64, static_mode, 2.0, dynamic_mode, dtype)


@pytest.mark.parametrize("H0,side,sigma", [(70, 64, 2.0), (140, 128, 16.0), (256, 256, 8.0)])
def test_a_pattern_does_not_depend_on_its_batch(cuda, H0, side, sigma):
    raw, bg = R.detector_patterns(5, H0, H0, seed=H0 + side)
    c = _correction(bg, "divide", sigma, "divide")
    batch = correct_patterns(raw, (side, side), c).cpu().numpy()
    for i in range(5):
        alone = correct_patterns(raw[i:i + 1], (side, side), c).cpu().numpy()
        assert alone.tobytes() == batch[i:i + 1].tobytes(), i


def test_a_single_2d_pattern_is_a_batch_of_one(cuda):
    raw, bg = R.detector_patterns(2, 140, 140, seed=268)
    c = _correction(bg, None, 16.0, "subtract")
    one = correct_patterns(raw[0], (128, 128), c)
    assert one.shape == (1, 1, 128, 128)
    assert one.cpu().numpy().tobytes() == correct_patterns(raw[:1], (128, 128), c).cpu().numpy().tobytes()


@pytest.mark.parametrize("H0,side", [(70, 64), (256, 256)])
def test_a_constant_pattern_gives_zeros(cuda, H0, side):
    raw = np.full((2, H0, H0), 93, np.uint8)
    out = torch.full((2, 1, side, side), -7.0, device=cuda)
    correct_patterns(raw, (side, side), PatternCorrection(), out=out)
    assert not out.cpu().numpy().any()


def test_out_is_written_in_place(cuda):
    raw, bg = R.detector_patterns(3, 70, 66, seed=134)
    c = _correction(bg, "subtract", 2.0, "subtract")
    want = correct_patterns(raw, (64, 64), c).cpu().numpy()
    big = torch.full((5, 1, 64, 64), -7.0, device=cuda)
    dev_raw = torch.from_numpy(raw).to(cuda)             # a device source
    assert correct_patterns(dev_raw, (64, 64), c, out=big[:3]).data_ptr() == big.data_ptr()
    host = big.cpu().numpy()
    assert host[:3].tobytes() == want.tobytes()
    assert (host[3:] == -7.0).all()
    with pytest.raises(ValueError, match="out must be"):
        correct_patterns(raw, (64, 64), c, out=torch.empty(3, 1, 64, 66, device=cuda))
    with pytest.raises(ValueError, match="out must be"):
        correct_patterns(raw, (64, 64), c, out=torch.empty(2, 1, 64, 64, device=cuda))
    # the background and the taps were uploaded once for this correction and device
    assert len(c._device_state) == 1
    bg_dev = c._device_state[dev_raw.device][0]
    correct_patterns(raw, (64, 64), c)
    assert c._device_state[dev_raw.device][0] is bg_dev


# ---------------------------------------------------------------- the indexer
@pytest.fixture(scope="module")
def indexer(cuda, tmp_path_factory):
    """A seeded random-weight model and a 64-row random dictionary.  The model is the 128 x 128
    one: the conv kernels take no 4 x 4 map (`conv3x3_fwd: unsupported shape H=4 W=4 cin=128
    cout=128`), so an image size of 64 builds a plan but cannot encode.  The scans of the
    plumbing test below are therefore 140 x 134 -> 128 x 128 (margins 12 and 6: offsets 6 and
    3) in place of 70 x 66 -> 64 x 64; pattern count, batch size and what is compared (every
    result array, bit for bit) are unchanged."""
    tmp = tmp_path_factory.mktemp("corr")
    m = VariationalAutoEncoderRawData(32, 16, 128)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0, 32, 16, 128).items()})
    rng = np.random.default_rng(5)
    db = F.FaissLatentVectorDatabase(F.FaissLatentVectorDatabaseConfig(dimension=16, device="cuda:0"))
    db.add_vectors(rng.standard_normal((64, 16)).astype(np.float32),
                   rng.uniform(0.0, 90.0, (64, 3)))
    cfg = IndexerConfig(pattern_path=tmp / "unused.npy", angles_path=tmp / "unused.txt",
                        batch_size=2, device="cuda", image_size=(128, 128))
    return DiffractionPatternIndexer(m.to(cuda), db=db, config=cfg), tmp


def test_scan_background_is_the_mean_pattern(indexer):
    ix, tmp = indexer
    scan, _ = R.detector_patterns(7, 70, 66, seed=7)
    want = np.float32(scan.astype(np.float64).mean(0))
    got = ix.scan_background(scan, batch_size=3)            # batches 3, 3, 1
    assert got.dtype == np.float32 and got.shape == (70, 66)
    assert np.array_equal(got, want)
    np.save(tmp / "scan.npy", scan)
    assert np.array_equal(ix.scan_background(tmp / "scan.npy", batch_size=3), want)
    assert np.array_equal(ix.scan_background(scan), want)   # the config's batch size (2)
    f32 = scan.astype(np.float32) * np.float32(1.37)
    got = ix.scan_background(f32, batch_size=3)
    ref = f32.astype(np.float64).mean(0)
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()
    with pytest.raises(ValueError):
        ix.scan_background(scan[:0])


def test_index_scan_with_a_correction_is_index_scan_of_the_corrected_patterns(indexer):
    ix, _ = indexer
    scan, _ = R.detector_patterns(5, 140, 134, seed=11)
    c = PatternCorrection(static_background=ix.scan_background(scan), static_mode="divide",
                          dynamic_sigma=2.0, dynamic_mode="subtract")
    kw = dict(top_n=10, orientation_threshold=5.0, min_required_matches=2, batch_size=2,
              return_candidates=True)
    got = ix.index_scan(scan, correction=c, **kw)
    want = ix.index_scan(correct_patterns(scan, (128, 128), c), **kw)
    assert len(got) == 5
    for name in ("orientations", "success", "scores", "top_index", "n_similar",
                 "candidate_indices", "candidate_scores"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    # the other staging dtypes take the same corrected ingest
    for dt in (np.float32, np.float64, np.uint16):
        again = ix.index_scan(scan.astype(dt), correction=c, **kw)
        assert again.scores.tobytes() == want.scores.tobytes(), dt
        assert again.top_index.tobytes() == want.top_index.tobytes(), dt
    # and without a correction the plain ingest still runs
    plain = ix.index_scan(scan, **kw)
    assert plain.scores.tobytes() != want.scores.tobytes()
    with pytest.raises(ValueError, match="already transformed"):
        ix.index_scan(correct_patterns(scan, (128, 128), c), correction=c)
