"""Detector resampling on the device (csrc/resample.hip): ebsdvae_resample_patterns called
through the C ABI on sentinel-guarded buffers, then latice.data_module.resample_patterns,
correct_patterns(resample=) and index_scan(resample=).

Parity gate, derived in tests/resample_ref.py (`gate`), not measured:
    max |out - ref| <= 2 (xtaps + ytaps + 4) 2^-24 max|v| / divisor
against the float64 restatement resample_ref.resample.  The shapes are the smallest at which
each mechanism of the kernel can go wrong:
    (60, 60) -> 16 x 16            factor 3.75, 5 taps, two bands of 8 output rows
    (50, 70) roi (3, 5, 45, 61) -> (12, 16)   odd offsets, a width that is no multiple of 4 (uint8
                                   rows start at every byte of a word; the source pointer is odd),
                                   factors 3.75 x 3.8125, a partial last band
    (128, 128) -> 16 x 16          factor 8: 8 taps of weight 1, and float64 planes that take two
                                   chunks of output columns (9 taps, the widest table rows, need
                                   a fractional factor: test_nine_taps, 127 -> 16)
    (39, 39) -> 32 x 32            factor 1.22, most outputs straddle two pixels
    (31, 64) -> 8 x 8              the region is the whole pattern: the first and the last word
                                   of the batch, source pointer odd
    (129, 129) -> 128 x 128        every band boundary shares a source row
The measured maxima are printed; DESIGN.md section 14 records them."""
import functools

import numpy as np
import pytest
import torch

import correction_ref as C
import resample_ref as R
from latice.data_module import (DetectorResample, NeighbourAverage, PatternCorrection,
                                correct_patterns, ingest_patterns, ingest_patterns_u8,
                                resample_axis, resample_patterns)
from latice.index import faiss_db as F
from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig
from latice.model import VariationalAutoEncoderRawData
from latice.seeding import seeded_state_dict
from rect_util import Guarded, run, stream

pytestmark = pytest.mark.gpu

NAME = "ebsdvae_resample_patterns"
CODES = {"float64": 0, "float32": 1, "uint8": 2}


@functools.lru_cache(maxsize=None)
def _tables(R_, O):
    start, wts = resample_axis(R_, O)
    return torch.from_numpy(start).cuda(), torch.from_numpy(wts).cuda(), wts.shape[1]


def _source(raw, shift=0):
    """The batch on the device, `shift` bytes past the allocation's (aligned) start."""
    flat = torch.from_numpy(np.ascontiguousarray(raw)).reshape(-1)
    if not shift:
        return flat.cuda()
    assert raw.dtype == np.uint8
    buf = torch.empty(flat.numel() + shift, dtype=torch.uint8, device="cuda")
    src = buf[shift:]
    src.copy_(flat)
    assert src.data_ptr() % 4 == shift % 4
    return src


def _args(src, raw, roi, size, divisor, dst):
    B, H0, W0 = raw.shape
    ys, yw, yt = _tables(roi[2], size[0])
    xs, xw, xt = _tables(roi[3], size[1])
    return dict(src=src.data_ptr(), src_dtype=CODES[str(raw.dtype)], B=B, H0=H0, W0=W0, top=roi[0],
                left=roi[1], rh=roi[2], rw=roi[3], out_h=size[0], out_w=size[1],
                ystart=ys.data_ptr(), ywts=yw.data_ptr(), ytaps=yt, xstart=xs.data_ptr(),
                xwts=xw.data_ptr(), xtaps=xt, denom=float(R.denominator(roi, size, divisor)),
                dst=dst.ptr(), stream=stream())


def _resample(raw, roi, size, divisor, shift=0):
    """The entry point on a guarded output: (B, 1, h, w) float32 on the host."""
    dst = Guarded((raw.shape[0], 1) + tuple(size), raw.shape[0])
    src = _source(raw, shift)
    assert run(NAME, [dst], *_args(src, raw, roi, size, divisor, dst).values(), must=True)
    assert dst.written()
    return dst.t.cpu().numpy()


def _check_parity(B, shape, roi, size, dtype, shift=0):
    roi = roi or R.default_roi(*shape, *size)
    raw = R.patterns(B, *shape, dtype, roi)
    div = 255.0 if dtype == "uint8" else 1.0
    got = _resample(raw, roi, size, div, shift)
    want = R.resample(raw, roi, size, div)
    xt, yt = _tables(roi[3], size[1])[2], _tables(roi[2], size[0])[2]
    gate = R.gate(xt, yt, R.load(raw, roi).max(), div)
    err = np.abs(got - want).max()
    print(f"{dtype} {shape} roi {roi} -> {size} taps {yt} x {xt}: max err {err:.2e}, gate {gate:.2e}")
    assert np.isfinite(got).all()
    assert err <= gate, (err, gate)
    assert _resample(raw, roi, size, div, shift).tobytes() == got.tobytes()   # two runs agree
    return got


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("shape,roi,size", R.PARITY_SHAPES)
def test_parity(cuda, shape, roi, size, dtype):
    odd_pointer = dtype == "uint8" and roi is not None
    _check_parity(3, shape, roi, size, dtype, shift=1 if odd_pointer else 0)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_uint8_rows_at_every_byte_of_a_word(cuda, shift):
    _check_parity(3, (50, 70), (3, 5, 45, 61), (12, 16), "uint8", shift)


def test_nine_taps(cuda):
    # 127 -> 16: factor 7.94, outputs that overlap 9 source pixels
    assert _tables(127, 16)[2] == 9
    _check_parity(3, (127, 127), None, (16, 16), "float32")


def test_parity_480x640_to_128(cuda):
    _check_parity(2, (480, 640), None, (128, 128), "uint8")


def test_parity_2048_to_256(cuda):
    # the source plane of a band does not fit LDS: chunks of output columns
    _check_parity(1, (2048, 2048), None, (256, 256), "uint8")


def test_column_chunks_with_fractional_factors(cuda):
    # float64 at 7.5 x: 10 output columns per chunk, a partial last chunk of 6
    _check_parity(2, (330, 570), (0, 0, 330, 570), (44, 76), "float64")


# ---------------------------------------------------------------- bitwise
@pytest.mark.parametrize("shape,roi,size", [((16, 16), (0, 0, 16, 16), (16, 16)),
                                            ((140, 140), (6, 6, 128, 128), (128, 128))])
def test_identity_is_the_uint8_ingest(cuda, shape, roi, size):
    raw = R.patterns(3, *shape)
    got = _resample(raw, roi, size, 255.0)
    want = ingest_patterns_u8(raw, size).cpu().numpy()
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("shape,size", [((32, 32), (16, 16)), ((48, 48), (16, 16)),
                                        ((128, 128), (16, 16)), ((32, 48), (16, 16))])
def test_integer_factors_on_uint8_are_exact_sums(cuda, shape, size):
    raw = R.patterns(3, *shape)
    k, l = shape[0] // size[0], shape[1] // size[1]
    got = _resample(raw, (0, 0) + shape, size, 255.0)
    sums = raw.astype(np.int64).reshape(3, size[0], k, size[1], l).sum(axis=(2, 4))
    want = (sums.astype(np.float32) / np.float32(k * l * 255))[:, None]
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("shape,size,dtype", [((60, 60), (16, 16), "float32"),
                                              ((129, 129), (128, 128), "uint8")])
def test_a_pattern_does_not_depend_on_its_batch(cuda, shape, size, dtype):
    roi = R.default_roi(*shape, *size)
    raw = R.patterns(5, *shape, dtype, roi)
    batch = _resample(raw, roi, size, 1.0)
    for i in (0, 3, 4):
        alone = _resample(raw[i:i + 1], roi, size, 1.0)
        assert alone.tobytes() == batch[i:i + 1].tobytes(), i
    swapped = _resample(np.ascontiguousarray(raw[::-1]), roi, size, 1.0)
    assert swapped[::-1].tobytes() == batch.tobytes()


# ---------------------------------------------------------------- refusals
REFUSALS = {
    "null src": dict(src=None), "null dst": dict(dst=None), "null ystart": dict(ystart=None),
    "null ywts": dict(ywts=None), "null xstart": dict(xstart=None), "null xwts": dict(xwts=None),
    "roi below": dict(top=20), "roi right": dict(left=10), "roi negative top": dict(top=-1),
    "roi negative left": dict(left=-1),
    "upsampling rows": dict(rh=15), "upsampling columns": dict(rw=15),
    "factor above 8": dict(out_h=7), "factor above 8 columns": dict(out_w=7),
    "out_h 0": dict(out_h=0), "out_w 257": dict(out_w=257, rw=60),
    "ytaps 0": dict(ytaps=0), "ytaps 10": dict(ytaps=10), "xtaps 0": dict(xtaps=0),
    "xtaps 10": dict(xtaps=10),
    "denom 0": dict(denom=0.0), "denom negative": dict(denom=-1.0),
    "denom inf": dict(denom=float("inf")), "denom nan": dict(denom=float("nan")),
    "src_dtype": dict(src_dtype=3),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_write_nothing(cuda, case):
    raw = R.patterns(3, 64, 64)
    roi, size = (2, 3, 60, 60), (16, 16)
    dst = Guarded((3, 1) + size, 3)
    src = _source(raw)
    args = _args(src, raw, roi, size, 255.0, dst)
    args.update(REFUSALS[case])
    if case == "null dst":
        lib_rc = run(NAME, [], *args.values())
    else:
        lib_rc = run(NAME, [dst], *args.values())     # asserts a message and an untouched dst
    assert lib_rc is False
    assert dst.untouched()


# ---------------------------------------------------------------- the Python entry points
def test_resample_patterns_is_the_entry_point(cuda):
    raw = R.patterns(3, 50, 70)
    d = DetectorResample((3, 5, 45, 61))
    want = _resample(raw, d.roi, (12, 16), 255.0)
    got = resample_patterns(raw, (12, 16), d, 255.0)
    assert got.shape == (3, 1, 12, 16) and got.dtype == torch.float32 and got.is_cuda
    assert got.cpu().numpy().tobytes() == want.tobytes()
    one = resample_patterns(raw[0], (12, 16), d, 255.0)      # a 2-D pattern is a batch of one
    assert one.shape == (1, 1, 12, 16) and one.cpu().numpy().tobytes() == want[:1].tobytes()
    big = torch.full((5, 1, 12, 16), -7.0, device=cuda)
    dev_raw = torch.from_numpy(raw).to(cuda)
    assert resample_patterns(dev_raw, (12, 16), d, 255.0, out=big[:3]).data_ptr() == big.data_ptr()
    host = big.cpu().numpy()
    assert host[:3].tobytes() == want.tobytes() and (host[3:] == -7.0).all()
    with pytest.raises(ValueError, match="out must be"):
        resample_patterns(raw, (12, 16), d, out=torch.empty(2, 1, 12, 16, device=cuda))
    # the tables were built once for this geometry and device
    assert len(d._device_state) == 1
    # the default window: the centred square
    sq = resample_patterns(raw, (16, 16)).cpu().numpy()
    assert sq.tobytes() == _resample(raw, (0, 10, 50, 50), (16, 16), 1.0).tobytes()


def _correction_case():
    raw, bg = C.detector_patterns(3, 150, 170, seed=321)
    sbg = C.static_background(bg, "subtract")                       # (150, 170) float32
    c = PatternCorrection(static_background=sbg, static_mode="subtract", dynamic_sigma=2.0,
                          dynamic_mode="divide")
    return raw, sbg, c


def test_correct_patterns_with_a_resample_is_the_two_stages(cuda):
    raw, sbg, c = _correction_case()
    d, size = DetectorResample(), (64, 64)
    got = correct_patterns(raw, size, c, resample=d).cpu().numpy()
    binned = resample_patterns(raw, size, d)[:, 0]                   # (3, 64, 64) float32, device
    binned_bg = resample_patterns(sbg, size, d).cpu().numpy()[0, 0]
    c2 = PatternCorrection(static_background=binned_bg, static_mode="subtract", dynamic_sigma=2.0,
                           dynamic_mode="divide")
    want = correct_patterns(binned, size, c2).cpu().numpy()
    assert got.tobytes() == want.tobytes()
    # the binned background is cached per (correction, device, geometry)
    n = len(c._device_state)
    assert correct_patterns(raw, size, c, resample=d).cpu().numpy().tobytes() == want.tobytes()
    assert len(c._device_state) == n
    # the intermediate may be supplied, and out is written in place
    mid = torch.empty(4, 1, 64, 64, device=cuda)
    out = torch.full((3, 1, 64, 64), -7.0, device=cuda)
    correct_patterns(raw, size, c, out=out, resample=d, intermediate=mid)
    assert out.cpu().numpy().tobytes() == want.tobytes()
    assert mid[:3].cpu().numpy().tobytes() == binned.cpu().numpy().tobytes()


def test_correct_patterns_with_a_resample_parity(cuda):
    raw, sbg, c = _correction_case()
    size = (64, 64)
    roi = R.default_roi(150, 170, *size)
    binned = R.resample(raw, roi, size)[:, 0]
    binned_bg = R.resample(sbg[None], roi, size)[0, 0]
    ref = C.correct(binned, size, binned_bg, "subtract", 2.0, "divide")
    C.assert_well_conditioned(ref, True)
    got = correct_patterns(raw, size, c, resample=DetectorResample()).cpu().numpy()
    err = np.abs(got - ref["out"]).max()
    print(f"correct_patterns(resample) (150, 170) -> 64 x 64: max err {err:.2e}")
    assert np.isfinite(got).all() and err <= 2e-5, err


# ---------------------------------------------------------------- the indexer
@pytest.fixture(scope="module")
def indexer(cuda, tmp_path_factory):
    """The seeded 128 x 128 model and a 64-row random dictionary, as
    tests/test_gpu_pattern_correction.py builds them."""
    tmp = tmp_path_factory.mktemp("resample")
    m = VariationalAutoEncoderRawData(32, 16, 128)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0, 32, 16, 128).items()})
    rng = np.random.default_rng(5)
    db = F.FaissLatentVectorDatabase(F.FaissLatentVectorDatabaseConfig(dimension=16, device="cuda:0"))
    db.add_vectors(rng.standard_normal((64, 16)).astype(np.float32),
                   rng.uniform(0.0, 90.0, (64, 3)))
    cfg = IndexerConfig(pattern_path=tmp / "unused.npy", angles_path=tmp / "unused.txt",
                        batch_size=2, device="cuda", image_size=(128, 128))
    return DiffractionPatternIndexer(m.to(cuda), db=db, config=cfg)


KW = dict(top_n=10, orientation_threshold=5.0, min_required_matches=2, return_candidates=True)
FIELDS = ("orientations", "success", "scores", "top_index", "n_similar", "candidate_indices",
          "candidate_scores")


def _same(got, want):
    assert len(got) == len(want)
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name


@pytest.fixture(scope="module")
def scan():
    return C.detector_patterns(12, 150, 170, seed=77)


@pytest.mark.parametrize("b", [5, 64])
def test_index_scan_with_a_resample(indexer, scan, b):
    raw, bg = scan
    d = DetectorResample()
    resident = resample_patterns(raw, (128, 128), d, 255.0)
    want = indexer.index_scan(resident, batch_size=b, **KW)
    _same(indexer.index_scan(raw, resample=d, batch_size=b, **KW), want)
    # with a neighbour average on the 3 x 4 scan grid
    na = NeighbourAverage((3, 4))
    _same(indexer.index_scan(raw, resample=d, neighbour_average=na, batch_size=b, **KW),
          indexer.index_scan(resident, neighbour_average=na, batch_size=b, **KW))
    # with a correction: the background stays at detector shape
    c = PatternCorrection(static_background=indexer.scan_background(raw), static_mode="divide",
                          dynamic_sigma=2.0, dynamic_mode="subtract")
    corrected = correct_patterns(raw, (128, 128), c, resample=d)
    want_c = indexer.index_scan(corrected, batch_size=b, **KW)
    _same(indexer.index_scan(raw, resample=d, correction=c, batch_size=b, **KW), want_c)
    assert want_c.scores.tobytes() != want.scores.tobytes()
    _same(indexer.index_scan(raw, resample=d, correction=c, neighbour_average=na, batch_size=b, **KW),
          indexer.index_scan(corrected, neighbour_average=na, batch_size=b, **KW))


def test_index_scan_of_a_float_scan_with_a_resample(indexer, scan):
    raw = (scan[0].astype(np.float32) / np.float32(255))
    d = DetectorResample()
    resident = ingest_patterns(resample_patterns(raw, (128, 128), d)[:, 0], (128, 128))
    _same(indexer.index_scan(raw, resample=d, batch_size=5, **KW),
          indexer.index_scan(resident, batch_size=5, **KW))


def test_index_scan_refuses_a_resample_it_cannot_run(indexer, scan):
    raw, _ = scan
    d = DetectorResample()
    with pytest.raises(ValueError, match="already transformed"):
        indexer.index_scan(resample_patterns(raw, (128, 128), d, 255.0), resample=d)
    with pytest.raises(ValueError, match="upsample"):
        indexer.index_scan(raw[:, :100, :100], resample=d)
    with pytest.raises(TypeError, match="DetectorResample"):
        indexer.index_scan(raw, resample=(0, 10, 150, 150))
