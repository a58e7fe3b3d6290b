"""Host side of the pattern correction (latice.data_module.PatternCorrection, gaussian_taps,
correct_patterns' checks, index_scan(correction=)) and the float64 oracle the GPU tests compare
against (tests/correction_ref.py).  No GPU: every rejection here must come before any device
use, so none of these reaches the library."""
from unittest.mock import MagicMock

import numpy as np
import pytest
import torch

import correction_ref as R
from latice import _native as N
from latice import data_module as D
from latice.data_module import PatternCorrection, correct_patterns, gaussian_taps
from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig
from latice.index.faiss_db import FaissLatentVectorDatabase


@pytest.mark.parametrize("side,sigma", [(64, 2.0), (64, 15.9), (128, 16.0)])
def test_oracle_blur_is_scipy_gaussian_filter(side, sigma):
    from scipy.ndimage import gaussian_filter
    raw, _ = R.detector_patterns(2, side, side, seed=3)
    s = raw.astype(np.float64)
    _, r = R.taps64(sigma)
    assert r == int(4 * sigma + 0.5) and r <= side
    if sigma == 15.9:
        assert r == side          # the maximal reflection
    for p in s:
        want = gaussian_filter(p, sigma, mode="reflect", truncate=4.0)
        assert np.abs(R.blur(p, sigma) - want).max() <= 1e-11


@pytest.mark.parametrize("sigma", [0.3, 2.0, 15.9, 16.0])
def test_gaussian_taps(sigma):
    taps, r = gaussian_taps(sigma)
    want, want_r = R.taps64(sigma)
    assert r == want_r == int(4 * sigma + 0.5)
    assert taps.dtype == np.float32 and taps.shape == (r + 1,)
    assert np.array_equal(taps, want.astype(np.float32))
    assert abs(float(taps[0]) + 2.0 * float(taps[1:].astype(np.float64).sum()) - 1.0) < 1e-6


def test_crop_offsets_round_half_to_even():
    for size, crop in [(70, 64), (66, 64), (140, 128), (133, 128), (131, 128), (64, 64)]:
        assert D._crop_offset(size, crop) == R.crop_offset(size, crop)
    assert [D._crop_offset(s, 64) for s in (65, 67, 69, 71)] == [0, 2, 2, 4]


def test_correction_validates_on_construction():
    bg = np.full((70, 66), 100.0)
    c = PatternCorrection(static_background=bg, static_mode="divide", dynamic_sigma=2,
                          dynamic_mode="subtract")
    assert c.static_background.dtype == np.float32 and c.static_background.shape == (70, 66)
    assert (c.static_code, c.dynamic_code) == (2, 1)
    assert (PatternCorrection().static_code, PatternCorrection().dynamic_code) == (0, 0)
    with pytest.raises(Exception):          # frozen
        c.dynamic_sigma = 3.0
    bg[0, 0] = -1.0                         # the correction holds its own copy
    assert c.static_background[0, 0] == 100.0
    with pytest.raises(ValueError, match="static_mode"):
        PatternCorrection(static_background=bg, static_mode="minus")
    with pytest.raises(ValueError, match="dynamic_mode"):
        PatternCorrection(dynamic_sigma=2.0, dynamic_mode="over")
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="dynamic_sigma"):
            PatternCorrection(dynamic_sigma=sigma)
    with pytest.raises(ValueError, match="2-D"):
        PatternCorrection(static_background=np.ones((3, 70, 66)))
    for bad in (np.nan, np.inf):
        b = np.ones((70, 66))
        b[5, 5] = bad
        with pytest.raises(ValueError, match="non-finite"):
            PatternCorrection(static_background=b)


@pytest.fixture
def no_device(monkeypatch):
    """Any call into the library fails the test."""
    def boom(name, *a):
        raise AssertionError(f"{name} reached the library")
    monkeypatch.setattr(N, "call", boom)


def test_correct_patterns_rejects_before_any_device_use(no_device):
    raw = np.zeros((2, 70, 66), np.uint8)
    ok = np.full((70, 66), 50.0)
    with pytest.raises(ValueError, match=r"\(70, 60\)"):       # a background of the wrong shape
        correct_patterns(raw, (64, 64), PatternCorrection(static_background=np.ones((70, 60))))
    neg = ok.copy()
    neg[35, 33] = 0.0                                          # inside the 64 x 64 window
    with pytest.raises(ValueError, match="positive"):
        correct_patterns(raw, (64, 64), PatternCorrection(static_background=neg, static_mode="divide"))
    with pytest.raises(ValueError, match="does not fit"):      # H0 < h: no padding
        correct_patterns(raw, (72, 64), PatternCorrection())
    with pytest.raises(ValueError, match="does not fit"):
        correct_patterns(raw, (64, 68), PatternCorrection(dynamic_sigma=2.0))
    with pytest.raises(ValueError, match="radius"):            # r = 65 > 64
        correct_patterns(raw, (64, 64), PatternCorrection(dynamic_sigma=16.2))
    with pytest.raises(ValueError, match="radius"):            # r = 33 > min(64, 32)
        correct_patterns(np.zeros((1, 64, 32), np.uint8), (64, 32), PatternCorrection(dynamic_sigma=8.2))
    with pytest.raises(ValueError, match="B, H, W"):
        correct_patterns(np.zeros((1, 1, 70, 66), np.uint8), (64, 64), PatternCorrection())
    with pytest.raises(ValueError, match="within"):
        correct_patterns(np.zeros((1, 300, 300), np.uint8), (288, 288), PatternCorrection())
    with pytest.raises(ValueError, match="out must be"):
        correct_patterns(raw, (64, 64), PatternCorrection(), out=torch.empty(2, 1, 64, 60))
    with pytest.raises(ValueError, match="out must be"):       # the plain ingest checks it too
        D.ingest_patterns(raw, (64, 64), out=torch.empty(2, 1, 64, 60))
    with pytest.raises(TypeError, match="uint8, float32 or float64"):
        correct_patterns(raw.astype(np.int16), (64, 64), PatternCorrection())
    with pytest.raises(TypeError, match="PatternCorrection"):
        correct_patterns(raw, (64, 64), None)


def test_a_background_that_is_bad_outside_the_window_only_is_accepted():
    bg = np.full((70, 66), 50.0)
    bg[0, 0] = 0.0            # rows 0..2 and column 0 are cropped away (offsets 3 and 1)
    PatternCorrection(static_background=bg, static_mode="divide").check(70, 66, 64, 64)
    bg[3, 1] = 0.0            # the window's first pixel
    with pytest.raises(ValueError, match="positive"):
        PatternCorrection(static_background=bg, static_mode="divide").check(70, 66, 64, 64)


def test_index_scan_rejects_a_correction_on_a_tensor_scan(tmp_path, no_device):
    cfg = IndexerConfig(pattern_path=tmp_path / "p.npy", angles_path=tmp_path / "a.txt",
                        device="cpu", image_size=(64, 64))
    ix = DiffractionPatternIndexer(MagicMock(), MagicMock(spec=FaissLatentVectorDatabase), cfg)
    c = PatternCorrection(dynamic_sigma=2.0)
    with pytest.raises(ValueError, match="already transformed"):
        ix.index_scan(torch.zeros(3, 1, 64, 64), correction=c)
    with pytest.raises(TypeError, match="PatternCorrection"):
        ix.index_scan(np.zeros((3, 70, 66), np.uint8), correction="dynamic")
    # sizes are checked before the scan is staged
    with pytest.raises(ValueError, match="does not fit"):
        ix.index_scan(np.zeros((3, 60, 66), np.uint8), correction=c)


def test_oracle_follows_the_definition_on_a_tiny_case():
    """One 70 x 66 pattern worked by hand: crop offsets (3, 1), static divide, then no dynamic
    step, rescale."""
    raw, bg = R.detector_patterns(1, 70, 66, seed=1)
    ref = R.correct(raw, (64, 64), R.static_background(bg, "divide"), "divide")
    s = raw[0, 3:67, 1:65].astype(np.float64) / bg.astype(np.float32)[3:67, 1:65]
    want = (s - s.min()) / (s.max() - s.min())
    assert np.array_equal(ref["out"][0, 0], want)
    assert ref["out"].min() == 0.0 and ref["out"].max() == 1.0
    const = R.correct(np.full((1, 70, 66), 7, np.uint8), (64, 64))
    assert not const["out"].any()
