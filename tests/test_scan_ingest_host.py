"""Construction of the per-scan ingest plan (latice.patterns.ScanIngest): the route it fixes and
the intermediate it allocates for every staging dtype, with and without a correction and a
resample, and the refusals it raises.  No GPU: the plan is built for the "cpu" device, where its
intermediate is an ordinary host tensor, and nothing here reaches the library."""
import numpy as np
import pytest
import torch

from latice import _native as N
from latice.index.scan import scan_dtype_code
from latice.patterns import DetectorResample, PatternCorrection, ScanIngest

SHAPE, SIZE, BATCH = (150, 170), (64, 64), 5


@pytest.fixture
def no_device(monkeypatch):
    """Any call into the library fails the test."""
    def boom(name, *a):
        raise AssertionError(f"{name} reached the library")
    monkeypatch.setattr(N, "call", boom)


# (staging dtype, correction, resample) -> (route, needs the float32 intermediate): what the
# streaming loops decided per batch before the plan existed.  Without a resample the correction
# wins over the dtype, else uint8 and float data have their own plain ingest; none needs a
# buffer.  With one, uint8 is binned straight to v / 255, float data is binned into the
# intermediate and ingested from there, and a corrected scan is binned into it whatever its dtype.
ROUTES = [
    ("float64", False, False, "float", False),
    ("float32", False, False, "float", False),
    ("uint8", False, False, "u8", False),
    ("float64", True, False, "corrected", False),
    ("float32", True, False, "corrected", False),
    ("uint8", True, False, "corrected", False),
    ("float64", False, True, "binned_float", True),
    ("float32", False, True, "binned_float", True),
    ("uint8", False, True, "binned_u8", False),
    ("float64", True, True, "binned_corrected", True),
    ("float32", True, True, "binned_corrected", True),
    ("uint8", True, True, "binned_corrected", True),
]


@pytest.mark.parametrize("dtype,corrected,binned,route,mid", ROUTES)
def test_route_and_intermediate(no_device, dtype, corrected, binned, route, mid):
    bg = np.full(SHAPE, 100.0, np.float32)
    c = PatternCorrection(static_background=bg, static_mode="divide", dynamic_sigma=2.0) \
        if corrected else None
    plan = ScanIngest(SHAPE, scan_dtype_code(np.dtype(dtype)), SIZE, "cpu", BATCH, c,
                      DetectorResample() if binned else None)
    assert plan.route == route
    assert plan.needs_intermediate is mid
    if mid:
        assert plan.intermediate.shape == (BATCH, 1) + SIZE
        assert plan.intermediate.dtype == torch.float32 and plan.intermediate.is_contiguous()
    else:
        assert plan.intermediate is None


def test_any_other_dtype_is_staged_as_float64():
    assert ScanIngest(SHAPE, scan_dtype_code(np.int16), SIZE, "cpu", BATCH).route == "float"


def _plan(shape=SHAPE, dtype=np.uint8, correction=None, resample=None):
    return ScanIngest(shape, scan_dtype_code(dtype), SIZE, "cpu", BATCH, correction, resample)


def test_refusals_come_from_construction(no_device):
    d = DetectorResample()
    with pytest.raises(ValueError, match="does not fit"):            # H0 < h: no padding
        _plan((60, 66), correction=PatternCorrection(dynamic_sigma=2.0))
    with pytest.raises(ValueError, match="upsample"):
        _plan((60, 60), resample=d)
    with pytest.raises(ValueError, match="upsample"):                # not "does not fit"
        _plan((60, 60), correction=PatternCorrection(), resample=d)
    with pytest.raises(ValueError, match="radius"):                  # r = 66 > 64
        _plan(correction=PatternCorrection(dynamic_sigma=16.4))
    with pytest.raises(ValueError, match="radius.*output's"):        # in output pixels
        _plan(correction=PatternCorrection(dynamic_sigma=16.4), resample=d)
    hole = np.full(SHAPE, 100.0, np.float32)
    hole[149, 159] = 0.0          # inside the resampled region (columns 10 .. 159), outside the crop
    divide = PatternCorrection(static_background=hole, static_mode="divide")
    _plan(correction=divide)
    with pytest.raises(ValueError, match="positive everywhere inside the resampled region"):
        _plan(correction=divide, resample=d)
    hole[75, 85] = 0.0            # inside both
    divide = PatternCorrection(static_background=hole, static_mode="divide")
    with pytest.raises(ValueError, match="positive everywhere inside the cropped window"):
        _plan(correction=divide)
    with pytest.raises(ValueError, match="static_background is"):    # stays at detector shape
        _plan(correction=PatternCorrection(static_background=hole[:64, :64]), resample=d)
    with pytest.raises(TypeError, match="correction must be a PatternCorrection"):
        _plan(correction="dynamic")
    with pytest.raises(TypeError, match="resample must be a DetectorResample"):
        _plan(resample=(0, 10, 150, 150))
