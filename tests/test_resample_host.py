"""Host side of the detector resample (latice.data_module: resample_axis, DetectorResample and
the size checks of resample_patterns / correct_patterns(resample=)) and the float64 restatement
tests/resample_ref.py against two independent evaluations.  No GPU.

The float32 restatement of the device's chains (resample_ref.resample_chain32) on the GPU tests'
inputs stays at most 3.0e-8 from the float64 restatement on uint8 / 255 (gates 8.5e-7 to
2.1e-6 there) and at most 5.5e-5 on the float sources of magnitude 350 (gates 3.0e-4 to
7.4e-4); the test below prints the figures and asserts the gate."""
import math

import numpy as np
import pytest

import resample_ref as R
from latice.data_module import (DetectorResample, PatternCorrection, check_resampled_correction,
                                resample_axis, resample_patterns)

AXIS_PAIRS = [(480, 128), (156, 128), (129, 128), (640, 128), (1024, 128), (2048, 256), (16, 16)]


@pytest.mark.parametrize("R_,O", AXIS_PAIRS)
def test_resample_axis_tables(R_, O):
    start, wts = resample_axis(R_, O)
    assert start.dtype == np.int32 and start.shape == (O,)
    assert wts.dtype == np.float32 and wts.shape[0] == O
    T = wts.shape[1]
    assert T <= math.ceil(R_ / O) + 1
    assert (start >= 0).all() and (start + T <= R_).all()          # every tap inside the region
    assert (np.diff(start) >= 0).all()
    # before the rounding to float32 the weights of an output sum to R / O within 1 ulp
    exact = R.overlap(R_, O, rounded=False)
    assert (np.abs(exact.sum(1) - R_ / O) <= np.spacing(R_ / O)).all()
    # and the table is that matrix: its taps, float32-rounded, zeros elsewhere
    dense = np.zeros((O, R_), np.float32)
    for t in range(T):
        dense[np.arange(O), start + t] += wts[:, t]
    assert np.array_equal(dense, exact.astype(np.float32))
    # the overlap is nonzero on consecutive pixels only
    for j in range(O):
        nz = np.flatnonzero(dense[j])
        assert nz.size and (np.diff(nz) == 1).all() and nz.size <= math.ceil(R_ / O) + 1
    if R_ % O == 0:
        assert T == R_ // O and (wts == 1.0).all()


def test_resample_axis_refuses_upsampling():
    with pytest.raises(ValueError):
        resample_axis(16, 17)
    with pytest.raises(ValueError):
        resample_axis(16, 0)


@pytest.mark.parametrize("shape,roi,size", [((64, 96), None, (16, 16)), ((60, 90), (2, 3, 48, 80), (8, 16)),
                                            ((128, 128), None, (16, 16)), ((32, 32), None, (32, 32))])
def test_reference_is_the_block_mean_for_integer_factors(shape, roi, size):
    raw = R.patterns(2, *shape)
    roi = roi or R.default_roi(*shape, *size)
    want = R.resample_block_mean(raw, roi, size, 255.0)
    for rounded in (True, False):
        got = R.resample(raw, roi, size, 255.0, rounded)
        assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("shape,roi,size", R.PARITY_SHAPES + [((480, 640), None, (128, 128))])
@pytest.mark.parametrize("dtype", ["uint8", "float64"])
def test_reference_is_the_summed_area_integral(shape, roi, size, dtype):
    roi = roi or R.default_roi(*shape, *size)
    raw = R.patterns(2, *shape, dtype, roi)
    div = 255.0 if dtype == "uint8" else 1.0
    got = R.resample(raw, roi, size, div, rounded=False)
    want = R.resample_summed_area(raw, roi, size, div)
    scale = R.load(raw, roi).max() / div
    assert np.abs(got - want).max() <= 1e-12 * max(scale, 1.0)


@pytest.mark.parametrize("shape,roi,size", R.PARITY_SHAPES)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_float32_chain_stays_inside_the_gpu_gate(shape, roi, size, dtype):
    roi = roi or R.default_roi(*shape, *size)
    raw = R.patterns(3, *shape, dtype, roi)
    div = 255.0 if dtype == "uint8" else 1.0
    got = R.resample_chain32(raw, roi, size, div, resample_axis)
    want = R.resample(raw, roi, size, div)
    xt, yt = resample_axis(roi[3], size[1])[1].shape[1], resample_axis(roi[2], size[0])[1].shape[1]
    gate = R.gate(xt, yt, R.load(raw, roi).max(), div)
    err = np.abs(got - want).max()
    print(f"{dtype} {shape} roi {roi} -> {size}: float32 chain err {err:.2e}, gate {gate:.2e}")
    assert np.isfinite(got).all() and err <= gate


def test_default_window():
    d = DetectorResample()
    assert d.window(480, 640, 128, 128) == (0, 80, 480, 480)
    assert d.window(150, 170, 128, 128) == (0, 10, 150, 150)
    assert d.window(150, 170, 64, 64) == (0, 10, 150, 150)
    # a non-square output: 3 : 4, m = min(480 // 3, 600 // 4) = 150
    assert d.window(480, 600, 96, 128) == (15, 0, 450, 600)
    # half-to-even offsets, as the centre crop: (135 - 130) / 2 = 2.5 -> 2, (133 - 130) / 2 -> 2
    assert d.window(135, 130, 64, 64) == (2, 0, 130, 130)
    assert d.window(133, 130, 64, 64) == (2, 0, 130, 130)
    assert DetectorResample((1, 2, 30, 40)).window(480, 640, 16, 16) == (1, 2, 30, 40)
    for shape, _, size in R.PARITY_SHAPES:
        assert d.window(*shape, *size) == R.default_roi(*shape, *size)


def test_size_checks_raise_before_the_device():
    d = DetectorResample()
    d.check(480, 640, 128, 128)
    d.check(1024, 1024, 128, 128)            # a factor of exactly 8
    d.check(128, 128, 128, 128)              # the identity
    with pytest.raises(ValueError, match="upsample"):
        d.check(100, 100, 128, 128)
    with pytest.raises(ValueError, match="factor above 8"):
        d.check(1025, 1025, 128, 128)
    with pytest.raises(ValueError, match="factor above 8"):
        DetectorResample((0, 0, 128, 1030)).check(128, 1100, 128, 128)
    for roi in ((-1, 0, 64, 64), (0, -1, 64, 64), (10, 0, 120, 64), (0, 70, 64, 64), (0, 0, 0, 64)):
        with pytest.raises(ValueError, match="leaves"):
            DetectorResample(roi).check(128, 128, 64, 64)
    with pytest.raises(ValueError, match="must lie within"):
        d.check(600, 600, 257, 257)
    with pytest.raises(ValueError, match="must lie within"):
        d.check(600, 600, 0, 16)
    with pytest.raises(ValueError, match="roi must be"):
        DetectorResample((1, 2, 3))
    # resample_patterns runs them (and its own) before it looks for a device
    raw = np.zeros((2, 100, 100), np.uint8)
    with pytest.raises(ValueError, match="upsample"):
        resample_patterns(raw, (128, 128))
    with pytest.raises(TypeError, match="uint8, float32 or float64"):
        resample_patterns(raw.astype(np.uint16), (64, 64))
    with pytest.raises(ValueError, match="divisor"):
        resample_patterns(raw, (64, 64), divisor=0.0)
    with pytest.raises(TypeError, match="DetectorResample"):
        resample_patterns(raw, (64, 64), resample=(0, 0, 64, 64))


def test_correction_checks_with_a_resample():
    d = DetectorResample()
    bg = np.full((150, 170), 100.0, np.float32)
    check_resampled_correction(PatternCorrection(static_background=bg, static_mode="divide",
                                                 dynamic_sigma=2.0), d, 150, 170, 64, 64)
    # the background stays at detector shape
    with pytest.raises(ValueError, match="static_background is"):
        check_resampled_correction(PatternCorrection(static_background=bg[:64, :64]), d, 150, 170, 64, 64)
    # divide: positive inside the region (columns 10 .. 159), anything outside it
    outside = bg.copy()
    outside[:, :10] = 0.0
    check_resampled_correction(PatternCorrection(static_background=outside, static_mode="divide"),
                               d, 150, 170, 64, 64)
    inside = bg.copy()
    inside[149, 159] = 0.0
    with pytest.raises(ValueError, match="positive"):
        check_resampled_correction(PatternCorrection(static_background=inside, static_mode="divide"),
                                   d, 150, 170, 64, 64)
    check_resampled_correction(PatternCorrection(static_background=inside, static_mode="subtract"),
                               d, 150, 170, 64, 64)
    # dynamic_sigma is in output pixels: radius 66 > 64
    with pytest.raises(ValueError, match="output pixels"):
        check_resampled_correction(PatternCorrection(dynamic_sigma=16.4), d, 150, 170, 64, 64)
    with pytest.raises(ValueError, match="upsample"):
        check_resampled_correction(PatternCorrection(), d, 60, 60, 64, 64)
