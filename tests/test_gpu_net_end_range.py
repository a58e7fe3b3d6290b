"""The fused network end across its input ranges (ebsdvae_net_end, ebsdvae_net_end_valu).

tests/test_gpu_kernels.py and tests/test_gpu_rect.py feed it one benign draw: targets
floor(u 255) / 255, w14 ~ 0.15 N(0, 1), loss gradient 1.  The MFMA form has two power-of-two
scalings of its own -- the weights by 2^kw from their maximum, the logit gradient g1 by 2^kg from
a bound on |g1| -- and two-piece fp16 splits of g1 and of the activation; the reference's BCE
takes any finite target (latice/lightning_module.py:79-92).  Every case here is
check_network_end (its asserts and gates, against the float64 oracle) with other inputs, on both
forms, through the C ABI on guarded buffers.

Maps, the smallest that reach each code shape: (64, 128) B = 2, one 64-row band with its 8-row
folds; (96, 128) B = 1, three 32-row bands whose halo rows cross band edges; (32, 256) B = 1, the
W = 256 kernels.

  u8      targets 0...255 (an unnormalised batch): |sigmoid - x| reaches 255, which a g1 scale
          taken from the loss gradient alone turns into fp16 infinities (NaN band sums and
          weight-gradient slices, while x_hat, g1 and the loss stay finite)
  hot     unit targets with single pixels of 255 on the first and last rows and on the two rows
          either side of the first band edge: a per-band scale has to see the halo rows r0 - 1
          and r0 + TH, and one outlier decides the scale of a whole band
  neg     targets in [-3, 4): outside [0, 1], inside the headroom of a scale from the loss
          gradient alone -- a failure of u8 / hot is the overflow, not the sign of a target
  wscale  w14 x 1e-5 and x 30: 2^kw and its exact undo; at 30 the logits reach several hundred,
          exp(-|x|) underflows, sigmoid is exactly 0 or 1
  g_loss  0, 65536, 1e-20: f16_shift_of(0) and both ends of kg; for 0 every gradient output is
          exactly zero while x_hat and the BCE sums still match
  planes  a one-hot plane (xhat ~ 90 at the pixel, -1e-2 elsewhere) and a constant one (xhat = 0,
          the a > 0 indicator at exactly 0): the activation's unscaled fp16 split at its largest
          and smallest magnitudes
"""
import pytest

from rect_util import AbiNetEnd, check_network_end

pytestmark = pytest.mark.gpu

MAPS = {"64x128": (64, 128, 2), "96x128": (96, 128, 1), "32x256": (32, 256, 1)}
ALL = list(MAPS)
FORMS = pytest.mark.parametrize("mfma", [True, False], ids=["mfma", "valu"])


def _check(mfma, where, **inputs):
    H, W, B = MAPS[where]
    check_network_end(H, W, ops=AbiNetEnd(mfma), B=B, **inputs)


@FORMS
@pytest.mark.parametrize("where", ALL)
def test_network_end_targets_0_to_255(cuda, where, mfma):
    _check(mfma, where, targets="u8")


@FORMS
@pytest.mark.parametrize("where", ALL)
def test_network_end_hot_pixels_at_band_edges(cuda, where, mfma):
    _check(mfma, where, targets="hot")


@FORMS
def test_network_end_targets_4_bytes_past_a_16_byte_boundary(cuda, mfma):
    """The header asks no alignment of x beyond a float's; the MFMA form's pass over the targets
    for its g1 scale reads them four at a time."""
    H, W, B = MAPS["96x128"]
    check_network_end(H, W, ops=AbiNetEnd(mfma, x_shift=1), B=B, targets="u8")


@FORMS
def test_network_end_targets_below_0_and_above_1(cuda, mfma):
    _check(mfma, "64x128", targets="neg")


@FORMS
@pytest.mark.parametrize("where,wscale", [("64x128", 1e-5), ("32x256", 30.0)])
def test_network_end_weight_magnitudes(cuda, where, wscale, mfma):
    _check(mfma, where, wscale=wscale)


@FORMS
@pytest.mark.parametrize("where,g_loss", [("64x128", 0.0), ("32x256", 65536.0), ("64x128", 1e-20)])
def test_network_end_loss_gradient_magnitudes(cuda, where, g_loss, mfma):
    _check(mfma, where, g_loss_value=g_loss)


@FORMS
def test_network_end_degenerate_planes(cuda, mfma):
    _check(mfma, "64x128", planes=True)
