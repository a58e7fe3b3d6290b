"""Split 3x3 convs, k-step 4: tap 8 stands alone there, and the lane half that used to multiply
the pack's zero tenth tap carries further piece products of tap 8 (csrc/conv_split.hip,
split_apiece / split_wrow).  A random nine-tap conv barely sees one wrong or missing cross
product of one tap (~2^-12 of a ninth of the sum), so these tests isolate single taps and make
one cross product carry 2^-12 = 2.4e-4 of every output value:

  ints_a  integer activations, weights m (1 + 2^-12): the pieces are a = (n, 0), b = (m, m 2^-12),
          so a0 b1 alone is 2^-12 of the result;
  ints_w  the roles swapped, activations n (1 + 2^-12) and integer weights: a1 b0 decisive.

A dropped, duplicated or mis-paired product misses SPLIT_TOL (1e-4 / 2e-5) by 2.4x / 12x or
more.  The forward's kernel tap t is the weight's (kh, kw) = (t / 3, t % 3); the input gradient
runs the flipped taps, so weight tap 0 is its kernel tap 8 -- both directions run taps 8, 7
and 0, which covers the packed k-step and its neighbours (k-step 3's hk = 1 half, k-step 0)
either way.  Reference: the float64 oracle (oracle/vae_oracle.py)."""
import numpy as np
import pytest

from latice import _native as N
from latice import engine as E
from oracle import vae_oracle as O
from test_gpu_kernels import FWD_PIECES, SPLIT_TOL, _pack_f16_dgrad, act_oracle, dev, h_oracle, host

pytestmark = pytest.mark.gpu

# (channels, H, B, forward source mode, pmode of the block feeding the layer): the smallest
# shapes that reach each instantiation family of plan_split -- resident weights with NF = 1,
# NF = 2 with double-buffered weights, NF = 2 with a single fragment set at 128 channels, the
# max-pool source (prefetch distance 1), and the 8x8 maps (register-resident weights under
# f16x3, two-image tiles under bf16x6; odd batch)
SHAPES = [
    (32, 128, 2, E.ACT_NORM, E.P_ID),
    (64, 64, 2, E.ACT_NORM, E.P_ID),
    (128, 32, 2, E.ACT_NORM, E.P_ID),
    (128, 16, 3, E.ACT_NORM_POOL, E.P_POOL),
    (128, 8, 5, E.ACT_NORM, E.P_ID),
]
TAPS = [8, 7, 0, None]   # the only non-zero weight tap; None: all nine, random
FWD_PRECS = [(s, p) for s in SHAPES for p in ("f16x3", "bf16x6")] + [(SHAPES[1], "bf16x3")]
DGRAD_PRECS = [(s, p) for s in SHAPES for p in ("f16x3", "bf16x6")]


def _id(v):
    if isinstance(v, tuple):
        return f"c{v[0]}h{v[1]}b{v[2]}"
    return "all" if v is None else str(v)


def _kinds(tap):
    return ("random",) if tap is None else ("random", "ints_a", "ints_w")


def _weights(rng, C, tap, kind):
    """(cout, cin, 3, 3) weights, non-zero at `tap` only (None: everywhere)."""
    if kind == "random":
        w = rng.standard_normal((C, C, 3, 3)) * 0.1
    else:
        w = rng.integers(1, 8, (C, C, 3, 3)).astype(np.float64) * rng.choice([-1.0, 1.0], (C, C, 3, 3))
        if kind == "ints_a":
            w *= 1 + 2.0 ** -12
    if tap is not None:
        keep = np.zeros((3, 3))
        keep[tap // 3, tap % 3] = 1.0
        w = w * keep
    return w


def _unit_stats(B, C):
    """{mean 0, rstd 1}: the normalisation is then exact, fma(v, 1, -0) = v."""
    return np.stack([np.zeros((B, C)), np.ones((B, C))], -1)


@pytest.mark.parametrize("tap", TAPS, ids=_id)
@pytest.mark.parametrize("shape,prec", FWD_PRECS, ids=_id)
def test_fwd_single_tap(cuda, shape, prec, tap):
    C, H, B, mode, _ = shape
    if not N.call("ebsdvae_conv3x3_split_supported", H, H, C, C, FWD_PIECES[prec]):
        pytest.skip("shape not covered by the split kernel")
    rng = np.random.default_rng(800 + C + H + (9 if tap is None else tap))
    Hs = 2 * H if mode == E.ACT_NORM_POOL else H
    layer = E.ConvLayer("t", E.KIND_CONV, C, C, H, mode, 0)
    for kind in _kinds(tap):
        w = _weights(rng, C, tap, kind)
        if kind == "random":
            s = rng.standard_normal((B, Hs, Hs, C)) * 1.5 + 0.3
            mean = s.mean(axis=(1, 2), keepdims=True)
            rstd = 1.0 / np.sqrt(s.var(axis=(1, 2), keepdims=True) + 1e-5)
            st = np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)
            b = rng.standard_normal(C) * 0.1
        else:
            # positive, so LeakyReLU is the identity and (pooled) activations stay integers
            s = rng.integers(1, 16, (B, Hs, Hs, C)).astype(np.float64)
            if kind == "ints_w":
                s *= 1 + 2.0 ** -12
            mean, rstd, st = 0.0, 1.0, _unit_stats(B, C)
            b = np.zeros(C)
        with E.precision(prec):
            y, _ = E.conv_forward(dev(s), dev(st), layer, dev(w), dev(b), B)
        ref = O.conv3x3(act_oracle(s, mean, rstd, mode), w, b)
        err = O.rel_err(host(y), ref)
        print(f"fwd {prec} C{C} H{H} tap {tap} {kind}: {err:.3e}")
        assert err < SPLIT_TOL[prec], (kind, err)


@pytest.mark.parametrize("tap", TAPS, ids=_id)
@pytest.mark.parametrize("shape,prec", DGRAD_PRECS, ids=_id)
def test_dgrad_fused_single_tap(cuda, shape, prec, tap):
    """The fused input gradient (h = g * lrelu'(xhat) of the block feeding the layer); under
    f16x3 with the per-image power-of-two gradient scale, the images 64x apart."""
    C, H, B, _, pmode = shape
    if not N.call("ebsdvae_conv3x3_split_supported", H, H, C, C, FWD_PIECES[prec]):
        pytest.skip("shape not covered by the split kernel")
    rng = np.random.default_rng(900 + C + H + (9 if tap is None else tap))
    Hy = 2 * H if pmode == E.P_POOL else H
    y = rng.standard_normal((B, Hy, Hy, C)) * 2 + 0.5
    xh, mean, rstd = O.instance_norm(y)
    st = np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)
    layer = E.ConvLayer("t", E.KIND_CONV, C, C, H, E.ACT_RAW, 0)
    y_d, st_d = dev(y), dev(st)
    for kind in _kinds(tap):
        w = _weights(rng, C, tap, kind)
        if kind == "random":
            gy = rng.standard_normal((B, H, H, C))
        else:
            gy = rng.integers(1, 16, (B, H, H, C)).astype(np.float64) * rng.choice([-1.0, 1.0], (B, H, H, C))
            if kind == "ints_w":
                gy *= 1 + 2.0 ** -12
        gy[1] *= 64.0
        with E.precision(prec):
            w_d, g_d = dev(w), dev(gy)
            wd = None
            if prec == "f16x3":
                wd = _pack_f16_dgrad(w_d, layer)
                g_d.ev_gmax = dev(np.abs(gy).reshape(B, -1).max(1, keepdims=True))
            gin, _ = E.conv_dgrad(g_d, layer, w_d, prev=(y_d, st_d, pmode), wd=wd)
        hn = h_oracle(O.conv3x3_dgrad(gy, w), xh, pmode)
        got = host(gin)
        for bi in range(B):   # per image: they differ in magnitude
            err = O.rel_err(got[bi], hn[bi])
            print(f"dgrad {prec} C{C} H{H} tap {tap} {kind} image {bi}: {err:.3e}")
            assert err < SPLIT_TOL[prec], (kind, bi, err)
