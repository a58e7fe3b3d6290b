"""Helpers of tests/test_gpu_rect.py (and, for the network end, tests/test_gpu_net_end_range.py):
the C ABI called directly on rectangular (H != W) maps.

Every output is carved out of a larger tensor filled with a sentinel (Guarded), with at least
one image's worth of elements of slack before and after it, so an overrun of a row or an image
is seen instead of landing in the caching allocator's pool.  `run` is the right-or-refused
rule: an entry point either returns 0 (then the slack is intact and the caller compares
against the float64 oracle at the gate of the square test of that entry point), or returns
nonzero with a message in ebsdvae_last_error() and every output still holding its sentinel.
Helpers and tolerances come from tests/test_gpu_kernels.py."""
import ctypes

import numpy as np
import pytest
import torch

from latice import _native as N
from latice import engine as E
from oracle import vae_oracle as O
from test_gpu_kernels import (FWD_PIECES, SPLIT_TOL, TOL, act_oracle, check_network_end,  # noqa: F401
                              dev, h_oracle, host)

SENTINEL = -1234.5
NORM_MODES = (E.ACT_NORM, E.ACT_NORM_POOL, E.ACT_NORM_UP)


class Guarded:
    """A contiguous output tensor `t` of `shape` inside a sentinel-filled buffer; `images` is
    the batch size the slack is sized by (one image's elements, at least 256, each side)."""

    def __init__(self, shape, images, dtype=torch.float32):
        n = int(np.prod(shape))
        self.slack = max(256, -(-(n // images) // 64) * 64)
        self.n = n
        self.big = torch.full((n + 2 * self.slack,), SENTINEL, dtype=dtype, device="cuda")
        self.t = self.big[self.slack:self.slack + n].view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def slack_intact(self):
        s = self.slack
        return bool((self.big[:s] == SENTINEL).all()) and bool((self.big[s + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.big == SENTINEL).all())

    def written(self):
        """No element of the output still holds the sentinel."""
        return not bool((self.t == SENTINEL).any())


def p(t):
    """Device pointer of a tensor of any dtype (None -> NULL)."""
    return None if t is None else t.data_ptr()


def run(name, outs, *args, must=False):
    """Right or refused.  True: the call returned 0 and left the slack of every output in
    `outs` intact.  False: it returned nonzero with a message and touched no output (never for
    a must-accept shape)."""
    lib = N.load()
    rc = getattr(lib, name)(*args)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: launch nothing more on this GPU
        pytest.exit(f"device error after {name}: {e}", returncode=3)
    if rc != 0:
        msg = lib.ebsdvae_last_error().decode(errors="replace")
        assert not must, f"{name} refused a must-accept shape ({rc}): {msg}"
        assert msg.strip(), f"{name} returned {rc} without a message"
        for g in outs:
            assert g.untouched(), f"{name} refused ({msg}) but wrote an output"
        return False
    for i, g in enumerate(outs):
        assert g.slack_intact(), f"{name}: output {i} overran its buffer"
    return True


def stream():
    return N.stream()


# ------------------------------------------------------------------------------ inputs
def src_shape(B, H, W, C, mode):
    if mode == E.ACT_NORM_POOL:
        return (B, 2 * H, 2 * W, C)
    if mode in (E.ACT_UP, E.ACT_NORM_UP):
        return (B, H // 2, W // 2, C)
    return (B, H, W, C)


def stats_of(y):
    """(xhat, mean, rstd, st (B, C, 2)) of a pre-norm tensor, float64."""
    xh, mean, rstd = O.instance_norm(y)
    return xh, mean, rstd, np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)


def make_src(rng, B, H, W, C, mode):
    s = rng.standard_normal(src_shape(B, H, W, C, mode)) * 1.5 + 0.3
    _, mean, rstd, st = stats_of(s)
    return s, mean, rstd, st


def prev_shape(B, H, W, C, pmode):
    """y_prev of a fused input gradient at (H, W)."""
    if pmode == E.P_POOL:
        return (B, 2 * H, 2 * W, C)
    if pmode in (E.P_UP, E.P_UPSUM):
        return (B, H // 2, W // 2, C)
    return (B, H, W, C)


def block_grad_oracle(gn, xh, rstd, pmode):
    """gy of a block from the gradient gn of its consumer's input (float64)."""
    if pmode == E.P_POOL:
        ga = O.maxpool2_bwd(gn, O.maxpool2(O.lrelu(xh))[1])
    elif pmode in (E.P_UP, E.P_UPSUM):
        ga = O.upsample2_bwd(gn)
    else:
        ga = gn
    return O.instance_norm_bwd(ga * O.lrelu_slope(xh), xh, rstd)


# ------------------------------------------------------------------------------ weights
def pack(w_d, cin, cout, kind, pieces, dgrad):
    """The layer's packed weight: fp32 (pieces 0) or split pieces, forward or input gradient."""
    if not pieces:
        out = torch.empty(9 * cin * cout, device="cuda")
        N.call("ebsdvae_pack_conv_weight", N.ptr(w_d), N.ptr(out), cin, cout, kind, int(dgrad), stream())
        return out
    ci_, co_ = (cout, cin) if dgrad else (cin, cout)
    out = torch.empty(N.call("ebsdvae_pack_split_bytes", ci_, co_, pieces) // 4, device="cuda")
    d = (N.PackDesc * 1)(N.PackDesc(N.ptr(w_d), N.ptr(out), cin, cout, kind, int(dgrad)))
    N.call("ebsdvae_pack_conv_weights_split", ctypes.addressof(d), 1, pieces, stream())
    return out


def reduce_slices(wpart, bpart, S_, cin, cout, kind):
    """ebsdvae_wgrad_reduce of S_ slices into guarded (dw, db) of the parameter layout."""
    shape = (cout, cin, 3, 3) if kind == 0 else (cin, cout, 3, 3)
    dw, db = Guarded(shape, 1), Guarded((cout,), 1)
    work = torch.empty(N.call("ebsdvae_wgrad_reduce_work", S_, cin, cout) // 8, dtype=torch.float64,
                       device="cuda")
    assert run("ebsdvae_wgrad_reduce", [dw, db], p(wpart), p(bpart), S_, dw.ptr(), db.ptr(), cin, cout,
               kind, p(work), stream(), must=True)
    return dw.t, db.t


def finalize_stats(part, B, C, T, n_per_tile):
    st = Guarded((B, C, 2), B)
    assert run("ebsdvae_in_stats_finalize", [st], p(part), st.ptr(), B, C, T, n_per_tile, stream(),
               must=True)
    return st.t


def finalize_bwd(part, B, C, T, HW):
    bst = Guarded((B, C, 2), B)
    assert run("ebsdvae_in_bwd_finalize", [bst], p(part), bst.ptr(), B, C, T, HW, stream(), must=True)
    return bst.t


def band_max(gy, B, T):
    """max |gy| per row band of T bands per image (NHWC: a band is contiguous)."""
    return gy.abs().reshape(B, T, -1).amax(2)


# ------------------------------------------------------------------------------ network end
class AbiNetEnd:
    """engine.network_end / in_backward_final_from on guarded buffers through the ABI; with
    x_shift the targets sit that many floats past a 16-byte boundary."""

    def __init__(self, mfma, x_shift=0):
        self.name = "ebsdvae_net_end" if mfma else "ebsdvae_net_end_valu"
        self.x_shift = x_shift

    def network_end(self, plan, saved, params, x, g_loss=None, scale=1.0):
        y13, st13 = saved[plan.dec[-1].name]
        Bn, H, W, C = y13.shape
        if self.x_shift:
            buf = torch.empty(x.numel() + 4, device=x.device)
            x = buf[self.x_shift:self.x_shift + x.numel()].view(x.shape).copy_(x)
            assert x.data_ptr() % 16 == 4 * self.x_shift
        T = N.call("ebsdvae_net_end_tiles", H, W)
        assert T > 0
        x_hat, g1, bce = Guarded((Bn, 1, H, W), Bn), Guarded((Bn, H, W), Bn), Guarded((Bn, T), Bn)
        part = Guarded((Bn, T, C, 2), Bn, torch.float64)
        wpart, bpart = Guarded((Bn * T, 9, 1, C), Bn), Guarded((Bn * T,), Bn)
        outs = [x_hat, g1, bce, part, wpart, bpart]
        assert run(self.name, outs, p(y13), p(st13), p(params["decoder.14.weight"]),
                   p(params["decoder.14.bias"]), p(x), p(g_loss), float(scale), x_hat.ptr(), g1.ptr(),
                   bce.ptr(), part.ptr(), wpart.ptr(), bpart.ptr(), Bn, H, W, C, stream(), must=True)
        assert all(g.written() for g in outs)
        return x_hat.t, E.NetEnd(g1.t, part.t, wpart.t, bpart.t, bce.t, T)

    def in_backward_final_from(self, end, w14, y, st, dw14, db14):
        Bn, H, W, C = y.shape
        bst = finalize_bwd(end.part, Bn, C, end.tiles, H * W)
        Tg = N.call("ebsdvae_in_bwd_final_tiles", H, W)
        gy, gmax = Guarded(y.shape, Bn), Guarded((Bn, Tg), Bn)
        assert run("ebsdvae_in_bwd_final_apply_max", [gy, gmax], p(end.g1), p(w14), p(y), p(st), p(bst),
                   gy.ptr(), gmax.ptr(), Bn, H, W, C, stream(), must=True)
        assert torch.equal(gmax.t, band_max(gy.t, Bn, Tg))
        gy2 = Guarded(y.shape, Bn)   # the form without the maxima: the same gradient
        assert run("ebsdvae_in_bwd_final_apply", [gy2], p(end.g1), p(w14), p(y), p(st), p(bst), gy2.ptr(),
                   Bn, H, W, C, stream(), must=True)
        assert torch.equal(gy.t, gy2.t)
        dw, db = reduce_slices(end.wpart, end.bpart, Bn * end.tiles, C, 1, E.KIND_CONV)
        dw14.copy_(dw)
        db14.copy_(db)
        return gy.t
