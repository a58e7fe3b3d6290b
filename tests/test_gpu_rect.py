"""Rectangular (H != W) maps through the C ABI (include/ebsdvae.h).

The engine and the rest of the suite drive every kernel with H == W; the header declares H and
W separately and the host planners accept rectangles.  Every case here is right or refused
(tests/rect_util.py: `run`): the entry point returns 0 and meets the gate of the square test of
the same entry point (tests/test_gpu_kernels.py, imported, not copied), or it returns nonzero
with a message and leaves every output untouched.  must=True marks the shapes the host queries
accept (re-run on the CPU: the lists below are their answers).  B = 3 throughout (partial
multi-image tiles, a last partly filled tile), both orientations of every shape, and every
output sits between sentinel-filled guard bands of at least one image.

What only these shapes reach: the 32-row bands of ebsdvae_net_end / _net_end_valu (H % 64 != 0:
four kernels), the one-launch ebsdvae_correct_patterns kernel on windows with a side longer
than 128, and row-band counts of the InstanceNorm backward that are no power of two."""
import functools

import numpy as np
import pytest
import torch

import correction_ref as R
import rect_util as U
from latice import _native as N
from latice import engine as E
from latice.data_module import PatternCorrection, correct_patterns
from oracle import vae_oracle as O
from rect_util import AbiNetEnd, Guarded, dev, host, p, run
from test_gpu_pattern_correction import GATE, THREE_PAIRS, _correction

pytestmark = pytest.mark.gpu

B = 3
F16 = E.PIECES_F16
PRECS = ["f16x3", "bf16x3", "bf16x6"]
RECT = [(16, 32), (32, 16)]
LONG = [(16, 64), (64, 16)]


def both(a, b):
    return [(a, b), (b, a)]


def _frozen(*arrays):
    """References are computed once per case and shared between the precisions: read-only."""
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


# ============================================================== 7. network ends
# (32,128), (96,128), (32,256): 32-row bands (1, 3, 1 per image); (64,128): one 64-row band
@pytest.mark.parametrize("mfma", [True, False], ids=["mfma", "valu"])
@pytest.mark.parametrize("H,W", [(32, 128), (96, 128), (64, 128), (32, 256)])
def test_network_end_rect(cuda, H, W, mfma):
    """The body of test_network_end_matches_oracle (its asserts and gates) at H != W, on guarded
    buffers; then the apply pass with its per-band maxima and the slice reduce."""
    U.check_network_end(H, W, ops=AbiNetEnd(mfma))


@pytest.mark.parametrize("mfma", [True, False], ids=["mfma", "valu"])
@pytest.mark.parametrize("with_b14,with_g_loss", [(False, True), (True, False)], ids=["no-b14", "no-g_loss"])
def test_network_end_rect_null_bias_and_loss_gradient(cuda, mfma, with_b14, with_g_loss):
    """b14 = NULL (bias 0) and g_loss = NULL (loss gradient 1), as the header documents, on the
    three 32-row bands of (96, 128)."""
    U.check_network_end(96, 128, ops=AbiNetEnd(mfma), with_b14=with_b14, with_g_loss=with_g_loss)


@pytest.mark.parametrize("name", ["ebsdvae_net_end", "ebsdvae_net_end_valu"])
def test_network_end_refuses_width_64(cuda, name):
    H, W, C = 128, 64, 32
    assert N.call("ebsdvae_net_end_tiles", H, W) == -1
    y, st = dev(np.zeros((B, H, W, C))), dev(np.ones((B, C, 2)))
    w14, x = dev(np.zeros((1, C, 3, 3))), dev(np.zeros((B, 1, H, W)))
    outs = [Guarded((B, 1, H, W), B), Guarded((B, H, W), B), Guarded((B, 2), B),
            Guarded((B, 2, C, 2), B, torch.float64), Guarded((B * 2, 9, 1, C), B), Guarded((B * 2,), B)]
    assert not run(name, outs, p(y), p(st), p(w14), None, p(x), None, 1.0, *[g.ptr() for g in outs],
                   B, H, W, C, U.stream())


@pytest.mark.parametrize("H,W", [(32, 64), (64, 32), (32, 128)])
def test_first_block_rect(cuda, H, W):
    """ebsdvae_conv_first_fwd and _conv_first_stats against the oracle (the gates of
    test_first_conv_valu_and_recomputed_backward and test_first_conv_stats_from_moments), then
    the first block's backward in its four forms: the recomputing (_rc) forms bitwise equal to
    the reading ones, all against the oracle's weight gradient."""
    rng = np.random.default_rng(23 + H + 2 * W)
    C = 32
    x = np.floor(rng.random((B, 1, H, W)) * 255) / 255
    w = rng.standard_normal((C, 1, 3, 3)) / 3.0
    b = rng.standard_normal(C) * 0.1
    xd, wd, bd = dev(x), dev(w), dev(b)
    xn = x.transpose(0, 2, 3, 1)
    ref = O.conv3x3(xn, w, b)
    xh, rm, rr = O.instance_norm(ref)
    # the moment-based statistics
    stm = Guarded((B, C, 2), B)
    if run("ebsdvae_conv_first_stats", [stm], p(xd), p(wd), p(bd), stm.ptr(), B, H, W, C, U.stream()):
        got = host(stm.t)
        assert O.rel_err(got[..., 0], rm[:, 0, 0, :]) < 1e-6
        assert O.rel_err(got[..., 1], rr[:, 0, 0, :]) < 1e-6
    T = N.call("ebsdvae_conv_first_stat_tiles", H, W)
    y, part = Guarded((B, H, W, C), B), Guarded((B, max(T, 1), C, 2), B)
    if not run("ebsdvae_conv_first_fwd", [y, part], p(xd), p(wd), p(bd), y.ptr(), part.ptr(), B, H, W, C,
               U.stream(), must=T > 0):
        return
    assert T > 0
    assert O.rel_err(host(y.t), ref) < 1e-6
    st = U.finalize_stats(part.t, B, C, T, H * W // T)
    got = host(st)
    assert O.rel_err(got[..., 0], rm[:, 0, 0, :]) < 1e-5
    assert O.rel_err(got[..., 1], rr[:, 0, 0, :]) < 1e-5
    # backward: reduce, finalize, then the fused apply + weight gradient
    gn = rng.standard_normal((B, H, W, C))
    gd = dev(gn)
    Tr = N.call("ebsdvae_in_bwd_tiles", H, W, C)
    rp = Guarded((B, Tr, C, 2), B, torch.float64)
    assert run("ebsdvae_in_bwd_reduce", [rp], p(gd), E.P_ID, y.ptr(), p(st), rp.ptr(), B, H, W, C,
               U.stream(), must=True)
    bst = U.finalize_bwd(rp.t, B, C, Tr, H * W)
    # h = g * lrelu'(xhat) as a fused input gradient writes it, with the device's own xhat
    xh_d = (y.t - st[:, None, None, :, 0]) * st[:, None, None, :, 1]
    hd = (gd * torch.where(xh_d > 0, 1.0, O.LRELU_SLOPE)).float().contiguous()
    S_ = B * Tr
    res = {}
    for name, first, second in [("ebsdvae_in_bwd_first_apply_wgrad", gd, (y.t,)),
                                ("ebsdvae_in_bwd_first_apply_wgrad_rc", gd, (wd, bd)),
                                ("ebsdvae_in_bwd_first_happly_wgrad", hd, (y.t,)),
                                ("ebsdvae_in_bwd_first_happly_wgrad_rc", hd, (wd, bd))]:
        wp_, bp_ = Guarded((S_, 9, C, 1), B), Guarded((S_, C), B)
        if run(name, [wp_, bp_], p(first), *[p(t) for t in second], p(st), p(bst), p(xd), wp_.ptr(),
               bp_.ptr(), B, H, W, C, U.stream()):
            assert wp_.written() and bp_.written()
            res[name] = (wp_.t, bp_.t)
    assert len(res) in (0, 4), sorted(res)   # the four forms share one guard
    if not res:
        return
    for base in ("ebsdvae_in_bwd_first_apply_wgrad", "ebsdvae_in_bwd_first_happly_wgrad"):
        assert torch.equal(res[base][0], res[base + "_rc"][0])
        assert torch.equal(res[base][1], res[base + "_rc"][1])
    gy = O.instance_norm_bwd(gn * O.lrelu_slope(xh), xh, rr)
    rw, rb = O.conv3x3_wgrad(xn, gy)
    l1 = np.abs(gy).sum(axis=(0, 1, 2))
    for name, (wp_, bp_) in res.items():
        dw, db = U.reduce_slices(wp_, bp_, S_, 1, C, E.KIND_CONV)
        print(f"\n{name} {H}x{W}: dW {O.rel_err(host(dw), rw):.2e}")
        assert O.rel_err(host(dw), rw) < 1e-4, name
        assert (np.abs(host(db) - rb) <= 2e-8 * l1).all(), name


# (4, 32): two whole images per 256-pixel tile (edge_geom), the third alone in the last tile
@pytest.mark.parametrize("H,W", [(16, 128), (128, 16), (4, 32)])
def test_cout1_conv_rect(cuda, H, W):
    rng = np.random.default_rng(9 + H + 2 * W)
    C = 32
    s, mean, rstd, st = U.make_src(rng, B, H, W, C, E.ACT_NORM)
    w = rng.standard_normal((1, C, 3, 3)) * 0.1
    bias = np.array([0.3])
    ds, dst, dw, db = dev(s), dev(st), dev(w), dev(bias)
    out = Guarded((B, 1, H, W), B)
    if run("ebsdvae_conv3x3_cout1_fwd", [out], p(ds), p(dst), E.ACT_NORM, p(dw), p(db), out.ptr(), 0, B, H, W,
           C, U.stream()):
        a = U.act_oracle(s, mean, rstd, E.ACT_NORM)
        assert O.rel_err(host(out.t)[:, 0], O.conv3x3(a, w, bias)[..., 0]) < U.TOL
    g = rng.standard_normal((B, H, W))
    dg = dev(g)
    gin = Guarded((B, H, W, C), B)
    if run("ebsdvae_conv3x3_cout1_dgrad", [gin], p(dg), p(dw), gin.ptr(), B, H, W, C, U.stream()):
        assert O.rel_err(host(gin.t), O.conv3x3_dgrad(g[..., None], w)) < U.TOL
    # the first conv's input gradient: flipped taps over a RAW source, no bias
    w0 = rng.standard_normal((C, 1, 3, 3)) * 0.2
    gy = rng.standard_normal((B, H, W, C))
    dgy, dw0 = dev(gy), dev(w0)
    gx = Guarded((B, 1, H, W), B)
    if run("ebsdvae_conv3x3_cout1_fwd", [gx], p(dgy), None, E.ACT_RAW, p(dw0), None, gx.ptr(), 1, B, H, W, C,
           U.stream()):
        assert O.rel_err(host(gx.t)[:, 0], O.conv3x3_dgrad(gy, w0)[..., 0]) < U.TOL


# ============================================================== 6. InstanceNorm backward, generic
# (24, 128) and (96, 128): 3 and 12 reduce bands, 12 and 48 apply bands at B = 3
IN_BWD = [(H, W, C) for C in (32, 128) for H, W in LONG] + [(24, 128, 32), (96, 128, 32)]


@pytest.mark.parametrize("pmode", [E.P_ID, E.P_POOL, E.P_UP], ids=["id", "pool", "up"])
@pytest.mark.parametrize("H,W,C", IN_BWD)
def test_instance_norm_backward_rect(cuda, H, W, C, pmode):
    """reduce -> finalize -> apply[_max] / happly against instance_norm_bwd at the gate of
    test_instance_norm_backward; gmax is the per-band max |gy|, exactly."""
    rng = np.random.default_rng(3 + pmode + H + 2 * W + C)
    y = rng.standard_normal((B, H, W, C)) * 2 + 0.5
    xh, mean, rstd, st = U.stats_of(y)
    gshape = {E.P_ID: (B, H, W, C), E.P_POOL: (B, H // 2, W // 2, C), E.P_UP: (B, 2 * H, 2 * W, C)}[pmode]
    gn = rng.standard_normal(gshape)
    yd, sd, gd = dev(y), dev(st), dev(gn)
    T = N.call("ebsdvae_in_bwd_tiles", H, W, C)
    Tg = N.call("ebsdvae_in_bwd_apply_tiles", B, H, W, C)
    assert T > 0 and Tg > 0
    if (H, W) == (24, 128):
        assert (T, Tg) == (3, 12)
    if (H, W) == (96, 128):
        assert (T, Tg) == (12, 48)
    part = Guarded((B, T, C, 2), B, torch.float64)
    assert run("ebsdvae_in_bwd_reduce", [part], p(gd), pmode, p(yd), p(sd), part.ptr(), B, H, W, C,
               U.stream(), must=True)
    assert part.written()
    bst = U.finalize_bwd(part.t, B, C, T, H * W)
    ref = U.block_grad_oracle(gn, xh, rstd, pmode)
    gy, gmax = Guarded(y.shape, B), Guarded((B, Tg), B)
    assert run("ebsdvae_in_bwd_apply_max", [gy, gmax], p(gd), pmode, p(yd), p(sd), p(bst), gy.ptr(),
               gmax.ptr(), B, H, W, C, U.stream(), must=True)
    print(f"\nin_bwd {H}x{W} C {C} pmode {pmode}: gy {O.rel_err(host(gy.t), ref):.2e}")
    assert O.rel_err(host(gy.t), ref) < 1e-4
    assert torch.equal(gmax.t, U.band_max(gy.t, B, Tg))
    # gmax = NULL, and the form without the argument: the same gradient
    for name, extra in (("ebsdvae_in_bwd_apply_max", (None,)), ("ebsdvae_in_bwd_apply", ())):
        g2 = Guarded(y.shape, B)
        assert run(name, [g2], p(gd), pmode, p(yd), p(sd), p(bst), g2.ptr(), *extra, B, H, W, C, U.stream(),
                   must=True)
        assert torch.equal(g2.t, gy.t), name
    # happly: h = g * lrelu'(xhat) at the routed pixel, from the device's own xhat
    xh_d = (yd - sd[:, None, None, :, 0]) * sd[:, None, None, :, 1]
    if pmode == E.P_POOL:
        a_d = torch.where(xh_d > 0, xh_d, O.LRELU_SLOPE * xh_d)
        def windows(t):   # (B, H/2, W/2, 4, C), window order (0,0), (0,1), (1,0), (1,1)
            t = t.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5)
            return t.reshape(B, H // 2, W // 2, 4, C)
        win, xwin = windows(a_d), windows(xh_d)
        # the first maximum of lrelu(xhat) in window order, as the kernel takes it
        slot = torch.arange(4, device=win.device).view(1, 1, 1, 4, 1)
        arg = torch.where(win == win.amax(3, keepdim=True), slot, 4).amin(3, keepdim=True)
        xsel = torch.gather(xwin, 3, arg)[:, :, :, 0]
    elif pmode == E.P_UP:
        xsel = xh_d.repeat_interleave(2, 1).repeat_interleave(2, 2)
    else:
        xsel = xh_d
    hd = (gd * torch.where(xsel > 0, 1.0, O.LRELU_SLOPE)).float().contiguous()
    g3, gm3 = Guarded(y.shape, B), Guarded((B, Tg), B)
    assert run("ebsdvae_in_bwd_happly", [g3, gm3], p(hd), pmode, p(yd), p(sd), p(bst), g3.ptr(), gm3.ptr(),
               B, H, W, C, U.stream(), must=True)
    assert O.rel_err(host(g3.t), ref) < 1e-4
    assert torch.equal(gm3.t, U.band_max(g3.t, B, Tg))


@pytest.mark.parametrize("H,W", LONG + [(24, 128)])
def test_act_apply_and_upsample_bwd_rect(cuda, H, W):
    rng = np.random.default_rng(5 + H + 2 * W)
    C = 32
    for mode in (E.ACT_NORM, E.ACT_NORM_POOL, E.ACT_NORM_UP, E.ACT_UP):
        s, mean, rstd, st = U.make_src(rng, B, H, W, C, mode)
        ds, dst = dev(s), dev(st)
        out = Guarded((B, H, W, C), B)
        assert run("ebsdvae_act_apply", [out], p(ds), p(dst), mode, out.ptr(), B, H, W, C, U.stream(),
                   must=True)
        assert O.rel_err(host(out.t), U.act_oracle(s, mean, rstd, mode)) < 1e-5, mode
    g = rng.standard_normal((B, 2 * H, 2 * W, C))
    dg = dev(g)
    o2 = Guarded((B, H, W, C), B)
    assert run("ebsdvae_upsample2_bwd", [o2], p(dg), o2.ptr(), B, H, W, C, U.stream(), must=True)
    assert O.rel_err(host(o2.t), O.upsample2_bwd(g)) < 1e-6


# ============================================================== 4. fp32 MFMA conv
# (cin, cout, mode, bias, act_out)
FP32_FWD = [(32, 32, E.ACT_NORM, True, False), (32, 64, E.ACT_NORM_POOL, True, True),
            (64, 128, E.ACT_NORM_UP, False, False), (128, 64, E.ACT_UP, True, False),
            (1, 32, E.ACT_RAW, True, False), (64, 32, E.ACT_RAW, True, True)]


@pytest.mark.parametrize("cin,cout,mode,with_bias,keep", FP32_FWD)
@pytest.mark.parametrize("H,W", RECT)
def test_conv3x3_fwd_fp32_rect(cuda, H, W, cin, cout, mode, with_bias, keep):
    rng = np.random.default_rng(cin * 1000 + cout + H + 2 * W + mode)
    s, mean, rstd, st = U.make_src(rng, B, H, W, cin, mode)
    w = rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)
    b = rng.standard_normal(cout) * 0.1 if with_bias else np.zeros(cout)
    ds, dst, dw, db = dev(s), dev(st), dev(w), dev(b)
    wp = U.pack(dw, cin, cout, 0, 0, False)
    T = N.call("ebsdvae_conv3x3_stat_tiles", H, W, cout)
    y, part = Guarded((B, H, W, cout), B), Guarded((B, T, cout, 2), B)
    act = Guarded((B, H, W, cin), B) if keep else None
    outs = [y, part] + ([act] if keep else [])
    assert run("ebsdvae_conv3x3_fwd", outs, p(ds), p(dst) if mode in U.NORM_MODES else None, mode, p(wp),
               p(db) if with_bias else None, y.ptr(), part.ptr(), act.ptr() if keep else None, B, H, W, cin,
               cout, U.stream(), must=True)
    a_ref = U.act_oracle(s, mean, rstd, mode)   # cin = 1: (B, 1, H, W) is (B, H, W, 1)
    ref = O.conv3x3(a_ref, w, b)
    print(f"\nconv3x3_fwd fp32 {cin}->{cout} {H}x{W} mode {mode}: y {O.rel_err(host(y.t), ref):.2e}")
    assert O.rel_err(host(y.t), ref) < U.TOL
    if keep:
        assert O.rel_err(host(act.t), a_ref) < 1e-6
    stt = host(U.finalize_stats(part.t, B, cout, T, H * W // T))
    _, rm, rr = O.instance_norm(ref)
    assert O.rel_err(stt[..., 0], rm[:, 0, 0, :]) < 1e-5
    assert O.rel_err(stt[..., 1], rr[:, 0, 0, :]) < 1e-4


@pytest.mark.parametrize("cin,cout,pmode", [(32, 32, E.P_ID), (32, 64, E.P_POOL), (128, 128, E.P_UP),
                                            (64, 32, E.P_UP), (128, 64, E.P_ID)])
@pytest.mark.parametrize("H,W", RECT)
def test_dgrad_inbwd_fp32_rect(cuda, H, W, cin, cout, pmode):
    """ebsdvae_conv3x3_dgrad_inbwd: h against h_oracle, then finalize + happly against the
    block's gradient (the gates of test_dgrad_fused_instance_norm_backward)."""
    rng = np.random.default_rng(5 + cin + cout + H + 2 * W + pmode)
    y = rng.standard_normal(U.prev_shape(B, H, W, cin, pmode)) * 2 + 0.5
    xh, mean, rstd, st = U.stats_of(y)
    gy = rng.standard_normal((B, H, W, cout))
    w = rng.standard_normal((cout, cin, 3, 3)) * 0.1
    yd, sd, gd, wd = dev(y), dev(st), dev(gy), dev(w)
    wpk = U.pack(wd, cin, cout, 0, 0, True)
    T = N.call("ebsdvae_conv3x3_stat_tiles", H, W, cin)
    gin, part = Guarded((B, H, W, cin), B), Guarded((B, T, cin, 2), B, torch.float64)
    assert run("ebsdvae_conv3x3_dgrad_inbwd", [gin, part], p(gd), p(wpk), gin.ptr(), p(yd), p(sd), pmode,
               part.ptr(), B, H, W, cout, cin, U.stream(), must=True)
    gn = O.conv3x3_dgrad(gy, w)
    e_h = O.rel_err(host(gin.t), U.h_oracle(gn, xh, pmode))
    print(f"\ndgrad_inbwd fp32 {cout}->{cin} {H}x{W} pmode {pmode}: h {e_h:.2e}")
    assert e_h < U.TOL
    _check_happly(gin.t, part.t, T, yd, sd, pmode, U.block_grad_oracle(gn, xh, rstd, pmode), 1e-4)


def _check_happly(h, part, T, yd, sd, pmode, ref, gate, per_image=False):
    """finalize the fused reduce's sums and apply them: the block's gradient vs the oracle."""
    Bn, Hp, Wp, C = yd.shape
    bst = U.finalize_bwd(part, Bn, C, T, Hp * Wp)
    Tg = N.call("ebsdvae_in_bwd_apply_tiles", Bn, Hp, Wp, C)
    gy, gmax = Guarded(yd.shape, Bn), Guarded((Bn, Tg), Bn)
    assert run("ebsdvae_in_bwd_happly", [gy, gmax], p(h), E.P_ID if pmode == E.P_UPSUM else pmode, p(yd),
               p(sd), p(bst), gy.ptr(), gmax.ptr(), Bn, Hp, Wp, C, U.stream(), must=True)
    got = host(gy.t)
    errs = [O.rel_err(got[b], ref[b]) for b in range(Bn)] if per_image else [O.rel_err(got, ref)]
    print(f"happly {Hp}x{Wp} C {C} pmode {pmode}: block gradient {max(errs):.2e}")
    assert max(errs) < gate, errs
    assert torch.equal(gmax.t, U.band_max(gy.t, Bn, Tg))
    return bst


# ============================================================== 1. split conv forward
PAIR_MODE = [(32, 32, E.ACT_NORM), (32, 64, E.ACT_NORM_POOL), (64, 128, E.ACT_RAW), (128, 128, E.ACT_UP),
             (128, 64, E.ACT_NORM_UP), (64, 32, E.ACT_NORM)]
# (H, W, cin, cout, mode, must): the host queries accept every must case in all three precisions
SPLIT_FWD = ([(H, W, ci, co, m, True) for H, W in RECT for ci, co, m in PAIR_MODE]
             + [(H, W, ci, co, m, True) for H, W in LONG
                for ci, co, m in [(32, 32, E.ACT_NORM), (128, 128, E.ACT_NORM_POOL)]]
             # bf16x6 refuses 128 -> 128 at (32, 128) and takes it at (128, 32)
             + [(H, W, 128, 128, E.ACT_NORM, False) for H, W in both(32, 128)]
             # W or H of 8: cout = 128 only, not in bf16x3... as the planner answers
             + [(H, W, 128, 128, E.ACT_NORM_UP, False) for H, W in both(8, 32)]
             # 64-pixel maps that are not 8 x 8
             + [(H, W, 128, 128, E.ACT_NORM_POOL, False) for H, W in both(4, 16)])


@functools.lru_cache(maxsize=None)
def _split_fwd_case(H, W, cin, cout, mode):
    rng = np.random.default_rng(31 + cin + cout + H + 2 * W + mode)
    s, mean, rstd, st = U.make_src(rng, B, H, W, cin, mode)
    w = rng.standard_normal((cout, cin, 3, 3)) * 0.1
    b = rng.standard_normal(cout) * 0.1
    return _frozen(s, st, w, b, O.conv3x3(U.act_oracle(s, mean, rstd, mode), w, b))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("H,W,cin,cout,mode,must", SPLIT_FWD)
def test_conv3x3_fwd_split_rect(cuda, H, W, cin, cout, mode, must, prec):
    """ebsdvae_conv3x3_fwd_split_st against the oracle (SPLIT_TOL, the statistics at the gates of
    the square tests) and bitwise against _fwd_split + in_stats_finalize; on ACT_NORM sources
    that allow it, the pooled producer: y unchanged, ypool the exact 2x2 max, _fwd_split_pooled
    + finalize bitwise, and y = NULL leaving ypool and the statistics as they are."""
    pieces = U.FWD_PIECES[prec]
    ok = N.call("ebsdvae_conv3x3_split_supported", H, W, cin, cout, pieces)
    assert ok or not must
    s, st, w, b, ref = _split_fwd_case(H, W, cin, cout, mode)
    ds, dw, db = dev(s), dev(w), dev(b)
    dst = dev(st) if mode in U.NORM_MODES else None
    wp = U.pack(dw, cin, cout, 0, pieces, False)
    T = max(N.call("ebsdvae_conv3x3_split_stat_tiles", H, W, cout), 1)
    y, part, stt = Guarded((B, H, W, cout), B), Guarded((B, T, cout, 2), B), Guarded((B, cout, 2), B)
    if not run("ebsdvae_conv3x3_fwd_split_st", [y, part, stt], p(ds), p(dst), mode, p(wp), p(db), y.ptr(), None,
               part.ptr(), stt.ptr(), B, H, W, cin, cout, pieces, U.stream(), must=must):
        assert not ok   # the query and the entry point agree
        y2, part2 = Guarded((B, H, W, cout), B), Guarded((B, T, cout, 2), B)
        assert not run("ebsdvae_conv3x3_fwd_split", [y2, part2], p(ds), p(dst), mode, p(wp), p(db), y2.ptr(),
                       part2.ptr(), None, B, H, W, cin, cout, pieces, U.stream())
        return
    assert ok
    assert y.written() and stt.written()
    err = O.rel_err(host(y.t), ref)
    print(f"\nfwd_split {prec} {cin}->{cout} {H}x{W} mode {mode}: y {err:.2e}")
    assert err < U.SPLIT_TOL[prec]
    _, rm, rr = O.instance_norm(ref)
    assert O.rel_err(host(stt.t)[..., 0], rm[:, 0, 0, :]) < 1e-4
    assert O.rel_err(host(stt.t)[..., 1], rr[:, 0, 0, :]) < 1e-4
    # the two-launch form, bit for bit
    y2, part2 = Guarded((B, H, W, cout), B), Guarded((B, T, cout, 2), B)
    assert run("ebsdvae_conv3x3_fwd_split", [y2, part2], p(ds), p(dst), mode, p(wp), p(db), y2.ptr(),
               part2.ptr(), None, B, H, W, cin, cout, pieces, U.stream(), must=True)
    st2 = U.finalize_stats(part2.t, B, cout, T, H * W // T)
    assert torch.equal(y.t, y2.t) and torch.equal(stt.t, st2)
    if mode != E.ACT_NORM:
        return
    pool_ok = N.call("ebsdvae_conv3x3_split_pool_ok", H, W, cin, cout, pieces)
    y3, yp, part3, st3 = (Guarded((B, H, W, cout), B), Guarded((B, H // 2, W // 2, cout), B),
                          Guarded((B, T, cout, 2), B), Guarded((B, cout, 2), B))
    if not run("ebsdvae_conv3x3_fwd_split_st", [y3, yp, part3, st3], p(ds), p(dst), mode, p(wp), p(db),
               y3.ptr(), yp.ptr(), part3.ptr(), st3.ptr(), B, H, W, cin, cout, pieces, U.stream(),
               must=must and bool(pool_ok)):
        assert not pool_ok
        return
    assert pool_ok
    assert torch.equal(y3.t, y.t)
    ref_pool = torch.nn.functional.max_pool2d(y3.t.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.equal(yp.t, ref_pool.contiguous())
    assert O.rel_err(host(st3.t), host(stt.t)) < 1e-5
    y4, yp4 = Guarded((B, H, W, cout), B), Guarded((B, H // 2, W // 2, cout), B)
    part4 = Guarded((B, T, cout, 2), B)
    assert run("ebsdvae_conv3x3_fwd_split_pooled", [y4, yp4, part4], p(ds), p(dst), mode, p(wp), p(db),
               y4.ptr(), yp4.ptr(), part4.ptr(), B, H, W, cin, cout, pieces, U.stream(), must=True)
    st4 = U.finalize_stats(part4.t, B, cout, T, H * W // T)
    assert torch.equal(y4.t, y3.t) and torch.equal(yp4.t, yp.t) and torch.equal(st4, st3.t)
    yp5, part5 = Guarded((B, H // 2, W // 2, cout), B), Guarded((B, T, cout, 2), B)
    st5 = Guarded((B, cout, 2), B)
    assert run("ebsdvae_conv3x3_fwd_split_st", [yp5, part5, st5], p(ds), p(dst), mode, p(wp), p(db), None,
               yp5.ptr(), part5.ptr(), st5.ptr(), B, H, W, cin, cout, pieces, U.stream(), must=True)
    assert torch.equal(yp5.t, yp.t) and torch.equal(st5.t, st3.t)


# ============================================================== 2. the fused first block
@pytest.mark.parametrize("with_b0,pooled", [(True, False), (True, True), (False, False)],
                         ids=["plain", "pooled", "no-b0"])
@pytest.mark.parametrize("H,W", RECT)
def test_fwd_split_first_rect(cuda, H, W, with_b0, pooled):
    """ebsdvae_conv3x3_fwd_split_first == conv_first_fwd + in_stats_finalize + _fwd_split_st bit
    for bit, and against the oracle."""
    C = 32
    assert N.call("ebsdvae_conv3x3_fwd_split_first_ok", H, W, C, C, F16) == 1
    rng = np.random.default_rng(71 + H + 2 * W)
    x = np.floor(rng.random((B, 1, H, W)) * 255) / 255
    w0 = rng.standard_normal((C, 1, 3, 3)) / 3.0
    b0 = rng.standard_normal(C) * 0.1 if with_b0 else np.zeros(C)
    w = rng.standard_normal((C, C, 3, 3)) * 0.1
    b = rng.standard_normal(C) * 0.1
    xd, w0d, wd, bd = dev(x), dev(w0), dev(w), dev(b)
    b0d = dev(b0) if with_b0 else None
    wp = U.pack(wd, C, C, 0, F16, False)
    T0 = N.call("ebsdvae_conv_first_stat_tiles", H, W)
    assert T0 > 0
    y0, part0 = Guarded((B, H, W, C), B), Guarded((B, T0, C, 2), B)
    assert run("ebsdvae_conv_first_fwd", [y0, part0], p(xd), p(w0d), p(b0d), y0.ptr(), part0.ptr(), B, H, W,
               C, U.stream(), must=True)
    st0 = U.finalize_stats(part0.t, B, C, T0, H * W // T0)
    T = N.call("ebsdvae_conv3x3_split_stat_tiles", H, W, C)
    shp = (B, H // 2, W // 2, C)
    outs = {}
    for fused in (True, False):
        y, part, st = Guarded((B, H, W, C), B), Guarded((B, T, C, 2), B), Guarded((B, C, 2), B)
        yp = Guarded(shp, B) if pooled else None
        lst = [y, part, st] + ([yp] if pooled else [])
        if fused:
            assert run("ebsdvae_conv3x3_fwd_split_first", lst, p(xd), p(st0), p(w0d), p(b0d), p(wp), p(bd),
                       y.ptr(), yp.ptr() if pooled else None, part.ptr(), st.ptr(), B, H, W, C, C, F16,
                       U.stream(), must=True)
        else:
            assert run("ebsdvae_conv3x3_fwd_split_st", lst, y0.ptr(), p(st0), E.ACT_NORM, p(wp), p(bd),
                       y.ptr(), yp.ptr() if pooled else None, part.ptr(), st.ptr(), B, H, W, C, C, F16,
                       U.stream(), must=True)
        outs[fused] = (y.t, st.t) + ((yp.t,) if pooled else ())
    for a, b_ in zip(outs[True], outs[False]):
        assert torch.equal(a, b_)
    a0 = O.lrelu(O.instance_norm(O.conv3x3(x.transpose(0, 2, 3, 1), w0, b0))[0])
    ref = O.conv3x3(a0, w, b)
    print(f"\nfwd_split_first {H}x{W}: y {O.rel_err(host(outs[True][0]), ref):.2e}")
    assert O.rel_err(host(outs[True][0]), ref) < U.SPLIT_TOL["f16x3"]
    _, rm, rr = O.instance_norm(ref)
    assert O.rel_err(host(outs[True][1])[..., 0], rm[:, 0, 0, :]) < 1e-4


# ============================================================== 3. split input gradient
# (layer cin, layer cout, pmode of the block feeding the layer)
DGRAD = [(128, 64, -1), (32, 32, E.P_ID), (32, 64, E.P_POOL), (128, 128, E.P_UP), (64, 32, E.P_UPSUM)]


@functools.lru_cache(maxsize=None)
def _dgrad_case(H, W, cin, cout, pmode):
    """(gy, w, conv input gradient, y_prev, h, the previous block's gradient); image 1 of gy is
    1e3 larger than the others."""
    rng = np.random.default_rng(41 + cin + cout + H + 2 * W + pmode)
    gy = rng.standard_normal((B, H, W, cout))
    gy[1] *= 1e3
    w = rng.standard_normal((cout, cin, 3, 3)) * 0.1
    gn = O.conv3x3_dgrad(gy, w)
    if pmode < 0:
        return _frozen(gy, w, gn, None, None, None)
    y = rng.standard_normal(U.prev_shape(B, H, W, cin, pmode)) * 2 + 0.5
    xh, mean, rstd, st = U.stats_of(y)
    hn = U.h_oracle(gn, xh, E.P_UP if pmode == E.P_UPSUM else pmode, summed=pmode == E.P_UPSUM)
    return _frozen(gy, w, gn, y, hn, U.block_grad_oracle(gn, xh, rstd, pmode))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cin,cout,pmode", DGRAD, ids=["plain", "id", "pool", "up", "upsum"])
@pytest.mark.parametrize("H,W", RECT + LONG)
def test_dgrad_split_rect(cuda, H, W, cin, cout, pmode, prec):
    """ebsdvae_conv3x3_dgrad_inbwd_split (bf16 pieces) and _f16 / _f16_bst (per-image gmax); one
    image is 1e3 larger than the others.  gin against h_oracle at SPLIT_TOL, the block's gradient
    through finalize + happly at the 2e-4 of the square tests, _bst bitwise equal to the two
    launches."""
    f16 = prec == "f16x3"
    pieces = F16 if f16 else U.FWD_PIECES[prec]
    # every shape / pair here is accepted by the planner (channels swapped: the conv runs cout -> cin)
    assert N.call("ebsdvae_conv3x3_split_supported", H, W, cout, cin, pieces) == 1
    if pmode == E.P_UPSUM:
        assert N.call("ebsdvae_conv3x3_split_pool_ok", H, W, cout, cin, pieces) == 1
    gy, w, gn, y, hn, ref = _dgrad_case(H, W, cin, cout, pmode)
    gd, wd = dev(gy), dev(w)
    wpk = U.pack(wd, cin, cout, 0, pieces, True)
    gmax = dev(np.abs(gy).reshape(B, -1).max(1, keepdims=True))
    oshape = (B, H // 2, W // 2, cin) if pmode == E.P_UPSUM else (B, H, W, cin)

    def launch(name, gin, part, bst=None, yd=None, sd=None, hw=0):
        outs = [gin] + ([part] if part else []) + ([bst] if bst else [])
        pm = (p(yd), p(sd), pmode, part.ptr() if part else None)
        if name == "ebsdvae_conv3x3_dgrad_inbwd_split":
            return run(name, outs, p(gd), p(wpk), gin.ptr(), *pm, B, H, W, cout, cin, pieces, U.stream(),
                       must=True)
        if name == "ebsdvae_conv3x3_dgrad_inbwd_f16":
            return run(name, outs, p(gd), p(gmax), 1, p(wpk), gin.ptr(), *pm, B, H, W, cout, cin, U.stream(),
                       must=True)
        return run(name, outs, p(gd), p(gmax), 1, p(wpk), gin.ptr(), *pm, bst.ptr(), hw, B, H, W, cout, cin,
                   U.stream(), must=True)

    base = "ebsdvae_conv3x3_dgrad_inbwd_f16" if f16 else "ebsdvae_conv3x3_dgrad_inbwd_split"
    gin = Guarded(oshape, B)
    if pmode < 0:
        assert launch(base, gin, None)
        got = host(gin.t)
        errs = [O.rel_err(got[b], gn[b]) for b in range(B)]
        print(f"\ndgrad_split {prec} {cout}->{cin} {H}x{W} plain: g {max(errs):.2e}")
        assert max(errs) < U.SPLIT_TOL[prec], errs
        return
    yd, sd = dev(y), dev(U.stats_of(y)[3])
    T = N.call("ebsdvae_conv3x3_split_stat_tiles", H, W, cin)
    part = Guarded((B, T, cin, 2), B, torch.float64)
    assert launch(base, gin, part, yd=yd, sd=sd)
    got = host(gin.t)
    errs = [O.rel_err(got[b], hn[b]) for b in range(B)]   # per image: one is 1e3 larger
    print(f"\ndgrad_split {prec} {cout}->{cin} {H}x{W} pmode {pmode}: h {max(errs):.2e}")
    assert max(errs) < U.SPLIT_TOL[prec], errs
    bst = _check_happly(gin.t, part.t, T, yd, sd, pmode, ref, 2e-4, per_image=True)
    if f16:
        gin2, part2 = Guarded(oshape, B), Guarded((B, T, cin, 2), B, torch.float64)
        bst2 = Guarded((B, cin, 2), B)
        assert launch("ebsdvae_conv3x3_dgrad_inbwd_f16_bst", gin2, part2, bst2, yd, sd, y.shape[1] * y.shape[2])
        assert torch.equal(gin2.t, gin.t) and torch.equal(part2.t, part.t) and torch.equal(bst2.t, bst)


# ============================================================== 5. weight gradients
# (cin, cout, source mode, kind); ACT_NORM_POOL: the pooled activation materialised, passed RAW
WGRAD = [(32, 32, E.ACT_NORM, 0), (128, 64, E.ACT_NORM, 1), (64, 32, E.ACT_NORM_UP, 1),
         (32, 64, E.ACT_NORM_POOL, 0), (64, 128, E.ACT_NORM_POOL, 0)]
WG_ENTRY = {"fp32": ("ebsdvae_conv3x3_wgrad", 0), "bf16x3": ("ebsdvae_conv3x3_wgrad_split", 2),
            "bf16x6": ("ebsdvae_conv3x3_wgrad_split", 3), "f16x3": ("ebsdvae_conv3x3_wgrad_f16", F16)}


@functools.lru_cache(maxsize=None)
def _wgrad_inputs(H, W, cin, cout, mode):
    rng = np.random.default_rng(11 + cin + cout + H + 2 * W + mode)
    s, mean, rstd, st = U.make_src(rng, B, H, W, cin, mode)
    a = U.act_oracle(s, mean, rstd, mode)
    gy = rng.standard_normal((B, H, W) if cout == 1 else (B, H, W, cout))
    return _frozen(s, st, a, gy, *O.conv3x3_wgrad(a, gy.reshape(B, H, W, cout)))


def _wgrad_case(H, W, cin, cout, mode, kind, prec, must):
    name, pieces = WG_ENTRY[prec]
    s, st, a, gy, rw, rb = _wgrad_inputs(H, W, cin, cout, mode)
    if mode == E.ACT_NORM_POOL:
        src, sst, smode = dev(a), None, E.ACT_RAW
    else:
        src, sst, smode = dev(s), dev(st) if mode in U.NORM_MODES else None, mode
    gd = dev(gy)
    if pieces:
        S_ = N.call("ebsdvae_conv3x3_wgrad_split_slices", B, H, W, cin, cout, pieces)
    else:
        S_ = N.call("ebsdvae_conv3x3_wgrad_slices", B, H, W, cin, cout)
    assert S_ > 0 or not must
    Sa = max(S_, 1)
    wpart, bpart = Guarded((Sa, 9, cout, cin), 1), Guarded((Sa, cout), 1)
    args = [p(src), p(sst), smode, p(gd)]
    if prec == "f16x3":
        gmax = dev(np.abs(gy).reshape(B, 4, -1).max(2))   # four row bands per image
        args += [p(gmax), 4]
    args += [wpart.ptr(), bpart.ptr(), B, H, W, cin, cout]
    if name.endswith("_split"):
        args.append(pieces)
    if not run(name, [wpart, bpart], *args, U.stream(), must=must):
        assert S_ <= 0, "the slice query answers for a shape the entry point refuses"
        return None
    assert S_ > 0, "the entry point runs a shape the slice query refuses"
    assert wpart.written() and bpart.written()
    dw, db = U.reduce_slices(wpart.t, bpart.t, S_, cin, cout, kind)
    if kind == 1:
        rw = rw.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]
    gate = {"fp32": 5e-5, "bf16x3": U.SPLIT_TOL["bf16x3"] * 2, "bf16x6": U.SPLIT_TOL["bf16x6"] * 2,
            "f16x3": U.SPLIT_TOL["f16x3"]}[prec]
    e_w, e_b = O.rel_err(host(dw), rw), O.rel_err(host(db), rb)
    print(f"\n{name} {prec} {cin}->{cout} {H}x{W} mode {mode}: dW {e_w:.2e} db {e_b:.2e}")
    assert e_w < gate
    assert e_b < 5e-5
    return e_w


@pytest.mark.parametrize("prec", ["fp32"] + PRECS)
@pytest.mark.parametrize("cin,cout,mode,kind", WGRAD)
@pytest.mark.parametrize("H,W", RECT)
def test_conv_wgrad_rect(cuda, H, W, cin, cout, mode, kind, prec):
    _wgrad_case(H, W, cin, cout, mode, kind, prec, must=True)


@pytest.mark.parametrize("cin,cout,mode", [(1, 32, E.ACT_RAW), (32, 1, E.ACT_NORM)])
@pytest.mark.parametrize("H,W", RECT)
def test_conv_wgrad_single_channel_rect(cuda, H, W, cin, cout, mode):
    """The cin = 1 and cout = 1 kernels of ebsdvae_conv3x3_wgrad."""
    _wgrad_case(H, W, cin, cout, mode, 0, "fp32", must=True)


@pytest.mark.parametrize("prec", ["fp32"] + PRECS)
@pytest.mark.parametrize("H,W", [(96, 128), (24, 128)])
def test_conv_wgrad_band_counts_not_a_power_of_two(cuda, H, W, prec):
    """H / 8 is no power of two: the 2-piece and f16 forms refuse (slices -1), the fp32 and the
    3-piece forms run."""
    got = _wgrad_case(H, W, 32, 32, E.ACT_NORM, 0, prec, must=prec in ("fp32", "bf16x6"))
    assert (got is not None) == (prec in ("fp32", "bf16x6"))


@pytest.mark.parametrize("H,W", [(32, 8), (16, 8)])
def test_conv_wgrad_refuses_width_8_unless_8x8(cuda, H, W):
    """ebsdvae_conv3x3_wgrad tiles W = 8 as two whole 8 x 8 images: taller maps are refused with
    a message and untouched partials, and ebsdvae_conv3x3_wgrad_slices answers -1 for them."""
    assert N.call("ebsdvae_conv3x3_wgrad_slices", B, H, W, 32, 32) == -1
    assert N.call("ebsdvae_conv3x3_wgrad_slices", B, 8, 8, 128, 128) > 0
    assert N.call("ebsdvae_conv3x3_wgrad_slices", B, H, W, 1, 32) > 0   # any tile
    assert _wgrad_case(H, W, 32, 32, E.ACT_NORM, 0, "fp32", must=False) is None


def test_dwgrad_refuses_rectangles(cuda):
    H, W, C = 16, 32, 32
    assert N.call("ebsdvae_conv3x3_dwgrad_slices", B, H, W, C, C) == -1
    z = dev(np.zeros((B, H, W, C)))
    st, gmax = dev(np.ones((B, C, 2))), dev(np.ones((B, 1)))
    wpk = U.pack(dev(np.zeros((C, C, 3, 3))), C, C, 0, F16, True)
    outs = [Guarded((B, H, W, C), B), Guarded((B, 8, C, 2), B, torch.float64), Guarded((4, 9, C, C), 1),
            Guarded((4, C), 1)]
    assert not run("ebsdvae_conv3x3_dwgrad_f16", outs, p(z), p(gmax), 1, p(wpk), p(z), p(st), E.ACT_NORM,
                   *[g.ptr() for g in outs], B, H, W, C, C, U.stream())


# ============================================================== 8. corrected ingest, rectangular windows
# windows whose area fits the one-launch kernel (side up to 256), and two for the phased path
ONE_LAUNCH = both(64, 96) + both(160, 96) + both(256, 64)
PHASED = both(192, 128)


def _detector(h, w):
    """A detector a few pixels larger than the window, odd margins that differ per axis."""
    return h + 5, w + 3


def _corr_oracle(Bn, h, w, static_mode, sigma, dynamic_mode, dtype="uint8"):
    H0, W0 = _detector(h, w)
    raw, bg = R.detector_patterns(Bn, H0, W0, seed=H0 + w)
    if dtype != "uint8":
        raw = raw.astype(dtype)
        t, l = R.crop_offset(H0, h), R.crop_offset(W0, w)
        raw[0, t + 10, l + 12] = np.nan          # both inside the window
        raw[Bn - 1, t + h - 1, l] = np.inf
    sbg = None if static_mode is None else R.static_background(bg, static_mode)
    ref = R.correct(raw, (h, w), sbg, static_mode, sigma, dynamic_mode)
    R.assert_well_conditioned(ref, dynamic_mode == "divide")
    return raw, bg, ref["out"]


def _corr_check(Bn, h, w, static_mode, sigma, dynamic_mode, dtype="uint8"):
    raw, bg, want = _corr_oracle(Bn, h, w, static_mode, sigma, dynamic_mode, dtype)
    assert (N.call("ebsdvae_correct_patterns_work", Bn, h, w) == 0) == (h * w <= 128 * 128)
    out = Guarded((Bn, 1, h, w), Bn)
    res = correct_patterns(raw, (h, w), _correction(bg, static_mode, sigma, dynamic_mode), out=out.t)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.ptr() and out.slack_intact()
    got = out.t.cpu().numpy()
    err = np.abs(got - want).max()
    print(f"\n{dtype} {raw.shape[1]}x{raw.shape[2]}->{h}x{w} static={static_mode} dynamic={dynamic_mode} "
          f"sigma={sigma}: max err {err:.2e}")
    assert np.isfinite(got).all()
    per = got.reshape(Bn, -1)
    assert (per.min(1) == 0.0).all() and (per.max(1) == 1.0).all()
    assert err <= GATE, err


def _sigma_for_radius(r):
    """A sigma whose 4-sigma radius int(4 sigma + 0.5) is exactly r."""
    sigma = (r - 0.4) / 4.0
    assert int(4.0 * sigma + 0.5) == r
    return sigma


@pytest.mark.parametrize("static_mode,dynamic_mode", THREE_PAIRS)
@pytest.mark.parametrize("h,w", ONE_LAUNCH + PHASED)
def test_correction_rect_windows(cuda, h, w, static_mode, dynamic_mode):
    _corr_check(B, h, w, static_mode, 4.0, dynamic_mode)


@pytest.mark.parametrize("h,w", ONE_LAUNCH + PHASED)
def test_correction_rect_maximal_reflection_on_the_short_side(cuda, h, w):
    """radius == min(h, w): the blur reflects across the whole short side and stays inside the
    long one."""
    _corr_check(B, h, w, "divide", _sigma_for_radius(min(h, w)), "subtract")


@pytest.mark.parametrize("h,w", both(160, 96) + both(192, 128))
def test_correction_rect_float32_source_with_non_finite_values(cuda, h, w):
    _corr_check(B, h, w, "divide", 4.0, "divide", "float32")


def test_correction_rect_pattern_does_not_depend_on_its_batch(cuda):
    h, w = 160, 96
    H0, W0 = _detector(h, w)
    raw, bg = R.detector_patterns(5, H0, W0, seed=H0 + w)
    c = _correction(bg, "divide", 4.0, "divide")
    batch = correct_patterns(raw, (h, w), c).cpu().numpy()
    for i in range(5):
        alone = correct_patterns(raw[i:i + 1], (h, w), c).cpu().numpy()
        assert alone.tobytes() == batch[i:i + 1].tobytes(), i


def test_correction_rect_radius_past_the_short_side_is_refused(cuda):
    """The ABI's own guard (data_module checks first and raises ValueError): radius > min side."""
    h, w = 160, 96
    H0, W0 = _detector(h, w)
    raw = torch.zeros(B, H0, W0, dtype=torch.uint8, device="cuda")
    taps = torch.ones(w + 2, device="cuda")
    out = Guarded((B, 1, h, w), B)
    assert not run("ebsdvae_correct_patterns", [out], p(raw), 2, B, H0, W0, h, w, None, 0, p(taps), w + 1, 1,
                   out.ptr(), None, U.stream())
    with pytest.raises(ValueError, match="blur radius"):
        correct_patterns(raw, (h, w), PatternCorrection(dynamic_sigma=_sigma_for_radius(w + 1)))
