"""Kernel-level parity: every HIP entry point vs the numpy oracle primitives (float64),
seeded random inputs at sizes the oracle finishes in seconds.  Tolerances are norm-wise
(max|d| / max|ref|) and stated per test."""
import numpy as np
import pytest
import torch

from latice import _native as N
from latice import engine as E
from oracle import vae_oracle as O

pytestmark = pytest.mark.gpu

TOL = 2e-5   # fp32 single-layer ops vs float64


@pytest.fixture(autouse=True)
def _fp32_kernels():
    """These tests pin the fp32-MFMA kernels; the split-bf16 tests switch precision
    explicitly inside."""
    with E.precision("fp32"):
        yield


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def act_oracle(src, mean, rstd, mode):
    """Logical conv input from a source tensor under an act mode (NHWC float64)."""
    if mode == E.ACT_RAW:
        return src
    if mode == E.ACT_UP:
        return O.upsample2(src)
    a = O.lrelu((src - mean) * rstd)
    if mode == E.ACT_NORM:
        return a
    if mode == E.ACT_NORM_POOL:
        return O.maxpool2(a)[0]
    return O.upsample2(a)


def src_shape(B, H, C, mode):
    if mode == E.ACT_NORM_POOL:
        return (B, 2 * H, 2 * H, C)
    if mode in (E.ACT_UP, E.ACT_NORM_UP):
        return (B, H // 2, H // 2, C)
    return (B, H, H, C)


def make_src(rng, B, H, C, mode):
    s = rng.standard_normal(src_shape(B, H, C, mode)) * 1.5 + 0.3
    mean = s.mean(axis=(1, 2), keepdims=True)
    rstd = 1.0 / np.sqrt(s.var(axis=(1, 2), keepdims=True) + 1e-5)
    st = np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)   # (B, C, 2)
    return s, mean, rstd, st


# (cin, cout, H, mode) covering every conv configuration of the 128 and 256 networks
FWD_CASES = [
    (1, 32, 128, E.ACT_RAW), (32, 32, 128, E.ACT_NORM), (32, 64, 64, E.ACT_NORM_POOL),
    (64, 64, 64, E.ACT_NORM), (64, 128, 32, E.ACT_NORM_POOL), (128, 128, 16, E.ACT_NORM_POOL),
    (128, 128, 8, E.ACT_NORM_POOL), (128, 128, 8, E.ACT_UP), (128, 128, 16, E.ACT_NORM_UP),
    (128, 64, 32, E.ACT_NORM), (64, 32, 64, E.ACT_NORM), (32, 32, 128, E.ACT_NORM_UP),
    (32, 32, 256, E.ACT_NORM), (64, 32, 64, E.ACT_RAW), (128, 64, 32, E.ACT_RAW),
    (64, 128, 32, E.ACT_RAW), (32, 64, 64, E.ACT_RAW),
]


@pytest.mark.parametrize("cin,cout,H,mode", FWD_CASES)
def test_conv3x3_fwd_and_in_stats(cuda, cin, cout, H, mode):
    rng = np.random.default_rng(cin * 1000 + cout + H + mode)
    B = 3 if H <= 64 else 2
    s, mean, rstd, st = make_src(rng, B, H, cin, mode)
    w = rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)
    b = rng.standard_normal(cout) * 0.1
    layer = E.ConvLayer("t", E.KIND_CONV, cin, cout, H, mode, 0)
    keep = cin > 1
    out = E.conv_forward(dev(s), dev(st) if mode in (1, 2, 4) else None, layer, dev(w), dev(b), B,
                         keep_act=keep)
    y, stt = out[0], out[1]
    a_ref = act_oracle(s, mean, rstd, mode)
    ref = O.conv3x3(a_ref, w, b)
    assert O.rel_err(host(y), ref) < TOL
    if keep:   # the materialised conv input (used by pool-fed layers' wgrad)
        assert O.rel_err(host(out[2]), a_ref) < 1e-6
    _, rm, rr = O.instance_norm(ref)
    got = host(stt)
    assert O.rel_err(got[..., 0], rm[:, 0, 0, :]) < 1e-5
    assert O.rel_err(got[..., 1], rr[:, 0, 0, :]) < 1e-4


@pytest.mark.parametrize("kind", [E.KIND_CONV, E.KIND_CONVT])
@pytest.mark.parametrize("cin,cout,H", [(32, 64, 32), (128, 128, 8), (64, 32, 64), (128, 64, 16)])
def test_conv_dgrad_matches_oracle(cuda, kind, cin, cout, H):
    rng = np.random.default_rng(7 + cin + cout + H + kind)
    B = 2
    gy = rng.standard_normal((B, H, H, cout))
    wsrc = rng.standard_normal((cout, cin, 3, 3) if kind == 0 else (cin, cout, 3, 3)) * 0.1
    wc = wsrc if kind == 0 else O.conv_w_from_convT(wsrc)
    layer = E.ConvLayer("t", kind, cin, cout, H, E.ACT_RAW, 0)
    gin = E.conv_dgrad(dev(gy), layer, dev(wsrc))
    assert O.rel_err(host(gin), O.conv3x3_dgrad(gy, wc)) < TOL


WG_CASES = [
    (1, 32, 128, E.ACT_RAW, 0), (32, 32, 128, E.ACT_NORM, 0), (32, 64, 64, E.ACT_NORM_POOL, 0),
    (64, 128, 32, E.ACT_NORM_POOL, 0), (128, 128, 8, E.ACT_NORM_POOL, 0),
    (128, 128, 8, E.ACT_UP, 1), (128, 64, 32, E.ACT_NORM, 1), (64, 32, 64, E.ACT_NORM, 1),
    (32, 32, 128, E.ACT_NORM_UP, 1), (32, 1, 128, E.ACT_NORM, 0),
]


@pytest.mark.parametrize("cin,cout,H,mode,kind", WG_CASES)
def test_conv_wgrad_matches_oracle(cuda, cin, cout, H, mode, kind):
    rng = np.random.default_rng(11 + cin + cout + H + mode)
    B = 3 if H <= 64 else 2
    s, mean, rstd, st = make_src(rng, B, H, cin, mode)
    gshape = (B, H, H) if cout == 1 else (B, H, H, cout)
    gy = rng.standard_normal(gshape)
    wshape = (cout, cin, 3, 3) if kind == 0 else (cin, cout, 3, 3)
    dw = torch.empty(wshape, device="cuda")
    db = torch.empty(cout, device="cuda")
    if mode == E.ACT_NORM_POOL:
        # pool-fed layers: the forward conv materialises the pooled activation, the wgrad
        # reads it RAW
        layer = E.ConvLayer("t", E.KIND_CONV, cin, cout, H, mode, 0)
        wdummy = dev(np.zeros((cout, cin, 3, 3)))
        _, _, act = E.conv_forward(dev(s), dev(st), layer, wdummy, dev(np.zeros(cout)), B, keep_act=True)
        E.conv_wgrad(act, None, E.ACT_RAW, dev(gy), cin, cout, kind, dw, db)
    else:
        E.conv_wgrad(dev(s), dev(st) if mode in (1, 2, 4) else None, mode, dev(gy), cin, cout, kind, dw, db)
    a = act_oracle(s, mean, rstd, mode)
    rw, rb = O.conv3x3_wgrad(a, gy.reshape(B, H, H, cout))
    if kind == 1:
        rw = rw.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]
    assert O.rel_err(host(dw), rw) < 5e-5
    assert O.rel_err(host(db), rb) < 5e-5


@pytest.mark.parametrize("pmode,H,C", [(E.P_ID, 64, 32), (E.P_POOL, 32, 64), (E.P_POOL, 8, 128),
                                       (E.P_UP, 16, 128), (E.P_UP, 64, 32), (E.P_ID, 128, 32)])
def test_instance_norm_backward(cuda, pmode, H, C):
    rng = np.random.default_rng(3 + pmode + H + C)
    B = 2
    y = rng.standard_normal((B, H, H, C)) * 2 + 0.5
    xh, mean, rstd = O.instance_norm(y)
    st = np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)
    gshape = {E.P_ID: (B, H, H, C), E.P_POOL: (B, H // 2, H // 2, C), E.P_UP: (B, 2 * H, 2 * H, C)}[pmode]
    gn = rng.standard_normal(gshape)
    gy = E.in_backward(dev(gn), pmode, dev(y), dev(st))
    a = O.lrelu(xh)
    if pmode == E.P_POOL:
        _, arg = O.maxpool2(a)
        ga = O.maxpool2_bwd(gn, arg)
    elif pmode == E.P_UP:
        ga = O.upsample2_bwd(gn)
    else:
        ga = gn
    ref = O.instance_norm_bwd(ga * O.lrelu_slope(xh), xh, rstd)
    assert O.rel_err(host(gy), ref) < 1e-4


def h_oracle(gn, xh, pmode, summed=False):
    """What a fused input gradient writes (csrc/conv_common.h): h = g * lrelu'(xhat) at the
    y_prev pixel g routes to -- pooled resolution for P_POOL (xhat at the window maximum),
    the consumer's resolution for P_UP (the parent's xhat), y_prev's for the summed upsample
    adjoint (summed=True: the 2x2 sums of g)."""
    if pmode == E.P_POOL:
        return gn * O.lrelu_slope(O.maxpool2(xh)[0])
    if pmode == E.P_UP and not summed:
        return gn * O.lrelu_slope(O.upsample2(xh))
    if summed:
        gn = O.upsample2_bwd(gn)
    return gn * O.lrelu_slope(xh)


FUSED_CASES = [  # (layer cin, layer cout, H, pmode of the block feeding the layer)
    (32, 32, 128, E.P_ID), (32, 64, 64, E.P_POOL), (64, 128, 32, E.P_POOL), (128, 128, 16, E.P_UP),
    (128, 128, 8, E.P_POOL), (128, 128, 8, E.P_ID), (64, 32, 64, E.P_UP), (128, 64, 32, E.P_ID),
]


@pytest.mark.parametrize("cin,cout,H,pmode", FUSED_CASES)
def test_dgrad_fused_instance_norm_backward(cuda, cin, cout, H, pmode):
    """Input-gradient conv with the previous block's InstanceNorm-backward reduce fused in
    its epilogue == conv dgrad, then the unfused IN backward (oracle)."""
    rng = np.random.default_rng(5 + cin + cout + H + pmode)
    B = 2
    Hy = {E.P_ID: H, E.P_POOL: 2 * H, E.P_UP: H // 2}[pmode]
    y = rng.standard_normal((B, Hy, Hy, cin)) * 2 + 0.5
    xh, mean, rstd = O.instance_norm(y)
    st = np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)
    gy = rng.standard_normal((B, H, H, cout))
    wsrc = rng.standard_normal((cout, cin, 3, 3)) * 0.1
    layer = E.ConvLayer("t", E.KIND_CONV, cin, cout, H, E.ACT_RAW, 0)
    y_d, st_d = dev(y), dev(st)
    gin, part = E.conv_dgrad(dev(gy), layer, dev(wsrc), prev=(y_d, st_d, pmode))
    g_prev = E.in_backward(gin, pmode, y_d, st_d, part=part)
    gn = O.conv3x3_dgrad(gy, wsrc)
    assert O.rel_err(host(gin), h_oracle(gn, xh, pmode)) < TOL
    a = O.lrelu(xh)
    if pmode == E.P_POOL:
        _, arg = O.maxpool2(a)
        ga = O.maxpool2_bwd(gn, arg)
    elif pmode == E.P_UP:
        ga = O.upsample2_bwd(gn)
    else:
        ga = gn
    ref = O.instance_norm_bwd(ga * O.lrelu_slope(xh), xh, rstd)
    assert O.rel_err(host(g_prev), ref) < 1e-4


def test_act_apply_and_upsample_bwd(cuda):
    rng = np.random.default_rng(5)
    s, mean, rstd, st = make_src(rng, 3, 4, 128, E.ACT_NORM_POOL)
    out = torch.empty(3, 4, 4, 128, device="cuda")
    ds, dst = dev(s), dev(st)     # keep the inputs alive until the kernel has run
    N.call("ebsdvae_act_apply", N.ptr(ds), N.ptr(dst), E.ACT_NORM_POOL, N.ptr(out), 3, 4, 4,
           128, N.stream())
    assert O.rel_err(host(out), act_oracle(s, mean, rstd, E.ACT_NORM_POOL)) < 1e-5
    g = rng.standard_normal((3, 8, 8, 128))
    o2 = torch.empty(3, 4, 4, 128, device="cuda")
    dg = dev(g)
    N.call("ebsdvae_upsample2_bwd", N.ptr(dg), N.ptr(o2), 3, 4, 4, 128, N.stream())
    assert O.rel_err(host(o2), O.upsample2_bwd(g)) < 1e-6


def test_cout1_conv_fwd_dgrad_and_first_conv_input_grad(cuda):
    rng = np.random.default_rng(9)
    B, H = 2, 128
    s, mean, rstd, st = make_src(rng, B, H, 32, E.ACT_NORM)
    w = rng.standard_normal((1, 32, 3, 3)) * 0.1
    b = np.array([0.3])
    out = torch.empty(B, 1, H, H, device="cuda")
    ds, dst, dw, db = dev(s), dev(st), dev(w), dev(b)
    N.call("ebsdvae_conv3x3_cout1_fwd", N.ptr(ds), N.ptr(dst), E.ACT_NORM, N.ptr(dw),
           N.ptr(db), N.ptr(out), 0, B, H, H, 32, N.stream())
    a = act_oracle(s, mean, rstd, E.ACT_NORM)
    assert O.rel_err(host(out)[:, 0], O.conv3x3(a, w, b)[..., 0]) < TOL
    g = rng.standard_normal((B, H, H))
    gin = torch.empty(B, H, H, 32, device="cuda")
    dg = dev(g)
    N.call("ebsdvae_conv3x3_cout1_dgrad", N.ptr(dg), N.ptr(dw), N.ptr(gin), B, H, H, 32,
           N.stream())
    assert O.rel_err(host(gin), O.conv3x3_dgrad(g[..., None], w)) < TOL
    # input gradient of the first conv (1 -> 32) = flipped cout1 conv over gy
    w0 = rng.standard_normal((32, 1, 3, 3)) * 0.2
    gy = rng.standard_normal((B, H, H, 32))
    gx = torch.empty(B, 1, H, H, device="cuda")
    dgy, dw0 = dev(gy), dev(w0)
    N.call("ebsdvae_conv3x3_cout1_fwd", N.ptr(dgy), None, E.ACT_RAW, N.ptr(dw0), None,
           N.ptr(gx), 1, B, H, H, 32, N.stream())
    assert O.rel_err(host(gx)[:, 0], O.conv3x3_dgrad(gy, w0)[..., 0]) < TOL


# B = 5: the one-pattern tiles; B = 300: two-pattern tiles with a partly filled last tile (the
# b < B masks at R > 1); B = 1024: the c4 batch
@pytest.mark.parametrize("B", [5, 300, 1024])
@pytest.mark.parametrize("S,L", [(128, 16), (256, 64)])
def test_heads_forward_backward(cuda, S, L, B):
    rng = np.random.default_rng(S + L + B)
    plan = E.build_plan(32, L, S)
    s, C, F = plan.enc_side, plan.enc_channels, plan.feat
    enc = rng.standard_normal((B, s, s, C))
    p = {"mu.0.weight": rng.standard_normal((L, F)) * 0.02, "mu.0.bias": rng.standard_normal(L) * 0.1,
         "logvar.0.weight": rng.standard_normal((L, F)) * 0.02,
         "logvar.0.bias": rng.standard_normal(L) * 0.1,
         "linear2.0.weight": rng.standard_normal((F, L)) * 0.2,
         "linear2.0.bias": rng.standard_normal(F) * 0.1}
    eps = rng.standard_normal((B, L))
    pd = {k: dev(v) for k, v in p.items()}
    flat, mu, std, z, dec_in = E.heads_forward(plan, dev(enc), pd, dev(eps))
    rflat = O.nchw_flatten(enc)
    rmu = rflat @ p["mu.0.weight"].T + p["mu.0.bias"]
    rlv = rflat @ p["logvar.0.weight"].T + p["logvar.0.bias"]
    rstd = np.exp(rlv / 2)
    rz = rmu + eps * rstd
    rout = rz @ p["linear2.0.weight"].T + p["linear2.0.bias"]
    assert O.rel_err(host(flat), rflat) < 1e-7
    for got, ref in ((mu, rmu), (std, rstd), (z, rz)):
        assert O.rel_err(host(got), ref) < 1e-5
    assert O.rel_err(host(dec_in), O.nchw_unflatten(rout, C, s)) < 1e-5
    # backward
    g_dec = rng.standard_normal((B, s, s, C))
    gz, gmu, gstd = (rng.standard_normal((B, L)) for _ in range(3))
    g_enc, grads = E.heads_backward(plan, dev(g_dec), dev(gz), dev(gmu), dev(gstd), flat, std, z,
                                    dev(eps), pd)
    g_out = O.nchw_flatten(g_dec)
    gzt = g_out @ p["linear2.0.weight"] + gz
    gmt = gzt + gmu
    glv = (gstd + gzt * eps) * rstd / 2
    ref = {"linear2.0.weight": g_out.T @ rz, "linear2.0.bias": g_out.sum(0),
           "mu.0.weight": gmt.T @ rflat, "mu.0.bias": gmt.sum(0),
           "logvar.0.weight": glv.T @ rflat, "logvar.0.bias": glv.sum(0)}
    for k, v in ref.items():
        assert O.rel_err(host(grads[k]), v) < 1e-4, k
    rgenc = O.nchw_unflatten(gmt @ p["mu.0.weight"] + glv @ p["logvar.0.weight"], C, s)
    assert O.rel_err(host(g_enc), rgenc) < 1e-4
    # the inference heads (encode_latents' ebsdvae_latent_mu) on the same features
    mu2 = torch.empty(B, L, device="cuda")
    work = E._heads_work(B, plan, mu2)
    N.call("ebsdvae_latent_mu", N.ptr(dev(enc)), N.ptr(pd["mu.0.weight"]), N.ptr(pd["mu.0.bias"]),
           N.ptr(mu2), N.ptr(work), B, C, s, L, N.stream())
    assert O.rel_err(host(mu2), rmu) < 1e-5


@pytest.mark.parametrize("B,P", [(4, 128 * 128), (3, 250)])
def test_vae_loss_forward_backward(cuda, B, P):
    rng = np.random.default_rng(B + P)
    L = 16
    xh = rng.standard_normal((B, P)) * 3
    x = np.floor(rng.random((B, P)) * 255) / 255
    mu = rng.standard_normal((B, L))
    std = np.exp(rng.standard_normal((B, L)) * 0.3)
    z = mu + rng.standard_normal((B, L)) * std
    lam = 0.1
    t = [dev(a) for a in (xh, x, z, mu, std)]
    (loss, kl_loss, rec_loss), (elbo, kl, rec) = E.loss_forward(*t, lam)
    ref = O.vae_loss(xh.reshape(B, 1, 1, P), x.reshape(B, 1, 1, P), z, mu, std, lam)
    assert abs(float(loss) - ref["loss"]) < 1e-6 * max(1, abs(ref["loss"]))
    assert abs(float(kl_loss) - ref["kl_loss"]) < 1e-5 * max(1e-3, abs(ref["kl_loss"]))
    assert O.rel_err(host(elbo), ref["elbo"]) < 1e-6
    one = torch.ones((), device="cuda")
    g_xhat, g_z, g_mu, g_std, g_x = E.loss_backward(*t, lam, g_loss=one, need_gx=True)
    sig = 1 / (1 + np.exp(-xh))
    assert O.rel_err(host(g_xhat), (sig - x) / (P * B)) < 1e-5
    assert O.rel_err(host(g_x), -xh / (P * B)) < 1e-5
    c = lam / (B * L)
    assert O.rel_err(host(g_z), c * (z - (z - mu) / std ** 2)) < 1e-5
    assert O.rel_err(host(g_mu), c * (z - mu) / std ** 2) < 1e-5
    assert O.rel_err(host(g_std), c * ((z - mu) ** 2 / std ** 3 - 1 / std)) < 1e-5


# (1, 252, 16): a single pattern; (300, 64, 64): the batch means stride past 256 patterns;
# (2, 250, 256): the largest latent the entry points take, the scalar loop of P % 4 != 0
@pytest.mark.parametrize("std_kind", ["lognormal", "1e-3"])
@pytest.mark.parametrize("targets", ["unit", "u8"])
@pytest.mark.parametrize("logit_std", [3, 200])
@pytest.mark.parametrize("B,P,L", [(1, 252, 16), (300, 64, 64), (2, 250, 256)])
def test_vae_loss_edges(cuda, B, P, L, logit_std, targets, std_kind):
    """ebsdvae_vae_loss_fwd / _bwd at the edges of their shapes and input ranges, at the gates of
    test_vae_loss_forward_backward: saturated logits (exp(-|x|) underflows, sigmoid is exactly 0
    or 1), targets 0...255, a posterior of std 1e-3 (z - mu is 1e-3 of z).  The inputs are
    rounded to float32 before the reference sees them: z - mu cancels, and the kernel is not to
    be charged with the rounding of its own input.
    The draw: with targets 0...255 a pattern's BCE sum runs over terms (1 - x) xhat of either
    sign whose mean is zero, and what the 1e-6 gate then measures is how far one draw's terms
    cancel: sum |term| / |sum term| is 50 ... 300 whatever the seed, and a float32 restatement
    of the 256-thread strided sums, on the CPU, lands between 2e-7 and 3e-6 over 40 seeds at
    B = 1.  With these seeds the restatement gives <= 1.7e-7 on loss and elbo and <= 1.2e-7 on
    kl_loss over all 24 cases; the kernels (fixed summation order) <= 5.5e-7, the largest at
    (1, 252, 16), logit std 3, targets 0...255, and <= 1.4e-7 wherever the targets are unit."""
    rng = np.random.default_rng(35 + 1000 * B + P + L + logit_std)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
    xh = f32(rng.standard_normal((B, P)) * logit_std)
    u = rng.random((B, P))
    x = np.floor(u * 256) if targets == "u8" else np.floor(u * 255) / 255
    x = f32(x)
    mu = f32(rng.standard_normal((B, L)))
    std = f32(np.exp(rng.standard_normal((B, L)) * 0.3) if std_kind == "lognormal" else np.full((B, L), 1e-3))
    z = f32(mu + rng.standard_normal((B, L)) * std)
    lam = 0.1
    t = [dev(a) for a in (xh, x, z, mu, std)]
    (loss, kl_loss, rec_loss), (elbo, kl, rec) = E.loss_forward(*t, lam)
    ref = O.vae_loss(xh.reshape(B, 1, 1, P), x.reshape(B, 1, 1, P), z, mu, std, lam)
    print(f"\nvae_loss B {B} P {P} L {L}: loss {abs(float(loss) - ref['loss']) / max(1, abs(ref['loss'])):.2e} "
          f"kl {abs(float(kl_loss) - ref['kl_loss']) / max(1e-3, abs(ref['kl_loss'])):.2e} "
          f"elbo {O.rel_err(host(elbo), ref['elbo']):.2e}")
    assert abs(float(loss) - ref["loss"]) < 1e-6 * max(1, abs(ref["loss"]))
    assert abs(float(kl_loss) - ref["kl_loss"]) < 1e-5 * max(1e-3, abs(ref["kl_loss"]))
    assert O.rel_err(host(elbo), ref["elbo"]) < 1e-6
    one = torch.ones((), device="cuda")
    g_xhat, g_z, g_mu, g_std, g_x = E.loss_backward(*t, lam, g_loss=one, need_gx=True)
    sig = np.exp(-np.logaddexp(0.0, -xh))   # overflow-safe, as O.vae_loss
    assert O.rel_err(host(g_xhat), (sig - x) / (P * B)) < 1e-5
    assert O.rel_err(host(g_x), -xh / (P * B)) < 1e-5
    c = lam / (B * L)
    assert O.rel_err(host(g_z), c * (z - (z - mu) / std ** 2)) < 1e-5
    assert O.rel_err(host(g_mu), c * (z - mu) / std ** 2) < 1e-5
    assert O.rel_err(host(g_std), c * ((z - mu) ** 2 / std ** 3 - 1 / std)) < 1e-5


def test_normal_sampler(cuda):
    a = torch.empty(1 << 20, device="cuda")
    b = torch.empty(1 << 20, device="cuda")
    E.normal_(a, 1234)
    E.normal_(b, 1234)
    assert torch.equal(a, b)
    m, s = float(a.mean()), float(a.std())
    assert abs(m) < 5e-3 and abs(s - 1) < 5e-3
    E.normal_(b, 1235)
    assert not torch.equal(a, b)
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    E.normal_(a, 7, counter=ctr)
    E.normal_(b, 7, counter=ctr)
    assert int(ctr) == 2 and not torch.equal(a, b)


@pytest.mark.parametrize("amsgrad", [False, True])
def test_fused_adam_matches_torch_adam(cuda, amsgrad):
    from latice.optim import FusedAdam
    torch.manual_seed(0)
    p0 = torch.randn(10007, device="cuda")
    pa = p0.clone().requires_grad_(True)
    pb = p0.clone().requires_grad_(True)
    oa = FusedAdam([pa], lr=1e-3, amsgrad=amsgrad, weight_decay=0.01)
    ob = torch.optim.Adam([pb], lr=1e-3, amsgrad=amsgrad, weight_decay=0.01, foreach=False)
    for _ in range(5):
        g = torch.randn(10007, device="cuda")
        pa.grad = g.clone()
        pb.grad = g.clone()
        oa.step()
        ob.step()
    torch.cuda.synchronize()
    assert torch.allclose(pa, pb, rtol=1e-6, atol=1e-7)


def test_fused_final_conv_backward(cuda):
    """Last block + final conv(32->1): gy of the block and dW/db of the final conv from the
    1-channel logit gradient, without materialising the block's output gradient."""
    rng = np.random.default_rng(21)
    B, H, C = 2, 64, 32
    y = rng.standard_normal((B, H, H, C)) * 1.7 + 0.2
    xh, mean, rstd = O.instance_norm(y)
    st = np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)
    w14 = rng.standard_normal((1, C, 3, 3)) * 0.2
    g1 = rng.standard_normal((B, H, H))
    dw = torch.empty(1, C, 3, 3, device="cuda")
    db = torch.empty(1, device="cuda")
    gy = E.in_backward_final(dev(g1), dev(w14), dev(y), dev(st), dw, db)
    ga = O.conv3x3_dgrad(g1[..., None], w14)
    ref_gy = O.instance_norm_bwd(ga * O.lrelu_slope(xh), xh, rstd)
    rw, rb = O.conv3x3_wgrad(O.lrelu(xh), g1[..., None])
    assert O.rel_err(host(gy), ref_gy) < 1e-4
    assert O.rel_err(host(dw), rw) < 5e-5
    assert O.rel_err(host(db), rb) < 5e-5


def test_fused_first_conv_weight_grad(cuda):
    """First block: dW/db of the conv(1->32) straight from the InstanceNorm-backward pass."""
    rng = np.random.default_rng(22)
    B, H, C = 2, 64, 32
    y = rng.standard_normal((B, H, H, C)) * 1.3 - 0.4
    xh, mean, rstd = O.instance_norm(y)
    st = np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)
    gn = rng.standard_normal((B, H, H, C))
    x = np.floor(rng.random((B, H, H, 1)) * 255) / 255
    dw = torch.empty(C, 1, 3, 3, device="cuda")
    db = torch.empty(C, device="cuda")
    E.in_backward_first(dev(gn), dev(y), dev(st), dev(x), dw, db)
    gy = O.instance_norm_bwd(gn * O.lrelu_slope(xh), xh, rstd)
    rw, rb = O.conv3x3_wgrad(x, gy)
    assert O.rel_err(host(dw), rw) < 1e-4
    assert np.abs(host(db) - rb).max() < 1e-4 * max(1.0, np.abs(rb).max())


@pytest.mark.parametrize("H", [128, 256, 64])
def test_first_conv_valu_and_recomputed_backward(cuda, H):
    """ebsdvae_conv_first_fwd (VALU fma chain) vs the oracle conv + InstanceNorm statistics,
    and the first block's backward with y0 recomputed from x
    (ebsdvae_in_bwd_first_apply_wgrad_rc) bit-identical to the one that reads y0."""
    rng = np.random.default_rng(23 + H)
    B, C = 2, 32
    x = np.floor(rng.random((B, 1, H, H)) * 255) / 255
    w = rng.standard_normal((C, 1, 3, 3)) / 3.0
    b = rng.standard_normal(C) * 0.1
    layer = E.ConvLayer("encoder.0.0", E.KIND_CONV, 1, C, H, E.ACT_RAW, E.P_ID)
    xd, wd, bd = dev(x), dev(w), dev(b)
    y, st = E.conv_forward(xd, None, layer, wd, bd, B)
    assert getattr(y, "ev_first_valu", False)
    ref = O.conv3x3(x.transpose(0, 2, 3, 1), w, b)
    assert O.rel_err(host(y), ref) < 1e-6
    xh, rm, rr = O.instance_norm(ref)
    got = host(st)
    assert O.rel_err(got[..., 0], rm[:, 0, 0, :]) < 1e-5
    assert O.rel_err(got[..., 1], rr[:, 0, 0, :]) < 1e-5
    gn = dev(rng.standard_normal((B, H, H, C)))
    dw_rc, db_rc = torch.empty(C, 1, 3, 3, device="cuda"), torch.empty(C, device="cuda")
    dw_rd, db_rd = torch.empty_like(dw_rc), torch.empty_like(db_rc)
    E.in_backward_first(gn, y, st, xd, dw_rc, db_rc, w0=wd, b0=bd)   # recomputes y0
    E.in_backward_first(gn, y, st, xd, dw_rd, db_rd)                   # reads y0
    torch.cuda.synchronize()
    assert torch.equal(dw_rc, dw_rd) and torch.equal(db_rc, db_rd)
    gy = O.instance_norm_bwd(host(gn) * O.lrelu_slope(xh), xh, rr)
    rw, rb = O.conv3x3_wgrad(x.transpose(0, 2, 3, 1), gy)
    # the fused first-block weight gradient accumulates B*H*W strongly cancelling products in
    # fp32 (the same kernel reading y0 gives the same bits, asserted above): 5e-4 at 256^2
    assert O.rel_err(host(dw_rc), rw) < (1e-4 if H <= 128 else 1e-3)
    # db is analytically zero (a bias before InstanceNorm): fp32 cancellation over the plane,
    # bounded by a few ulps of the L1 norm of the summands
    l1 = np.abs(gy).sum(axis=(0, 1, 2))
    assert (np.abs(host(db_rc) - rb) <= 2e-8 * l1).all()


def test_batched_weight_pack_matches_single_packs(cuda):
    """ebsdvae_pack_conv_weights (one launch per step) == per-layer ebsdvae_pack_conv_weight."""
    plan = E.build_plan(32, 16, 128)
    rng = np.random.default_rng(17)
    params = {}
    for L in plan.enc + plan.dec:
        shape = (L.cout, L.cin, 3, 3) if L.kind == E.KIND_CONV else (L.cin, L.cout, 3, 3)
        params[L.name + ".weight"] = dev(rng.standard_normal(shape))
    ps = E.PackSet(plan, params)
    packs = ps.refresh()
    for i, L in enumerate(plan.enc + plan.dec):
        w = params[L.name + ".weight"]
        pf, pd = packs[L.name]
        if pf is None:   # the VALU first conv reads its weight unpacked
            assert L.cin == 1 and i == 0, L.name
            continue
        single = E.pack_weight(w, L, dgrad=False)
        assert pf.pieces == single.pieces and torch.equal(pf.t, single.t), L.name
        if pd is not None:
            single = E.pack_weight(w, L, dgrad=True)
            assert pd.pieces == single.pieces and torch.equal(pd.t, single.t), L.name


def test_batched_wgrad_reduce_matches_per_layer(cuda):
    """ebsdvae_wgrad_reduce_batch (two launches for many layers) is bit-identical to the
    per-layer ebsdvae_wgrad_reduce, for conv and convT layouts, with and without bias."""
    rng = np.random.default_rng(23)
    layers = [(300, 32, 32, E.KIND_CONV, True), (17, 64, 128, E.KIND_CONVT, True),
              (64, 1, 32, E.KIND_CONV, True), (5, 32, 1, E.KIND_CONV, False)]
    items, singles = [], []
    for S_, cin, cout, kind, has_b in layers:
        wp = dev(rng.standard_normal((S_, 9, cout, cin)))
        bp = dev(rng.standard_normal((S_, cout)))
        shape = (cout, cin, 3, 3) if kind == E.KIND_CONV else (cin, cout, 3, 3)
        dw_b, dw_s = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
        db_b = torch.empty(cout, device="cuda") if has_b else None
        db_s = torch.empty(cout, device="cuda") if has_b else None
        items.append((wp, bp, S_, cin, cout, kind, dw_b, db_b))
        singles.append((wp, bp, S_, cin, cout, kind, dw_s, db_s))
    with E.batched_wgrad_reduce():
        for it in items:
            E._reduce_slices(*it)
    for it in singles:
        E._reduce_slices(*it)
    torch.cuda.synchronize()
    for (wp, bp, S_, cin, cout, kind, dwb, dbb), (*_, dws, dbs) in zip(items, singles):
        assert torch.equal(dwb, dws)
        if dbb is not None:
            assert torch.equal(dbb, dbs)
        ref = host(wp).sum(0)   # [tap][co][ci]
        ref = ref.transpose(1, 2, 0).reshape(cout, cin, 3, 3) if kind == E.KIND_CONV else \
            ref.transpose(2, 1, 0)[:, :, ::-1].reshape(cin, cout, 3, 3)
        assert np.abs(host(dwb) - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())


# ~2^-16.5 / ~2^-25 / ~2^-22.5 per product
SPLIT_TOL = {"bf16x3": 1e-4, "bf16x6": 2e-5, "f16x3": 2e-5}
FWD_PIECES = {"bf16x3": 2, "bf16x6": 3, "f16x3": E.PIECES_F16}


# the weight-scale sweep targets the fp16 pieces (bf16 has fp32's exponent range)
PREC_WSCALE = [("bf16x3", 0.1), ("bf16x6", 0.1)] + [("f16x3", w) for w in (0.1, 1e-3, 1e-5, 100.0)]


@pytest.mark.parametrize("prec,wscale", PREC_WSCALE)
@pytest.mark.parametrize("cin,cout,H,mode", [c for c in FWD_CASES if c[0] > 1 and c[2] >= 8])
def test_conv3x3_fwd_split_bf16(cuda, cin, cout, H, mode, prec, wscale):
    """Split forward == float64 oracle (bf16x3 within 1e-4, bf16x6 and f16x3 at 2e-5).
    wscale 1e-3 / 1e-5 / 100: weights far from 1, which fp16 pieces hold only through the
    pack's per-layer power-of-two scale (1e-5 unscaled would be subnormal in fp16, 100 x 256
    would overflow the old fixed x256 scale)."""
    if not N.call("ebsdvae_conv3x3_split_supported", H, H, cin, cout, FWD_PIECES[prec]):
        pytest.skip("shape not covered by the split kernel")
    rng = np.random.default_rng(31 + cin + cout + H + mode)
    B = 2
    s, mean, rstd, st = make_src(rng, B, H, cin, mode)
    w = rng.standard_normal((cout, cin, 3, 3)) * wscale
    b = rng.standard_normal(cout) * wscale
    layer = E.ConvLayer("t", E.KIND_CONV, cin, cout, H, mode, 0)
    old = E.get_precision()
    E.set_precision(prec)
    try:
        y, stt = E.conv_forward(dev(s), dev(st) if mode in (1, 2, 4) else None, layer, dev(w), dev(b), B)
    finally:
        E.set_precision(old)
    a = act_oracle(s, mean, rstd, mode)
    ref = O.conv3x3(a, w, b)
    assert O.rel_err(host(y), ref) < SPLIT_TOL[prec]
    _, rm, rr = O.instance_norm(ref)
    assert O.rel_err(host(stt)[..., 0], rm[:, 0, 0, :]) < 1e-4


@pytest.mark.parametrize("prec", ["bf16x6", "f16x3"])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("mode", [E.ACT_NORM_POOL, E.ACT_UP])
def test_conv3x3_split_8x8_partial_tiles(cuda, B, mode, prec):
    """8x8 maps run two whole images per tile (csrc/conv_split.hip plan_split); an odd batch
    leaves a half-empty last tile whose missing image must neither be read nor written."""
    if not N.call("ebsdvae_conv3x3_split_supported", 8, 8, 128, 128, 3):
        pytest.skip("8x8 split tiles need the pipelined kernel")
    rng = np.random.default_rng(61 + B + mode)
    s, mean, rstd, st = make_src(rng, B, 8, 128, mode)
    w = rng.standard_normal((128, 128, 3, 3)) * 0.05
    b = rng.standard_normal(128) * 0.1
    layer = E.ConvLayer("t", E.KIND_CONV, 128, 128, 8, mode, 0)
    with E.precision(prec):
        y, stt = E.conv_forward(dev(s), dev(st) if mode in (1, 2, 4) else None, layer, dev(w), dev(b), B,
                                keep_act=False)
    ref = O.conv3x3(act_oracle(s, mean, rstd, mode), w, b)
    assert O.rel_err(host(y), ref) < SPLIT_TOL[prec]
    _, rm, rr = O.instance_norm(ref)
    assert O.rel_err(host(stt)[..., 0], rm[:, 0, 0, :]) < 1e-4


@pytest.mark.parametrize("prec", ["bf16x3", "bf16x6"])
@pytest.mark.parametrize("cin,cout,H,pmode", [c for c in FUSED_CASES if c[2] >= 8])
def test_dgrad_fused_split_bf16(cuda, cin, cout, H, pmode, prec):
    rng = np.random.default_rng(41 + cin + cout + H + pmode)
    B = 2
    Hy = {E.P_ID: H, E.P_POOL: 2 * H, E.P_UP: H // 2}[pmode]
    y = rng.standard_normal((B, Hy, Hy, cin)) * 2 + 0.5
    xh, mean, rstd = O.instance_norm(y)
    st = np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)
    gy = rng.standard_normal((B, H, H, cout))
    wsrc = rng.standard_normal((cout, cin, 3, 3)) * 0.1
    layer = E.ConvLayer("t", E.KIND_CONV, cin, cout, H, E.ACT_RAW, 0)
    old = E.get_precision()
    E.set_precision(prec)
    try:
        y_d, st_d = dev(y), dev(st)
        gin, part = E.conv_dgrad(dev(gy), layer, dev(wsrc), prev=(y_d, st_d, pmode))
        g_prev = E.in_backward(gin, pmode, y_d, st_d, part=part)
        gin2 = E.conv_dgrad(dev(gy), layer, dev(wsrc))
    finally:
        E.set_precision(old)
    gn = O.conv3x3_dgrad(gy, wsrc)
    assert O.rel_err(host(gin), h_oracle(gn, xh, pmode)) < SPLIT_TOL[prec]
    assert O.rel_err(host(gin2), gn) < SPLIT_TOL[prec]
    a = O.lrelu(xh)
    if pmode == E.P_POOL:
        _, arg = O.maxpool2(a)
        ga = O.maxpool2_bwd(gn, arg)
    elif pmode == E.P_UP:
        ga = O.upsample2_bwd(gn)
    else:
        ga = gn
    ref = O.instance_norm_bwd(ga * O.lrelu_slope(xh), xh, rstd)
    assert O.rel_err(host(g_prev), ref) < 2e-4


def _pack_f16_dgrad(w_d, layer):
    import ctypes
    numel = N.call("ebsdvae_pack_split_bytes", layer.cout, layer.cin, E.PIECES_F16) // 4
    out = torch.empty(numel, dtype=torch.float32, device=w_d.device)
    d = (N.PackDesc * 1)(N.PackDesc(N.ptr(w_d), N.ptr(out), layer.cin, layer.cout, layer.kind, 1))
    N.call("ebsdvae_pack_conv_weights_split", ctypes.addressof(d), 1, E.PIECES_F16, N.stream())
    return E.PackedW(out, E.PIECES_F16)


@pytest.mark.parametrize("wscale", [0.1, 1e-5, 100.0])
@pytest.mark.parametrize("gscale", [1.0, 1e-7])
@pytest.mark.parametrize("cin,cout,H,pmode", [c for c in FUSED_CASES if c[2] >= 8])
def test_dgrad_fused_split_f16(cuda, cin, cout, H, pmode, gscale, wscale):
    """Split-fp16 input gradient (f16x3) == float64 oracle at 2e-5, with the gradient operand
    scaled per image from its maximum: images 1e3 apart in magnitude, and tiny gradients
    (1e-7: far below fp16's normal range unscaled).  Also pins the per-tile maxima that the
    InstanceNorm-backward apply emits (ebsdvae_in_bwd_apply_max)."""
    if not N.call("ebsdvae_conv3x3_split_supported", H, H, cout, cin, E.PIECES_F16):
        pytest.skip("shape not covered by the split kernel")
    rng = np.random.default_rng(43 + cin + cout + H + pmode)
    B = 3 if H == 8 else 2   # 8x8: two images per tile, the third one alone in its tile
    Hy = {E.P_ID: H, E.P_POOL: 2 * H, E.P_UP: H // 2}[pmode]
    y = rng.standard_normal((B, Hy, Hy, cin)) * 2 + 0.5
    xh, mean, rstd = O.instance_norm(y)
    st = np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)
    gy = rng.standard_normal((B, H, H, cout)) * gscale
    gy[1] *= 1e3
    wsrc = rng.standard_normal((cout, cin, 3, 3)) * wscale
    layer = E.ConvLayer("t", E.KIND_CONV, cin, cout, H, E.ACT_RAW, 0)
    with E.precision("f16x3"):
        y_d, st_d, w_d = dev(y), dev(st), dev(wsrc)
        wd = _pack_f16_dgrad(w_d, layer)
        g_d = dev(gy)
        g_d.ev_gmax = dev(np.abs(gy).reshape(B, -1).max(1, keepdims=True))
        gin, part = E.conv_dgrad(g_d, layer, w_d, prev=(y_d, st_d, pmode), wd=wd)
        g_prev = E.in_backward(gin, pmode, y_d, st_d, part=part)
        gin2 = E.conv_dgrad(g_d, layer, w_d, wd=wd)
        gmax = host(g_prev.ev_gmax)
    gn = O.conv3x3_dgrad(gy, wsrc)
    hn = h_oracle(gn, xh, pmode)
    for b in range(B):   # per image: the two differ by 1e3 in magnitude
        assert O.rel_err(host(gin)[b], hn[b]) < SPLIT_TOL["f16x3"], b
        assert O.rel_err(host(gin2)[b], gn[b]) < SPLIT_TOL["f16x3"], b
    a = O.lrelu(xh)
    if pmode == E.P_POOL:
        _, arg = O.maxpool2(a)
        ga = O.maxpool2_bwd(gn, arg)
    elif pmode == E.P_UP:
        ga = O.upsample2_bwd(gn)
    else:
        ga = gn
    ref = O.instance_norm_bwd(ga * O.lrelu_slope(xh), xh, rstd)
    for b in range(B):
        assert O.rel_err(host(g_prev)[b], ref[b]) < 2e-4, b
    assert np.array_equal(gmax.max(1), np.abs(host(g_prev)).reshape(B, -1).max(1))


@pytest.mark.parametrize("cin,cout,H", [(32, 64, 64), (64, 128, 32), (128, 128, 16), (128, 128, 8)])
def test_pooled_reduce_matches_window_reduce(cuda, cin, cout, H):
    """The fused InstanceNorm-backward reduce of a max-pooled block read from the pooled raw
    output in identity mode (engine.conv_dgrad(..., ypool=)) == the reduce over the 2x2
    windows of y (first argmax): the same input gradient bit for bit and the same finalized
    {m1, m2} (only the window maximum gets gradient, and x-hat at it is (ypool - mean) * rstd)."""
    rng = np.random.default_rng(61 + cin + cout + H)
    B = 2
    y = rng.standard_normal((B, 2 * H, 2 * H, cin)) * 2 + 0.5
    _, mean, rstd = O.instance_norm(y)
    st = np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)
    ypool = y.reshape(B, H, 2, H, 2, cin).max(axis=(2, 4))
    gy = rng.standard_normal((B, H, H, cout))
    wsrc = rng.standard_normal((cout, cin, 3, 3)) * 0.05
    layer = E.ConvLayer("t", E.KIND_CONV, cin, cout, H, E.ACT_RAW, 0)
    with E.precision("f16x3"):
        y_d, st_d, w_d = dev(y), dev(st), dev(wsrc)
        wd = _pack_f16_dgrad(w_d, layer)
        outs = []
        for yp in (None, dev(ypool)):
            g_d = dev(gy)
            g_d.ev_gmax = dev(np.abs(gy).reshape(B, -1).max(1, keepdims=True))
            gin, part = E.conv_dgrad(g_d, layer, w_d, prev=(y_d, st_d, E.P_POOL), wd=wd, ypool=yp)
            g_prev = E.in_backward(gin, E.P_POOL, y_d, st_d, part=part)
            torch.cuda.synchronize()
            outs.append((gin, g_prev))
    assert torch.equal(outs[0][0], outs[1][0])
    # {m1, m2} agree to the last bits of the double sums, so the applied gradient does too
    assert O.rel_err(host(outs[1][1]), host(outs[0][1])) < 1e-6


@pytest.mark.parametrize("prec", ["bf16x3", "bf16x6"])
@pytest.mark.parametrize("cin,cout,H,mode,kind", [c for c in WG_CASES if c[0] >= 32 and c[1] >= 32])
def test_conv_wgrad_split_bf16(cuda, cin, cout, H, mode, kind, prec):
    """Split-bf16 weight gradient == float64 oracle (bf16x3 within 1e-4, bf16x6 at fp32 grade)."""
    rng = np.random.default_rng(51 + cin + cout + H + mode)
    B = 3 if H <= 64 else 2
    s, mean, rstd, st = make_src(rng, B, H, cin, mode)
    gy = rng.standard_normal((B, H, H, cout))
    wshape = (cout, cin, 3, 3) if kind == 0 else (cin, cout, 3, 3)
    dw = torch.empty(wshape, device="cuda")
    db = torch.empty(cout, device="cuda")
    old = E.get_precision()
    E.set_precision(prec)
    try:
        if mode == E.ACT_NORM_POOL:
            layer = E.ConvLayer("t", E.KIND_CONV, cin, cout, H, mode, 0)
            wdummy = dev(np.zeros((cout, cin, 3, 3)))
            _, _, act = E.conv_forward(dev(s), dev(st), layer, wdummy, dev(np.zeros(cout)), B, keep_act=True)
            E.conv_wgrad(act, None, E.ACT_RAW, dev(gy), cin, cout, kind, dw, db)
        else:
            E.conv_wgrad(dev(s), dev(st) if mode in (1, 2, 4) else None, mode, dev(gy), cin, cout, kind, dw, db)
    finally:
        E.set_precision(old)
    a = act_oracle(s, mean, rstd, mode)
    rw, rb = O.conv3x3_wgrad(a, gy)
    if kind == 1:
        rw = rw.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]
    assert O.rel_err(host(dw), rw) < SPLIT_TOL[prec] * 2
    assert O.rel_err(host(db), rb) < 5e-5


@pytest.mark.parametrize("prec", ["bf16x3", "bf16x6"])
@pytest.mark.parametrize("cin,cout,H", [(32, 32, 128), (32, 64, 64), (64, 64, 64), (64, 128, 32),
                                        (128, 128, 32), (128, 128, 16)])
def test_conv3x3_split_pooled_output(cuda, cin, cout, H, prec):
    """ebsdvae_conv3x3_fwd_split_pooled (producer of a max-pooled layer): y is bit-identical
    to the plain split forward, ypool is exactly the 2x2 max of y, and the InstanceNorm
    statistics (grouped by row pairs) agree to rounding."""
    rng = np.random.default_rng(83 + cin + cout + H)
    B = 2
    s, mean, rstd, st = make_src(rng, B, H, cin, E.ACT_NORM)
    w = rng.standard_normal((cout, cin, 3, 3)) * 0.05
    b = rng.standard_normal(cout) * 0.1
    layer = E.ConvLayer("t", E.KIND_CONV, cin, cout, H, E.ACT_NORM, E.P_POOL)
    with E.precision(prec):
        wp = E.pack_weight(dev(w), layer, dgrad=False)
        if not E.pool_out_ok(layer, wp):
            pytest.skip("pooled epilogue needs the pipelined split kernel")
        y1, st1 = E.conv_forward(dev(s), dev(st), layer, dev(w), dev(b), B, wp=wp)
        y2, st2, yp = E.conv_forward(dev(s), dev(st), layer, dev(w), dev(b), B, wp=wp, pool_out=True)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)
    ref_pool = torch.nn.functional.max_pool2d(y1.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.equal(yp, ref_pool.contiguous())
    assert O.rel_err(host(st2), host(st1)) < 1e-5


@pytest.mark.parametrize("prec", ["bf16x3", "bf16x6"])
@pytest.mark.parametrize("cin,cout,H", [(32, 32, 128), (64, 32, 64), (128, 64, 32), (128, 128, 16)])
def test_dgrad_summed_upsample_adjoint(cuda, cin, cout, H, prec):
    """pmode P_UPSUM (decoder blocks feeding an upsampling consumer): the input gradient
    comes back already 2x2-summed at the previous block's resolution, with that block's
    InstanceNorm-backward reduce fused per window; the block gradient matches the oracle
    and the P_UP path."""
    rng = np.random.default_rng(97 + cin + cout + H)
    B = 2
    y = rng.standard_normal((B, H // 2, H // 2, cin)) * 2 + 0.5
    xh, mean, rstd = O.instance_norm(y)
    st = np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)
    gy = rng.standard_normal((B, H, H, cout))
    wsrc = rng.standard_normal((cout, cin, 3, 3)) * 0.1
    layer = E.ConvLayer("t", E.KIND_CONV, cin, cout, H, E.ACT_RAW, 0)
    with E.precision(prec):
        wd = E.pack_weight(dev(wsrc), layer, dgrad=True)
        if not N.call("ebsdvae_conv3x3_split_pool_ok", H, H, cout, cin, wd.pieces):
            pytest.skip("window epilogues need the pipelined split kernel")
        y_d, st_d = dev(y), dev(st)
        gsum, part = E.conv_dgrad(dev(gy), layer, dev(wsrc), prev=(y_d, st_d, E.P_UP), wd=wd,
                                  sum_up=True)
        assert gsum.shape == (B, H // 2, H // 2, cin)
        g_prev = E.in_backward(gsum, E.P_ID, y_d, st_d, part=part)
        gin, part2 = E.conv_dgrad(dev(gy), layer, dev(wsrc), prev=(y_d, st_d, E.P_UP), wd=wd)
        g_prev2 = E.in_backward(gin, E.P_UP, y_d, st_d, part=part2)
    gn = O.conv3x3_dgrad(gy, wsrc)
    ga = O.upsample2_bwd(gn)
    assert O.rel_err(host(gsum), h_oracle(gn, xh, E.P_UP, summed=True)) < SPLIT_TOL[prec]
    ref = O.instance_norm_bwd(ga * O.lrelu_slope(xh), xh, rstd)
    assert O.rel_err(host(g_prev), ref) < 2e-4
    assert O.rel_err(host(g_prev), host(g_prev2)) < 2e-4


WG_F16_CASES = [  # (cin, cout, H, source mode, kind): NORM, NORM_UP and pooled-RAW sources
    (32, 32, 128, E.ACT_NORM, 0), (32, 64, 64, E.ACT_NORM_POOL, 0), (64, 128, 32, E.ACT_NORM_POOL, 0),
    (128, 64, 32, E.ACT_NORM, 1), (64, 32, 64, E.ACT_NORM, 1), (32, 32, 128, E.ACT_NORM_UP, 1),
    (128, 128, 16, E.ACT_NORM_UP, 1), (64, 64, 64, E.ACT_NORM, 0), (128, 128, 32, E.ACT_NORM, 0),
]


@pytest.mark.parametrize("spike", [False, True])
@pytest.mark.parametrize("spread", [1.0, 1e3])
@pytest.mark.parametrize("gscale", [1.0, 1e-7])
@pytest.mark.parametrize("cin,cout,H,mode,kind", WG_F16_CASES)
def test_conv_wgrad_f16(cuda, cin, cout, H, mode, kind, gscale, spread, spike):
    """Split-fp16 weight gradient (ebsdvae_conv3x3_wgrad_f16, the f16x3 default) == float64
    oracle at 2e-5 norm-wise.  The gradient operand is scaled per slice by a power of two
    from the per-tile maxima (gmax); gscale 1e-7 puts the unscaled gradient far below fp16's
    normal range, and spread 1e3 makes the images of one slice 1e3 apart in magnitude
    (one scale per slice from the largest).  The activation operand is not scaled: it is a
    normalised activation, |xhat| <= sqrt(H*W - 1) by construction; spike puts one value per
    plane at that bound (all others near 0) to cover the widest range it can take."""
    if not N.call("ebsdvae_conv3x3_wgrad_split_slices", 2, H, H, cin, cout, E.PIECES_F16) > 0:
        pytest.skip("shape not covered by the f16 weight gradient")
    rng = np.random.default_rng(71 + cin + cout + H + mode)
    B = 3 if H <= 64 else 2
    s, mean, rstd, st = make_src(rng, B, H, cin, mode)
    if spike:
        s[:, 1, 2, :] = 1e6
        mean = s.mean(axis=(1, 2), keepdims=True)
        rstd = 1.0 / np.sqrt(s.var(axis=(1, 2), keepdims=True) + 1e-5)
        st = np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)
    gy = rng.standard_normal((B, H, H, cout)) * gscale
    gy[0] /= spread
    wshape = (cout, cin, 3, 3) if kind == 0 else (cin, cout, 3, 3)
    dw = torch.empty(wshape, device="cuda")
    db = torch.empty(cout, device="cuda")
    with E.precision("f16x3"):
        g_d = dev(gy)
        Tg = 4
        g_d.ev_gmax = dev(np.abs(gy).reshape(B, Tg, -1).max(2))   # per-tile maxima (row bands)
        if mode == E.ACT_NORM_POOL:
            layer = E.ConvLayer("t", E.KIND_CONV, cin, cout, H, mode, 0)
            wdummy = dev(np.zeros((cout, cin, 3, 3)))
            _, _, act = E.conv_forward(dev(s), dev(st), layer, wdummy, dev(np.zeros(cout)), B, keep_act=True)
            with E.record_launches() as launched:
                E.conv_wgrad(act, None, E.ACT_RAW, g_d, cin, cout, kind, dw, db, normalized=True)
        else:
            with E.record_launches() as launched:
                E.conv_wgrad(dev(s), dev(st), mode, g_d, cin, cout, kind, dw, db)
    assert "ebsdvae_conv3x3_wgrad_f16" in launched
    a = act_oracle(s, mean, rstd, mode)
    rw, rb = O.conv3x3_wgrad(a, gy)
    if kind == 1:
        rw = rw.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]
    assert O.rel_err(host(dw), rw) < SPLIT_TOL["f16x3"]
    assert O.rel_err(host(db), rb) < 5e-5


def test_f16_weight_pack_trailer_and_batch(cuda):
    """Split-fp16 packs: the batched PackSet launch == per-layer packs bit for bit (pieces and
    the per-layer weight-shift trailer), and the trailer holds k with max|w| 2^k in
    [2^11, 2^12) for weights of very different magnitudes."""
    plan = E.build_plan(32, 16, 128)
    rng = np.random.default_rng(19)
    params = {}
    for i, L in enumerate(plan.enc + plan.dec):
        shape = (L.cout, L.cin, 3, 3) if L.kind == E.KIND_CONV else (L.cin, L.cout, 3, 3)
        params[L.name + ".weight"] = dev(rng.standard_normal(shape) * 10.0 ** (i % 7 - 4))
    with E.precision("f16x3"):
        packs = E.PackSet(plan, params).refresh()
        for L in plan.enc[1:] + plan.dec:
            w = params[L.name + ".weight"]
            pf, pd = packs[L.name]
            single = E.pack_weight(w, L, dgrad=False)
            assert pf.pieces == single.pieces and torch.equal(pf.t, single.t), L.name
            if pf.pieces == E.PIECES_F16:
                body = (L.cin // 8) * 10 * 2 * L.cout * 8 * 2   # bytes before the trailer
                k = int(pf.t.view(torch.int32)[body // 4])
                m = float(w.abs().max())
                assert 2.0 ** 11 <= m * 2.0 ** k < 2.0 ** 12, (L.name, m, k)
            if pd is not None:
                single = E.pack_weight(w, L, dgrad=True, scaled=True)
                assert pd.pieces == single.pieces and torch.equal(pd.t, single.t), L.name


@pytest.mark.parametrize("B,H,cin,cout,mode", [(3, 16, 128, 128, 1), (5, 8, 128, 128, 1),
                                               (256, 32, 64, 128, 2), (2, 128, 32, 32, 1)])
def test_fused_stats_finalize_bitwise(cuda, B, H, cin, cout, mode):
    """ebsdvae_conv3x3_fwd_split_st == ebsdvae_conv3x3_fwd_split + ebsdvae_in_stats_finalize
    bit for bit, whether the persistent blocks finalize their own images in-kernel (16x16,
    8x8 two-image tiles, B=256 at 32x32) or the standalone kernel runs (B=2 at 128x128)."""
    rng = np.random.default_rng(83 + B + H)
    s, mean, rstd, st = make_src(rng, B, H, cin, mode)
    w = dev(rng.standard_normal((cout, cin, 3, 3)) * 0.05)
    b = dev(rng.standard_normal(cout) * 0.1)
    layer = E.ConvLayer("t", E.KIND_CONV, cin, cout, H, mode, 0)
    with E.precision("f16x3"):
        wp = E.pack_weight(w, layer, dgrad=False)
    assert wp.pieces == E.PIECES_F16
    src, sst = dev(s), dev(st)
    T = N.call("ebsdvae_conv3x3_split_stat_tiles", H, H, cout)
    outs = []
    for fused in (True, False):
        y = torch.empty(B, H, H, cout, device=cuda)
        part = torch.empty(B, T, cout, 2, device=cuda)
        stt = torch.full((B, cout, 2), float("nan"), device=cuda)
        if fused:
            N.call("ebsdvae_conv3x3_fwd_split_st", N.ptr(src), N.ptr(sst), mode, N.ptr(wp.t), N.ptr(b),
                   N.ptr(y), None, N.ptr(part), N.ptr(stt), B, H, H, cin, cout, wp.pieces, N.stream())
        else:
            N.call("ebsdvae_conv3x3_fwd_split", N.ptr(src), N.ptr(sst), mode, N.ptr(wp.t), N.ptr(b),
                   N.ptr(y), N.ptr(part), None, B, H, H, cin, cout, wp.pieces, N.stream())
            N.call("ebsdvae_in_stats_finalize", N.ptr(part), N.ptr(stt), B, cout, T, (H * H) // T,
                   N.stream())
        outs.append((y, stt))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])   # no NaN left: every image finalized


@pytest.mark.parametrize("B,H,cin,cout,pmode", [(3, 16, 128, 128, 0), (256, 32, 64, 128, 1),
                                                (2, 128, 32, 32, 0), (4, 32, 128, 128, 2)])
def test_fused_bwd_finalize_bitwise(cuda, B, H, cin, cout, pmode):
    """ebsdvae_conv3x3_dgrad_inbwd_f16_bst == ebsdvae_conv3x3_dgrad_inbwd_f16 +
    ebsdvae_in_bwd_finalize bit for bit (gin, the reduce partials and bst), in-kernel
    (16x16; B=256 at 32x32 with the max-pool routing) and standalone (B=2 at 128x128)."""
    rng = np.random.default_rng(89 + B + H + pmode)
    Hp = {0: H, 1: 2 * H, 2: H // 2}[pmode]   # the previous block's resolution
    gy = rng.standard_normal((B, H, H, cout)).astype(np.float32)
    yp = rng.standard_normal((B, Hp, Hp, cin)).astype(np.float32)
    stp = np.stack([yp.mean(axis=(1, 2)), 1.0 / np.sqrt(yp.var(axis=(1, 2)) + 1e-5)], -1)
    w = dev(rng.standard_normal((cout, cin, 3, 3)) * 0.05)
    layer = E.ConvLayer("t", E.KIND_CONV, cin, cout, H, 1, 0)
    with E.precision("f16x3"):
        wd = E.pack_weight(w, layer, dgrad=True, scaled=True)
    assert wd.pieces == E.PIECES_F16
    g, y_prev, st_prev = dev(gy), dev(yp), dev(stp)
    gmax = g.abs().reshape(B, 4, -1).amax(2).contiguous()
    T = N.call("ebsdvae_conv3x3_split_stat_tiles", H, H, cin)
    outs = []
    for fused in (True, False):
        gin = torch.empty(B, H, H, cin, device=cuda)
        part = torch.empty(B, T, cin, 2, dtype=torch.float64, device=cuda)
        bst = torch.full((B, cin, 2), float("nan"), device=cuda)
        if fused:
            N.call("ebsdvae_conv3x3_dgrad_inbwd_f16_bst", N.ptr(g), N.ptr(gmax), 4, N.ptr(wd.t),
                   N.ptr(gin), N.ptr(y_prev), N.ptr(st_prev), pmode, part.data_ptr(), N.ptr(bst),
                   Hp * Hp, B, H, H, cout, cin, N.stream())
        else:
            N.call("ebsdvae_conv3x3_dgrad_inbwd_f16", N.ptr(g), N.ptr(gmax), 4, N.ptr(wd.t), N.ptr(gin),
                   N.ptr(y_prev), N.ptr(st_prev), pmode, part.data_ptr(), B, H, H, cout, cin, N.stream())
            N.call("ebsdvae_in_bwd_finalize", part.data_ptr(), N.ptr(bst), B, cin, T, Hp * Hp, N.stream())
        outs.append((gin, part, bst))
    torch.cuda.synchronize()
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("mfma", [True, False], ids=["mfma", "valu"])
def test_network_end_matches_oracle(cuda, monkeypatch, H, mfma):
    """ebsdvae_net_end (the training step's network end in one pass over y13): x_hat of the final
    conv, the mean-BCE logit gradient g1, the per-band BCE sums, the last block's
    InstanceNorm-backward reduce (finalized here) and the final conv's gradient slices, against
    the float64 oracle; then the apply pass it feeds gives the block's output gradient.  Both
    forms: the split-fp16 MFMA kernel (default, round 6) and the fp32 VALU kernel (round 5)."""
    monkeypatch.setattr(E, "_NET_END_MFMA", mfma)
    check_network_end(H, H)


def net_end_targets(u, kind, H):
    """BCE targets (B, 1, H, W) from uniform draws u in [0, 1), for check_network_end:
      unit  floor(u 255) / 255, the 8-bit patterns every other test feeds;
      u8    floor(u 256), an unnormalised batch 0...255;
      neg   uniform in [-3, 4);
      hot   unit, with 255 at columns 0 and W - 1 of rows 0, e - 1, e and H - 1, e the first
            band edge (the first row of the second band; on a one-band map H - 1)."""
    if kind == "u8":
        return np.floor(u * 256)
    if kind == "neg":
        return u * 7 - 3
    x = np.floor(u * 255) / 255
    if kind == "hot":
        T = H // (64 if H % 64 == 0 else 32)
        e = H // T if T > 1 else H - 1
        for r in (0, e - 1, e, H - 1):
            x[:, 0, r, 0] = x[:, 0, r, -1] = 255.0
    else:
        assert kind == "unit", kind
    return x


def check_network_end(H, W, ops=E, with_b14=True, with_g_loss=True, *, targets="unit", wscale=1.0,
                      g_loss_value=1.0, planes=False, B=3):
    """The body of test_network_end_matches_oracle on an (H, W) map.  ops supplies network_end
    and in_backward_final_from (the engine's, or a caller's own with the engine's signatures:
    tests/test_gpu_rect.py calls the C ABI on guarded buffers); without b14 / g_loss the entry
    point gets NULL (bias 0, loss gradient 1).  The keyword arguments shape the inputs
    (tests/test_gpu_net_end_range.py; the defaults are the draws of the tests above): targets as
    net_end_targets, w14 times wscale, the loss gradient g_loss_value, and with planes two
    degenerate planes in image 0 of y13: channel 5 one pixel 1 among zeros (xhat ~ 90 there, the
    rest on the slope branch at -1e-2), channel 7 constant (variance 0, xhat = 0 everywhere)."""
    rng = np.random.default_rng(33)
    C = 32
    y = rng.standard_normal((B, H, W, C)) * 1.3 - 0.4
    if planes:
        y[0, :, :, 5] = 0.0
        y[0, H // 2, W - 1, 5] = 1.0
        y[0, :, :, 7] = 0.25
    xh, mean, rstd = O.instance_norm(y)
    st = np.stack([mean[:, 0, 0, :], rstd[:, 0, 0, :]], -1)
    w14 = rng.standard_normal((1, C, 3, 3)) * 0.15 * wscale
    b14 = np.array([0.07 if with_b14 else 0.0])
    x = net_end_targets(rng.random((B, 1, H, W)), targets, H)
    scale = 0.5
    P = H * W
    T = N.call("ebsdvae_net_end_tiles", H, W)
    assert T == H // (64 if H % 64 == 0 else 32)   # 64-row bands where H allows
    plan = E.build_plan()
    params = {"decoder.14.weight": dev(w14), "decoder.14.bias": dev(b14) if with_b14 else None}
    saved = {plan.dec[-1].name: (dev(y), dev(st))}
    g_loss = torch.full((), g_loss_value, device="cuda") if with_g_loss else None
    gl = float(np.float32(g_loss_value)) if with_g_loss else 1.0
    x_hat, end = ops.network_end(plan, saved, params, dev(x), g_loss=g_loss, scale=scale)
    a = O.lrelu(xh)
    if planes:   # the constant plane is exactly 0 after the norm, on the slope branch
        assert (xh[0, :, :, 7] == 0).all() and xh[0, H // 2, W - 1, 5] > 80
    ref_xhat = O.conv3x3(a, w14, b14)[..., 0]                     # (B, H, W)
    # sigmoid and BCE in the overflow-safe form of O.vae_loss
    sig = np.exp(-np.logaddexp(0.0, -ref_xhat))
    ref_g1 = gl * scale / (B * P) * (sig - x[:, 0])
    bce = (1 - x[:, 0]) * ref_xhat + np.logaddexp(0.0, -ref_xhat)
    got = {"x_hat": host(x_hat), "g1": host(end.g1), "bce": host(end.bce), "part": host(end.part),
           "wpart": host(end.wpart), "bpart": host(end.bpart)}
    bad = [k for k, v in got.items() if not np.isfinite(v).all()]
    assert not bad, f"non-finite outputs: {bad}"
    assert O.rel_err(got["x_hat"][:, 0], ref_xhat) < 2e-5
    assert O.rel_err(got["g1"], ref_g1) < 2e-5
    ref_bce = bce.reshape(B, T, -1).sum(-1)
    assert O.rel_err(got["bce"], ref_bce) < 1e-5
    # reduce sums of the last block, finalized, and the apply that consumes them
    ga = O.conv3x3_dgrad(ref_g1[..., None], w14)
    gxs = ga * O.lrelu_slope(xh)
    s1 = gxs.reshape(B, T, -1, C).sum(2)
    s2 = (gxs * xh).reshape(B, T, -1, C).sum(2)
    part = got["part"]
    print(f"\nnet_end {H}x{W}: s1 {O.rel_err(part[..., 0], s1):.2e} s2 {O.rel_err(part[..., 1], s2):.2e}")
    assert O.rel_err(part[..., 0], s1) < 1e-4 and O.rel_err(part[..., 1], s2) < 1e-4
    dw = torch.empty(1, C, 3, 3, device="cuda")
    db = torch.empty(1, device="cuda")
    gy = ops.in_backward_final_from(end, dev(w14), dev(y), dev(st), dw, db)
    ref_gy = O.instance_norm_bwd(gxs, xh, rstd)
    rw, rb = O.conv3x3_wgrad(a, ref_g1[..., None])
    print(f"net_end: gy {O.rel_err(host(gy), ref_gy):.2e} dW14 {O.rel_err(host(dw), rw):.2e} "
          f"db14 {O.rel_err(host(db), rb):.2e}")
    assert np.isfinite(host(gy)).all() and np.isfinite(host(dw)).all() and np.isfinite(host(db)).all()
    assert O.rel_err(host(gy), ref_gy) < 1e-4
    assert O.rel_err(host(dw), rw) < 5e-5
    assert O.rel_err(host(db), rb) < 5e-5
    if gl == 0:   # rel_err has a floor: a zero loss gradient gives exact zeros
        for k in ("g1", "part", "wpart", "bpart"):
            assert (got[k] == 0).all(), k
        assert (host(gy) == 0).all() and (host(dw) == 0).all() and (host(db) == 0).all()
    # the loss values from the band sums
    z = rng.standard_normal((B, 16)); mu = rng.standard_normal((B, 16)) * 0.3
    sd = np.exp(rng.standard_normal((B, 16)) * 0.2)
    (loss, klm, recm), (elbo, kl, rec) = E.loss_forward_parts(end, dev(z), dev(mu), dev(sd), 5e-6, P)
    ref = O.vae_loss(ref_xhat[:, None], x, z, mu, sd, 5e-6)
    assert abs(float(loss) - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    assert O.rel_err(host(elbo), ref["elbo"]) < 1e-5
