"""The direct-call surface of the middle of the model against float64 restatements
(tests/heads_ref.py): the autograd wrappers users reach by calling submodules (LinearFn,
ReparamFn, KLFn of latice/functional.py: model.mu / .logvar / .linear2 / .reparameterize), the
composed path encoder -> mu / logvar -> reparameterize -> linear2 -> decoder against the fused
forward, the Philox sampler value by value, and ebsdvae_adam.  Inputs are rounded to float32
before the reference sees them; errors are norm-wise (O.rel_err) unless stated.
"""
import functools

import numpy as np
import pytest
import torch

import heads_ref as H
import pinned
from latice import _native as N
from latice import engine as E
from latice import functional as Fn
from latice.model import HipLinear, VariationalAutoEncoderRawData
from oracle import vae_oracle as O

pytestmark = pytest.mark.gpu


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().requires_grad_(grad)


def host(t):
    return t.detach().double().cpu().numpy()


# ----------------------------------------------------------------------------- LinearFn
LIN_FWD, LIN_BWD = 1e-5, 1e-4     # the heads' gates, for the same contraction lengths
LIN_SHAPES = [(1, 1, 1), (3, 2048, 16), (5, 16, 2048), (257, 33, 7)]


@functools.lru_cache(maxsize=None)
def linear_case(M, K, Nn):
    rng = np.random.default_rng(101 * M + 7 * K + Nn)
    c = {"x": H.f32(rng.standard_normal((M, K))), "w": H.f32(rng.standard_normal((Nn, K)) / np.sqrt(K)),
         "b": H.f32(rng.standard_normal(Nn) * 0.1), "gy": H.f32(rng.standard_normal((M, Nn)))}
    c["y"] = c["x"] @ c["w"].T + c["b"]
    return c


def linear_grads(c, gy):
    return {"x": gy @ c["w"], "w": gy.T @ c["x"], "b": gy.sum(0)}


def check(label, got, ref, gate):
    e = O.rel_err(host(got), ref)
    print(f"{label}: {e:.2e} (gate {gate:g})")
    assert e < gate, (label, e)


@pytest.mark.parametrize("M,K,Nn", LIN_SHAPES)
def test_linear_fn_forward_backward(cuda, M, K, Nn):
    c = linear_case(M, K, Nn)
    x, w, b = dev(c["x"], True), dev(c["w"], True), dev(c["b"], True)
    y = Fn.LinearFn.apply(x, w, b)
    assert y.shape == (M, Nn)
    (y * dev(c["gy"])).sum().backward()
    check(f"linear {M, K, Nn} y", y, c["y"], LIN_FWD)
    for k, t in (("x", x), ("w", w), ("b", b)):
        assert t.grad.shape == t.shape
        check(f"linear {M, K, Nn} g{k}", t.grad, linear_grads(c, c["gy"])[k], LIN_BWD)


LIN_VARIANTS = ["3d", "x-transposed", "expanded-grad", "transposed-grad", "x-only", "w-frozen",
                "b-frozen", "no-bias"]


@pytest.mark.parametrize("variant", LIN_VARIANTS)
def test_linear_fn_variants(cuda, monkeypatch, variant):
    """The ways autograd reaches LinearFn: a 3-D input, non-contiguous inputs and incoming
    gradients, every requires_grad subset (a gradient nobody asked for is not computed:
    ebsdvae_linear_bwd gets NULL for it) and HipLinear(bias=False)."""
    M, K, Nn = 6, 33, 7
    c = linear_case(M, K, Nn)
    calls = []
    real_call = N.call

    def spy(name, *args):
        calls.append((name, args))
        return real_call(name, *args)

    monkeypatch.setattr(Fn.N, "call", spy)
    need = {"x": True, "w": variant not in ("x-only", "w-frozen"),
            "b": variant not in ("x-only", "b-frozen", "no-bias")}
    lin = HipLinear(K, Nn, bias=variant != "no-bias").cuda()
    with torch.no_grad():
        lin.weight.copy_(dev(c["w"]))
        if lin.bias is not None:
            lin.bias.copy_(dev(c["b"]))
    lin.weight.requires_grad_(need["w"])
    if lin.bias is not None:
        lin.bias.requires_grad_(need["b"])
    y_ref = c["y"] if variant != "no-bias" else c["x"] @ c["w"].T
    gy_ref = c["gy"]
    leaf = dev(c["x"], True)
    x = leaf
    if variant == "3d":
        leaf = dev(c["x"].reshape(2, 3, K), True)
        x = leaf
    elif variant == "x-transposed":
        leaf = dev(c["x"].T, True)      # (K, M) contiguous
        x = leaf.t()
        assert not x.is_contiguous()
    y = lin(x)
    if variant == "3d":
        assert y.shape == (2, 3, Nn)
    else:
        assert y.shape == (M, Nn)
    if variant == "expanded-grad":
        gy_ref = np.ones((M, Nn))
        y.sum().backward()              # autograd delivers an expanded (stride 0) gradient
    elif variant == "transposed-grad":
        mt = dev(c["gy"].T)             # (Nn, M): y * mt.t() hands back a transposed gradient
        (y * mt.t()).sum().backward()
    else:
        (y * dev(c["gy"]).reshape(y.shape)).sum().backward()
    check(f"linear[{variant}] y", y.reshape(M, Nn), y_ref, LIN_FWD)
    g = linear_grads(c, gy_ref)
    assert leaf.grad.shape == leaf.shape
    gx = leaf.grad.t() if variant == "x-transposed" else leaf.grad.reshape(M, K)
    check(f"linear[{variant}] gx", gx, g["x"], LIN_BWD)
    for k, p in (("w", lin.weight), ("b", lin.bias)):
        if need[k]:
            check(f"linear[{variant}] g{k}", p.grad, g[k], LIN_BWD)
        elif p is not None:
            assert p.grad is None, k
    (bwd,) = [a for n, a in calls if n == "ebsdvae_linear_bwd"]
    gx_ptr, gw_ptr, gb_ptr = bwd[3:6]
    assert gx_ptr is not None
    assert (gw_ptr is not None) == need["w"] and (gb_ptr is not None) == need["b"]


# ----------------------------------------------------------------------------- ReparamFn
REPARAM_GATE = 1e-6   # elementwise: a few roundings and one expf


def reparam_case(shape, logvar=None):
    rng = np.random.default_rng(int(np.prod(shape)) + 5)
    mu, eps, gz = (H.f32(rng.standard_normal(shape)) for _ in range(3))
    lv = H.f32(rng.standard_normal(shape)) if logvar is None else H.f32(np.resize(logvar, shape))
    std = np.exp(lv / 2)
    return {"mu": mu, "lv": lv, "eps": eps, "gz": gz, "std": std, "z": mu + eps * std,
            "g_mu": gz, "g_lv": gz * eps * std / 2}


@pytest.mark.parametrize("shape,logvar", [((1,), None), ((255,), None), ((256,), None), ((257,), None),
                                          ((5, 64), None), ((3, 50), (-80.0, 0.0, 80.0))],
                         ids=["1", "255", "256", "257", "5x64", "logvar-80-0-80"])
def test_reparam_fn_forward_backward(cuda, shape, logvar):
    """z = mu + eps exp(logvar / 2) and its adjoints; logvar = -80 / 80 puts std at 4e-18 /
    2e+17, tiny or huge but finite in float32."""
    c = reparam_case(shape, logvar)
    mu, lv = dev(c["mu"], True), dev(c["lv"], True)
    z = Fn.ReparamFn.apply(mu, lv, dev(c["eps"]))
    assert z.shape == shape and torch.isfinite(z).all()
    (z * dev(c["gz"])).sum().backward()
    check(f"reparam {shape} z", z, c["z"], REPARAM_GATE)
    check(f"reparam {shape} g_mu", mu.grad, c["g_mu"], REPARAM_GATE)
    check(f"reparam {shape} g_logvar", lv.grad, c["g_lv"], REPARAM_GATE)
    if logvar is not None:   # norm-wise errors see the huge std only: each logvar on its own
        for v in logvar:
            sel = c["lv"] == v
            mask = torch.from_numpy(sel)
            check(f"reparam logvar {v} z", z.detach().cpu()[mask], c["z"][sel], REPARAM_GATE)
            check(f"reparam logvar {v} g_logvar", lv.grad.cpu()[mask], c["g_lv"][sel], REPARAM_GATE)


def test_reparam_bwd_direct_branches(cuda):
    """ebsdvae_reparam_bwd with the arguments the wrapper never passes: a std gradient
    (g_logvar = (g_std + g_z eps) std / 2) and NULL for either output."""
    n = 257
    c = reparam_case((n,))
    rng = np.random.default_rng(9)
    gstd = H.f32(rng.standard_normal(n))
    std32 = H.f32(c["std"])               # the kernel reads the saved float32 std
    t = {k: dev(v) for k, v in (("gz", c["gz"]), ("gstd", gstd), ("eps", c["eps"]), ("std", std32))}
    nan = lambda: torch.full((n,), float("nan"), device="cuda")   # noqa: E731
    gmu, glv = nan(), nan()
    N.call("ebsdvae_reparam_bwd", N.ptr(t["gz"]), N.ptr(t["gstd"]), N.ptr(t["eps"]), N.ptr(t["std"]),
           N.ptr(gmu), N.ptr(glv), n, N.stream())
    check("reparam_bwd g_mu", gmu, c["gz"], REPARAM_GATE)
    ref_glv = (gstd + c["gz"] * c["eps"]) * std32 / 2
    check("reparam_bwd g_logvar with g_std", glv, ref_glv, REPARAM_GATE)
    glv2 = nan()
    N.call("ebsdvae_reparam_bwd", N.ptr(t["gz"]), N.ptr(t["gstd"]), N.ptr(t["eps"]), N.ptr(t["std"]),
           None, N.ptr(glv2), n, N.stream())
    assert torch.equal(glv2, glv)
    gmu2 = nan()
    N.call("ebsdvae_reparam_bwd", N.ptr(t["gz"]), N.ptr(t["gstd"]), N.ptr(t["eps"]), N.ptr(t["std"]),
           N.ptr(gmu2), None, n, N.stream())
    assert torch.equal(gmu2, gmu)


# ----------------------------------------------------------------------------- KLFn
def test_kl_fn_backward_with_per_sample_gradient(cuda):
    """KLFn.backward under a non-uniform upstream gradient g (B,), against the float64 gradient
    of mean_j [0.5 z^2 - 0.5 ((z - mu) / std)^2 - log std], at the 1e-5 gates of
    test_vae_loss_forward_backward."""
    B, L = 37, 16
    rng = np.random.default_rng(3)
    mu = H.f32(rng.standard_normal((B, L)))
    std = H.f32(np.exp(rng.standard_normal((B, L)) * 0.3))
    z = H.f32(mu + rng.standard_normal((B, L)) * std)
    g = H.f32(rng.standard_normal(B))
    zz, mm, ss = dev(z, True), dev(mu, True), dev(std, True)
    kl = Fn.KLFn.apply(zz, mm, ss)
    assert kl.shape == (B,)
    (kl * dev(g)).sum().backward()
    check("kl", kl, (0.5 * z ** 2 - 0.5 * ((z - mu) / std) ** 2 - np.log(std)).mean(-1), 2e-5)
    gb = g[:, None] / L
    check("kl g_z", zz.grad, gb * (z - (z - mu) / std ** 2), 1e-5)
    check("kl g_mu", mm.grad, gb * (z - mu) / std ** 2, 1e-5)
    check("kl g_std", ss.grad, gb * ((z - mu) ** 2 / std ** 3 - 1 / std), 1e-5)


# ----------------------------------------------------------------------------- composed == fused
def test_composed_direct_calls_equal_the_fused_forward(cuda):
    """encoder -> flatten -> mu / logvar -> ReparamFn -> linear2 -> decoder (the reference's
    latent_embedding usage, with gradients) against the model's fused forward on vae128_b4,
    under s = x_hat.mean() + z^2.mean() + mu^2.mean() + std.mean().  The fused run (checked
    against the fixture in test_gpu_model.py) is the anchor.  Outputs: the model-level 1e-4.
    Parameter gradients: the gates tests/pinned.py applies to that parameter -- the state-pinned
    1e-4, and for the conv biases feeding an InstanceNorm (analytically zero) the two residues
    differ by at most ZERO_BIAS_K x 2^-24 x A_c, A_c = sum |gy| of the float64 oracle under s.

    The two runs are float32 evaluations of one function only where their LeakyReLU branches
    agree: the composed dec_in differs from the fused one in the last bits, and on MI355X 4 of
    the decoder's 4.8 million branch decisions came out the other way (1 in block 4, 3 in block
    8; 5 under fp32 and bf16x6).  Under this s the decoder's gradient is the adjoint of a
    constant map, which InstanceNorm's backward strips of its mean: what is left is mostly the
    branch pattern, and those 4 decisions moved linear2's and the decoder's weight gradients by
    6.1e-3 ... 9.9e-3 of their scale while each run sat 2e-5 ... 5e-5 from the float64 oracle
    pinned to its own decisions.  So the oracle's own answer to the differing decisions,
    oracle(composed's pins) - oracle(fused's pins) -- exactly zero where the decisions agree --
    is taken out of composed - fused before the 1e-4 gate is applied (measured: <= 1.8e-5 on
    every parameter); the direct figure is printed beside it."""
    name = "vae128_b4"
    f, sd = pinned.fixture(name)
    Bn, S, L, _, _ = (int(v) for v in f["meta"])
    m = VariationalAutoEncoderRawData(32, L, S)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(cuda).train()
    x = torch.from_numpy(f["x"]).to(cuda)
    eps = torch.from_numpy(f["eps"]).to(cuda)

    def scalar(x_hat, z, mu, std):
        return x_hat.mean() + z.square().mean() + mu.square().mean() + std.mean()

    with E.record_state() as rec_f:
        z, x_hat, mu, std = m(x, eps=eps)
    scalar(x_hat, z, mu, std).backward()
    fused = {"x_hat": x_hat, "z": z, "mu": mu, "std": std}
    g_fused = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)

    with E.record_state() as rec_c:
        enc = m.encoder(x)
        flat = enc.flatten(1, -1)
        mu_c, lv = m.mu(flat), m.logvar(flat)
        z_c = Fn.ReparamFn.apply(mu_c, lv, eps)
        x_hat_c = m.decoder(m.linear2(z_c).view(-1, 128, 4, 4))
    std_c = (lv / 2).exp()
    scalar(x_hat_c, z_c, mu_c, std_c).backward()
    torch.cuda.synchronize()
    for k, t in (("x_hat", x_hat_c), ("z", z_c), ("mu", mu_c), ("std", std_c)):
        check(f"composed vs fused {k}", t, host(fused[k]), 1e-4)
    for k, t in (("mu", mu_c), ("std", std_c), ("z", z_c)):
        check(f"composed vs fixture {k}", t, f[k], 1e-4)

    # the float64 oracle's backward of the same scalar under either run's decisions
    outs, cache64 = pinned.oracle_fp64(name)
    up = {"x_hat": np.full((Bn, S, S, 1), 1.0 / (Bn * S * S)), "z": 2 * outs["z"] / (Bn * L),
          "mu": 2 * outs["mu"] / (Bn * L), "std": np.full((Bn, L), 1.0 / (Bn * L))}
    pins_f = O.pins_from_blocks(*pinned.blocks(m.plan, rec_f))
    pins_c = O.pins_from_blocks(*pinned.blocks(m.plan, rec_c))
    apart = {k: int((pins_f[k][0] != pins_c[k][0]).sum()) for k in pins_f}
    print(f"    LeakyReLU decisions apart: { {k: v for k, v in apart.items() if v} }")
    absum = {}
    ref_f = O.backward(cache64, f["x"], 0.0, pins=pins_f, absum=absum, upstream=up)
    ref_c = ref_f if not any(apart.values()) else O.backward(cache64, f["x"], 0.0, pins=pins_c, upstream=up)
    kz = pinned.ZERO_BIAS_K[E.get_precision()]
    fails = []
    for n, p in m.named_parameters():
        gc, gf = host(p.grad), host(g_fused[n])
        if n in pinned.ZERO_GRAD_BIAS:
            a = float((np.abs(gc - gf) / (pinned.U32 * np.maximum(absum[n], 1e-300))).max())
            print(f"    {n:22s} residues apart {a:.2f} x 2^-24 A (gate {kz:g})")
            if a > kz:
                fails.append((n, a))
        else:
            e = O.rel_err(gc - (ref_c[n] - ref_f[n]), gf)
            print(f"    {n:22s} composed vs fused {e:.2e} (as computed {O.rel_err(gc, gf):.2e}); "
                  f"vs float64: fused {O.rel_err(gf, ref_f[n]):.2e} composed {O.rel_err(gc, ref_c[n]):.2e}")
            if e > pinned.STATE_GATE:
                fails.append((n, e))
    assert not fails, fails


# ----------------------------------------------------------------------------- sampler
# Largest |float32 restatement - float64 restatement| of the chain (heads_ref.normal_ref) over
# the seeds x offsets below at n = 2^20 + 3, and its 99.9 % quantile (the worst of the 16
# draws each).  The outliers are u0 next to 1, where the radius is tiny and du / r is large.
SAMPLER_F32_MAX, SAMPLER_F32_Q999 = 4.31e-5, 1.05e-6
SAMPLER_GATE, SAMPLER_GATE_Q999 = 4 * SAMPLER_F32_MAX, 4 * SAMPLER_F32_Q999
SAMPLER_N = [1, 2, 3, 5, 1027, 2 ** 20 + 3]
SAMPLER_SEEDS = [0, 1234, 2 ** 40 + 3, 2 ** 64 - 1]
SAMPLER_OFFSETS = [0, 3, 2 ** 32 - 2, 2 ** 63]
PAD = 8


def fill(n, seed, offset=0, counter=None):
    """E.normal_ into the first n of n + PAD NaNs; the NaNs behind must survive."""
    buf = torch.full((n + PAD,), float("nan"), device="cuda")
    E.normal_(buf[:n], seed, offset, counter=counter)
    torch.cuda.synchronize()
    assert torch.isnan(buf[n:]).all(), "normal_fill wrote past n"
    assert not torch.isnan(buf[:n]).any(), "normal_fill left draws unwritten"
    return buf[:n]


@pytest.mark.parametrize("offset", SAMPLER_OFFSETS)
@pytest.mark.parametrize("seed", SAMPLER_SEEDS)
def test_normal_fill_matches_philox_restatement(cuda, seed, offset):
    """Every draw against the float64 restatement of Philox4x32-10 + Box-Muller, for n of every
    tail length n % 4, one past a block and 2^20 + 3; offset 2^32 - 2 carries the counter's low
    word into the high one inside the call, 2^63 sets its top bit.
    Gate: the float32 numpy restatement of the same chain lies within 4.31e-5 of the float64 one
    over these seeds and offsets at n = 2^20 + 3 (99.9 % of the draws within 1.05e-6); the
    device's logf / cosf / sinf are not numpy's, so the GPU is held to 4 x that: 1.72e-4 on
    every draw and 4.2e-6 on the 99.9 % quantile."""
    ref = H.normal_ref(SAMPLER_N[-1], seed, offset)   # without a counter, n draws are a prefix
    for n in SAMPLER_N:
        d = np.abs(host(fill(n, seed, offset)) - ref[:n])
        if n == SAMPLER_N[-1]:
            print(f"normal_fill seed {seed} offset {offset}: max {d.max():.2e} (gate {SAMPLER_GATE:.2e}) "
                  f"q99.9 {np.quantile(d, 0.999):.2e} (gate {SAMPLER_GATE_Q999:.2e})")
            assert np.quantile(d, 0.999) < SAMPLER_GATE_Q999
        assert d.max() < SAMPLER_GATE, (n, d.max())


@pytest.mark.parametrize("k", [3, 1000])
def test_normal_fill_offset_identity(cuda, k):
    """fill(n, seed, offset = k) == fill(n + 4 k, seed, 0)[4 k:], bit for bit."""
    n, seed = 1027, 2 ** 40 + 3
    assert torch.equal(fill(n, seed, k), fill(n + 4 * k, seed, 0)[4 * k:])


@pytest.mark.parametrize("c", [0, 2 ** 32 - 1])
def test_normal_fill_device_counter(cuda, c):
    """The device counter is bumped before each draw, which starts at
    offset + counter * ceil(n / 4); c = 2^32 - 1 carries into the counter's high word."""
    n, seed, offset = 1027, 1234, 3
    t = (n + 3) // 4
    ctr = torch.full((1,), c, dtype=torch.int64, device="cuda")
    a = fill(n, seed, offset, counter=ctr).clone()
    b = fill(n, seed, offset, counter=ctr)
    assert int(ctr) == c + 2
    for got, base in ((a, offset + (c + 1) * t), (b, offset + (c + 2) * t)):
        d = np.abs(host(got) - H.normal_ref(n, seed, base))
        assert d.max() < SAMPLER_GATE, d.max()
        assert torch.equal(got, fill(n, seed, base))


def test_normal_fill_distribution(cuda):
    """Moments and serial correlation of one draw of 2^20 + 3, each at 5 standard errors (the
    float64 restatement gives at most 1.8 over three seeds)."""
    n = 2 ** 20 + 3
    x = host(fill(n, 1234))
    mean, std = x.mean(), x.std()
    z = (x - mean) / std
    stats = {"mean": abs(mean) * np.sqrt(n), "std": abs(std - 1) * np.sqrt(2 * n),
             "skew": abs((z ** 3).mean()) * np.sqrt(n / 6),
             "kurtosis": abs((z ** 4).mean() - 3) * np.sqrt(n / 24)}
    for lag in (1, 2, 3, 4):
        stats[f"lag{lag}"] = abs((z[lag:] * z[:-lag]).mean()) * np.sqrt(n)
    print("normal_fill standard errors: " + " ".join(f"{k} {v:.2f}" for k, v in stats.items()))
    for k, v in stats.items():
        assert v < 5, (k, v)


# ----------------------------------------------------------------------------- Adam
# Largest O.rel_err of the float32 numpy restatement of adam.hip's expression order from the
# float64 restatement of torch.optim.Adam, over p, m, v, vmax of H.ADAM_CASES (late-steps, on v).
ADAM_F32_DEV = 3.7e-7
ADAM_GATE = 4 * ADAM_F32_DEV


def adam_call(t, n, wd, amsgrad, vmax=True):
    N.call("ebsdvae_adam", N.ptr(t["p"]), N.ptr(t["g"]), N.ptr(t["m"]), N.ptr(t["v"]),
           N.ptr(t["vmax"]) if vmax else None, N.ptr(t["step"]), n, H.ADAM_HYPER["lr"],
           H.ADAM_HYPER["b1"], H.ADAM_HYPER["b2"], H.ADAM_HYPER["eps"], wd, int(amsgrad), N.stream())


@pytest.mark.parametrize("name", H.ADAM_CASES)
def test_adam_matches_float64_restatement(cuda, name):
    """ebsdvae_adam, called directly on state the test owns, against the float64 restatement of
    single-tensor torch.optim.Adam: n past one grid pass of 4096 x 256 threads, n = 1, 20 steps
    from step 1000 with nonzero m, v, vmax (the counter reads 1020 afterwards), gradients of
    1e-12 and 1e+6 in one tensor (each magnitude compared on its own scale).
    Gate: the float32 numpy restatement of the kernel's expression order lies within 3.7e-7 of
    the float64 one over these cases; the GPU is held to 4 x that, 1.48e-6."""
    c = H.adam_case(name)
    n = c["n"]
    t = {k: dev(c[k]) for k in ("p", "m", "v", "vmax")}
    t["step"] = torch.full((1,), c["step"], device="cuda")
    for g in c["g_steps"]:
        t["g"] = dev(g)
        adam_call(t, n, c["wd"], c["amsgrad"], vmax=c["amsgrad"])
    torch.cuda.synchronize()
    assert float(t["step"]) == c["ref"]["step"]
    got = {k: host(t[k]) for k in ("p", "m", "v", "vmax")}
    assert all(np.isfinite(v).all() for v in got.values())
    e = H.adam_deviation(c, got)
    print(f"adam {name}: {e:.2e} (gate {ADAM_GATE:.2e})")
    assert e < ADAM_GATE
    if not c["amsgrad"]:
        assert np.array_equal(got["vmax"], c["vmax"]), "vmax written without amsgrad"


@pytest.mark.parametrize("amsgrad", [False, True])
def test_adam_zero_gradients_leave_the_parameters(cuda, amsgrad):
    """All-zero gradients from a zero state without weight decay: denom = eps, the update is
    0 / eps; p is unchanged bit for bit and m, v stay 0."""
    n = 1000
    p0 = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    t = {"p": p0.clone(), "g": torch.zeros(n, device="cuda"), "m": torch.zeros(n, device="cuda"),
         "v": torch.zeros(n, device="cuda"), "vmax": torch.zeros(n, device="cuda"),
         "step": torch.zeros(1, device="cuda")}
    for _ in range(3):
        adam_call(t, n, 0.0, amsgrad)
    assert torch.equal(t["p"], p0)
    assert float(t["step"]) == 3.0
    for k in ("m", "v", "vmax"):
        assert not t[k].any(), k


def test_adam_amsgrad_without_vmax_is_refused(cuda):
    n = 100
    t = {k: torch.full((n,), v, device="cuda") for k, v in (("p", 1.0), ("g", 0.5), ("m", 0.25), ("v", 0.125))}
    t["vmax"] = None
    t["step"] = torch.full((1,), 7.0, device="cuda")
    before = {k: v.clone() for k, v in t.items() if v is not None}
    with pytest.raises(RuntimeError, match="vmax"):
        adam_call(t, n, 0.0, True, vmax=False)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(t[k], v), k
