"""Float64 references of the middle of the model, shared by tests/test_gpu_heads_shapes.py,
tests/test_gpu_direct_calls.py and tests/test_abi.py: the latent heads (csrc/heads.hip) with a
host-side port of their launch planning, the Philox4x32-10 + Box-Muller sampler, and
single-tensor Adam (csrc/adam.hip).  Plain numpy; nothing here touches the GPU.
"""
import functools

import numpy as np

from oracle import vae_oracle as O


def f32(a):
    """Round to float32 and back: the reference sees the values the kernel sees."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ----------------------------------------------------------------------------- heads planning
# Port of heads_np / heads_tile / heads_cc / heads_partial_launch / heads_expand_launch /
# heads_shape_ok of csrc/heads.hip.
HT = 256
LDS_MAX = 160 * 1024
MAXL = 64


def heads_np(n):
    p = 16
    while p < n:
        p *= 2
    return p


def heads_tile(B, SS, n):
    bt = 2048 // n
    while bt > 256 // n and SS * ((B + bt - 1) // bt) < 256:
        bt //= 2
    return bt


def heads_cc(C, SS):
    cc = 1
    while cc * 2 * SS <= 128 and cc * 2 <= C:
        cc *= 2
    return cc


def partial_launch(B, C, SS, N):
    """(bt, R, lds bytes, KS, KC, NP) of the split-K partial pass over N output rows."""
    NP = heads_np(N)
    CC = heads_cc(C, SS)
    KS, KC = C // CC, CC * SS
    bt = heads_tile(B, KS, NP)
    return bt, bt * NP // HT, (KC * (NP + 1) + bt * (KC + 1)) * 4, KS, KC, NP


def expand_launch(B, C, SS, J):
    """(bt, R, lds bytes) of the expand pass over J latent columns."""
    bt = heads_tile(B, SS, C)
    return bt, bt * C // HT, (J * C + bt * J) * 4


def heads_shape_ok(B, C, S, L):
    if not (B > 0 and 0 < L <= MAXL and 0 < S <= 1024 and 16 <= C <= 256 and C & (C - 1) == 0):
        return False
    SS = S * S
    launches = [partial_launch(B, C, SS, 2 * L)[:3], partial_launch(B, C, SS, L)[:3],
                expand_launch(B, C, SS, L), expand_launch(B, C, SS, 2 * L)]
    return all(lds <= LDS_MAX and R in (1, 2, 4, 8) for _, R, lds in launches)


def heads_work_bytes(B, C, S, L):
    """What ebsdvae_heads_work answers."""
    if not heads_shape_ok(B, C, S, L):
        return 0
    return (C // heads_cc(C, S * S)) * B * heads_np(2 * L) * 4


# (C, S, L, B): the shape family of the heads' C ABI, each chosen from the port above
HEADS_CASES = [
    (16, 2, 1, 1),       # smallest of everything; one block; L = 1
    (16, 1, 3, 70),      # S*S = 1, KS = 1, 5 pattern tiles with a partly filled last one
    (32, 4, 10, 3),      # L not a power of two (N = 20 in NP = 32)
    (64, 3, 20, 37),     # S*S = 9: KC = 72, not a power of two; NP = 64
    (256, 1, 7, 5),      # C = 256: PB = 1, expand bt = 1; CC = 128
    (256, 3, 9, 129),    # partial R = 2, expand R = 4, B one past a tile multiple
    (256, 2, 64, 300),   # partial R = 4; expand LDS 133 KiB (above the 128 KiB mark)
    (16, 16, 64, 9),     # S*S = 256 > 128: CC = 1, KC = 256; partial LDS 134 KiB; expand R = 8
    (64, 12, 24, 4),     # CC = 1 with KC = 144
    (16, 3, 40, 700),    # NP = 128 from L = 40; 175 pattern tiles
    (32, 2, 64, 2000),   # KS = 1 with R = 2; B well past 256
]
PLAN_SHAPES = [(128, 4, 16, 256), (128, 8, 64, 256)]   # the 128 x 128 and 256 x 256 models
LARGEST_ADMITTED = (16, 17, 64, 4)                     # partial LDS 151 KiB
# (B, C, S, L) the size query and the entry points refuse
REFUSED = [(4, 16, 18, 64),    # staged chunk 324 x 129 floats = 167 KiB
           (4, 128, 40, 4),    # KC = 1600: 211 KiB
           (4, 48, 2, 16), (4, 8, 2, 16), (4, 512, 2, 16),   # C no power of two in 16..256
           (4, 128, 4, 0), (4, 128, 4, 65), (0, 128, 4, 16)]


@functools.lru_cache(maxsize=None)
def heads_case(C, S, L, B, seed=0):
    """Inputs (float32-representable float64) and the float64 reference of heads_fwd /
    heads_bwd / heads_wgrad at one shape.  Scales as test_heads_forward_backward, with W_mu and
    W_lv at 1 / sqrt(F) so that logvar is O(1) at every F.  Computed once per case; callers do
    not modify it."""
    rng = np.random.default_rng(1000003 * seed + 7919 * C + 131 * S + 17 * L + B)
    F = C * S * S
    d = {"enc": f32(rng.standard_normal((B, S, S, C))),
         "w_mu": f32(rng.standard_normal((L, F)) / np.sqrt(F)), "b_mu": f32(rng.standard_normal(L) * 0.1),
         "w_lv": f32(rng.standard_normal((L, F)) / np.sqrt(F)), "b_lv": f32(rng.standard_normal(L) * 0.1),
         "w_l2": f32(rng.standard_normal((F, L)) * 0.2), "b_l2": f32(rng.standard_normal(F) * 0.1),
         "eps": f32(rng.standard_normal((B, L))),
         "g_dec": f32(rng.standard_normal((B, S, S, C))),
         "g_z": f32(rng.standard_normal((B, L))), "g_mu": f32(rng.standard_normal((B, L))),
         "g_std": f32(rng.standard_normal((B, L)))}
    flat = O.nchw_flatten(d["enc"])
    mu = flat @ d["w_mu"].T + d["b_mu"]
    std = np.exp((flat @ d["w_lv"].T + d["b_lv"]) / 2)
    z = mu + d["eps"] * std
    ref = {"flat": flat, "mu": mu, "std": std, "z": z,
           "dec_in": O.nchw_unflatten(z @ d["w_l2"].T + d["b_l2"], C, S)}
    d["ref"] = ref
    return d


def heads_bwd_ref(d, C, S, null=()):
    """Float64 backward of a heads_case; the upstream gradients named in `null` are zero."""
    ref = d["ref"]
    g_z, g_mu, g_std = (np.zeros_like(d[k]) if k in null else d[k] for k in ("g_z", "g_mu", "g_std"))
    g_out = O.nchw_flatten(d["g_dec"])
    gzt = g_out @ d["w_l2"] + g_z
    gmt = gzt + g_mu
    glv = (g_std + gzt * d["eps"]) * ref["std"] / 2
    return {"g_enc": O.nchw_unflatten(gmt @ d["w_mu"] + glv @ d["w_lv"], C, S),
            "gs": np.concatenate([gmt, glv, g_out], axis=1),
            "gw_mu": gmt.T @ ref["flat"], "gb_mu": gmt.sum(0),
            "gw_lv": glv.T @ ref["flat"], "gb_lv": glv.sum(0),
            "gw_l2": g_out.T @ ref["z"], "gb_l2": g_out.sum(0)}


# ----------------------------------------------------------------------------- sampler
M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def philox4x32_10(ctr, key):
    """Philox4x32-10.  ctr: four uint64 arrays (or scalars) holding 32-bit words, key: two.
    Returns the four output words as uint64 arrays."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, np.uint64)) & M32 for c in ctr)
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2          # 32 x 32 -> 64 bits: no overflow
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def normal_ref(n, seed, offset=0, dtype=np.float64):
    """ebsdvae_normal_fill(out, n, seed, offset, NULL) restated: counter {offset + i, 0, 0} (64
    bits over the first two words), key the two halves of seed, u = (c + 0.5) 2^-32, Box-Muller
    {r0 cos, r0 sin, r1 cos, r1 sin} with r0 from (c0, u1) and r1 from (c2, u3).  dtype float64
    is the reference; float32 restates the kernel's own arithmetic (numpy's logf / cosf / sinf
    in place of the device's) and measures what float32 costs."""
    t = (n + 3) // 4
    with np.errstate(over="ignore"):
        ctr = np.uint64(offset & (2 ** 64 - 1)) + np.arange(t, dtype=np.uint64)   # wraps mod 2^64
    c = philox4x32_10((ctr & M32, ctr >> np.uint64(32), 0, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    ft = dtype
    u0, u1, u2, u3 = ((w.astype(ft) + ft(0.5)) * ft(2.0 ** -32) for w in c)
    r0, r1 = np.sqrt(ft(-2.0) * np.log(u0)), np.sqrt(ft(-2.0) * np.log(u2))
    tp = ft(6.283185307179586)
    out = np.stack([r0 * np.cos(tp * u1), r0 * np.sin(tp * u1), r1 * np.cos(tp * u3), r1 * np.sin(tp * u3)], 1)
    assert out.dtype == ft
    return out.reshape(-1)[:n]


# ----------------------------------------------------------------------------- Adam
def adam_ref(p, g_steps, m, v, vmax, step, lr, b1, b2, eps, wd, amsgrad, dtype=np.float64):
    """Single-tensor torch.optim.Adam over the gradients g_steps, restated.  dtype float64 is
    the reference (hyper-parameters as the float32 values the kernel receives); float32 follows
    the kernel's expression order (adam.hip; its two fmaf through an exact product) and measures
    what float32 costs.  Returns (p, m, v, vmax, step)."""
    ft = dtype
    p, m, v = (np.array(a, ft) for a in (p, m, v))
    vmax = np.array(vmax, ft) if amsgrad else None
    lr, b1, b2, eps, wd = (ft(np.float32(a)) for a in (lr, b1, b2, eps, wd))
    t = ft(step)
    one = ft(1)

    def fma(a, b, c):   # a * b exact in float64 for float32 operands
        if ft is np.float64:
            return a * b + c
        a, b, c = (np.asarray(t, np.float64) for t in (a, b, c))
        return (a * b + c).astype(ft)

    for g in g_steps:
        t = t + one
        bc1, bc2 = one - np.power(b1, t), one - np.power(b2, t)
        step_size, bc2s = lr / bc1, np.sqrt(bc2)
        g = np.array(g, ft)
        if wd != 0:
            g = fma(wd, p, g)
        m = m + (one - b1) * (g - m)
        v = fma(b2, v, (one - b2) * g * g)
        vv = v
        if amsgrad:
            vmax = np.maximum(vmax, v)
            vv = vmax
        denom = np.sqrt(vv) / bc2s + eps
        p = p - step_size * (m / denom)
        assert p.dtype == ft and v.dtype == ft and m.dtype == ft
    return p, m, v, vmax, float(t)


ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
ADAM_CASES = ["grid-pass", "grid-pass-amsgrad", "one", "late-steps", "late-steps-amsgrad",
              "wide-range", "wide-range-amsgrad"]


@functools.lru_cache(maxsize=None)
def adam_case(name):
    """Inputs of one ebsdvae_adam case (float32-representable) and its float64 result.
    grid-pass: n one grid pass of 4096 x 256 threads plus 777, 3 steps from a zero state;
    one: n = 1; late-steps: 20 steps from step 1000 with nonzero m, v, vmax (powf(beta, t) far
    from t = 1); wide-range: gradients of magnitude 1e-12 and 1e+6 interleaved in one tensor, no
    weight decay -- `groups` then splits the elements by magnitude, and each group is compared
    on its own scale (v spans 1e-27 ... 1e+9)."""
    amsgrad = name.endswith("-amsgrad")
    kind = name[:-len("-amsgrad")] if amsgrad else name
    rng = np.random.default_rng(ADAM_CASES.index(name) + 11)
    n, steps, step, wd = {"grid-pass": (4096 * 256 + 777, 3, 0, 0.01), "one": (1, 3, 0, 0.01),
                          "late-steps": (10007, 20, 1000, 0.01), "wide-range": (4098, 3, 0, 0.0)}[kind]
    c = {"n": n, "step": float(step), "wd": wd, "amsgrad": amsgrad, "groups": [slice(None)]}
    c["p"] = f32(rng.standard_normal(n))
    gs = rng.standard_normal((steps, n))
    if kind == "wide-range":
        gs[:, 0::2] *= 1e-12
        gs[:, 1::2] *= 1e6
        c["groups"] = [slice(0, None, 2), slice(1, None, 2)]
    c["g_steps"] = f32(gs)
    if kind == "late-steps":
        c["m"] = f32(rng.standard_normal(n) * 0.3)
        c["v"] = f32(rng.random(n) + 0.01)
        c["vmax"] = f32(c["v"] * (1 + rng.random(n)))
    else:
        c["m"], c["v"], c["vmax"] = np.zeros(n), np.zeros(n), np.zeros(n)
    c["ref"] = adam_run(c, np.float64)
    return c


def adam_run(c, dtype):
    """{p, m, v[, vmax], step} of a case's steps in dtype (adam_ref)."""
    p, m, v, vmax, t = adam_ref(c["p"], c["g_steps"], c["m"], c["v"], c["vmax"], c["step"],
                                wd=c["wd"], amsgrad=c["amsgrad"], dtype=dtype, **ADAM_HYPER)
    out = {"p": p, "m": m, "v": v, "step": t}
    if c["amsgrad"]:
        out["vmax"] = vmax
    return out


def adam_deviation(c, got):
    """Largest O.rel_err of got's p, m, v, vmax from the case's float64 result, per group."""
    worst = 0.0
    for k, r in c["ref"].items():
        if k != "step":
            for g in c["groups"]:
                worst = max(worst, O.rel_err(np.asarray(got[k], np.float64)[g], r[g]))
    return worst
