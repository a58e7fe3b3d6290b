"""The latent heads through the C ABI over the shape family heads_shape_ok admits
(csrc/heads.hip): ebsdvae_heads_fwd / _latent_mu / _heads_bwd / _heads_wgrad called directly
(a Plan expresses C = 128 only) against the float64 reference of tests/heads_ref.py, at the
gates of test_heads_forward_backward: O.rel_err < 1e-7 for flat, < 1e-5 for mu, std, z and
dec_in, < 1e-4 for g_enc and the six parameter gradients.

Every buffer a kernel writes is allocated at exactly its documented size, NaN-filled, with 1024
canary floats behind it in the same tensor: a canary that changed is a write past the end, a NaN
left in an output an element nobody wrote (or a read of an unwritten partial sum).
"""
import numpy as np
import pytest
import torch

import heads_ref as H
from latice import _native as N
from oracle import vae_oracle as O

pytestmark = pytest.mark.gpu

CANARY = 1024
CANARY_VALUE = -12345.5
FWD_GATES = {"flat": 1e-7, "mu": 1e-5, "std": 1e-5, "z": 1e-5, "dec_in": 1e-5}
BWD_GATE = 1e-4
WGRAD_NAMES = ("gw_mu", "gb_mu", "gw_lv", "gb_lv", "gw_l2", "gb_l2")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


class Guarded:
    """n NaN floats followed by CANARY canaries in one tensor; .t is the n-float view."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.full = torch.full((n + CANARY,), CANARY_VALUE, device="cuda")
        self.t = self.full[:n].view(*shape)
        self.t.fill_(float("nan"))

    def intact(self):
        return bool((self.full[self.t.numel():] == CANARY_VALUE).all())


def guarded_bytes(nbytes):
    assert nbytes > 0 and nbytes % 4 == 0
    return Guarded(nbytes // 4)


def check_guards(bufs, outputs):
    torch.cuda.synchronize()
    for k, g in bufs.items():
        assert g.intact(), f"{k}: written past its end"
    for k in outputs:
        assert not torch.isnan(bufs[k].t).any(), f"{k}: elements left unwritten"


def inputs(d):
    return {k: dev(v) for k, v in d.items() if k != "ref"}


def run_fwd(t, C, S, L, B):
    """heads_fwd and latent_mu with guarded buffers -> {flat, mu, std, z, dec_in, mu_only}."""
    F = C * S * S
    bufs = {"flat": Guarded(B, F), "mu": Guarded(B, L), "std": Guarded(B, L), "z": Guarded(B, L),
            "dec_in": Guarded(B, S, S, C),
            "work": guarded_bytes(N.call("ebsdvae_heads_work", B, C, S, L))}
    N.call("ebsdvae_heads_fwd", N.ptr(t["enc"]), N.ptr(t["w_mu"]), N.ptr(t["b_mu"]), N.ptr(t["w_lv"]),
           N.ptr(t["b_lv"]), N.ptr(t["w_l2"]), N.ptr(t["b_l2"]), N.ptr(t["eps"]), N.ptr(bufs["flat"].t),
           N.ptr(bufs["mu"].t), N.ptr(bufs["std"].t), N.ptr(bufs["z"].t), N.ptr(bufs["dec_in"].t),
           N.ptr(bufs["work"].t), B, C, S, L, N.stream())
    check_guards(bufs, ("flat", "mu", "std", "z", "dec_in"))
    bufs2 = {"mu_only": Guarded(B, L), "work": guarded_bytes(N.call("ebsdvae_heads_work", B, C, S, L))}
    N.call("ebsdvae_latent_mu", N.ptr(t["enc"]), N.ptr(t["w_mu"]), N.ptr(t["b_mu"]),
           N.ptr(bufs2["mu_only"].t), N.ptr(bufs2["work"].t), B, C, S, L, N.stream())
    check_guards(bufs2, ("mu_only",))
    out = {k: bufs[k].t for k in FWD_GATES}
    out["mu_only"] = bufs2["mu_only"].t
    return out


def run_bwd(t, fwd, C, S, L, B, g_z="g_z", g_mu="g_mu", g_std="g_std", wgrad=True):
    """heads_bwd (+ heads_wgrad) with guarded buffers; g_z / g_mu / g_std: the name of the
    input to pass, None for NULL, or a tensor."""
    F = C * S * S
    up = [t[g] if isinstance(g, str) else g for g in (g_z, g_mu, g_std)]
    bufs = {"g_enc": Guarded(B, S, S, C), "gs": Guarded(B, 2 * L + F),
            "work": guarded_bytes(N.call("ebsdvae_heads_work", B, C, S, L))}
    N.call("ebsdvae_heads_bwd", N.ptr(t["g_dec"]), N.ptr(up[0]), N.ptr(up[1]), N.ptr(up[2]),
           N.ptr(fwd["std"]), N.ptr(t["eps"]), N.ptr(t["w_mu"]), N.ptr(t["w_lv"]), N.ptr(t["w_l2"]),
           N.ptr(bufs["g_enc"].t), N.ptr(bufs["gs"].t), N.ptr(bufs["work"].t), B, C, S, L, N.stream())
    check_guards(bufs, ("g_enc", "gs"))
    out = {"g_enc": bufs["g_enc"].t, "gs": bufs["gs"].t}
    if wgrad:
        wb = {"gw_mu": Guarded(L, F), "gb_mu": Guarded(L), "gw_lv": Guarded(L, F), "gb_lv": Guarded(L),
              "gw_l2": Guarded(F, L), "gb_l2": Guarded(F),
              "wwork": guarded_bytes(N.call("ebsdvae_heads_wgrad_work", B, F, L))}
        N.call("ebsdvae_heads_wgrad", N.ptr(fwd["flat"]), N.ptr(fwd["z"]), N.ptr(out["gs"]),
               *[N.ptr(wb[k].t) for k in WGRAD_NAMES], N.ptr(wb["wwork"].t), B, F, L, N.stream())
        check_guards(wb, WGRAD_NAMES)
        out.update({k: wb[k].t for k in WGRAD_NAMES})
    return out


def check_against_reference(case, fwd, bwd, d):
    C, S, L, B = case
    errs = {k: O.rel_err(host(fwd[k]), d["ref"][k]) for k in FWD_GATES}
    errs["mu_only"] = O.rel_err(host(fwd["mu_only"]), d["ref"]["mu"])
    rb = H.heads_bwd_ref(d, C, S)
    berrs = {k: O.rel_err(host(bwd[k]), rb[k]) for k in ("g_enc", "gs") + WGRAD_NAMES}
    print(f"\nheads (C,S,L,B)={case}: " + " ".join(f"{k} {v:.1e}" for k, v in {**errs, **berrs}.items()))
    for k, gate in FWD_GATES.items():
        assert errs[k] < gate, (k, errs[k])
    assert errs["mu_only"] < 1e-5
    for k, v in berrs.items():
        assert v < BWD_GATE, (k, v)


@pytest.mark.parametrize("case", H.HEADS_CASES + [H.LARGEST_ADMITTED], ids=lambda c: "C%d-S%d-L%d-B%d" % c)
def test_heads_shape_family(cuda, case):
    """Forward, backward and weight gradients against float64 at each shape; every output
    bitwise equal over two runs (the sums have a fixed order); ebsdvae_latent_mu bitwise equal to
    the mu of ebsdvae_heads_fwd (encode_mu's docstring: mu == forward(x)[2]; both run the same
    chunking, the same fmaf chain over a chunk and the same chunk-ordered finalize)."""
    C, S, L, B = case
    d = H.heads_case(C, S, L, B)
    t = inputs(d)
    fwd = run_fwd(t, C, S, L, B)
    bwd = run_bwd(t, fwd, C, S, L, B)
    check_against_reference(case, fwd, bwd, d)
    assert torch.equal(fwd["mu_only"], fwd["mu"]), \
        f"latent_mu differs from heads_fwd's mu by {float((fwd['mu_only'] - fwd['mu']).abs().max()):.3e}"
    fwd2 = run_fwd(t, C, S, L, B)
    bwd2 = run_bwd(t, fwd2, C, S, L, B)
    for k in fwd:
        assert torch.equal(fwd[k], fwd2[k]), k
    for k in bwd:
        assert torch.equal(bwd[k], bwd2[k]), k


NULL_VARIANTS = [("g_z",), ("g_mu",), ("g_std",), ("g_z", "g_mu", "g_std")]


@pytest.mark.parametrize("null", NULL_VARIANTS, ids=lambda n: "+".join(n))
@pytest.mark.parametrize("case", [(32, 4, 10, 3), (256, 3, 9, 129)], ids=lambda c: "C%d-S%d-L%d-B%d" % c)
def test_heads_bwd_null_upstream_gradients(cuda, case, null):
    """A NULL g_z / g_mu / g_std is a zero gradient: the float64 reference with zeros in its
    place, and bit for bit what explicit zero tensors give."""
    C, S, L, B = case
    d = H.heads_case(C, S, L, B)
    t = inputs(d)
    fwd = run_fwd(t, C, S, L, B)
    names = ("g_z", "g_mu", "g_std")
    with_null = run_bwd(t, fwd, C, S, L, B, *[None if k in null else k for k in names])
    zeros = torch.zeros(B, L, device="cuda")
    with_zero = run_bwd(t, fwd, C, S, L, B, *[zeros if k in null else k for k in names])
    rb = H.heads_bwd_ref(d, C, S, null=null)
    for k in ("g_enc", "gs") + WGRAD_NAMES:
        e = O.rel_err(host(with_null[k]), rb[k])
        print(f"heads_bwd {case} NULL {null}: {k} {e:.1e}")
        assert e < BWD_GATE, (k, e)
        assert torch.equal(with_null[k], with_zero[k]), k


@pytest.mark.parametrize("shape", H.REFUSED[:2], ids=lambda s: "B%d-C%d-S%d-L%d" % s)
def test_heads_entry_points_refuse_what_the_query_refuses(cuda, shape):
    """Shapes whose staged chunk does not fit the LDS: ebsdvae_heads_work answers 0 and the three
    entry points return nonzero, name the shape and launch nothing (every NaN-filled output is
    still all NaN).  A host-side refusal; the buffers are real and sized for the shape."""
    B, C, S, L = shape
    assert N.call("ebsdvae_heads_work", B, C, S, L) == 0
    F = C * S * S
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)   # noqa: E731
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")    # noqa: E731
    enc, eps, g_dec, std = rnd(B, S, S, C), rnd(B, L), rnd(B, S, S, C), rnd(B, L).exp()
    w_mu, b_mu, w_lv, b_lv, w_l2, b_l2 = rnd(L, F), rnd(L), rnd(L, F), rnd(L), rnd(F, L), rnd(F)
    work = nan(C * B * 128)     # at most C chunks x B patterns x 128 padded rows
    named = f"B={B} C={C} S={S} L={L}"
    flat, mu, sd, z, dec_in = nan(B, F), nan(B, L), nan(B, L), nan(B, L), nan(B, S, S, C)
    with pytest.raises(RuntimeError, match=named):
        N.call("ebsdvae_heads_fwd", N.ptr(enc), N.ptr(w_mu), N.ptr(b_mu), N.ptr(w_lv), N.ptr(b_lv),
               N.ptr(w_l2), N.ptr(b_l2), N.ptr(eps), N.ptr(flat), N.ptr(mu), N.ptr(sd), N.ptr(z),
               N.ptr(dec_in), N.ptr(work), B, C, S, L, N.stream())
    mu2 = nan(B, L)
    with pytest.raises(RuntimeError, match=named):
        N.call("ebsdvae_latent_mu", N.ptr(enc), N.ptr(w_mu), N.ptr(b_mu), N.ptr(mu2), N.ptr(work),
               B, C, S, L, N.stream())
    g_enc, gs = nan(B, S, S, C), nan(B, 2 * L + F)
    with pytest.raises(RuntimeError, match=named):
        N.call("ebsdvae_heads_bwd", N.ptr(g_dec), N.ptr(eps), N.ptr(eps), N.ptr(eps), N.ptr(std),
               N.ptr(eps), N.ptr(w_mu), N.ptr(w_lv), N.ptr(w_l2), N.ptr(g_enc), N.ptr(gs),
               N.ptr(work), B, C, S, L, N.stream())
    torch.cuda.synchronize()
    for name, o in (("flat", flat), ("mu", mu), ("std", sd), ("z", z), ("dec_in", dec_in),
                    ("latent_mu", mu2), ("g_enc", g_enc), ("gs", gs), ("work", work)):
        assert torch.isnan(o).all(), f"{name}: written although the call was refused"

