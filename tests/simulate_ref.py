"""Float64 restatement of the dictionary simulation (include/ebsdvae.h, steps (a) to (e) of
ebsdvae_simulate_patterns; DESIGN.md section 14, "Dictionary simulation"), the inverse Lambert
map, the derived gate and the seeded masters the simulation tests share.  Plain numpy: a
restatement of the definition, not of the kernel."""
import functools
import math

import numpy as np

EPS = 2.0 ** -24            # float32 unit roundoff: |fl(a) - a| <= EPS |a|
ATAN_ULP = 5                # atanf's error bound in ulp (see gate)
V_COMPONENT_ERR = 5 * EPS   # |v_device - v_reference| per component (see gate)


# ------------------------------------------------------------------------------ (a)
def orientation_matrix(euler):
    """The Bunge passive matrix of (..., 3) angles in degrees, float64."""
    e = np.asarray(euler, dtype=np.float64) * (math.pi / 180.0)
    c1, s1 = np.cos(e[..., 0]), np.sin(e[..., 0])
    c, s = np.cos(e[..., 1]), np.sin(e[..., 1])
    c2, s2 = np.cos(e[..., 2]), np.sin(e[..., 2])
    return np.stack([
        np.stack([c1 * c2 - s1 * s2 * c, s1 * c2 + c1 * s2 * c, s2 * s], -1),
        np.stack([-c1 * s2 - s1 * c2 * c, -s1 * s2 + c1 * c2 * c, c2 * s], -1),
        np.stack([s1 * s, -c1 * s, c], -1)], -2)


# ------------------------------------------------------------------------------ (c)
def lambert_forward(v):
    """Step (c) in float64: (..., 3) vectors -> (tx, ty, lower)."""
    v = np.asarray(v, dtype=np.float64)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    s = np.sqrt((x * x + y * y) / (1.0 + np.abs(z)))
    zero = (x == 0) & (y == 0)
    first = np.abs(y) <= np.abs(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(first, np.arctan(y / x), np.arctan(x / y))
    a = np.where(zero, 0.0, a)
    lead = np.where(first, np.copysign(s, x), np.copysign(s, y))
    other = lead * (4.0 / math.pi) * a
    tx = np.where(zero, 0.0, np.where(first, lead, other))
    ty = np.where(zero, 0.0, np.where(first, other, lead))
    return tx, ty, z < 0


def lambert_inverse(X, Y, lower=False):
    """The unit vector of the Lambert coordinates (X, Y) in [-1, 1]^2 on the upper hemisphere
    (z >= 0), or its mirror image in z.  With |Y| <= |X|: 1 - |z| = X^2, the azimuth
    (pi / 4) Y / X measured from the axis X points along; otherwise with X and Y exchanged."""
    X, Y = np.broadcast_arrays(np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64))
    first = np.abs(Y) <= np.abs(X)
    lead = np.where(first, X, Y)
    other = np.where(first, Y, X)
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = np.where(lead != 0, (math.pi / 4.0) * other / lead, 0.0)
    z = 1.0 - lead * lead
    rho = np.abs(lead) * np.sqrt(2.0 - lead * lead)
    p = np.copysign(rho, lead) * np.cos(phi)
    q = np.copysign(rho, lead) * np.sin(phi)
    x = np.where(first, p, q)
    y = np.where(first, q, p)
    return np.stack([x, y, -z if lower else z], -1)


# ------------------------------------------------------------------------------ (d), (e)
def _texel(t, n):
    u = np.clip(n + n * t, 0.0, 2.0 * n)
    i0 = np.minimum(u.astype(np.int64), 2 * n - 1)
    return i0, u - i0


def interpolate(master, r0, fr, j0, fu):
    top = master[r0, j0] + fu * (master[r0, j0 + 1] - master[r0, j0])
    bot = master[r0 + 1, j0] + fu * (master[r0 + 1, j0 + 1] - master[r0 + 1, j0])
    return top + fr * (bot - top)


def rescale(v):
    """Step (e) per pattern on (B, ...) float64."""
    flat = v.reshape(v.shape[0], -1)
    lo, hi = flat.min(1)[:, None], flat.max(1)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(hi == lo, 0.0, (flat - lo) / (hi - lo))
    return out.reshape(v.shape)


def rotate(dirs32, euler):
    """Steps (a), (b): g rounded to float32, v = g d in float64; (B, n, 3)."""
    g = orientation_matrix(euler).astype(np.float32).astype(np.float64)
    d = np.asarray(dirs32, dtype=np.float32).astype(np.float64)     # (3, n)
    return np.einsum("bij,jn->bni", g, d)


def simulate(upper, lower, dirs32, euler, shape, do_rescale):
    """(a) to (e) in float64 from the float32 master and the float32 planar directions (3, n):
    (B, 1, h, w) float64.  Also returns the coordinates (r, u) of every sample in texels and
    the hemisphere mask, (B, n) each."""
    up = np.asarray(upper, dtype=np.float32).astype(np.float64)
    lo = np.asarray(lower, dtype=np.float32).astype(np.float64)
    n = (up.shape[0] - 1) // 2
    euler = np.asarray(euler, dtype=np.float64).reshape(-1, 3)
    v = rotate(dirs32, euler)
    tx, ty, low = lambert_forward(v)
    j0, fu = _texel(tx, n)
    r0, fr = _texel(ty, n)
    val = np.where(low, interpolate(lo, r0, fr, j0, fu), interpolate(up, r0, fr, j0, fu))
    if do_rescale:
        val = rescale(val)
    return val.reshape(euler.shape[0], 1, *shape), (r0 + fr, j0 + fu, low)


# ------------------------------------------------------------------------------ the gate
def texel_step(upper, lower):
    """G: the largest difference between adjacent texels (along a row or a column) of either
    hemisphere, and across the equator between the two hemispheres' border texels, which are
    the same points of the sphere."""
    up = np.asarray(upper, dtype=np.float64)
    lo = np.asarray(lower, dtype=np.float64)
    g = 0.0
    for m in (up, lo):
        g = max(g, np.abs(np.diff(m, axis=0)).max(), np.abs(np.diff(m, axis=1)).max())
    return float(max(g, equator_step(up, lo)))


def equator_step(upper, lower):
    up = np.asarray(upper, dtype=np.float64)
    lo = np.asarray(lower, dtype=np.float64)
    border = np.ones(up.shape, bool)
    border[1:-1, 1:-1] = False
    return float(np.abs(up[border] - lo[border]).max())


def gate(upper, lower, value_range=None, equator=None):
    """max |out - reference| allowed, derived (EPS = 2^-24, n = (M - 1) / 2, G = texel_step,
    mmax = max |m|):

    Coordinate error, in Lambert units.
    * v: the reference rotates the same float32 directions by the float32-rounded g of its own
      float64 sines and cosines.  The device's float64 ones may round an entry of g to the
      neighbouring float32: at most 2^-24 per entry (|g| <= 1), sqrt(3) EPS on a component of v
      for a unit d.  The chain g_i0 d_x, fma, fma rounds 3 times, each against a partial sum of at
      most |g_i| |d| = 1: 3 EPS.  Per component (3 + sqrt 3) EPS < 5 EPS (V_COMPONENT_ERR), in
      norm < 9 EPS.
    * The map (c) is one continuous function of v (its branches agree where they meet) with
      Lipschitz constant K < 2 against the Euclidean norm near the unit sphere: the equal-area
      projection onto the disc of radius 1 stretches by at most 1 (at the equator), the disc to
      square map has the Jacobian [[1, 0], [4 phi / pi, 4 / pi]], |phi| <= pi / 4, of spectral norm
      < 1.77, and a radial change of v by delta moves (tx, ty) by at most sqrt(2) delta
      (tests/test_simulate_host.py measures K on random pairs).  So 2 * 9 EPS = 18 EPS.
    * Evaluating (c) in float32: s takes y y, the fma, 1 + |z|, the division (4 roundings, halved
      by the root) and the root: 3 EPS, which is tx's.  The quotient y / x rounds once (EPS, and
      atan' <= 1); atanf is within ATAN_ULP = 5 ulp (the OpenCL full-profile bound the device
      library is built to; HIP documents 2), an ulp at most 2 EPS |atan| <= 2 EPS pi / 4, which
      times k is 2 * 5 EPS; k, k atan and the last product round once each.  With |tx|, |k atan|
      <= 1: ty's error <= 3 + (4 / pi + 10 + 2) + 1 < 18 EPS.
    Per axis 18 + 18 = 36 EPS, times n in texels; u = fma(n, t, n) rounds once against 2n:
    38 n EPS texels per axis (the clamp and u - j0 are exact).

    Value error.  The bilinear interpolant is continuous and piecewise linear along each axis
    with slopes of at most G per texel: 2 axes * 38 n EPS G.  Its own arithmetic: b - a (2 EPS
    mmax), the fma (EPS mmax) for top and bot, which enter with weights 1 - fr and fr; bot - top
    (2 EPS mmax); the last fma (EPS mmax): 6 EPS mmax.  A sample whose v_z changes sign between
    device and reference reads the other hemisphere at the same border position: `equator`,
    the step between the hemispheres' border texels, is added whole (it is 0 for the smooth
    master; a test that passes equator=0 for another master shows that v_z is exact).

        e_raw = (76 n G + 6 mmax) EPS + equator

    With `value_range` R = max - min of the reference pattern, the gate of the rescaled output:
    numerator and denominator move by at most 2 e_raw each and the quotient is at most 1, so
    4 e_raw / (R - 2 e_raw); v - lo, hi - lo and the division round once each: + 3 EPS."""
    up = np.asarray(upper, dtype=np.float64)
    lo = np.asarray(lower, dtype=np.float64)
    n = (up.shape[0] - 1) // 2
    G = texel_step(up, lo)
    mmax = max(np.abs(up).max(), np.abs(lo).max())
    eq = equator_step(up, lo) if equator is None else float(equator)
    e_raw = (76.0 * n * G + 6.0 * mmax) * EPS + eq
    if value_range is None:
        return e_raw
    R = float(value_range)
    assert R > 4 * e_raw, "the pattern's range is inside the raw gate: nothing can be checked"
    return 4.0 * e_raw / (R - 2.0 * e_raw) + 3.0 * EPS


def cap(upper, lower, value_range=None):
    """What a gate must stay below: G / 50 (over the range R after a rescale), so that a sample
    one texel off, or from the wrong hemisphere, cannot pass where the master moves by G."""
    G = texel_step(upper, lower)
    return G / 50.0 if value_range is None else G / 50.0 / float(value_range)


# ------------------------------------------------------------------------------ masters
def lambert_grid(M):
    n = (M - 1) // 2
    t = (np.arange(M, dtype=np.float64) - n) / n
    Y, X = np.meshgrid(t, t, indexing="ij")       # rows follow Y, columns follow X
    return X, Y


BAND_NORMALS = np.array([[0.2, 0.5, 0.84], [0.9, -0.3, 0.31], [-0.55, 0.1, 0.83], [0.3, 0.8, -0.52],
                         [0.05, -0.7, 0.71]])
BAND_WIDTHS = np.array([0.12, 0.2, 0.16, 0.25, 0.14])
POLAR_AXIS = np.array([0.3, -0.5, 0.81])


def sphere_function(v):
    """A non-centrosymmetric function on the sphere: Gaussian bands exp(-((v . n_k) / w_k)^2)
    plus 0.3 v . a."""
    nk = BAND_NORMALS / np.linalg.norm(BAND_NORMALS, axis=1, keepdims=True)
    a = POLAR_AXIS / np.linalg.norm(POLAR_AXIS)
    f = 0.3 * (v @ a)
    for k in range(len(nk)):
        f = f + np.exp(-(((v @ nk[k]) / BAND_WIDTHS[k]) ** 2))
    return f


@functools.lru_cache(maxsize=None)
def smooth_master(M):
    """(upper, lower) float32, read-only: sphere_function sampled through the inverse Lambert
    map, so that the two hemispheres hold the same values on the equator."""
    X, Y = lambert_grid(M)
    out = []
    for lower in (False, True):
        m = sphere_function(lambert_inverse(X, Y, lower)).astype(np.float32)
        m.setflags(write=False)
        out.append(m)
    return tuple(out)


RAMP_A, RAMP_B = 1.0, 0.375          # per row, per column: a != b, both exact in float32
RAMP_C0 = (2.0, 40.0)                # upper, lower


@functools.lru_cache(maxsize=None)
def ramp_master(M):
    """m[r][c] = a r + b c + c0, another c0 per hemisphere: bilinear interpolation reproduces
    it, so an output reads back its sample's (r, u) and hemisphere."""
    r, c = np.meshgrid(np.arange(M, dtype=np.float64), np.arange(M, dtype=np.float64), indexing="ij")
    out = []
    for c0 in RAMP_C0:
        m = (RAMP_A * r + RAMP_B * c + c0).astype(np.float32)
        m.setflags(write=False)
        out.append(m)
    return tuple(out)


# ------------------------------------------------------------------------------ inputs
def spread_orientations(N, seed=0, min_deg=10.0):
    """N seeded Bunge triples whose rotations are pairwise at least `min_deg` apart."""
    rng = np.random.default_rng(seed)
    out, mats = [], []
    while len(out) < N:
        e = np.array([rng.uniform(0, 360), np.degrees(np.arccos(rng.uniform(-1, 1))),
                      rng.uniform(0, 360)])
        g = orientation_matrix(e)
        ok = True
        for h in mats:
            c = (np.trace(g @ h.T) - 1.0) / 2.0
            if np.degrees(np.arccos(np.clip(c, -1, 1))) < min_deg:
                ok = False
                break
        if ok:
            out.append(e)
            mats.append(g)
    return np.array(out)
