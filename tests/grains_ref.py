"""The grain segmentation of latice/index/grains.py (csrc/grains.hip) in float64 numpy / scipy,
written from its definitions in include/ebsdvae.h ("grains"): the reference for the host and the
GPU tests, with the generators of their cases."""
import functools
from types import SimpleNamespace

import numpy as np
from scipy.spatial.transform import Rotation as R

from maps_ref import SYM, neighbours, offsets

THRESHOLD = 5.0          # degrees, every generated case
NOISE = 0.5              # degrees of noise per point
BASE_GAP = 10.0          # the bases of a case differ by more than this, in cubic disorientation
EDGE_CAP = 1e-6          # no forward-edge angle lies this close to the threshold ...
PROJECTION_CAP = 1e-3    # ... and the best equivalent of a member beats the second by this


def forward_offsets(connectivity):
    """right, below (4); right, below-left, below, below-right (8): the later half of `offsets`."""
    return [(a, b) for a, b in offsets(connectivity) if (a, b) > (0, 0)]


def usable_points(euler, valid=None):
    ok = np.isfinite(euler).all(axis=1)
    return ok if valid is None else ok & (np.asarray(valid).reshape(-1) != 0)


def edge_angles(euler, scan_shape, connectivity, ok):
    """(p, q, degrees) of every forward edge between usable points, p the lower flat index:
    min over the 24 S of |conj(q_p) (S q_q)|."""
    rows, cols = scan_shape
    ii, jj = np.divmod(np.arange(rows * cols), cols)
    ps, qs = [], []
    for a, b in forward_offsets(connectivity):
        keep = (ii + a < rows) & (jj + b >= 0) & (jj + b < cols)
        p = np.flatnonzero(keep)
        q = p + a * cols + b
        both = ok[p] & ok[q]
        ps.append(p[both]), qs.append(q[both])
    p, q = np.concatenate(ps), np.concatenate(qs)
    if len(p) == 0:
        return p, q, np.zeros(0)
    rp = R.from_euler("zxz", euler[p], degrees=True).inv()
    rq = R.from_euler("zxz", euler[q], degrees=True)
    best = np.full(len(p), np.inf)
    for c in range(24):
        best = np.minimum(best, np.atleast_1d((rp * (SYM[c] * rq)).magnitude()))
    return p, q, np.degrees(best)


def _disorientation_to(rots, target):
    """min over S of |conj(r) (S target)| in degrees for every r of `rots`."""
    best = np.full(len(rots), np.inf)
    for c in range(24):
        best = np.minimum(best, np.atleast_1d((rots.inv() * (SYM[c] * target)).magnitude()))
    return np.degrees(best)


def segment(euler, scan_shape, threshold=THRESHOLD, connectivity=4, valid=None):
    """The five per-point outputs on the grid, the number of grains, and the two diagnostics
    `edge_margin` (the smallest |edge angle - threshold|) and `projection_gap` (the smallest gap
    between the best and the second-best equivalent of a member in the projection step)."""
    rows, cols = scan_shape
    n = rows * cols
    euler = np.asarray(euler, np.float64).reshape(n, 3)
    ok = usable_points(euler, valid)
    p, q, deg = edge_angles(euler, scan_shape, connectivity, ok)
    edge_margin = float(np.abs(deg - threshold).min()) if len(deg) else np.inf

    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(p[deg <= threshold], q[deg <= threshold]):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(x) for x in range(n)])            # the lowest flat index of the component

    grain_id = np.full(n, -1, np.int32)
    roots = np.unique(root[ok])                              # ascending = by first point
    grain_id[ok] = np.searchsorted(roots, root[ok])

    mean = np.full((n, 3), np.nan)
    grod = np.full(n, np.nan)
    gos = np.full(n, np.nan)
    projection_gap = np.inf
    mean_quat = {}
    for g, r in enumerate(roots):
        members = np.flatnonzero(grain_id == g)
        qr = R.from_euler("zxz", euler[r], degrees=True)
        rm = R.from_euler("zxz", euler[members], degrees=True)
        angles = np.stack([np.atleast_1d((qr.inv() * (SYM[c] * rm)).magnitude()) for c in range(24)])
        pick = angles.argmin(axis=0)                         # the first of the smallest
        two = np.sort(angles, axis=0)[:2]
        projection_gap = min(projection_gap, float(np.degrees(two[1] - two[0]).min()))
        eq = np.atleast_2d((SYM[pick] * rm).as_quat())
        ref = qr.as_quat()
        eq[eq @ ref < 0] *= -1.0
        total = eq.sum(axis=0)
        m = R.from_quat(total / np.linalg.norm(total))
        mean_quat[g] = m
        mean[members] = m.as_euler("zxz", degrees=True)
        grod[members] = _disorientation_to(rm, m)
        gos[members] = grod[members].mean()

    boundary = np.zeros(n, np.uint8)
    ids = grain_id.reshape(rows, cols)
    for i in range(rows):
        for j in range(cols):
            if ids[i, j] >= 0 and any(ids[a, b] != ids[i, j]
                                      for a, b in neighbours(i, j, rows, cols, connectivity)):
                boundary[i * cols + j] = 1
    return SimpleNamespace(grain_id=ids, grain_orientation=mean.reshape(rows, cols, 3),
                           grod=grod.reshape(rows, cols), gos=gos.reshape(rows, cols),
                           boundary=boundary.reshape(rows, cols), n_grains=len(roots),
                           mean_rotations=mean_quat, edge_margin=edge_margin,
                           projection_gap=projection_gap)


def rotation_angle_deg(euler_a, euler_b):
    """The plain rotation angle between two orientations given as ZXZ Euler degrees."""
    a = R.from_euler("zxz", np.asarray(euler_a).reshape(-1, 3), degrees=True)
    b = R.from_euler("zxz", np.asarray(euler_b).reshape(-1, 3), degrees=True)
    return np.degrees(np.atleast_1d((a.inv() * b).magnitude()))


# ---------------------------------------------------------------- cases
def _bases(rng, count):
    """`count` random orientations, every pair more than BASE_GAP apart under the cubic group."""
    quats = []
    while len(quats) < count:                      # one at a time: redraw only the newcomer
        new = R.random(random_state=int(rng.integers(1 << 30)))
        if not quats or _disorientation_to(R.from_quat(np.array(quats)), new).min() > BASE_GAP:
            quats.append(new.as_quat())
    return R.from_quat(np.array(quats))


def from_labels(labels, seed):
    """A label image -> (rows * cols, 3) Euler degrees: a base per label, up to NOISE degrees of
    noise per point, and a third of the points behind a cubic operator."""
    labels = np.asarray(labels)
    rows, cols = labels.shape
    rng = np.random.default_rng(seed)
    names = np.unique(labels)
    bases = _bases(rng, len(names))
    where = np.searchsorted(names, labels)
    e = np.empty((rows, cols, 3))
    for i in range(rows):
        for j in range(cols):
            axis = rng.standard_normal(3)
            noise = R.from_rotvec(np.radians(rng.uniform(0, NOISE)) * axis / np.linalg.norm(axis))
            rot = noise * bases[int(where[i, j])]
            if (i + 2 * j) % 3 == 1:
                rot = SYM[int(rng.integers(1, 24))] * rot
            e[i, j] = rot.as_euler("zxz", degrees=True)
    return e.reshape(-1, 3)


def quadrants(rows, cols):
    i, j = np.mgrid[:rows, :cols]
    return (i * 2 // max(rows, 2)) * 2 + (j * 2 // max(cols, 2))


def split(rows, cols, at):
    """Two labels: the flat indices below `at`, and the rest."""
    return (np.arange(rows * cols) >= at).astype(int).reshape(rows, cols)


def u_shape(size=12):
    lab = np.zeros((size, size), int)
    lab[:-1, 4:size - 4] = 1                      # the gap between the arms, open at the top
    return lab


def comb(size=12):
    lab = np.zeros((size, size), int)
    lab[:-1, 1::2] = 1                            # teeth in the even columns, joined by the last row
    lab[:-1, 1::4] = 2                            # two kinds of gap, each column its own grain
    return lab


def spirals(size=15):
    """Two interleaved rectangular spirals, each one cell wide: a walk from the top left corner
    that turns right whenever the cell ahead is off the grid or the one behind it is already on
    the walk; the cells it leaves out are the other spiral."""
    lab = np.zeros((size, size), int)

    def on_walk(a, b):
        return 0 <= a < size and 0 <= b < size and lab[a, b] == 1
    i = j = 0
    di, dj = 0, 1
    lab[0, 0] = 1
    while True:
        for _ in range(2):
            a, b = i + di, j + dj
            if 0 <= a < size and 0 <= b < size and not on_walk(a, b) and not on_walk(a + di, b + dj):
                break
            di, dj = dj, -di
        else:
            return lab
        i, j = a, b
        lab[i, j] = 1


def checkerboard(size=8):
    i, j = np.mgrid[:size, :size]
    return (i + j) % 2


def rings(size=9):
    i, j = np.mgrid[:size, :size]
    return np.minimum(np.minimum(i, j), np.minimum(size - 1 - i, size - 1 - j)) % 3


def voronoi(rows, cols, cell=8, seed=5):
    rng = np.random.default_rng(seed)
    count = (rows * cols) // (cell * cell)
    sites = np.stack([rng.uniform(0, rows, count), rng.uniform(0, cols, count)], 1)
    i, j = np.mgrid[:rows, :cols]
    d = (i[..., None] - sites[:, 0]) ** 2 + (j[..., None] - sites[:, 1]) ** 2
    return d.argmin(axis=2)


def chain(length=21, step=1.0, seed=3):
    """(1, length): every point `step` degrees about one axis from the one before."""
    rng = np.random.default_rng(seed)
    base = R.random(random_state=int(rng.integers(1 << 30)))
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    return np.stack([(R.from_rotvec(np.radians(step * k) * axis) * base).as_euler("zxz", degrees=True)
                     for k in range(length)])


SCAN_BLOCK = 4096      # points per block of the device's prefix sum (csrc/grains.hip kScanBlock)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (euler (n, 3), scan_shape, connectivity, valid or None, single grain?)"""
    def lab(labels, seed, conn=4, single=False):
        labels = np.asarray(labels)
        return from_labels(labels, seed), labels.shape, conn, None, single
    simple = {"1x1": (1, 1), "1x5": (1, 5), "5x1": (5, 1), "3x4": (3, 4), "7x9": (7, 9)}
    if name in simple:
        r, c = simple[name]
        return lab(quadrants(r, c), 11 + r * c, conn=8 if name == "7x9" else 4,
                   single=r * c == 1)
    table = {
        "1x65_one": lambda: lab(np.zeros((1, 65), int), 21, single=True),
        "2x129_one": lambda: lab(np.zeros((2, 129), int), 22, conn=8, single=True),
        "1x65_two": lambda: lab(split(1, 65, 37), 23),
        "2x129_two": lambda: lab(split(2, 129, 129 + 40), 24, conn=8),
        "u": lambda: lab(u_shape(), 25),
        "comb": lambda: lab(comb(), 26),
        "spirals": lambda: lab(spirals(), 27),
        "checker4": lambda: lab(checkerboard(), 28, conn=4),
        "checker8": lambda: lab(checkerboard(), 28, conn=8),
        "rings": lambda: lab(rings(), 29, conn=8),
        "voronoi": lambda: lab(voronoi(96, 96), 30),
        "chain": lambda: (chain(), (1, 21), 4, None, True),
    }
    if name in table:
        return table[name]()
    if name in ("3x4_bad", "7x9_bad"):
        e, shape, conn, _, _ = case(name[:3])
        e = e.copy()
        n = len(e)
        valid = np.ones(n, np.int32)
        if name == "3x4_bad":
            e[5, 1] = np.nan                     # (1, 1): an inner point
            e[11] = np.inf                       # the last corner
            valid[2] = 0
        else:
            e[0, 0], e[31, 2], e[40] = -np.inf, np.nan, np.nan
            valid[[8, 22, 23, 62]] = 0
        return e, shape, conn, valid, False
    if name == "1x3_lone":
        e = np.full((3, 3), np.nan)
        e[1] = [10.0, 20.0, 30.0]
        return e, (1, 3), 4, None, True
    raise KeyError(name)


CASES = ["1x1", "1x5", "5x1", "3x4", "7x9", "1x65_one", "2x129_one", "1x65_two", "2x129_two", "u",
         "comb", "spirals", "checker4", "checker8", "rings", "voronoi", "chain", "3x4_bad",
         "7x9_bad", "1x3_lone"]


@functools.lru_cache(maxsize=None)
def reference(name):
    e, shape, conn, valid, _ = case(name)
    return segment(e, shape, THRESHOLD, conn, valid)


def check_preconditions(name):
    """The conditions that keep a case honest (from the reference, on the CPU)."""
    _, _, _, _, single = case(name)
    ref = reference(name)
    assert ref.edge_margin >= EDGE_CAP, (name, ref.edge_margin)
    assert ref.projection_gap >= PROJECTION_CAP, (name, ref.projection_gap)
    if single:
        assert ref.n_grains == 1, (name, ref.n_grains)
    else:
        assert ref.n_grains >= 2, (name, ref.n_grains)
    return ref
