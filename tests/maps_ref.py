"""The scan maps of latice/index/maps.py (csrc/scan_maps.hip) in float64 numpy / scipy, written
from their definitions in include/ebsdvae.h: the reference for the host and the GPU tests."""
from math import acos, atan2, sqrt

import numpy as np
from scipy.spatial.transform import Rotation as R

# QUAT_SYM, scalar last, in the order of the reference's latice/utils/constants.py:13-39
_H = 0.5
_S = 1.0 / np.sqrt(2.0)
CUBIC_SYMMETRY = [
    [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1],
    [_H, _H, _H, _H], [_H, -_H, -_H, -_H], [_H, _H, -_H, _H], [_H, -_H, _H, -_H],
    [_H, -_H, _H, _H], [_H, _H, -_H, -_H], [_H, -_H, -_H, _H], [_H, _H, _H, -_H],
    [_S, _S, 0, 0], [_S, 0, _S, 0], [_S, 0, 0, _S], [_S, -_S, 0, 0], [_S, 0, -_S, 0], [_S, 0, 0, -_S],
    [0, _S, _S, 0], [0, -_S, _S, 0], [0, 0, _S, _S], [0, 0, -_S, _S], [0, _S, 0, _S], [0, -_S, 0, _S],
]
SYM = R.from_quat(CUBIC_SYMMETRY)
AXES = {"x": 0, "y": 1, "z": 2}
ETA_MAX = 45.0 * (np.pi / 180.0)
CHI_MAX = acos(1.0 / sqrt(3.0))


def offsets(connectivity):
    """The neighbour offsets (a, b), a ascending then b ascending: the cross or the square."""
    assert connectivity in (4, 8)
    return [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)
            if (a, b) != (0, 0) and (connectivity == 8 or a == 0 or b == 0)]


def neighbours(i, j, rows, cols, connectivity):
    return [(i + a, j + b) for a, b in offsets(connectivity)
            if 0 <= i + a < rows and 0 <= j + b < cols]


def ipf_one(v):
    """The colour of one direction: the first cubic equivalent (the 24 of QUAT_SYM, then their
    negations, each flipped to z >= 0) inside 0 <= eta <= 45 deg, 0 <= chi <= acos(1 / sqrt 3)."""
    v = np.asarray(v, np.float64) / np.linalg.norm(v)
    eq = SYM.as_matrix() @ v
    chi = eta = 0.0
    for e in np.concatenate([eq, -eq]):
        if e[2] < 0:
            e = -e
        chi, eta = acos(min(e[2], 1.0)), atan2(e[1], e[0])
        if 0 <= eta <= ETA_MAX and 0 <= chi <= CHI_MAX:
            break
    c = np.degrees(chi) / np.degrees(CHI_MAX)
    f = abs(np.degrees(eta)) / 45.0
    rgb = np.sqrt(np.array([1.0 - c, (1.0 - f) * c, f * c]))
    return np.rint(255.0 * rgb / rgb.max()).astype(np.uint8)


def ipf(euler, direction="z"):
    """(n, 3) ZXZ Euler degrees -> (n, 3) uint8; a non-finite row gives (0, 0, 0)."""
    euler = np.asarray(euler, np.float64).reshape(-1, 3)
    out = np.zeros((len(euler), 3), np.uint8)
    ok = np.isfinite(euler).all(axis=1)
    if ok.any():
        rows = R.from_euler("zxz", euler[ok], degrees=True).as_matrix()[:, AXES[direction], :]
        out[ok] = [ipf_one(v) for v in rows]
    return out


def osm(cand, scan_shape, connectivity=4, normalize=False):
    """(rows * cols, k) int64 -> (rows, cols) float32: per point the entries >= 0 of its row that
    occur in a neighbour's row, summed over the neighbours, over their number (and over k)."""
    rows, cols = scan_shape
    cand = np.asarray(cand).reshape(rows, cols, -1)
    k = cand.shape[2]
    out = np.zeros((rows, cols), np.float32)
    for i in range(rows):
        for j in range(cols):
            nb = neighbours(i, j, rows, cols, connectivity)
            if not nb:
                continue
            total = sum(int(x >= 0 and x in set(cand[a, b].tolist()))
                        for a, b in nb for x in cand[i, j].tolist())
            v = np.float32(total) / np.float32(len(nb))
            out[i, j] = v / np.float32(k) if normalize else v
    return out


def disorientation(ep, eq):
    """min over the 24 operators S of |conj(q_p) (S q_q)| in degrees."""
    p = R.from_euler("zxz", ep, degrees=True)
    q = R.from_euler("zxz", eq, degrees=True)
    return float(np.degrees((p.inv() * (SYM * q)).magnitude().min()))


def neighbour_angles(euler, scan_shape, connectivity=4):
    """{(i, j): [disorientation to every finite on-grid neighbour, in offset order]} for the
    points whose own row is finite."""
    rows, cols = scan_shape
    e = np.asarray(euler, np.float64).reshape(rows, cols, 3)
    fin = np.isfinite(e).all(axis=2)
    return {(i, j): [disorientation(e[i, j], e[a, b])
                     for a, b in neighbours(i, j, rows, cols, connectivity) if fin[a, b]]
            for i in range(rows) for j in range(cols) if fin[i, j]}


def kam(euler, scan_shape, connectivity=4, max_angle=5.0):
    """(rows * cols, 3) -> (rows, cols) float64 (the device rounds it to float32): the mean of the
    neighbour angles <= max_angle, 0 without any, NaN where the point's own row is not finite."""
    out = np.full(scan_shape, np.nan)
    for (i, j), w in neighbour_angles(euler, scan_shape, connectivity).items():
        kept = [x for x in w if x <= max_angle]
        out[i, j] = sum(kept) / len(kept) if kept else 0.0
    return out
