"""Record the reference's IPF colours for tests/test_scan_maps_host.py and
tests/test_gpu_scan_maps.py (needs a checkout of the reference; nothing of it is stored but the
colours it returns).

What `get_color_key(euler, "ipf_x" / "ipf_y" / "ipf_z")` (latice/utils/utils.py:206-240) does, without
importing that module (it pulls in plotting packages): rows 0 / 1 / 2 of
`R.from_euler("zxz", euler, degrees=True).as_matrix()` through
`ColorKeyGenerator.generate_ipf_color` (latice/utils/colorkey.py:64-130), one orientation at a time.

Inputs: 1024 seeded random Euler triples; 8 with the second angle 0, the exact [001] pole of
ipf_z; and 8 whose ipf_z direction approaches the [101] and [111] corners of the colour sector
from 1e-3 degrees inside (the exact corners sit on the sector's edge, where one ulp picks another
equivalent: they are left out).  With ZXZ angles (a, b, c) the ipf_z direction is
(sin a sin b, cos a sin b, cos b): polar angle b, azimuth 90 - a.

    python tests/golden/make_ipf_golden.py --ref <reference root>   ->  tests/golden/ipf_colors.npz
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def inputs() -> np.ndarray:
    rng = np.random.default_rng(20260)
    e = np.stack([rng.uniform(-180, 180, 1024), rng.uniform(0, 180, 1024),
                  rng.uniform(-180, 180, 1024)], axis=1)
    pole = np.stack([rng.uniform(-180, 180, 8), np.zeros(8), rng.uniform(-180, 180, 8)], axis=1)
    d = 1e-3
    chi111 = np.degrees(np.arccos(1.0 / np.sqrt(3.0)))
    corners = []
    for c in (0.0, 37.0, -112.5, 180.0):
        corners.append([90.0 - d, 45.0 - d, c])          # towards [101]: chi 45, eta 0
        corners.append([45.0 + d, chi111 - d, c])        # towards [111]: chi 54.74, eta 45
    return np.concatenate([e, pole, np.array(corners)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("LATICE_REFERENCE_ROOT", ""))
    a = ap.parse_args()
    if not a.ref:
        sys.exit("give the reference root with --ref or LATICE_REFERENCE_ROOT")
    sys.path.insert(0, a.ref)
    from scipy.spatial.transform import Rotation as R

    from latice.utils.colorkey import ColorKeyGenerator
    gen = ColorKeyGenerator()
    euler = inputs()
    m = R.from_euler("zxz", euler, degrees=True).as_matrix()
    out = {"euler": euler}
    for axis, name in enumerate("xyz"):
        out["ipf_" + name] = np.array([gen.generate_ipf_color(m[i, axis, :])
                                       for i in range(len(euler))], dtype=np.uint8)
    path = os.path.join(HERE, "ipf_colors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
