"""The dictionary simulation's host side (latice/simulation.py, tests/simulate_ref.py) and the
C ABI's refusals: no GPU needed."""
import math
import types

import numpy as np
import pytest
import torch

import simulate_ref as R
from latice import _native as N
from latice import data_module as D
from latice import simulation as S
from latice.index.dp_indexer import DiffractionPatternIndexer
from latice.patterns import PatternCorrection


# ------------------------------------------------------------------------------ (a)
def _triples():
    rng = np.random.default_rng(5)
    e = rng.uniform(-400.0, 400.0, size=(50, 3))
    special = np.array([[0, 0, 0], [37, 0, 112], [37, 180, 112], [-725, 180, 400], [90, 90, 90],
                        [361, 0, -361], [400, 45, -400], [0, 180, 0]], dtype=np.float64)
    return np.concatenate([e, special])


def test_orientation_matrix_is_the_inverse_of_scipys_intrinsic_zxz():
    from scipy.spatial.transform import Rotation
    e = _triples()
    ref = Rotation.from_euler("ZXZ", e, degrees=True).inv().as_matrix()
    for fn in (S.orientation_matrix, R.orientation_matrix):
        g = fn(e)
        assert g.shape == (len(e), 3, 3)
        assert np.abs(g - ref).max() < 2e-15
    # and it is not the extrinsic "zxz" reading the orientation consensus uses
    other = Rotation.from_euler("zxz", e[:50], degrees=True).as_matrix()
    assert np.abs(S.orientation_matrix(e[:50]) - other).max() > 0.1
    assert np.array_equal(S.orientation_matrix([0.0, 0.0, 0.0]), np.eye(3))


# ------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("lower", [False, True])
def test_lambert_forward_inverts_the_inverse_on_a_grid(lower):
    X, Y = R.lambert_grid(65)
    v = R.lambert_inverse(X, Y, lower)
    assert np.abs(np.linalg.norm(v, axis=-1) - 1.0).max() < 1e-15
    assert (v[..., 2] <= 0).all() if lower else (v[..., 2] >= 0).all()
    tx, ty, low = R.lambert_forward(v)
    assert np.abs(tx - X).max() < 1e-14 and np.abs(ty - Y).max() < 1e-14
    inner = np.abs(v[..., 2]) > 0
    assert (low[inner] == lower).all()


def test_lambert_forward_range_continuity_and_area():
    rng = np.random.default_rng(2)
    v = rng.standard_normal((20000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    tx, ty, _ = R.lambert_forward(v)
    assert max(np.abs(tx).max(), np.abs(ty).max()) <= 1.0 + 1e-15
    # continuous across |x| = |y|: the two branches give the same point there
    t = rng.uniform(0.01, 0.7, 2000)
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                z = sz * np.sqrt(1 - 2 * t * t)
                a = np.stack([sx * t, sy * t * (1 - 1e-9), z], -1)
                b = np.stack([sx * t * (1 - 1e-9), sy * t, z], -1)
                ta, tb = R.lambert_forward(a), R.lambert_forward(b)
                assert np.abs(ta[0] - tb[0]).max() < 5e-9 and np.abs(ta[1] - tb[1]).max() < 5e-9
    # poles and axes
    ax = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], float)
    tx, ty, low = R.lambert_forward(ax)
    assert np.array_equal(tx, [0, 0, 1, -1, 0, 0]) and np.array_equal(ty, [0, 0, 0, 0, 1, -1])
    assert np.array_equal(low, [False, True, False, False, False, False])
    # equal-area: uniform points of a hemisphere fill the square uniformly (4 x 4 cells)
    up = v[v[:, 2] > 0]
    tx, ty, _ = R.lambert_forward(up)
    hist, _, _ = np.histogram2d(tx, ty, bins=4, range=[[-1, 1], [-1, 1]])
    expect = len(up) / 16.0
    assert np.abs(hist - expect).max() < 6 * math.sqrt(expect)


def test_lambert_map_lipschitz_constant_is_below_the_gates():
    rng = np.random.default_rng(3)
    v = rng.standard_normal((200000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    d = rng.standard_normal(v.shape)
    d *= 1e-7 / np.linalg.norm(d, axis=1, keepdims=True)
    a, b = R.lambert_forward(v), R.lambert_forward(v + d)
    flip = a[2] != b[2]
    k = np.hypot(a[0] - b[0], a[1] - b[1]) / 1e-7
    assert k[~flip].max() < 2.0
    assert k[flip].max() < 2.0 if flip.any() else True


# ------------------------------------------------------------------------------ masters, gates
def test_smooth_master_agrees_on_the_equator_and_is_not_centrosymmetric():
    up, lo = R.smooth_master(21)
    assert R.equator_step(up, lo) == 0.0
    assert np.abs(up - lo).max() > 0.1
    assert np.abs(up - up[::-1, ::-1]).max() > 0.1


def test_ramp_master_reads_back_its_coordinates():
    up, lo = R.ramp_master(5)
    dirs = np.array([[0.0, 0.3, -0.2], [0.0, 0.1, 0.5], [1.0, 0.9, -0.8]], np.float32)
    dirs /= np.linalg.norm(dirs.astype(np.float64), axis=0).astype(np.float32)
    val, (r, u, low) = R.simulate(up, lo, dirs, [[0, 0, 0]], (1, 3), False)
    c0 = np.where(low, R.RAMP_C0[1], R.RAMP_C0[0])
    assert np.abs(val.reshape(1, 3) - (R.RAMP_A * r + R.RAMP_B * u + c0)).max() < 1e-12
    assert np.array_equal(low[0], [False, False, True])
    assert r[0, 0] == 2.0 and u[0, 0] == 2.0


# the (M, h, w, pc) of the GPU parity cases of tests/test_gpu_simulate.py: every gate stays below
# its cap, so a sample one texel off or from the wrong hemisphere cannot pass
GPU_CASES = [(21, 16, 12, (0.5, 0.5, 0.3)), (101, 128, 128, (0.5, 0.5, 0.5)),
             (101, 256, 256, (0.5, 0.5, 0.5))]


@pytest.mark.parametrize("M,h,w,pc", GPU_CASES)
def test_gates_stay_below_their_caps(M, h, w, pc):
    up, lo = R.smooth_master(M)
    assert R.gate(up, lo) < R.cap(up, lo)
    det = S.DetectorGeometry((h, w), pc=pc)
    ref, _ = R.simulate(up, lo, det.planar_directions(), [[10.0, 95.0, 20.0]], (h, w), False)
    rng_ = ref.max() - ref.min()
    assert R.gate(up, lo, rng_) < R.cap(up, lo, rng_)
    ramp = R.ramp_master(3)
    assert R.gate(*ramp, equator=0.0) < min(R.RAMP_A, R.RAMP_B) / 50.0


# ------------------------------------------------------------------------------ DetectorGeometry
def test_detector_directions_follow_the_stated_formula():
    det = S.DetectorGeometry((6, 8), pc=(0.4, 0.3, 0.7), sample_tilt=70.0, tilt=5.0, azimuthal=3.0)
    v = det.direction_cosines()
    assert v.shape == (48, 3) and v.dtype == np.float64
    assert np.abs(np.linalg.norm(v, axis=1) - 1.0).max() < 1e-15
    al, om = math.radians(90 - 70 + 5), math.radians(3.0)
    for i, j in ((0, 0), (5, 7), (2, 3)):
        dx = ((j + 0.5) / 8 - 0.4) * (8 / 6)
        dy = 0.3 - (i + 0.5) / 6
        Ls = -math.sin(om) * dx + 0.7 * math.cos(om)
        Lc = math.cos(om) * dx + 0.7 * math.sin(om)
        e = np.array([dy * math.cos(al) + math.sin(al) * Ls, Lc, -math.sin(al) * dy + math.cos(al) * Ls])
        assert np.abs(v[i * 8 + j] - e / np.linalg.norm(e)).max() < 1e-15
    p = det.planar_directions()
    assert p.shape == (3, 48) and p.dtype == np.float32 and p.flags.c_contiguous
    assert np.array_equal(p, v.T.astype(np.float32))


def test_detector_pattern_centre_and_handedness():
    # an odd detector with the PC on the centre of its middle pixel
    h, w = 5, 7
    det = S.DetectorGeometry((h, w), pc=((3 + 0.5) / w, (2 + 0.5) / h, 0.6), sample_tilt=70.0)
    v = det.direction_cosines().reshape(h, w, 3)
    al = math.radians(20.0)
    assert np.abs(v[2, 3] - [math.sin(al), 0.0, math.cos(al)]).max() < 1e-15
    # right-handed: the image axes and the ray, (towards the next column) x (towards the next
    # row, downwards) along the direction of the centre pixel, for every tilt and azimuth
    # (the pattern as seen from the detector side; a mirrored mapping would give -1)
    for kw in ({}, {"tilt": 12.0}, {"azimuthal": 20.0}, {"sample_tilt": 55.0, "tilt": -7.0, "azimuthal": -15.0}):
        v = S.DetectorGeometry((h, w), pc=((3 + 0.5) / w, (2 + 0.5) / h, 0.6), **kw) \
            .direction_cosines().reshape(h, w, 3)
        right, down = v[2, 4] - v[2, 3], v[3, 3] - v[2, 3]
        n = np.cross(right, down)
        assert n @ v[2, 3] / np.linalg.norm(n) > 0.9     # chords of a coarse grid, not tangents
    # with no azimuth the columns run along the sample's +y, the rows above towards +x
    v = det.direction_cosines().reshape(h, w, 3)
    assert v[2, 4, 1] > 0 and abs(v[1, 3, 1]) < 1e-15 and v[1, 3, 0] > v[2, 3, 0]
    assert S.DetectorGeometry(4).shape == (4, 4)


def test_detector_directions_override_is_normalised_and_passed_through():
    rng = np.random.default_rng(1)
    d = rng.standard_normal((3, 4, 3)) * 5.0
    det = S.DetectorGeometry((3, 4), directions=d)
    e = d.reshape(12, 3) / np.linalg.norm(d.reshape(12, 3), axis=1, keepdims=True)
    assert np.array_equal(det.direction_cosines(), e)
    assert np.array_equal(S.DetectorGeometry((3, 4), directions=d.reshape(12, 3)).direction_cosines(), e)
    for bad in (np.zeros((12, 3)), np.ones((11, 3)), np.full((12, 3), np.nan), np.ones((4, 3, 3))):
        with pytest.raises(ValueError):
            S.DetectorGeometry((3, 4), directions=bad)
    for shape in ((0, 4), (4, 257), (4,), (1, 2, 3), "ab"):
        with pytest.raises(ValueError):
            S.DetectorGeometry(shape)
    for pc in ((0.5, 0.5), (0.5, 0.5, 0.0), (0.5, np.nan, 0.5)):
        with pytest.raises(ValueError):
            S.DetectorGeometry((4, 4), pc=pc)


# ------------------------------------------------------------------------------ ValueErrors
@pytest.fixture
def no_device(monkeypatch):
    """Anything that would touch the device fails the test."""
    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(S.N, "call", boom)
    monkeypatch.setattr(S.MasterPattern, "_on", boom)
    monkeypatch.setattr(S.DetectorGeometry, "_on", boom)


def test_master_pattern_checks_its_arrays():
    m = S.MasterPattern(np.ones((5, 5)))
    assert m.side == 5 and m.centrosymmetric and m.upper.dtype == np.float32
    both = S.MasterPattern(np.arange(18.0).reshape(2, 3, 3))
    assert not both.centrosymmetric and both.lower[0, 0] == 9.0
    assert not S.MasterPattern(np.ones((3, 3)), np.zeros((3, 3))).centrosymmetric
    nan = np.ones((5, 5))
    nan[2, 2] = np.nan
    inf = np.ones((5, 5))
    inf[0, 4] = np.inf
    for bad in (np.ones((5, 4)), np.ones((4, 4)), np.ones((1, 1)), np.ones((4099, 1)), np.ones(5),
                nan, inf, np.ones((3, 5, 5)), np.ones((5, 5), dtype=complex)):
        with pytest.raises(ValueError):
            S.MasterPattern(bad)
    with pytest.raises(ValueError):
        S.MasterPattern(np.ones((5, 5)), np.ones((7, 7)))
    with pytest.raises(ValueError):
        S.MasterPattern(np.ones((5, 5)), nan)
    assert D.MasterPattern is S.MasterPattern and D.simulate_patterns is S.simulate_patterns
    assert D.DetectorGeometry is S.DetectorGeometry


def test_simulate_patterns_checks_before_the_device(no_device):
    m = S.MasterPattern(np.ones((5, 5)))
    det = S.DetectorGeometry((4, 6))
    ok = np.zeros((2, 3))
    bad_calls = [
        (np.ones((5, 5)), ok, det, {}),
        (m, ok, (4, 6), {}),
        (m, np.zeros((2, 4)), det, {}),
        (m, np.zeros((2, 3, 1)), det, {}),
        (m, np.zeros((2, 3), np.float32), det, {}),
        (m, torch.zeros(2, 3), det, {}),
        (m, np.zeros(4), det, {}),
        (m, np.array([[0.0, np.nan, 0.0]]), det, {}),
        (m, "abc", det, {}),
        (m, ok, det, {"out": torch.empty(2, 1, 4, 5)}),
        (m, ok, det, {"out": torch.empty(2, 1, 4, 6, dtype=torch.float64)}),
        (m, ok, det, {"out": torch.empty(2, 1, 6, 4).transpose(2, 3)}),
    ]
    for master, ori, d, kw in bad_calls:
        with pytest.raises(ValueError):
            S.simulate_patterns(master, ori, d, **kw)
    # no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.simulate_patterns(m, ok, det, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.simulate_patterns(m, ok, det, out=torch.empty(2, 1, 4, 6))


def _bare_indexer(image_size=(128, 128)):
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was used before the arguments were checked")
    ix = object.__new__(DiffractionPatternIndexer)
    ix.config = types.SimpleNamespace(image_size=image_size, batch_size=16)
    ix.device = torch.device("cuda")
    ix.model, ix.db = Untouchable(), Untouchable()
    return ix


def test_build_dictionary_from_master_checks_before_the_device(no_device):
    ix = _bare_indexer()
    m = S.MasterPattern(np.ones((5, 5)))
    ori = np.zeros((4, 3))
    bg = PatternCorrection(static_background=np.ones((128, 128)), dynamic_sigma=2.0)
    bad_calls = [
        dict(master=np.ones((5, 5)), orientations=ori),
        dict(master=m, orientations=ori, detector=S.DetectorGeometry((64, 64))),
        dict(master=m, orientations=ori, detector=(128, 128)),
        dict(master=m, orientations=np.zeros((4, 2))),
        dict(master=m, orientations=np.zeros((4, 3), np.float32)),
        dict(master=m, orientations=np.zeros((0, 3))),
        dict(master=m, orientations=ori, batch_size=-1),
        dict(master=m, orientations=ori, correction=bg),
        dict(master=m, orientations=ori, correction="dynamic"),
        dict(master=m, orientations=ori, correction=PatternCorrection(dynamic_sigma=100.0)),
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            ix.build_dictionary_from_master(**kw)
    ix.device = torch.device("cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ix.build_dictionary_from_master(m, ori)


# ------------------------------------------------------------------------------ the C ABI
def test_abi_version_is_5_and_the_entry_point_is_bound():
    assert N.ABI_VERSION == 5
    assert N.load().ebsdvae_version() == 5
    assert "ebsdvae_simulate_patterns" in N.SIGNATURES


def test_c_abi_refusals_without_gpu():
    """Every refusal comes from argument validation, before any launch; the pointers are never
    dereferenced on the host, so any non-null value stands in for one."""
    p = 4096
    good = dict(up=p, lo=p, M=5, dirs=p, euler=p, B=2, h=4, w=6, rescale=1, dst=p)

    def call(**kw):
        a = dict(good, **kw)
        return N.call("ebsdvae_simulate_patterns", a["up"], a["lo"], a["M"], a["dirs"], a["euler"],
                      a["B"], a["h"], a["w"], a["rescale"], a["dst"], None)

    for name in ("up", "lo", "dirs", "euler", "dst"):
        with pytest.raises(RuntimeError, match="null pointer"):
            call(**{name: None})
    for M in (4, 1, 2, 0, -3, 4098, 4099):
        with pytest.raises(RuntimeError, match="master side"):
            call(M=M)
    for h, w in ((0, 6), (4, 0), (257, 6), (4, 257), (-1, 6)):
        with pytest.raises(RuntimeError, match="detector"):
            call(h=h, w=w)
    with pytest.raises(RuntimeError, match="B = -1"):
        call(B=-1)
    for r in (-1, 2):
        with pytest.raises(RuntimeError, match="rescale"):
            call(rescale=r)
    assert call(B=0) == 0
    assert call(B=0, M=4097, h=256, w=256, rescale=0) == 0
