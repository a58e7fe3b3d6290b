"""The dictionary simulation on the device (csrc/simulate.hip, latice/simulation.py) against the
float64 restatement of tests/simulate_ref.py at its derived gate: through the C ABI on guarded
outputs, then the Python surface and `build_dictionary_from_master`.

Measured on an MI355X (max |out - reference| of the raw output, and its gate; every test prints
its own figures; DESIGN.md section 14, "Dictionary simulation", has the table):
    ramp M 3, 5 x 7        2.93e-06 / 1.87e-04      smooth M 101, 256 x 256   2.32e-06 / 9.34e-05
    smooth M 21, 16 x 12   1.96e-06 / 7.39e-05      smooth M 21, 129 x 131    2.09e-06 / 7.39e-05
    smooth M 101, 128^2    2.10e-06 / 9.34e-05      smooth M 21, 1 x 256      1.09e-06 / 7.39e-05
rescaled outputs: at most 0.007 of their gate."""
import functools

import numpy as np
import pytest
import torch

import rect_util as RU
import simulate_ref as R
from latice import _native as N
from latice import simulation as S
from latice.data_module import correct_patterns
from latice.index import faiss_db as F
from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig
from latice.model import VariationalAutoEncoderRawData
from latice.patterns import PatternCorrection
from latice.seeding import seeded_state_dict

pytestmark = pytest.mark.gpu

NAME = "ebsdvae_simulate_patterns"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def abi(up, lo, dirs, euler, shape, rescale, must=True, out=None, M=None, B=None):
    """One call through the C ABI into a guarded output; returns (accepted, the Guarded)."""
    h, w = shape
    B = len(euler) if B is None else B
    g = out if out is not None else RU.Guarded((max(B, 1), 1, h, w), max(B, 1))
    ok = RU.run(NAME, [g], RU.p(up), RU.p(lo), up.shape[0] if M is None else M, RU.p(dirs),
                RU.p(euler), B, h, w, rescale, g.ptr(), RU.stream(), must=must)
    return ok, g


def parity(master, dirs32, euler, shape, label, equator=None, caps=True):
    """rescale 0 and 1 of one case against the reference at the gate; prints the maxima."""
    up, lo = master
    up_d, lo_d = dev(up), (dev(lo) if lo is not up else None)
    lo_d = up_d if lo_d is None else lo_d
    dirs_d, eu_d = dev(dirs32), dev(np.asarray(euler, np.float64))
    B = len(euler)
    ref, (_, _, low) = R.simulate(up, lo, dirs32, euler, shape, False)
    _, g = abi(up_d, lo_d, dirs_d, eu_d, shape, 0)
    assert g.written()
    raw = g.t.double().cpu().numpy()
    gate = R.gate(up, lo, equator=equator)
    err = np.abs(raw - ref).max()
    print(f"{label}: raw max err {err:.3e} gate {gate:.3e}")
    if caps:
        assert gate < R.cap(up, lo)
    assert err <= gate, (label, err, gate)
    _, g1 = abi(up_d, lo_d, dirs_d, eu_d, shape, 1)
    res = g1.t.double().cpu().numpy()
    ref1 = R.rescale(ref)
    worst = 0.0
    for b in range(B):
        rng_ = ref[b].max() - ref[b].min()
        gb = R.gate(up, lo, rng_, equator=equator)
        if caps:
            assert gb < R.cap(up, lo, rng_)
        eb = np.abs(res[b] - ref1[b]).max()
        worst = max(worst, eb / gb)
        assert eb <= gb, (label, b, eb, gb)
        assert res[b].min() == 0.0 and res[b].max() == 1.0
    print(f"{label}: rescaled max err / gate {worst:.3f}")
    return raw, res, low


# ------------------------------------------------------------------------------ 1
def _special_directions():
    """Poles, axes, |x| = |y| in the four quadrants (both signs of z), z = +-0.0, and every one
    of them with each component moved one float32 ulp either way."""
    a = np.float32(0.5)
    zq = np.float32(np.sqrt(0.5))
    base = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)]
    base += [(sx * a, sy * a, sz * zq) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    base += [(0.6, 0.8, 0.0), (0.6, 0.8, -0.0), (-0.8, 0.6, 0.0), (0.0, -1.0, -0.0)]
    out = []
    for v in base:
        v = np.array(v, np.float32)
        out.append(v)
        for c in range(3):
            for to in (np.float32(np.inf), np.float32(-np.inf)):
                m = v.copy()
                m[c] = np.nextafter(v[c], to)
                out.append(m)
    return np.array(out, np.float32)          # (K, 3)


def test_ramp_master_special_directions():
    """M = 3 (n = 1), 5 x 7 (35 pixels: the scalar path, no store a whole line), B = 3: the
    clamps, the int(u) = 2n edge, the branch choice and the hemisphere rule, read back from a
    ramp master.  The orientations turn about z only, so v_z = d_z exactly on the device and in
    the reference (checked below): the hemisphere is never in doubt, equator = 0 in the gate."""
    up, lo = R.ramp_master(3)
    euler = np.array([[0.0, 0.0, 0.0], [90.0, 0.0, 0.0], [30.0, 0.0, 100.0]])
    g32 = R.orientation_matrix(euler).astype(np.float32)
    assert (g32[:, 2, :] == [0, 0, 1]).all() and (g32[:, :2, 2] == 0).all()
    assert np.array_equal(g32[0], np.eye(3, dtype=np.float32))
    vecs = _special_directions()
    gate = R.gate(up, lo, equator=0.0)
    assert gate < min(R.RAMP_A, R.RAMP_B) / 50.0
    up_d, lo_d, eu_d = dev(up), dev(lo), dev(euler)
    worst = 0.0
    for s in range(0, len(vecs), 35):
        chunk = vecs[s:s + 35]
        chunk = np.concatenate([chunk, np.repeat(chunk[-1:], 35 - len(chunk), 0)])
        dirs32 = np.ascontiguousarray(chunk.T)
        ref, (r, u, low) = R.simulate(up, lo, dirs32, euler, (5, 7), False)
        _, g = abi(up_d, lo_d, dev(dirs32), eu_d, (5, 7), 0)
        out = g.t.double().cpu().numpy()
        worst = max(worst, np.abs(out - ref).max())
        assert np.abs(out - ref).max() <= gate
        # the identity reads its coordinates back exactly where they are exact
        c0 = np.where(low[0], R.RAMP_C0[1], R.RAMP_C0[0])
        assert np.abs(out[0].ravel() - (R.RAMP_A * r[0] + R.RAMP_B * u[0] + c0)).max() <= gate
        # hemisphere: lower iff z < 0, and -0.0 is not
        hemi = out[0].ravel() > 20.0
        assert np.array_equal(hemi, chunk[:, 2] < 0)
        _, g1 = abi(up_d, lo_d, dev(dirs32), eu_d, (5, 7), 1)
        res, ref1 = g1.t.double().cpu().numpy(), R.rescale(ref)
        for b in range(3):
            gb = R.gate(up, lo, ref[b].max() - ref[b].min(), equator=0.0)
            assert np.abs(res[b] - ref1[b]).max() <= gb
    print(f"ramp: raw max err {worst:.3e} gate {gate:.3e}")
    # exact hits of the identity: pole, -pole, +x (u = 2n: j0 = 2n - 1, fu = 1), -y (r = 0)
    dirs32 = np.zeros((3, 35), np.float32)
    dirs32[:, :4] = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0]], np.float32).T
    dirs32[2, 4:] = 1.0
    _, g = abi(up_d, lo_d, dev(dirs32), eu_d, (5, 7), 0)
    first = g.t[0].ravel()[:4].cpu().numpy()
    a, b = R.RAMP_A, R.RAMP_B
    assert np.array_equal(first, np.array([a + b + 2, a + b + 40, a + 2 * b + 2, b + 2], np.float32))


# ------------------------------------------------------------------------------ 2
def test_both_hemispheres_in_one_pattern():
    """M = 21, 16 x 12, B = 5, a wide detector (pcz 0.3) and orientations that put the equator
    through the pattern."""
    det = S.DetectorGeometry((16, 12), pc=(0.5, 0.5, 0.3))
    euler = np.array([[0.0, 90.0, 0.0], [10.0, 95.0, 20.0], [200.0, 80.0, -30.0], [0.0, 0.0, 0.0],
                      [45.0, 180.0, 10.0]])
    _, _, low = parity(R.smooth_master(21), det.planar_directions(), euler, (16, 12), "M21 16x12")
    mixed = [0 < low[b].sum() < low[b].size for b in range(5)]
    assert sum(mixed) >= 3, mixed


# ------------------------------------------------------------------------------ 3
def test_constant_master_gives_zeros_under_rescale():
    m = np.full((5, 5), 3.25, np.float32)
    m_d = dev(m)
    det = S.DetectorGeometry((16, 12), pc=(0.5, 0.5, 0.3))
    dirs_d = dev(det.planar_directions())
    eu_d = dev(np.array([[10.0, 95.0, 20.0], [0.0, 0.0, 0.0]]))
    _, g = abi(m_d, m_d, dirs_d, eu_d, (16, 12), 1)
    assert bool((g.t == 0).all())
    _, g = abi(m_d, m_d, dirs_d, eu_d, (16, 12), 0)
    assert bool((g.t == 3.25).all())


# ------------------------------------------------------------------------------ 4, 5
FULL_EULER = np.array([[12.0, 0.0, 33.0], [250.0, 180.0, 40.0], [77.0, 54.0, 310.0]])


def test_full_size_128():
    """M = 101, 128 x 128, B = 3, default geometry: the register path; Phi = 0 and Phi = 180."""
    det = S.DetectorGeometry((128, 128))
    parity(R.smooth_master(101), det.planar_directions(), FULL_EULER, (128, 128), "M101 128x128")


def test_full_size_256():
    """256 x 256, B = 2, M = 101: the path that rescales its own stores in place."""
    det = S.DetectorGeometry((256, 256))
    parity(R.smooth_master(101), det.planar_directions(), FULL_EULER[1:], (256, 256), "M101 256x256")


def test_odd_sizes_past_the_register_limit():
    """129 x 131 = 16899 pixels: no multiple of 4 and more than 128 x 128, the scalar form of
    the in-place path; 1 x 1 and 1 x 256 are the smallest and a one-row detector."""
    det = S.DetectorGeometry((129, 131), pc=(0.45, 0.55, 0.6))
    parity(R.smooth_master(21), det.planar_directions(), FULL_EULER[1:], (129, 131), "M21 129x131")
    det = S.DetectorGeometry((1, 256), pc=(0.5, 0.5, 60.0))
    parity(R.smooth_master(21), det.planar_directions(), FULL_EULER, (1, 256), "M21 1x256")
    up, lo = R.smooth_master(21)
    d1 = np.array([[0.6], [0.0], [0.8]], np.float32)
    ref, _ = R.simulate(up, lo, d1, FULL_EULER, (1, 1), False)
    assert R.gate(up, lo) < R.cap(up, lo)
    _, g = abi(dev(up), dev(lo), dev(d1), dev(FULL_EULER), (1, 1), 0)
    assert np.abs(g.t.double().cpu().numpy() - ref).max() <= R.gate(up, lo)
    _, g = abi(dev(up), dev(lo), dev(d1), dev(FULL_EULER), (1, 1), 1)
    assert bool((g.t == 0).all())


# ------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("shape,pcz", [((16, 12), 0.3), ((128, 128), 0.5), ((130, 128), 0.5)])
def test_batch_independence_and_paths_agree(shape, pcz):
    """B = 7 in one call against 3 + 4 and 7 x 1, byte for byte; and the one-pixel-per-thread
    form (taken for an output that is not 16-byte aligned) against the four-pixel one."""
    h, w = shape
    up, lo = R.smooth_master(21)
    up_d, lo_d = dev(up), dev(lo)
    dirs_d = dev(S.DetectorGeometry(shape, pc=(0.5, 0.5, pcz)).planar_directions())
    euler = R.spread_orientations(7, seed=3)
    euler[2] = [0.0, 90.0, 0.0]
    eu_d = dev(euler)
    for rescale in (0, 1):
        _, whole = abi(up_d, lo_d, dirs_d, eu_d, shape, rescale)
        parts = [abi(up_d, lo_d, dirs_d, eu_d[a:b].contiguous(), shape, rescale)[1].t
                 for a, b in ((0, 3), (3, 7))]
        assert torch.equal(whole.t, torch.cat(parts))
        ones = [abi(up_d, lo_d, dirs_d, eu_d[b:b + 1].contiguous(), shape, rescale)[1].t
                for b in range(7)]
        assert torch.equal(whole.t, torch.cat(ones))
        # the same bytes one float past a 16-byte boundary (the scalar form of the kernel)
        buf = torch.full((7 * h * w + 8,), RU.SENTINEL, device="cuda")
        off = buf[1:1 + 7 * h * w]
        assert off.data_ptr() % 16 == 4
        N.call(NAME, N.ptr(up_d), N.ptr(lo_d), 21, N.ptr(dirs_d), eu_d.data_ptr(), 7, h, w,
               rescale, off.data_ptr(), N.stream())
        assert torch.equal(off.view(7, 1, h, w), whole.t)
        assert float(buf[0]) == RU.SENTINEL and bool((buf[1 + 7 * h * w:] == RU.SENTINEL).all())


# ------------------------------------------------------------------------------ 7
def test_refusals_leave_the_output_untouched():
    up, lo = R.smooth_master(21)
    up_d, lo_d = dev(up), dev(lo)
    dirs_d = dev(S.DetectorGeometry((16, 12)).planar_directions())
    eu_d = dev(FULL_EULER)
    g = RU.Guarded((3, 1, 16, 12), 3)
    lib = N.load()

    def refused(*args):
        rc = getattr(lib, NAME)(*args)
        torch.cuda.synchronize()
        assert rc != 0 and lib.ebsdvae_last_error().decode().strip()
        assert g.untouched()

    a = [RU.p(up_d), RU.p(lo_d), 21, RU.p(dirs_d), RU.p(eu_d), 3, 16, 12, 1, g.ptr(), RU.stream()]
    for i in (0, 1, 3, 4):
        refused(*[None if k == i else v for k, v in enumerate(a)])
    for M in (20, 22, 1, 4099):
        refused(*[M if k == 2 else v for k, v in enumerate(a)])
    for k, bad in ((6, 0), (6, 257), (7, 0), (7, 257), (5, -1), (8, 2), (8, -1)):
        refused(*[bad if i == k else v for i, v in enumerate(a)])
    assert getattr(lib, NAME)(*[0 if k == 5 else v for k, v in enumerate(a)]) == 0   # B = 0
    torch.cuda.synchronize()
    assert g.untouched()
    assert getattr(lib, NAME)(*[None if k == 9 else v for k, v in enumerate(a)]) != 0  # null dst


# ------------------------------------------------------------------------------ the Python surface
def test_simulate_patterns_python_surface():
    up, lo = R.smooth_master(21)
    master = S.MasterPattern(up, lo)
    det = S.DetectorGeometry((16, 12), pc=(0.5, 0.5, 0.3))
    euler = R.spread_orientations(5, seed=1)
    x = S.simulate_patterns(master, euler, det)
    assert x.shape == (5, 1, 16, 12) and x.dtype == torch.float32 and x.is_cuda
    ref, _ = R.simulate(up, lo, det.planar_directions(), euler, (16, 12), True)
    raw, _ = R.simulate(up, lo, det.planar_directions(), euler, (16, 12), False)
    assert R.gate(up, lo) < R.cap(up, lo) and R.gate(up, up) < R.cap(up, up)
    for b in range(5):
        gb = R.gate(up, lo, raw[b].max() - raw[b].min())
        assert gb < R.cap(up, lo, raw[b].max() - raw[b].min())
        assert np.abs(x[b].double().cpu().numpy() - ref[b]).max() <= gb
    # device orientations, one triple, out=, rescale=False, a stacked and a centrosymmetric master
    assert torch.equal(S.simulate_patterns(master, dev(euler), det), x)
    assert torch.equal(S.simulate_patterns(master, euler[2], det), x[2:3])
    out = torch.empty(5, 1, 16, 12, device="cuda")
    assert S.simulate_patterns(master, euler, det, out=out) is out and torch.equal(out, x)
    y = S.simulate_patterns(S.MasterPattern(np.stack([up, lo])), euler, det, rescale=False)
    assert np.abs(y.double().cpu().numpy() - raw).max() <= R.gate(up, lo)
    sym, _ = R.simulate(up, up, det.planar_directions(), euler, (16, 12), False)
    z = S.simulate_patterns(S.MasterPattern(up), euler, det, rescale=False)
    assert np.abs(z.double().cpu().numpy() - sym).max() <= R.gate(up, up)
    # directions= overrides the geometry
    d = det.direction_cosines()[:, [1, 0, 2]] * 3.0
    o = S.simulate_patterns(master, euler, S.DetectorGeometry((16, 12), directions=d), rescale=False)
    d32 = np.ascontiguousarray((d / np.linalg.norm(d, axis=1, keepdims=True)).T.astype(np.float32))
    refo, _ = R.simulate(up, lo, d32, euler, (16, 12), False)
    assert np.abs(o.double().cpu().numpy() - refo).max() <= R.gate(up, lo)


# ------------------------------------------------------------------------------ 8
N_DICT, DICT_BATCH = 40, 16


@functools.lru_cache(maxsize=None)
def _dictionary_inputs():
    up, lo = R.smooth_master(101)
    return S.MasterPattern(up, lo), R.spread_orientations(N_DICT, seed=11, min_deg=10.0)


def _indexer(tmp_path, name):
    m = VariationalAutoEncoderRawData()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0).items()})
    cfg = IndexerConfig(pattern_path=tmp_path / "none.npy", angles_path=tmp_path / "none.txt",
                        batch_size=DICT_BATCH, device="cuda")
    db = F.FaissLatentVectorDatabase(F.FaissLatentVectorDatabaseConfig(
        npz_path=str(tmp_path / f"{name}.npz")))
    return DiffractionPatternIndexer(m.cuda(), db=db, config=cfg)


def test_build_dictionary_from_master(tmp_path):
    master, euler = _dictionary_inputs()
    ix = _indexer(tmp_path, "a")
    appends = []
    append = ix.db._append
    ix.db._append = lambda *a, **k: (appends.append(a[0].shape[0]), append(*a, **k))[1]
    ix.build_dictionary_from_master(master, euler, batch_size=DICT_BATCH)
    assert appends == [N_DICT]                   # one add_vectors, not one per batch
    det = S.DetectorGeometry((128, 128))
    x = S.simulate_patterns(master, euler, det)
    expect = F.l2_normalize(ix.model.encode_mu(x))
    assert ix.db.get_count() == N_DICT
    assert torch.equal(ix.db._db, expect)
    assert np.array_equal(ix.db._orientations, euler)
    assert torch.equal(ix.db._ori_dev, dev(euler))
    # every simulated pattern scores highest on its own row
    res = ix.index_scan(x, batch_size=DICT_BATCH, top_n=10, min_required_matches=1)
    assert np.array_equal(res.top_index, np.arange(N_DICT))
    # the default batch size (config.batch_size) and an explicit detector give the same rows
    ix2 = _indexer(tmp_path, "b")
    ix2.build_dictionary_from_master(master, euler, detector=det)
    assert torch.equal(ix2.db._db, expect)


def test_build_dictionary_from_master_with_correction(tmp_path):
    master, euler = _dictionary_inputs()
    corr = PatternCorrection(dynamic_sigma=6.0)
    ix = _indexer(tmp_path, "c")
    ix.build_dictionary_from_master(master, euler, batch_size=DICT_BATCH, correction=corr)
    raw = S.simulate_patterns(master, euler, S.DetectorGeometry((128, 128)), rescale=False)
    x = correct_patterns(raw.view(N_DICT, 128, 128), (128, 128), corr)
    assert torch.equal(ix.db._db, F.l2_normalize(ix.model.encode_mu(x)))
    plain = S.simulate_patterns(master, euler, S.DetectorGeometry((128, 128)))
    assert not torch.equal(x, plain)
