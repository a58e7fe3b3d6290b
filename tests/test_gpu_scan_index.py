"""Whole-scan indexing on the device: the fused search + consensus entry point
(csrc/scan_index.hip), the uint8 ingest (csrc/ingest.hip), `FaissLatentVectorDatabase
.index_latents` and `DiffractionPatternIndexer.index_scan`.

The contract of the fused kernel is bitwise: every output equals ebsdvae_cosine_topk followed
by ebsdvae_orient_consensus on the same inputs, a query's outputs do not depend on the other
queries of the launch, and index_scan reports what the per-pattern API reports for the same
batches."""
import functools

import numpy as np
import pytest
import torch

from latice import _native as N
from latice.data_module import ingest_patterns, ingest_patterns_u8
from latice.index import faiss_db as F
from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig, ScanIndexResult
from latice.model import VariationalAutoEncoderRawData
from latice.seeding import seeded_state_dict
from oracle import index_oracle as IO

pytestmark = pytest.mark.gpu

CASES = [(960, 16, 70, 20),      # more than one 16-query group, plus a tail
         (100003, 16, 37, 20),   # many chunks, ragged last chunk
         (130, 64, 3, 17),
         (64, 16, 5, 64),        # k = N = 64
         (4096, 32, 1, 1)]
PARAMS = [(1.0, 18, 3), (2.0, 12, 3), (5.0, 1, 1), (0.5, 21, 3)]   # the last never succeeds at k = 20
DUP_OF = 5                       # the last dictionary row is a bit-identical copy of this row


def _cluster_db(rng, n_clusters=40, per=24, noise_deg=0.3, dim=16):
    """Latents clustered per orientation; orientations noisy around cluster centres, some
    copies hidden behind random cubic symmetry operators (as in test_gpu_search.py)."""
    from scipy.spatial.transform import Rotation as R
    sym = R.from_quat(IO.CUBIC_SYMMETRY)
    lat, ori = [], []
    for c in range(n_clusters):
        centre = R.random(random_state=int(rng.integers(1 << 30)))
        z = rng.standard_normal(dim)
        for j in range(per):
            rot = R.from_rotvec(np.radians(noise_deg) * rng.standard_normal(3)) * centre
            if j % 7 == 3:
                rot = sym[int(rng.integers(24))] * rot
            ori.append(rot.as_euler("zxz", degrees=True))
            lat.append(z + 0.05 * rng.standard_normal(dim))
    return np.array(lat, np.float32), np.array(ori)


@functools.lru_cache(maxsize=None)
def _case(n, d, Q, k):
    """Normalised dictionary (clusters, then unrelated rows up to n, the last row a duplicate),
    its orientations and Q normalised queries near cluster members, on the device."""
    rng = np.random.default_rng(n + d + Q + k)
    ncl = min(40, n // 24)
    lat, ori = _cluster_db(rng, n_clusters=ncl, dim=d)
    rest = n - len(lat)
    lat = np.concatenate([lat, rng.standard_normal((rest, d)).astype(np.float32)])
    ori = np.concatenate([ori, rng.uniform(-180, 180, (rest, 3)) * [1, 0.5, 1] + [0, 90, 0]])
    lat[n - 1] = lat[DUP_OF]
    pick = (np.arange(Q) * 9) % (ncl * 24)
    q = lat[pick] + 0.02 * rng.standard_normal((Q, d)).astype(np.float32)
    q[0] = lat[DUP_OF]           # query 0 scores rows DUP_OF and n - 1 identically, above all others
    dbn = F.l2_normalize(torch.from_numpy(lat).cuda())
    qn = F.l2_normalize(torch.from_numpy(q).cuda())
    return dbn, torch.from_numpy(ori).cuda(), qn, ori


def _two_launch(dbn, ori, qn, k, thr, minm, maxit):
    scores, idx = F.cosine_topk(dbn, qn, k)
    Q = qn.shape[0]
    best = torch.empty(Q, 3, dtype=torch.float64, device=qn.device)
    mean = torch.empty(Q, 3, dtype=torch.float64, device=qn.device)
    ok = torch.empty(Q, dtype=torch.int32, device=qn.device)
    mask = torch.empty(Q, dtype=torch.int64, device=qn.device)
    N.call("ebsdvae_orient_consensus", ori.data_ptr(), idx.data_ptr(), Q, k, float(thr), minm, maxit,
           best.data_ptr(), mean.data_ptr(), ok.data_ptr(), mask.data_ptr(), N.stream(qn.device))
    pop = np.array([bin(int(m)).count("1") for m in mask.cpu().numpy().view(np.uint64)], np.int32)
    return dict(best=best.cpu().numpy(), success=ok.cpu().numpy(), n_similar=pop,
                score=scores[:, 0].cpu().numpy(), row=idx[:, 0].cpu().numpy(),
                cand_scores=scores.cpu().numpy(), cand_idx=idx.cpu().numpy())


def _fused(dbn, ori, qn, k, thr, minm, maxit, candidates=True):
    n, d = dbn.shape
    Q, dev = qn.shape[0], qn.device
    # poisoned outputs: a field the kernel skips cannot pass by luck
    best = torch.full((Q, 3), -7.0, dtype=torch.float64, device=dev)
    ok = torch.full((Q,), -7, dtype=torch.int32, device=dev)
    score = torch.full((Q,), -7.0, dtype=torch.float32, device=dev)
    row = torch.full((Q,), -7, dtype=torch.int64, device=dev)
    nsim = torch.full((Q,), -7, dtype=torch.int32, device=dev)
    cs = torch.full((Q, k), -7.0, dtype=torch.float32, device=dev) if candidates else None
    ci = torch.full((Q, k), -7, dtype=torch.int64, device=dev) if candidates else None
    nbytes = N.call("ebsdvae_index_latents_work", n, Q, d, k)
    assert nbytes == N.call("ebsdvae_cosine_topk_work", n, Q, d, k)
    work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    N.call("ebsdvae_index_latents", dbn.data_ptr(), n, ori.data_ptr(), qn.data_ptr(), Q, d, k,
           float(thr), minm, maxit, best.data_ptr(), ok.data_ptr(), score.data_ptr(),
           row.data_ptr(), nsim.data_ptr(), cs.data_ptr() if candidates else None,
           ci.data_ptr() if candidates else None, work.data_ptr(), N.stream(dev))
    out = dict(best=best.cpu().numpy(), success=ok.cpu().numpy(), n_similar=nsim.cpu().numpy(),
               score=score.cpu().numpy(), row=row.cpu().numpy())
    if candidates:
        out.update(cand_scores=cs.cpu().numpy(), cand_idx=ci.cpu().numpy())
    return out


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n,d,Q,k", CASES)
def test_fused_equals_two_launches_bitwise(cuda, n, d, Q, k):
    dbn, ori, qn, _ = _case(n, d, Q, k)
    n_ok = n_fail = 0
    for thr, minm, maxit in PARAMS:
        ref = _two_launch(dbn, ori, qn, k, thr, minm, maxit)
        got = _fused(dbn, ori, qn, k, thr, minm, maxit, candidates=True)
        lean = _fused(dbn, ori, qn, k, thr, minm, maxit, candidates=False)
        for name, want in ref.items():
            assert _same_bits(got[name], want), (name, thr, minm, maxit)
            if name in lean:
                assert _same_bits(lean[name], want), (name, "null candidate pointers")
        assert set(np.unique(ref["success"])) <= {0, 1}
        n_ok += int(ref["success"].sum())
        n_fail += int((ref["success"] == 0).sum())
        if minm > k:
            assert not ref["success"].any()
    # (5.0, 1, 1) always succeeds (the reference matches itself); minm > k never does
    assert n_ok > 0 and (n_fail > 0 or k >= 21)
    # ties break to the lower row: query 0 scores rows DUP_OF and n - 1 identically
    assert ref["row"][0] == DUP_OF
    if k >= 2:
        assert list(ref["cand_idx"][0, :2]) == [DUP_OF, n - 1]
        assert ref["cand_scores"][0, 0] == ref["cand_scores"][0, 1]


def test_result_does_not_depend_on_the_launch(cuda):
    n, d, Q, k = CASES[0]
    dbn, ori, qn, _ = _case(n, d, Q, k)
    for thr, minm, maxit in PARAMS[:2]:
        batch = _fused(dbn, ori, qn, k, thr, minm, maxit)
        for j in (0, 17, 69):
            alone = _fused(dbn, ori, qn[j:j + 1].contiguous(), k, thr, minm, maxit)
            for name, v in alone.items():
                assert _same_bits(v, batch[name][j:j + 1]), (name, j)


def test_fused_consensus_matches_oracle(cuda):
    n, d, Q, k = CASES[0]
    dbn, ori, qn, ori_np = _case(n, d, Q, k)
    thr, minm, maxit = PARAMS[1]
    got = _fused(dbn, ori, qn, k, thr, minm, maxit)
    assert got["success"].sum() > 0
    for j in range(Q):
        best, _, ok, sim = IO.find_best_orientation(ori_np[got["cand_idx"][j]], thr, minm, maxit)
        assert bool(got["success"][j]) == ok
        assert got["n_similar"][j] == len(sim)
        if ok:   # same rotation; Euler angles compared modulo 360 (wrap at +-180)
            diff = (got["best"][j] - best + 180.0) % 360.0 - 180.0
            assert np.abs(diff).max() < 1e-6, (got["best"][j], best)
        else:
            assert np.array_equal(got["best"][j], best)


@pytest.mark.parametrize("B,H0,W0", [(5, 140, 133),    # crop, odd margins
                                     (3, 100, 100)])   # zero pad
def test_uint8_ingest_is_the_float_ingest_of_v_over_255(cuda, B, H0, W0):
    rng = np.random.default_rng(B + H0)
    raw = rng.integers(0, 256, (B, H0, W0), dtype=np.uint8)
    raw[0, :16, :16] = np.arange(256, dtype=np.uint8).reshape(16, 16)   # every value
    raw[-1, H0 // 2, W0 // 2] = 0
    raw[-1, H0 // 2, W0 // 2 + 1] = 255
    got = ingest_patterns_u8(raw, (128, 128)).cpu().numpy()
    assert got.shape == (B, 1, 128, 128) and got.dtype == np.float32
    assert _same_bits(got, IO.ingest_patterns(raw / 255.0).astype(np.float32).reshape(got.shape))
    assert _same_bits(got, ingest_patterns(raw.astype(np.float64) / 255.0, (128, 128)).cpu().numpy())
    out = torch.empty(B, 1, 128, 128, device=cuda)
    assert ingest_patterns_u8(torch.from_numpy(raw).cuda(), (128, 128), out=out) is out
    assert _same_bits(out.cpu().numpy(), got)
    with pytest.raises(TypeError, match="uint8"):
        ingest_patterns_u8(raw.astype(np.float32))


# ---------------------------------------------------------------- index_scan
N_SCAN, SIDE, BATCH = 48, 140, 16


def _model(cuda):
    m = VariationalAutoEncoderRawData()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0).items()})
    return m.to(cuda)


@pytest.fixture(scope="module")
def scan(cuda, tmp_path_factory):
    """48 patterns = 4 random base patterns x 12 near copies; angles scatter by 0.3 degrees
    around 4 centres, one copy per group moved by a cubic symmetry operator.  The dictionary
    is built from the same patterns with build_dictionary."""
    from scipy.spatial.transform import Rotation as R
    tmp = tmp_path_factory.mktemp("scan")
    rng = np.random.default_rng(21)
    sym = R.from_quat(IO.CUBIC_SYMMETRY)
    raw, ang = [], []
    for c in range(4):
        base = rng.random((SIDE, SIDE))
        centre = R.random(random_state=int(rng.integers(1 << 30)))
        for j in range(12):
            raw.append(np.clip(base + 1e-3 * rng.standard_normal((SIDE, SIDE)), 0.0, 1.0))
            rot = R.from_rotvec(np.radians(0.3) * rng.standard_normal(3)) * centre
            if j == 5:
                rot = sym[7 + c] * rot
            ang.append(rot.as_euler("zxz", degrees=True))
    raw, ang = np.array(raw), np.array(ang)
    np.save(tmp / "patterns.npy", raw)
    with open(tmp / "angles.txt", "w") as f:
        f.write(f"eu\n{N_SCAN}\n")
        for a in ang:
            f.write(" ".join(repr(float(v)) for v in a) + "\n")
    m = _model(cuda)
    cfg = IndexerConfig(pattern_path=tmp / "patterns.npy", angles_path=tmp / "angles.txt",
                        batch_size=BATCH, device="cuda")
    ix = DiffractionPatternIndexer(m, config=cfg)
    ix.build_dictionary()
    assert ix.db.get_count() == N_SCAN
    raw_u8 = np.round(raw[:37] * 255).astype(np.uint8)
    np.save(tmp / "scan_u8.npy", raw_u8)
    return dict(ix=ix, m=m, raw=raw, raw_u8=raw_u8, u8_path=tmp / "scan_u8.npy")


def _per_pattern(scan, **kw):
    ix, m, raw = scan["ix"], scan["m"], scan["raw"]
    res = []
    for s in range(0, N_SCAN, BATCH):
        x = ingest_patterns(raw[s:s + BATCH], (128, 128))
        res += ix.db.find_best_orientations_batch(m.encode_mu(x), **kw)
    return res


def test_index_scan_equals_the_per_pattern_api(scan):
    ix, raw = scan["ix"], scan["raw"]
    kw = dict(top_n=10, orientation_threshold=2.0, min_required_matches=8)
    got = ix.index_scan(raw, batch_size=BATCH, return_candidates=True, **kw)
    assert isinstance(got, ScanIndexResult) and len(got) == N_SCAN
    assert got.orientations.shape == (N_SCAN, 3) and got.orientations.dtype == np.float64
    assert got.success.dtype == bool and got.scores.dtype == np.float32
    assert got.top_index.dtype == np.int64 and got.n_similar.dtype == np.int32
    assert got.candidate_indices.shape == (N_SCAN, 10) and got.candidate_scores.shape == (N_SCAN, 10)
    ref = _per_pattern(scan, **kw)
    for j, r in enumerate(ref):
        assert _same_bits(got.orientations[j], np.asarray(r.best_orientation)), j
        assert got.success[j] == r.success
        assert got.scores[j] == r.distances[0]
        assert _same_bits(got.candidate_scores[j], r.distances)
        assert got.top_index[j] == got.candidate_indices[j, 0]
        assert np.array_equal(ix.db.orientations[got.candidate_indices[j]], r.candidate_orientations)
        assert got.n_similar[j] == len(r.similar_indices)
    assert got.success.any()
    # without candidates: the same compact result, no lists
    lean = ix.index_scan(raw, batch_size=BATCH, **kw)
    assert lean.candidate_indices is None and lean.candidate_scores is None
    for name in ("orientations", "success", "scores", "top_index", "n_similar"):
        assert _same_bits(getattr(lean, name), getattr(got, name)), name
    # more matches required than candidates: every pattern reports its closest match
    none = ix.index_scan(raw, batch_size=BATCH, top_n=10, orientation_threshold=2.0,
                         min_required_matches=11)
    assert not none.success.any()
    assert _same_bits(none.orientations, ix.db.orientations[none.top_index])


def _same_result(a, b):
    for name in ("orientations", "success", "scores", "top_index", "n_similar",
                 "candidate_indices", "candidate_scores"):
        assert _same_bits(getattr(a, name), getattr(b, name)), name


def test_streaming_and_input_forms(scan, monkeypatch):
    ix, m, raw_u8 = scan["ix"], scan["m"], scan["raw_u8"]
    kw = dict(top_n=10, orientation_threshold=2.0, min_required_matches=8, batch_size=BATCH,
              return_candidates=True)
    passes = []
    encode_mu = m.encode_mu
    monkeypatch.setattr(m, "encode_mu", lambda x: (passes.append(x.shape[0]), encode_mu(x))[1])
    by_path = ix.index_scan(scan["u8_path"], **kw)
    assert passes == [16, 16, 5]                     # 3 encoder passes, a tail of 5
    assert len(by_path) == 37
    _same_result(by_path, ix.index_scan(str(scan["u8_path"]), **kw))   # staging buffers reused again
    _same_result(by_path, ix.index_scan(raw_u8, **kw))
    _same_result(by_path, ix.index_scan(ingest_patterns_u8(raw_u8, (128, 128)), **kw))
    # the uint8 scan is the float scan of v / 255
    _same_result(by_path, ix.index_scan(raw_u8 / 255.0, **kw))
    # a float32 scan goes through the float ingest
    f32 = (raw_u8 / 255.0).astype(np.float32)
    _same_result(ix.index_scan(f32, **kw), ix.index_scan(ingest_patterns(f32, (128, 128)), **kw))
    assert passes == [16, 16, 5] * 7


def test_errors_and_edges(scan, cuda):
    ix, m, raw = scan["ix"], scan["m"], scan["raw"]

    class NoScanDb:
        def add_vectors(self, *a):
            pass

        def find_best_orientation(self, *a, **k):
            raise AssertionError("index_scan must not fall back to the per-pattern API")

        find_best_orientations_batch = find_best_orientation

    mock = DiffractionPatternIndexer(m, db=NoScanDb(), config=ix.config)
    with pytest.raises(TypeError, match="index_latents"):
        mock.index_scan(raw[:4])
    with pytest.raises(ValueError, match="top_n=65"):
        ix.index_scan(raw[:4], top_n=65)
    with pytest.raises(ValueError, match="top_n=65"):
        ix.db.index_latents(torch.zeros(2, 16, device=cuda), top_n=65)
    with pytest.raises(ValueError):
        ix.index_scan(raw[0])                        # one 2-D pattern is not a scan
    empty_db = F.FaissLatentVectorDatabase(F.FaissLatentVectorDatabaseConfig(npz_path="/nonexistent/z.npz"))
    empty = DiffractionPatternIndexer(m, db=empty_db, config=ix.config)
    for cands in (False, True):
        r = empty.index_scan(raw[:20], batch_size=BATCH, return_candidates=cands)
        assert len(r) == 20 and not r.success.any()
        assert np.isnan(r.orientations).all() and (r.top_index == -1).all()
        assert (r.n_similar == 0).all()
        assert (r.candidate_indices.shape == (20, 0)) if cands else r.candidate_indices is None
    none = ix.index_scan(raw[:0], batch_size=BATCH)
    assert len(none) == 0 and none.orientations.shape == (0, 3)
