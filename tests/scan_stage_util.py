"""What the index_scan tests of the scan-grid averaging stages share
(tests/test_gpu_neighbour_average.py, tests/test_gpu_nlpar.py): the indexer with a clustered
dictionary around a scan's latents, and the bytewise comparison of two results."""
import numpy as np
import torch

from latice.data_module import ingest_patterns_u8
from latice.index import faiss_db as F
from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig
from latice.model import VariationalAutoEncoderRawData
from latice.seeding import seeded_state_dict

FIELDS = ("orientations", "success", "scores", "top_index", "n_similar", "candidate_indices",
          "candidate_scores")


def clustered_indexer(cuda, tmp, scan, average, rng):
    """The default 128 x 128 model with seeded weights over `scan` (uint8 detector patterns) and
    a small clustered dictionary: clusters of 12 near copies, one around the latent of every
    scan pattern as ingested and one around the latent of every pattern of `average(T)`, each
    with orientations scattered by 0.3 degrees around its own centre (drawn from `rng`).
    Returns (indexer, scan)."""
    from scipy.spatial.transform import Rotation
    m = VariationalAutoEncoderRawData()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0).items()})
    m = m.to(cuda).eval()
    T = ingest_patterns_u8(scan, (128, 128))
    A = average(T)
    with torch.no_grad():
        centres = torch.cat([m.encode_mu(T), m.encode_mu(A)]).cpu().numpy()
    spread = 0.05 * np.abs(centres - centres.mean(0)).mean()
    lat, ori = [], []
    for z in centres:
        centre = Rotation.random(random_state=int(rng.integers(1 << 30)))
        for _ in range(12):
            rot = Rotation.from_rotvec(np.radians(0.3) * rng.standard_normal(3)) * centre
            ori.append(rot.as_euler("zxz", degrees=True))
            lat.append(z + spread * rng.standard_normal(z.shape))
    db = F.FaissLatentVectorDatabase(F.FaissLatentVectorDatabaseConfig(dimension=16, device="cuda:0"))
    db.add_vectors(np.array(lat, np.float32), np.array(ori))
    cfg = IndexerConfig(pattern_path=tmp / "unused.npy", angles_path=tmp / "unused.txt",
                        batch_size=16, device="cuda")
    return DiffractionPatternIndexer(m, db=db, config=cfg), scan


def same_result(a, b, what):
    for name in FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, what)
