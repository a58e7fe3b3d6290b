"""Device time of the background-corrected ingest (`correct_patterns`, csrc/correct.hip) beside
the plain uint8 ingest it replaces, and what a correction costs a whole `index_scan`.

Per 1024-batch, from device events with the stage alone on the stream (medians of 7):
`ingest_patterns_u8` at 140 x 140 -> 128 x 128; `correct_patterns` there with sigma = 16,
dynamic subtract only and static divide + dynamic divide (the fused path); `correct_patterns`
at 256 x 256 -> 256 x 256 (the phased path); the scan-mean accumulation.  Then
`DiffractionPatternIndexer.index_scan` on the scan of tools/scan_index_rate.py (16 x 1024 uint8
patterns at 140 x 140 in pinned memory, 1,048,576 dictionary rows, top_n = 20) without and with
the static divide + dynamic divide correction, alternating the two.

Prints one JSON line.  Needs a ROCm GPU: there is no CPU path.

    python tools/ingest_correct_rate.py [--repeats 3] [--batches 16] [--batch 1024] [--rows 1048576]
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ebsd-vae_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _events(fn, repeats=7):
    """Median device time (ms) of fn() on the current stream."""
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--side", type=int, default=140)
    ap.add_argument("--sigma", type=float, default=16.0)
    ap.add_argument("--top-n", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_correct_rate: no ROCm GPU (a time is measured on the device or not at all)")
    if a.repeats < 3:
        raise SystemExit("ingest_correct_rate: at least 3 repeats")

    from latice.data_module import (PatternCorrection, accumulate_patterns, correct_patterns,
                                    ingest_patterns_u8)
    from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig
    from latice.index.faiss_db import FaissLatentVectorDatabase, FaissLatentVectorDatabaseConfig
    from latice.model import VariationalAutoEncoderRawData
    from latice.seeding import seeded_state_dict

    logging.getLogger("latice").setLevel(logging.ERROR)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    n = a.batches * a.batch
    scan_t = torch.empty(n, a.side, a.side, dtype=torch.uint8).pin_memory()
    scan = scan_t.numpy()
    scan[:] = rng.integers(1, 256, scan.shape, dtype=np.uint8)

    model = VariationalAutoEncoderRawData()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0).items()})
    db = FaissLatentVectorDatabase(FaissLatentVectorDatabaseConfig(
        npz_path="/nonexistent/ingest_correct_rate.npz", dimension=16, device="cuda:0"))
    db.reserve(a.rows)
    step = 1 << 18
    for s in range(0, a.rows, step):
        m = min(step, a.rows - s)
        db.add_vectors(rng.standard_normal((m, 16)).astype(np.float32),
                       rng.uniform(0, 360, (m, 3)) * [1, 0.5, 1])
    cfg = IndexerConfig(pattern_path="unused.npy", angles_path="unused.txt", batch_size=a.batch,
                        device="cuda", top_n=a.top_n)
    ix = DiffractionPatternIndexer(model, db=db, config=cfg)
    kw = dict(top_n=a.top_n, orientation_threshold=1.0, min_required_matches=18)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    background = ix.scan_background(scan, batch_size=a.batch)
    t_background = time.perf_counter() - t0
    dynamic = PatternCorrection(dynamic_sigma=a.sigma, dynamic_mode="subtract")
    both = PatternCorrection(static_background=background, static_mode="divide",
                             dynamic_sigma=a.sigma, dynamic_mode="divide")

    # ---- one batch, each stage alone on the stream
    B = min(a.batch, n)
    staged = torch.from_numpy(scan[:B]).to(dev)
    x = torch.empty(B, 1, 128, 128, dtype=torch.float32, device=dev)
    big = torch.from_numpy(rng.integers(1, 256, (B, 256, 256), dtype=np.uint8)).to(dev)
    xbig = torch.empty(B, 1, 256, 256, dtype=torch.float32, device=dev)
    acc = torch.zeros(a.side, a.side, dtype=torch.float64, device=dev)
    stages = {
        "ingest_u8_ms": lambda: ingest_patterns_u8(staged, (128, 128), dev, out=x),
        "correct_dynamic_ms": lambda: correct_patterns(staged, (128, 128), dynamic, dev, out=x),
        "correct_static_dynamic_ms": lambda: correct_patterns(staged, (128, 128), both, dev, out=x),
        "correct_rescale_only_ms": lambda: correct_patterns(staged, (128, 128), PatternCorrection(),
                                                            dev, out=x),
        "correct_256_phased_dynamic_ms": lambda: correct_patterns(big, (256, 256), dynamic, dev,
                                                                  out=xbig),
        "accumulate_ms": lambda: accumulate_patterns(staged, acc),
    }
    for fn in stages.values():
        fn()
    torch.cuda.synchronize()
    per_batch = {name: round(_events(fn), 4) for name, fn in stages.items()}
    del big, xbig

    # ---- the whole scan, without and with the correction
    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def run_plain():
        return ix.index_scan(scan, batch_size=a.batch, **kw)

    def run_corrected():
        return ix.index_scan(scan, batch_size=a.batch, correction=both, **kw)

    warm = min(n, 2 * a.batch)
    ix.index_scan(scan[:warm], batch_size=a.batch, **kw)
    ix.index_scan(scan[:warm], batch_size=a.batch, correction=both, **kw)
    t_plain, t_corr = [], []
    for _ in range(a.repeats):                      # alternate: the host is shared
        t_plain.append(timed(run_plain)[0])
        t_corr.append(timed(run_corrected)[0])

    def rate(ts):
        return {"min_s": round(min(ts), 4), "median_s": round(statistics.median(ts), 4),
                "patterns_per_s_best": round(n / min(ts), 1),
                "patterns_per_s_median": round(n / statistics.median(ts), 1)}

    print(json.dumps({
        "tool": "ingest_correct_rate", "patterns": n, "batch": a.batch, "side": a.side,
        "sigma": a.sigma, "dictionary_rows": a.rows, "top_n": a.top_n, "repeats": a.repeats,
        "per_batch": per_batch, "scan_background_s": round(t_background, 4),
        "index_scan": rate(t_plain), "index_scan_corrected": rate(t_corr),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
