"""Device time of the neighbour pattern averaging (`ebsdvae_average_neighbours`,
csrc/neighbour.hip) and what it costs a whole `index_scan`.

Per 1024-batch, from device events with the stage alone on the stream (medians of 7): 1024
consecutive outputs of a 128 x 128 scan of 128 x 128 patterns, averaged out of a ring of
1024 + 2 (hr cols + hc) transformed patterns into the encoder's batch buffer, for the 3 x 3
circular and the 5 x 5 gaussian window; beside them the byte floor (every output read once and
written once, 2 x 1024 x 64 KiB, at --copy-tbs, the streaming-copy rate of DESIGN.md section 7)
and a device-to-device copy of the batch.  Then `DiffractionPatternIndexer.index_scan` on the
scan of tools/scan_index_rate.py (16 x 1024 uint8 patterns at 140 x 140 in pinned memory, here a
128 x 128 grid, 1,048,576 dictionary rows, top_n = 20) without averaging and with each window,
alternating the three.

EBSDVAE_NEIGHBOUR_RUN=<n> (read once per process by the library) sets the outputs a thread walks
along a scan row; 1 is the plain tap loop.  --stage-only skips the scans (for that A/B).

Prints one JSON line.  Needs a ROCm GPU: there is no CPU path.

    python tools/neighbour_average_rate.py [--repeats 3] [--batches 16] [--batch 1024] [--stage-only]
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
    ap.add_argument("--cols", type=int, default=128, help="scan columns (patterns / cols rows)")
    ap.add_argument("--rows", type=int, default=1 << 20, help="dictionary rows")
    ap.add_argument("--side", type=int, default=140)
    ap.add_argument("--top-n", type=int, default=20)
    ap.add_argument("--copy-tbs", type=float, default=6.3)
    ap.add_argument("--stage-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neighbour_average_rate: no ROCm GPU (a time is measured on the device or not at all)")
    if a.repeats < 3:
        raise SystemExit("neighbour_average_rate: at least 3 repeats")
    n = a.batches * a.batch
    if n % a.cols:
        raise SystemExit(f"neighbour_average_rate: {n} patterns do not fill rows of {a.cols}")

    from latice.data_module import NeighbourAverage, average_neighbour_range

    logging.getLogger("latice").setLevel(logging.ERROR)
    dev = torch.device("cuda:0")
    grid = (n // a.cols, a.cols)
    windows = {"circular_3x3": NeighbourAverage(grid, "circular", (3, 3)),
               "gaussian_5x5": NeighbourAverage(grid, "gaussian", (5, 5), std=1.0)}

    # ---- one batch, the stage alone on the stream
    B = min(a.batch, n)
    p0 = (n // 2) // a.cols * a.cols if n > B else 0       # rows in the middle of the scan
    x = torch.empty(B, 1, 128, 128, dtype=torch.float32, device=dev)
    per_batch = {}
    for name, na in windows.items():
        cap = min(n, B + 2 * na.reach)
        ring = torch.rand(cap, 1, 128, 128, dtype=torch.float32, device=dev)
        fn = lambda: average_neighbour_range(ring, na, p0, B, x)   # noqa: E731
        fn()
        torch.cuda.synchronize()
        per_batch[f"average_{name}_ms"] = round(_events(fn), 4)
        del ring
    src = torch.rand(B, 1, 128, 128, dtype=torch.float32, device=dev)
    x.copy_(src)
    torch.cuda.synchronize()
    per_batch["device_copy_ms"] = round(_events(lambda: x.copy_(src)), 4)
    moved = 2 * B * 128 * 128 * 4
    per_batch["floor_bytes"] = moved
    per_batch["floor_ms"] = round(moved / (a.copy_tbs * 1e12) * 1e3, 4)
    del src

    out = {"tool": "neighbour_average_rate", "patterns": n, "scan_shape": list(grid),
           "batch": a.batch, "side": a.side, "copy_tbs": a.copy_tbs,
           "run": os.environ.get("EBSDVAE_NEIGHBOUR_RUN", "default"), "per_batch": per_batch}

    # ---- the whole scan, without and with the averaging
    if not a.stage_only:
        from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig
        from latice.index.faiss_db import FaissLatentVectorDatabase, FaissLatentVectorDatabaseConfig
        from latice.model import VariationalAutoEncoderRawData
        from latice.seeding import seeded_state_dict

        rng = np.random.default_rng(0)
        scan_t = torch.empty(n, a.side, a.side, dtype=torch.uint8).pin_memory()
        scan = scan_t.numpy()
        scan[:] = rng.integers(0, 256, scan.shape, dtype=np.uint8)
        model = VariationalAutoEncoderRawData()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0).items()})
        db = FaissLatentVectorDatabase(FaissLatentVectorDatabaseConfig(
            npz_path="/nonexistent/neighbour_average_rate.npz", dimension=16, device="cuda:0"))
        db.reserve(a.rows)
        step = 1 << 18
        for s in range(0, a.rows, step):
            m = min(step, a.rows - s)
            db.add_vectors(rng.standard_normal((m, 16)).astype(np.float32),
                           rng.uniform(0, 360, (m, 3)) * [1, 0.5, 1])
        cfg = IndexerConfig(pattern_path="unused.npy", angles_path="unused.txt",
                            batch_size=a.batch, device="cuda", top_n=a.top_n)
        ix = DiffractionPatternIndexer(model, db=db, config=cfg)
        kw = dict(top_n=a.top_n, orientation_threshold=1.0, min_required_matches=18)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res

        runs = {"index_scan": lambda: ix.index_scan(scan, batch_size=a.batch, **kw)}
        for name, na in windows.items():
            runs[f"index_scan_{name}"] = (
                lambda na=na: ix.index_scan(scan, batch_size=a.batch, neighbour_average=na, **kw))
        for fn in runs.values():                         # warm-up: every shape of the timed window
            fn()
        times = {name: [] for name in runs}
        for _ in range(a.repeats):                       # alternate: the host is shared
            for name, fn in runs.items():
                times[name].append(timed(fn)[0])

        def rate(ts):
            return {"min_s": round(min(ts), 4), "median_s": round(statistics.median(ts), 4),
                    "patterns_per_s_best": round(n / min(ts), 1),
                    "patterns_per_s_median": round(n / statistics.median(ts), 1)}

        out.update(dictionary_rows=a.rows, top_n=a.top_n, repeats=a.repeats,
                   **{name: rate(ts) for name, ts in times.items()})
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
