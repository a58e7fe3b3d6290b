"""Device time of the detector resample (`resample_patterns`, csrc/resample.hip) beside a plain
device copy of the same traffic, and what binning on the device costs a whole `index_scan`.

Per 1024-batch, from device events with the stage alone on the stream (medians of 7):
`resample_patterns` of uint8 patterns at 480 x 480 -> 128 x 128 and at 256 x 256 -> 128 x 128
(divisor 255), each beside a `torch` device-to-device copy that moves the same bytes: the stage
reads the region once and writes 4 h w bytes per pattern, the copy reads and writes half that
sum.  Both are timed behind a few milliseconds of queued matrix products, so that the device,
not the host's launch path, sets the time between the events; `resample_host_paced_ms` is the
same stage without that head start.  Then `DiffractionPatternIndexer.index_scan` on a scan of 16 x 1024 uint8 patterns in pinned
memory (1,048,576 dictionary rows, top_n = 20), alternating: the 480 x 480 scan with
`resample=DetectorResample()` against a pre-binned 128 x 128 scan through the plain ingest.

Prints one JSON line.  Needs a ROCm GPU: there is no CPU path.

    python tools/resample_rate.py [--repeats 3] [--batches 16] [--batch 1024] [--rows 1048576]
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


def _events(fn, repeats=7, ahead=None):
    """Median device time (ms) of fn() on the current stream.  `ahead()` enqueues a few
    milliseconds of other work first, so the host has enqueued fn() and both events before the
    device reaches them: a stage shorter than its own launch path is then timed on the device,
    not by the host."""
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if ahead is not None:
            ahead()
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
    ap.add_argument("--side", type=int, default=480)
    ap.add_argument("--top-n", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_rate: no ROCm GPU (a time is measured on the device or not at all)")
    if a.repeats < 3:
        raise SystemExit("resample_rate: at least 3 repeats")

    from latice.data_module import DetectorResample, resample_patterns
    from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig
    from latice.index.faiss_db import FaissLatentVectorDatabase, FaissLatentVectorDatabaseConfig
    from latice.model import VariationalAutoEncoderRawData
    from latice.seeding import seeded_state_dict

    logging.getLogger("latice").setLevel(logging.ERROR)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    size = (128, 128)
    resample = DetectorResample()

    # ---- one batch, the stage alone on the stream, beside a copy of the same traffic
    B = a.batch
    x = torch.empty(B, 1, *size, dtype=torch.float32, device=dev)
    per_batch = {}
    m1 = torch.randn(4096, 4096, device=dev)
    m2 = torch.empty_like(m1)

    def ahead():
        for _ in range(4):
            torch.mm(m1, m1, out=m2)

    for side in (a.side, 256):
        staged = torch.from_numpy(rng.integers(1, 256, (B, side, side), dtype=np.uint8)).to(dev)
        src_bytes, dst_bytes = staged.numel(), x.numel() * 4
        half = (src_bytes + dst_bytes) // 2
        c_src = torch.empty(half, dtype=torch.uint8, device=dev)
        c_dst = torch.empty(half, dtype=torch.uint8, device=dev)
        stages = {"resample": lambda: resample_patterns(staged, size, resample, 255.0, dev, out=x),
                  "copy": lambda: c_dst.copy_(c_src)}
        for fn in stages.values():
            fn()
        torch.cuda.synchronize()
        t = {name: _events(fn, ahead=ahead) for name, fn in stages.items()}
        t["resample_host_paced"] = _events(stages["resample"])
        per_batch[f"{side}_to_128"] = {
            "resample_ms": round(t["resample"], 4), "copy_same_traffic_ms": round(t["copy"], 4),
            "multiple_of_copy": round(t["resample"] / t["copy"], 2),
            "resample_host_paced_ms": round(t["resample_host_paced"], 4),
            "bytes_read": src_bytes, "bytes_written": dst_bytes,
            "resample_GBps": round((src_bytes + dst_bytes) / t["resample"] / 1e6, 1),
            "copy_GBps": round(2 * half / t["copy"] / 1e6, 1)}
        del staged, c_src, c_dst

    # ---- the whole scan: binned on the device against pre-binned on the host
    n = a.batches * a.batch
    scan_t = torch.empty(n, a.side, a.side, dtype=torch.uint8).pin_memory()
    scan = scan_t.numpy()
    scan[:B] = rng.integers(1, 256, (B, a.side, a.side), dtype=np.uint8)
    for s in range(B, n, B):                         # the rate does not depend on the values
        scan[s:s + B] = scan[:min(B, n - s)]
    small_t = torch.empty(n, *size, dtype=torch.uint8).pin_memory()
    small = small_t.numpy()
    small[:] = rng.integers(1, 256, small.shape, dtype=np.uint8)

    model = VariationalAutoEncoderRawData()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0).items()})
    db = FaissLatentVectorDatabase(FaissLatentVectorDatabaseConfig(
        npz_path="/nonexistent/resample_rate.npz", dimension=16, device="cuda:0"))
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

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def run_binned():
        return ix.index_scan(small, batch_size=a.batch, **kw)

    def run_resampled():
        return ix.index_scan(scan, batch_size=a.batch, resample=resample, **kw)

    warm = min(n, 2 * a.batch)
    ix.index_scan(small[:warm], batch_size=a.batch, **kw)
    ix.index_scan(scan[:warm], batch_size=a.batch, resample=resample, **kw)
    t_binned, t_res = [], []
    for _ in range(a.repeats):                      # alternate: the host is shared
        t_binned.append(timed(run_binned)[0])
        t_res.append(timed(run_resampled)[0])

    # the two host-side stages of a staged batch, alone: scan -> pinned buffer, pinned -> device
    pinned = torch.empty(B, a.side, a.side, dtype=torch.uint8).pin_memory()
    on_dev = torch.empty(B, a.side, a.side, dtype=torch.uint8, device=dev)
    pinned_np = pinned.numpy()
    t_host = []
    for i in range(7):
        t0 = time.perf_counter()
        np.copyto(pinned_np, scan[(i % a.batches) * B:(i % a.batches + 1) * B])
        t_host.append((time.perf_counter() - t0) * 1e3)
    on_dev.copy_(pinned, non_blocking=True)
    torch.cuda.synchronize()
    t_upload = _events(lambda: on_dev.copy_(pinned, non_blocking=True))
    del m1, m2

    def rate(ts):
        return {"min_s": round(min(ts), 4), "median_s": round(statistics.median(ts), 4),
                "patterns_per_s_best": round(n / min(ts), 1),
                "patterns_per_s_median": round(n / statistics.median(ts), 1)}

    print(json.dumps({
        "tool": "resample_rate", "patterns": n, "batch": a.batch, "side": a.side,
        "dictionary_rows": a.rows, "top_n": a.top_n, "repeats": a.repeats,
        "per_batch": per_batch,
        "staging_per_batch": {"host_copy_to_pinned_ms": round(statistics.median(t_host), 4),
                              "upload_ms": round(t_upload, 4), "bytes": B * a.side * a.side},
        "index_scan_prebinned_128": rate(t_binned), "index_scan_resampled": rate(t_res),
        "scan_rate_ratio": round(statistics.median(t_binned) / statistics.median(t_res), 3),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
