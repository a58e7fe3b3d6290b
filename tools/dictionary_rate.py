"""Patterns per second of building a dictionary from a master pattern on the device:
`DiffractionPatternIndexer.build_dictionary_from_master` against the existing `build_dictionary`
on a .npy file of the same patterns (the only way to build this dictionary without the
simulation), and the two stages of a batch alone from device events.

Fixed inputs (the defaults): a synthetic non-centrosymmetric master of M = 1001 (two hemispheres,
8 MB), the default 128 x 128 detector geometry, 16 x 1024 seeded random orientations, batches of
1024, the seeded model at 128 x 128.  Reported:

    simulate_ms             one `simulate_patterns` launch of 1024 patterns (median of the repeats)
    encoder_ms              `encode_mu` alone on the same buffer
    from_master             build_dictionary_from_master end to end, patterns per second
    from_npy                build_dictionary on the .npy file of the same patterns
    simulate_bound          what the launch must move at the least: 4 h w B bytes written, 4
                            gathered texels per pixel, and the rates the measured time makes of them

Prints one JSON line.  Needs a ROCm GPU: there is no CPU path.

    python tools/dictionary_rate.py [--repeats 3] [--batches 16] [--batch 1024] [--master 1001]
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ebsd-vae_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _events(fn, repeats):
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


def synthetic_master(M: int):
    """Two smooth (M, M) hemispheres that differ: crossed sinusoid bands in the Lambert plane."""
    t = np.linspace(-1.0, 1.0, M)
    Y, X = np.meshgrid(t, t, indexing="ij")
    up = np.sin(9.0 * X + 4.0 * Y) * np.cos(7.0 * Y - 2.0 * X) + 0.3 * X
    lo = np.cos(8.0 * X - 5.0 * Y) * np.sin(6.0 * Y + 3.0 * X) - 0.3 * Y
    return up.astype(np.float32), lo.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--master", type=int, default=1001)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dictionary_rate: no ROCm GPU (a rate is measured on the device or not at all)")
    if a.repeats < 3:
        raise SystemExit("dictionary_rate: at least 3 repeats")

    from latice.data_module import DetectorGeometry, MasterPattern, simulate_patterns
    from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig
    from latice.index.faiss_db import FaissLatentVectorDatabase, FaissLatentVectorDatabaseConfig
    from latice.model import VariationalAutoEncoderRawData
    from latice.seeding import seeded_state_dict

    logging.getLogger("latice").setLevel(logging.ERROR)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    n, h, w = a.batches * a.batch, 128, 128
    euler = np.stack([rng.uniform(0, 360, n), np.degrees(np.arccos(rng.uniform(-1, 1, n))),
                      rng.uniform(0, 360, n)], axis=1)
    master = MasterPattern(*synthetic_master(a.master))
    det = DetectorGeometry((h, w))

    model = VariationalAutoEncoderRawData()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0).items()})

    with tempfile.TemporaryDirectory() as tmp:
        def indexer():
            db = FaissLatentVectorDatabase(FaissLatentVectorDatabaseConfig(
                npz_path=os.path.join(tmp, "absent.npz"), dimension=16, device="cuda:0"))
            db.reserve(n)
            cfg = IndexerConfig(pattern_path=os.path.join(tmp, "patterns.npy"),
                                angles_path=os.path.join(tmp, "angles.txt"), batch_size=a.batch,
                                device="cuda")
            return DiffractionPatternIndexer(model, db=db, config=cfg)

        # the two stages of one batch, each alone on the stream
        B = min(a.batch, n)
        eu_d = torch.from_numpy(euler[:B]).to(dev)
        x = torch.empty(B, 1, h, w, dtype=torch.float32, device=dev)
        indexer()                                   # moves the model to the device
        stages = {"simulate_ms": lambda: simulate_patterns(master, eu_d, det, out=x),
                  "encoder_ms": lambda: model.encode_mu(x)}
        for fn in stages.values():
            fn()
        torch.cuda.synchronize()
        serial = {name: round(_events(fn, max(7, a.repeats)), 4) for name, fn in stages.items()}

        # the pattern file the existing path needs: the same patterns, simulated once
        pat = np.lib.format.open_memmap(os.path.join(tmp, "patterns.npy"), mode="w+",
                                        dtype=np.float32, shape=(n, h, w))
        for s in range(0, n, a.batch):
            e = min(s + a.batch, n)
            pat[s:e] = simulate_patterns(master, euler[s:e], det).view(e - s, h, w).cpu().numpy()
        pat.flush()
        del pat
        with open(os.path.join(tmp, "angles.txt"), "w") as f:
            f.write(f"eu\n{n}\n")
            for row in euler:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def from_master():
            ix = indexer()
            ix.build_dictionary_from_master(master, euler, det, batch_size=a.batch)
            assert ix.db.get_count() == n

        def from_npy():
            ix = indexer()
            ix.build_dictionary()
            assert ix.db.get_count() == n

        from_master()                               # warm-up: every shape of the timed window
        from_npy()
        t_master, t_npy = [], []
        for _ in range(a.repeats):                  # alternate: the host is shared
            t_master.append(timed(from_master))
            t_npy.append(timed(from_npy))

    def rate(ts):
        return {"min_s": round(min(ts), 4), "median_s": round(statistics.median(ts), 4),
                "patterns_per_s_best": round(n / min(ts), 1),
                "patterns_per_s_median": round(n / statistics.median(ts), 1)}

    sim_s = serial["simulate_ms"] * 1e-3
    enc_rate = B / (serial["encoder_ms"] * 1e-3)
    out_bytes, gathers = 4 * h * w * B, 4 * h * w * B
    print(json.dumps({
        "tool": "dictionary_rate", "patterns": n, "batch": a.batch, "master_side": a.master,
        "detector": [h, w], "repeats": a.repeats, "per_batch_serial": serial,
        "simulate_over_encoder": round(serial["simulate_ms"] / serial["encoder_ms"], 4),
        "encoder_alone_patterns_per_s": round(enc_rate, 1),
        "from_master": rate(t_master), "from_npy": rate(t_npy),
        "from_master_over_encoder_alone": round(n / statistics.median(t_master) / enc_rate, 4),
        "speedup_median": round(statistics.median(t_npy) / statistics.median(t_master), 3),
        "simulate_bound": {"bytes_written": out_bytes, "gathers": gathers,
                           "written_GB_per_s": round(out_bytes / sim_s / 1e9, 1),
                           "gathers_G_per_s": round(gathers / sim_s / 1e9, 1)},
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
