"""Device time of the scan maps (`ebsdvae_ipf_colors`, `ebsdvae_orientation_similarity`,
`ebsdvae_kernel_misorientation`, csrc/scan_maps.hip) and what they cost a whole `index_scan`.

Per map, from device events with the kernel alone on the stream (medians of 7), on a
--grid x --grid scan (1000 x 1000) at k = --top-n candidates (20): the IPF colours of one
direction, the similarity map at both connectivities, and the kernel average misorientation at
both connectivities within 5 degrees.  The orientations are grains of 50 x 50 points with 1 degree
of noise; a point's candidate rows are drawn from a pool of 2 k rows per grain, so neighbours share
about half of them.  Beside them the bytes each map reads and writes once and their time at
--copy-tbs, the streaming-copy rate of DESIGN.md section 7.

Then `DiffractionPatternIndexer.index_scan` on the scan of tools/scan_index_rate.py (16 x 1024
uint8 patterns at 140 x 140 in pinned memory, here a 128 x 128 grid, 1,048,576 dictionary rows,
top_n = 20) without maps, with the default map (IPF z) and with every map (three IPF directions,
similarity, KAM, connectivity 8), alternating the three in one process.

The grains leg (`ebsdvae_segment_grains`, csrc/grains.hip) runs on the same --grid scan in three
shapes: (a) the 50 x 50-point grains above at 5 degrees, (b) one grain filling the scan, the worst
case for contention on the per-grain accumulators, and (c) every point its own grain (threshold 0
on the noisy data); each at both connectivities, once with every output and once with the ids
only, beside the KAM time at the same connectivity from the same run.  The whole-scan comparison
gets a fourth variant, every map plus grains.

--maps-only skips the scans.

Prints one JSON line.  Needs a ROCm GPU: there is no CPU path.

    python tools/scan_maps_rate.py [--repeats 3] [--grid 1000] [--top-n 20] [--maps-only]
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
    ap.add_argument("--grid", type=int, default=1000, help="the maps' scan is grid x grid points")
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=128, help="scan columns of the index_scan runs")
    ap.add_argument("--rows", type=int, default=1 << 20, help="dictionary rows")
    ap.add_argument("--side", type=int, default=140)
    ap.add_argument("--top-n", type=int, default=20)
    ap.add_argument("--copy-tbs", type=float, default=6.3)
    ap.add_argument("--maps-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scan_maps_rate: no ROCm GPU (a time is measured on the device or not at all)")
    if a.repeats < 3:
        raise SystemExit("scan_maps_rate: at least 3 repeats")
    n = a.batches * a.batch
    if n % a.cols:
        raise SystemExit(f"scan_maps_rate: {n} patterns do not fill rows of {a.cols}")

    from latice import _native as N
    from latice.index.maps import ScanMaps, ipf_rows, misorientation_rows, similarity_rows

    logging.getLogger("latice").setLevel(logging.ERROR)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)

    # ---- each map alone on the stream
    g, k = a.grid, a.top_n
    pts = g * g
    grain = (np.arange(g)[:, None] // 50) * ((g + 49) // 50) + np.arange(g)[None, :] // 50
    base = rng.uniform(0, 360, (int(grain.max()) + 1, 3)) * [1, 0.5, 1]
    euler = torch.from_numpy((base[grain] + rng.uniform(-0.5, 0.5, (g, g, 3))).reshape(pts, 3)).to(dev)
    cand = torch.from_numpy((grain.reshape(pts, 1) * 2 * k
                             + rng.integers(0, 2 * k, (pts, k))).astype(np.int64)).to(dev)
    rgb = torch.empty(pts, 3, dtype=torch.uint8, device=dev)
    f32 = torch.empty(pts, dtype=torch.float32, device=dev)
    calls = {"ipf_z_ms": (lambda: ipf_rows(euler, 2, rgb), pts * (24 + 3)),
             "similarity_4_ms": (lambda: similarity_rows(cand, (g, g), 4, False, f32), pts * (8 * k + 4)),
             "similarity_8_ms": (lambda: similarity_rows(cand, (g, g), 8, False, f32), pts * (8 * k + 4)),
             "kam_4_ms": (lambda: misorientation_rows(euler, (g, g), 4, 5.0, f32), pts * (24 + 4)),
             "kam_8_ms": (lambda: misorientation_rows(euler, (g, g), 8, 5.0, f32), pts * (24 + 4))}
    per_map = {}
    for key, (fn, moved) in calls.items():
        fn()
        torch.cuda.synchronize()
        per_map[key] = round(_events(fn), 4)
        per_map[key.replace("_ms", "_floor_ms")] = round(moved / (a.copy_tbs * 1e12) * 1e3, 4)
    similarity_rows(cand, (g, g), 4, False, f32)
    per_map["similarity_mean"] = round(float(f32.mean()), 3)
    misorientation_rows(euler, (g, g), 4, 5.0, f32)
    per_map["kam_mean_deg"] = round(float(f32.mean()), 4)

    # ---- grains: three shapes x two connectivities x (every output, ids only)
    from latice.index.grains import grain_rows
    one = torch.from_numpy((base[0] + rng.uniform(-0.5, 0.5, (pts, 3)))).to(dev)
    ids = torch.empty(pts, dtype=torch.int32, device=dev)
    outs = dict(grain_euler=torch.empty(pts, 3, dtype=torch.float64, device=dev),
                gos=torch.empty(pts, dtype=torch.float32, device=dev),
                grod=torch.empty(pts, dtype=torch.float32, device=dev),
                boundary=torch.empty(pts, dtype=torch.uint8, device=dev))
    work = torch.empty(N.call("ebsdvae_grain_work", g, g), dtype=torch.uint8, device=dev)
    grains = {}
    for shape_name, e, thr in (("grains_50x50", euler, 5.0), ("one_grain", one, 5.0),
                               ("every_point", euler, 0.0)):
        for conn in (4, 8):
            for what, kw_out in (("all", outs), ("ids", {})):
                fn = lambda: grain_rows(e, None, (g, g), conn, thr, ids, work=work, **kw_out)  # noqa: E731
                fn()
                torch.cuda.synchronize()
                key = f"{shape_name}_{conn}_{what}"
                grains[key + "_ms"] = round(_events(fn), 4)
                grains[key + "_over_kam"] = round(grains[key + "_ms"] / per_map[f"kam_{conn}_ms"], 3)
            grains[f"{shape_name}_{conn}_n_grains"] = int(ids.max()) + 1
    per_map["grains"] = grains
    del euler, cand, rgb, f32, one, ids, outs, work

    out = {"tool": "scan_maps_rate", "grid": [g, g], "top_n": k, "copy_tbs": a.copy_tbs,
           "per_map": per_map}

    # ---- the whole scan, without and with maps
    if not a.maps_only:
        from latice.index.dp_indexer import DiffractionPatternIndexer, IndexerConfig
        from latice.index.faiss_db import FaissLatentVectorDatabase, FaissLatentVectorDatabaseConfig
        from latice.model import VariationalAutoEncoderRawData
        from latice.seeding import seeded_state_dict

        scan_t = torch.empty(n, a.side, a.side, dtype=torch.uint8).pin_memory()
        scan = scan_t.numpy()
        scan[:] = rng.integers(0, 256, scan.shape, dtype=np.uint8)
        model = VariationalAutoEncoderRawData()
        model.load_state_dict({k_: torch.from_numpy(v) for k_, v in seeded_state_dict(0).items()})
        db = FaissLatentVectorDatabase(FaissLatentVectorDatabaseConfig(
            npz_path="/nonexistent/scan_maps_rate.npz", dimension=16, device="cuda:0"))
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
        shape = (n // a.cols, a.cols)
        every = ScanMaps(shape, ipf=("x", "y", "z"), similarity=True, kam=True, connectivity=8)
        with_grains = ScanMaps(shape, ipf=("x", "y", "z"), similarity=True, kam=True, connectivity=8,
                               grains=True)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res

        runs = {"index_scan": lambda: ix.index_scan(scan, batch_size=a.batch, **kw),
                "index_scan_ipf_z": lambda: ix.index_scan(scan, batch_size=a.batch,
                                                          maps=ScanMaps(shape), **kw),
                "index_scan_every_map": lambda: ix.index_scan(scan, batch_size=a.batch, maps=every, **kw),
                "index_scan_every_map_grains": lambda: ix.index_scan(scan, batch_size=a.batch,
                                                                     maps=with_grains, **kw)}
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

        out.update(patterns=n, scan_shape=list(shape), batch=a.batch, side=a.side,
                   dictionary_rows=a.rows, repeats=a.repeats,
                   **{name: rate(ts) for name, ts in times.items()})
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
