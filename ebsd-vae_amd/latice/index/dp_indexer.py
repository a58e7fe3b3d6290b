"""Drop-in `latice.index.dp_indexer` (reference: latice/index/dp_indexer.py) on the MI355X
path: same `IndexerConfig` and `DiffractionPatternIndexer` API and call contracts.

* `build_dictionary` (:92-111) -> `_create_dataloader` (:234-252, the drop-in DPDataModule:
  device batches from one transform launch each) -> `_extract_latent_vectors_with_angles`
  (:254-297), which calls `self.model(data)` exactly once per batch and keeps `mu`, as the
  reference's tests pin (tests/index/test_dp_indexer.py:117-119, :305).  With the drop-in
  model that call runs the encoder and the heads only: its eval/no-grad forward defers the
  decoder (latice.model, latice.deferred).
* The default database is the HBM-resident `FaissLatentVectorDatabase` (exact cosine top-k +
  batched orientation consensus as HIP kernels); the reference defaults to a Chroma HNSW
  collection (chromadb is a third-party service, out of scope).  Any object with
  add_vectors / find_best_orientation / find_best_orientations_batch can be passed as `db`.
* encode_patterns_batch transforms a numpy stack in ONE launch when the transform is the
  default one (the reference loops per pattern, :149-163).
* `index_scan` has no counterpart in the reference: a whole scan (a .npy path, a host array of
  float or uint8 patterns, or a transformed device tensor) streams through pinned staging
  buffers (`_stream_batches`), the scan's ingest plan, `encode_mu` and `db.index_latents`,
  and comes back as one `ScanIndexResult` of numpy arrays (latice/index/scan.py).  The plan
  is a `latice.patterns.ScanIngest`, built once per scan: it checks `correction=
  PatternCorrection(...)` (raw detector scans: static and dynamic background, rescale) and
  `resample=DetectorResample(...)` (detector-size patterns binned to the model's input size
  in front of either ingest) against the scan and fixes which device stages a staged batch
  runs through.  `neighbour_average=NeighbourAverage(...)` averages every transformed pattern
  with its neighbours on the scan grid between ingest and encoder; a host scan then streams
  through a device ring of transformed patterns (latice/index/scan.py `neighbour_schedule`).
  `nlpar=NLPAR(...)` takes the averaging's place with weights from the pattern distances
  (csrc/nlpar.hip): the same ring and schedule, one scan row and column further each way.
  `scan_background` streams a scan into its mean pattern, the usual static background.
  `maps=ScanMaps(...)` appends the scan maps (latice/index/maps.py, csrc/scan_maps.hip: IPF
  colours, orientation similarity, kernel average misorientation), built from the result rows
  behind the last batch, to the same result buffer and the same single copy back.
* `build_dictionary_from_master` has no counterpart either: the dictionary patterns are projected
  from a master pattern on the device, batch by batch, in front of `encode_mu`
  (latice/simulation.py, csrc/simulate.hip); only the orientation list is uploaded.
"""
from __future__ import annotations

import logging
from functools import cached_property
from pathlib import Path
from typing import Literal

import numpy as np
import torch
from pydantic.dataclasses import dataclass

from latice.data_module import DPDataModule, PatternTransform, create_default_transform
from latice.index.faiss_db import (MAX_K, FaissLatentVectorDatabase,
                                   FaissLatentVectorDatabaseConfig, LatentIndexResult,
                                   OrientationResult)
from latice.index.grains import GrainMap, grain_rows
from latice.index.maps import (IPF_DIRECTIONS, ScanMaps, ipf_rows, misorientation_rows,
                               similarity_rows)
from latice.index.scan import (SCAN_F32, SCAN_F64, SCAN_U8, ScanIndexResult, neighbour_schedule,
                               open_scan, scan_batches, scan_dtype_code)
from latice.model import VariationalAutoEncoder
from latice.patterns import (NLPAR, DetectorResample, NeighbourAverage, PatternCorrection,
                             ScanIngest, accumulate_patterns, average_neighbour_range,
                             correct_patterns, nlpar_range)
from latice.simulation import (DetectorGeometry, MasterPattern, check_dictionary_request,
                               simulate_patterns)

logger = logging.getLogger(__name__)

__all__ = ["IndexerConfig", "DiffractionPatternIndexer", "OrientationResult", "ScanIndexResult"]


@dataclass
class IndexerConfig:
    """dp_indexer.py:26-48 (identical fields and defaults)."""

    pattern_path: Path
    angles_path: Path
    batch_size: int = 64
    device: Literal["cuda", "cpu", "mps"] = "cpu"
    latent_dim: int = 16
    random_seed: int = 42
    image_size: tuple[int, int] = (128, 128)
    top_n: int = 20
    orientation_threshold: float = 3.0


def _default_db(dimension: int, device: torch.device):
    """The reference's default store is `ChromaLatentVectorDatabase(dimension=...)`
    (dp_indexer.py:73-77).  It is used when `latice.index.chroma_db` resolves (a reference
    checkout on LATICE_REFERENCE_ROOT and chromadb installed); otherwise the HBM-resident
    exact inner-product store `FaissLatentVectorDatabase` takes its place, with a warning
    (same add / query API, exact instead of HNSW search)."""
    try:
        from latice.index.chroma_db import ChromaLatentVectorDatabase
    except Exception as e:  # noqa: BLE001 - chromadb or the module absent
        logger.warning("ChromaLatentVectorDatabase is not available (%s: %s); using the "
                       "HBM-resident exact FaissLatentVectorDatabase as the default store",
                       type(e).__name__, e)
        return FaissLatentVectorDatabase(
            FaissLatentVectorDatabaseConfig(dimension=dimension, device=str(device)))
    return ChromaLatentVectorDatabase(dimension=dimension)


_NUMPY = {torch.float64: np.float64, torch.int64: np.int64, torch.float32: np.float32,
          torch.int32: np.int32, torch.uint8: np.uint8}


def _check_raw_stage(name: str, stage, cls, patterns) -> None:
    """An optional stage of index_scan that works on raw host patterns: its type, and that the
    scan is not a tensor."""
    if stage is None:
        return
    if not isinstance(stage, cls):
        raise TypeError(f"{name} must be a {cls.__name__}, got {type(stage).__name__}")
    if torch.is_tensor(patterns):
        raise ValueError(f"a tensor scan is already transformed: `{name}` applies to "
                         "host scans of raw detector patterns")


def _result_buffer(n: int, k: int, candidates: bool, dev, maps: ScanMaps | None = None):
    """The results of an n-pattern scan (k candidates per pattern if `candidates`) as views
    of ONE device buffer, so one copy brings them all back; with `maps`, the scan maps are
    further fields of it.  Returns (the buffer, its layout [(name, dtype, shape, byte offset,
    bytes)], the index fields as a `LatentIndexResult`, the map fields by name)."""
    grains = maps is not None and maps.grains
    # the 8-byte fields come first to keep every view aligned, the bytes last
    fields = [("best", torch.float64, (n, 3)), ("row", torch.int64, (n,))]
    fields += [("cand_idx", torch.int64, (n, k))] if candidates else []
    # the grains' only 8-byte field sits with the 8-byte group; without grains nothing moves
    map_fields = [("grain_orientation", torch.float64, (n, 3))] if grains else []
    fields += map_fields
    fields += [("score", torch.float32, (n,)), ("success", torch.int32, (n,)),
               ("n_similar", torch.int32, (n,))]
    fields += [("cand_scores", torch.float32, (n, k))] if candidates else []
    tail_fields = []
    if maps is not None:
        tail_fields += [("osm", torch.float32, (n,))] if maps.similarity else []
        tail_fields += [("kam", torch.float32, (n,))] if maps.kam else []
        if grains:
            tail_fields += [("grain_id", torch.int32, (n,)), ("gos", torch.float32, (n,)),
                            ("grod", torch.float32, (n,))]
        tail_fields += [("ipf_" + d, torch.uint8, (n, 3)) for d in maps.ipf]
        tail_fields += [("grain_boundary", torch.uint8, (n,))] if grains else []
    map_fields = map_fields + tail_fields
    layout, end = [], 0
    for name, dt, shape in fields + tail_fields:
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
        layout.append((name, dt, shape, end, nbytes))
        end += nbytes
    buf = torch.empty(max(end, 8), dtype=torch.uint8, device=dev)
    views = {name: buf[o:o + nb].view(dt).view(shape) for name, dt, shape, o, nb in layout}
    map_views = {name: views.pop(name) for name, _, _ in map_fields}
    return buf, layout, LatentIndexResult(**views), map_views


def _unpack_result(buf: torch.Tensor, layout, maps: ScanMaps | None = None) -> ScanIndexResult:
    """The one device-to-host copy of a scan's results (and the host's only wait)."""
    host = buf.cpu().numpy()
    h = {name: host[o:o + nb].view(_NUMPY[dt]).reshape(shape) for name, dt, shape, o, nb in layout}
    result = ScanIndexResult(orientations=h["best"], success=h["success"].astype(bool),
                             scores=h["score"], top_index=h["row"], n_similar=h["n_similar"],
                             candidate_indices=h.get("cand_idx"),
                             candidate_scores=h.get("cand_scores"))
    if maps is not None:
        grid = maps.scan_shape
        result.ipf_colors = {d: h["ipf_" + d].reshape(grid + (3,)) for d in maps.ipf}
        if maps.similarity:
            result.orientation_similarity = h["osm"].reshape(grid)
        if maps.kam:
            result.kam = h["kam"].reshape(grid)
        if maps.grains:
            result.grains = GrainMap(grain_id=h["grain_id"].reshape(grid),
                                     grain_orientation=h["grain_orientation"].reshape(grid + (3,)),
                                     gos=h["gos"].reshape(grid), grod=h["grod"].reshape(grid),
                                     boundary=h["grain_boundary"].reshape(grid))
    return result


def _run_maps(maps: ScanMaps, res: LatentIndexResult, views: dict):
    """The scan maps of the whole scan's result rows `res` into their fields `views` of the result
    buffer, on the current stream: behind the last batch, in front of the copy back.  Returns the
    grains' device scratch (None without grains), to be kept until the copy back."""
    for d in maps.ipf:
        ipf_rows(res.best, IPF_DIRECTIONS[d], views["ipf_" + d])
        if maps.mask_failed:
            views["ipf_" + d].masked_fill_((res.success == 0).unsqueeze(1), 0)
    if maps.similarity:
        similarity_rows(res.cand_idx, maps.scan_shape, maps.connectivity,
                        maps.similarity_normalize, views["osm"])
    if maps.kam:
        misorientation_rows(res.best, maps.scan_shape, maps.connectivity, maps.kam_max_angle,
                            views["kam"])
    if maps.grains:
        return grain_rows(res.best, res.success if maps.grain_mask_failed else None,
                          maps.scan_shape, maps.connectivity, maps.grain_threshold,
                          views["grain_id"], views["grain_orientation"], views["gos"],
                          views["grod"], views["grain_boundary"])
    return None


class DiffractionPatternIndexer:
    """dp_indexer.py:51-297."""

    def __init__(self, model: VariationalAutoEncoder, db=None, config: IndexerConfig | None = None) -> None:
        self.config = config if config is not None else IndexerConfig()
        np.random.seed(self.config.random_seed)
        torch.manual_seed(self.config.random_seed)
        self.device = torch.device(self.config.device)
        if self.config.device == "cuda" and not torch.cuda.is_available():
            logger.warning("CUDA not available, falling back to CPU")
            self.device = torch.device("cpu")
        logger.info(f"Using device: {self.device}")
        if self.device.type == "cpu" and isinstance(model, VariationalAutoEncoder):
            # the drop-in model has no CPU path: IndexerConfig's default device "cpu" would
            # only fail later, deep inside the first encode
            if not torch.cuda.is_available():
                raise RuntimeError("DiffractionPatternIndexer: the MI355X VAE needs a ROCm device "
                                   "(config.device='cpu' and no GPU is visible; no CPU fallback)")
            logger.warning("config.device='cpu': the drop-in VAE runs on the ROCm device; using "
                           "cuda:%d", torch.cuda.current_device())
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.db = db if db is not None else _default_db(self.config.latent_dim, self.device)
        self.model = model
        self.model.eval()
        self.model.to(self.device)

    def build_dictionary(self) -> None:
        """dp_indexer.py:92-111: latent vectors of every pattern -> the database."""
        data_module = self._create_dataloader
        logger.info(f"Generating latent vectors from patterns in {self.config.pattern_path}")
        latent_vectors, orientations = self._extract_latent_vectors_with_angles(data_module)
        logger.info(f"Adding {len(latent_vectors)} vectors to database")
        self.db.add_vectors(latent_vectors, orientations)

    def build_dictionary_from_master(self, master: MasterPattern, orientations,
                                     detector: DetectorGeometry | None = None,
                                     batch_size: int | None = None,
                                     correction: PatternCorrection | None = None) -> None:
        """The dictionary of `orientations` ((N, 3) float64 host array, Bunge angles in degrees)
        simulated from `master` on the device instead of read from a pattern file; the reference
        has no counterpart.  `detector` defaults to `DetectorGeometry(config.image_size)` and must
        have the model's image size.  The orientation list is uploaded once; per batch one
        `simulate_patterns` launch fills a reused batch buffer, `model.encode_mu` reads it and the
        latents go into their rows of one (N, d) device tensor; one `db.add_vectors(latents,
        orientations)` follows the last batch.  Nothing inside the loop waits for the device and
        no pattern ever leaves it.

        With `correction` (a `PatternCorrection` without a static background, which belongs to a
        detector) every batch is simulated without the rescale and passes through
        `correct_patterns` at equal size: the dynamic background step and the rescale of the
        experimental side.  Everything is checked (ValueError) before the device is touched."""
        ori, detector, batch_size = check_dictionary_request(
            self.config.image_size, master, orientations, detector,
            batch_size or self.config.batch_size, correction)
        if self.device.type != "cuda":
            raise RuntimeError("build_dictionary_from_master needs a ROCm device (no CPU fallback)")
        n, dev = ori.shape[0], self.device
        h, w = detector.shape
        logger.info(f"Simulating and encoding {n} dictionary patterns from a master pattern")
        with torch.cuda.device(dev):
            ori_dev = torch.from_numpy(ori).to(dev)
            x = torch.empty(min(batch_size, n), 1, h, w, dtype=torch.float32, device=dev)
            y = torch.empty_like(x) if correction is not None else None
            latents = None
            for s in range(0, n, batch_size):
                m = min(batch_size, n - s)
                simulate_patterns(master, ori_dev[s:s + m], detector, rescale=correction is None,
                                  out=x[:m])
                xb = x[:m]
                if correction is not None:
                    xb = correct_patterns(x[:m].view(m, h, w), (h, w), correction, dev, out=y[:m])
                mu = self.model.encode_mu(xb)
                if latents is None:
                    latents = torch.empty(n, mu.shape[1], dtype=torch.float32, device=dev)
                latents[s:s + m].copy_(mu)
        logger.info(f"Adding {n} vectors to database")
        self.db.add_vectors(latents, ori)

    def encode_pattern(self, pattern) -> np.ndarray:
        """dp_indexer.py:113-136."""
        transform = create_default_transform(self.config.image_size)
        if isinstance(pattern, np.ndarray):
            pattern = transform(pattern)
        if pattern.dim() == 2:
            pattern = pattern.unsqueeze(0)
        if pattern.dim() == 3:
            pattern = pattern.unsqueeze(0)
        pattern = pattern.to(self.device)
        with torch.no_grad():
            _, _, mu, _ = self.model(pattern)
        return mu.cpu().numpy().squeeze()

    def encode_patterns_batch(self, patterns) -> np.ndarray:
        """dp_indexer.py:138-186."""
        transform = create_default_transform(self.config.image_size)
        if isinstance(patterns, np.ndarray):
            if patterns.ndim == 2:
                patterns = transform(patterns).unsqueeze(0)
            elif patterns.ndim == 3:
                if isinstance(transform, PatternTransform):
                    patterns = transform.batch(patterns)   # one launch for the whole stack
                else:
                    patterns = torch.stack([transform(patterns[i]) for i in range(patterns.shape[0])])
        else:
            if patterns.dim() == 2:
                patterns = patterns.unsqueeze(0).unsqueeze(0)
            elif patterns.dim() == 3:
                patterns = patterns.unsqueeze(1)
        assert patterns.dim() == 4, f"Expected 4D tensor, got {patterns.dim()}D"
        patterns = patterns.to(self.device)
        batch_size = self.config.batch_size
        latent_vectors = []
        with torch.no_grad():
            for i in range(0, patterns.shape[0], batch_size):
                _, _, mu, _ = self.model(patterns[i:i + batch_size])
                latent_vectors.append(mu.cpu().numpy())
        return np.vstack(latent_vectors)

    def index_pattern(self, pattern, top_n: int | None = None,
                      orientation_threshold: float | None = None) -> OrientationResult:
        """dp_indexer.py:188-214."""
        top_n = top_n or self.config.top_n
        orientation_threshold = orientation_threshold or self.config.orientation_threshold
        latent_vector = self.encode_pattern(pattern)
        return self.db.find_best_orientation(latent_vector, top_n=top_n,
                                             orientation_threshold=orientation_threshold)

    def index_patterns_batch(self, patterns, **kwargs):
        """dp_indexer.py:216-232."""
        latent_vectors = self.encode_patterns_batch(patterns)
        return self.db.find_best_orientations_batch(latent_vectors, batch_size=self.config.batch_size,
                                                    **kwargs)

    def index_scan(self, patterns, top_n: int | None = None,
                   orientation_threshold: float | None = None, min_required_matches: int = 18,
                   max_iterations: int = 3, batch_size: int | None = None,
                   return_candidates: bool = False,
                   correction: PatternCorrection | None = None,
                   neighbour_average: NeighbourAverage | None = None,
                   resample: DetectorResample | None = None,
                   nlpar: NLPAR | None = None,
                   maps: ScanMaps | None = None) -> ScanIndexResult:
        """A whole scan in, an orientation map out, everything between on the device.

        `patterns` is a path to a .npy file (memory-mapped), a numpy array / memmap
        (N, H0, W0) of float64, float32 (the DPdataset transform, `ingest_patterns`) or uint8
        (detector data, `ingest_patterns_u8`: v / 255), or a device tensor (N, 1, h, w)
        float32 that is already transformed.  Per batch: host slice -> one of two pinned
        staging buffers -> async copy on a copy stream -> ingest -> `model.encode_mu` ->
        `db.index_latents` into result arrays preallocated for all N patterns (44 B per
        pattern without candidates).  The host waits only for a staging buffer to be free
        again, never for a batch's results; the results come back in one copy at the end.

        With `correction` (a `PatternCorrection`) a host scan of raw detector patterns takes
        the background-corrected ingest `correct_patterns` in place of the plain one, for
        every staging dtype; a device tensor is already transformed and cannot take one.

        With `neighbour_average` (a `NeighbourAverage` whose scan_shape holds the N patterns)
        every transformed pattern is averaged with its neighbours on the scan grid before the
        encoder reads it: ingest or correction, then averaging, then encoder.  It acts on
        transformed patterns, so a device tensor may take it too.  A host scan is ingested, each
        pattern once, into a device ring of batch_size + 2 (hr cols + hc) transformed patterns;
        the outputs whose neighbours have all arrived are averaged straight into the encoder's
        batch buffer, in chunks of at most batch_size.

        With `resample` (a `DetectorResample`) a host scan of detector-size patterns is binned
        to the model's input size on the device, in front of everything else
        (`resample_patterns`: the area mean of the resample's region): uint8 patterns straight
        into the encoder's batch buffer (or the ring) at v / 255, float patterns through one
        intermediate and the plain ingest at equal size, and with a `correction` through that
        intermediate into `correct_patterns`, whose static background stays at detector shape
        and whose `dynamic_sigma` is in output pixels.  The intermediate is allocated once per
        scan.  A device tensor is already transformed and cannot take one.

        With `nlpar` (an `NLPAR` whose scan_shape holds the N patterns) non-local pattern
        averaging takes the place of `neighbour_average` (one or the other): ingest, correction
        or resample, then NLPAR, then encoder.  A device tensor may take it; a host scan streams
        through the same ring, which holds batch_size + 2 ((hr + 1) cols + hc + 1) patterns,
        because a neighbour's noise estimate needs that neighbour's own surroundings.  The
        result does not depend on batch_size.

        With `maps` (a `ScanMaps` whose scan_shape holds the N patterns, and equals the
        scan_shape of `neighbour_average` / `nlpar` when one is given) the requested scan maps
        -- IPF colours, orientation similarity, kernel average misorientation
        (latice/index/maps.py) -- are built once on the compute stream from the result rows of
        the whole scan, after the last batch is queued, for host and tensor scans alike.  They
        are further fields of the one result buffer (still one copy back and one host wait) and
        of the `ScanIndexResult`.  The similarity map needs every pattern's candidate rows on
        the device: without `return_candidates` they live in a device tensor that is not copied
        back.  With `maps.grains` the grain segmentation (latice/index/grains.py) follows them the
        same way and comes back as `ScanIndexResult.grains`.  Without `maps` nothing runs
        differently."""
        _check_raw_stage("resample", resample, DetectorResample, patterns)
        if nlpar is not None and not isinstance(nlpar, NLPAR):
            raise TypeError(f"nlpar must be an NLPAR, got {type(nlpar).__name__}")
        if nlpar is not None and neighbour_average is not None:
            raise ValueError("index_scan takes `nlpar` or `neighbour_average`, not both")
        if neighbour_average is not None and not isinstance(neighbour_average, NeighbourAverage):
            raise TypeError("neighbour_average must be a NeighbourAverage, got "
                            f"{type(neighbour_average).__name__}")
        _check_raw_stage("correction", correction, PatternCorrection, patterns)
        top_n = top_n or self.config.top_n
        orientation_threshold = orientation_threshold or self.config.orientation_threshold
        batch_size = int(batch_size or self.config.batch_size)
        if not callable(getattr(self.db, "index_latents", None)):
            raise TypeError(f"index_scan needs a database with index_latents(latents, ..., out=) "
                            f"that works on device tensors (FaissLatentVectorDatabase); "
                            f"{type(self.db).__name__} has none")
        if top_n > MAX_K:
            raise ValueError(f"top_n={top_n} > {MAX_K} (GPU top-k limit)")
        if batch_size < 1:
            raise ValueError(f"batch_size={batch_size} must be at least 1")
        kw = dict(top_n=top_n, orientation_threshold=orientation_threshold,
                  min_required_matches=min_required_matches, max_iterations=max_iterations)
        on_device = torch.is_tensor(patterns)
        if on_device:
            if not (patterns.is_cuda and patterns.dim() == 4 and patterns.shape[1] == 1
                    and patterns.dtype == torch.float32):
                raise ValueError("a tensor scan must be a transformed (N, 1, h, w) float32 device "
                                 f"tensor, got {tuple(patterns.shape)} {patterns.dtype} on "
                                 f"{patterns.device}")
            n, dev = patterns.shape[0], patterns.device
        else:
            patterns = open_scan(patterns)
            items = scan_batches(patterns, batch_size)
            n, dev = patterns.shape[0], self.device
            plan = ScanIngest(patterns.shape[1:], scan_dtype_code(patterns.dtype),
                              self.config.image_size, dev, min(batch_size, n), correction, resample)
        # the averaging stage, if any: the record and its ring function (the schedule plans
        # with the record's schedule_half)
        stage, stage_range = neighbour_average, average_neighbour_range
        if nlpar is not None:
            stage, stage_range = nlpar, nlpar_range
        if stage is not None:
            stage.check(n)
        if maps is not None:
            if not isinstance(maps, ScanMaps):
                raise TypeError(f"maps must be a ScanMaps, got {type(maps).__name__}")
            maps.check(n)
            if stage is not None and tuple(stage.scan_shape) != maps.scan_shape:
                raise ValueError(f"maps.scan_shape {maps.scan_shape} differs from the scan_shape "
                                 f"{tuple(stage.scan_shape)} of the averaging stage")
        need_rows = maps is not None and maps.similarity
        k = min(top_n, self.db.get_count()) if return_candidates or need_rows else 0
        if need_rows and k < 1:
            raise ValueError("the similarity map needs candidate rows: the dictionary is empty")
        buf, layout, res, map_views = _result_buffer(n, k, return_candidates, dev, maps)
        if need_rows and not return_candidates:
            # the whole scan's candidate rows, for the similarity map alone: never copied back
            res.cand_idx = torch.empty(n, k, dtype=torch.int64, device=dev)

        def encode_index(x, a, b):
            """Transformed patterns x of the scan's [a, b) -> their rows of the result."""
            self.db.index_latents(self.model.encode_mu(x), out=res.slice(a, b), **kw)

        def average_index(ring, x, chunks):
            """Every chunk [a, b) averaged out of `ring` into x[:b - a], encoded and indexed."""
            for a, b in chunks:
                stage_range(ring, stage, a, b - a, x)
                encode_index(x[:b - a], a, b)

        staging = None
        if on_device and stage is not None and n:
            ring = patterns.contiguous()     # a resident scan is its own ring
            with torch.cuda.device(dev):
                x = torch.empty((min(batch_size, n),) + tuple(ring.shape[1:]),
                                dtype=torch.float32, device=dev)
            average_index(ring, x, [(s, min(s + batch_size, n)) for s in range(0, n, batch_size)])
            staging = (ring, x)
        elif on_device:
            for s in range(0, n, batch_size):
                e = min(s + batch_size, n)
                encode_index(patterns[s:e], s, e)
        elif n and stage is not None:
            staging = self._stream_scan_averaged(patterns, items, batch_size, dev, plan,
                                                 stage.scan_shape[1], stage.schedule_half,
                                                 average_index)
        elif n:
            staging = self._stream_scan(patterns, items, batch_size, dev, plan, encode_index)

        if maps is not None:
            with torch.cuda.device(dev):
                staging = (staging, _run_maps(maps, res, map_views))   # and the grains' scratch
        result = _unpack_result(buf, layout, maps)     # the host's only wait
        del staging                  # every copy-stream buffer outlived its last consumer
        return result

    def _stream_scan(self, patterns, items, batch_size, dev, plan, encode_index):
        """index_scan over a host scan: every staged batch goes through the scan's ingest `plan`
        into one (B, 1, h, w) buffer, then is encoded and indexed into its rows of the result."""
        h, w = self.config.image_size
        with torch.cuda.device(dev):
            x = torch.empty(min(batch_size, patterns.shape[0]), 1, h, w, dtype=torch.float32,
                            device=dev)
        return self._stream_batches(patterns, items, batch_size, dev,
                                    lambda i, raw: plan.plan(raw, x[:raw.shape[0]]),
                                    lambda i, s, e: encode_index(x[:e - s], s, e)) + (x,)

    def _stream_scan_averaged(self, patterns, items, batch_size, dev, plan, cols, half,
                              average_index):
        """index_scan over a host scan of `cols` columns with neighbour averaging or NLPAR over
        a reach of `half` = (rows, columns) each way: every staged batch is ingested,
        once, into its slots of a ring of transformed patterns (`neighbour_schedule`, one step
        per batch; in two parts where it passes the ring's end); the outputs that are complete
        after it are averaged from the ring into the encoder's batch buffer, chunk by chunk,
        then encoded and indexed into their rows of the result.  All of it is work on the
        compute stream, in order: the ring is overwritten only after the last averaging that
        reads the old patterns."""
        h, w = self.config.image_size
        n = patterns.shape[0]
        schedule = neighbour_schedule(n, cols, half[0], half[1], batch_size)
        steps = schedule.steps
        with torch.cuda.device(dev):
            ring = torch.empty(schedule.ring_cap, 1, h, w, dtype=torch.float32, device=dev)
            x = torch.empty(min(batch_size, n), 1, h, w, dtype=torch.float32, device=dev)

        def ingest(i, raw):
            start = steps[i].start
            for a, b, slot in steps[i].ingest:
                plan.plan(raw[a - start:b - start], ring[slot:slot + b - a])

        return self._stream_batches(patterns, items, batch_size, dev, ingest,
                                    lambda i, s, e: average_index(ring, x, steps[i].ready)) + (ring, x)

    def _stream_batches(self, patterns, items, batch_size, dev, ingest, then=None):
        """The host half of a streamed scan: batch i is copied from the scan into pinned buffer
        i & 1, then to device buffer i & 1 on a copy stream, while the compute stream still
        works on batch i - 1; `ingest(i, staged batch)` is the one consumer of the device buffer,
        `then(i, start, stop)` whatever follows it on the compute stream.  Events order the two
        streams in both directions; the host waits only for `copied[j]` (the copy out of the
        pinned buffer it is about to refill).  The staging buffers are returned: the caller
        keeps them alive until it has synchronised the compute stream, which has waited for
        every copy."""
        per = tuple(patterns.shape[1:])
        code = items[0][2]
        th_dt = {SCAN_F64: torch.float64, SCAN_F32: torch.float32, SCAN_U8: torch.uint8}[code]
        shape = (min(batch_size, patterns.shape[0]),) + per
        with torch.cuda.device(dev):
            compute = torch.cuda.current_stream(dev)
            copy = torch.cuda.Stream(dev)
            pinned = [torch.empty(shape, dtype=th_dt).pin_memory() for _ in range(2)]
            pinned_np = [p.numpy() for p in pinned]
            staged = [torch.empty(shape, dtype=th_dt, device=dev) for _ in range(2)]
            # the allocator may hand out blocks with work still pending on the compute stream
            begun = torch.cuda.Event()
            begun.record(compute)
            copy.wait_event(begun)
            copied = [None, None]     # copy stream: pinned[j] -> staged[j] finished
            ingested = [None, None]   # compute stream: the ingest that read staged[j] finished
            for i, (s, e, _) in enumerate(items):
                j, m = i & 1, e - s
                if copied[j] is not None:
                    copied[j].synchronize()          # pinned[j] is free to refill
                np.copyto(pinned_np[j][:m], patterns[s:e], casting="unsafe")
                if ingested[j] is not None:
                    copy.wait_event(ingested[j])     # staged[j] is free to overwrite
                with torch.cuda.stream(copy):
                    staged[j][:m].copy_(pinned[j][:m], non_blocking=True)
                copied[j] = torch.cuda.Event()
                copied[j].record(copy)
                compute.wait_event(copied[j])
                ingest(i, staged[j][:m])
                ingested[j] = torch.cuda.Event()
                ingested[j].record(compute)
                if then is not None:
                    then(i, s, e)
        return pinned, staged

    def scan_background(self, patterns, batch_size: int | None = None) -> np.ndarray:
        """The mean pattern of a scan, the usual static background: `patterns` (a .npy path or a
        host array (N, H0, W0)) streams through the staging buffers of index_scan into a
        float64 running sum on the device (`ebsdvae_accumulate_patterns`).  Returns the
        (H0, W0) float32 pattern float32(sum / N), the division in float64."""
        batch_size = int(batch_size or self.config.batch_size)
        patterns = open_scan(patterns)
        items = scan_batches(patterns, batch_size)
        if not items:
            raise ValueError("scan_background needs at least one pattern")
        if self.device.type != "cuda":
            raise RuntimeError("scan_background needs a ROCm device (no CPU fallback)")
        acc = torch.zeros(tuple(patterns.shape[1:]), dtype=torch.float64, device=self.device)
        staging = self._stream_batches(patterns, items, batch_size, self.device,
                                       lambda i, raw: accumulate_patterns(raw, acc))
        total = acc.cpu().numpy()    # the host's one wait: every batch has been added
        del staging
        return (total / patterns.shape[0]).astype(np.float32)

    @cached_property
    def _create_dataloader(self):
        """dp_indexer.py:234-252."""
        datamodule = DPDataModule(path=self.config.pattern_path,
                                  rot_angles_path=self.config.angles_path,
                                  image_size=self.config.image_size,
                                  batch_size=self.config.batch_size)
        datamodule.setup("test")
        return datamodule.test_dataloader()

    def _extract_latent_vectors_with_angles(self, data_loader):
        """dp_indexer.py:254-297: one model call per batch, mu kept (a rich progress bar as
        in the reference when rich is importable)."""
        latent_vectors, orientations = [], []
        try:
            from rich.progress import (BarColumn, Progress, SpinnerColumn, TextColumn,
                                       TimeElapsedColumn)
            progress = Progress(SpinnerColumn(), TextColumn("[progress.description]{task.description}"),
                                BarColumn(), TextColumn("[progress.percentage]{task.percentage:>3.0f}%"),
                                TimeElapsedColumn())
        except Exception:  # noqa: BLE001
            progress = None
        ctx = progress if progress is not None else _NullProgress()
        with ctx:
            task = ctx.add_task("[cyan]Processing patterns...", total=len(data_loader))
            with torch.no_grad():
                for batch in data_loader:
                    data, angles = batch
                    data = data.to(self.device)
                    _, _, mu, _ = self.model(data)
                    latent_vectors.append(mu.cpu().numpy())
                    orientations.append(np.asarray(angles))
                    ctx.update(task, advance=1)
        return np.concatenate(latent_vectors, axis=0), np.concatenate(orientations, axis=0)


class _NullProgress:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def add_task(self, *a, **k):
        return 0

    def update(self, *a, **k):
        return None
