"""EBSD pattern indexer on the MI355X path (latice/index in the reference).

`dp_indexer.DiffractionPatternIndexer` keeps the reference's API and call contracts;
`faiss_db.FaissLatentVectorDatabase` keeps the FAISS-backed API (latice/index/faiss_db.py)
with the dictionary resident in HBM: exact cosine top-k and the orientation consensus run as
HIP kernels (csrc/search.hip, csrc/orient.hip; fused for whole scans in csrc/scan_index.hip,
`DiffractionPatternIndexer.index_scan`).  Other reference modules of this package
(chroma_db, latent_embedding) resolve from LATICE_REFERENCE_ROOT (see latice/__init__.py).
`maps` holds the scan maps built from an indexed scan's result rows (csrc/scan_maps.hip): IPF
colours, the orientation similarity map and the kernel average misorientation; `grains` the grain
segmentation of such a scan with the grain mean orientation, GROD, GOS and the boundary map
(csrc/grains.hip).
"""
from latice import _extend_path

_extend_path(__path__, "index")

from latice.index.maps import (ScanMaps, ipf_colors, kernel_average_misorientation,  # noqa: E402
                               orientation_similarity_map)
from latice.index.grains import GrainMap, segment_grains  # noqa: E402

__all__ = ["ScanMaps", "ipf_colors", "kernel_average_misorientation",
           "orientation_similarity_map", "GrainMap", "segment_grains"]
