"""The cells' k-nearest-neighbour graph and shared-nearest-neighbour graph by heteroplasmy.

The step of mgatk's vignette after the heatmap, "Integration with Seurat/Signac": Signac's
``FindClonotypes`` calls ``FindNeighbors`` on the heteroplasmy matrix, a kNN graph of the cells
over the variants and Seurat's ``ComputeSNN`` on it, and gives the SNN graph to a graph clusterer.
The device makes both graphs (``mgp_knn`` / ``mgp_snn``, mgp_graph.hip) without the n x n
distance matrix. Community detection on the SNN graph is :mod:`.clonotypes` (a deterministic
Louvain on the device); ``FindClusters``, igraph and leidenalg also take the graph written here.

Definitions (include/mgpileup.h). Items are the columns of ``x [n_feat, n_items]``. The distance
of a pair is the number ``pair_dist`` gives for it, bit for bit. Row i of the kNN holds the k
items j != i smallest under (distance, then j), in that order, 0-based. With
``S_i = {i} + knn[i]`` (K = k + 1 members, Seurat's ``k.param``), ``shared = |S_i & S_j|`` and the
weight is Seurat's ``shared / (2K - shared)``, kept when ``weight >= prune``. The device counts in
integers: ``prune`` becomes the smallest count that passes (:func:`min_shared_for`) and the
weight is one division here. Every output is unique: the order is strict.

Item numbers (:func:`.variants.heteroplasmy_matrix` has the reason): cells in column order, features in genomic order.
"""

from __future__ import annotations

import logging
import time
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from .. import engine as _engine
from ..exceptions import InvalidInputError
from .variants import heteroplasmy_matrix, variants_dir

logger = logging.getLogger(__name__)

GRAPH_MAX_ITEMS = _engine.GRAPH_MAX_ITEMS
GRAPH_MAX_K = _engine.GRAPH_MAX_K
DEFAULT_PRUNE = 1.0 / 15.0  # Seurat's prune.SNN


def check_neighbors(neighbors) -> int:
    """Seurat's k.param (the cell and its K - 1 nearest others) as an int, 2 <= K <= GRAPH_MAX_K + 1."""
    neighbors = int(neighbors)
    if not 2 <= neighbors <= GRAPH_MAX_K + 1:
        raise InvalidInputError(f"neighbors must be in 2..{GRAPH_MAX_K + 1}, got {neighbors}")
    return neighbors


def check_prune(prune) -> float:
    """Seurat's prune.SNN as a float, 0 <= prune <= 1 (a NaN is refused)."""
    prune = float(prune)
    if not 0.0 <= prune <= 1.0:
        raise InvalidInputError(f"prune must be in [0, 1], got {prune}")
    return prune


def min_shared_for(K: int, prune: float) -> int:
    """The smallest shared count s in 1..K that Seurat's ComputeSNN keeps among sets of K members:
    its own fp64 expression s / (2K - s), kept unless below `prune` (0 <= prune <= 1)."""
    K = int(K)
    if K < 1:
        raise InvalidInputError(f"K must be at least 1, got {K}")
    prune = check_prune(prune)
    for s in range(1, K + 1):
        if not float(s) / float(2 * K - s) < prune:
            return s
    raise InvalidInputError(f"no shared count passes prune = {prune}")  # (not reached: s = K gives 1)


def knn(x, k: int, device: int = 0):
    """(idx [n, k] int32, dist [n, k]) of the columns of x [n_feat, n_items] on the device. k above
    n - 1 is clipped (logged); fewer than 2 items give empty [n, 0] arrays without a launch."""
    x = np.ascontiguousarray(x, np.float64)
    if x.ndim != 2:
        raise InvalidInputError("x is [n_feat, n_items]")
    k, n = int(k), x.shape[1]
    if k < 1:
        raise InvalidInputError(f"k must be at least 1, got {k}")
    if n <= 1:
        return np.zeros((n, 0), np.int32), np.zeros((n, 0), np.float64)
    if k > n - 1:
        logger.info("kNN: k = %d clipped to %d (the other items)", k, n - 1)
        k = n - 1
    return _engine.graph_knn(x, k, device)


def snn(idx, prune: float = DEFAULT_PRUNE, device: int = 0):
    """(i, j, shared, weight) of the SNN graph of the kNN table idx [n, k], i < j, sorted by
    (i, j): int32, int32, int32 and fp64 (Seurat's Jaccard weight, >= prune)."""
    idx = np.ascontiguousarray(idx, np.int32)
    if idx.ndim != 2:
        raise InvalidInputError("idx is [n_items, k]")
    n, k = idx.shape
    K = k + 1
    ms = min_shared_for(K, prune)
    if n <= 1 or k == 0:
        e = np.zeros(0, np.int32)
        return e, e.copy(), e.copy(), np.zeros(0, np.float64)
    i, j, shared = _engine.graph_snn(idx, ms, device)
    return i, j, shared, shared.astype(np.float64) / (2.0 * K - shared.astype(np.float64))


@dataclass
class NeighborGraph:
    """Both graphs of the cells; idx is None when there was nothing to build (fewer than 2
    cells or no variant)."""

    n: int
    k_param: int                 # Seurat's k.param after clipping: the cell and its k_param - 1 neighbours
    idx: np.ndarray | None       # [n, k_param - 1] int32, 0-based
    dist: np.ndarray | None      # [n, k_param - 1]
    i: np.ndarray | None = None  # the SNN edges, i < j, sorted by (i, j)
    j: np.ndarray | None = None
    shared: np.ndarray | None = None
    weight: np.ndarray | None = None
    prune: float = DEFAULT_PRUNE
    seconds: dict = field(default_factory=dict)


def neighbor_graph(result_or_matrix, barcodes=None, table=None, neighbors: int = 20, prune: float = DEFAULT_PRUNE,
                   device: int = 0) -> NeighborGraph:
    """The kNN and SNN graphs of the cells of the heteroplasmy matrix [n_variants, n_cells] (a
    VariantResult, or the matrix itself). `neighbors` = K is Seurat's k.param (the cell and its
    K - 1 nearest others, 2 <= K <= GRAPH_MAX_K + 1; clipped to the number of cells), `prune` its
    prune.SNN. `barcodes` and `table`, when given, must match the matrix's shape; with a
    VariantTable the features are taken in genomic order (heteroplasmy_matrix's note). Fewer than 2 cells
    or no variant give no graph (logged). More than GRAPH_MAX_ITEMS cells raise InvalidInputError."""
    neighbors, prune = check_neighbors(neighbors), check_prune(prune)
    t0 = time.perf_counter()
    af, table, rows = heteroplasmy_matrix(result_or_matrix, barcodes, table)
    nv, nc = af.shape
    if nv < 1 or nc < 2:
        logger.info("Neighbour graph skipped: %d variants x %d cells (at least 1 variant and 2 cells are needed)",
                    nv, nc)
        return NeighborGraph(nc, neighbors, None, None, prune=prune,
                             seconds={"knn": 0.0, "snn": 0.0, "total": time.perf_counter() - t0})
    if nc > GRAPH_MAX_ITEMS:
        raise InvalidInputError(f"neighbour graph: {nc} cells, more than {GRAPH_MAX_ITEMS} in one call")
    idx, dist = knn(af if rows is None else af[rows], neighbors - 1, device)
    t1 = time.perf_counter()
    i, j, shared, weight = snn(idx, prune, device)
    t2 = time.perf_counter()
    return NeighborGraph(nc, idx.shape[1] + 1, idx, dist, i, j, shared, weight, prune,
                         {"knn": t1 - t0, "snn": t2 - t1, "total": t2 - t0})


# ---- output files --------------------------------------------------------------------

def write_knn(graph: NeighborGraph, barcodes: list[str], path) -> None:
    """cell_knn.tsv: barcode, rank, neighbor, distance; k lines per cell, rank 1 first."""
    with open(path, "w") as fh:
        fh.write("barcode\trank\tneighbor\tdistance\n")
        for c, (row, drow) in enumerate(zip(graph.idx.tolist(), graph.dist.tolist())):
            for r, (j, d) in enumerate(zip(row, drow)):
                fh.write(f"{barcodes[c]}\t{r + 1}\t{barcodes[j]}\t{d!r}\n")


def write_snn_mtx(graph: NeighborGraph, path) -> None:
    """cell_snn.mtx: Matrix Market coordinate real symmetric, 1-based, n x n, the lower triangle
    with the diagonal at weight 1 (Seurat's matrix), sorted by column, then row."""
    n = int(graph.n)
    ei, ej, w = graph.i.tolist(), graph.j.tolist(), graph.weight.tolist()
    with open(path, "w") as fh:
        fh.write("%%MatrixMarket matrix coordinate real symmetric\n")
        fh.write(f"{n} {n} {n + len(ei)}\n")
        e = 0
        for c in range(n):
            fh.write(f"{c + 1} {c + 1} {1.0!r}\n")
            while e < len(ei) and ei[e] == c:  # (the edges are sorted by (i, j): column i, rows j > i)
                fh.write(f"{ej[e] + 1} {c + 1} {w[e]!r}\n")
                e += 1


def write_neighbor_outputs(graph: NeighborGraph, barcodes: list[str], output_dir) -> Path:
    """The graphs' files in the run's variants/ directory: cell_knn.tsv, cell_snn.mtx and
    cell_snn_barcodes.tsv (one barcode per line, the matrix's order). No graph writes nothing."""
    vdir = variants_dir(output_dir)
    if graph is None or graph.idx is None:
        return vdir
    barcodes = list(barcodes)
    write_knn(graph, barcodes, vdir / "cell_knn.tsv")
    write_snn_mtx(graph, vdir / "cell_snn.mtx")
    (vdir / "cell_snn_barcodes.tsv").write_text("".join(b + "\n" for b in barcodes))
    return vdir
