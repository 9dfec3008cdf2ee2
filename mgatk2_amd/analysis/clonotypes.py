"""The cells' clonotypes: Louvain communities of the shared-nearest-neighbour graph on the device.

The second half of Signac's ``FindClonotypes``: after ``FindNeighbors`` (:mod:`.neighbors`) it
calls ``FindClusters`` on the SNN graph and then orders the clusters by a complete-linkage tree
over their mean heteroplasmy. The CPU tools' community detection is randomised because it visits
the vertices one by one in a random order. Here a pass is synchronous (every vertex decides from
one snapshot) and every sum is an integer sum, so the result is a function of the graph alone:
the same labels, the same bytes of Q, on every call (``mgp_louvain``, mgp_louvain.hip; the
definition is pinned in include/mgpileup.h and DESIGN.md 7.10).

Weights are integers in units of 2^-20, quantised once (:func:`quantise`). The SNN's implicit
diagonal is left out, as Seurat's ``RunModularityClusteringCpp`` leaves it out. Signac's own
defaults differ from ours before this step (cosine metric, k = 10, the SLM algorithm); the graph
here is the Euclidean one ``--neighbors`` defines.

Clonotypes are numbered from 0 by descending size (ties by smallest member) in the result and
from 1 in the files, as ``cell_clones.tsv`` numbers its clones.
"""

from __future__ import annotations

import logging
import math
import time
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from .. import engine as _engine
from ..exceptions import InvalidInputError
from .variants import heteroplasmy_matrix, variants_dir

logger = logging.getLogger(__name__)

WEIGHT_ONE = _engine.LOUVAIN_MAX_WEIGHT  # the integer of weight 1.0
MAX_VERTICES = _engine.LOUVAIN_MAX_VERTICES
MAX_EDGES = _engine.LOUVAIN_MAX_EDGES
MAX_LEVELS = _engine.LOUVAIN_MAX_LEVELS
MAX_PASSES = _engine.LOUVAIN_MAX_PASSES


def quantise(weight) -> np.ndarray:
    """floor(weight * 2^20 + 0.5) of the fp64 weights, int64 (in range: 1..2^20)."""
    w = np.asarray(weight, np.float64)
    if not np.all(np.isfinite(w)):
        raise InvalidInputError("a weight is not finite")
    return np.floor(w * float(WEIGHT_ONE) + 0.5).astype(np.int64)


def _checked_edges(n, i, j, wq):
    """The edge list as the C entry takes it, every refusal of its made here first (no device)."""
    n = int(n)
    i, j, wq = (np.asarray(a).reshape(-1) for a in (i, j, wq))
    if not i.size == j.size == wq.size:
        raise InvalidInputError("i, j and the weights have one entry per edge")
    for a in (i, j, wq):
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise InvalidInputError("edge ends and quantised weights are integers")
    if not 0 <= n <= MAX_VERTICES:
        raise InvalidInputError(f"communities: {n} vertices, not in 0..{MAX_VERTICES}")
    if i.size > MAX_EDGES:
        raise InvalidInputError(f"communities: {i.size} edges, more than {MAX_EDGES} in one call")
    i, j, wq = i.astype(np.int64), j.astype(np.int64), wq.astype(np.int64)
    if i.size:
        if np.any(i >= j):
            raise InvalidInputError("an edge is not i < j")
        if i.min() < 0 or j.max() >= n:
            raise InvalidInputError(f"an edge's end is outside [0, {n})")
        if wq.min() < 1 or wq.max() > WEIGHT_ONE:
            raise InvalidInputError(f"a quantised weight is outside 1..{WEIGHT_ONE}")
        if np.unique(i * n + j).size != i.size:
            raise InvalidInputError("a pair is repeated")
    return n, i.astype(np.int32), j.astype(np.int32), wq.astype(np.int32)


def check_resolution(resolution) -> float:
    """Seurat's resolution as a float, finite and above 0."""
    resolution = float(resolution)
    if not (math.isfinite(resolution) and resolution > 0.0):
        raise InvalidInputError(f"the resolution must be finite and above 0, got {resolution}")
    return resolution


def _checked_options(resolution, max_levels, max_passes):
    resolution, max_levels, max_passes = check_resolution(resolution), int(max_levels), int(max_passes)
    if not 1 <= max_levels <= MAX_LEVELS:
        raise InvalidInputError(f"max_levels must be in 1..{MAX_LEVELS}, got {max_levels}")
    if not 1 <= max_passes <= MAX_PASSES:
        raise InvalidInputError(f"max_passes must be in 1..{MAX_PASSES}, got {max_passes}")
    return resolution, max_levels, max_passes


@dataclass
class Communities:
    """mgp_louvain's result. labels: 0.. by descending size, ties by smallest member; m2,
    internal, b: the integers M2, I, B of the final partition; levels: (vertices, communities,
    passes, accepted passes) of each level run."""

    labels: np.ndarray
    n_communities: int
    modularity: float
    m2: int = 0
    internal: int = 0
    b: int = 0
    levels: list = field(default_factory=list)
    seconds: float = 0.0


def communities(n, i, j, weight, resolution: float = 1.0, max_levels: int = 32, max_passes: int = 64,
                device: int = 0) -> Communities:
    """The Louvain communities (the module's definition) of the graph of n vertices with the
    undirected edges (i, j), i < j, each pair once. `weight`: fp64 weights in (0, 1], quantised
    here, or integers already quantised (1..2^20). Every invalid input raises InvalidInputError
    before the device is touched; without an edge nothing is launched."""
    w = np.asarray(weight)
    wq = w if (w.size == 0 or np.issubdtype(w.dtype, np.integer)) else quantise(w)
    n, i, j, wq = _checked_edges(n, i, j, wq)
    resolution, max_levels, max_passes = _checked_options(resolution, max_levels, max_passes)
    t0 = time.perf_counter()
    r = _engine.graph_louvain(n, i, j, wq, resolution, max_levels, max_passes, device)
    return Communities(r["labels"], r["n_communities"], r["modularity"], r["m2"], r["internal"], r["b"],
                       r["levels"], time.perf_counter() - t0)


def modularity(n, i, j, weight, labels, resolution: float = 1.0) -> float:
    """The definition's Q of anyone's labels, on the host in Python integers:
    Q = (double(M2) * double(I) - resolution * double(B)) / double(M2) / double(M2). No edge: 0."""
    w = np.asarray(weight)
    wq = w if (w.size == 0 or np.issubdtype(w.dtype, np.integer)) else quantise(w)
    n, i, j, wq = _checked_edges(n, i, j, wq)
    labels = [int(c) for c in np.asarray(labels).reshape(-1)]
    if len(labels) != n:
        raise InvalidInputError(f"{len(labels)} labels for {n} vertices")
    resolution = float(resolution)
    tot: dict = {}
    m2 = internal = 0
    for a, b, q in zip(i.tolist(), j.tolist(), wq.tolist()):
        m2 += 2 * q
        tot[labels[a]] = tot.get(labels[a], 0) + q
        tot[labels[b]] = tot.get(labels[b], 0) + q
        if labels[a] == labels[b]:
            internal += 2 * q
    if m2 == 0:
        return 0.0
    big = sum(t * t for t in tot.values())
    return (float(m2) * float(internal) - resolution * float(big)) / float(m2) / float(m2)


@dataclass
class Clonotypes:
    """find_clonotypes' result. result is None when there was no graph (fewer than 2 cells or no
    variant). With the heteroplasmy matrix: mean_af [n_variants, n_clonotypes] in the matrix's
    row order, and rank [n_clonotypes], the heatmap position (1-based) of each clonotype."""

    n: int
    result: Communities | None
    resolution: float = 1.0
    n_cells: np.ndarray | None = None   # [n_clonotypes] cells of each
    mean_af: np.ndarray | None = None
    rank: np.ndarray | None = None
    seconds: dict = field(default_factory=dict)


def find_clonotypes(neighbor_graph, allele_freq=None, table=None, resolution: float = 1.0, max_levels: int = 32,
                    max_passes: int = 64, device: int = 0) -> Clonotypes:
    """The clonotypes of a NeighborGraph's SNN graph. With `allele_freq` [n_variants, n_cells]
    (and `table`, whose genomic order the tree's features then take: heteroplasmy_matrix's note)
    also each clonotype's mean heteroplasmy and the clonotypes' heatmap order by the device's
    complete-linkage tree over those means (what FindClonotypes does after clustering; one
    clonotype has rank 1). No graph gives no result (logged)."""
    from .clustering import hclust

    resolution, max_levels, max_passes = _checked_options(resolution, max_levels, max_passes)
    t0 = time.perf_counter()
    g = neighbor_graph
    if g is None or g.idx is None:
        logger.info("Clonotypes skipped: no neighbour graph (at least 1 variant and 2 cells are needed)")
        return Clonotypes(int(getattr(g, "n", 0) or 0), None, resolution, seconds={"louvain": 0.0, "order": 0.0,
                                                                                  "total": 0.0})
    n = int(g.n)
    res = communities(n, g.i, g.j, np.asarray(g.weight, np.float64), resolution, max_levels, max_passes, device)
    t1 = time.perf_counter()
    sizes = np.bincount(res.labels, minlength=res.n_communities).astype(np.int64)
    mean_af = rank = None
    if allele_freq is not None:
        af, table, rows = heteroplasmy_matrix(allele_freq, table=table)
        if af.shape[1] != n:
            raise InvalidInputError(f"the heteroplasmy matrix is [n_variants, {n}]")
        mean_af = np.zeros((af.shape[0], res.n_communities), np.float64)
        for k in range(res.n_communities):
            mean_af[:, k] = af[:, res.labels == k].mean(axis=1)
        if res.n_communities >= 2 and af.shape[0] >= 1:
            x = mean_af if rows is None else mean_af[rows]
            order = hclust(x=np.ascontiguousarray(x), device=device).order
            rank = np.empty(res.n_communities, np.int32)
            rank[order - 1] = np.arange(1, res.n_communities + 1, dtype=np.int32)
        else:
            rank = np.arange(1, res.n_communities + 1, dtype=np.int32)
    t2 = time.perf_counter()
    return Clonotypes(n, res, resolution, sizes, mean_af, rank,
                      {"louvain": t1 - t0, "order": t2 - t1, "total": t2 - t0})


# ---- output files --------------------------------------------------------------------

def write_cell_clonotypes(clono: Clonotypes, barcodes: list[str], path) -> None:
    """cell_clonotypes.tsv: barcode, clonotype (1-based, 1 the largest)."""
    with open(path, "w") as fh:
        fh.write("barcode\tclonotype\n")
        for b, c in zip(barcodes, clono.result.labels.tolist()):
            fh.write(f"{b}\t{int(c) + 1}\n")


def write_clonotype_table(clono: Clonotypes, path) -> None:
    """clonotypes.tsv: clonotype, n_cells, rank (the heatmap position; the clonotype's own number
    when no matrix was given)."""
    with open(path, "w") as fh:
        fh.write("clonotype\tn_cells\trank\n")
        for k, nc in enumerate(clono.n_cells.tolist()):
            r = k + 1 if clono.rank is None else int(clono.rank[k])
            fh.write(f"{k + 1}\t{int(nc)}\t{r}\n")


def write_clonotype_outputs(clono: Clonotypes, barcodes: list[str], output_dir) -> Path:
    """The clonotypes' files in the run's variants/ directory: cell_clonotypes.tsv and
    clonotypes.tsv. No graph writes nothing."""
    vdir = variants_dir(output_dir)
    if clono is None or clono.result is None:
        return vdir
    barcodes = list(barcodes)
    if len(barcodes) != clono.n:
        raise InvalidInputError(f"{len(barcodes)} barcodes for {clono.n} cells")
    write_cell_clonotypes(clono, barcodes, vdir / "cell_clonotypes.tsv")
    write_clonotype_table(clono, vdir / "clonotypes.tsv")
    return vdir
