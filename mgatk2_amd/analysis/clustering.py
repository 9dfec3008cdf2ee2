"""Cells and variants clustered by heteroplasmy: Euclidean distances and complete linkage.

The step of mgatk's vignette after ``calculate_allele_freq`` (R/mgatk2_qc_plots.R:121-139):
``pheatmap(allele_freq_mat, cluster_rows = TRUE, cluster_cols = TRUE)`` with its defaults,
that is ``dist()`` over the variants and over the cells of the heteroplasmy matrix and
``hclust(..., "complete")`` on each. The device makes the pair distances and the linkage
(``mgp_pair_dist`` / ``mgp_hclust_dist`` / ``mgp_hclust``, mgp_cluster.hip); the host turns
the n - 1 raw steps into R's ``merge`` and ``order`` (in the library) and cuts the tree (here).

Items are the columns of ``x [n_feat, n_items]``, the layout of ``allele_freq`` with cells
as items; for variants as items the transpose is passed. Outputs follow R's ``hclust``:
1-based, item i as ``-(i + 1)`` and the cluster of step s as ``s`` in ``merge``, so an R user
can rebuild an ``hclust`` object from the files and hand it to ``pheatmap(cluster_cols = ...)``.
Ties go to the smallest i, then the smallest j (R's rule); given the distances, every output
is exact.

Item numbers (:func:`.variants.heteroplasmy_matrix` has the reason): cells in column order, variants in genomic order.
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

CLUSTER_MAX_ITEMS = _engine.CLUSTER_MAX_ITEMS


@dataclass
class HClust:
    """R's hclust object, 1-based: merge [n - 1, 2], height [n - 1] (non-decreasing), order [n]."""

    merge: np.ndarray
    height: np.ndarray
    order: np.ndarray
    n: int

    def cutree(self, k: int) -> np.ndarray:
        """R's cutree(tree, k): the first n - k merges applied, the clusters numbered 1.. by
        their first appearance in item order. [n] int32."""
        n, k = int(self.n), int(k)
        if n == 0 and k == 0:
            return np.zeros(0, np.int32)
        if not 1 <= k <= n:
            raise InvalidInputError(f"cutree: k must be in 1..{n}, got {k}")
        # nodes: items 0..n-1, then the cluster of step s as n + s; a node takes its parent's root,
        # parents before children (steps descending)
        root = list(range(2 * n - 1))
        merge = self.merge.tolist()
        for s in range(n - k - 1, -1, -1):
            for v in merge[s]:
                root[-v - 1 if v < 0 else n + v - 1] = root[n + s]
        _, first, inv = np.unique(np.array(root[:n], np.int64), return_index=True, return_inverse=True)
        rank = np.empty(first.size, np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(1, first.size + 1)  # by first appearance in item order
        return rank[inv.reshape(-1)].astype(np.int32)


def _result(merge, height, order) -> HClust:
    return HClust(np.asarray(merge, np.int32).reshape(-1, 2), np.asarray(height, np.float64),
                  np.asarray(order, np.int32), int(np.asarray(order).shape[0]))


def pair_dist(x, device: int = 0) -> np.ndarray:
    """[n, n] Euclidean distances of the columns of x [n_feat, n_items] in fp64, on the device:
    exactly symmetric, zero diagonal, equal columns at exactly 0, the same bytes on every call."""
    return _engine.cluster_pair_dist(x, device)


def hclust(x=None, dist=None, device: int = 0) -> HClust:
    """Complete linkage on the device, of the columns of x [n_feat, n_items] (the distances
    never leave the device) or of a symmetric, finite, non-negative matrix dist [n, n]."""
    if (x is None) == (dist is None):
        raise InvalidInputError("hclust: give x or dist (one of them)")
    if dist is not None:
        return _result(*_engine.cluster_hclust_dist(dist, device))
    return _result(*_engine.cluster_hclust(x, device)[:3])


@dataclass
class ClusterResult:
    """Both sides of the heatmap; a side is None when it has fewer than 2 items or features."""

    cells: HClust | None
    variants: HClust | None
    clones: np.ndarray | None  # [n cells] int32, 1-based (cutree of the cell tree), when asked for
    seconds: dict = field(default_factory=dict)
    variant_rows: np.ndarray | None = None  # the matrix row of each variant item (None: item i is row i)


def check_clones(clones) -> int | None:
    """`clones` as cluster_heteroplasmy takes it: None (no cut), or K >= 1 as an int."""
    if clones is not None and int(clones) < 1:
        raise InvalidInputError(f"clones must be at least 1, got {clones}")
    return None if clones is None else int(clones)


def cluster_heteroplasmy(result_or_matrix, barcodes=None, table=None, clones: int | None = None,
                         device: int = 0) -> ClusterResult:
    """The two trees of the heteroplasmy matrix [n_variants, n_cells] (a VariantResult, or the
    matrix itself): cells clustered over the variants and variants over the cells, and with
    `clones` = K the cell tree cut into K clones. `barcodes` and `table` (the matrix's column
    and row names), when given, must match its shape; with a VariantTable the variants are
    numbered in genomic order (heteroplasmy_matrix's note; `variant_rows` is the matrix row of each
    item), otherwise in row order. A matrix with fewer than 2 cells or fewer
    than 2 variants gives no tree on either side (logged). More than CLUSTER_MAX_ITEMS items
    on a side raise InvalidInputError."""
    clones = check_clones(clones)
    t0 = time.perf_counter()
    af, table, rows = heteroplasmy_matrix(result_or_matrix, barcodes, table)
    nv, nc = af.shape
    if nv < 2 or nc < 2:
        logger.info("Clustering skipped: %d variants x %d cells (at least 2 of each are needed)", nv, nc)
        return ClusterResult(None, None, None, {"cells": 0.0, "variants": 0.0, "total": time.perf_counter() - t0})
    if clones is not None and clones > nc:
        raise InvalidInputError(f"clones must be in 1..{nc} (the cells), got {clones}")
    for side, n in (("cells", nc), ("variants", nv)):
        if n > CLUSTER_MAX_ITEMS:
            raise InvalidInputError(f"clustering: {n} {side}, more than {CLUSTER_MAX_ITEMS} in one call "
                                    "(the distance matrix is 8 n^2 bytes)")
    af = af if rows is None else np.ascontiguousarray(af[rows])
    cells = hclust(x=af, device=device)
    t1 = time.perf_counter()
    variants = hclust(x=np.ascontiguousarray(af.T), device=device)
    t2 = time.perf_counter()
    labels = cells.cutree(clones) if clones is not None else None
    return ClusterResult(cells, variants, labels, {"cells": t1 - t0, "variants": t2 - t1,
                                                   "total": time.perf_counter() - t0}, rows)


# ---- output files --------------------------------------------------------------------

def write_hclust(tree: HClust, path) -> None:
    """<side>_hclust.tsv: step, a, b, height (R's merge rows, floats as repr)."""
    with open(path, "w") as fh:
        fh.write("step\ta\tb\theight\n")
        for s in range(max(tree.n - 1, 0)):
            fh.write(f"{s + 1}\t{int(tree.merge[s, 0])}\t{int(tree.merge[s, 1])}\t{float(tree.height[s])!r}\n")


def read_hclust(path) -> HClust:
    """<side>_hclust.tsv back as an HClust (order rebuilt from the merges as R does)."""
    merge, height = [], []
    with open(path) as fh:
        fh.readline()
        for line in fh:
            _, a, b, h = line.rstrip("\n").split("\t")
            merge.append((int(a), int(b)))
            height.append(float(h))
    n = len(merge) + 1
    order, stack = [], [n - 1] if n > 1 else [-1]
    while stack:
        e = stack.pop()
        if e < 0:
            order.append(-e)
        else:
            stack.extend((merge[e - 1][1], merge[e - 1][0]))
    return _result(np.array(merge, np.int32).reshape(-1, 2), np.array(height, np.float64), np.array(order, np.int32))


def write_order(tree: HClust, names: list[str], path, what: str) -> None:
    """<side>_order.tsv: rank, name, the heatmap's order (rank 1 first)."""
    with open(path, "w") as fh:
        fh.write(f"rank\t{what}\n")
        for r, item in enumerate(tree.order.tolist()):
            fh.write(f"{r + 1}\t{names[item - 1]}\n")


def write_cluster_outputs(result: ClusterResult, barcodes: list[str], table, output_dir) -> Path:
    """The clustering's files in the run's variants/ directory: cell_hclust.tsv, cell_order.tsv,
    variant_hclust.tsv, variant_order.tsv and, when the cell tree was cut, cell_clones.tsv
    (barcode, clone). A side without a tree writes nothing. `table`: the VariantTable, or the
    variants' names, in the matrix's row order."""
    vdir = variants_dir(output_dir)
    names = list(getattr(table, "variant", table))
    if result.variant_rows is not None:
        names = [names[int(r)] for r in result.variant_rows]
    if result.cells is not None:
        write_hclust(result.cells, vdir / "cell_hclust.tsv")
        write_order(result.cells, list(barcodes), vdir / "cell_order.tsv", "barcode")
    if result.variants is not None:
        write_hclust(result.variants, vdir / "variant_hclust.tsv")
        write_order(result.variants, names, vdir / "variant_order.tsv", "variant")
    if result.cells is not None and result.clones is not None:
        with open(vdir / "cell_clones.tsv", "w") as fh:
            fh.write("barcode\tclone\n")
            for b, c in zip(barcodes, result.clones.tolist()):
                fh.write(f"{b}\t{int(c)}\n")
    return vdir
