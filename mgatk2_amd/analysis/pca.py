"""Principal components of the heteroplasmy matrix.

mgatk's vignette closes by naming what the matrix is for; the first item is dimensionality
reduction. This is R's ``prcomp(t(af), center = TRUE, scale. = scale)`` on the device
(``mgp_pca``, mgp_pca.hip): the variants' means (and standard deviations), the covariance of the
centred (scaled) variants over the cells, its eigenpairs by a fixed-order Jacobi iteration and the
cells' scores on the first components. Every number is a chain of fp64 operations whose order the
matrix's shape fixes (include/mgpileup.h), so the same matrix gives the same bytes on every run.

Definitions. Items are the columns of ``x [n_feat, n_items]``. Eigenvalues descend (ties: the lower
diagonal place first); each eigenvector's entry of largest magnitude is positive (the lowest index
among equals); ``scores[c, i]`` is the projection of item i's centred (scaled) column on eigenvector c.

Item numbers (:func:`.variants.heteroplasmy_matrix` has the reason): cells in column order, features in genomic order.
"""

from __future__ import annotations

import logging
import math
import time
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from .. import engine as _engine
from ..exceptions import InvalidInputError
from .variants import heteroplasmy_matrix, variants_dir

logger = logging.getLogger(__name__)

PCA_MAX_ITEMS = _engine.PCA_MAX_ITEMS
PCA_MAX_FEAT = _engine.PCA_MAX_FEAT
PCA_MAX_COMP = 50  # components asked for on the command line


def check_pca(n) -> int:
    """The number of components as an int, 1 <= n <= PCA_MAX_COMP."""
    if isinstance(n, bool) or (isinstance(n, float) and not n.is_integer()):
        raise InvalidInputError(f"pca must be an integer in 1..{PCA_MAX_COMP}, got {n!r}")
    try:
        n = int(n)
    except (TypeError, ValueError):
        raise InvalidInputError(f"pca must be an integer in 1..{PCA_MAX_COMP}, got {n!r}") from None
    if not 1 <= n <= PCA_MAX_COMP:
        raise InvalidInputError(f"pca must be in 1..{PCA_MAX_COMP}, got {n}")
    return n


@dataclass
class PcaResult:
    """The components of the cells; scores is None when there was nothing to decompose (fewer than
    2 cells or no variant)."""

    n: int                                 # cells (items)
    n_comp: int                            # components after clipping to min(variants, cells - 1)
    mean: np.ndarray | None = None         # [m] the variants' means
    sd: np.ndarray | None = None           # [m] the divisor with scale, else sqrt of the covariance's diagonal
    eigenvalues: np.ndarray | None = None  # [m] all of them, descending
    loadings: np.ndarray | None = None     # [n_comp, m] row c = eigenvector c
    scores: np.ndarray | None = None       # [n_comp, n]
    sweeps: int = 0                        # Jacobi sweeps that rotated
    scale: bool = False
    seconds: float = 0.0


def pca(x, n_comp: int, scale: bool = False, device: int = 0) -> PcaResult:
    """The first n_comp principal components of the columns of x [n_feat, n_items] on the device. n_comp above
    min(n_feat, n_items - 1) is clipped (logged); fewer than 2 items or no feature give an empty result
    without a launch."""
    x = np.ascontiguousarray(x, np.float64)
    if x.ndim != 2:
        raise InvalidInputError("x is [n_feat, n_items]")
    k, (m, n) = int(n_comp), x.shape
    if k < 1:
        raise InvalidInputError(f"n_comp must be at least 1, got {k}")
    t0 = time.perf_counter()
    if n < 2 or m < 1:
        return PcaResult(n, 0, scale=bool(scale))
    if k > min(m, n - 1):
        logger.info("PCA: %d components clipped to %d (min of the features and the other items)", k, min(m, n - 1))
        k = min(m, n - 1)
    out = _engine.pca(x, k, bool(scale), device)
    return PcaResult(n, k, out["mean"], out["sd"], out["eigenvalues"], out["loadings"], out["scores"], out["sweeps"],
                     bool(scale), time.perf_counter() - t0)


def principal_components(result_or_matrix, barcodes=None, table=None, n_comp: int = 10, scale: bool = False,
                         device: int = 0) -> PcaResult:
    """The principal components of the cells of the heteroplasmy matrix [n_variants, n_cells] (a
    VariantResult, or the matrix itself). `barcodes` and `table`, when given, must match the matrix's
    shape; with a VariantTable the variants are taken in genomic order (heteroplasmy_matrix's note), and
    mean, sd and the loadings' columns are in that order. Fewer than 2 cells or no variant give an empty
    result (logged). More than PCA_MAX_ITEMS cells or PCA_MAX_FEAT variants raise InvalidInputError."""
    n_comp = check_pca(n_comp)
    af, table, rows = heteroplasmy_matrix(result_or_matrix, barcodes, table)
    nv, nc = af.shape
    if nv < 1 or nc < 2:
        logger.info("PCA skipped: %d variants x %d cells (at least 1 variant and 2 cells are needed)", nv, nc)
        return PcaResult(nc, 0, scale=bool(scale))
    if nc > PCA_MAX_ITEMS:
        raise InvalidInputError(f"PCA: {nc} cells, more than {PCA_MAX_ITEMS} in one call")
    if nv > PCA_MAX_FEAT:
        raise InvalidInputError(f"PCA: {nv} variants, more than {PCA_MAX_FEAT} in one call")
    return pca(af if rows is None else af[rows], n_comp, scale, device)


# ---- output files --------------------------------------------------------------------

def variance_table(eigenvalues, n_comp: int):
    """(sdev, variance_fraction, cumulative) of the first n_comp components: sdev = sqrt(max(eigenvalue, 0)),
    the fraction over the sum of all eigenvalues added in their (descending) order, the running sum of the
    fractions."""
    ev = [float(v) for v in np.asarray(eigenvalues, np.float64).tolist()]
    total = 0.0
    for v in ev:
        total += v
    sdev, frac, cum, run = [], [], [], 0.0
    for v in ev[:n_comp]:
        sdev.append(math.sqrt(max(v, 0.0)))
        frac.append(v / total if total != 0.0 else 0.0)
        run += frac[-1]
        cum.append(run)
    return sdev, frac, cum


def _variant_names(table, m: int) -> list[str]:
    """The variants' names in genomic order (the order of the loadings' columns), or V1.. without a table."""
    if table is None or not hasattr(table, "variant"):
        return [f"V{f + 1}" for f in range(m)]
    names = list(table.variant)
    if hasattr(table, "position") and hasattr(table, "base"):
        order = np.lexsort((np.asarray(table.base), np.asarray(table.position)))
        names = [names[int(f)] for f in order]
    return names


def write_cell_pca(result: PcaResult, barcodes: list[str], path) -> None:
    """cell_pca.tsv: barcode, PC1 .. PCk; one line per cell, floats as repr."""
    cols = result.scores.T.tolist()
    with open(path, "w") as fh:
        fh.write("\t".join(["barcode"] + [f"PC{c + 1}" for c in range(result.n_comp)]) + "\n")
        for b, row in zip(barcodes, cols):
            fh.write("\t".join([b] + [repr(v) for v in row]) + "\n")


def write_variant_loadings(result: PcaResult, names: list[str], path) -> None:
    """variant_loadings.tsv: variant, mean, sd, PC1 .. PCk; one line per variant in genomic order."""
    cols = result.loadings.T.tolist()
    with open(path, "w") as fh:
        fh.write("\t".join(["variant", "mean", "sd"] + [f"PC{c + 1}" for c in range(result.n_comp)]) + "\n")
        for name, mu, sd, row in zip(names, result.mean.tolist(), result.sd.tolist(), cols):
            fh.write("\t".join([name, repr(mu), repr(sd)] + [repr(v) for v in row]) + "\n")


def write_pca_variance(result: PcaResult, path) -> None:
    """pca_variance.tsv: component, eigenvalue, sdev, variance_fraction, cumulative."""
    sdev, frac, cum = variance_table(result.eigenvalues, result.n_comp)
    with open(path, "w") as fh:
        fh.write("component\teigenvalue\tsdev\tvariance_fraction\tcumulative\n")
        for c in range(result.n_comp):
            fh.write(f"PC{c + 1}\t{float(result.eigenvalues[c])!r}\t{sdev[c]!r}\t{frac[c]!r}\t{cum[c]!r}\n")


def write_pca_outputs(result: PcaResult, barcodes: list[str], table, output_dir) -> Path:
    """The components' files in the run's variants/ directory: cell_pca.tsv, variant_loadings.tsv and
    pca_variance.tsv. An empty result writes nothing."""
    vdir = variants_dir(output_dir)
    if result is None or result.scores is None:
        return vdir
    barcodes = list(barcodes)
    if len(barcodes) != result.scores.shape[1]:
        raise InvalidInputError(f"{len(barcodes)} barcodes for {result.scores.shape[1]} cells")
    write_cell_pca(result, barcodes, vdir / "cell_pca.tsv")
    write_variant_loadings(result, _variant_names(table, result.loadings.shape[1]), vdir / "variant_loadings.tsv")
    write_pca_variance(result, vdir / "pca_variance.tsv")
    return vdir
