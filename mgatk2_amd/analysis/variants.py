"""Variant calling from the engine's count rows: per-variant statistics and heteroplasmy.

The step mgatk users run next on ``counts.h5`` (``identify_variants`` and
``calculate_allele_freq`` of the reference's R functions, R/mgatk2_functions.R:282-372),
computed from the rows that are still on the device when a run ends. The device does the
reductions over cells (``Engine.variant_moments`` / ``variant_dev2`` / ``allele_freq``,
mgp_variants.hip); everything here is host numpy over their [L, 4] results.

Per cell, position and base b: ``f``, ``r`` the fwd / rev counts of b, ``cov`` the filtered
depth, ``af = (f + r) / cov`` (0 where cov == 0). The population is a list of cells; a cell
that did not pass is an all-zero row and counts with af = 0, exactly as the zero columns of
counts.h5 do in R. A variant is (position, base) with base != the reference allele
(``ref_alleles`` of the run's tally; an "N" position is a candidate for all four bases).

Values are the engine's exact counts, while counts.h5 stores min(v, 65535): the table and
the matrix equal R's on the HDF5 output wherever no count saturates. A whitelist with
duplicate barcodes is not supported (the population is one row per whitelist entry).
"""

from __future__ import annotations

import gzip
import math
import time
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from ..engine import MOMENT_FIELDS
from ..exceptions import InvalidInputError
from ..shard import DeviceParts

BASES = "ACGT"
TSV_COLUMNS = ("position", "nucleotide", "variant", "mean", "vmr", "n_cells_detected", "n_cells_conf_detected",
               "strand_correlation")


def merge_moments(parts: list[dict]) -> dict:
    """The moments of a population made of several device calls: the integer fields added,
    the fp64 partial sums added in part order."""
    if not parts:
        raise InvalidInputError("merge_moments: no parts")
    out = {k: np.array(parts[0][k], copy=True) for k in MOMENT_FIELDS}
    for p in parts[1:]:
        for k in MOMENT_FIELDS:
            out[k] += p[k]
    return out


def bulk_mean(moments: dict) -> np.ndarray:
    """[L, 4] bulk allele frequency, sum(total) / sum(cov): one fp64 division of exact sums
    (0 where the depth sum is 0)."""
    cov = moments["s_cov"].astype(np.float64)[:, None]
    tot = moments["s_total"].astype(np.float64)
    return np.divide(tot, cov, out=np.zeros_like(tot), where=cov > 0)


def mean_af(moments: dict, n: int) -> np.ndarray:
    """[L, 4] mean over the n cells of the population of af', the per-cell allele frequency
    with the low-coverage cells (pass 1's n_low, when stabilising) set to the bulk mean."""
    if n <= 0:
        return np.zeros_like(moments["s_af"])
    low = moments["n_low"].astype(np.float64)[:, None]
    return (moments["s_af"] + low * bulk_mean(moments)) / float(n)


def variance(moments: dict, dev2: np.ndarray, n: int) -> np.ndarray:
    """[L, 4] sample variance (n - 1) of af' over the population: pass 2's squared
    deviations of the cells that are not low, plus the low cells' (all at the bulk mean)."""
    if n < 2:
        return np.zeros_like(dev2)
    low = moments["n_low"].astype(np.float64)[:, None]
    d = bulk_mean(moments) - mean_af(moments, n)
    return (np.asarray(dev2, np.float64) + low * d * d) / float(n - 1)


def strand_correlation(m: int, sf: int, sr: int, sff: int, srr: int, sfr: int) -> float:
    """Pearson correlation of (f, r) over the m cells with f > 0, from their exact integer
    moments; 0 with fewer than 2 such cells or a zero variance (tested on the integers)."""
    m, sf, sr, sff, srr, sfr = int(m), int(sf), int(sr), int(sff), int(srr), int(sfr)
    if m < 2:
        return 0.0
    vf = m * sff - sf * sf
    vr = m * srr - sr * sr
    if vf == 0 or vr == 0:
        return 0.0
    num = m * sfr - sf * sr
    return max(-1.0, min(1.0, num / (math.sqrt(vf) * math.sqrt(vr))))  # (|cor| <= 1 whatever the rounding)


@dataclass
class VariantTable:
    """The variants that pass, ordered by vmr descending (ties: position, then base)."""

    position: np.ndarray  # int64, 1-based
    base: np.ndarray  # int64, 0..3 = A, C, G, T (the alternative allele)
    ref: list[str]
    mean: np.ndarray
    vmr: np.ndarray
    variance: np.ndarray  # the sample variance vmr was made of (vmr = variance / mean)
    n_cells_detected: np.ndarray
    n_cells_conf_detected: np.ndarray
    strand_correlation: np.ndarray
    nucleotide: list[str] = field(default_factory=list)  # "ref>alt"
    variant: list[str] = field(default_factory=list)  # "<pos><ref>><alt>"

    def __len__(self) -> int:
        return int(self.position.shape[0])

    def pairs(self) -> list[tuple[int, int]]:
        """(0-based position, base) of each row: the variants argument of allele_freq."""
        return [(int(p) - 1, int(b)) for p, b in zip(self.position, self.base)]

    def h5_names(self) -> list[str]:
        """The variants as R names the matrix rows (">" replaced by "-")."""
        return [v.replace(">", "-") for v in self.variant]


def variant_table(moments: dict, dev2: np.ndarray, ref_alleles: list[str], n: int, min_cells: int = 0,
                  min_strand_cor: float = 0, min_vmr: float = 0) -> VariantTable:
    """The per-variant statistics of identify_variants from pass 1's moments and pass 2's
    squared deviations over a population of n cells. Rows with no depth, no alternative
    read, n < 2, n_cells_conf_detected < min_cells, strand_correlation < min_strand_cor or
    vmr <= min_vmr are dropped."""
    L = moments["s_cov"].shape[0]
    if len(ref_alleles) != L:
        raise InvalidInputError("one reference allele per position")
    mean = bulk_mean(moments)
    var = variance(moments, dev2, n)
    rows = []
    if n >= 2:
        ref_idx = np.array([BASES.find(r) for r in ref_alleles], np.int64)  # -1: "N"
        cand = (moments["s_total"] > 0) & (moments["s_cov"] > 0)[:, None]
        cand &= np.arange(4)[None, :] != ref_idx[:, None]
        cand &= moments["n_conf"] >= max(0, int(min_cells))
        with np.errstate(divide="ignore", invalid="ignore"):
            vmr_all = var / mean
        for p, b in np.argwhere(cand).tolist():
            vmr = float(vmr_all[p, b])
            if not vmr > min_vmr:
                continue
            cor = strand_correlation(*(moments[k][p, b] for k in ("m", "sf", "sr", "sff", "srr", "sfr")))
            if not cor >= min_strand_cor:
                continue
            rows.append((-vmr, p, b, cor))
    rows.sort(key=lambda t: t[:3])
    pos = np.array([t[1] for t in rows], np.int64)
    base = np.array([t[2] for t in rows], np.int64)
    ref = [ref_alleles[p] for p in pos.tolist()]
    tab = VariantTable(
        position=pos + 1, base=base, ref=ref, mean=mean[pos, base], vmr=np.array([-t[0] for t in rows], np.float64),
        variance=var[pos, base], n_cells_detected=moments["n_det"][pos, base].astype(np.int64),
        n_cells_conf_detected=moments["n_conf"][pos, base].astype(np.int64),
        strand_correlation=np.array([t[3] for t in rows], np.float64))
    tab.nucleotide = [f"{r}>{BASES[b]}" for r, b in zip(ref, base.tolist())]
    tab.variant = [f"{p}{nt}" for p, nt in zip(tab.position.tolist(), tab.nucleotide)]
    return tab


# ---- the device passes over one or several contexts ---------------------------------

@dataclass
class VariantResult:
    table: VariantTable
    allele_freq: np.ndarray | None  # [n_variants, n population], fp64; None when not asked for
    moments: dict
    dev2: np.ndarray
    n: int
    seconds: dict


def run_variants(source, ref_alleles: list[str] | None = None, cells=None, min_cells: int = 0,
                 min_strand_cor: float = 0, min_vmr: float = 0, stabilize_variance: bool = False,
                 low_coverage_threshold: int = 10, min_coverage: int = 1, matrix: bool = True) -> VariantResult:
    """Pass 1 on every part, the host merge, pass 2, the table, and the heteroplasmy matrix
    of the passing variants (each part fills its own columns). `source`: an Engine after
    run(), or parts [(engine, lo, hi)] whose engines hold the cells [lo, hi) as their
    0..hi-lo. `cells`: the population as global cell indices (-1: an all-zero row), default
    every cell of the parts. `ref_alleles`: default ref_alleles() of the parts' summed tally."""
    from ..file_io.writers import ref_alleles as ref_of

    parts = DeviceParts(source)
    t0 = time.perf_counter()
    cells = parts.all_cells() if cells is None else np.asarray(cells, np.int64)
    n = int(cells.size)
    thr = int(low_coverage_threshold) if stabilize_variance else 0
    if ref_alleles is None:
        ref_alleles = ref_of(sum(e.fetch(dense=False).ref_tally.astype(np.int64) for e, _, _ in parts))
    calls = parts.split(cells)

    def pass1(d):
        return [parts[d][0].variant_moments(loc, thr) for _, loc in calls[d]]

    mom = merge_moments([m for ms in parts.map(pass1) for m in ms] or
                        [parts[0][0].variant_moments(np.zeros(0, np.int32), thr)])
    t1 = time.perf_counter()
    mu = mean_af(mom, n)

    def pass2(d):
        return [parts[d][0].variant_dev2(mu, loc, thr) for _, loc in calls[d]]

    dev2 = np.zeros_like(mu)
    for ds in parts.map(pass2):
        for x in ds:
            dev2 += x
    t2 = time.perf_counter()
    table = variant_table(mom, dev2, ref_alleles, n, min_cells, min_strand_cor, min_vmr)
    t3 = time.perf_counter()
    af = None
    if matrix:
        af = np.zeros((len(table), n), np.float64)
        if len(table) and n:
            pairs = table.pairs()

            def gather(d):
                return [(ix, parts[d][0].allele_freq(pairs, loc, min_coverage)) for ix, loc in calls[d]]

            for got in parts.map(gather):
                for ix, block in got:
                    af[:, ix] = block
    t4 = time.perf_counter()
    return VariantResult(table, af, mom, dev2, n,
                         {"pass1": t1 - t0, "pass2": t2 - t1, "table": t3 - t2, "gather": t4 - t3, "total": t4 - t0})


def identify_variants(source, ref_alleles: list[str] | None = None, cells=None, min_cells: int = 0,
                      min_strand_cor: float = 0, min_vmr: float = 0, stabilize_variance: bool = False,
                      low_coverage_threshold: int = 10) -> VariantTable:
    """R's identify_variants on the device rows: `source` is an Engine after run(), parts
    [(engine, lo, hi)], or a CellProcessor whose last run had enable_variants (its table is
    returned). R's defaults (no filtering); mgatk's customary thresholds are min_cells=5,
    min_strand_cor=0.65, min_vmr=0.01."""
    if hasattr(source, "last_result") and hasattr(source, "enable_variants"):
        res = source.last_result
        if res is None or res.variants is None:
            raise InvalidInputError("identify_variants: the processor's last run did not call variants "
                                    "(enable_variants before the run)")
        return res.variants
    return run_variants(source, ref_alleles, cells, min_cells, min_strand_cor, min_vmr, stabilize_variance,
                        low_coverage_threshold, matrix=False).table


# ---- the matrix as the analyses take it ----------------------------------------------

def heteroplasmy_matrix(result_or_matrix, barcodes=None, table=None):
    """(af, table, rows) for the analyses of the heteroplasmy matrix (a VariantResult, or the matrix itself): af
    [n_variants, n_cells] contiguous fp64 (None: 0 x 0), `table` or the result's own, `barcodes` and `table` (the
    column and row names), when given, checked against its shape; rows: its rows in genomic order, or None.

    Item numbers. Cells are numbered in the matrix's column order (the run's population). With a variant table,
    variants are numbered in genomic order (position, then base A, C, G, T), not in the table's vmr order, and
    the cells' features are taken in that order too: vmr carries a rounding that depends on how the cells were
    split over device contexts, so its order can differ in the last place between two runs on the same reads,
    ties between equal rows go to the lower item, and a sum's order fixes a distance's last bits. In genomic
    order the same reads give the same files however they were sharded. In R,
    ``labels = rownames(allele_freq_mat)[order(position, match(base, c("A", "C", "G", "T")))]``."""
    af = getattr(result_or_matrix, "allele_freq", result_or_matrix)
    if table is None:
        table = getattr(result_or_matrix, "table", None)
    af = np.ascontiguousarray(np.zeros((0, 0)) if af is None else af, np.float64)
    if af.ndim != 2:
        raise InvalidInputError("the heteroplasmy matrix is [n_variants, n_cells]")
    if barcodes is not None and len(barcodes) != af.shape[1]:
        raise InvalidInputError(f"{len(barcodes)} barcodes for {af.shape[1]} cells")
    if table is not None and len(table) != af.shape[0]:
        raise InvalidInputError(f"{len(table)} variants in the table for {af.shape[0]} rows")
    genomic = hasattr(table, "position") and hasattr(table, "base")
    return af, table, np.lexsort((np.asarray(table.base), np.asarray(table.position))) if genomic else None


# ---- output files --------------------------------------------------------------------

def variants_dir(output_dir) -> Path:
    """The run's variants/ directory, made if missing."""
    vdir = Path(output_dir) / "variants"
    vdir.mkdir(parents=True, exist_ok=True)
    return vdir


def write_variant_stats(table: VariantTable, path) -> None:
    """variant_stats.tsv: a header and one line per variant, floats as repr."""
    with open(path, "w") as fh:
        fh.write("\t".join(TSV_COLUMNS) + "\n")
        for i in range(len(table)):
            fh.write("\t".join([str(int(table.position[i])), table.nucleotide[i], table.variant[i],
                                repr(float(table.mean[i])), repr(float(table.vmr[i])),
                                str(int(table.n_cells_detected[i])), str(int(table.n_cells_conf_detected[i])),
                                repr(float(table.strand_correlation[i]))]) + "\n")


def read_variant_stats(path) -> dict:
    """variant_stats.tsv back as {column: list} (ints, strings and floats as written)."""
    kinds = {"position": int, "n_cells_detected": int, "n_cells_conf_detected": int, "mean": float, "vmr": float,
             "strand_correlation": float}
    with open(path) as fh:
        cols = fh.readline().rstrip("\n").split("\t")
        out = {c: [] for c in cols}
        for line in fh:
            for c, v in zip(cols, line.rstrip("\n").split("\t")):
                out[c].append(kinds.get(c, str)(v))
    return out


def write_allele_freq_h5(table: VariantTable, af: np.ndarray, barcodes: list[str], path, h5=None) -> None:
    """allele_freq.h5: allele_freq f64 [n_variants][n_barcodes] (gzip 4), variant and barcode names."""
    if h5 is None:
        from ..file_io.writers import _h5py

        h5 = _h5py()
    af = np.ascontiguousarray(af, np.float64)
    nv, nb = af.shape
    with h5.File(str(path), "w") as f:
        f.create_dataset("allele_freq", data=af, chunks=(min(nv, 100), min(nb, 1000)), compression="gzip",
                         compression_opts=4)
        f.create_dataset("variant", data=np.array(table.h5_names(), dtype="S"))
        f.create_dataset("barcode", data=np.array(list(barcodes), dtype="S"))


def write_allele_freq_txt(table: VariantTable, af: np.ndarray, barcodes: list[str], path) -> None:
    """output.allele_freq.txt.gz: "variant,barcode,af" for af > 0, variants in table order,
    barcodes in whitelist order."""
    # (no name and no time in the gzip header: the same matrix gives the same bytes)
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as fh:
        for v, name in enumerate(table.variant):
            row = af[v]
            fh.write("".join(f"{name},{barcodes[j]},{float(row[j])!r}\n"
                             for j in np.flatnonzero(row > 0).tolist()).encode())


def write_variant_outputs(table: VariantTable, af: np.ndarray | None, barcodes: list[str], output_dir,
                          output_format: str) -> Path:
    """The run's variants/ directory: variant_stats.tsv always, and the matrix (allele_freq.h5
    for hdf5 output, output.allele_freq.txt.gz otherwise) unless the table is empty."""
    vdir = variants_dir(output_dir)
    write_variant_stats(table, vdir / "variant_stats.tsv")
    if len(table) and af is not None:
        if output_format == "hdf5":
            write_allele_freq_h5(table, af, barcodes, vdir / "allele_freq.h5")
        else:
            write_allele_freq_txt(table, af, barcodes, vdir / "output.allele_freq.txt.gz")
    return vdir
