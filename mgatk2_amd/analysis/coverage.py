"""Coverage QC from the engine's count rows: cell and position tables, the cell filter and
the recomputed reference.

The front half of the workflow mgatk users run on ``counts.h5`` (R/mgatk2_functions.R:138-280),
in the vignette's order: ``calculate_cell_coverage_stats``, ``filter_cells_by_coverage``,
``recompute_reference_alleles``, then ``calculate_position_coverage_stats``,
``calculate_strand_coverage_stats`` and ``calculate_transposition_stats`` on the kept cells.
The device makes the integers (``Engine.cell_coverage`` / ``position_coverage`` /
``position_depth_hist`` / ``position_depth_next``, mgp_qc.hip) from the rows that are still
in HBM when a run ends; everything here is host arithmetic on them.

A population is a list of cell indices (-1: an all-zero row, duplicates allowed), as for the
variants. ``d`` is the filtered depth, ``f_b`` / ``r_b`` the fwd / rev counts of base b,
``t_f`` / ``t_r`` the Tn5 cuts; the engine's exact values (counts.h5 stores min(v, 65535)).

Floating point: every fp column is made here from exact integers. A mean is one division of
Python integers (correctly rounded); the sample variance is
(n * sum(d^2) - sum(d)^2) / (n * (n - 1)) evaluated in Python integers and divided once,
never an fp sum(x^2) - sum(x)^2 / n. Where the mean is 0 the cv is NaN, as in R; with fewer
than two values the sd and the cv are NaN; an empty population gives empty or NaN tables.

The recomputed reference is ``file_io.writers.ref_alleles`` of the kept cells' tallies: the
first maximum in A, C, G, T order, "N" where a position has no read. R's ``which.max`` says
"A" there; no variant row can result at such a position either way.
"""

from __future__ import annotations

import math
import time
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from ..exceptions import InvalidInputError
from ..shard import DeviceParts

NAN = float("nan")
NONE_NEXT = 0xFFFFFFFF  # position_depth_next: no depth above v

CELL_COLUMNS = ("mean_coverage", "median_coverage", "max_coverage", "coverage_cv", "positions_covered",
                "positions_10x", "positions_50x", "coverage_breadth")
POSITION_COLUMNS = ("position", "mean_coverage", "median_coverage", "max_coverage", "coverage_cv", "cells_covered",
                    "cells_10x", "cells_50x", "coverage_dropout")
STRAND_COLUMNS = ("position", "mean_fwd_coverage", "mean_rev_coverage", "total_coverage", "strand_balance",
                  "strand_imbalance")
TRANSPOSITION_COLUMNS = ("position", "tn5_cuts_total", "tn5_cuts_fwd", "tn5_cuts_rev", "total_bases",
                         "tn5_frequency", "cells_with_tn5_cuts", "mean_tn5_cuts_per_cell", "strand_bias")
INT_COLUMNS = frozenset(("position", "max_coverage", "positions_covered", "positions_10x", "positions_50x",
                         "cells_covered", "cells_10x", "cells_50x", "tn5_cuts_total", "tn5_cuts_fwd", "tn5_cuts_rev",
                         "total_bases", "cells_with_tn5_cuts"))


# ---- exact integers -> fp columns --------------------------------------------------------

def _div(a: int, b: int) -> float:
    return a / b if b else NAN


def _mean_cv(s: int, s2: int, n: int) -> tuple[float, float]:
    """(mean, sd / mean) of n values with sum s and sum of squares s2 (sample sd, n - 1)."""
    s, s2, n = int(s), int(s2), int(n)
    mean = _div(s, n)
    if n < 2 or s == 0:
        return mean, NAN
    var = (n * s2 - s * s) / (n * (n - 1))
    return mean, math.sqrt(var) / mean


def _ints(a) -> list[int]:
    return np.asarray(a).tolist()


def cell_coverage_stats(cov: dict, L: int) -> dict:
    """calculate_cell_coverage_stats: one row per population cell, over all L positions, from
    Engine.cell_coverage's integers. Columns CELL_COLUMNS."""
    L = int(L)
    n = int(np.asarray(cov["s_depth"]).shape[0])
    mc = [_mean_cv(s, s2, L) for s, s2 in zip(_ints(cov["s_depth"]), _ints(cov["s_depth2"]))]
    covered = np.asarray(cov["n_covered"], np.int64)
    return {
        "mean_coverage": np.array([m for m, _ in mc], np.float64).reshape(n),
        "median_coverage": (np.asarray(cov["mid_lo"], np.float64) + np.asarray(cov["mid_hi"], np.float64)) / 2.0,
        "max_coverage": np.asarray(cov["max_depth"], np.int64),
        "coverage_cv": np.array([c for _, c in mc], np.float64).reshape(n),
        "positions_covered": covered,
        "positions_10x": np.asarray(cov["n_10x"], np.int64),
        "positions_50x": np.asarray(cov["n_50x"], np.int64),
        "coverage_breadth": covered.astype(np.float64) / float(L) if L else np.full(n, NAN),
    }


def _positions(L: int) -> np.ndarray:
    return np.arange(1, L + 1, dtype=np.int64)


def position_coverage_stats(pos: dict, mid_lo, mid_hi, n: int) -> dict:
    """calculate_position_coverage_stats: one row per position over the n population cells,
    from Engine.position_coverage's integers and the two middle order statistics
    (position_medians). Columns POSITION_COLUMNS."""
    n = int(n)
    L = int(np.asarray(pos["s_depth"]).shape[0])
    mc = [_mean_cv(s, s2, n) for s, s2 in zip(_ints(pos["s_depth"]), _ints(pos["s_depth2"]))]
    covered = np.asarray(pos["n_covered"], np.int64)
    if n:
        median = (np.asarray(mid_lo, np.float64) + np.asarray(mid_hi, np.float64)) / 2.0
        dropout = (n - covered).astype(np.float64) / float(n)
    else:
        median = dropout = np.full(L, NAN)
    return {
        "position": _positions(L),
        "mean_coverage": np.array([m for m, _ in mc], np.float64).reshape(L),
        "median_coverage": median,
        "max_coverage": np.asarray(pos["max_depth"], np.int64),
        "coverage_cv": np.array([c for _, c in mc], np.float64).reshape(L),
        "cells_covered": covered,
        "cells_10x": np.asarray(pos["n_10x"], np.int64),
        "cells_50x": np.asarray(pos["n_50x"], np.int64),
        "coverage_dropout": dropout,
    }


def strand_coverage_stats(pos: dict, n: int) -> dict:
    """calculate_strand_coverage_stats. Columns STRAND_COLUMNS."""
    n = int(n)
    L = int(np.asarray(pos["s_depth"]).shape[0])
    fwd = np.array([_div(v, n) for v in _ints(pos["s_fwd"])], np.float64).reshape(L)
    rev = np.array([_div(v, n) for v in _ints(pos["s_rev"])], np.float64).reshape(L)
    tot = np.array([_div(v, n) for v in _ints(pos["s_depth"])], np.float64).reshape(L)
    return {
        "position": _positions(L),
        "mean_fwd_coverage": fwd,
        "mean_rev_coverage": rev,
        "total_coverage": tot,
        "strand_balance": fwd / np.maximum(tot, 1.0),
        "strand_imbalance": np.abs(fwd - rev),
    }


def transposition_stats(pos: dict, n: int) -> dict:
    """calculate_transposition_stats. Columns TRANSPOSITION_COLUMNS."""
    n = int(n)
    L = int(np.asarray(pos["s_depth"]).shape[0])
    tf, tr, sd = _ints(pos["s_tn5_fwd"]), _ints(pos["s_tn5_rev"]), _ints(pos["s_depth"])
    total = [a + b for a, b in zip(tf, tr)]
    return {
        "position": _positions(L),
        "tn5_cuts_total": np.array(total, np.int64).reshape(L),
        "tn5_cuts_fwd": np.array(tf, np.int64).reshape(L),
        "tn5_cuts_rev": np.array(tr, np.int64).reshape(L),
        "total_bases": np.array(sd, np.int64).reshape(L),
        "tn5_frequency": np.array([t / d if d else 0.0 for t, d in zip(total, sd)], np.float64).reshape(L),
        "cells_with_tn5_cuts": np.asarray(pos["n_tn5"], np.int64),
        "mean_tn5_cuts_per_cell": np.array([_div(t, n) for t in total], np.float64).reshape(L),
        "strand_bias": np.array([abs(a - b) / max(a + b, 1) for a, b in zip(tf, tr)], np.float64).reshape(L),
    }


def filter_cells_by_coverage(cell_table: dict, min_mean_coverage: float = 10, min_coverage_breadth: float = 0.5
                             ) -> np.ndarray:
    """filter_cells_by_coverage: the kept mask, mean_coverage >= min_mean_coverage and
    coverage_breadth >= min_coverage_breadth (both inclusive; with both at 0 every cell of the
    population is kept, zero rows included)."""
    return ((np.asarray(cell_table["mean_coverage"]) >= float(min_mean_coverage)) &
            (np.asarray(cell_table["coverage_breadth"]) >= float(min_coverage_breadth)))


def recompute_reference_alleles(tally) -> list[str]:
    """recompute_reference_alleles from the kept cells' per-position tallies [L, 4] (sum over
    cells of f_b + r_b): the first maximum in A, C, G, T order, "N" where all are zero."""
    from ..file_io.writers import ref_alleles

    return ref_alleles(np.asarray(tally).astype(np.int64))


# ---- the median over cells ---------------------------------------------------------------

def position_medians(hist_fn, next_fn, max_depth, n: int) -> tuple[np.ndarray, np.ndarray]:
    """The two middle order statistics (ranks (n - 1) // 2 and n // 2) of every position's n
    depths, by a radix select over the cells from the most significant byte the largest depth
    makes necessary. hist_fn(shift, prefix) -> [L, 256] counts of the population's cells with
    d >> (shift + 8) == prefix[p] by (d >> shift) & 255 (the sum over every part and call);
    next_fn(v) -> (cells with d <= v[p], the smallest d > v[p] or NONE_NEXT), likewise merged.
    next_fn is called only when a position's upper middle is not its lower middle."""
    max_depth = np.asarray(max_depth, np.uint32)
    L, n = int(max_depth.shape[0]), int(n)
    if n <= 0 or L == 0:
        return np.zeros(L, np.uint32), np.zeros(L, np.uint32)
    top = int(max_depth.max())
    shift = 24 if top >> 24 else 16 if top >> 16 else 8 if top >> 8 else 0
    k_lo, k_hi = (n - 1) // 2, n // 2
    prefix = np.zeros(L, np.uint32)
    rank = np.full(L, k_lo, np.int64)  # the rank among the cells that share the prefix
    below = np.zeros(L, np.int64)      # cells under the prefix's range
    at = np.zeros(L, np.int64)
    rows = np.arange(L)
    while shift >= 0:
        h = np.asarray(hist_fn(shift, prefix), np.int64)
        cum = np.cumsum(h, axis=1)
        if np.any(cum[:, -1] <= rank):
            raise InvalidInputError("position_medians: the histograms do not cover the population")
        b = np.argmax(cum > rank[:, None], axis=1)
        at = h[rows, b]
        under = cum[rows, b] - at
        rank -= under
        below += under
        prefix = (prefix << np.uint32(8)) | b.astype(np.uint32)
        shift -= 8
    lo = prefix
    hi = lo.copy()
    need = below + at <= k_hi
    if need.any():
        n_le, nxt = next_fn(lo)
        if np.any(np.asarray(n_le, np.int64)[need] != (below + at)[need]):
            raise InvalidInputError("position_medians: the two device passes disagree")
        hi[need] = np.asarray(nxt, np.uint32)[need]
    return lo, hi


# ---- the device passes over one or several contexts --------------------------------------

@dataclass
class CoverageResult:
    cells: np.ndarray  # the population (global cell indices, -1: an all-zero row)
    kept: np.ndarray  # bool [n]: the filter's mask over the population
    cell: dict  # CELL_COLUMNS over the population
    position: dict  # the three position tables, over the kept cells
    strand: dict
    transposition: dict
    tally: np.ndarray  # [L, 4] the kept cells' tallies
    ref_alleles: list[str] | None  # the recomputed reference (recompute_reference), else None
    seconds: dict = field(default_factory=dict)

    @property
    def kept_cells(self) -> np.ndarray:
        return self.cells[self.kept]


POS_MAX_FIELDS = ("max_depth",)


def merge_position(parts: list[dict], L: int) -> dict:
    """The position integers of a population made of several device calls: sums added,
    max_depth combined by max."""
    from ..engine import POSITION_COVERAGE_FIELDS

    out = {k: np.zeros((L, 4) if k == "tally" else L, dt) for k, dt in POSITION_COVERAGE_FIELDS}
    for p in parts:
        for k, _ in POSITION_COVERAGE_FIELDS:
            out[k] = np.maximum(out[k], p[k]) if k in POS_MAX_FIELDS else out[k] + p[k]
    return out


def _position_pass(parts, cells: np.ndarray, L: int):
    """(merged position integers, mid_lo, mid_hi) of the population `cells` over the parts."""
    parts = DeviceParts(parts)
    calls = parts.split(cells)
    n = int(cells.size)
    if n == 0:
        z = np.zeros(L, np.uint32)
        return merge_position([], L), z, z

    def every(fn):  # fn(engine, local) for every call of every part, the devices concurrently
        got = parts.map(lambda d: [fn(parts[d][0], loc) for _, loc in calls[d]])
        return [x for g in got for x in g]

    pos = merge_position(every(lambda e, loc: e.position_coverage(loc)), L)

    def hist_fn(shift, prefix):
        return sum(h["hist"].astype(np.int64) for h in every(lambda e, loc: e.position_depth_hist(shift, prefix, loc)))

    def next_fn(v):
        got = every(lambda e, loc: e.position_depth_next(v, loc))
        n_le = sum(g["n_le"].astype(np.int64) for g in got)
        nxt = got[0]["next"]
        for g in got[1:]:
            nxt = np.minimum(nxt, g["next"])
        return n_le, nxt

    lo, hi = position_medians(hist_fn, next_fn, pos["max_depth"], n)
    return pos, lo, hi


def run_coverage(source, cells=None, min_mean_coverage: float = 0.0, min_coverage_breadth: float = 0.0,
                 recompute_reference: bool = False) -> CoverageResult:
    """The vignette's front half on the device rows: the cell table over the population, the
    filter, then the position, strand and transposition tables (and, with recompute_reference,
    the reference alleles) over the kept cells. `source`: an Engine after run(), or parts
    [(engine, lo, hi)] whose engines hold the cells [lo, hi) as their 0..hi-lo. `cells`: the
    population as global cell indices (-1: an all-zero row), default every cell of the parts.
    Calls are split at VARIANT_MAX_CELLS cells and the parts run concurrently; the host adds
    the integers, combines the max / min and puts the cell rows in population order."""
    from ..engine import CELL_COVERAGE_FIELDS

    parts = DeviceParts(source)
    L = int(parts[0][0].cfg.mito_len)
    t0 = time.perf_counter()
    cells = parts.all_cells() if cells is None else np.asarray(cells, np.int64).reshape(-1)
    n = int(cells.size)
    raw = {k: np.zeros(n, dt) for k, dt in CELL_COVERAGE_FIELDS}
    if n:
        calls = parts.split(cells)
        for got in parts.map(lambda d: [(ix, parts[d][0].cell_coverage(loc)) for ix, loc in calls[d]]):
            for ix, block in got:
                for k in raw:
                    raw[k][ix] = block[k]
    cell = cell_coverage_stats(raw, L)
    kept = filter_cells_by_coverage(cell, min_mean_coverage, min_coverage_breadth)
    t1 = time.perf_counter()
    pop = cells[kept]
    pos, lo, hi = _position_pass(parts, pop, L)
    t2 = time.perf_counter()
    m = int(pop.size)
    res = CoverageResult(cells=cells, kept=kept, cell=cell, position=position_coverage_stats(pos, lo, hi, m),
                         strand=strand_coverage_stats(pos, m), transposition=transposition_stats(pos, m),
                         tally=pos["tally"],
                         ref_alleles=recompute_reference_alleles(pos["tally"]) if recompute_reference else None)
    t3 = time.perf_counter()
    res.seconds = {"cells": t1 - t0, "positions": t2 - t1, "tables": t3 - t2, "total": t3 - t0}
    return res


# ---- output files ------------------------------------------------------------------------

def _fmt(col: str, v) -> str:
    return str(int(v)) if col in INT_COLUMNS else repr(float(v))


def write_table(table: dict, columns, path, lead: tuple[str, list[str]] | None = None,
                tail: tuple[str, list[str]] | None = None) -> None:
    """A tsv: a header and one line per row, ints as str and floats as repr; `lead` / `tail`:
    a string column in front / at the end."""
    n = int(np.asarray(table[columns[0]]).shape[0])
    cols = [np.asarray(table[c]).tolist() for c in columns]
    head = ([lead[0]] if lead else []) + list(columns) + ([tail[0]] if tail else [])
    with open(path, "w") as fh:
        fh.write("\t".join(head) + "\n")
        for i in range(n):
            row = ([lead[1][i]] if lead else []) + [_fmt(c, v[i]) for c, v in zip(columns, cols)]
            fh.write("\t".join(row + ([tail[1][i]] if tail else [])) + "\n")


def read_table(path) -> dict:
    """A coverage tsv back as {column: list} (ints, floats and strings as written)."""
    with open(path) as fh:
        cols = fh.readline().rstrip("\n").split("\t")
        out = {c: [] for c in cols}
        for line in fh:
            for c, v in zip(cols, line.rstrip("\n").split("\t")):
                out[c].append(int(v) if c in INT_COLUMNS else v if c in ("barcode", "kept", "reference",
                                                                         "recomputed") else float(v))
    return out


def write_coverage_outputs(res: CoverageResult, barcodes: list[str], output_dir,
                           run_ref_alleles: list[str] | None = None, tables: bool = True) -> Path:
    """The run's coverage/ directory: cell_coverage_stats.tsv (barcode, CELL_COLUMNS, kept;
    one line per population cell), position_coverage_stats.tsv, strand_coverage_stats.tsv and
    transposition_stats.tsv over the kept cells, and with a recomputed reference
    reference_alleles.tsv (position, the run's allele, the recomputed allele). tables=False:
    reference_alleles.tsv only."""
    cdir = Path(output_dir) / "coverage"
    cdir.mkdir(parents=True, exist_ok=True)
    if len(barcodes) != int(res.cells.size):
        raise InvalidInputError("write_coverage_outputs: one barcode per population cell")
    if tables:
        _write_tables(res, barcodes, cdir)
    if res.ref_alleles is not None:
        L = len(res.ref_alleles)
        run = list(run_ref_alleles) if run_ref_alleles is not None else ["N"] * L
        with open(cdir / "reference_alleles.tsv", "w") as fh:
            fh.write("position\treference\trecomputed\n")
            for p in range(L):
                fh.write(f"{p + 1}\t{run[p]}\t{res.ref_alleles[p]}\n")
    return cdir


def _write_tables(res: CoverageResult, barcodes: list[str], cdir: Path) -> None:
    write_table(res.cell, CELL_COLUMNS, cdir / "cell_coverage_stats.tsv", lead=("barcode", list(barcodes)),
                tail=("kept", ["TRUE" if k else "FALSE" for k in res.kept.tolist()]))
    write_table(res.position, POSITION_COLUMNS, cdir / "position_coverage_stats.tsv")
    write_table(res.strand, STRAND_COLUMNS, cdir / "strand_coverage_stats.tsv")
    write_table(res.transposition, TRANSPOSITION_COLUMNS, cdir / "transposition_stats.tsv")
