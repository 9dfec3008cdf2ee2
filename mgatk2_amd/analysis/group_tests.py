"""The rank-sum test of each variant per cell group: which variants distinguish a group from the rest.

After ``FindClonotypes`` the vignette's user asks Seurat's ``FindAllMarkers`` on the alleles assay, whose
default test is the Wilcoxon rank-sum test of each feature, a group against the rest of the cells.
``groups/group_variants.tsv`` answers with thresholds on pooled counts; one deep cell can carry a group's
pseudobulk heteroplasmy, and nothing there says how surprising a difference is given the group's size. This
test ranks the cells.

Per variant the device sorts the heteroplasmy of all cells once and returns, per group, twice the sum of the
midranks of its cells (``r2``), its cells with a value > 0 (``pos``) and, per variant, the tie term
sum(t^3 - t) over the classes of equal values (``engine.rank_sums``, mgp_rank.hip). These are exact integers
that do not depend on the order of the adds, so everything here is one fixed formula in host numpy and the
file is the same bytes however the cells were split over device contexts.

With n1 the group's cells, n2 = n - n1 the rest (unlabelled cells are ranked and belong to every group's rest):

    U      = (r2 - n1 (n1 + 1)) / 2
    auc    = U / (n1 n2)
    sigma2 = n1 n2 / 12 * ((n + 1) - ties / (n (n - 1)))
    z      = (|U - n1 n2 / 2| - 1/2) / sigma         (= ((|2U - n1 n2| - 1) / 2) / sigma)
    p      = min(1, erfc(z / sqrt 2))                two-sided

the normal approximation with the tie correction and the continuity correction: R's
``wilcox.test(correct = TRUE)``, limma's ``rankSumTestWithCorrelation`` that Seurat calls, and scipy's
``mannwhitneyu(method="asymptotic", use_continuity=True)``. sigma = 0 (every value tied) gives z = 0 and p = 1.
The exact small-sample distribution is not used, whatever the group's size. ``p_adj`` is Seurat's Bonferroni:
min(1, p x the number of tested variants).
"""

from __future__ import annotations

import math
import time
from dataclasses import dataclass, field

import numpy as np

from ..exceptions import InvalidInputError
from ..shard import DeviceParts

BASES = "ACGT"
TEST_COLUMNS = ("group", "variant", "position", "nucleotide", "n_cells", "n_rest", "pct_in", "pct_rest", "u", "auc", "z",
                "p_value", "p_adj", "marker", "called")
TEST_KINDS = {"position": int, "n_cells": int, "n_rest": int, "pct_in": float, "pct_rest": float, "u": float,
              "auc": float, "z": float, "p_value": float, "p_adj": float, "marker": int, "called": int}
_erfc = np.frompyfunc(math.erfc, 1, 1)


def check_group_test_max_p(max_p) -> float:
    """`max_p` of the written lines as a float, 0 <= max_p <= 1 (a NaN is refused)."""
    max_p = float(max_p)
    if not 0.0 <= max_p <= 1.0:
        raise InvalidInputError(f"group_test_max_p must be in [0, 1], got {max_p}")
    return max_p


# ---- the formula ---------------------------------------------------------------------------

def rank_sum_table(r2, pos, ties, n_in, n: int, pos_total=None) -> dict:
    """The test of every (feature, group) from the device's integers (the module's note). r2, pos: [n_feat, G];
    ties: [n_feat]; n_in: [G], the groups' sizes; n: all ranked items (the groups need not cover them: the others
    are in every group's rest); pos_total: [n_feat], the items with a value > 0 (default: pos summed over G, right
    when the G groups cover the n items). A dict of [n_feat, G] arrays: `tested` (n1 > 0 and n2 > 0; the other
    pairs are left out: NaN in the float columns), u, auc, z, p_value, p_adj, pct_in, pct_rest, and n_in, n_rest
    [G]. The normal approximation only: no exact small-sample p-value."""
    r2 = np.asarray(r2, np.uint64)
    if r2.ndim != 2:
        raise InvalidInputError("rank_sum_table: r2 is [n_feat, n_groups]")
    nf, G = r2.shape
    pos = np.asarray(pos, np.uint32).reshape(nf, G).astype(np.float64)
    ties = np.asarray(ties, np.uint64).reshape(nf).astype(np.float64)  # (<= 2^60: rounded once, as scipy's sum)
    n = int(n)
    n1 = np.asarray(n_in, np.int64).reshape(G)
    if n1.size and (n1.min() < 0 or n1.max() > n):
        raise InvalidInputError("rank_sum_table: a group's size is outside 0 .. n")
    n2 = n - n1
    tested = np.broadcast_to((n1 > 0) & (n2 > 0), (nf, G)).copy()
    total = pos.sum(axis=1) if pos_total is None else np.asarray(pos_total, np.float64).reshape(nf)
    f1, f2 = n1.astype(np.float64), n2.astype(np.float64)
    nan = np.full((nf, G), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (r2.astype(np.float64) - f1 * (f1 + 1.0)) / 2.0  # (exact: r2 <= 2^41, halves)
        mu = f1 * f2 / 2.0
        auc = u / (f1 * f2)
        tie_part = ties / (float(n) * float(n - 1)) if n > 1 else np.zeros(nf)
        sigma = np.sqrt(f1 * f2 / 12.0 * ((n + 1) - tie_part[:, None]))
        z = np.where(sigma > 0, (np.abs(u - mu) - 0.5) / sigma, 0.0)
        p = np.minimum(1.0, _erfc(np.where(tested, z, 0.0) / math.sqrt(2.0)).astype(np.float64))
        pct_in = pos / f1
        pct_rest = (total[:, None] - pos) / f2
    out = {"tested": tested, "u": u, "auc": auc, "z": z, "p_value": p, "p_adj": np.minimum(1.0, p * float(nf)),
           "pct_in": pct_in, "pct_rest": pct_rest}
    for k in ("u", "auc", "z", "p_value", "p_adj", "pct_in", "pct_rest"):
        out[k] = np.where(tested, out[k], nan)
    out["n_in"], out["n_rest"] = n1, n2
    return out


def group_tests(matrix, labels, n_groups: int, device: int = 0) -> dict:
    """rank_sum_table of the [n_variants, n_cells] matrix over the groups 0 .. n_groups - 1; labels[c] is cell
    c's group, or -1 for an unlabelled cell, which is ranked and belongs to every group's rest (it goes to the
    device as the extra group `n_groups`). One device sort per variant serves every group."""
    from ..engine import rank_sums

    matrix = np.ascontiguousarray(matrix, np.float64)
    labels = np.asarray(labels, np.int64)
    n_groups = int(n_groups)
    if matrix.ndim != 2 or labels.shape != (matrix.shape[1],):
        raise InvalidInputError("group_tests: the matrix is [n_variants, n_cells], with one label per cell")
    if n_groups < 1 or (labels.size and (labels.min() < -1 or labels.max() >= n_groups)):
        raise InvalidInputError("group_tests: group label out of range")
    with_rest = np.where(labels < 0, n_groups, labels).astype(np.int32)
    got = rank_sums(matrix, with_rest, n_groups + 1, device=device)
    n_in = np.bincount(with_rest, minlength=n_groups + 1)[:n_groups]
    return rank_sum_table(got["r2"][:, :n_groups], got["pos"][:, :n_groups], got["ties"], n_in, labels.size,
                          pos_total=got["pos"].sum(axis=1, dtype=np.uint64))


# ---- the table -----------------------------------------------------------------------------

@dataclass
class GroupTestTable:
    """group_tests.tsv: the (group, variant) pairs higher in the group (U > n1 n2 / 2, Seurat's only.pos) with
    p_value <= max_p, by group, then p_value, then position, then base."""

    group: np.ndarray  # int64, the group's number
    position: np.ndarray  # int64, 1-based
    base: np.ndarray  # int64, 0..3 = A, C, G, T
    ref: list[str]
    n_cells: np.ndarray
    n_rest: np.ndarray
    pct_in: np.ndarray
    pct_rest: np.ndarray
    u: np.ndarray
    auc: np.ndarray
    z: np.ndarray
    p_value: np.ndarray
    p_adj: np.ndarray
    marker: np.ndarray  # 1: group_variants.tsv lists the pair
    called: np.ndarray  # 1: the run's own variant table holds the variant
    n_tested: int = 0  # the variants tested
    n_groups: int = 0
    max_p: float = 0.01
    nucleotide: list[str] = field(default_factory=list)
    variant: list[str] = field(default_factory=list)
    seconds: dict = field(default_factory=dict)

    def __len__(self) -> int:
        return int(self.position.shape[0])


def group_test_table(stats: dict | None, pairs, ref_alleles: list[str], n_groups: int, max_p: float = 0.01,
                     markers=None, called=None) -> GroupTestTable:
    """The lines of group_tests.tsv from group_tests' result over the variants `pairs` ((0-based position, base),
    one per row of the matrix; none: `stats` may be None and the table is empty). markers: (group, position,
    base) triples of the marker table; called: the pairs of the run's own variant table."""
    max_p = check_group_test_max_p(max_p)
    pairs = [(int(p), int(b)) for p, b in pairs]
    markers = set() if markers is None else {(int(g), int(p), int(b)) for g, p, b in markers}
    called = set() if called is None else {(int(p), int(b)) for p, b in called}
    rows = []
    if pairs:
        if stats["u"].shape != (len(pairs), int(n_groups)):
            raise InvalidInputError("group_test_table: one row of the tests per variant, one column per group")
        mu = stats["n_in"].astype(np.float64) * stats["n_rest"].astype(np.float64) / 2.0
        keep = stats["tested"] & (stats["u"] > mu[None, :]) & (stats["p_value"] <= max_p)
        for v, g in np.argwhere(keep).tolist():
            rows.append((g, float(stats["p_value"][v, g]), pairs[v][0], pairs[v][1], v))
        rows.sort()
    gi = np.array([t[0] for t in rows], np.int64)
    vi = np.array([t[4] for t in rows], np.int64)
    pos = np.array([t[2] for t in rows], np.int64)
    base = np.array([t[3] for t in rows], np.int64)
    ref = [ref_alleles[p] for p in pos.tolist()]

    def col(k):
        return stats[k][vi, gi].astype(np.float64) if rows else np.zeros(0, np.float64)

    tab = GroupTestTable(
        group=gi, position=pos + 1, base=base, ref=ref,
        n_cells=stats["n_in"][gi] if rows else np.zeros(0, np.int64),
        n_rest=stats["n_rest"][gi] if rows else np.zeros(0, np.int64),
        pct_in=col("pct_in"), pct_rest=col("pct_rest"), u=col("u"), auc=col("auc"), z=col("z"), p_value=col("p_value"),
        p_adj=col("p_adj"),
        marker=np.array([int((t[0], t[2], t[3]) in markers) for t in rows], np.int64),
        called=np.array([int((t[2], t[3]) in called) for t in rows], np.int64),
        n_tested=len(pairs), n_groups=int(n_groups), max_p=max_p)
    tab.nucleotide = [f"{r}>{BASES[b]}" for r, b in zip(ref, base.tolist())]
    tab.variant = [f"{p}{nt}" for p, nt in zip(tab.position.tolist(), tab.nucleotide)]
    return tab


# ---- the run's tested variants and their matrix --------------------------------------------------

def tested_pairs(markers, variants=None) -> list[tuple[int, int]]:
    """The variants a run tests, as (0-based position, base) in genomic order: the marker variants of every
    group (a MarkerTable), each once, united with the run's called variants (a VariantTable) when it has any."""
    pairs = {(int(p) - 1, int(b)) for p, b in zip(markers.position.tolist(), markers.base.tolist())}
    if variants is not None:
        pairs.update(variants.pairs())
    return sorted(pairs)


def heteroplasmy_matrix(source, pairs, cells, min_coverage: int = 1) -> np.ndarray:
    """[len(pairs), len(cells)] heteroplasmy of the variants `pairs` over the population `cells` (global cell
    indices, -1: an all-zero row, whose value is 0), made on the device as run_variants makes its own matrix:
    Engine.allele_freq per part, each part filling its own columns."""
    parts = DeviceParts(source)
    cells = np.asarray(cells, np.int64)
    af = np.zeros((len(pairs), cells.size), np.float64)
    if len(pairs) and cells.size:
        calls = parts.split(cells)

        def gather(d):
            return [(ix, parts[d][0].allele_freq(pairs, loc, min_coverage)) for ix, loc in calls[d]]

        for got in parts.map(gather):
            for ix, block in got:
                af[:, ix] = block
    return af


def run_group_tests(source, markers, labels, n_groups: int, ref_alleles: list[str], cells, variants=None,
                    min_coverage: int = 1, max_p: float = 0.01, device: int = 0) -> GroupTestTable:
    """The run's group_tests.tsv: tested_pairs, their heteroplasmy_matrix over the groups' population `cells`
    labelled `labels`, group_tests on `device`, and the table. No tested variant: an empty table."""
    t0 = time.perf_counter()
    pairs = tested_pairs(markers, variants)
    af = heteroplasmy_matrix(source, pairs, cells, min_coverage)
    t1 = time.perf_counter()
    stats = group_tests(af, labels, n_groups, device=device) if pairs else None
    t2 = time.perf_counter()
    triples = zip(markers.group.tolist(), (markers.position - 1).tolist(), markers.base.tolist())
    tab = group_test_table(stats, pairs, ref_alleles, n_groups, max_p, triples,
                           None if variants is None else variants.pairs())
    tab.seconds = {"matrix": t1 - t0, "sweep": t2 - t1, "table": time.perf_counter() - t2}
    return tab


# ---- output file ---------------------------------------------------------------------------

def write_group_tests(table: GroupTestTable, group_names: list[str], path) -> None:
    """group_tests.tsv: a header and one line per kept (group, variant) pair (none: the header only); floats
    as repr."""
    with open(path, "w") as fh:
        fh.write("\t".join(TEST_COLUMNS) + "\n")
        for i in range(len(table)):
            fh.write("\t".join([group_names[int(table.group[i])], table.variant[i], str(int(table.position[i])),
                                table.nucleotide[i], str(int(table.n_cells[i])), str(int(table.n_rest[i])),
                                repr(float(table.pct_in[i])), repr(float(table.pct_rest[i])), repr(float(table.u[i])),
                                repr(float(table.auc[i])), repr(float(table.z[i])), repr(float(table.p_value[i])),
                                repr(float(table.p_adj[i])), str(int(table.marker[i])), str(int(table.called[i]))])
                     + "\n")


def read_group_tests(path) -> dict:
    """A written group_tests.tsv back as {column: list}, the numbers as numbers."""
    from .groups import read_tsv

    return read_tsv(path, TEST_KINDS)
