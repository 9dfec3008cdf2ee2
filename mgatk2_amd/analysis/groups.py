"""Pseudobulk counts and marker variants per cell group, from the engine's count rows.

A group is any labelling of the cells: the clones or clonotypes of an earlier run
(``variants/cell_clones.tsv``, ``variants/cell_clonotypes.tsv``), cell types, donors, samples.
Per group the device returns, at all L x 4 (position, base) pairs, the exact sums of the fwd and
rev counts and of the filtered depth, and the cells that carry the base (``Engine.group_moments``,
mgp_groups.hip, one sweep for every group). Everything here is host numpy over those integers:
every floating-point column is one fp64 division of exact sums, so the files are the same bytes
however the cells were split over device contexts.

Marker variants. For group g and (p, b) with b != the reference allele (an "N" position is a
candidate for all four bases): ``alt_in = fwd + rev``, ``af_in = alt_in / cov_in`` and
``af_rest = (alt_all - alt_in) / (cov_all - cov_in)`` over the rest of the population (0 where a
denominator is 0). A variant is kept where ``n_conf >= min_cells``, ``af_in >= min_af`` and
``af_in > af_rest``. The thresholds (2 cells, 0.01) are this project's choice: mgatk defines
none. The population-wide variant filter cannot see a small group's private variants (a variant
of a 4-cell clone never reaches ``--variant-min-cells 5``); the count rows can.

A whitelist with duplicate barcodes is not supported (one label per barcode).
"""

from __future__ import annotations

import gzip
import logging
import time
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from ..engine import GROUP_FIELDS
from ..exceptions import InvalidInputError
from ..shard import DeviceParts

logger = logging.getLogger(__name__)

BASES = "ACGT"
NONE_NAME = "(none)"  # the last line of groups.tsv: the population's unlabelled cells
GROUP_COLUMNS = ("group", "n_cells", "n_cells_with_rows", "total_depth", "mean_depth")
MARKER_COLUMNS = ("group", "position", "nucleotide", "variant", "n_cells", "n_cells_detected", "n_cells_conf_detected",
                  "alt_fwd", "alt_rev", "depth", "heteroplasmy", "heteroplasmy_rest", "called")
H5_PLANES = tuple(f"{b}_{s}" for b in BASES for s in ("fwd", "rev"))


def check_group_min_cells(min_cells) -> int:
    """`min_cells` of the marker variants as an int >= 0."""
    if int(min_cells) != min_cells or int(min_cells) < 0:
        raise InvalidInputError(f"group_min_cells must be an integer >= 0, got {min_cells}")
    return int(min_cells)


def check_group_min_af(min_af) -> float:
    """`min_af` of the marker variants as a float, 0 <= min_af <= 1 (a NaN is refused)."""
    min_af = float(min_af)
    if not 0.0 <= min_af <= 1.0:
        raise InvalidInputError(f"group_min_af must be in [0, 1], got {min_af}")
    return min_af


# ---- the groups file and the labels ------------------------------------------------------

def read_groups(path) -> dict[str, str]:
    """{barcode: group} of a groups file: two tab-separated columns, barcode and group, an optional header
    line whose first field is "barcode", further columns and blank lines ignored, .gz accepted
    (variants/cell_clonotypes.tsv and cell_clones.tsv as written). A barcode listed with two different
    groups is refused."""
    path = Path(path)
    if not path.exists():
        raise InvalidInputError(f"Groups file not found: {path}")
    mapping: dict[str, str] = {}
    with (gzip.open(path, "rt") if path.name.endswith(".gz") else open(path)) as fh:
        for i, line in enumerate(fh):
            f = line.rstrip("\r\n").split("\t")
            if not line.strip() or (i == 0 and f[0] == "barcode"):
                continue
            if len(f) < 2 or not f[0] or not f[1]:
                raise InvalidInputError(f"{path}: line {i + 1} is not 'barcode<TAB>group'")
            if mapping.setdefault(f[0], f[1]) != f[1]:
                raise InvalidInputError(f"{path}: barcode {f[0]} is listed with two groups, {mapping[f[0]]} and {f[1]}")
    return mapping


def labels_for(names: list[str], mapping: dict) -> tuple[np.ndarray, list[str]]:
    """(labels int32 [len(names)], group_names): the group number of each of `names` (-1: not in the mapping)
    and the groups' names in number order: numerically when every name is a decimal integer, else by code
    point. Only groups with a barcode among `names` are numbered. Barcodes of the mapping that `names` does
    not hold are warned about; none matching is refused."""
    have = set(names)
    missing = sorted(b for b in mapping if b not in have)
    if missing:
        logger.warning("%d of %d barcodes of the groups are not among the cells: %s%s", len(missing), len(mapping),
                       ", ".join(missing[:5]), ", ..." if len(missing) > 5 else "")
    used = {str(mapping[b]) for b in names if b in mapping}
    if not used:
        raise InvalidInputError("No barcode of the groups matches a cell")
    numeric = all(g.isascii() and g.isdigit() for g in used)
    group_names = sorted(used, key=(lambda g: (int(g), g)) if numeric else None)
    number = {g: k for k, g in enumerate(group_names)}
    labels = np.array([number[str(mapping[b])] if b in mapping else -1 for b in names], np.int32)
    return labels, group_names


def resolve_groups(groups, names: list[str]) -> tuple[np.ndarray, list[str]]:
    """labels_for of `groups`, a groups file's path or a {barcode: group} mapping, over `names`."""
    mapping = groups if isinstance(groups, dict) else read_groups(groups)
    if len(set(names)) != len(names):
        raise InvalidInputError("groups: a whitelist with duplicate barcodes is not supported")
    return labels_for(list(names), mapping)


# ---- the device sweep over one or several contexts ---------------------------------------

def merge_group_moments(parts: list[dict]) -> dict:
    """The group moments of a population made of several device calls: integers, added."""
    out = {k: np.array(parts[0][k], copy=True) for k, _ in GROUP_FIELDS}
    for p in parts[1:]:
        for k, _ in GROUP_FIELDS:
            out[k] += p[k]
    return out


def run_groups(source, labels, n_groups: int, cells=None) -> tuple[dict, dict]:
    """(moments, totals) of the population `cells` (global cell indices, -1: an all-zero row; default every
    cell of the parts) whose entry k has the label labels[k] (0 .. n_groups - 1, or -1). `source`: an Engine
    after run(), or parts [(engine, lo, hi)]. moments: GROUP_FIELDS arrays [n_groups, L(, 4)]; totals: the
    same fields over the whole population ([L(, 4)]), unlabelled cells included: they are swept as one
    extra group. Every part sweeps its own cells (the parts concurrently) and the integers are added."""
    parts = DeviceParts(source)
    cells = parts.all_cells() if cells is None else np.asarray(cells, np.int64)
    labels = np.asarray(labels, np.int64)
    n_groups = int(n_groups)
    if labels.shape != cells.shape:
        raise InvalidInputError(f"run_groups: {labels.size} labels for {cells.size} cells")
    if n_groups < 1 or (labels.size and (labels.min() < -1 or labels.max() >= n_groups)):
        raise InvalidInputError("run_groups: group label out of range")
    with_rest = np.where(labels < 0, n_groups, labels).astype(np.int32)
    calls = parts.split(cells)

    def sweep(d):
        return [parts[d][0].group_moments(with_rest[ix], n_groups + 1, loc) for ix, loc in calls[d]]

    got = [m for ms in parts.map(sweep) for m in ms]
    if not got:
        got = [parts[0][0].group_moments(np.zeros(0, np.int32), n_groups + 1, np.zeros(0, np.int32))]
    both = merge_group_moments(got)
    return ({k: both[k][:n_groups] for k, _ in GROUP_FIELDS},
            {k: both[k].sum(axis=0, dtype=both[k].dtype) for k, _ in GROUP_FIELDS})


# ---- the tables --------------------------------------------------------------------------

def _ratio(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    """num / den in fp64 of exact integers, 0 where den == 0."""
    num, den = np.broadcast_arrays(num.astype(np.float64), den.astype(np.float64))
    return np.divide(num, den, out=np.zeros(num.shape, np.float64), where=den > 0)


@dataclass
class GroupTable:
    """groups.tsv: one row per group, then the population's unlabelled cells as the last one."""

    group: list[str]
    n_cells: np.ndarray  # the population's entries with the label (all-zero rows included)
    n_cells_with_rows: np.ndarray  # those that have rows
    total_depth: np.ndarray  # the sum of the filtered depth over the positions
    mean_depth: np.ndarray  # total_depth / (n_cells x L), 0 for an empty group


def group_table(moments: dict, totals: dict, labels, cells, group_names: list[str]) -> GroupTable:
    """The group sizes and depths of run_groups' results for the population `cells` labelled `labels`."""
    labels, cells = np.asarray(labels, np.int64), np.asarray(cells, np.int64)
    G, L = moments["cov"].shape
    lab = np.where(labels < 0, G, labels)
    n_cells = np.bincount(lab, minlength=G + 1).astype(np.int64)
    with_rows = np.bincount(lab[cells >= 0], minlength=G + 1).astype(np.int64)
    depth = np.array([int(moments["cov"][g].sum(dtype=np.uint64)) for g in range(G)], np.int64)
    depth = np.append(depth, int(totals["cov"].sum(dtype=np.uint64)) - int(depth.sum()))
    return GroupTable(list(group_names) + [NONE_NAME], n_cells, with_rows, depth, _ratio(depth, n_cells * L))


@dataclass
class MarkerTable:
    """group_variants.tsv: the marker variants, by group, then heteroplasmy - heteroplasmy_rest descending,
    then position, then base."""

    group: np.ndarray  # int64, the group's number
    position: np.ndarray  # int64, 1-based
    base: np.ndarray  # int64, 0..3 = A, C, G, T
    ref: list[str]
    n_cells: np.ndarray
    n_cells_detected: np.ndarray
    n_cells_conf_detected: np.ndarray
    alt_fwd: np.ndarray
    alt_rev: np.ndarray
    depth: np.ndarray
    heteroplasmy: np.ndarray
    heteroplasmy_rest: np.ndarray
    called: np.ndarray  # 1: the run's own variant table holds the variant
    nucleotide: list[str] = field(default_factory=list)
    variant: list[str] = field(default_factory=list)

    def __len__(self) -> int:
        return int(self.position.shape[0])


def marker_table(moments: dict, totals: dict, ref_alleles: list[str], n_cells, min_cells: int = 2,
                 min_af: float = 0.01, called=None) -> MarkerTable:
    """The marker variants of every group (the module's note) from run_groups' moments and totals. n_cells:
    the groups' sizes; called: the (0-based position, base) pairs of the run's own variant table."""
    G, L = moments["cov"].shape
    if len(ref_alleles) != L:
        raise InvalidInputError("one reference allele per position")
    min_cells, min_af = check_group_min_cells(min_cells), check_group_min_af(min_af)
    called = set() if called is None else {(int(p), int(b)) for p, b in called}
    ref_idx = np.array([BASES.find(r) for r in ref_alleles], np.int64)  # -1: "N"
    alt_ok = np.arange(4)[None, :] != ref_idx[:, None]
    alt_all = totals["fwd"] + totals["rev"]
    rows = []
    for g in range(G):
        alt_in = moments["fwd"][g] + moments["rev"][g]
        cov_in = moments["cov"][g][:, None]
        af_in = _ratio(alt_in, cov_in)
        af_rest = _ratio(alt_all - alt_in, totals["cov"][:, None] - cov_in)
        keep = alt_ok & (moments["n_conf"][g] >= min_cells) & (af_in >= min_af) & (af_in > af_rest)
        found = [(g, -(float(af_in[p, b]) - float(af_rest[p, b])), p, b, float(af_in[p, b]), float(af_rest[p, b]))
                 for p, b in np.argwhere(keep).tolist()]
        rows.extend(sorted(found))
    gi = np.array([t[0] for t in rows], np.int64)
    pos = np.array([t[2] for t in rows], np.int64)
    base = np.array([t[3] for t in rows], np.int64)
    ref = [ref_alleles[p] for p in pos.tolist()]
    tab = MarkerTable(
        group=gi, position=pos + 1, base=base, ref=ref, n_cells=np.asarray(n_cells, np.int64)[gi],
        n_cells_detected=moments["n_det"][gi, pos, base].astype(np.int64),
        n_cells_conf_detected=moments["n_conf"][gi, pos, base].astype(np.int64),
        alt_fwd=moments["fwd"][gi, pos, base].astype(np.int64), alt_rev=moments["rev"][gi, pos, base].astype(np.int64),
        depth=moments["cov"][gi, pos].astype(np.int64), heteroplasmy=np.array([t[4] for t in rows], np.float64),
        heteroplasmy_rest=np.array([t[5] for t in rows], np.float64),
        called=np.array([int((p, b) in called) for p, b in zip(pos.tolist(), base.tolist())], np.int64))
    tab.nucleotide = [f"{r}>{BASES[b]}" for r, b in zip(ref, base.tolist())]
    tab.variant = [f"{p}{nt}" for p, nt in zip(tab.position.tolist(), tab.nucleotide)]
    return tab


def group_allele_freq(moments: dict, pairs) -> np.ndarray:
    """[n variants, n_groups] pseudobulk alt / depth of the (0-based position, base) `pairs`."""
    v = np.asarray(list(pairs), np.int64).reshape(-1, 2)
    alt = moments["fwd"][:, v[:, 0], v[:, 1]] + moments["rev"][:, v[:, 0], v[:, 1]]
    return _ratio(alt, moments["cov"][:, v[:, 0]]).T


@dataclass
class GroupResult:
    group_names: list[str]
    moments: dict  # GROUP_FIELDS arrays [n_groups, L(, 4)]
    totals: dict  # the same over the whole population [L(, 4)]
    table: GroupTable
    markers: MarkerTable
    ref_alleles: list[str]
    allele_freq: np.ndarray | None = None  # [n called variants, n_groups], with the run's variant table
    variant_names: list[str] | None = None
    seconds: dict = field(default_factory=dict)
    tests: object | None = None  # with the rank-sum tests on: the GroupTestTable (analysis/group_tests.py)


def group_result(source, labels, group_names: list[str], ref_alleles: list[str], cells=None, min_cells: int = 2,
                 min_af: float = 0.01, variants=None) -> GroupResult:
    """run_groups and the tables made of it. variants: the run's VariantTable, when it called variants (the
    markers' `called` column and group_allele_freq.tsv)."""
    t0 = time.perf_counter()
    parts = DeviceParts(source)
    cells = parts.all_cells() if cells is None else np.asarray(cells, np.int64)
    moments, totals = run_groups(parts, labels, len(group_names), cells)
    t1 = time.perf_counter()
    table = group_table(moments, totals, labels, cells, group_names)
    pairs = None if variants is None else variants.pairs()
    markers = marker_table(moments, totals, ref_alleles, table.n_cells[:-1], min_cells, min_af, pairs)
    res = GroupResult(list(group_names), moments, totals, table, markers, list(ref_alleles))
    if pairs:
        res.allele_freq, res.variant_names = group_allele_freq(moments, pairs), list(variants.variant)
    res.seconds = {"sweep": t1 - t0, "tables": time.perf_counter() - t1}
    return res


# ---- output files ------------------------------------------------------------------------

def write_group_table(table: GroupTable, path) -> None:
    """groups.tsv: a header and one line per group, the unlabelled cells last; floats as repr."""
    with open(path, "w") as fh:
        fh.write("\t".join(GROUP_COLUMNS) + "\n")
        for i, g in enumerate(table.group):
            fh.write("\t".join([g, str(int(table.n_cells[i])), str(int(table.n_cells_with_rows[i])),
                                str(int(table.total_depth[i])), repr(float(table.mean_depth[i]))]) + "\n")


def write_marker_table(markers: MarkerTable, group_names: list[str], path) -> None:
    """group_variants.tsv: a header and one line per marker variant (an empty table: the header only)."""
    with open(path, "w") as fh:
        fh.write("\t".join(MARKER_COLUMNS) + "\n")
        for i in range(len(markers)):
            fh.write("\t".join([group_names[int(markers.group[i])], str(int(markers.position[i])),
                                markers.nucleotide[i], markers.variant[i], str(int(markers.n_cells[i])),
                                str(int(markers.n_cells_detected[i])), str(int(markers.n_cells_conf_detected[i])),
                                str(int(markers.alt_fwd[i])), str(int(markers.alt_rev[i])), str(int(markers.depth[i])),
                                repr(float(markers.heteroplasmy[i])), repr(float(markers.heteroplasmy_rest[i])),
                                str(int(markers.called[i]))]) + "\n")


def read_tsv(path, kinds: dict | None = None) -> dict:
    """A written table back as {column: list}; kinds: {column: type}, default str."""
    kinds = kinds or {}
    with open(path) as fh:
        cols = fh.readline().rstrip("\n").split("\t")
        out = {c: [] for c in cols}
        for line in fh:
            for c, v in zip(cols, line.rstrip("\n").split("\t")):
                out[c].append(kinds.get(c, str)(v))
    return out


def write_group_counts_h5(moments: dict, group_names: list[str], n_cells, ref_alleles: list[str], path,
                          h5=None) -> None:
    """group_counts.h5: A_fwd .. T_rev and coverage as uint64 [L][n_groups] (the orientation of counts.h5,
    gzip 4), and group, n_cells, reference. uint64, not counts.h5's u16: a pseudobulk would saturate it."""
    if h5 is None:
        from ..file_io.writers import _h5py

        h5 = _h5py()
    G, L = moments["cov"].shape
    kw = dict(chunks=(min(L, 4096), min(G, 64)), compression="gzip", compression_opts=4)
    with h5.File(str(path), "w") as f:
        for b in range(4):
            for s in ("fwd", "rev"):
                f.create_dataset(f"{BASES[b]}_{s}", data=np.ascontiguousarray(moments[s][:, :, b].T, np.uint64), **kw)
        f.create_dataset("coverage", data=np.ascontiguousarray(moments["cov"].T, np.uint64), **kw)
        f.create_dataset("group", data=np.array(list(group_names), dtype="S"))
        f.create_dataset("n_cells", data=np.asarray(n_cells, np.int64))
        f.create_dataset("reference", data=np.array(list(ref_alleles), dtype="S"))


def write_group_allele_freq(af: np.ndarray, variant_names: list[str], group_names: list[str], path) -> None:
    """group_allele_freq.tsv: one line per called variant in variant_stats.tsv order, one column per group."""
    with open(path, "w") as fh:
        fh.write("\t".join(["variant"] + list(group_names)) + "\n")
        for name, row in zip(variant_names, af):
            fh.write("\t".join([name] + [repr(float(x)) for x in row]) + "\n")


def groups_dir(output_dir) -> Path:
    """The run's groups/ directory, made if missing."""
    gdir = Path(output_dir) / "groups"
    gdir.mkdir(parents=True, exist_ok=True)
    return gdir


def write_group_result(res: GroupResult, output_dir) -> Path:
    """The run's groups/ directory: groups.tsv, group_counts.h5, group_variants.tsv, when the run called
    variants and its table is not empty, group_allele_freq.tsv, and with the rank-sum tests on, group_tests.tsv."""
    gdir = groups_dir(output_dir)
    write_group_table(res.table, gdir / "groups.tsv")
    write_group_counts_h5(res.moments, res.group_names, res.table.n_cells[:-1], res.ref_alleles,
                          gdir / "group_counts.h5")
    write_marker_table(res.markers, res.group_names, gdir / "group_variants.tsv")
    if res.allele_freq is not None:
        write_group_allele_freq(res.allele_freq, res.variant_names, res.group_names, gdir / "group_allele_freq.tsv")
    if res.tests is not None:
        from .group_tests import write_group_tests

        write_group_tests(res.tests, res.group_names, gdir / "group_tests.tsv")
    return gdir
