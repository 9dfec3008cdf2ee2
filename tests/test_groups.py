"""Pseudobulk counts and marker variants per cell group (analysis/groups.py), without a device: a numpy
oracle of the grouped sweep made from per-cell arrays, the marker table against a brute-force loop over the
cells, the groups file and the labels, the host merge over parts and over calls of 256 groups, the files,
the command line and the ABI. Every comparison is bit-equal. tests/test_gpu_groups.py runs the device
against the same oracle."""

from __future__ import annotations

import ctypes as C
import gzip
import logging
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_variants import _invoke, crafted_rows, per_cell, population, ref_of

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("mgp_group_moments_run", "mgp_rows_group_moments")
FIELDS = ("fwd", "rev", "cov", "n_det", "n_conf")


# ---- the oracle ------------------------------------------------------------------------------
def oracle_group_moments(counts, depth, cells, group, n_groups):
    """The grouped sweep from per-cell arrays: entry k of the population `cells` (None: every row) belongs to
    group[k] (-1: none). uint64 fwd, rev [G, L, 4] and cov [G, L], uint32 n_det, n_conf [G, L, 4]."""
    f, r, cov, _ = per_cell(*population(counts, depth, cells))
    group = np.asarray(group, np.int64)
    L = f.shape[1]
    out = {"fwd": np.zeros((n_groups, L, 4), np.uint64), "rev": np.zeros((n_groups, L, 4), np.uint64),
           "cov": np.zeros((n_groups, L), np.uint64), "n_det": np.zeros((n_groups, L, 4), np.uint32),
           "n_conf": np.zeros((n_groups, L, 4), np.uint32)}
    for g in range(n_groups):
        m = group == g
        out["fwd"][g], out["rev"][g], out["cov"][g] = f[m].sum(0), r[m].sum(0), cov[m].sum(0)
        out["n_det"][g] = ((f[m] + r[m]) > 0).sum(0)
        out["n_conf"][g] = ((f[m] >= 2) & (r[m] >= 2)).sum(0)
    return out


def oracle_totals(counts, depth, cells):
    n = np.asarray(depth).shape[0] if cells is None else len(cells)
    return {k: v[0] for k, v in oracle_group_moments(counts, depth, cells, np.zeros(n, np.int64), 1).items()}


def same(got, want, what=""):
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")


def oracle_markers(counts, depth, cells, group, n_groups, ref, min_cells, min_af):
    """The marker variants by a loop over groups, positions, bases and cells: {(g, p, b): row}."""
    f, r, cov, _ = per_cell(*population(counts, depth, cells))
    group = np.asarray(group, np.int64)
    n, L = cov.shape
    out = {}
    for g in range(n_groups):
        inside = [k for k in range(n) if group[k] == g]
        rest = [k for k in range(n) if group[k] != g]
        for p in range(L):
            cov_in, cov_rest = sum(int(cov[k, p]) for k in inside), sum(int(cov[k, p]) for k in rest)
            for b in range(4):
                if ref[p] == "ACGT"[b]:
                    continue
                af_, ar_ = sum(int(f[k, p, b]) for k in inside), sum(int(r[k, p, b]) for k in inside)
                alt_rest = sum(int(f[k, p, b] + r[k, p, b]) for k in rest)
                n_conf = sum(1 for k in inside if f[k, p, b] >= 2 and r[k, p, b] >= 2)
                af_in = float(af_ + ar_) / float(cov_in) if cov_in else 0.0
                af_rest = float(alt_rest) / float(cov_rest) if cov_rest else 0.0
                if n_conf >= min_cells and af_in >= min_af and af_in > af_rest:
                    out[(g, p, b)] = dict(n_cells=len(inside), n_conf=n_conf, alt_fwd=af_, alt_rev=ar_, depth=cov_in,
                                          n_det=sum(1 for k in inside if f[k, p, b] + r[k, p, b] > 0), af_in=af_in,
                                          af_rest=af_rest)
    return out


def check_markers(tab, want):
    keys = list(zip(tab.group.tolist(), (tab.position - 1).tolist(), tab.base.tolist()))
    assert sorted(keys) == sorted(want)
    for i, k in enumerate(keys):
        w = want[k]
        assert (int(tab.n_cells[i]), int(tab.n_cells_conf_detected[i]), int(tab.n_cells_detected[i]), int(tab.alt_fwd[i]),
                int(tab.alt_rev[i]), int(tab.depth[i])) == (w["n_cells"], w["n_conf"], w["n_det"], w["alt_fwd"],
                                                            w["alt_rev"], w["depth"]), k
        assert tab.heteroplasmy[i] == w["af_in"] and tab.heteroplasmy_rest[i] == w["af_rest"], k
    order = [(g, -(a - b), p, c) for (g, p, c), a, b in zip(keys, tab.heteroplasmy.tolist(),
                                                           tab.heteroplasmy_rest.tolist())]
    assert order == sorted(order)


# ---- the marker table ------------------------------------------------------------------------
@pytest.mark.parametrize("thresholds", [(2, 0.01), (0, 0.0), (1, 0.2)])
def test_marker_table_matches_the_brute_force(thresholds):
    from mgatk2_amd.analysis.groups import group_table, marker_table

    counts, depth = crafted_rows()
    rng = np.random.default_rng(3)
    cells = np.concatenate([rng.permutation(40), [-1, 7, -1, 7]]).astype(np.int64)
    group = rng.integers(-1, 5, cells.size)
    group[group == 3] = 2  # group 3 is empty
    ref = ref_of(counts)
    assert ref[20] == "N"
    mom = oracle_group_moments(counts, depth, cells, group, 5)
    tot = oracle_totals(counts, depth, cells)
    names = [str(g) for g in range(5)]
    gt = group_table(mom, tot, group, cells, names)
    assert gt.group == names + ["(none)"]
    for g in range(5):
        assert int(gt.n_cells[g]) == int((group == g).sum())
        assert int(gt.n_cells_with_rows[g]) == int(((group == g) & (cells >= 0)).sum())
        assert int(gt.total_depth[g]) == int(mom["cov"][g].sum())
        assert gt.mean_depth[g] == (float(gt.total_depth[g]) / float(gt.n_cells[g] * 300) if gt.n_cells[g] else 0.0)
    assert int(gt.n_cells[5]) == int((group < 0).sum()) and int(gt.n_cells[3]) == 0 and gt.mean_depth[3] == 0.0
    assert int(gt.total_depth.sum()) == int(tot["cov"].sum())
    tab = marker_table(mom, tot, ref, gt.n_cells[:-1], *thresholds)
    want = oracle_markers(counts, depth, cells, group, 5, ref, *thresholds)
    assert len(want) > 0
    check_markers(tab, want)
    assert not tab.called.any()
    some = [(int(p) - 1, int(b)) for p, b in zip(tab.position[:3], tab.base[:3])]
    called = marker_table(mom, tot, ref, gt.n_cells[:-1], *thresholds, called=some)
    assert [int(c) for c in called.called] == [int((int(p) - 1, int(b)) in some)
                                               for p, b in zip(called.position, called.base)]
    assert tab.variant[0] == f"{tab.position[0]}{tab.ref[0]}>{'ACGT'[tab.base[0]]}"


def _two_groups(rows):
    """counts, depth of cells with one position each: rows = [(group, ref fwd, ref rev, alt fwd, alt rev)],
    the reference A and the alternative C."""
    counts = np.zeros((len(rows), 1, 8), np.uint32)
    for k, (_, a, b, c, d) in enumerate(rows):
        counts[k, 0, :4] = (a, b, c, d)
    depth = counts.astype(np.int64).sum(axis=2).astype(np.uint32)
    group = np.array([r[0] for r in rows], np.int64)
    return counts, depth, group


def test_marker_thresholds_at_their_edges():
    from mgatk2_amd.analysis.groups import marker_table

    def markers(rows, ref="A", min_cells=2, min_af=0.25):
        counts, depth, group = _two_groups(rows)
        G = int(group.max()) + 1
        mom, tot = oracle_group_moments(counts, depth, None, group, G), oracle_totals(counts, depth, None)
        tab = marker_table(mom, tot, [ref], np.bincount(group[group >= 0], minlength=G), min_cells, min_af)
        return list(zip(tab.group.tolist(), tab.base.tolist(), tab.heteroplasmy.tolist(), tab.heteroplasmy_rest.tolist()))

    # group 0: two confident cells, af_in = 4 / 16 = 0.25 == min_af; the rest carries none: kept at the edges
    rows = [(0, 6, 6, 2, 2), (0, 6, 6, 2, 2), (1, 5, 5, 0, 0)]
    assert markers(rows) == [(0, 1, 0.25, 0.0)]
    assert markers(rows, min_cells=3) == [] and markers(rows, min_af=0.2500001) == []
    # one cell confident only (r = 1 in the other): n_conf = 1 < 2
    assert markers([(0, 6, 6, 2, 2), (0, 6, 5, 2, 1), (1, 5, 5, 0, 0)], min_af=0.0) == []
    # af_in == af_rest: excluded (strictly greater)
    assert markers([(0, 3, 3, 2, 2), (0, 3, 3, 2, 2), (1, 3, 3, 2, 2)], min_af=0.0) == []
    assert markers([(0, 3, 3, 2, 2), (0, 3, 3, 2, 2), (1, 3, 4, 2, 2)], min_af=0.0)[0][:2] == (0, 1)
    # the reference allele itself is no variant; at an "N" position all four bases are candidates
    assert markers(rows, ref="C", min_af=0.0) == []
    got = markers(rows, ref="N", min_cells=0, min_af=0.0)
    assert sorted((g, b) for g, b, _, _ in got) == [(0, 1), (1, 0)]
    # a group without coverage at the position: af_in = 0, never above the rest; min_af = 0 does not let it in
    assert markers([(0, 0, 0, 0, 0), (0, 0, 0, 0, 0), (1, 5, 5, 2, 2)], min_cells=0, min_af=0.0) == [(1, 1, 4 / 14, 0.0)]
    # a group equal to the whole population: the rest's denominator is 0, af_rest = 0
    assert markers([(0, 6, 6, 2, 2), (0, 6, 6, 2, 2)]) == [(0, 1, 0.25, 0.0)]


def test_threshold_checkers():
    from mgatk2_amd.analysis.groups import check_group_min_af, check_group_min_cells
    from mgatk2_amd.exceptions import InvalidInputError

    assert check_group_min_cells(0) == 0 and check_group_min_cells(7) == 7
    assert check_group_min_af(0) == 0.0 and check_group_min_af(1) == 1.0
    for bad in (-1, 1.5):
        with pytest.raises(InvalidInputError, match="group_min_cells"):
            check_group_min_cells(bad)
    for bad in (-0.1, 1.1, float("nan"), float("inf")):
        with pytest.raises(InvalidInputError, match="group_min_af"):
            check_group_min_af(bad)


# ---- the groups file and the labels ------------------------------------------------------------
def test_read_groups_takes_the_clone_and_clonotype_files(tmp_path):
    from types import SimpleNamespace

    from mgatk2_amd.analysis.clonotypes import write_cell_clonotypes
    from mgatk2_amd.analysis.clustering import write_cluster_outputs
    from mgatk2_amd.analysis.groups import read_groups

    barcodes = ["AAAC-1", "AAAG-1", "AAAT-1", "AACA-1"]
    labels = np.array([1, 0, 1, 2])
    write_cell_clonotypes(SimpleNamespace(result=SimpleNamespace(labels=labels)), barcodes, tmp_path / "cc.tsv")
    assert (tmp_path / "cc.tsv").read_text().startswith("barcode\tclonotype\n")
    assert read_groups(tmp_path / "cc.tsv") == dict(zip(barcodes, ["2", "1", "2", "3"]))
    tree = SimpleNamespace(n=1, merge=np.zeros((0, 2), np.int32), height=np.zeros(0), order=np.arange(1, 5))
    write_cluster_outputs(SimpleNamespace(variant_rows=None, cells=tree, variants=None, clones=labels + 1), barcodes,
                          ["v"], tmp_path)
    assert (tmp_path / "variants" / "cell_clones.tsv").read_text().startswith("barcode\tclone\n")
    assert read_groups(tmp_path / "variants" / "cell_clones.tsv") == dict(zip(barcodes, ["2", "1", "2", "3"]))


def test_read_groups_formats(tmp_path):
    from mgatk2_amd.analysis.groups import read_groups
    from mgatk2_amd.exceptions import InvalidInputError

    want = {"b1": "T cell", "b2": "B", "b3": "T cell"}
    (tmp_path / "plain.tsv").write_text("b1\tT cell\nb2\tB\n\nb3\tT cell\textra\tcolumns\n")
    assert read_groups(tmp_path / "plain.tsv") == want
    (tmp_path / "head.tsv").write_text("barcode\tcell_type\tscore\nb1\tT cell\t0.5\nb2\tB\t1\nb3\tT cell\t2\n")
    assert read_groups(tmp_path / "head.tsv") == want
    with gzip.open(tmp_path / "g.tsv.gz", "wt") as fh:
        fh.write("barcode\tgroup\nb1\tT cell\nb2\tB\nb3\tT cell\nb1\tT cell\n")  # (a repeat with the same group)
    assert read_groups(tmp_path / "g.tsv.gz") == want
    (tmp_path / "twice.tsv").write_text("b1\tx\nb2\ty\nb1\tz\n")
    with pytest.raises(InvalidInputError, match="barcode b1 is listed with two groups"):
        read_groups(tmp_path / "twice.tsv")
    (tmp_path / "one.tsv").write_text("b1\n")
    with pytest.raises(InvalidInputError, match="line 1"):
        read_groups(tmp_path / "one.tsv")
    with pytest.raises(InvalidInputError, match="not found"):
        read_groups(tmp_path / "missing.tsv")


def test_labels_for(caplog):
    from mgatk2_amd.analysis.groups import labels_for, resolve_groups
    from mgatk2_amd.exceptions import InvalidInputError

    names = ["c0", "c1", "c2", "c3", "c4"]
    labels, groups = labels_for(names, {"c0": "10", "c1": "9", "c3": "10", "c4": "2"})
    assert groups == ["2", "9", "10"] and labels.tolist() == [2, 1, -1, 2, 0] and labels.dtype == np.int32  # numeric
    labels, groups = labels_for(names, {"c0": "10", "c1": "9", "c3": "b", "c4": "B"})
    assert groups == ["10", "9", "B", "b"] and labels.tolist() == [0, 1, -1, 3, 2]  # code points
    unknown = {f"x{i}": "1" for i in range(7)}
    with caplog.at_level(logging.WARNING, logger="mgatk2_amd.analysis.groups"):
        labels, groups = labels_for(names, {"c2": "1", **unknown})
    assert labels.tolist() == [-1, -1, 0, -1, -1] and groups == ["1"]
    assert "7 of 8 barcodes" in caplog.text and "x0, x1, x2, x3, x4, ..." in caplog.text
    with pytest.raises(InvalidInputError, match="No barcode of the groups matches"):
        labels_for(names, unknown)
    with pytest.raises(InvalidInputError, match="duplicate barcodes"):
        resolve_groups({"c0": "1"}, ["c0", "c0"])


# ---- the host merge ------------------------------------------------------------------------------
class NumpyEngine:
    """Engine.group_moments of the rows [lo, hi) of (counts, depth), by the oracle."""

    def __init__(self, counts, depth, lo, hi):
        self.counts, self.depth, self.calls = counts[lo:hi], depth[lo:hi], []

    def group_moments(self, group, n_groups, cells=None, max_item_cells=0):
        self.calls.append(np.asarray(cells).copy())
        assert cells is None or (np.asarray(cells) < self.depth.shape[0]).all()
        return oracle_group_moments(self.counts, self.depth, cells, group, n_groups)


def test_run_groups_over_two_parts_equals_one():
    from mgatk2_amd.analysis.groups import run_groups

    counts, depth = crafted_rows()
    rng = np.random.default_rng(11)
    cells = np.concatenate([rng.permutation(40), [-1, 5, 5, -1]]).astype(np.int64)
    rng.shuffle(cells)
    labels = rng.integers(-1, 4, cells.size)
    one = [(NumpyEngine(counts, depth, 0, 40), 0, 40)]
    two = [(NumpyEngine(counts, depth, 0, 13), 0, 13), (NumpyEngine(counts, depth, 13, 40), 13, 40)]
    m1, t1 = run_groups(one, labels, 4, cells)
    m2, t2 = run_groups(two, labels, 4, cells)
    same(m1, oracle_group_moments(counts, depth, cells, labels, 4), "one part")
    same(m2, m1, "two parts")
    for k in FIELDS:
        np.testing.assert_array_equal(t1[k], oracle_totals(counts, depth, cells)[k], err_msg=k)
        assert t1[k].tobytes() == t2[k].tobytes() and t1[k].dtype == m1[k].dtype
    assert sum(c.size for c in two[0][0].calls + two[1][0].calls) == cells.size  # every entry swept once
    m0, t0 = run_groups(one, np.zeros(0, np.int64), 2, np.zeros(0, np.int64))  # an empty population
    assert m0["fwd"].shape == (2, 300, 4) and not any(v.any() for v in m0.values()) and not t0["cov"].any()


def test_more_than_256_groups_go_in_several_calls():
    """engine._group_calls against a stand-in for the library call: calls of at most 256 groups whose other
    labels are -1, reassembled in group order."""
    from mgatk2_amd import engine
    from mgatk2_amd.exceptions import InvalidInputError

    rng = np.random.default_rng(5)
    counts = rng.integers(0, 9, (50, 8, 8)).astype(np.uint32)
    depth = counts.sum(axis=2).astype(np.uint32)
    cells = rng.integers(-1, 50, 900).astype(np.int32)
    group = rng.integers(-1, 600, 900).astype(np.int32)
    ctype = {np.uint64: C.c_uint64, np.uint32: C.c_uint32}
    seen = []

    def call(job_ref, group_ptr, n_groups, max_item_cells, out_ref):
        job, out = job_ref._obj, out_ref._obj
        n = int(job.n_cells)
        lab = np.ctypeslib.as_array(C.cast(group_ptr, C.POINTER(C.c_int32)), (n,)).copy()
        own = np.ctypeslib.as_array(C.cast(C.c_void_p(job.cells), C.POINTER(C.c_int32)), (n,)).copy()
        assert 1 <= n_groups <= 256 and lab.min() >= -1 and lab.max() < n_groups and max_item_cells == 3
        seen.append((n_groups, int((lab >= 0).sum())))
        want = oracle_group_moments(counts, depth, own, lab, n_groups)
        for k, dt in engine.GROUP_FIELDS:
            dst = np.ctypeslib.as_array(C.cast(C.c_void_p(getattr(out, k)), C.POINTER(ctype[dt])), want[k].shape)
            dst[...] = want[k]

    got = engine._group_calls(call, 50, 8, group, 600, cells, 3)
    same(got, oracle_group_moments(counts, depth, cells, group, 600), "600 groups")
    assert [g for g, _ in seen] == [256, 256, 88] and sum(m for _, m in seen) == int((group >= 0).sum())
    with pytest.raises(InvalidInputError, match="out of range"):
        engine._group_calls(call, 50, 8, np.concatenate([[600], group[1:]]), 600, cells, 3)
    with pytest.raises(InvalidInputError, match="labels for"):
        engine._group_calls(call, 50, 8, group[:-1], 600, cells, 3)


# ---- the files ---------------------------------------------------------------------------------------
def _result(variants=None, min_cells=0, min_af=0.0):
    from mgatk2_amd.analysis.groups import group_result

    counts, depth = crafted_rows()
    rng = np.random.default_rng(2)
    labels = rng.integers(-1, 3, 40)
    names = ["B", "NK", "T"]
    res = group_result([(NumpyEngine(counts, depth, 0, 40), 0, 40)], labels, names, ref_of(counts), None, min_cells,
                       min_af, variants)
    return res, counts, depth, labels


def test_group_files_round_trip(tmp_path):
    from types import SimpleNamespace

    from mgatk2_amd import h5lite
    from mgatk2_amd.analysis.groups import GROUP_COLUMNS, MARKER_COLUMNS, read_tsv, write_group_result

    pairs = [(9, 1), (5, 2), (120, 0)]
    variants = SimpleNamespace(pairs=lambda: pairs, variant=["10X>C", "6X>G", "121X>A"])
    res, counts, depth, labels = _result(variants)
    gdir = write_group_result(res, tmp_path)
    assert sorted(p.name for p in gdir.iterdir()) == ["group_allele_freq.tsv", "group_counts.h5", "group_variants.tsv",
                                                      "groups.tsv"]
    want = oracle_group_moments(counts, depth, None, labels, 3)
    g = read_tsv(gdir / "groups.tsv", {"n_cells": int, "n_cells_with_rows": int, "total_depth": int, "mean_depth": float})
    assert tuple(g) == GROUP_COLUMNS and g["group"] == ["B", "NK", "T", "(none)"]
    assert g["n_cells"] == [int((labels == k).sum()) for k in (0, 1, 2, -1)] == g["n_cells_with_rows"]
    assert g["total_depth"][:3] == [int(want["cov"][k].sum()) for k in range(3)]
    assert g["mean_depth"] == [float(d) / float(n * 300) for d, n in zip(g["total_depth"], g["n_cells"])]
    m = read_tsv(gdir / "group_variants.tsv", {k: int for k in MARKER_COLUMNS[4:10] + ("position", "called")} |
                 {"heteroplasmy": float, "heteroplasmy_rest": float})
    assert tuple(m) == MARKER_COLUMNS and len(m["group"]) == len(res.markers) > 0
    assert m["heteroplasmy"] == res.markers.heteroplasmy.tolist() and m["alt_fwd"] == res.markers.alt_fwd.tolist()
    assert m["group"] == [res.group_names[k] for k in res.markers.group.tolist()] and m["variant"] == res.markers.variant
    assert m["called"] == [int((p - 1, "ACGT".index(nt[-1])) in pairs) for p, nt in zip(m["position"], m["nucleotide"])]
    assert sum(m["called"]) > 0
    with h5lite.File(gdir / "group_counts.h5", "r") as f:
        for b in range(4):
            for s in ("fwd", "rev"):
                a = f[f"{'ACGT'[b]}_{s}"][...]
                assert a.dtype == np.uint64 and a.shape == (300, 3)
                np.testing.assert_array_equal(a, want[s][:, :, b].T)
        np.testing.assert_array_equal(f["coverage"][...], want["cov"].T)
        assert [x.decode() for x in f["group"][...].tolist()] == ["B", "NK", "T"]
        assert f["n_cells"][...].tolist() == g["n_cells"][:3]
        assert [x.decode() for x in f["reference"][...].tolist()] == res.ref_alleles
    assert int(want["fwd"].max()) > 65535  # a u16 dataset would have saturated
    af = read_tsv(gdir / "group_allele_freq.tsv", {k: float for k in res.group_names})
    assert list(af) == ["variant", "B", "NK", "T"] and af["variant"] == variants.variant
    for j, name in enumerate(res.group_names):
        assert af[name] == [float(int(want["fwd"][j, p, b]) + int(want["rev"][j, p, b])) / float(want["cov"][j, p])
                            if want["cov"][j, p] else 0.0 for p, b in pairs]


def test_empty_marker_table_writes_the_header_only(tmp_path):
    from mgatk2_amd.analysis.groups import MARKER_COLUMNS, write_group_result

    res, *_ = _result(min_cells=1000)
    assert len(res.markers) == 0 and res.allele_freq is None
    gdir = write_group_result(res, tmp_path)
    assert (gdir / "group_variants.tsv").read_text() == "\t".join(MARKER_COLUMNS) + "\n"
    assert sorted(p.name for p in gdir.iterdir()) == ["group_counts.h5", "group_variants.tsv", "groups.tsv"]


# ---- the processor ---------------------------------------------------------------------------------
def test_after_run_makes_the_groups_of_the_variants_population(tmp_path):
    """The groups step of CellProcessor._after_run over a stand-in engine: labels by the run's cell, a cell
    that did not pass is an all-zero row that counts in n_cells only, and the step's seconds are reported
    only when enabled."""
    from mgatk2_amd.config import PipelineConfig
    from mgatk2_amd.engine import EngineResult
    from mgatk2_amd.exceptions import InvalidInputError
    from mgatk2_amd.processing.processors import CellProcessor

    counts, depth = crafted_rows()
    res = EngineResult.alloc(40, 300, dense=False)
    res.passed[:] = 1
    res.passed[[4, 9]] = 0
    res.ref_tally[:] = (counts[:, :, 0::2].astype(np.int64) + counts[:, :, 1::2]).sum(0).astype(np.uint64)
    labels = np.random.default_rng(8).integers(-1, 3, 40)
    labels[[4, 9]] = (1, -1)
    proc = CellProcessor(PipelineConfig(), tmp_path)
    parts = [(NumpyEngine(counts, depth, 0, 40), 0, 40)]
    assert "groups" not in proc._after_run(res, parts, writers=False) and res.groups is None
    with pytest.raises(InvalidInputError, match="outside the group names"):
        proc.enable_groups(labels, ["a", "b"])
    proc.enable_groups(labels, ["a", "b", "c"], min_cells=1, min_af=0.05)
    assert set(proc._after_run(res, parts, writers=False)) == {"groups"}
    pop = np.where(res.passed.astype(bool), np.arange(40), -1)
    same(res.groups.moments, oracle_group_moments(counts, depth, pop, labels, 3), "processor")
    assert res.groups.table.n_cells.tolist() == [int((labels == k).sum()) for k in (0, 1, 2, -1)]
    assert int(res.groups.table.n_cells_with_rows[1]) == int((labels == 1).sum()) - 1
    check_markers(res.groups.markers, oracle_markers(counts, depth, pop, labels, 3, ref_of(counts), 1, 0.05))
    # a loaded table's subset: labels by the file's column
    proc.population = np.array([30, 2, 17, 5], np.int64)
    proc._after_run(res, parts, writers=False)
    same(res.groups.moments, oracle_group_moments(counts, depth, proc.population, labels[proc.population], 3), "subset")


# ---- the command line and the pipeline ---------------------------------------------------------------
@pytest.mark.parametrize("cmd", ["run", "tenx"])
def test_cli_group_options_reach_run_pipeline(cmd, tmp_path, monkeypatch):
    from click.testing import CliRunner

    from mgatk2_amd import cli

    gf = tmp_path / "groups.tsv"
    gf.write_text("barcode\tgroup\nA\t1\n")
    seen = _invoke(monkeypatch, tmp_path, [cmd])
    assert seen and not any(k.startswith("group") for k in seen)  # off unless asked for
    seen = _invoke(monkeypatch, tmp_path, [cmd, "--groups", str(gf)])
    assert seen["groups"] == str(gf) and "group_min_cells" not in seen and "group_min_af" not in seen
    seen = _invoke(monkeypatch, tmp_path, [cmd, "--groups", str(gf), "--group-min-cells", "0", "--group-min-af", "0.2"])
    assert (seen["groups"], seen["group_min_cells"], seen["group_min_af"]) == (str(gf), 0, 0.2)
    for flag, value in (("--group-min-af", "0.1"), ("--group-min-cells", "3")):
        r = CliRunner().invoke(cli.cli, [cmd, "-i", str(tmp_path / "x.bam"), flag, value])
        assert r.exit_code == 2 and f"{flag} requires --groups" in r.output, r.output
    flags = [p.opts[0] for p in getattr(cli, cmd).params]
    assert flags.index("--groups") < flags.index("--group-min-cells") < flags.index("--group-min-af") < \
        flags.index("--variants")


def test_cli_call_and_analyze_take_the_group_options(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from golden_io import Golden

    from mgatk2_amd import cli, pipeline
    from mgatk2_amd.bam import soa_to_bam

    gf = tmp_path / "groups.tsv"
    gf.write_text("A\t1\n")
    g = Golden("kat_run")
    (tmp_path / "bams").mkdir()
    soa_to_bam(tmp_path / "bams" / "cell1.bam", g.soa, g.whitelist)
    seen = []
    monkeypatch.setattr(pipeline, "run_pipeline", lambda **kw: seen.append(kw) or {})
    r = CliRunner().invoke(cli.cli, ["call", "-i", str(tmp_path / "bams"), "-o", str(tmp_path / "o"), "--groups", str(gf),
                                     "--group-min-cells", "1"])
    assert r.exit_code == 0, r.output
    assert len(seen) == 1 and seen[0]["groups"] == str(gf) and seen[0]["group_min_cells"] == 1
    got = {}
    monkeypatch.setattr(pipeline, "analyze_outputs", lambda *a, **kw: got.update(kw, args=a) or {})
    r = CliRunner().invoke(cli.cli, ["analyze", "-i", str(tmp_path), "--groups", str(gf), "--group-min-af", "0.5"])
    assert r.exit_code == 0, r.output
    assert got["groups"] == str(gf) and got["group_min_af"] == 0.5 and "group_min_cells" not in got
    r = CliRunner().invoke(cli.cli, ["analyze", "-i", str(tmp_path), "--group-min-af", "0.5"])
    assert r.exit_code == 2 and "--group-min-af requires --groups" in r.output
    flags = [p.opts[0] for p in cli.analyze.params]
    assert flags.index("--device") < flags.index("--groups") < flags.index("--variants")
    assert "--groups" in CliRunner().invoke(cli.cli, ["analyze", "--help"]).output


def test_pipeline_keywords_default_off():
    import inspect

    from mgatk2_amd.exceptions import InvalidInputError
    from mgatk2_amd.pipeline import MtDNAPipeline, analysis_settings, run_pipeline

    want = dict(groups=None, group_min_cells=2, group_min_af=0.01)
    for fn in (run_pipeline, MtDNAPipeline.__init__, analysis_settings):
        sig = inspect.signature(fn).parameters
        assert {k: sig[k].default for k in want} == want
        assert list(sig)[-3:] == list(want) or fn is not analysis_settings
    s = analysis_settings()
    assert s["groups"] is None
    with pytest.raises(InvalidInputError, match="group_min_af"):
        analysis_settings(groups={"a": "1"}, group_min_af=2.0)
    with pytest.raises(InvalidInputError, match="group_min_cells"):
        analysis_settings(groups={"a": "1"}, group_min_cells=-1)


# ---- the ABI -----------------------------------------------------------------------------------------
def test_header_and_abi_symbols_list_the_new_names():
    from mgatk2_amd import engine

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mgpileup.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(mgp_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    for s in NEW_SYMBOLS:
        assert s in declared and s in engine.ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.mgp_abi_version() == 7
    assert re.search(r"#define\s+MGP_GROUP_MAX_GROUPS\s+256\b", text) and engine.GROUP_MAX_GROUPS == 256


def test_group_struct_layout_matches_header(tmp_path):
    from mgatk2_amd import engine

    cls = engine.mgp_group_moments
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/mgpileup.h"', "int main(){",
             'printf("%zu\\n", sizeof(mgp_group_moments));']
    lines += [f'printf("%zu\\n", offsetof(mgp_group_moments, {f}));' for f, _ in cls._fields_]
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    assert [f for f, _ in cls._fields_] == [k for k, _ in engine.GROUP_FIELDS] == list(FIELDS)


def test_group_entry_points_refuse_null_arguments_before_any_device_call():
    """Both forms, each pointer in turn, with MGP_E_INVALID and "<call>: bad arguments"; no device is touched
    (this runs without one)."""
    from mgatk2_amd import engine

    lib = engine.load_library()
    counts, depth = np.zeros((1, 8, 8), np.uint32), np.zeros((1, 8), np.uint32)
    group = np.zeros(1, np.int32)
    arrays = engine.alloc_group_moments(1, 8)
    job = engine.mgp_variant_job(0, None, 0)

    def out(missing=None):
        return engine.mgp_group_moments(*[None if k == missing else arrays[k].ctypes.data for k, _ in engine.GROUP_FIELDS])

    def refused(name, *args):
        assert getattr(lib, name)(*args) == engine.MGP_E_INVALID, (name, args)
        assert lib.mgp_last_error().decode() == f"{name}: bad arguments", (name, args)

    rows = (0, counts.ctypes.data, depth.ctypes.data, 1, 8)
    g = group.ctypes.data
    refused("mgp_rows_group_moments", *rows, None, g, 1, 0, C.byref(out()))
    refused("mgp_rows_group_moments", *rows, C.byref(job), None, 1, 0, C.byref(out()))
    refused("mgp_rows_group_moments", *rows, C.byref(job), g, 1, 0, None)
    for k, _ in engine.GROUP_FIELDS:
        refused("mgp_rows_group_moments", *rows, C.byref(job), g, 1, 0, C.byref(out(k)))
    refused("mgp_rows_group_moments", *rows, C.byref(engine.mgp_variant_job(-1, g, 0)), g, 1, 0, C.byref(out()))
    refused("mgp_group_moments_run", None, C.byref(job), g, 1, 0, C.byref(out()))
    refused("mgp_group_moments_run", None, None, None, 1, 0, None)
