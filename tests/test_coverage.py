"""Coverage QC (analysis/coverage.py): the host side against a numpy oracle that works from
per-cell arrays (np.mean, np.median, np.std(ddof=1), comparisons and sums).

Every integer field, every median, the kept mask, the recomputed alleles and the strings are
bit-equal. The only floating-point comparisons are against numpy's own rounded means and
sds: rtol = test_variants.tol(m) = 16 m 2^-53 with m the number of terms numpy summed, atol =
tol(m) x the case's largest depth. That allowance is the oracle's rounding; the tables under
test are single divisions of exact integers. tests/test_gpu_coverage.py imports the oracle.
"""

from __future__ import annotations

import re
import subprocess
import warnings
from pathlib import Path

import numpy as np
import pytest

from test_variants import tol

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("mgp_cell_coverage_run", "mgp_position_coverage_run", "mgp_position_depth_hist_run",
               "mgp_position_depth_next_run", "mgp_cell_coverage_rows", "mgp_position_coverage_rows",
               "mgp_position_depth_hist_rows", "mgp_position_depth_next_rows")
CELL_INTS = ("s_depth", "s_depth2", "max_depth", "n_covered", "n_10x", "n_50x", "mid_lo", "mid_hi")
POS_INTS = ("s_depth", "s_depth2", "s_fwd", "s_rev", "s_tn5_fwd", "s_tn5_rev", "tally", "n_covered", "n_10x", "n_50x",
            "n_tn5", "max_depth")


# ---- the oracle ----------------------------------------------------------------------
def population(counts, tn5, depth, cells=None):
    """The population's u32 rows: row cells[k] of (counts [n, L, 8], tn5 [n, L, 2], depth
    [n, L]), zeros for -1."""
    arrays = [np.asarray(a) for a in (counts, tn5, depth)]
    if cells is None:
        return tuple(arrays)
    cells = np.asarray(cells, np.int64)
    out = []
    for a in arrays:
        b = np.zeros((cells.size,) + a.shape[1:], a.dtype)
        b[cells >= 0] = a[cells[cells >= 0]]
        out.append(b)
    return tuple(out)


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


def _stats(d, axis):
    """numpy's mean, median, max, sd / mean and the counts of the int64 matrix d along axis."""
    m = d.shape[axis]
    x = d.astype(np.float64)
    if m == 0:
        shape = d.shape[1 - axis]
        nan = np.full(shape, np.nan)
        return dict(mean=nan, median=nan, max=np.zeros(shape, np.int64), cv=nan, covered=np.zeros(shape, np.int64),
                    n10=np.zeros(shape, np.int64), n50=np.zeros(shape, np.int64))
    mean = np.mean(x, axis=axis)
    sd = _quiet(np.std, x, axis=axis, ddof=1)
    return dict(mean=mean, median=np.median(x, axis=axis), max=d.max(axis=axis), cv=_quiet(np.divide, sd, mean),
                covered=(d > 0).sum(axis=axis), n10=(d >= 10).sum(axis=axis), n50=(d >= 50).sum(axis=axis))


def _mids(d, axis):
    m = d.shape[axis]
    if m == 0:
        z = np.zeros(d.shape[1 - axis], np.int64)
        return z, z
    s = np.sort(d, axis=axis)
    return np.take(s, (m - 1) // 2, axis=axis), np.take(s, m // 2, axis=axis)


def _exact(a):
    """int64 sums as exact Python integers in an object array (sums of squares pass 2^63)."""
    return np.asarray(a, dtype=object)


def oracle_cell_ints(depth):
    """What Engine.cell_coverage returns, from per-cell arrays."""
    d = depth.astype(np.int64)
    lo, hi = _mids(d, 1)
    st = _stats(d, 1)
    return {"s_depth": d.sum(axis=1), "s_depth2": (d.astype(object) ** 2).sum(axis=1) if d.size else d.sum(axis=1),
            "max_depth": st["max"], "n_covered": st["covered"], "n_10x": st["n10"], "n_50x": st["n50"],
            "mid_lo": lo, "mid_hi": hi}


def oracle_cell_table(depth):
    d = depth.astype(np.int64)
    L = d.shape[1]
    st = _stats(d, 1)
    return {"mean_coverage": st["mean"], "median_coverage": st["median"], "max_coverage": st["max"],
            "coverage_cv": st["cv"], "positions_covered": st["covered"], "positions_10x": st["n10"],
            "positions_50x": st["n50"], "coverage_breadth": st["covered"] / L}


def oracle_position_ints(counts, tn5, depth):
    """What Engine.position_coverage returns (and the two middles), from per-cell arrays."""
    d = depth.astype(np.int64)
    c = counts.astype(np.int64)
    t = tn5.astype(np.int64)
    lo, hi = _mids(d, 0)
    st = _stats(d, 0)
    sq = (d.astype(object) ** 2).sum(axis=0) if d.shape[0] else d.sum(axis=0)
    return {"s_depth": d.sum(axis=0), "s_depth2": sq, "s_fwd": c[:, :, 0::2].sum(axis=(0, 2)),
            "s_rev": c[:, :, 1::2].sum(axis=(0, 2)), "s_tn5_fwd": t[:, :, 0].sum(axis=0),
            "s_tn5_rev": t[:, :, 1].sum(axis=0), "tally": (c[:, :, 0::2] + c[:, :, 1::2]).sum(axis=0),
            "n_covered": st["covered"], "n_10x": st["n10"], "n_50x": st["n50"],
            "n_tn5": (t.sum(axis=2) > 0).sum(axis=0), "max_depth": st["max"], "mid_lo": lo, "mid_hi": hi}


def oracle_position_tables(counts, tn5, depth):
    """(position, strand, transposition) tables as R computes them, from per-cell arrays."""
    d = depth.astype(np.int64)
    n, L = d.shape
    st = _stats(d, 0)
    pos = np.arange(1, L + 1)
    position = {"position": pos, "mean_coverage": st["mean"], "median_coverage": st["median"],
                "max_coverage": st["max"], "coverage_cv": st["cv"], "cells_covered": st["covered"],
                "cells_10x": st["n10"], "cells_50x": st["n50"],
                "coverage_dropout": (d == 0).sum(axis=0) / n if n else np.full(L, np.nan)}
    fwd = counts[:, :, 0::2].astype(np.float64).sum(axis=2)
    rev = counts[:, :, 1::2].astype(np.float64).sum(axis=2)
    nanL = np.full(L, np.nan)
    mf, mr = (np.mean(fwd, axis=0), np.mean(rev, axis=0)) if n else (nanL, nanL)
    strand = {"position": pos, "mean_fwd_coverage": mf, "mean_rev_coverage": mr, "total_coverage": st["mean"],
              "strand_balance": mf / np.maximum(st["mean"], 1.0), "strand_imbalance": np.abs(mf - mr)}
    t = tn5.astype(np.int64)
    tf, tr, sd = t[:, :, 0].sum(axis=0), t[:, :, 1].sum(axis=0), d.sum(axis=0)
    tot = tf + tr
    trans = {"position": pos, "tn5_cuts_total": tot, "tn5_cuts_fwd": tf, "tn5_cuts_rev": tr, "total_bases": sd,
             "tn5_frequency": np.divide(tot, sd, out=np.zeros(L), where=sd > 0),
             "cells_with_tn5_cuts": (t.sum(axis=2) > 0).sum(axis=0),
             "mean_tn5_cuts_per_cell": tot / n if n else nanL,
             "strand_bias": np.abs(tf - tr) / np.maximum(tot, 1)}
    return position, strand, trans


def check_ints(got, want, keys, what=""):
    for k in keys:
        g = np.asarray(got[k])
        assert g.dtype in (np.uint64, np.uint32), (what, k, g.dtype)
        assert g.shape == np.asarray(want[k]).shape, (what, k)
        assert _exact(g).tolist() == _exact(want[k]).tolist(), f"{what} {k}"


def check_table(got, want, m, top, what=""):
    """Integer columns bit-equal; fp columns within the oracle's rounding over m terms of
    depths up to top. NaN where and only where the oracle has NaN."""
    from mgatk2_amd.analysis.coverage import INT_COLUMNS

    assert list(got) == list(want), what
    t = tol(max(m, 1))
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k)
        if k in INT_COLUMNS or k == "median_coverage":
            np.testing.assert_array_equal(g, w, err_msg=f"{what} {k}")
        else:
            np.testing.assert_allclose(g, w, rtol=t, atol=t * max(top, 1), equal_nan=True, err_msg=f"{what} {k}")


def crafted_rows(n=150, L=333, seed=11):
    """u32 rows (counts [n, L, 8], tn5 [n, L, 2], depth [n, L]) with the columns the device
    tests name: position 0 all zero, 1 constant, 2 with differing middles for an even
    population, 3..5 with depths in [1, 255], [256, 65,535] and [65,536, 2^24 - 1] alone, 6 with
    Tn5 cuts at depth 0, 7 with ties across the middle; the rest mixed, about half zeros."""
    rng = np.random.default_rng(seed)
    counts = np.zeros((n, L, 8), np.uint32)
    scale = rng.choice([0, 0, 3, 40, 300, 70_000, 2_000_000], size=(n, L))
    for k in range(8):
        counts[:, :, k] = (rng.random((n, L)) * scale).astype(np.uint32)
    counts[:, 0] = 0
    counts[:, 1] = 0
    counts[:, 1, 2] = 37
    counts[:, 2] = 0
    counts[:, 2, 0] = np.arange(n) * 3  # distinct values: the two middles of an even n differ
    for p, (a, b) in zip((3, 4, 5), ((1, 255), (256, 65_535), (65_536, (1 << 24) - 1))):
        counts[:, p] = 0
        counts[:, p, 5] = rng.integers(a, b + 1, size=n)
    counts[:, 5, 5][:2] = (65_536, (1 << 24) - 1)
    counts[:, 6] = 0
    counts[:, 7] = 0
    counts[:, 7, 1] = np.where(np.arange(n) % 3 == 0, 9, 500)
    depth = counts.astype(np.int64).sum(axis=2)
    assert depth.max() < 1 << 24
    tn5 = (rng.random((n, L, 2)) * 6 * (rng.random((n, L, 1)) < 0.3)).astype(np.uint32)
    tn5[:, 6, 0] = 2
    tn5[::2, 6, 1] = 1
    tn5[:, 0] = 0
    return counts, tn5, depth.astype(np.uint32)


def device_like_cell(depth):
    """Engine.cell_coverage's arrays made by the oracle (dtype as the device returns them)."""
    o = oracle_cell_ints(depth)
    return {k: np.array(_exact(o[k]).tolist(), np.uint64 if k.startswith("s_") else np.uint32).reshape(depth.shape[0])
            for k in CELL_INTS}


def device_like_position(counts, tn5, depth):
    o = oracle_position_ints(counts, tn5, depth)
    L = depth.shape[1]
    return {k: np.array(_exact(o[k]).tolist(), np.uint64 if k.startswith("s_") or k == "tally" else np.uint32
                        ).reshape((L, 4) if k == "tally" else L) for k in POS_INTS}, o["mid_lo"], o["mid_hi"]


# ---- tables --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 7, 8])
def test_tables_match_the_oracle(n):
    """n = 0, 1, 2, odd and even; position 0 (and 6) have mean 0: cv NaN there, and for n < 2."""
    from mgatk2_amd.analysis import coverage as cov

    counts, tn5, depth = (a[:n] for a in crafted_rows(8, 41))
    top = int(depth.max()) if n else 0
    L = depth.shape[1]
    cell = cov.cell_coverage_stats(device_like_cell(depth), L)
    check_table(cell, oracle_cell_table(depth), L, top, f"cell n={n}")
    pos, lo, hi = device_like_position(counts, tn5, depth)
    want = oracle_position_tables(counts, tn5, depth)
    check_table(cov.position_coverage_stats(pos, lo, hi, n), want[0], n, top, f"position n={n}")
    check_table(cov.strand_coverage_stats(pos, n), want[1], 4 * n, top, f"strand n={n}")
    check_table(cov.transposition_stats(pos, n), want[2], n, top, f"tn5 n={n}")
    p = cov.position_coverage_stats(pos, lo, hi, n)
    assert np.isnan(p["coverage_cv"][0]) and (n >= 2) == bool(np.isfinite(p["coverage_cv"][1]))
    if n:
        assert p["mean_coverage"][1] == 37.0 and p["coverage_dropout"][0] == 1.0
    if n >= 2:
        assert p["coverage_cv"][1] == 0.0  # a constant column: the integer variance is exactly 0


def test_cell_table_of_zero_rows_and_one_position():
    from mgatk2_amd.analysis import coverage as cov

    depth = np.zeros((3, 5), np.uint32)
    depth[1] = (4, 0, 9, 0, 0)
    cell = cov.cell_coverage_stats(device_like_cell(depth), 5)
    check_table(cell, oracle_cell_table(depth), 5, 9)
    assert np.isnan(cell["coverage_cv"][0]) and cell["median_coverage"][1] == 0.0
    one = cov.cell_coverage_stats(device_like_cell(depth[:, :1]), 1)
    assert np.isnan(one["coverage_cv"]).all() and one["mean_coverage"].tolist() == [0.0, 4.0, 0.0]


# ---- the median driver ---------------------------------------------------------------
def numpy_primitives(parts):
    """numpy stand-ins for the two device passes over `parts` (a list of depth matrices
    [n_i, L]): each part's result computed alone, merged as run_coverage merges them."""
    calls = {"hist": 0, "next": 0}

    def hist_fn(shift, prefix):
        calls["hist"] += 1
        out = 0
        for d in parts:
            d = d.astype(np.uint64)
            on = np.ones(d.shape, bool) if shift == 24 else (d >> np.uint64(shift + 8)) == prefix[None, :]
            b = ((d >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
            h = np.zeros((d.shape[1], 256), np.int64)
            for p in range(d.shape[1]):
                h[p] = np.bincount(b[on[:, p], p], minlength=256)
            out = out + h
        return out

    def next_fn(v):
        calls["next"] += 1
        n_le, nxt = 0, np.full(v.shape, 0xFFFFFFFF, np.uint32)
        for d in parts:
            d = d.astype(np.int64)
            n_le = n_le + (d <= v[None, :].astype(np.int64)).sum(axis=0)
            above = np.where(d > v[None, :].astype(np.int64), d, 0xFFFFFFFF)
            nxt = np.minimum(nxt, above.min(axis=0).astype(np.uint32) if d.shape[0] else nxt)
        return n_le, nxt

    return hist_fn, next_fn, calls


def median_cases():
    rng = np.random.default_rng(3)
    small = rng.integers(0, 256, size=(9, 12)).astype(np.uint32)
    mid = rng.integers(0, 65_536, size=(10, 12)).astype(np.uint32)
    big = rng.integers(0, 1 << 32, size=(10, 12), dtype=np.uint64).astype(np.uint32)
    big[0, 0] = 0xFFFFFFFF
    big[:, 1] = 0xFFFFFFFF
    ties = np.repeat(np.array([[5, 5, 5, 7, 7, 7, 300, 300]], np.uint32).T, 4, axis=1)
    ties[:, 1] = (1, 2, 3, 4, 70_000, 70_001, 70_002, 70_003)  # the middles 4 and 70,000 differ
    ties[:, 2] = 0
    ties[:, 3] = (0, 0, 0, 0, 0, 0, 0, 1 << 31)
    return {"below256": small, "below65536": mid, "u32": big, "ties": ties, "one": mid[:1], "two": big[:2]}


@pytest.mark.parametrize("case", list(median_cases()))
@pytest.mark.parametrize("split", [None, 3])
def test_median_driver(case, split):
    """The radix select against np.median: one round below 256, two below 65,536, four up to
    2^32 - 1; ties across the middle need no `next` pass; two parts merge exactly."""
    from mgatk2_amd.analysis.coverage import position_medians

    d = median_cases()[case]
    parts = [d] if split is None else [d[:split], d[split:]]
    hist_fn, next_fn, calls = numpy_primitives(parts)
    lo, hi = position_medians(hist_fn, next_fn, d.max(axis=0), d.shape[0])
    wlo, whi = _mids(d.astype(np.int64), 0)
    np.testing.assert_array_equal(lo, wlo)
    np.testing.assert_array_equal(hi, whi)
    assert lo.dtype == np.uint32 and hi.dtype == np.uint32
    np.testing.assert_array_equal((lo.astype(np.float64) + hi.astype(np.float64)) / 2, np.median(d.astype(np.float64), axis=0))
    assert calls["hist"] == {"below256": 1, "below65536": 2, "u32": 4, "ties": 4, "one": 2, "two": 4}[case]
    assert calls["next"] == (1 if (wlo != whi).any() else 0)
    if case == "ties":
        assert (wlo != whi).tolist() == [False, True, False, False]


def test_median_driver_empty_population():
    from mgatk2_amd.analysis.coverage import position_medians

    def never(*a):
        raise AssertionError("no device pass for an empty population")

    lo, hi = position_medians(never, never, np.zeros(4, np.uint32), 0)
    assert lo.tolist() == hi.tolist() == [0, 0, 0, 0]


# ---- filter and reference ------------------------------------------------------------
def test_filter_thresholds_are_inclusive():
    from mgatk2_amd.analysis.coverage import filter_cells_by_coverage

    t = {"mean_coverage": np.array([10.0, 9.999, 10.0, 0.0, 50.0]), "coverage_breadth": np.array([0.5, 0.9, 0.49, 0.0, 1.0])}
    assert filter_cells_by_coverage(t, 10, 0.5).tolist() == [True, False, False, False, True]
    assert filter_cells_by_coverage(t, 0.0, 0.0).tolist() == [True] * 5  # zero rows included
    assert filter_cells_by_coverage(t).tolist() == [True, False, False, False, True]  # R's defaults


def test_recomputed_reference_ties_and_empty():
    from mgatk2_amd.analysis.coverage import recompute_reference_alleles

    tally = np.array([[0, 0, 0, 0], [3, 3, 1, 0], [0, 2, 2, 2], [0, 0, 0, 9], [1, 0, 5, 5], [2 ** 40, 2 ** 40 + 1, 0, 0]],
                     np.uint64)
    assert recompute_reference_alleles(tally) == ["N", "A", "C", "T", "G", "C"]


# ---- files ---------------------------------------------------------------------------
def test_coverage_files_round_trip(tmp_path):
    from mgatk2_amd.analysis import coverage as cov

    counts, tn5, depth = crafted_rows(6, 23)
    L = depth.shape[1]
    cell = cov.cell_coverage_stats(device_like_cell(depth), L)
    kept = cov.filter_cells_by_coverage(cell, float(np.sort(cell["mean_coverage"])[3]), 0.3)  # the upper three
    assert kept.sum() == 3
    kc, kt, kd = counts[kept], tn5[kept], depth[kept]
    pos, lo, hi = device_like_position(kc, kt, kd)
    m = int(kept.sum())
    res = cov.CoverageResult(cells=np.arange(6), kept=kept, cell=cell, position=cov.position_coverage_stats(pos, lo, hi, m),
                             strand=cov.strand_coverage_stats(pos, m), transposition=cov.transposition_stats(pos, m),
                             tally=pos["tally"], ref_alleles=cov.recompute_reference_alleles(pos["tally"]))
    names = [f"BC{i}" for i in range(6)]
    run_ref = ["A"] * L
    cdir = cov.write_coverage_outputs(res, names, tmp_path, run_ref)
    assert sorted(p.name for p in cdir.iterdir()) == ["cell_coverage_stats.tsv", "position_coverage_stats.tsv",
                                                      "reference_alleles.tsv", "strand_coverage_stats.tsv",
                                                      "transposition_stats.tsv"]
    got = cov.read_table(cdir / "cell_coverage_stats.tsv")
    assert list(got) == ["barcode", *cov.CELL_COLUMNS, "kept"] and got["barcode"] == names
    assert got["kept"] == ["TRUE" if k else "FALSE" for k in kept]
    for table, cols, name in ((res.cell, cov.CELL_COLUMNS, "cell_coverage_stats.tsv"),
                              (res.position, cov.POSITION_COLUMNS, "position_coverage_stats.tsv"),
                              (res.strand, cov.STRAND_COLUMNS, "strand_coverage_stats.tsv"),
                              (res.transposition, cov.TRANSPOSITION_COLUMNS, "transposition_stats.tsv")):
        got = cov.read_table(cdir / name)
        for c in cols:  # floats as repr: the same bits back (NaN as NaN)
            np.testing.assert_array_equal(np.asarray(got[c], np.asarray(table[c]).dtype), table[c], err_msg=f"{name} {c}")
    text = (cdir / "position_coverage_stats.tsv").read_text().splitlines()
    assert text[0].split("\t") == list(cov.POSITION_COLUMNS) and len(text) == L + 1 and "nan" in text[1]
    ref = cov.read_table(cdir / "reference_alleles.tsv")
    assert ref["position"] == list(range(1, L + 1)) and ref["reference"] == run_ref
    assert ref["recomputed"] == res.ref_alleles and ref["recomputed"][0] == "N"
    res.ref_alleles = None
    cov.write_coverage_outputs(res, names, tmp_path / "b")
    assert not (tmp_path / "b" / "coverage" / "reference_alleles.tsv").exists()


# ---- CLI -----------------------------------------------------------------------------
COVERAGE_KEYS = ("coverage_stats", "cell_min_mean_coverage", "cell_min_coverage_breadth", "recompute_reference")


@pytest.mark.parametrize("cmd", ["run", "tenx"])
def test_cli_coverage_options_reach_run_pipeline(cmd, tmp_path, monkeypatch):
    from test_variants import _invoke

    seen = _invoke(monkeypatch, tmp_path, [cmd])
    assert seen and not any(k in seen for k in COVERAGE_KEYS)  # absent unless asked for
    seen = _invoke(monkeypatch, tmp_path, [cmd, "--coverage-stats"])
    assert seen["coverage_stats"] is True and seen["cell_min_mean_coverage"] == 0.0
    assert seen["cell_min_coverage_breadth"] == 0.0 and seen["recompute_reference"] is False
    assert not any(k.startswith("variant_") or k == "call_variants" for k in seen)
    seen = _invoke(monkeypatch, tmp_path, [cmd, "--coverage-stats", "--cell-min-mean-coverage", "10",
                                           "--cell-min-coverage-breadth", "0.5", "--recompute-reference", "--variants"])
    assert (seen["coverage_stats"], seen["cell_min_mean_coverage"], seen["cell_min_coverage_breadth"],
            seen["recompute_reference"], seen["call_variants"]) == (True, 10.0, 0.5, True, True)
    seen = _invoke(monkeypatch, tmp_path, [cmd, "--variants", "--cell-min-mean-coverage", "3"])
    assert seen["call_variants"] is True and seen["cell_min_mean_coverage"] == 3.0 and "coverage_stats" not in seen
    seen = _invoke(monkeypatch, tmp_path, [cmd, "--coverage-stats", "--dry-run"])
    assert seen == {} and not (tmp_path / "out" / "coverage").exists()


def test_cli_call_takes_the_coverage_options(tmp_path, monkeypatch):
    from click.testing import CliRunner

    from golden_io import Golden
    from mgatk2_amd import cli as cli_mod
    from mgatk2_amd import pipeline
    from mgatk2_amd.bam import soa_to_bam

    g = Golden("kat_run")
    (tmp_path / "bams").mkdir()
    soa_to_bam(tmp_path / "bams" / "cell1.bam", g.soa, g.whitelist)
    seen = []
    monkeypatch.setattr(pipeline, "run_pipeline", lambda **kw: seen.append(kw) or {})
    r = CliRunner().invoke(cli_mod.cli, ["call", "-i", str(tmp_path / "bams"), "-o", str(tmp_path / "o"),
                                         "--coverage-stats", "--cell-min-coverage-breadth", "0.25"])
    assert r.exit_code == 0, r.output
    assert len(seen) == 1 and seen[0]["coverage_stats"] is True and seen[0]["cell_min_coverage_breadth"] == 0.25


def test_pipeline_coverage_keywords_default_off():
    import inspect

    from mgatk2_amd.pipeline import MtDNAPipeline, run_pipeline
    from mgatk2_amd.processing.processors import CellProcessor

    want = dict(coverage_stats=False, cell_min_mean_coverage=0.0, cell_min_coverage_breadth=0.0,
                recompute_reference=False)
    for fn in (run_pipeline, MtDNAPipeline.__init__):
        sig = inspect.signature(fn).parameters
        assert {k: sig[k].default for k in want} == want
    sig = inspect.signature(CellProcessor.enable_coverage).parameters
    assert {k: sig[k].default for k in ("min_mean_coverage", "min_coverage_breadth", "recompute_reference")} == \
        dict(min_mean_coverage=0.0, min_coverage_breadth=0.0, recompute_reference=False)


# ---- ABI -----------------------------------------------------------------------------
def test_header_and_abi_symbols_list_the_coverage_names():
    from mgatk2_amd import engine

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mgpileup.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(mgp_[a-z_0-9]+)\s*\(", text))
    for s in NEW_SYMBOLS:
        assert s in declared and s in engine.ABI_SYMBOLS, s
    lib = engine.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.mgp_abi_version() == 7


def test_coverage_struct_layouts_match_header(tmp_path):
    import ctypes as C

    from mgatk2_amd import engine

    structs = {"mgp_cell_coverage": engine.mgp_cell_coverage, "mgp_position_coverage": engine.mgp_position_coverage}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/mgpileup.h"', "int main(){"]
    for name, cls in structs.items():
        lines.append(f'printf("%zu\\n", sizeof({name}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("%zu\\n", offsetof({name}, {fname}));')
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    want = []
    for cls in structs.values():
        want.append(C.sizeof(cls))
        want.extend(getattr(cls, f).offset for f, _ in cls._fields_)
    assert got == want
    assert [f for f, _ in engine.mgp_cell_coverage._fields_] == [k for k, _ in engine.CELL_COVERAGE_FIELDS] == list(CELL_INTS)
    assert [f for f, _ in engine.mgp_position_coverage._fields_] == [k for k, _ in engine.POSITION_COVERAGE_FIELDS] \
        == list(POS_INTS)
