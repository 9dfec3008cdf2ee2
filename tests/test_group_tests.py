"""The rank-sum test of each variant per cell group, host side (analysis/group_tests.py): the numpy model of
the device's integers (the GPU file imports it), the formula against scipy, its corner cases, the options
and the file."""

from __future__ import annotations

import inspect
import math

import numpy as np
import pytest

from test_variants import _invoke


# ---- the model of mgp_rank_sums ----------------------------------------------------------------------
def model_rank_sums(x, group, n_groups):
    """What mgp_rank_sums returns, in numpy: per feature np.unique of x + 0.0 gives the tie classes, their
    cumulative counts lo and hi; r2 = the group's sum of lo + hi + 2, pos its values > 0, ties sum t^3 - t."""
    x = np.asarray(x, np.float64)
    group = np.asarray(group, np.int64)
    nf, n = x.shape
    r2 = np.zeros((nf, n_groups), np.uint64)
    pos = np.zeros((nf, n_groups), np.uint32)
    ties = np.zeros(nf, np.uint64)
    for f in range(nf):
        v = x[f] + 0.0
        _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
        cnt = cnt.astype(np.int64)
        hi = np.cumsum(cnt) - 1
        lo = hi - cnt + 1
        val = (lo + hi + 2)[inv.reshape(-1)]
        # (fp64 weights are exact here: every sum is an integer below 2^53)
        r2[f] = np.bincount(group, weights=val.astype(np.float64), minlength=n_groups).astype(np.uint64)
        pos[f] = np.bincount(group[v > 0], minlength=n_groups)
        ties[f] = int((cnt ** 3 - cnt).sum())
    return {"r2": r2, "pos": pos, "ties": ties}


def crafted_matrix(n, seed=0):
    """7 features over n items: all zeros, all distinct, 90 % zeros, two values only, one with -0.0 and negative
    values, a row sorted descending, and random rationals a / d."""
    rng = np.random.default_rng(seed)
    distinct = rng.permutation(n).astype(np.float64) / max(n, 1)
    sparse = np.where(rng.random(n) < 0.9, 0.0, rng.integers(1, 50, n) / 64.0)
    two = np.where(rng.random(n) < 0.5, 0.25, 0.75)
    signed = rng.integers(-3, 4, n) / 8.0
    signed[::5] = -0.0
    descending = np.arange(n, 0, -1, dtype=np.float64) / 7.0
    rationals = rng.integers(0, 12, n) / rng.integers(1, 12, n)
    return np.stack([np.zeros(n), distinct, sparse, two, signed, descending, rationals])


def interleaved_labels(n, n_groups, empty=None):
    """Item i in group i mod n_groups, moved to the next group where that is `empty` (n_groups > 1)."""
    g = np.arange(n, dtype=np.int64) % n_groups
    if empty is not None and n_groups > 1:
        g = np.where(g == empty, (g + 1) % n_groups, g)
    return g.astype(np.int32)


def test_model_is_scipys_midranks():
    stats = pytest.importorskip("scipy.stats")
    x = crafted_matrix(301, 3)
    group = interleaved_labels(301, 4, empty=2)
    m = model_rank_sums(x, group, 4)
    for f in range(x.shape[0]):
        r = stats.rankdata(x[f] + 0.0)
        for g in range(4):
            assert int(m["r2"][f, g]) == int(round(2 * r[group == g].sum()))
    assert int(m["r2"][1].sum()) == 301 * 302 and int(m["ties"][0]) == 301 ** 3 - 301 and int(m["ties"][1]) == 0
    assert m["pos"][0].sum() == 0 and m["r2"][:, 2].sum() == 0


def _scipy_cases():
    rng = np.random.default_rng(11)
    cases = []
    x = np.where(rng.random(301) < 0.7, 0.0, rng.integers(1, 40, 301) / 40.0)  # 70 % zeros, a -0.0 among them
    x[3] = -0.0
    cases.append((x, (rng.random(301) < 0.3).astype(np.int32)))
    cases.append((rng.random(64), (np.arange(64) % 3 == 0).astype(np.int32)))  # no ties
    x = np.concatenate([np.zeros(400), 0.5 + rng.random(200)])  # z above 10: a group of all the largest values
    cases.append((x, (np.arange(600) >= 400).astype(np.int32)))
    x = rng.integers(0, 4, 50) / 4.0  # heavy ties, a small group
    cases.append((x, (np.arange(50) < 5).astype(np.int32)))
    return cases


def test_rank_sum_table_against_scipy():
    """U equals scipy's exactly; z and p are its asymptotic method's with the continuity correction. Measured on
    these cases on the CPU (scipy 1.15): the largest relative difference of p is 1.31e-13, at z = 23.8 and
    p = 2e-125 (erfc(z / sqrt 2) of libm against scipy's ndtr(-z), which multiplies z by 1/sqrt 2: one rounding of
    the argument, amplified by about z^2 = 567); at z = 2.1 it is 6.2e-16, below z = 1 it is 0. Ten times the
    largest, 1.31e-12, is asserted."""
    stats = pytest.importorskip("scipy.stats")
    from mgatk2_amd.analysis.group_tests import rank_sum_table

    worst, z_max = 0.0, 0.0
    for x, group in _scipy_cases():
        m = model_rank_sums(x[None, :], group, 2)
        n_in = np.bincount(group, minlength=2)
        t = rank_sum_table(m["r2"], m["pos"], m["ties"], n_in, x.size)
        for g in range(2):
            ref = stats.mannwhitneyu(x[group == g], x[group != g], alternative="two-sided", method="asymptotic",
                                     use_continuity=True)
            assert float(t["u"][0, g]) == float(ref.statistic)
            assert t["auc"][0, g] == ref.statistic / (n_in[g] * (x.size - n_in[g]))
            p = float(t["p_value"][0, g])
            rel = abs(p - ref.pvalue) / ref.pvalue if ref.pvalue > 0 else abs(p)
            worst, z_max = max(worst, rel), max(z_max, float(t["z"][0, g]))
            assert t["pct_in"][0, g] == (x[group == g] > 0).mean() and t["pct_rest"][0, g] == (x[group != g] > 0).mean()
    print(f"largest relative difference of p: {worst:.3g}; largest z: {z_max:.3g}")
    assert z_max > 10
    assert worst <= 1.31e-12


# ---- the formula's corner cases ----------------------------------------------------------------------
def test_all_values_tied_gives_p_one():
    from mgatk2_amd.analysis.group_tests import rank_sum_table

    x = np.full((1, 40), 0.25)
    group = interleaved_labels(40, 3)
    m = model_rank_sums(x, group, 3)
    t = rank_sum_table(m["r2"], m["pos"], m["ties"], np.bincount(group, minlength=3), 40)
    assert t["tested"].all()
    assert (t["p_value"] == 1.0).all() and (t["auc"] == 0.5).all() and (t["z"] == 0.0).all() and (t["p_adj"] == 1.0).all()
    assert (t["pct_in"] == 1.0).all() and (t["pct_rest"] == 1.0).all()


def test_empty_group_and_whole_population_are_left_out():
    from mgatk2_amd.analysis.group_tests import group_test_table, rank_sum_table

    x = np.arange(12, dtype=np.float64)[None, :]
    group = np.zeros(12, np.int32)  # group 0 is everyone (n2 = 0), group 1 empty (n1 = 0)
    m = model_rank_sums(x, group, 2)
    t = rank_sum_table(m["r2"], m["pos"], m["ties"], [12, 0], 12)
    assert not t["tested"].any() and np.isnan(t["p_value"]).all() and np.isnan(t["u"]).all()
    assert len(group_test_table(t, [(7, 2)], ["A"] * 16, 2, max_p=1.0)) == 0


def test_group_of_all_the_largest_values():
    from mgatk2_amd.analysis.group_tests import rank_sum_table

    x = np.concatenate([np.zeros(30), np.linspace(0.5, 0.9, 10)])[None, :]
    group = (np.arange(40) >= 30).astype(np.int32)
    m = model_rank_sums(x, group, 2)
    t = rank_sum_table(m["r2"], m["pos"], m["ties"], [30, 10], 40)
    assert t["auc"][0, 1] == 1.0 and t["auc"][0, 0] == 0.0 and t["u"][0, 1] == 300.0 and t["u"][0, 0] == 0.0
    assert t["p_value"][0, 0] == t["p_value"][0, 1] < 1e-6  # two-sided: the same test from either side
    assert t["pct_in"][0, 1] == 1.0 and t["pct_rest"][0, 1] == 0.0
    # the groups need not cover the items: the same numbers with group 0 unlabelled and pos_total given
    t1 = rank_sum_table(m["r2"][:, 1:], m["pos"][:, 1:], m["ties"], [10], 40, pos_total=[10])
    for k in ("u", "auc", "z", "p_value", "pct_in", "pct_rest"):
        assert t1[k][0, 0] == t[k][0, 1]
    # Bonferroni over the tested variants
    three = rank_sum_table(np.repeat(m["r2"], 3, 0), np.repeat(m["pos"], 3, 0), np.repeat(m["ties"], 3), [30, 10], 40)
    assert three["p_adj"][0, 1] == min(1.0, 3 * t["p_value"][0, 1])


def test_max_p_checker():
    from mgatk2_amd.analysis.group_tests import check_group_test_max_p
    from mgatk2_amd.exceptions import InvalidInputError

    assert check_group_test_max_p(0) == 0.0 and check_group_test_max_p("0.05") == 0.05 and check_group_test_max_p(1) == 1.0
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(InvalidInputError, match="group_test_max_p"):
            check_group_test_max_p(bad)


# ---- the options -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cmd", ["run", "tenx"])
def test_cli_group_test_options_reach_run_pipeline(cmd, tmp_path, monkeypatch):
    from click.testing import CliRunner

    from mgatk2_amd import cli

    gf = tmp_path / "groups.tsv"
    gf.write_text("barcode\tgroup\nA\t1\n")
    seen = _invoke(monkeypatch, tmp_path, [cmd, "--groups", str(gf)])
    assert seen and not any(k.startswith("group_test") for k in seen)  # off unless asked for
    seen = _invoke(monkeypatch, tmp_path, [cmd, "--groups", str(gf), "--group-test"])
    assert seen["group_test"] is True and "group_test_max_p" not in seen
    seen = _invoke(monkeypatch, tmp_path, [cmd, "--groups", str(gf), "--group-test", "--group-test-max-p", "0.2"])
    assert (seen["group_test"], seen["group_test_max_p"]) == (True, 0.2)
    bam = str(tmp_path / "x.bam")
    r = CliRunner().invoke(cli.cli, [cmd, "-i", bam, "--group-test"])
    assert r.exit_code == 2 and "--group-test requires --groups" in r.output, r.output
    r = CliRunner().invoke(cli.cli, [cmd, "-i", bam, "--groups", str(gf), "--group-test-max-p", "0.2"])
    assert r.exit_code == 2 and "--group-test-max-p requires --group-test" in r.output, r.output
    r = CliRunner().invoke(cli.cli, [cmd, "-i", bam, "--groups", str(gf), "--group-test", "--group-test-max-p", "2"])
    assert r.exit_code == 2, r.output
    flags = [p.opts[0] for p in getattr(cli, cmd).params]
    assert flags.index("--group-min-af") < flags.index("--group-test") < flags.index("--group-test-max-p") < \
        flags.index("--variants")


def test_cli_call_and_analyze_take_the_group_test_options(tmp_path, monkeypatch):
    from click.testing import CliRunner

    from mgatk2_amd import cli, pipeline

    gf = tmp_path / "groups.tsv"
    gf.write_text("A\t1\n")
    got = {}
    monkeypatch.setattr(pipeline, "analyze_outputs", lambda *a, **kw: got.update(kw, args=a) or {})
    r = CliRunner().invoke(cli.cli, ["analyze", "-i", str(tmp_path), "--groups", str(gf), "--group-test"])
    assert r.exit_code == 0, r.output
    assert got["group_test"] is True and "group_test_max_p" not in got
    r = CliRunner().invoke(cli.cli, ["analyze", "-i", str(tmp_path), "--group-test"])
    assert r.exit_code == 2 and "--group-test requires --groups" in r.output
    for cmd in ("call", "analyze"):
        flags = [p.opts[0] for p in getattr(cli, cmd).params]
        assert "--group-test" in flags and "--group-test-max-p" in flags


def test_pipeline_keywords_default_off():
    from mgatk2_amd.exceptions import InvalidInputError
    from mgatk2_amd.pipeline import MtDNAPipeline, analysis_settings, run_pipeline
    from mgatk2_amd.processing.processors import CellProcessor

    want = dict(group_test=False, group_test_max_p=0.01)
    for fn in (run_pipeline, MtDNAPipeline.__init__, analysis_settings, CellProcessor.enable_groups):
        sig = inspect.signature(fn).parameters
        assert {k: sig[k].default for k in want} == want
    # before `groups`, whose place at the end is pinned
    assert list(inspect.signature(analysis_settings).parameters)[-5:] == [
        "group_test", "group_test_max_p", "groups", "group_min_cells", "group_min_af"]
    s = analysis_settings()
    assert s["group_test"] is False and s["group_test_max_p"] == 0.01
    assert analysis_settings(groups={"a": "1"}, group_test=True, group_test_max_p=0.5)["group_test_max_p"] == 0.5
    with pytest.raises(InvalidInputError, match="group_test requires groups"):
        analysis_settings(group_test=True)
    with pytest.raises(InvalidInputError, match="group_test_max_p"):
        analysis_settings(groups={"a": "1"}, group_test=True, group_test_max_p=1.5)


def test_abi_lists_the_entry_point():
    from mgatk2_amd import engine
    from mgatk2_amd.build import ROOT

    assert "mgp_rank_sums" in engine.ABI_SYMBOLS
    assert "mgp_rank_sums(" in (ROOT / "include" / "mgpileup.h").read_text()
    assert engine.RANK_MAX_ITEMS == 1 << 20 and engine.RANK_MAX_GROUPS == 1 << 16


# ---- the table and the file --------------------------------------------------------------------------
def _planted_stats():
    """3 groups of 20 cells and 6 unlabelled ones; variant 0 high in group 1 only, variant 1 in groups 0 and 2
    alike, variant 2 flat (U = n1 n2 / 2 everywhere: never "higher"), variant 3 in two cells of group 1 (p = 0.03)."""
    from mgatk2_amd.analysis.group_tests import rank_sum_table

    rng = np.random.default_rng(5)
    labels = np.concatenate([np.repeat([0, 1, 2], 20), np.full(6, -1)])
    x = np.zeros((4, 66))
    x[0, labels == 1] = 0.5 + rng.random(20) / 4
    x[1, labels == 0] = 0.4 + rng.random(20) / 4
    x[1, labels == 2] = 0.4 + rng.random(20) / 4
    x[2] = 0.3
    x[3, np.flatnonzero(labels == 1)[:2]] = 0.2
    dev = np.where(labels < 0, 3, labels)
    m = model_rank_sums(x, dev, 4)
    t = rank_sum_table(m["r2"][:, :3], m["pos"][:, :3], m["ties"], [20, 20, 20], 66, pos_total=m["pos"].sum(axis=1))
    return t, x, labels


def test_table_order_and_round_trip(tmp_path):
    from mgatk2_amd.analysis.group_tests import (TEST_COLUMNS, group_test_table, read_group_tests, write_group_tests)

    t, x, labels = _planted_stats()
    pairs = [(100, 2), (100, 3), (7, 0), (50, 1)]  # (not in genomic order here: the table orders its lines itself)
    ref = ["C"] * 200
    tab = group_test_table(t, pairs, ref, 3, max_p=0.01, markers=[(1, 100, 2), (2, 100, 2)], called=[(100, 3)])
    # variant 0 under group 1 alone; variant 1 under groups 0 and 2; the flat one nowhere; only.pos
    assert [(int(g), int(p), int(b)) for g, p, b in zip(tab.group, tab.position, tab.base)] == [
        (0, 101, 3), (1, 101, 2), (2, 101, 3)]
    assert tab.marker.tolist() == [0, 1, 0] and tab.called.tolist() == [1, 0, 1]
    assert (tab.n_cells == 20).all() and (tab.n_rest == 46).all() and (tab.auc > 0.5).all()
    assert tab.n_tested == 4 and tab.variant == ["101C>T", "101C>G", "101C>T"]
    assert tab.p_adj.tolist() == [min(1.0, 4 * p) for p in tab.p_value.tolist()]
    # with every line let through: by group, then p, then position, then base
    every = group_test_table(t, pairs, ref, 3, max_p=1.0)
    keys = list(zip(every.group.tolist(), every.p_value.tolist(), every.position.tolist(), every.base.tolist()))
    assert keys == sorted(keys) and [k[0::2] for k in keys] == [(0, 101), (1, 101), (1, 51), (2, 101)]
    assert 0.01 < every.p_value[2] < 0.05
    mu = 20 * 46 / 2
    assert (every.u > mu).all()
    names = ["a", "b", "c"]
    path = tmp_path / "group_tests.tsv"
    write_group_tests(tab, names, path)
    back = read_group_tests(path)
    assert tuple(back) == TEST_COLUMNS
    assert back["group"] == ["a", "b", "c"] and back["variant"] == tab.variant and back["nucleotide"] == ["C>T", "C>G", "C>T"]
    for k in ("pct_in", "pct_rest", "u", "auc", "z", "p_value", "p_adj"):
        assert back[k] == getattr(tab, k).tolist()  # repr round-trips every float
    assert back["position"] == [101, 101, 101] and back["marker"] == [0, 1, 0] and back["called"] == [1, 0, 1]
    assert back["n_cells"] == [20] * 3 and back["n_rest"] == [46] * 3
    text = path.read_text().splitlines()
    assert text[1].split("\t")[8] == repr(float(tab.u[0]))


def test_no_tested_variant_writes_the_header_only(tmp_path):
    from mgatk2_amd.analysis.group_tests import TEST_COLUMNS, group_test_table, write_group_tests

    tab = group_test_table(None, [], ["A"] * 10, 3)
    assert len(tab) == 0 and tab.n_tested == 0
    write_group_tests(tab, ["a", "b", "c"], tmp_path / "t.tsv")
    assert (tmp_path / "t.tsv").read_text() == "\t".join(TEST_COLUMNS) + "\n"


def test_tested_pairs_unite_markers_and_called_in_genomic_order():
    from types import SimpleNamespace

    from mgatk2_amd.analysis.group_tests import tested_pairs

    markers = SimpleNamespace(position=np.array([300, 5, 300]), base=np.array([1, 3, 1]))
    called = SimpleNamespace(pairs=lambda: [(299, 0), (4, 3), (1000, 2)])
    assert tested_pairs(markers) == [(4, 3), (299, 1)]
    assert tested_pairs(markers, called) == [(4, 3), (299, 0), (299, 1), (1000, 2)]


def test_erfc_is_the_two_sided_normal_tail():
    from mgatk2_amd.analysis.group_tests import rank_sum_table

    # 2 against 2 without ties: U = 4, sigma^2 = 4 * 5 / 12, z = (2 - 1/2) / sigma
    x = np.array([[0.1, 0.2, 0.3, 0.4]])
    m = model_rank_sums(x, np.array([0, 0, 1, 1]), 2)
    t = rank_sum_table(m["r2"], m["pos"], m["ties"], [2, 2], 4)
    z = 1.5 / math.sqrt(4 * 5 / 12)
    assert t["u"][0].tolist() == [0.0, 4.0] and t["z"][0, 1] == z and t["p_value"][0, 1] == math.erfc(z / math.sqrt(2))
