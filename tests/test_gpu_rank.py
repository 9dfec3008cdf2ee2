"""mgp_rank_sums on the device (mgp_rank.hip) against the numpy model of tests/test_group_tests.py: exact
integers, the same bytes for every tile and batch; then the rank-sum tests of the cell groups end to end and
through the pipeline (groups/group_tests.tsv)."""

from __future__ import annotations

import numpy as np
import pytest

from golden_io import Golden
from test_group_tests import crafted_matrix, interleaved_labels, model_rank_sums
from test_gpu_groups import GROUP_NAMES, THRESHOLDS, VARIANTS, _groups_file, _label_of, _run_counts
from test_gpu_variants import _files, _pipeline, _same_file
from test_variants import oracle_allele_freq

pytestmark = pytest.mark.gpu

CAP = 2048  # the groups the rank kernel's LDS table holds (engine.RANK_LDS_GROUPS)


def same(got, want, what=""):
    for k, dt in (("r2", np.uint64), ("pos", np.uint32), ("ties", np.uint64)):
        assert got[k].dtype == dt and got[k].shape == want[k].shape, (what, k)
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")


def raw(got):
    return b"".join(got[k].tobytes() for k in ("r2", "pos", "ties"))


# ---- 1. crafted matrices against the model --------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_crafted_matrices(engine_lib, n):
    """The 7 crafted features at sizes around the tile and the padding, the groups at 1, 2 and around the LDS
    table's cap, interleaved labels with one empty group: r2, pos and ties equal the model's as integers, and a
    second call returns the same bytes."""
    assert engine_lib.RANK_LDS_GROUPS == CAP
    x = crafted_matrix(n, seed=n)
    for n_groups in (1, 2, CAP - 1, CAP, CAP + 1):
        group = interleaved_labels(n, n_groups, empty=1)
        got = engine_lib.rank_sums(x, group, n_groups)
        same(got, model_rank_sums(x, group, n_groups), f"n {n} groups {n_groups}")
        assert n_groups == 1 or not got["r2"][:, 1].any()
        assert raw(engine_lib.rank_sums(x, group, n_groups)) == raw(got)


@pytest.mark.parametrize("n_groups", [3, CAP + 5])
def test_sums_that_hold_on_any_input(engine_lib, n_groups):
    rng = np.random.default_rng(n_groups)
    n = 5000
    x = np.where(rng.random((9, n)) < 0.6, 0.0, rng.integers(-20, 60, (9, n)) / 16.0)
    group = rng.integers(0, n_groups, n).astype(np.int32)
    got = engine_lib.rank_sums(x, group, n_groups)
    assert (got["r2"].sum(axis=1, dtype=np.uint64) == n * (n + 1)).all()
    np.testing.assert_array_equal(got["pos"].sum(axis=1, dtype=np.uint64), (x > 0).sum(axis=1))
    same(got, model_rank_sums(x, group, n_groups))


# ---- 2. the knobs, the global passes, the bounds ---------------------------------------------------------
def test_tile_and_batch_change_no_byte(engine_lib, monkeypatch):
    x = np.concatenate([crafted_matrix(8193, seed=1), crafted_matrix(8193, seed=2)[1:]])
    want = None
    for n_groups in (3, CAP + 1):
        group = interleaved_labels(8193, n_groups, empty=1)
        want = model_rank_sums(x, group, n_groups)
        plain = engine_lib.rank_sums(x, group, n_groups)
        same(plain, want, "defaults")
        monkeypatch.setenv("MGP_RANK_TILE", "64")  # P = 16,384: the strides 64 .. 8,192 are global passes
        for batch in ("1", "2", "0"):
            monkeypatch.setenv("MGP_RANK_BATCH", batch)
            assert raw(engine_lib.rank_sums(x, group, n_groups)) == raw(plain), (n_groups, batch)
        monkeypatch.delenv("MGP_RANK_TILE")
        monkeypatch.setenv("MGP_RANK_BATCH", "5")
        assert raw(engine_lib.rank_sums(x, group, n_groups)) == raw(plain)
        monkeypatch.delenv("MGP_RANK_BATCH")
        monkeypatch.setenv("MGP_RANK_TILE", "100")  # not a power of two: the default
        assert raw(engine_lib.rank_sums(x, group, n_groups)) == raw(plain)
        monkeypatch.delenv("MGP_RANK_TILE")


def test_a_row_of_several_global_passes(engine_lib):
    n = 65537  # P = 131,072: 15 global passes at the default tile
    rng = np.random.default_rng(7)
    x = np.stack([np.where(rng.random(n) < 0.8, 0.0, rng.integers(1, 200, n) / 256.0), rng.permutation(n) / 3.0])
    group = interleaved_labels(n, 5, empty=1)
    same(engine_lib.rank_sums(x, group, 5), model_rank_sums(x, group, 5))


def test_the_largest_row(engine_lib):
    n = engine_lib.RANK_MAX_ITEMS
    rng = np.random.default_rng(8)
    x = np.where(rng.random((1, n)) < 0.7, 0.0, rng.integers(1, 1000, (1, n)) / 1024.0)
    group = interleaved_labels(n, 3)
    got = engine_lib.rank_sums(x, group, 3)
    same(got, model_rank_sums(x, group, 3))
    assert int(got["r2"].sum(dtype=np.uint64)) == n * (n + 1)
    with pytest.raises(engine_lib.InvalidInputError, match="2\\^20 items"):
        engine_lib.rank_sums(np.zeros((1, n + 1)), np.zeros(n + 1, np.int32), 3)


def test_refusals(engine_lib):
    bad = engine_lib.InvalidInputError
    x = crafted_matrix(300, seed=4)
    group = interleaved_labels(300, 4)
    for value in (np.nan, np.inf, -np.inf):
        for f, i in ((0, 0), (6, 299), (3, 150)):
            y = x.copy()
            y[f, i] = value
            with pytest.raises(bad, match="not finite"):
                engine_lib.rank_sums(y, group, 4)
    for label, at in ((-1, 0), (4, 299), (-(2 ** 31), 7), (70000, 150)):
        g = group.copy()
        g[at] = label
        with pytest.raises(bad, match="label"):
            engine_lib.rank_sums(x, g, 4)
    for n_groups in (0, -1, 65537):
        with pytest.raises(bad, match="n_groups"):
            engine_lib.rank_sums(x, group, n_groups)
    with pytest.raises(bad, match="labels for 300 items"):
        engine_lib.rank_sums(x, group[:-1], 4)
    with pytest.raises(bad):
        engine_lib.rank_sums(x[0], group, 4)
    same(engine_lib.rank_sums(x, group, 65536), model_rank_sums(x, group, 65536), "the most groups")
    # nothing to rank: zeroed outputs, nothing launched
    for shape in ((0, 300), (3, 0)):
        got = engine_lib.rank_sums(np.zeros(shape), group[: shape[1]], 4)
        assert got["r2"].shape == (shape[0], 4) and not got["r2"].any() and not got["pos"].any() and not got["ties"].any()
    # the call that failed left nothing behind: the next one is right
    same(engine_lib.rank_sums(x, group, 4), model_rank_sums(x, group, 4))


# ---- 3. group_tests end to end ----------------------------------------------------------------------------
def test_group_tests_find_the_planted_variant(engine_lib):
    from mgatk2_amd.analysis.group_tests import group_test_table, group_tests, rank_sum_table

    rng = np.random.default_rng(21)
    labels = np.concatenate([np.repeat([0, 1, 2], 30), np.full(9, -1)])[rng.permutation(99)]
    x = np.where(rng.random((4, 99)) < 0.8, 0.0, rng.integers(1, 8, (4, 99)) / 64.0)  # sparse noise
    x[2, labels == 1] = 0.5 + rng.random(30) / 4  # variant 2: high in group 1 only
    stats = group_tests(x, labels, 3)
    dev = np.where(labels < 0, 3, labels)
    m = model_rank_sums(x, dev, 4)
    want = rank_sum_table(m["r2"][:, :3], m["pos"][:, :3], m["ties"], [30, 30, 30], 99, pos_total=m["pos"].sum(axis=1))
    for k in want:
        np.testing.assert_array_equal(stats[k], want[k], err_msg=k)
    pairs = [(10, 1), (20, 2), (30, 3), (40, 0)]
    tab = group_test_table(stats, pairs, ["A"] * 50, 3, max_p=1.0)
    first = {int(g): i for i, g in reversed(list(enumerate(tab.group.tolist())))}
    assert (int(tab.position[first[1]]), int(tab.base[first[1]])) == (31, 3)
    assert tab.p_value[first[1]] < 1e-10 and tab.auc[first[1]] == 1.0 and tab.pct_in[first[1]] == 1.0
    planted = (tab.position == 31) & (tab.base == 3)
    assert tab.group[planted].tolist() == [1]  # under no other group: there it is lower than in the rest
    strict = group_test_table(stats, pairs, ["A"] * 50, 3)  # the default 0.01
    assert (strict.p_value <= 0.01).all() and (1, 31, 3) in set(zip(strict.group.tolist(), strict.position.tolist(),
                                                                   strict.base.tolist()))


# ---- 4. the pipeline, from the user's side ------------------------------------------------------------------
def _model_file(path, run, group_test_max_p):
    """group_tests.tsv by the model from the run's own files: the heteroplasmy of the count files at the marker
    variants of group_variants.tsv united with variant_stats.tsv's, every cell of the file ranked."""
    from mgatk2_amd.analysis.group_tests import group_test_table, rank_sum_table, write_group_tests
    from mgatk2_amd.analysis.groups import read_tsv
    from mgatk2_amd.analysis.variants import read_variant_stats

    counts, depth, ref, barcodes = _run_counts(run)
    labels = np.array([_label_of(i) for i in range(len(barcodes))])
    mk = read_tsv(run / "groups" / "group_variants.tsv", {"position": int})
    markers = [(GROUP_NAMES.index(g), p - 1, "ACGT".index(nt[-1])) for g, p, nt in
               zip(mk["group"], mk["position"], mk["nucleotide"])]
    stats = read_variant_stats(run / "variants" / "variant_stats.tsv")
    called = [(p - 1, "ACGT".index(nt[-1])) for p, nt in zip(stats["position"], stats["nucleotide"])]
    pairs = sorted({(p, b) for _, p, b in markers} | set(called))
    af = oracle_allele_freq(counts, depth, pairs, 1)
    G = len(GROUP_NAMES)
    m = model_rank_sums(af, np.where(labels < 0, G, labels), G + 1)
    n_in = [int((labels == k).sum()) for k in range(G)]
    t = rank_sum_table(m["r2"][:, :G], m["pos"][:, :G], m["ties"], n_in, labels.size, pos_total=m["pos"].sum(axis=1))
    tab = group_test_table(t, pairs, ref, G, group_test_max_p, markers, called)
    write_group_tests(tab, GROUP_NAMES, path)
    return tab, af, labels, pairs


def test_pipeline_group_tests(tmp_path, engine_lib, monkeypatch):
    """run_pipeline(groups=FILE, group_test=True, call_variants=True) on the synth_run_h5 golden reads writes
    groups/group_tests.tsv equal to the model applied to the heteroplasmy of the written count files and leaves
    every other file what the run without the flag writes, where the file is absent; analyze on the run's
    output writes the same file; U of the first lines equals the count over all pairs of cells."""
    from click.testing import CliRunner

    from mgatk2_amd import cli
    from mgatk2_amd.analysis.group_tests import read_group_tests
    from mgatk2_amd.pipeline import analyze_outputs

    g = Golden("synth_run_h5")
    gf = _groups_file(tmp_path, g.whitelist)
    kw = dict(groups=gf, **THRESHOLDS, **VARIANTS)
    _, plain = _pipeline(tmp_path, "plain", "hdf5", monkeypatch, **kw)
    _, out = _pipeline(tmp_path, "tested", "hdf5", monkeypatch, group_test=True, group_test_max_p=1.0, **kw)
    assert "groups/group_tests.tsv" not in _files(plain)
    assert _files(out) == sorted(_files(plain) + ["groups/group_tests.tsv"])
    for rel in _files(plain):
        _same_file(out, plain, rel)
    tab, af, labels, pairs = _model_file(tmp_path / "model.tsv", out, 1.0)
    assert len(tab) > 0 and tab.marker.any() and tab.called.any()  # not vacuous
    assert (out / "groups" / "group_tests.tsv").read_bytes() == (tmp_path / "model.tsv").read_bytes()
    got = read_group_tests(out / "groups" / "group_tests.tsv")
    for i in range(min(5, len(tab))):  # U as its definition: the pairs (cell of the group, other cell) won, ties half
        x = af[pairs.index((got["position"][i] - 1, "ACGT".index(got["nucleotide"][i][-1])))]
        a, b = x[labels == GROUP_NAMES.index(got["group"][i])], x[labels != GROUP_NAMES.index(got["group"][i])]
        assert got["u"][i] == float((a[:, None] > b[None, :]).sum()) + 0.5 * float((a[:, None] == b[None, :]).sum())
        assert (got["n_cells"][i], got["n_rest"][i]) == (a.size, b.size)
    # analyze on the finished run: the same file, by the keyword and by the command (the default max p there)
    analyze_outputs(out, tmp_path / "again", group_test=True, group_test_max_p=1.0, **kw)
    _same_file(out, tmp_path / "again", "groups/group_tests.tsv")
    r = CliRunner().invoke(cli.cli, ["analyze", "-i", str(out), "-o", str(tmp_path / "cmd"), "--groups", gf,
                                     "--group-min-cells", "0", "--group-min-af", "0", "--group-test", "--variants",
                                     "--variant-min-cells", "0", "--variant-min-strand-cor", "-1", "--variant-min-vmr", "0"])
    assert r.exit_code == 0, r.output
    strict, *_ = _model_file(tmp_path / "strict.tsv", out, 0.01)
    assert (tmp_path / "cmd" / "groups" / "group_tests.tsv").read_bytes() == (tmp_path / "strict.tsv").read_bytes()
    assert len(strict) <= len(tab)


def test_pipeline_group_tests_sharded(tmp_path, engine_lib, monkeypatch):
    """The cells over two routed contexts (one GPU): group_tests.tsv is the single context's, byte for byte."""
    g = Golden("synth_run_h5")
    monkeypatch.setenv("MGP_STREAM_BATCH", "1500")
    kw = dict(groups=_groups_file(tmp_path, g.whitelist), group_test=True, group_test_max_p=1.0, **THRESHOLDS, **VARIANTS)
    _, one = _pipeline(tmp_path, "one", "txt", monkeypatch, **kw)
    _, many = _pipeline(tmp_path, "many", "txt", monkeypatch, devices=[0, 0], **kw)
    assert "groups/group_tests.tsv" in _files(one) and len((one / "groups" / "group_tests.tsv").read_text().splitlines()) > 1
    _same_file(one, many, "groups/group_tests.tsv")
