"""Clustering by heteroplasmy, host side (no GPU): a numpy oracle of the definitions in
include/mgpileup.h (Euclidean pair distances; complete linkage with R's tie rule; R's merge,
order and cutree conventions), checked against scipy where there are no ties and against the
conventions where there are; HClust.cutree, the file writers, the CLI options, the ABI and
the pipeline's plumbing with the oracle standing in for the device calls.

tests/test_gpu_cluster.py compares the device with this oracle.
"""

from __future__ import annotations

import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("mgp_pair_dist", "mgp_hclust_dist", "mgp_hclust")
CLUSTER_FILES = ["variants/cell_hclust.tsv", "variants/cell_order.tsv", "variants/variant_hclust.tsv",
                 "variants/variant_order.tsv"]


# ---- the oracle ----------------------------------------------------------------------
def oracle_dist(x):
    """D[i][j] = sqrt(sum_k (x[k][i] - x[k][j])^2), k ascending, of x [n_feat, n_items]."""
    x = np.asarray(x, np.float64)
    s = np.zeros((x.shape[1], x.shape[1]))
    for k in range(x.shape[0]):
        d = x[k][:, None] - x[k][None, :]
        s += d * d
    return np.sqrt(s)


def oracle_steps(dist):
    """The n - 1 raw steps (i, j, height) of complete linkage: the smallest distance over the
    active pairs i < j, np.argmin over the row-major matrix with the lower triangle, the
    diagonal and the inactive rows and columns at +inf (ties: smallest i, then smallest j);
    j leaves, D(i, k) = max(D(i, k), D(j, k)). The working matrix is compacted to the active
    clusters now and then (their order is kept, so the tie rule is unchanged)."""
    full = np.array(dist, np.float64)
    n = full.shape[0]
    ids = np.arange(n)
    alive = np.ones(n, bool)

    def masked(f):
        m = f.copy()
        m[np.tril_indices(m.shape[0])] = np.inf
        return m

    up = masked(full)
    steps = []
    for _ in range(n - 1):
        a, b = divmod(int(np.argmin(up)), up.shape[1])
        steps.append((int(ids[a]), int(ids[b]), float(up[a, b])))
        new = np.maximum(full[a], full[b])
        full[a, :] = new
        full[:, a] = new
        alive[b] = False
        shown = np.where(alive, new, np.inf)
        up[a, a + 1:] = shown[a + 1:]
        up[:a, a] = shown[:a]
        up[b, :] = np.inf
        up[:, b] = np.inf
        if alive.sum() < 0.9 * alive.size:
            keep = np.flatnonzero(alive)
            full = full[np.ix_(keep, keep)]
            ids, alive = ids[keep], np.ones(keep.size, bool)
            up = masked(full)
    return steps


def oracle_tree(steps, n):
    """R's merge [n - 1, 2], height and order (1-based) from the raw steps."""
    lab = {i: -(i + 1) for i in range(n)}
    merge = np.zeros((max(n - 1, 0), 2), np.int32)
    for s, (i, j, _) in enumerate(steps):
        a, b = lab[i], lab[j]
        if a < 0 and b < 0:
            pair = (a, b) if -a < -b else (b, a)  # two singletons: ascending item
        elif a < 0 or b < 0:
            pair = (min(a, b), max(a, b))  # the singleton first
        else:
            pair = (min(a, b), max(a, b))  # two clusters: ascending step
        merge[s] = pair
        lab[i] = s + 1
    order = [int(v) for v in merge[-1]] if n > 1 else [-1] * n
    while any(v > 0 for v in order):
        order = [w for v in order for w in ((int(merge[v - 1][0]), int(merge[v - 1][1])) if v > 0 else (v,))]
    return merge, np.array([h for _, _, h in steps], np.float64), np.array([-v for v in order], np.int32)


def oracle_hclust(dist):
    n = np.asarray(dist).shape[0]
    return oracle_tree(oracle_steps(dist), n)


def oracle_cutree(merge, n, k):
    """The first n - k merges applied; clusters numbered 1.. by first appearance in item order."""
    members = {}
    label = list(range(n))
    for s in range(n - k):
        got = []
        for v in merge[s]:
            got += [-int(v) - 1] if v < 0 else members.pop(int(v))
        members[s + 1] = got
        for i in got:
            label[i] = n + s
    seen = {}
    return np.array([seen.setdefault(v, len(seen) + 1) for v in label], np.int32)


def partition(labels):
    """A labelling as a canonical partition (numbered by first appearance)."""
    seen = {}
    return [seen.setdefault(int(v), len(seen)) for v in labels]


def tied_matrix(n, nf, values, seed):
    """[nf, n] of a few integer values: heavy ties among the distances."""
    return np.random.default_rng(seed).integers(0, values, (nf, n)).astype(np.float64)


def check_conventions(merge, height, order, n):
    """R's conventions row by row: valid entries, a singleton before a cluster, two singletons
    by item, two clusters by step, every item and every earlier cluster used once; heights
    non-decreasing; order a permutation consistent with the merges."""
    assert merge.shape == (max(n - 1, 0), 2) and height.shape == (max(n - 1, 0),) and order.shape == (n,)
    assert sorted(order.tolist()) == list(range(1, n + 1))
    assert np.all(np.diff(height) >= 0)
    used = set()
    for s in range(n - 1):
        a, b = int(merge[s, 0]), int(merge[s, 1])
        for v in (a, b):
            assert v != 0 and -n <= v <= s and v not in used, (s, v)
            used.add(v)
        if a < 0 and b < 0:
            assert -a < -b
        else:
            assert a < 0 < b or 0 < a < b
    assert len(used) == 2 * (n - 1)
    if n > 1:  # the leaves of every cluster are a contiguous run of `order`, left child first
        pos = {item: r for r, item in enumerate(order.tolist())}
        span = {}
        for s in range(n - 1):
            runs = [(pos[-v], pos[-v]) if v < 0 else span[int(v)] for v in merge[s].tolist()]
            assert runs[0][1] + 1 == runs[1][0], s
            span[s + 1] = (runs[0][0], runs[1][1])
        assert span[n - 1] == (0, n - 1)


# ---- the oracle against scipy and against the conventions -----------------------------
def test_oracle_equals_scipy_without_ties():
    from scipy.cluster.hierarchy import cut_tree, linkage
    from scipy.spatial.distance import squareform

    n = 130
    x = np.random.default_rng(11).random((7, n))
    d = oracle_dist(x)
    iu = np.triu_indices(n, 1)
    assert np.unique(d[iu]).size == n * (n - 1) // 2 == 8385  # tie-free: the order of the merges is forced
    assert np.array_equal(d, d.T) and np.all(np.diag(d) == 0)
    np.testing.assert_allclose(d[iu], squareform(d, checks=False), rtol=0, atol=0)
    merge, height, order = oracle_hclust(d)
    check_conventions(merge, height, order, n)
    z = linkage(squareform(d, checks=False), "complete")
    np.testing.assert_array_equal(height, z[:, 2])
    for k in (1, 2, 5, 17, 130):
        assert partition(oracle_cutree(merge, n, k)) == partition(cut_tree(z, n_clusters=k).reshape(-1)), k


def test_oracle_conventions_on_tied_data():
    n = 40
    d = oracle_dist(tied_matrix(n, 3, 2, 5))
    assert np.unique(d).size <= 4
    merge, height, order = oracle_hclust(d)
    check_conventions(merge, height, order, n)
    assert merge[0].tolist() == [-1, -int(np.flatnonzero(d[0, 1:] == 0)[0] + 2)]  # the first zero of row 0
    # all distances equal: every step is a tie and takes (0, next): (1, 2), (3, step 1), ...
    merge, height, order = oracle_hclust(np.zeros((6, 6)))
    assert merge.tolist() == [[-1, -2], [-3, 1], [-4, 2], [-5, 3], [-6, 4]]
    assert height.tolist() == [0.0] * 5 and order.tolist() == [6, 5, 4, 3, 1, 2]


# ---- HClust.cutree and the small cases -------------------------------------------------
def _hclust_of(dist):
    from mgatk2_amd.analysis.clustering import HClust

    merge, height, order = oracle_hclust(dist)
    return HClust(merge, height, order, int(np.asarray(dist).shape[0]))


def test_cutree_numbers_clusters_by_first_appearance():
    from mgatk2_amd.exceptions import InvalidInputError

    # items 0, 3 close; 1, 2 close; 4 far from all
    pts = np.array([[0.0, 10.0, 10.5, 0.25, 40.0]])
    tree = _hclust_of(oracle_dist(pts))
    assert tree.merge.tolist() == [[-1, -4], [-2, -3], [1, 2], [-5, 3]]
    assert tree.order.tolist() == [5, 1, 4, 2, 3]
    assert tree.cutree(5).tolist() == [1, 2, 3, 4, 5]
    assert tree.cutree(3).tolist() == [1, 2, 2, 1, 3]
    assert tree.cutree(2).tolist() == [1, 1, 1, 1, 2]
    assert tree.cutree(1).tolist() == [1] * 5
    for k in (0, 6, -1):
        with pytest.raises(InvalidInputError):
            tree.cutree(k)
    for seed, n in ((1, 2), (2, 3), (3, 57)):
        d = oracle_dist(tied_matrix(n, 3, 3, seed))
        tree = _hclust_of(d)
        for k in range(1, n + 1):
            np.testing.assert_array_equal(tree.cutree(k), oracle_cutree(tree.merge, n, k))


def test_small_trees():
    from mgatk2_amd.analysis.clustering import HClust

    one = _hclust_of(np.zeros((1, 1)))
    assert one.merge.shape == (0, 2) and one.height.shape == (0,) and one.order.tolist() == [1]
    assert one.cutree(1).tolist() == [1]
    two = _hclust_of(np.array([[0.0, 3.0], [3.0, 0.0]]))
    assert two.merge.tolist() == [[-1, -2]] and two.height.tolist() == [3.0] and two.order.tolist() == [1, 2]
    assert two.cutree(1).tolist() == [1, 1] and two.cutree(2).tolist() == [1, 2]
    none = HClust(np.zeros((0, 2), np.int32), np.zeros(0), np.zeros(0, np.int32), 0)
    assert none.cutree(0).shape == (0,)


def test_no_items_need_no_device():
    """n_items = 0: empty outputs, nothing launched (so this runs without a device)."""
    from mgatk2_amd import engine
    from mgatk2_amd.build import build_engine

    build_engine()
    assert engine.cluster_pair_dist(np.zeros((3, 0))).shape == (0, 0)
    merge, height, order = engine.cluster_hclust_dist(np.zeros((0, 0)))
    assert merge.shape == (0, 2) and height.shape == (0,) and order.shape == (0,)
    merge, height, order, dist = engine.cluster_hclust(np.zeros((4, 0)), want_dist=True)
    assert merge.shape == (0, 2) and order.shape == (0,) and dist.shape == (0, 0)


# ---- the files -----------------------------------------------------------------------------
def test_cluster_files_round_trip(tmp_path):
    from mgatk2_amd.analysis.clustering import ClusterResult, read_hclust, write_cluster_outputs

    rng = np.random.default_rng(4)
    af = rng.random((5, 9))
    cells, variants = _hclust_of(oracle_dist(af)), _hclust_of(oracle_dist(af.T))
    barcodes = [f"BC{i:02d}-1" for i in range(9)]
    names = [f"{100 + i}A>G" for i in range(5)]
    vdir = write_cluster_outputs(ClusterResult(cells, variants, cells.cutree(3)), barcodes, names, tmp_path)
    assert vdir == tmp_path / "variants"
    assert sorted(p.name for p in vdir.iterdir()) == ["cell_clones.tsv", "cell_hclust.tsv", "cell_order.tsv",
                                                      "variant_hclust.tsv", "variant_order.tsv"]
    for name, tree in (("cell", cells), ("variant", variants)):
        back = read_hclust(vdir / f"{name}_hclust.tsv")
        np.testing.assert_array_equal(back.merge, tree.merge)
        np.testing.assert_array_equal(back.height, tree.height)  # (repr round-trips fp64)
        np.testing.assert_array_equal(back.order, tree.order)
    lines = (vdir / "cell_hclust.tsv").read_text().splitlines()
    assert lines[0] == "step\ta\tb\theight" and len(lines) == 9
    assert lines[1] == f"1\t{cells.merge[0, 0]}\t{cells.merge[0, 1]}\t{float(cells.height[0])!r}"
    lines = (vdir / "cell_order.tsv").read_text().splitlines()
    assert lines[0] == "rank\tbarcode" and lines[1:] == [f"{r + 1}\t{barcodes[i - 1]}" for r, i in
                                                         enumerate(cells.order.tolist())]
    lines = (vdir / "variant_order.tsv").read_text().splitlines()
    assert lines[0] == "rank\tvariant" and lines[1:] == [f"{r + 1}\t{names[i - 1]}" for r, i in
                                                         enumerate(variants.order.tolist())]
    lines = (vdir / "cell_clones.tsv").read_text().splitlines()
    assert lines[0] == "barcode\tclone" and lines[1:] == [f"{b}\t{c}" for b, c in zip(barcodes, cells.cutree(3))]
    # without clones no clone file; a side without a tree writes nothing
    write_cluster_outputs(ClusterResult(cells, variants, None), barcodes, names, tmp_path / "b")
    assert not (tmp_path / "b" / "variants" / "cell_clones.tsv").exists()
    write_cluster_outputs(ClusterResult(None, None, None), barcodes, names, tmp_path / "c")
    assert list((tmp_path / "c" / "variants").iterdir()) == []


# ---- the device calls' stand-in, and cluster_heteroplasmy ------------------------------------
def stand_in_device(monkeypatch):
    """The oracle behind engine.cluster_*: the host logic is then testable without a device."""
    from mgatk2_amd import engine

    calls = []

    def pair_dist(x, device=0):
        calls.append(("pair_dist", device))
        return oracle_dist(x)

    def hclust_dist(dist, device=0):
        calls.append(("hclust_dist", device))
        return oracle_hclust(dist)

    def hclust(x, device=0, want_dist=False):
        calls.append(("hclust", device))
        d = oracle_dist(x)
        return (*oracle_hclust(d), d if want_dist else None)

    monkeypatch.setattr(engine, "cluster_pair_dist", pair_dist)
    monkeypatch.setattr(engine, "cluster_hclust_dist", hclust_dist)
    monkeypatch.setattr(engine, "cluster_hclust", hclust)
    return calls


def test_cluster_heteroplasmy_sides_and_errors(monkeypatch, caplog):
    from mgatk2_amd import analysis
    from mgatk2_amd.analysis.clustering import CLUSTER_MAX_ITEMS, cluster_heteroplasmy, hclust, pair_dist
    from mgatk2_amd.exceptions import InvalidInputError

    assert analysis.cluster_heteroplasmy is cluster_heteroplasmy and analysis.hclust is hclust
    assert analysis.pair_dist is pair_dist and analysis.HClust and analysis.write_cluster_outputs
    calls = stand_in_device(monkeypatch)
    af = np.random.default_rng(8).random((4, 7))
    res = cluster_heteroplasmy(af, clones=3, device=2)
    assert calls == [("hclust", 2), ("hclust", 2)]
    want_c, want_v = oracle_hclust(oracle_dist(af)), oracle_hclust(oracle_dist(af.T))
    for got, want, n in ((res.cells, want_c, 7), (res.variants, want_v, 4)):
        assert got.n == n
        for a, b in zip((got.merge, got.height, got.order), want):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(res.clones, oracle_cutree(want_c[0], 7, 3))
    assert cluster_heteroplasmy(af).clones is None
    tree = hclust(dist=oracle_dist(af))
    np.testing.assert_array_equal(tree.merge, want_c[0])
    np.testing.assert_array_equal(pair_dist(af), oracle_dist(af))
    with pytest.raises(InvalidInputError):
        hclust()
    with pytest.raises(InvalidInputError):
        hclust(x=af, dist=oracle_dist(af))
    for bad in (0, 8):
        with pytest.raises(InvalidInputError):
            cluster_heteroplasmy(af, clones=bad)
    with pytest.raises(InvalidInputError):
        cluster_heteroplasmy(af, barcodes=["a"] * 6)
    # fewer than two cells or variants: no tree on either side, a log line, no device call
    del calls[:]
    import logging

    with caplog.at_level(logging.INFO, logger="mgatk2_amd.analysis.clustering"):
        for shape in ((0, 7), (1, 7), (4, 1), (0, 0)):
            res = cluster_heteroplasmy(np.zeros(shape), clones=None)
            assert res.cells is None and res.variants is None and res.clones is None
    assert calls == [] and caplog.text.count("Clustering skipped") == 4
    # above the bound: refused before any device call
    with pytest.raises(InvalidInputError, match="more than 65536"):
        cluster_heteroplasmy(np.zeros((2, CLUSTER_MAX_ITEMS + 1)))
    assert calls == []


def test_variant_items_are_numbered_in_genomic_order(tmp_path, monkeypatch):
    """With a VariantTable the variants are clustered in (position, base) order whatever the
    table's own (vmr) order: two tables of the same variants in different orders, as two
    shardings of one run can give, write the same files."""
    from mgatk2_amd.analysis.clustering import cluster_heteroplasmy, write_cluster_outputs
    from mgatk2_amd.analysis.variants import VariantTable

    stand_in_device(monkeypatch)
    rng = np.random.default_rng(3)
    pos = np.array([900, 12, 12, 4000, 77, 900])
    base = np.array([2, 3, 0, 1, 1, 0])
    af = rng.integers(0, 3, (6, 8)) / 2.0  # (tied rows and columns)
    barcodes = [f"c{i}" for i in range(8)]

    def table(perm):
        z = np.zeros(6)
        t = VariantTable(position=pos[perm], base=base[perm], ref=["N"] * 6, mean=z, vmr=z, variance=z,
                         n_cells_detected=z, n_cells_conf_detected=z, strand_correlation=z)
        t.variant = [f"{p}N>{'ACGT'[b]}" for p, b in zip(t.position, t.base)]
        return t

    want_rows = [2, 1, 4, 5, 0, 3]  # (12, A), (12, T), (77, C), (900, A), (900, G), (4000, C)
    outs = []
    for k, perm in enumerate((np.arange(6), np.array([3, 0, 5, 1, 4, 2]))):
        res = cluster_heteroplasmy(af[perm], barcodes, table(perm), clones=2)
        assert perm[res.variant_rows].tolist() == want_rows
        canon = af[want_rows]
        for got, want in ((res.cells, oracle_hclust(oracle_dist(canon))), (res.variants, oracle_hclust(oracle_dist(canon.T)))):
            for a, b in zip((got.merge, got.height, got.order), want):
                np.testing.assert_array_equal(a, b)
        outs.append(write_cluster_outputs(res, barcodes, table(perm), tmp_path / str(k)))
    for f in sorted(p.name for p in outs[0].iterdir()):
        assert (outs[0] / f).read_bytes() == (outs[1] / f).read_bytes(), f
    names = [f"{pos[r]}N>{'ACGT'[base[r]]}" for r in want_rows]
    lines = (outs[0] / "variant_order.tsv").read_text().splitlines()[1:]
    assert lines == [f"{r + 1}\t{names[i - 1]}" for r, i in enumerate(res.variants.order.tolist())]
    # a bare matrix, or names alone: items in row order
    assert cluster_heteroplasmy(af, table=[str(i) for i in range(6)]).variant_rows is None


# ---- CLI and signatures ------------------------------------------------------------------
def _cli(tmp_path, monkeypatch, args):
    from click.testing import CliRunner

    from golden_io import Golden
    from mgatk2_amd import cli as cli_mod
    from mgatk2_amd import pipeline
    from mgatk2_amd.bam import soa_to_bam

    g = Golden("kat_run")
    bam = tmp_path / "x.bam"
    if not bam.exists():
        soa_to_bam(bam, g.soa, g.whitelist)
        (tmp_path / "bc.tsv").write_text("".join(b + "\n" for b in g.whitelist))
    seen = {}
    monkeypatch.setattr(pipeline, "run_pipeline", lambda **kw: seen.update(kw) or {})
    r = CliRunner().invoke(cli_mod.cli, [args[0], "-i", str(bam), "-b", str(tmp_path / "bc.tsv"), "-o",
                                         str(tmp_path / "out"), *args[1:]])
    return r, seen


@pytest.mark.parametrize("cmd", ["run", "tenx"])
def test_cli_cluster_options(cmd, tmp_path, monkeypatch):
    r, seen = _cli(tmp_path, monkeypatch, [cmd, "--variants"])
    assert r.exit_code == 0 and "cluster" not in seen and "clones" not in seen  # off unless asked for
    r, seen = _cli(tmp_path, monkeypatch, [cmd, "--variants", "--cluster"])
    assert r.exit_code == 0 and seen["cluster"] is True and "clones" not in seen and seen["call_variants"] is True
    r, seen = _cli(tmp_path, monkeypatch, [cmd, "--variants", "--cluster", "--clones", "4"])
    assert r.exit_code == 0 and seen["cluster"] is True and seen["clones"] == 4
    for args, text in ((["--cluster"], "--cluster requires --variants"),
                       (["--variants", "--clones", "3"], "--clones requires --cluster"),
                       (["--variants", "--cluster", "--clones", "0"], "--clones"),
                       (["--variants", "--cluster", "--clones", "-2"], "--clones")):
        r, seen = _cli(tmp_path, monkeypatch, [cmd, *args])
        assert r.exit_code == 2 and text in r.output and seen == {}, (args, r.output)
    r, _ = _cli(tmp_path, monkeypatch, [cmd, "--help"])
    assert "--cluster" in r.output and "--clones" in r.output


def test_cli_call_takes_the_cluster_options(tmp_path, monkeypatch):
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
    base = ["call", "-i", str(tmp_path / "bams"), "-o", str(tmp_path / "o")]
    r = CliRunner().invoke(cli_mod.cli, [*base, "--variants", "--cluster", "--clones", "2"])
    assert r.exit_code == 0, r.output
    assert len(seen) == 1 and seen[0]["cluster"] is True and seen[0]["clones"] == 2
    for args, text in ((["--cluster"], "--cluster requires --variants"),
                       (["--variants", "--clones", "2"], "--clones requires --cluster")):
        r = CliRunner().invoke(cli_mod.cli, [*base, *args])
        assert r.exit_code == 2 and text in r.output and len(seen) == 1


def test_pipeline_keywords_default_off_and_checked(tmp_path):
    from mgatk2_amd.exceptions import InvalidInputError
    from mgatk2_amd.pipeline import MtDNAPipeline, run_pipeline
    from mgatk2_amd.processing.processors import CellProcessor

    for fn in (run_pipeline, MtDNAPipeline.__init__):
        sig = inspect.signature(fn).parameters
        assert sig["cluster"].default is False and sig["clones"].default is None
    for kw in (dict(cluster=True), dict(call_variants=True, clones=2), dict(call_variants=True, cluster=True, clones=0)):
        with pytest.raises(InvalidInputError):
            MtDNAPipeline("no.bam", ["A"], tmp_path, **kw)
    proc = CellProcessor(None, tmp_path)
    with pytest.raises(InvalidInputError):
        proc.enable_clustering()
    proc.enable_variants()
    with pytest.raises(InvalidInputError):
        proc.enable_clustering(clones=0)
    proc.enable_clustering(clones=5)
    assert proc.cluster_opt == {"clones": 5}


# ---- ABI -----------------------------------------------------------------------------------
def test_header_and_abi_symbols_list_the_new_names():
    from mgatk2_amd import engine
    from mgatk2_amd.build import HIP_SOURCES, build_engine

    assert "mgp_cluster.hip" in HIP_SOURCES
    build_engine()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mgpileup.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(mgp_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    for s in NEW_SYMBOLS:
        assert s in declared and s in engine.ABI_SYMBOLS and hasattr(lib, s), s
        assert not s.endswith("_rows")
    assert lib.mgp_abi_version() == engine.ABI_VERSION == 7


def test_cluster_calls_refuse_bad_arguments_before_any_device_call():
    """Null or negative arguments and sizes above the bounds: MGP_E_INVALID with the call's own
    message, before any device call (so this runs without a device)."""
    from mgatk2_amd import engine
    from mgatk2_amd.build import build_engine

    build_engine()
    lib = engine.load_library()
    x = np.zeros((2, 3))
    d = np.zeros((3, 3))
    merge, height, order = np.zeros((2, 2), np.int32), np.zeros(2), np.zeros(3, np.int32)
    p = lambda a: a.ctypes.data  # noqa: E731

    def refused(name, message, *args):
        rc = getattr(lib, name)(0, *args)
        assert rc == engine.MGP_E_INVALID, (name, args, rc)
        assert lib.mgp_last_error().decode() == message, (name, args, lib.mgp_last_error())

    for args in ((None, 3, 2, p(d)), (p(x), 3, 2, None), (p(x), -1, 2, p(d)), (p(x), 3, -1, p(d))):
        refused("mgp_pair_dist", "mgp_pair_dist: bad arguments", *args)
    for args in ((None, 3, p(merge), p(height), p(order)), (p(d), 3, None, p(height), p(order)),
                 (p(d), 3, p(merge), None, p(order)), (p(d), 3, p(merge), p(height), None),
                 (p(d), -3, p(merge), p(height), p(order))):
        refused("mgp_hclust_dist", "mgp_hclust_dist: bad arguments", *args)
    for args in ((None, 3, 2, p(merge), p(height), p(order), None), (p(x), 3, 2, None, p(height), p(order), None),
                 (p(x), 3, 2, p(merge), None, p(order), None), (p(x), 3, 2, p(merge), p(height), None, None),
                 (p(x), -3, 2, p(merge), p(height), p(order), None), (p(x), 3, -2, p(merge), p(height), p(order), None)):
        refused("mgp_hclust", "mgp_hclust: bad arguments", *args)
    big = "more than 65536 items in one call (the distance matrix is 8 n^2 bytes)"
    refused("mgp_pair_dist", f"mgp_pair_dist: {big}", p(x), 65537, 1, p(d))
    refused("mgp_hclust_dist", f"mgp_hclust_dist: {big}", p(d), 65537, p(merge), p(height), p(order))
    refused("mgp_hclust", f"mgp_hclust: {big}", p(x), 65537, 1, p(merge), p(height), p(order), None)
    refused("mgp_hclust", "mgp_hclust: more than 2^24 features in one call", p(x), 3, (1 << 24) + 1, p(merge),
            p(height), p(order), None)
    # n_feat = 0 needs no x, a single item no merge or height: not refused for a null there
    # (they go on to the device: only the refusals are checked here)


# ---- the pipeline's plumbing, the oracle standing in for the device --------------------------
def _patch_run(monkeypatch, oracle_lib, variants=True):
    """The oracle engine of tests/test_pipeline.py, which also calls the variants as
    CellProcessor._call_variants does, from numpy-made moments: with two devices the
    matrix is made in two column parts and merged, as the sharded run's is."""
    from test_pipeline import patch_oracle_engine
    from test_variants import oracle_allele_freq, oracle_dev2, oracle_moments, population

    from mgatk2_amd.analysis.variants import mean_af, variant_table
    from mgatk2_amd.file_io.writers import ref_alleles
    from mgatk2_amd.processing import processors

    patch_oracle_engine(monkeypatch, oracle_lib)
    plain = processors.CellProcessor.run_soa

    def run_soa(self, soa_batches, n_cells):
        res = plain(self, soa_batches, n_cells)
        if self.variants_opt is not None:
            pop = self._population(res)
            counts, depth = population(res.counts, res.depth, pop)
            n = pop.size
            mom = oracle_moments(counts, depth)
            opt = self.variants_opt
            filters = (opt["min_cells"], opt["min_strand_cor"], opt["min_vmr"]) if variants else (10 ** 6, 0, 0)
            res.variants = variant_table(mom, oracle_dev2(counts, depth, mean_af(mom, n)), ref_alleles(res.ref_tally),
                                         n, *filters)
            cut = n // 2 if len(self.devices) > 1 else n
            res.allele_freq = np.concatenate([oracle_allele_freq(counts[:cut], depth[:cut], res.variants.pairs()),
                                              oracle_allele_freq(counts[cut:], depth[cut:], res.variants.pairs())],
                                             axis=1)
            res.variant_cells = None
        return res

    def run_stream(self, reader, n_cells, batch_reads=None, rows_target=True):
        from test_pipeline import stream_batches

        return run_soa(self, stream_batches(reader, n_cells), n_cells)

    monkeypatch.setattr(processors.CellProcessor, "run_soa", run_soa)
    monkeypatch.setattr(processors.CellProcessor, "run_stream", run_stream)


def _pipeline(tmp_path, name, **kw):
    from golden_io import Golden
    from mgatk2_amd.bam import soa_to_bam
    from mgatk2_amd.pipeline import run_pipeline

    g = Golden("synth_run_h5")
    p = g.params
    d = tmp_path / name
    d.mkdir()
    soa_to_bam(d / "x.bam", g.soa, g.whitelist)
    (d / "barcodes.tsv").write_text("".join(b + "\n" for b in g.whitelist))
    run_pipeline(str(d / "x.bam"), str(d / "barcodes.tsv"), str(d / "out"), min_baseq=p["min_baseq"],
                 min_mapq=p["min_mapq"], min_reads_per_cell=p["min_reads_per_cell"],
                 max_strand_bias=p["max_strand_bias"], skip_deduplication=p["skip_deduplication"],
                 use_fragment_length_dedup=p["use_fragment_length_dedup"], output_format="txt", **kw)
    return g, d / "out"


def written_matrix(out, barcodes):
    """The heteroplasmy matrix a txt run wrote, its rows in genomic order (position, then base:
    the clustering's variant items), and their names."""
    import gzip

    rows = [line.split("\t") for line in (out / "variants" / "variant_stats.tsv").read_text().splitlines()[1:]]
    rows.sort(key=lambda r: (int(r[0]), "ACGT".index(r[1][-1])))
    names = [r[2] for r in rows]
    af = np.zeros((len(names), len(barcodes)))
    for line in gzip.decompress((out / "variants" / "output.allele_freq.txt.gz").read_bytes()).decode().splitlines():
        v, b, x = line.split(",")
        af[names.index(v), barcodes.index(b)] = float(x)
    return names, af


def _files(out):
    return sorted(str(p.relative_to(out)) for p in out.rglob("*") if p.is_file())


# (thresholds lowered so that variants pass at this depth: 94 of them)
LOW = dict(call_variants=True, variant_min_cells=0, variant_min_strand_cor=-1.0, variant_min_vmr=1.0)


def test_pipeline_writes_the_cluster_files(tmp_path, oracle_lib, monkeypatch):
    from mgatk2_amd.analysis.clustering import read_hclust

    _patch_run(monkeypatch, oracle_lib)
    calls = stand_in_device(monkeypatch)
    g, plain = _pipeline(tmp_path, "plain", **LOW)
    assert calls == [] and not any("hclust" in f or "order" in f or "clones" in f for f in _files(plain))
    _, out = _pipeline(tmp_path, "clustered", cluster=True, clones=3, **LOW)
    assert calls == [("hclust", 0), ("hclust", 0)]
    new = sorted(CLUSTER_FILES + ["variants/cell_clones.tsv"])
    assert [f for f in _files(out) if f not in _files(plain)] == new
    for rel in _files(plain):
        if not rel.endswith(("summary.txt", "output.log")):
            assert (out / rel).read_bytes() == (plain / rel).read_bytes(), rel
    # the files are the oracle's trees of the matrix the same run wrote
    names, af = written_matrix(out, g.whitelist)
    assert af.shape[0] >= 2 and af.shape[1] == 12
    for side, x, labels in (("cell", af, g.whitelist), ("variant", af.T, names)):
        want = oracle_hclust(oracle_dist(x))
        got = read_hclust(out / "variants" / f"{side}_hclust.tsv")
        for a, b in zip((got.merge, got.height, got.order), want):
            np.testing.assert_array_equal(a, b)
        order = (out / "variants" / f"{side}_order.tsv").read_text().splitlines()[1:]
        assert order == [f"{r + 1}\t{labels[i - 1]}" for r, i in enumerate(want[2].tolist())]
    clones = (out / "variants" / "cell_clones.tsv").read_text().splitlines()[1:]
    want = oracle_cutree(oracle_hclust(oracle_dist(af))[0], 12, 3)
    assert clones == [f"{b}\t{c}" for b, c in zip(g.whitelist, want.tolist())]
    # the matrix merged from two parts gives the same files
    _, two = _pipeline(tmp_path, "two", cluster=True, clones=3, devices=[0, 0], **LOW)
    for rel in new:
        assert (two / rel).read_bytes() == (out / rel).read_bytes(), rel
    # without --clones no clone file
    _, noclones = _pipeline(tmp_path, "noclones", cluster=True, **LOW)
    assert [f for f in _files(noclones) if f not in _files(plain)] == sorted(CLUSTER_FILES)
    # K above the number of cells: raised after every other output was written
    from mgatk2_amd.exceptions import InvalidInputError

    with pytest.raises(InvalidInputError, match="clones must be in 1..12"):
        _pipeline(tmp_path, "toomany", cluster=True, clones=13, **LOW)
    assert [f for f in _files(tmp_path / "toomany" / "out")] == _files(plain)


def test_pipeline_without_variants_writes_no_cluster_files(tmp_path, oracle_lib, monkeypatch, caplog):
    import logging

    _patch_run(monkeypatch, oracle_lib, variants=False)
    calls = stand_in_device(monkeypatch)
    with caplog.at_level(logging.INFO, logger="mgatk2_amd"):
        _, out = _pipeline(tmp_path, "empty", cluster=True, clones=2, **LOW)
    assert calls == [] and "Clustering skipped: 0 variants x 12 cells" in caplog.text
    assert [f for f in _files(out) if f.startswith("variants")] == ["variants/variant_stats.tsv"]
