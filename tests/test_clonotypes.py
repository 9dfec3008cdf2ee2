"""The cells' clonotypes, host side (no GPU): the plain-Python model of the definition in
include/mgpileup.h (tests/louvain_model.py) on hand graphs with the partitions written out,
modularity() against networkx, the model's quality against networkx's Louvain on planted SNN
graphs built with the numpy oracle of test_neighbors, the small helpers, every refusal, the CLI
options, the pipeline's keywords and the file writers.

tests/test_gpu_clonotypes.py compares the device with the model, bit for bit.
"""

from __future__ import annotations

import inspect
import logging

import numpy as np
import pytest

from louvain_model import Model, louvain, number_labels, score
from test_cluster import _cli, oracle_dist, partition
from test_neighbors import oracle_knn, oracle_snn

ONE = 1 << 20
CLONOTYPE_FILES = ["variants/cell_clonotypes.tsv", "variants/clonotypes.tsv"]


# ---- graphs ------------------------------------------------------------------------------
def clique(vertices, w=ONE):
    v = list(vertices)
    return [(v[a], v[b], w) for a in range(len(v)) for b in range(a + 1, len(v))]


def arrays(edges):
    """(i, j, wq) int arrays of a list of (i, j, wq)."""
    e = np.array(edges, np.int64).reshape(-1, 3)
    return e[:, 0], e[:, 1], e[:, 2]


HAND = {
    # name: (n, edges, the partition the definition gives at resolution 1)
    "one_edge": (2, [(0, 1, ONE)], [[0, 1]]),
    "path3": (3, [(0, 1, ONE), (1, 2, ONE)], [[0, 1, 2]]),
    "two_triangles": (6, clique([0, 1, 2]) + clique([3, 4, 5]) + [(2, 3, ONE)], [[0, 1, 2], [3, 4, 5]]),
    "cliques_1_2_5_70": (78, clique([1, 2]) + clique(range(3, 8)) + clique(range(8, 78)),
                         [[0], [1, 2], list(range(3, 8)), list(range(8, 78))]),
}


def hub_graph(degree, seed):
    """A hub (vertex 0) of `degree` leaves in linked pairs, the weights random integers: the hub's
    row names many communities once the pairs have joined."""
    rng = np.random.default_rng(seed)
    edges = [(0, v, int(rng.integers(1, ONE + 1))) for v in range(1, degree + 1)]
    edges += [(v, v + 1, int(rng.integers(ONE // 2, ONE + 1))) for v in range(1, degree, 2)]
    return degree + 1, edges


def star(leaves):
    return leaves + 1, [(0, v, 1 + (v * 7919) % ONE) for v in range(1, leaves + 1)]


def coarse_hub():
    """200 cliques of 4, each tied by one light edge to one central clique of 8: once the cliques
    have collapsed, the central vertex of the next level has 200 neighbours."""
    edges = clique(range(8))
    for q in range(200):
        base = 8 + 4 * q
        edges += clique(range(base, base + 4)) + [(q % 8, base, ONE // 16)]
    return 8 + 800, edges


def planted_matrix(n, K, seed, clones=True):
    """([n_variants, n] heteroplasmy, the planted labels): clones of K + 1 .. K + 1 + K // 4 cells
    (a short rest joins the last), three private variants each at 0.6, everything under a little
    noise. Separable at the resolutions 0.5, 1 and 2: a clone is larger than K, so a cell's K - 1
    nearest others are of its own clone and no SNN edge leaves a clone (merging two never pays);
    and it is at most 5/4 K, so those K - 1 are most of the clone and its SNN graph is close to
    a uniform clique, which of a share a of the weight loses a / 2 and wins resolution a^2 / 2 by
    splitting in halves: with five clones or more, a <= 1/4 and even resolution 2 does not pay.
    clones=False: noise alone."""
    rng = np.random.default_rng(seed)
    labels, c = [], 0
    while len(labels) < n:
        size = int(rng.integers(K + 1, K + 2 + K // 4))
        if n - len(labels) - size < K + 1:
            size = n - len(labels)
        labels += [c] * size
        c += 1
    labels = np.array(labels)
    if not clones:
        return np.abs(rng.normal(0.0, 0.05, (12, n))), np.zeros(n, np.int64)
    af = np.abs(rng.normal(0.0, 0.01, (3 * c, n)))
    for k in range(c):
        af[3 * k: 3 * k + 3, labels == k] = 0.6 + rng.normal(0.0, 0.03, (3, int((labels == k).sum())))
    return af, labels


def planted_snn(n, K, seed, clones=True):
    """(i, j, wq, planted labels) of the SNN graph (Seurat's defaults) of a planted matrix, by the
    numpy oracle."""
    from mgatk2_amd.analysis.clonotypes import quantise
    from mgatk2_amd.analysis.neighbors import min_shared_for

    af, labels = planted_matrix(n, K, seed, clones)
    idx, _ = oracle_knn(oracle_dist(af), min(K - 1, n - 1))
    kk = idx.shape[1] + 1
    i, j, s = oracle_snn(idx, min_shared_for(kk, 1 / 15))
    return i, j, quantise(s / (2.0 * kk - s)), labels


def knn_graph(n, k, seed):
    """(i, j, wq) of a structureless graph: the symmetrised kNN graph of n random points in the
    plane, each pair once, the weights integers spread over 1..2^20."""
    x = np.random.default_rng(seed).random((2, n))
    idx, _ = oracle_knn(oracle_dist(x), k)
    pairs = sorted({(min(v, int(u)), max(v, int(u))) for v in range(n) for u in idx[v]})
    i, j = np.array(pairs, np.int64).T
    return i, j, 1 + (i * 7919 + j * 104729) % ONE


def same_partition(a, b):
    return partition(a) == partition(b)


def labels_of(groups, n):
    """The label of each vertex from a partition written as lists of members."""
    return [next(k for k, c in enumerate(groups) if v in c) for v in range(n)]


def members(labels):
    """A labelling as a list of member sets."""
    out = {}
    for v, c in enumerate(labels):
        out.setdefault(int(c), set()).add(v)
    return list(out.values())


_planted = {}


def planted_case(name):
    """The three planted graphs of the quality test and their models, made once."""
    spec = {"small": (130, 5, 1, True), "medium": (600, 20, 2, True), "structureless": (400, 20, 3, False)}[name]
    if name not in _planted:
        i, j, wq, labels = planted_snn(*spec)
        _planted[name] = (spec[0], i, j, wq, labels, louvain(spec[0], i, j, wq))
    return _planted[name]


# ---- the model on hand graphs ------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_model_on_hand_graphs(name):
    n, edges, want = HAND[name]
    m = louvain(n, *arrays(edges))
    assert same_partition(m.labels, labels_of(want, n))
    assert m.n_communities == len(want)
    assert m.m2 == 2 * sum(w for _, _, w in edges)
    # the integers are those of the partition, and Q the definition's expression of them
    tot = [sum(w for a, b, w in edges for v in (a, b) if v in c) for c in want]
    assert m.b == sum(t * t for t in tot)
    assert m.internal == 2 * sum(w for a, b, w in edges if any(a in c and b in c for c in want))
    assert m.modularity == score(m.m2, m.internal, m.b, 1.0) / float(m.m2) / float(m.m2)
    assert m.levels[0][0] == n and m.levels[-1][1] == len(want)
    assert all(acc <= p for _, _, p, acc in m.levels)


def test_model_hand_details():
    m = louvain(2, [0], [1], [ONE])
    assert m.labels == [0, 0] and m.modularity == 0.0 and m.levels == [(2, 1, 3, 1)]
    m = louvain(3, [0, 1], [1, 2], [ONE, ONE])
    assert m.labels == [0, 0, 0] and m.levels == [(3, 1, 5, 2)]  # 1 -> 0 and 2 -> 1, then 2 follows
    m = louvain(2, [], [], [])
    assert m.labels == [0, 1] and m.n_communities == 2 and m.modularity == 0.0 and m.levels == []
    assert (m.m2, m.internal, m.b) == (0, 0, 0)
    n, edges, _ = HAND["cliques_1_2_5_70"]
    m = louvain(n, *arrays(edges))
    assert m.labels[8] == 0 and m.labels[3] == 1 and m.labels[1] == 2 and m.labels[0] == 3  # by size
    n, edges = coarse_hub()
    m = louvain(n, *arrays(edges))
    assert m.levels[0][:2] == (808, 201) and len(m.levels) >= 2  # level 1: the hub of 200 neighbours


def test_final_numbering():
    assert number_labels([7, 7, 3, 3, 3, 9]) == [1, 1, 0, 0, 0, 2]
    assert number_labels([5, 4, 5, 4]) == [0, 1, 0, 1]  # equal sizes: by smallest member
    assert number_labels([]) == []


def test_caps_are_honoured():
    n, i, j, wq, _, full = planted_case("structureless")
    assert len(full.levels) >= 2 and full.levels[0][2] > 2
    m = louvain(n, i, j, wq, max_passes=2)
    assert all(p <= 2 for _, _, p, _ in m.levels)
    m = louvain(n, i, j, wq, max_levels=1)
    assert m.levels == full.levels[:1] and m.n_communities == full.levels[0][1]
    # the structureless kNN graph of the device test: the cap of 4 is hit and a pass is undone
    m = louvain(300, *knn_graph(300, 10, 7), max_passes=4)
    assert m.levels[0][2] == 4 and any(acc < p for _, _, p, acc in m.levels)


# ---- modularity() ------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0])
def test_modularity_equals_networkx(gamma):
    import networkx as nx

    from mgatk2_amd.analysis.clonotypes import modularity

    rng = np.random.default_rng(11)
    for name in ("small", "medium"):
        n, i, j, wq, _, m = planted_case(name)
        g = nx.Graph()
        g.add_nodes_from(range(n))
        g.add_weighted_edges_from((int(a), int(b), int(w) / ONE) for a, b, w in zip(i, j, wq))
        for labels in (louvain(n, i, j, wq, gamma).labels, rng.integers(0, 7, n).tolist()):
            comms = members(labels)
            want = nx.community.modularity(g, comms, weight="weight", resolution=gamma)
            assert abs(modularity(n, i, j, wq, labels, gamma) - want) <= 1e-12
        own = louvain(n, i, j, wq, gamma)
        assert modularity(n, i, j, wq, own.labels, gamma) == own.modularity  # the same expression
    assert modularity(3, [], [], [], [0, 1, 2]) == 0.0
    # fp64 weights are quantised on the way in
    assert modularity(2, [0], [1], [0.25], [0, 0]) == modularity(2, [0], [1], [ONE // 4], [0, 0]) == 0.0


# ---- quality -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "medium", "structureless"])
def test_quality_against_networkx(name):
    """The model's Q is at least the lowest Q of networkx's Louvain over seeds 0..4 minus 0.01
    (a cap, not a target); where clones are planted they come back exactly."""
    import networkx as nx

    n, i, j, wq, planted, m = planted_case(name)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_weighted_edges_from((int(a), int(b), int(w) / ONE) for a, b, w in zip(i, j, wq))
    qs = [nx.community.modularity(g, nx.community.louvain_communities(g, weight="weight", resolution=1.0, seed=s),
                                  weight="weight") for s in range(5)]
    print(f"{name}: n={n} edges={len(i)} model Q={m.modularity:.6f} networkx Q={min(qs):.6f}..{max(qs):.6f} "
          f"levels={m.levels}")
    assert m.modularity >= min(qs) - 0.01
    if name != "structureless":
        assert same_partition(m.labels, planted)
    else:
        assert m.n_communities > 1  # (a structureless graph still splits; networkx's does too)


# ---- helpers -----------------------------------------------------------------------------
def test_quantise():
    from mgatk2_amd.analysis.clonotypes import WEIGHT_ONE, quantise
    from mgatk2_amd.exceptions import InvalidInputError

    assert WEIGHT_ONE == ONE
    for K in (2, 20, 65):
        for s in range(1, K + 1):
            w = float(s) / float(2 * K - s)
            q = int(quantise(np.array([w]))[0])
            assert q == (s * ONE * 2 + (2 * K - s)) // (2 * (2 * K - s))  # floor(w 2^20 + 1/2) in integers
            assert 1 <= q <= ONE and abs(q / ONE - w) <= 2.0 ** -21
        assert int(quantise(np.array([1.0]))[0]) == ONE
    assert quantise(np.zeros(0)).shape == (0,)
    with pytest.raises(InvalidInputError):
        quantise(np.array([np.nan]))


def test_refusals_without_a_device(monkeypatch):
    from mgatk2_amd import engine
    from mgatk2_amd.analysis.clonotypes import communities, modularity
    from mgatk2_amd.exceptions import InvalidInputError

    def no_device(*a, **k):
        raise AssertionError("the device was called")

    monkeypatch.setattr(engine, "graph_louvain", no_device)
    ok = dict(n=4, i=[0, 1], j=[1, 2], weight=[ONE, 5])
    bad = [dict(ok, n=(1 << 20) + 1), dict(ok, n=-1), dict(ok, i=[1, 1], j=[1, 2]), dict(ok, i=[2, 1], j=[1, 2]),
           dict(ok, j=[1, 4]), dict(ok, i=[-1, 1]), dict(ok, i=[0, 0], j=[1, 1]), dict(ok, weight=[0, 5]),
           dict(ok, weight=[ONE + 1, 5]), dict(ok, weight=[0.0, 0.5]), dict(ok, weight=[1.5, 0.5]),
           dict(ok, weight=[np.nan, 0.5]), dict(ok, weight=[ONE]), dict(ok, i=[0.5, 1.0]),
           dict(ok, resolution=0.0), dict(ok, resolution=-1.0), dict(ok, resolution=np.inf),
           dict(ok, resolution=np.nan), dict(ok, max_levels=0), dict(ok, max_levels=65), dict(ok, max_passes=0),
           dict(ok, max_passes=(1 << 16) + 1)]
    for kw in bad:
        with pytest.raises(InvalidInputError):
            communities(**kw)
    with pytest.raises(InvalidInputError):
        modularity(4, [0, 0], [1, 1], [ONE, ONE], [0, 0, 0, 0])
    with pytest.raises(InvalidInputError):
        modularity(4, [0], [1], [ONE], [0, 0, 0])
    with pytest.raises(AssertionError, match="the device was called"):
        communities(**ok)  # (a valid call gets as far as the device)


def test_c_entry_refuses_before_any_device_call():
    import ctypes as C

    from mgatk2_amd import engine
    from mgatk2_amd.build import build_engine

    build_engine()
    lib = engine.load_library()
    i, j, w = (np.array(a, np.int32) for a in ([0], [1], [ONE]))
    labels, sums, levels = np.zeros(2, np.int32), np.zeros(4, np.uint64), np.zeros((64, 4), np.int64)
    nc, nl, q = C.c_int64(-1), C.c_int32(-1), C.c_double(0.0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(n=2, ne=1, ei=i, ej=j, ew=w, gamma=1.0, ml=32, mp=64, lab=labels, pnc=C.byref(nc), pq=C.byref(q),
             sm=sums, pnl=C.byref(nl), lv=levels):
        return lib.mgp_louvain(0, n, ne, p(ei), p(ej), p(ew), gamma, ml, mp, p(lab), pnc, pq, p(sm), pnl, p(lv))

    cases = [(dict(ei=None), "bad arguments"), (dict(ej=None), "bad arguments"), (dict(ew=None), "bad arguments"),
             (dict(lab=None), "bad arguments"), (dict(pnc=None), "bad arguments"), (dict(pq=None), "bad arguments"),
             (dict(sm=None), "bad arguments"), (dict(pnl=None), "bad arguments"), (dict(lv=None), "bad arguments"),
             (dict(n=-1), "bad arguments"), (dict(ne=-1), "bad arguments"),
             (dict(n=(1 << 20) + 1), "more than 2^20 vertices"), (dict(ne=(1 << 30) + 1), "more than 2^30 edges"),
             (dict(gamma=0.0), "resolution"), (dict(gamma=-2.0), "resolution"), (dict(gamma=float("inf")), "resolution"),
             (dict(gamma=float("nan")), "resolution"), (dict(ml=0), "max_levels"), (dict(ml=65), "max_levels"),
             (dict(mp=0), "max_passes"), (dict(mp=(1 << 16) + 1), "max_passes"), (dict(n=1), "two vertices")]
    for kw, text in cases:
        assert call(**kw) == engine.MGP_E_INVALID, kw
        assert text in lib.mgp_last_error().decode(), kw
    # no edge: nothing to launch, so it answers without a device
    lab3 = np.full(3, -1, np.int32)
    assert call(n=3, ne=0, ei=None, ej=None, ew=None, lab=lab3) == engine.MGP_OK
    assert lab3.tolist() == [0, 1, 2] and nc.value == 3 and nl.value == 0 and q.value == 0.0 and not sums.any()
    assert call(n=0, ne=0, ei=None, ej=None, ew=None, lab=None) == engine.MGP_OK and nc.value == 0
    r = engine.graph_louvain(2, [], [], [])
    assert r["labels"].tolist() == [0, 1] and r["levels"] == [] and (r["m2"], r["internal"], r["b"]) == (0, 0, 0)
    assert engine.LOUVAIN_WAVE_ROW == 64 and engine.LOUVAIN_LDS_ROW == 2048
    assert "mgp_louvain" in engine.ABI_SYMBOLS and engine.ABI_VERSION == 7


# ---- find_clonotypes and the writers -----------------------------------------------------
def stand_in_device(monkeypatch):
    """The model behind engine.graph_louvain, and a trivial order behind the tree."""
    from mgatk2_amd import engine
    from mgatk2_amd.analysis import clustering

    calls = []

    def graph_louvain(n, i, j, wq, resolution=1.0, max_levels=32, max_passes=64, device=0):
        calls.append(("louvain", int(n), float(resolution), device))
        m = louvain(n, i, j, wq, resolution, max_levels, max_passes)
        return {"labels": np.array(m.labels, np.int32), "n_communities": m.n_communities,
                "modularity": m.modularity, "m2": m.m2, "internal": m.internal, "b": m.b, "levels": m.levels}

    def hclust(x=None, dist=None, device=0):
        n = x.shape[1]
        calls.append(("hclust", x.shape, device))
        return clustering.HClust(np.zeros((n - 1, 2), np.int32), np.zeros(n - 1), np.arange(n, 0, -1).astype(np.int32),
                                 n)

    monkeypatch.setattr(engine, "graph_louvain", graph_louvain)
    monkeypatch.setattr(clustering, "hclust", hclust)
    return calls


def test_find_clonotypes_and_files(tmp_path, monkeypatch, caplog):
    from mgatk2_amd import analysis
    from mgatk2_amd.analysis.clonotypes import Clonotypes, Communities, find_clonotypes, write_clonotype_outputs
    from mgatk2_amd.analysis.neighbors import NeighborGraph
    from mgatk2_amd.exceptions import InvalidInputError

    assert analysis.find_clonotypes is find_clonotypes and analysis.communities and analysis.modularity
    calls = stand_in_device(monkeypatch)
    n, edges, want = HAND["cliques_1_2_5_70"]
    i, j, wq = arrays(edges)
    g = NeighborGraph(n, 20, np.zeros((n, 1), np.int32), np.zeros((n, 1)), i.astype(np.int32), j.astype(np.int32),
                      None, wq / ONE)
    af = np.zeros((2, n))
    af[0, 8:] = 0.5
    af[1, 3:8] = 0.25
    c = find_clonotypes(g, af, resolution=1.0, device=3)
    assert calls == [("louvain", n, 1.0, 3), ("hclust", (2, 4), 3)]
    assert same_partition(c.result.labels, labels_of(want, n))
    assert c.n_cells.tolist() == [70, 5, 2, 1] and c.rank.tolist() == [4, 3, 2, 1]  # (the stand-in's order, reversed)
    np.testing.assert_array_equal(c.mean_af, [[0.5, 0, 0, 0], [0, 0.25, 0, 0]])
    barcodes = [f"BC{v:02d}-1" for v in range(n)]
    vdir = write_clonotype_outputs(c, barcodes, tmp_path)
    assert sorted(p.name for p in vdir.iterdir()) == ["cell_clonotypes.tsv", "clonotypes.tsv"]
    lines = (vdir / "cell_clonotypes.tsv").read_text().splitlines()
    assert lines[0] == "barcode\tclonotype" and lines[1] == "BC00-1\t4" and lines[2] == "BC01-1\t3"
    assert lines[4] == "BC03-1\t2" and lines[9:] == [f"BC{v:02d}-1\t1" for v in range(8, 78)]
    assert (vdir / "clonotypes.tsv").read_text() == "clonotype\tn_cells\trank\n1\t70\t4\n2\t5\t3\n3\t2\t2\n4\t1\t1\n"
    # without the matrix: no means, the rank is the clonotype's number
    c = find_clonotypes(g)
    assert c.mean_af is None and c.rank is None
    write_clonotype_outputs(c, barcodes, tmp_path / "b")
    assert (tmp_path / "b" / "variants" / "clonotypes.tsv").read_text().splitlines()[1:] == \
        ["1\t70\t1", "2\t5\t2", "3\t2\t3", "4\t1\t4"]
    # one clonotype has rank 1 and needs no tree
    del calls[:]
    one = NeighborGraph(2, 2, np.zeros((2, 1), np.int32), np.zeros((2, 1)), np.array([0], np.int32),
                        np.array([1], np.int32), None, np.array([1.0]))
    c = find_clonotypes(one, np.ones((3, 2)))
    assert c.rank.tolist() == [1] and [x[0] for x in calls] == ["louvain"]
    # no graph: no result, nothing written, logged
    with caplog.at_level(logging.INFO, logger="mgatk2_amd"):
        c = find_clonotypes(NeighborGraph(1, 20, None, None))
    assert c.result is None and "Clonotypes skipped" in caplog.text
    write_clonotype_outputs(c, barcodes[:1], tmp_path / "c")
    assert list((tmp_path / "c" / "variants").iterdir()) == []
    with pytest.raises(InvalidInputError):
        find_clonotypes(g, np.zeros((2, n + 1)))
    with pytest.raises(InvalidInputError):
        write_clonotype_outputs(Clonotypes(3, Communities(np.zeros(3, np.int32), 1, 0.0), n_cells=np.array([3])),
                                barcodes[:2], tmp_path / "d")


# ---- CLI and signatures ------------------------------------------------------------------
@pytest.mark.parametrize("cmd", ["run", "tenx"])
def test_cli_clonotype_options(cmd, tmp_path, monkeypatch):
    base = ["--variants", "--neighbors", "10"]
    r, seen = _cli(tmp_path, monkeypatch, [cmd, *base])
    assert r.exit_code == 0 and "clonotypes" not in seen and "clonotype_resolution" not in seen  # off unless asked
    r, seen = _cli(tmp_path, monkeypatch, [cmd, *base, "--clonotypes"])
    assert r.exit_code == 0 and seen["clonotypes"] is True and "clonotype_resolution" not in seen
    assert seen["neighbors"] == 10 and "cluster" not in seen  # independent of --cluster
    r, seen = _cli(tmp_path, monkeypatch, [cmd, *base, "--clonotypes", "--clonotype-resolution", "0.5"])
    assert r.exit_code == 0 and seen["clonotypes"] is True and seen["clonotype_resolution"] == 0.5
    for args, text in ((["--variants", "--clonotypes"], "--clonotypes requires --neighbors"),
                       ([*base, "--clonotype-resolution", "2"], "--clonotype-resolution requires --clonotypes"),
                       ([*base, "--clonotypes", "--clonotype-resolution", "0"], "--clonotype-resolution"),
                       ([*base, "--clonotypes", "--clonotype-resolution", "-1"], "--clonotype-resolution"),
                       ([*base, "--clonotypes", "--clonotype-resolution", "inf"], "--clonotype-resolution"),
                       ([*base, "--clonotypes", "--clonotype-resolution", "nan"], "--clonotype-resolution")):
        r, seen = _cli(tmp_path, monkeypatch, [cmd, *args])
        assert r.exit_code == 2 and text in r.output and seen == {}, (args, r.output)
    r, _ = _cli(tmp_path, monkeypatch, [cmd, "--help"])
    assert "--clonotypes" in r.output and "--clonotype-resolution" in r.output


def test_cli_call_takes_the_clonotype_options(tmp_path, monkeypatch):
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
    base = ["call", "-i", str(tmp_path / "bams"), "-o", str(tmp_path / "o"), "--variants"]
    r = CliRunner().invoke(cli_mod.cli, [*base, "--neighbors", "5", "--clonotypes", "--clonotype-resolution", "2"])
    assert r.exit_code == 0, r.output
    assert len(seen) == 1 and seen[0]["clonotypes"] is True and seen[0]["clonotype_resolution"] == 2.0
    for args, text in ((["--clonotypes"], "--clonotypes requires --neighbors"),
                       (["--neighbors", "5", "--clonotype-resolution", "2"],
                        "--clonotype-resolution requires --clonotypes")):
        r = CliRunner().invoke(cli_mod.cli, [*base, *args])
        assert r.exit_code == 2 and text in r.output and len(seen) == 1


def test_cli_dry_run_prints_the_setting(tmp_path, monkeypatch, caplog):
    with caplog.at_level(logging.INFO, logger="mgatk2_amd"):
        r, seen = _cli(tmp_path, monkeypatch, ["run", "--variants", "--neighbors", "10", "--clonotypes", "--dry-run"])
    assert r.exit_code == 0 and seen == {}
    assert "Clonotypes:" in caplog.text and "resolution 1.0" in caplog.text


def test_pipeline_keywords_default_off_and_checked(tmp_path):
    from mgatk2_amd.engine import EngineResult
    from mgatk2_amd.exceptions import InvalidInputError
    from mgatk2_amd.pipeline import MtDNAPipeline, run_pipeline
    from mgatk2_amd.processing.processors import CellProcessor

    for fn in (run_pipeline, MtDNAPipeline.__init__):
        sig = inspect.signature(fn).parameters
        assert sig["clonotypes"].default is False and sig["clonotype_resolution"].default == 1.0
    on = dict(call_variants=True, neighbors=10)
    for kw in (dict(call_variants=True, clonotypes=True), dict(on, clonotype_resolution=2.0),
               dict(on, clonotypes=True, clonotype_resolution=0.0),
               dict(on, clonotypes=True, clonotype_resolution=float("nan"))):
        with pytest.raises(InvalidInputError):
            MtDNAPipeline("no.bam", ["A"], tmp_path, **kw)
    proc = CellProcessor(None, tmp_path)
    proc.enable_variants()
    with pytest.raises(InvalidInputError):
        proc.enable_clonotypes()
    proc.enable_neighbors(10)
    with pytest.raises(InvalidInputError):
        proc.enable_clonotypes(0.0)
    assert proc.clonotypes_opt is None
    proc.enable_clonotypes(0.5)
    assert proc.clonotypes_opt == {"resolution": 0.5}
    assert "clonotypes" in {f.name for f in __import__("dataclasses").fields(EngineResult)}
    assert CellProcessor(None, tmp_path).clonotype_result(None) is None  # not enabled: nothing
    assert isinstance(louvain(1, [], [], []), Model)
