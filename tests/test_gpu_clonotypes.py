"""Louvain communities on the device (mgp_louvain, mgp_louvain.hip) against the plain-Python model
of the definition (tests/louvain_model.py): the labels, the bytes of Q, the integers M2, I, B and
every level tuple are equal, on every call.

The sizes follow the move kernel's shapes: a row of at most 64 entries is a wave's (a vertex of
degree 63, 64, 65), a row of at most 2,048 a workgroup's with the table in LDS (a hub of 2,047,
2,048, 2,049 leaves), longer rows use the table in global memory; the environment's thresholds
push the small graphs through the two table paths as well. 200 cliques around a central clique
give a hub at a coarse level.
"""

from __future__ import annotations

import numpy as np
import pytest

from louvain_model import louvain
from test_clonotypes import (CLONOTYPE_FILES, HAND, ONE, arrays, coarse_hub, hub_graph, knn_graph, labels_of,
                             planted_matrix, same_partition, star)
from test_gpu_variants import _files, _pipeline, _same_file
from test_neighbors import GRAPH_FILES

pytestmark = pytest.mark.gpu

LOW = dict(call_variants=True, variant_min_cells=0, variant_min_strand_cor=-1.0, variant_min_vmr=0.0)
ENV = ("MGP_LOUVAIN_WAVE_ROW", "MGP_LOUVAIN_LDS_ROW")


def equal_to_model(engine, n, edges, gamma=1.0, **caps):
    """The device's result, equal to the model's in every output, twice over."""
    i, j, wq = arrays(edges) if isinstance(edges, list) else edges
    want = louvain(n, i, j, wq, gamma, **caps)
    got = engine.graph_louvain(n, i, j, wq, gamma, **caps)
    assert got["labels"].dtype == np.int32 and got["labels"].tolist() == want.labels
    assert got["n_communities"] == want.n_communities
    assert np.float64(got["modularity"]).tobytes() == np.float64(want.modularity).tobytes()
    assert (got["m2"], got["internal"], got["b"]) == (want.m2, want.internal, want.b)
    assert got["levels"] == want.levels
    again = engine.graph_louvain(n, i, j, wq, gamma, **caps)
    assert again["labels"].tobytes() == got["labels"].tobytes() and again["levels"] == got["levels"]
    assert np.float64(again["modularity"]).tobytes() == np.float64(got["modularity"]).tobytes()
    assert (again["m2"], again["internal"], again["b"]) == (got["m2"], got["internal"], got["b"])
    return got, want


@pytest.fixture
def default_thresholds(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_graphs(engine_lib, default_thresholds, name):
    n, edges, want = HAND[name]
    got, _ = equal_to_model(engine_lib, n, edges)
    assert same_partition(got["labels"], labels_of(want, n))


def test_no_edge_launches_nothing(engine_lib, default_thresholds):
    got, _ = equal_to_model(engine_lib, 2, (np.zeros(0, np.int64),) * 3)
    assert got["labels"].tolist() == [0, 1] and got["levels"] == [] and got["modularity"] == 0.0


@pytest.mark.parametrize("degree", [63, 64, 65])
def test_rows_around_the_wave_threshold(engine_lib, default_thresholds, degree):
    assert engine_lib.LOUVAIN_WAVE_ROW == 64
    for gamma in (0.5, 1.0, 2.0):
        equal_to_model(engine_lib, *hub_graph(degree, degree), gamma)


@pytest.mark.parametrize("leaves", [2047, 2048, 2049])
def test_hub_around_the_lds_capacity(engine_lib, default_thresholds, leaves):
    assert engine_lib.LOUVAIN_LDS_ROW == 2048
    equal_to_model(engine_lib, *star(leaves))
    equal_to_model(engine_lib, *hub_graph(leaves, leaves))


@pytest.mark.parametrize("wave_row, lds_row", [("0", "2048"), ("0", "0"), ("3", "5"), ("64", "0")])
def test_forced_paths_change_nothing(engine_lib, monkeypatch, wave_row, lds_row):
    """Every row through the workgroup path (LDS table), then through the global table, then a mix
    of the three on short rows: the thresholds are read on every call and change no output."""
    monkeypatch.setenv("MGP_LOUVAIN_WAVE_ROW", wave_row)
    monkeypatch.setenv("MGP_LOUVAIN_LDS_ROW", lds_row)
    for name in sorted(HAND):
        equal_to_model(engine_lib, *HAND[name][:2])
    equal_to_model(engine_lib, *hub_graph(65, 65))
    equal_to_model(engine_lib, *coarse_hub())
    equal_to_model(engine_lib, 300, knn_graph(300, 10, 7), max_passes=4)


def test_hub_at_a_coarse_level(engine_lib, default_thresholds):
    got, want = equal_to_model(engine_lib, *coarse_hub())
    assert got["levels"][0][:2] == (808, 201) and len(got["levels"]) >= 2  # level 1: a vertex of 200 neighbours


@pytest.mark.parametrize("n, K", [(65, 5), (130, 20), (1100, 65)])
def test_planted_snn_graphs(engine_lib, default_thresholds, n, K):
    from mgatk2_amd.analysis.clonotypes import communities, quantise
    from mgatk2_amd.analysis.neighbors import neighbor_graph

    af, planted = planted_matrix(n, K, 1000 * n + K)
    g = neighbor_graph(af, neighbors=K)
    wq = quantise(g.weight)
    assert len(g.i) > n
    for gamma in (0.5, 1.0, 2.0):
        got, _ = equal_to_model(engine_lib, n, (g.i, g.j, wq), gamma)
        assert same_partition(got["labels"], planted), gamma  # (an adjusted Rand index of 1)
        c = communities(n, g.i, g.j, g.weight, gamma)  # the public call quantises the same way
        assert c.labels.tobytes() == got["labels"].tobytes() and c.modularity == got["modularity"]
        assert (c.m2, c.internal, c.b, c.levels) == (got["m2"], got["internal"], got["b"], got["levels"])


def test_structureless_graph_hits_the_pass_cap(engine_lib, default_thresholds):
    got, _ = equal_to_model(engine_lib, 300, knn_graph(300, 10, 7), max_passes=4)
    assert got["levels"][0][2] == 4  # the cap is hit
    assert any(acc < p for _, _, p, acc in got["levels"])  # an undone pass
    equal_to_model(engine_lib, 300, knn_graph(300, 10, 7), max_levels=1)
    equal_to_model(engine_lib, 300, knn_graph(300, 10, 7))


def test_refusals_on_the_device(engine_lib, default_thresholds):
    from mgatk2_amd.exceptions import InvalidInputError

    n, edges, _ = HAND["two_triangles"]
    i, j, wq = (np.array(a, np.int32) for a in arrays(edges))
    ok = engine_lib.graph_louvain(n, i, j, wq)

    def changed(arr, at, v):
        out = arr.copy()
        out[at] = v
        return out

    for args, text in (((np.append(i, 0), np.append(j, 1), np.append(wq, 9)), "repeated"),
                       ((changed(i, 3, 4), j, wq), "i < j"),          # (4, 4): i == j
                       ((changed(i, 0, 2), changed(j, 0, 0), wq), "i < j"),  # (2, 0): i > j
                       ((i, changed(j, 5, n), wq), "i < j"),           # out of range above
                       ((changed(i, 0, -1), j, wq), "i < j"),          # and below
                       ((i, j, changed(wq, 2, 0)), "weight"),
                       ((i, j, changed(wq, 6, ONE + 1)), "weight")):
        with pytest.raises(InvalidInputError, match=text):
            engine_lib.graph_louvain(n, *args)
        again = engine_lib.graph_louvain(n, i, j, wq)  # the next valid call succeeds
        assert again["labels"].tolist() == ok["labels"].tolist() and again["levels"] == ok["levels"]


# ---- the pipeline ------------------------------------------------------------------------
def read_mtx_edges(path):
    """(n, i, j, weight) of the strict lower triangle of cell_snn.mtx, 0-based, i < j."""
    lines = path.read_text().splitlines()
    n = int(lines[1].split()[0])
    ei, ej, w = [], [], []
    for line in lines[2:]:
        r, c, x = line.split()
        if r != c:
            ei.append(int(c) - 1)
            ej.append(int(r) - 1)
            w.append(float(x))
    return n, np.array(ei, np.int64), np.array(ej, np.int64), np.array(w, np.float64)


@pytest.mark.parametrize("fmt", ["txt", "hdf5"])
def test_pipeline_clonotypes(fmt, tmp_path, engine_lib, monkeypatch, default_thresholds):
    """run_pipeline(call_variants, neighbors=10, clonotypes) on the synth_run_h5 golden reads: the two
    new files equal the model run on the cell_snn.mtx the same run wrote, a run sharded over two
    contexts writes the same bytes, every other file is what a run without the flag writes, and
    that run writes exactly the files it wrote before."""
    from mgatk2_amd.analysis.clonotypes import quantise

    g, out = _pipeline(tmp_path, "clono", fmt, monkeypatch, neighbors=10, clonotypes=True, **LOW)
    _, graph = _pipeline(tmp_path, "graph", fmt, monkeypatch, neighbors=10, **LOW)
    _, plain = _pipeline(tmp_path, "plain", fmt, monkeypatch, **LOW)
    assert [f for f in _files(graph) if f not in _files(plain)] == GRAPH_FILES  # as before this flag existed
    assert [f for f in _files(out) if f not in _files(graph)] == CLONOTYPE_FILES
    assert [f for f in _files(out) if f not in CLONOTYPE_FILES] == _files(graph)
    for rel in _files(graph):
        _same_file(out, graph, rel)
    n, i, j, w = read_mtx_edges(out / "variants" / "cell_snn.mtx")
    assert n == len(g.whitelist) and len(i) > 0
    want = louvain(n, i, j, quantise(w))
    cells = (out / "variants" / "cell_clonotypes.tsv").read_text().splitlines()
    assert cells == ["barcode\tclonotype"] + [f"{b}\t{c + 1}" for b, c in zip(g.whitelist, want.labels)]
    table = [line.split("\t") for line in (out / "variants" / "clonotypes.tsv").read_text().splitlines()]
    assert table[0] == ["clonotype", "n_cells", "rank"]
    sizes = np.bincount(want.labels, minlength=want.n_communities)
    assert [(int(a), int(b)) for a, b, _ in table[1:]] == [(k + 1, int(s)) for k, s in enumerate(sizes)]
    assert sorted(int(r) for _, _, r in table[1:]) == list(range(1, want.n_communities + 1))
    _, two = _pipeline(tmp_path, "two", fmt, monkeypatch, devices=[0, 0], neighbors=10, clonotypes=True, **LOW)
    for rel in CLONOTYPE_FILES + GRAPH_FILES:
        assert (two / rel).read_bytes() == (out / rel).read_bytes(), rel
    _, half = _pipeline(tmp_path, "half", fmt, monkeypatch, neighbors=10, clonotypes=True, clonotype_resolution=0.5,
                        **LOW)
    want = louvain(n, i, j, quantise(w), 0.5)
    assert (half / "variants" / "cell_clonotypes.tsv").read_text().splitlines()[1:] == \
        [f"{b}\t{c + 1}" for b, c in zip(g.whitelist, want.labels)]
