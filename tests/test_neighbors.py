"""The cells' kNN and SNN graphs, host side (no GPU): a numpy oracle of the definitions in
include/mgpileup.h (the k smallest of a row of the distance matrix under (value, index) with the
diagonal removed; Seurat's ComputeSNN as the dense product of the membership matrix),
min_shared_for against Seurat's expression, the file writers, the genomic feature order, the
small cases, the CLI options, the ABI and its refusals, and the pipeline's plumbing with the
oracle standing in for the two device calls.

tests/test_gpu_neighbors.py compares the device with this oracle.
"""

from __future__ import annotations

import inspect
import logging
import re
from pathlib import Path

import numpy as np
import pytest

from test_cluster import LOW, _cli, _files, _patch_run, _pipeline, oracle_dist, written_matrix

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("mgp_knn", "mgp_snn")
GRAPH_FILES = ["variants/cell_knn.tsv", "variants/cell_snn.mtx", "variants/cell_snn_barcodes.tsv"]


# ---- the oracle ----------------------------------------------------------------------
def oracle_knn(dist, k):
    """(idx [n, k] int32, dist [n, k]): per row of the matrix the k entries smallest under
    (value, index), the diagonal removed."""
    dist = np.asarray(dist, np.float64)
    n = dist.shape[0]
    idx = np.zeros((n, k), np.int32)
    out = np.zeros((n, k), np.float64)
    cols = np.arange(n)
    for i in range(n):
        order = np.lexsort((cols, dist[i]))
        order = order[order != i][:k]
        idx[i], out[i] = order, dist[i, order]
    return idx, out


def oracle_snn(idx, min_shared):
    """(i, j, shared) int32, i < j, sorted by (i, j): the entries >= min_shared of A A^T above the
    diagonal, A the 0/1 membership matrix of S_i = {i} + idx[i]."""
    idx = np.asarray(idx)
    n = idx.shape[0]
    a = np.zeros((n, n), np.int64)
    a[np.arange(n), np.arange(n)] = 1
    a[np.repeat(np.arange(n), idx.shape[1]), idx.reshape(-1)] = 1
    p = np.triu(a @ a.T, 1)
    i, j = np.nonzero(p >= max(int(min_shared), 1))
    return i.astype(np.int32), j.astype(np.int32), p[i, j].astype(np.int32)


def oracle_weight(shared, K):
    return np.asarray(shared, np.float64) / (2.0 * K - np.asarray(shared, np.float64))


def stand_in_device(monkeypatch):
    """The oracle behind engine.graph_knn / graph_snn: the host logic is testable without a device."""
    from mgatk2_amd import engine

    calls = []

    def graph_knn(x, k, device=0):
        calls.append(("knn", int(k), device))
        return oracle_knn(oracle_dist(x), int(k))

    def graph_snn(idx, min_shared, device=0):
        calls.append(("snn", int(min_shared), device))
        return oracle_snn(idx, min_shared)

    monkeypatch.setattr(engine, "graph_knn", graph_knn)
    monkeypatch.setattr(engine, "graph_snn", graph_snn)
    return calls


def test_oracle_on_a_hand_made_case():
    # points on a line: 0, 1, 3, 3, 10 (items 2 and 3 equal)
    d = oracle_dist(np.array([[0.0, 1.0, 3.0, 3.0, 10.0]]))
    idx, dist = oracle_knn(d, 2)
    assert idx.tolist() == [[1, 2], [0, 2], [3, 1], [2, 1], [2, 3]]  # (ties to the lower index)
    assert dist.tolist() == [[1.0, 3.0], [1.0, 2.0], [0.0, 2.0], [0.0, 2.0], [7.0, 7.0]]
    # S: {0,1,2} {0,1,2} {1,2,3} {1,2,3} {2,3,4}
    i, j, s = oracle_snn(idx, 1)
    got = {(a, b): c for a, b, c in zip(i.tolist(), j.tolist(), s.tolist())}
    assert got == {(0, 1): 3, (0, 2): 2, (0, 3): 2, (0, 4): 1, (1, 2): 2, (1, 3): 2, (1, 4): 1, (2, 3): 3,
                   (2, 4): 2, (3, 4): 2}
    assert list(zip(i.tolist(), j.tolist())) == sorted(got)
    i, j, s = oracle_snn(idx, 3)
    assert list(zip(i.tolist(), j.tolist(), s.tolist())) == [(0, 1, 3), (2, 3, 3)]


# ---- min_shared_for ----------------------------------------------------------------------
def test_min_shared_for_is_seurats_expression():
    from mgatk2_amd.analysis.neighbors import DEFAULT_PRUNE, min_shared_for
    from mgatk2_amd.exceptions import InvalidInputError

    assert DEFAULT_PRUNE == 1.0 / 15.0
    assert min_shared_for(20, 1 / 15) == 3  # 2 / 38 < 1 / 15 <= 3 / 37
    assert min_shared_for(20, 0.0) == 1
    assert min_shared_for(20, 1.0) == 20
    for K in (2, 5, 21, 65):
        for prune in (0.0, 1 / 15, 0.1, 1 / 3, 0.5, 0.999, 1.0):
            s = min_shared_for(K, prune)
            kept = [t for t in range(1, K + 1) if not (float(t) / float(2 * K - t) < prune)]
            assert s == kept[0] and kept == list(range(s, K + 1))
    for K, prune in ((0, 0.1), (5, -0.1), (5, 1.5), (5, float("nan"))):
        with pytest.raises(InvalidInputError):
            min_shared_for(K, prune)


# ---- knn / snn / neighbor_graph behind the stand-in ---------------------------------------
def test_knn_and_snn_small_cases_and_clipping(monkeypatch, caplog):
    from mgatk2_amd import analysis
    from mgatk2_amd.analysis.neighbors import knn, neighbor_graph, snn
    from mgatk2_amd.exceptions import InvalidInputError

    assert analysis.knn is knn and analysis.snn is snn and analysis.neighbor_graph is neighbor_graph
    assert analysis.min_shared_for and analysis.write_neighbor_outputs and analysis.NeighborGraph
    calls = stand_in_device(monkeypatch)
    # n = 0 and 1: empty results, no device call
    for n in (0, 1):
        idx, dist = knn(np.zeros((3, n)), 5)
        assert idx.shape == (n, 0) and idx.dtype == np.int32 and dist.shape == (n, 0) and dist.dtype == np.float64
        i, j, s, w = snn(idx)
        assert i.shape == j.shape == s.shape == w.shape == (0,) and w.dtype == np.float64
    assert calls == []
    # n = 2: each is the other's neighbour, one edge sharing both members
    idx, dist = knn(np.array([[0.0, 3.0], [0.0, 4.0]]), 1)
    assert idx.tolist() == [[1], [0]] and dist.tolist() == [[5.0], [5.0]]
    i, j, s, w = snn(idx, prune=0.0)
    assert (i.tolist(), j.tolist(), s.tolist(), w.tolist()) == ([0], [1], [2], [1.0])
    assert calls == [("knn", 1, 0), ("snn", 1, 0)]
    # k above n - 1 is clipped, with a log line
    del calls[:]
    x = np.random.default_rng(1).random((4, 6))
    with caplog.at_level(logging.INFO, logger="mgatk2_amd.analysis.neighbors"):
        idx, dist = knn(x, 19, device=3)
    assert calls == [("knn", 5, 3)] and idx.shape == (6, 5) and "clipped to 5" in caplog.text
    want = oracle_knn(oracle_dist(x), 5)
    np.testing.assert_array_equal(idx, want[0])
    np.testing.assert_array_equal(dist, want[1])
    # the weight is Seurat's s / (2K - s), one division; the default prune's count is passed on
    del calls[:]
    i, j, s, w = snn(idx, device=2)
    assert calls == [("snn", 1, 2)]  # K = 6: 1 / 11 >= 1 / 15
    wi, wj, ws = oracle_snn(idx, 1)
    for a, b in ((i, wi), (j, wj), (s, ws), (w, oracle_weight(ws, 6))):
        np.testing.assert_array_equal(a, b)
    for bad in (dict(k=0), dict(k=-2)):
        with pytest.raises(InvalidInputError):
            knn(x, **bad)
    with pytest.raises(InvalidInputError):
        knn(np.zeros(5), 2)
    with pytest.raises(InvalidInputError):
        snn(np.zeros(5, np.int32))
    with pytest.raises(InvalidInputError):
        snn(idx, prune=1.5)


def test_neighbor_graph_sides_and_errors(monkeypatch, caplog):
    from mgatk2_amd.analysis.neighbors import GRAPH_MAX_ITEMS, GRAPH_MAX_K, neighbor_graph
    from mgatk2_amd.exceptions import InvalidInputError

    assert GRAPH_MAX_ITEMS == 1 << 20 and GRAPH_MAX_K == 64
    calls = stand_in_device(monkeypatch)
    af = np.random.default_rng(8).random((4, 30))
    g = neighbor_graph(af, neighbors=20, device=2)
    assert calls == [("knn", 19, 2), ("snn", 3, 2)]
    assert g.n == 30 and g.k_param == 20 and g.idx.shape == (30, 19) and g.prune == 1 / 15
    idx, dist = oracle_knn(oracle_dist(af), 19)
    wi, wj, ws = oracle_snn(idx, 3)
    for a, b in ((g.idx, idx), (g.dist, dist), (g.i, wi), (g.j, wj), (g.shared, ws), (g.weight, oracle_weight(ws, 20))):
        np.testing.assert_array_equal(a, b)
    assert np.all(g.weight >= 1 / 15) and set(g.seconds) == {"knn", "snn", "total"}
    # K clipped to the cells: the weights then use the clipped K
    del calls[:]
    g = neighbor_graph(af[:, :7], neighbors=20, prune=0.0)
    assert calls == [("knn", 6, 0), ("snn", 1, 0)] and g.k_param == 7
    np.testing.assert_array_equal(g.weight, oracle_weight(g.shared, 7))
    for kw in (dict(neighbors=1), dict(neighbors=GRAPH_MAX_K + 2), dict(prune=-0.5), dict(prune=2.0),
               dict(barcodes=["a"] * 6), dict(table=["v"] * 3)):
        with pytest.raises(InvalidInputError):
            neighbor_graph(af, **kw)
    with pytest.raises(InvalidInputError):
        neighbor_graph(np.zeros(4))
    # fewer than two cells or no variant: no graph, a log line, no device call
    del calls[:]
    with caplog.at_level(logging.INFO, logger="mgatk2_amd.analysis.neighbors"):
        for shape in ((0, 7), (4, 1), (4, 0), (0, 0)):
            g = neighbor_graph(np.zeros(shape))
            assert g.idx is None and g.i is None and g.n == shape[1]
        assert neighbor_graph(None).idx is None
    assert calls == [] and caplog.text.count("Neighbour graph skipped") == 5
    # one variant is enough
    assert neighbor_graph(np.arange(5.0)[None, :], neighbors=3).idx.tolist()[0] == [1, 2]
    # above the bound: refused before any device call
    del calls[:]
    with pytest.raises(InvalidInputError, match="more than 1048576"):
        neighbor_graph(np.zeros((1, GRAPH_MAX_ITEMS + 1)))
    assert calls == []


def _table(pos, base, perm):
    from mgatk2_amd.analysis.variants import VariantTable

    z = np.zeros(len(perm))
    t = VariantTable(position=pos[perm], base=base[perm], ref=["N"] * len(perm), mean=z, vmr=z, variance=z,
                     n_cells_detected=z, n_cells_conf_detected=z, strand_correlation=z)
    t.variant = [f"{p}N>{'ACGT'[b]}" for p, b in zip(t.position, t.base)]
    return t


def test_features_are_taken_in_genomic_order(tmp_path, monkeypatch):
    """With a VariantTable the features are summed in (position, base) order whatever the table's
    own (vmr) order: the fma chain's order fixes the last bits, so two tables of the same variants
    in different orders, as two shardings of one run can give, write the same files."""
    from mgatk2_amd import engine
    from mgatk2_amd.analysis.neighbors import neighbor_graph, write_neighbor_outputs

    stand_in_device(monkeypatch)
    seen = []
    plain = engine.graph_knn
    monkeypatch.setattr(engine, "graph_knn", lambda x, k, device=0: seen.append(np.array(x)) or plain(x, k, device))
    rng = np.random.default_rng(3)
    pos = np.array([900, 12, 12, 4000, 77, 900])
    base = np.array([2, 3, 0, 1, 1, 0])
    af = rng.random((6, 9)) * np.array([1e-9, 1.0, 1e9, 1.0, 1e-3, 7.0])[:, None]
    barcodes = [f"c{i}" for i in range(9)]
    want_rows = [2, 1, 4, 5, 0, 3]  # (12, A), (12, T), (77, C), (900, A), (900, G), (4000, C)
    outs = []
    for k, perm in enumerate((np.arange(6), np.array([3, 0, 5, 1, 4, 2]))):
        g = neighbor_graph(af[perm], barcodes, _table(pos, base, perm), neighbors=4)
        np.testing.assert_array_equal(seen[-1], af[want_rows])
        outs.append(write_neighbor_outputs(g, barcodes, tmp_path / str(k)))
    for f in sorted(p.name for p in outs[0].iterdir()):
        assert (outs[0] / f).read_bytes() == (outs[1] / f).read_bytes(), f
    # a bare matrix, or names alone: the features in row order
    neighbor_graph(af, table=[str(i) for i in range(6)], neighbors=4)
    np.testing.assert_array_equal(seen[-1], af)


# ---- the files -----------------------------------------------------------------------------
def check_graph_files(vdir, barcodes, idx, dist, edges, K):
    """The three files against a kNN table and the SNN triples (i, j, shared) sorted by (i, j)."""
    from scipy.io import mmread

    n = len(barcodes)
    lines = (vdir / "cell_knn.tsv").read_text().splitlines()
    assert lines[0] == "barcode\trank\tneighbor\tdistance"
    assert lines[1:] == [f"{barcodes[c]}\t{r + 1}\t{barcodes[int(idx[c, r])]}\t{float(dist[c, r])!r}"
                         for c in range(n) for r in range(idx.shape[1])]
    assert (vdir / "cell_snn_barcodes.tsv").read_text() == "".join(b + "\n" for b in barcodes)
    ei, ej, es = edges
    w = oracle_weight(es, K)
    text = (vdir / "cell_snn.mtx").read_text().splitlines()
    assert text[0] == "%%MatrixMarket matrix coordinate real symmetric" and text[1] == f"{n} {n} {n + len(ei)}"
    want = []
    for c in range(n):
        want.append(f"{c + 1} {c + 1} 1.0")
        want += [f"{int(b) + 1} {c + 1} {float(x)!r}" for a, b, x in zip(ei, ej, w) if a == c]
    assert text[2:] == want  # 1-based, the lower triangle, sorted by column, then row
    m = np.asarray(mmread(str(vdir / "cell_snn.mtx")).todense())
    dense = np.eye(n)
    dense[ei, ej] = w
    dense[ej, ei] = w
    np.testing.assert_array_equal(m, dense)  # (repr round-trips fp64)


def test_graph_files_round_trip(tmp_path):
    from mgatk2_amd.analysis.neighbors import NeighborGraph, write_neighbor_outputs

    x = np.random.default_rng(4).integers(0, 3, (3, 17)).astype(np.float64) / 3  # (ties and equal cells)
    idx, dist = oracle_knn(oracle_dist(x), 4)
    ei, ej, es = oracle_snn(idx, 2)
    barcodes = [f"BC{i:02d}-1" for i in range(17)]
    g = NeighborGraph(17, 5, idx, dist, ei, ej, es, oracle_weight(es, 5))
    vdir = write_neighbor_outputs(g, barcodes, tmp_path)
    assert vdir == tmp_path / "variants"
    assert sorted(p.name for p in vdir.iterdir()) == ["cell_knn.tsv", "cell_snn.mtx", "cell_snn_barcodes.tsv"]
    assert len(ei) > 0
    check_graph_files(vdir, barcodes, idx, dist, (ei, ej, es), 5)
    # no graph writes nothing
    write_neighbor_outputs(NeighborGraph(1, 20, None, None), barcodes[:1], tmp_path / "b")
    assert list((tmp_path / "b" / "variants").iterdir()) == []


# ---- CLI and signatures ------------------------------------------------------------------
@pytest.mark.parametrize("cmd", ["run", "tenx"])
def test_cli_neighbor_options(cmd, tmp_path, monkeypatch):
    r, seen = _cli(tmp_path, monkeypatch, [cmd, "--variants"])
    assert r.exit_code == 0 and "neighbors" not in seen and "snn_prune" not in seen  # off unless asked for
    r, seen = _cli(tmp_path, monkeypatch, [cmd, "--variants", "--neighbors", "20"])
    assert r.exit_code == 0 and seen["neighbors"] == 20 and "snn_prune" not in seen and "cluster" not in seen
    r, seen = _cli(tmp_path, monkeypatch, [cmd, "--variants", "--neighbors", "65", "--snn-prune", "0.25", "--cluster"])
    assert r.exit_code == 0 and seen["neighbors"] == 65 and seen["snn_prune"] == 0.25 and seen["cluster"] is True
    for args, text in ((["--neighbors", "20"], "--neighbors requires --variants"),
                       (["--variants", "--snn-prune", "0.1"], "--snn-prune requires --neighbors"),
                       (["--variants", "--neighbors", "1"], "--neighbors"),
                       (["--variants", "--neighbors", "66"], "--neighbors"),
                       (["--variants", "--neighbors", "20", "--snn-prune", "1.5"], "--snn-prune"),
                       (["--variants", "--neighbors", "20", "--snn-prune", "-0.1"], "--snn-prune")):
        r, seen = _cli(tmp_path, monkeypatch, [cmd, *args])
        assert r.exit_code == 2 and text in r.output and seen == {}, (args, r.output)
    r, _ = _cli(tmp_path, monkeypatch, [cmd, "--help"])
    assert "--neighbors" in r.output and "--snn-prune" in r.output


def test_cli_dry_run_prints_the_setting(tmp_path, monkeypatch, caplog):
    with caplog.at_level(logging.INFO, logger="mgatk2_amd"):
        r, seen = _cli(tmp_path, monkeypatch, ["run", "--variants", "--neighbors", "12", "--dry-run"])
    assert r.exit_code == 0 and seen == {}
    assert "Neighbour graph:        k.param 12, SNN prune 1/15" in caplog.text


def test_cli_call_takes_the_neighbor_options(tmp_path, monkeypatch):
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
    r = CliRunner().invoke(cli_mod.cli, [*base, "--variants", "--neighbors", "5", "--snn-prune", "0"])
    assert r.exit_code == 0, r.output
    assert len(seen) == 1 and seen[0]["neighbors"] == 5 and seen[0]["snn_prune"] == 0.0
    for args, text in ((["--neighbors", "5"], "--neighbors requires --variants"),
                       (["--variants", "--snn-prune", "0.5"], "--snn-prune requires --neighbors")):
        r = CliRunner().invoke(cli_mod.cli, [*base, *args])
        assert r.exit_code == 2 and text in r.output and len(seen) == 1


def test_pipeline_keywords_default_off_and_checked(tmp_path):
    from mgatk2_amd.exceptions import InvalidInputError
    from mgatk2_amd.pipeline import MtDNAPipeline, run_pipeline
    from mgatk2_amd.processing.processors import CellProcessor

    for fn in (run_pipeline, MtDNAPipeline.__init__):
        sig = inspect.signature(fn).parameters
        assert sig["neighbors"].default is None and sig["snn_prune"].default == 1 / 15
    for kw in (dict(neighbors=20), dict(call_variants=True, neighbors=1), dict(call_variants=True, neighbors=66),
               dict(call_variants=True, neighbors=20, snn_prune=1.5)):
        with pytest.raises(InvalidInputError):
            MtDNAPipeline("no.bam", ["A"], tmp_path, **kw)
    proc = CellProcessor(None, tmp_path)
    with pytest.raises(InvalidInputError):
        proc.enable_neighbors()
    proc.enable_variants()
    for kw in (dict(neighbors=1), dict(neighbors=66), dict(prune=-1.0)):
        with pytest.raises(InvalidInputError):
            proc.enable_neighbors(**kw)
    proc.enable_neighbors(12, 0.5)
    assert proc.neighbors_opt == {"neighbors": 12, "prune": 0.5}


# ---- ABI -----------------------------------------------------------------------------------
def test_header_and_abi_symbols_list_the_new_names():
    from mgatk2_amd import engine
    from mgatk2_amd.build import HIP_SOURCES, build_engine

    assert "mgp_graph.hip" in HIP_SOURCES
    build_engine()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mgpileup.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(mgp_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    for s in NEW_SYMBOLS:
        assert s in declared and s in engine.ABI_SYMBOLS and hasattr(lib, s), s
        assert not s.endswith("_rows")
    assert lib.mgp_abi_version() == engine.ABI_VERSION == 7
    assert callable(engine.graph_knn) and callable(engine.graph_snn)


def test_graph_calls_refuse_bad_arguments_before_any_device_call():
    """Null or negative arguments and sizes outside the bounds: MGP_E_INVALID with the call's own
    message, before any allocation or device call (so this runs without a device)."""
    import ctypes as C

    from mgatk2_amd import engine
    from mgatk2_amd.build import build_engine

    build_engine()
    lib = engine.load_library()
    x = np.zeros((2, 5))
    idx, dist = np.zeros((5, 2), np.int32), np.zeros((5, 2))
    tri = [np.full(8, -7, np.int32) for _ in range(3)]
    p = lambda a: a.ctypes.data  # noqa: E731
    count = C.c_int64(99)

    def refused(name, text, *args):
        rc = getattr(lib, name)(0, *args)
        assert rc == engine.MGP_E_INVALID, (name, args, rc)
        assert lib.mgp_last_error().decode().startswith(f"{name}: {text}"), (name, args, lib.mgp_last_error())

    # mgp_knn(device, x, n, nf, k, idx, dist)
    for args in ((None, 5, 2, 2, p(idx), p(dist)), (p(x), 5, 2, 2, None, p(dist)), (p(x), 5, 2, 2, p(idx), None),
                 (p(x), -5, 2, 2, p(idx), p(dist)), (p(x), 5, -2, 2, p(idx), p(dist))):
        refused("mgp_knn", "bad arguments", *args)
    for k in (0, -1, 65):
        refused("mgp_knn", "k must be in 1..64", p(x), 5, 2, k, p(idx), p(dist))
    for n, k in ((5, 5), (3, 3), (1, 1), (2, 64)):
        refused("mgp_knn", "k must be at most n_items - 1", p(x), n, 2, k, p(idx), p(dist))
    refused("mgp_knn", "more than 2^20 items in one call", p(x), (1 << 20) + 1, 2, 2, p(idx), p(dist))
    refused("mgp_knn", "more than 2^24 features in one call", p(x), 5, (1 << 24) + 1, 2, p(idx), p(dist))
    # mgp_snn(device, idx, n, k, min_shared, capacity, n_edges, i, j, shared)
    cb = C.byref(count)
    for args in ((None, 5, 2, 1, 8, cb, *map(p, tri)), (p(idx), -5, 2, 1, 8, cb, *map(p, tri)),
                 (p(idx), 5, 2, 1, -1, cb, *map(p, tri)), (p(idx), 5, 2, 1, 8, None, *map(p, tri)),
                 (p(idx), 5, 2, 1, 8, cb, None, p(tri[1]), p(tri[2])), (p(idx), 5, 2, 1, 8, cb, p(tri[0]), None, p(tri[2])),
                 (p(idx), 5, 2, 1, 8, cb, p(tri[0]), p(tri[1]), None)):
        count.value = 99
        refused("mgp_snn", "bad arguments", *args)
        assert count.value == (99 if args[5] is None else 0)  # (set even when refused)
    for k in (0, 65):
        refused("mgp_snn", "k must be in 1..64", p(idx), 5, k, 1, 8, cb, *map(p, tri))
    refused("mgp_snn", "k must be at most n_items - 1", p(idx), 2, 2, 1, 8, cb, *map(p, tri))
    refused("mgp_snn", "more than 2^20 items in one call", p(idx), (1 << 20) + 1, 2, 1, 8, cb, *map(p, tri))
    for ms in (0, -3, 4):
        refused("mgp_snn", "min_shared must be in 1..k + 1", p(idx), 5, 2, ms, 8, cb, *map(p, tri))
    assert all(np.all(t == -7) for t in tri)
    # n_items = 0: nothing is launched (so this too runs without a device)
    assert lib.mgp_knn(0, None, 0, 2, 2, None, None) == engine.MGP_OK
    count.value = 99
    assert lib.mgp_snn(0, None, 0, 2, 1, 0, cb, None, None, None) == engine.MGP_OK and count.value == 0


# ---- the pipeline's plumbing, the oracle standing in for the device --------------------------
def test_pipeline_writes_the_graph_files(tmp_path, oracle_lib, monkeypatch):
    from test_cluster import CLUSTER_FILES
    from test_cluster import stand_in_device as cluster_stand_in

    from mgatk2_amd.analysis.neighbors import min_shared_for

    _patch_run(monkeypatch, oracle_lib)
    calls = stand_in_device(monkeypatch)
    cluster_calls = cluster_stand_in(monkeypatch)
    g, plain = _pipeline(tmp_path, "plain", **LOW)
    assert calls == [] and not any("knn" in f or "snn" in f for f in _files(plain))
    # 12 cells: K = 20 is clipped to 12, the device's k to 11
    _, out = _pipeline(tmp_path, "graph", neighbors=20, **LOW)
    assert calls == [("knn", 11, 0), ("snn", min_shared_for(12, 1 / 15), 0)] and cluster_calls == []
    assert [f for f in _files(out) if f not in _files(plain)] == GRAPH_FILES
    for rel in _files(plain):
        if not rel.endswith(("summary.txt", "output.log")):
            assert (out / rel).read_bytes() == (plain / rel).read_bytes(), rel
    # the files are the oracle's graphs of the matrix the same run wrote
    _, af = written_matrix(out, g.whitelist)
    assert af.shape[0] >= 2 and af.shape[1] == 12
    idx, dist = oracle_knn(oracle_dist(af), 11)
    check_graph_files(out / "variants", g.whitelist, idx, dist, oracle_snn(idx, min_shared_for(12, 1 / 15)), 12)
    # a smaller K and another prune; the matrix merged from two parts gives the same files
    del calls[:]
    _, small = _pipeline(tmp_path, "small", neighbors=4, snn_prune=0.5, **LOW)
    assert calls == [("knn", 3, 0), ("snn", min_shared_for(4, 0.5), 0)]
    idx, dist = oracle_knn(oracle_dist(af), 3)
    check_graph_files(small / "variants", g.whitelist, idx, dist, oracle_snn(idx, min_shared_for(4, 0.5)), 4)
    _, two = _pipeline(tmp_path, "two", neighbors=4, snn_prune=0.5, devices=[0, 0], **LOW)
    for rel in GRAPH_FILES:
        assert (two / rel).read_bytes() == (small / rel).read_bytes(), rel
    # with the clustering: both sets, the graphs after the trees
    del calls[:]
    _, both = _pipeline(tmp_path, "both", neighbors=4, cluster=True, clones=3, **LOW)
    assert len(cluster_calls) == 2 and [c[0] for c in calls] == ["knn", "snn"]
    new = sorted(CLUSTER_FILES + ["variants/cell_clones.tsv"] + GRAPH_FILES)
    assert [f for f in _files(both) if f not in _files(plain)] == new


def test_pipeline_without_variants_writes_no_graph_files(tmp_path, oracle_lib, monkeypatch, caplog):
    _patch_run(monkeypatch, oracle_lib, variants=False)
    calls = stand_in_device(monkeypatch)
    with caplog.at_level(logging.INFO, logger="mgatk2_amd"):
        _, out = _pipeline(tmp_path, "empty", neighbors=20, **LOW)
    assert calls == [] and "Neighbour graph skipped: 0 variants x 12 cells" in caplog.text
    assert [f for f in _files(out) if f.startswith("variants")] == ["variants/variant_stats.tsv"]
