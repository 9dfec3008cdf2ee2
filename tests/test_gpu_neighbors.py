"""The cells' kNN and SNN graphs on the device (mgp_knn / mgp_snn, mgp_graph.hip) against the
numpy oracle of tests/test_neighbors.py.

The sizes follow the kernels' shapes: the query and candidate tile edge T = 64 (n = T + 1 and
2T + 2: one and two tiles plus a remainder; n = 1,100: 18 tiles, several workgroups and, with
splits, several partial lists), the feature chunk of 32 (n_feat = 33 and 65), the list width of
64 lanes (k = 64 fills it, k = 1 is its other end) and the splits of the candidate range.

The kNN only selects among distances that are mgp_pair_dist's by definition, so its indices are
compared exactly with the oracle on the device's own matrix and its distances bit for bit with
that matrix's entries; against numpy's own sums the distances are within test_variants.tol(n_feat)
(16 m 2^-53 for an m-term fp64 sum), relative. The SNN counts in integers: everything is exact.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from test_cluster import written_matrix
from test_gpu_variants import _files, _pipeline, _same_file
from test_neighbors import GRAPH_FILES, check_graph_files, oracle_knn, oracle_snn
from test_variants import tol

pytestmark = pytest.mark.gpu

T, CHUNK = 64, 32
KS = (1, 5, 20, 64)


def planted(n, nf, seed):
    """[nf, n] random values with duplicate columns and all-zero columns planted across tiles."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nf, n)) * rng.choice([1e-3, 1.0, 50.0], (nf, 1))
    if n >= 3:
        x[:, n - 1] = x[:, 0]  # a duplicate across the first and the last tile
        x[:, n // 2] = 0.0
    if n >= 65:
        x[:, 7] = x[:, 3]
        x[:, 64] = x[:, 3]  # the same column in two tiles
        x[:, [11, 40, n - 2]] = 0.0
    return x


_matrix = {}


def device_matrix(engine, n, nf):
    """(x, mgp_pair_dist's matrix of it), made once per shape and left unchanged."""
    if (n, nf) not in _matrix:
        x = planted(n, nf, 100 * n + nf)
        _matrix[n, nf] = (x, engine.cluster_pair_dist(x))
    return _matrix[n, nf]


@pytest.mark.parametrize("n_feat", [1, CHUNK + 1, 2 * CHUNK + 1])
@pytest.mark.parametrize("n", [2, 3, T + 1, 2 * T + 2, 1100])
def test_knn_against_the_devices_own_matrix(engine_lib, n, n_feat):
    x, d = device_matrix(engine_lib, n, n_feat)
    ks = sorted({k for k in KS if k <= n - 1} | ({n - 1} if n in (3, T + 1) else set()))
    assert ks
    for k in ks:
        idx, dist = engine_lib.graph_knn(x, k)
        assert idx.shape == (n, k) and idx.dtype == np.int32 and dist.shape == (n, k) and dist.dtype == np.float64
        want_idx, want_dist = oracle_knn(d, k)
        np.testing.assert_array_equal(idx, want_idx, err_msg=f"k={k}")
        assert dist.tobytes() == want_dist.tobytes(), k  # the matrix's own entries, bit for bit
        again = engine_lib.graph_knn(x, k)
        assert again[0].tobytes() == idx.tobytes() and again[1].tobytes() == dist.tobytes()
        own = np.sqrt(((x[:, :, None] - x[:, idx]) ** 2).sum(axis=0))  # numpy's own sums
        err = np.abs(dist - own)
        print(f"n={n} n_feat={n_feat} k={k}: max relative error "
              f"{np.max(err / np.where(own > 0, own, 1.0)):.3g} (bound {tol(n_feat):.3g})")
        assert np.all(err <= tol(n_feat) * own)
    if n >= 3:  # the planted duplicates find each other first, at exactly 0 (ties to the lower index)
        idx, dist = engine_lib.graph_knn(x, 1)
        if n != T + 1:  # (there column n - 1 is column 64, planted again below)
            assert idx[n - 1, 0] == 0 and dist[n - 1, 0] == 0.0 and dist[0, 0] == 0.0
        if n >= T + 1:
            assert idx[[3, 7, 64], 0].tolist() == [7, 3, 3] and not dist[[3, 7, 64], 0].any()


def line_row(i, n, k):
    """Items at x = 0..n-1: row i alternates i - d and i + d, ties to the lower index, clipped."""
    out = []
    for d in range(1, n):
        out += [j for j in (i - d, i + d) if 0 <= j < n]
        if len(out) >= k:
            break
    return out[:k]


@pytest.mark.parametrize("k", [20, 64])
def test_order_of_arrival_on_a_line(engine_lib, k):
    """n_feat = 1, x[0, j] = j: for high rows the nearer candidates arrive in late tiles (every
    tile inserts), for low rows in the first tile (no later tile inserts)."""
    n = 5000
    x = np.arange(n, dtype=np.float64)[None, :]
    idx, dist = engine_lib.graph_knn(x, k)
    want = np.array([line_row(i, n, k) for i in range(n)], np.int32)
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_array_equal(dist, np.abs(want - np.arange(n)[:, None]).astype(np.float64))


def test_all_columns_equal(engine_lib):
    n, k = 300, 20
    idx, dist = engine_lib.graph_knn(np.full((7, n), 0.375), k)
    assert not dist.any()
    want = np.array([[j for j in range(k + 1) if j != i][:k] for i in range(n)], np.int32)
    np.testing.assert_array_equal(idx, want)  # the 20 lowest indices other than its own


@pytest.mark.parametrize("n", [2 * T + 2, 1100])
def test_splits_do_not_change_a_byte(engine_lib, n, monkeypatch):
    x = planted(n, 9, n)
    monkeypatch.delenv("MGP_KNN_SPLITS", raising=False)
    base = engine_lib.graph_knn(x, 20)
    np.testing.assert_array_equal(base[0], oracle_knn(engine_lib.cluster_pair_dist(x), 20)[0])
    for splits in ("1", "2", "7", "0", "1000"):  # (the driver reads the knob on every call)
        monkeypatch.setenv("MGP_KNN_SPLITS", splits)
        got = engine_lib.graph_knn(x, 20)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes(), splits


def test_knn_against_a_kd_tree(engine_lib):
    """A cross-check that uses no project code: tie-free random data, scipy's cKDTree."""
    from scipy.spatial import cKDTree

    n, k = 2050, 20
    x = np.random.default_rng(2050).random((9, n))
    idx, dist = engine_lib.graph_knn(x, k)
    kd_dist, kd_idx = cKDTree(x.T).query(x.T, k + 1)
    assert np.array_equal(kd_idx[:, 0], np.arange(n)) and np.all(np.diff(kd_dist, axis=1) > 0)  # tie-free
    np.testing.assert_array_equal(idx, kd_idx[:, 1:])
    np.testing.assert_allclose(dist, kd_dist[:, 1:], rtol=tol(9), atol=0)


def test_refusals_on_the_device(engine_lib):
    from mgatk2_amd.exceptions import InvalidInputError

    x = planted(T + 1, 7, 5)
    for v, at in ((np.nan, (6, 64)), (np.inf, (0, 0)), (-np.inf, (3, 30))):
        bad = x.copy()
        bad[at] = v
        with pytest.raises(InvalidInputError, match="not finite"):
            engine_lib.graph_knn(bad, 5)
    idx, _ = engine_lib.graph_knn(x, 5)
    for (row, col), v in (((64, 4), T + 1), ((0, 0), -1), ((9, 2), 9), ((30, 1), None)):
        bad = idx.copy()
        bad[row, col] = bad[row, 0] if v is None else v  # out of range, its own row, a repeated entry
        with pytest.raises(InvalidInputError, match="kNN table"):
            engine_lib.graph_snn(bad, 1)
    assert len(engine_lib.graph_snn(idx, 1)[0]) > 0


@pytest.mark.parametrize("k", [5, 20])
@pytest.mark.parametrize("n", [2 * T + 2, 1100])
def test_snn_against_the_oracle(engine_lib, n, k):
    from mgatk2_amd.analysis.neighbors import min_shared_for, snn

    x, _ = device_matrix(engine_lib, n, 9)
    idx, _ = engine_lib.graph_knn(x, k)
    for ms in sorted({1, min_shared_for(k + 1, 1 / 15)}):
        got = engine_lib.graph_snn(idx, ms)
        want = oracle_snn(idx, ms)
        assert len(want[0]) > n
        for a, b, what in zip(got, want, ("i", "j", "shared")):
            assert a.dtype == np.int32
            np.testing.assert_array_equal(a, b, err_msg=f"{what}, min_shared {ms}")
    i, j, shared, weight = snn(idx)  # Seurat's default prune
    want = oracle_snn(idx, min_shared_for(k + 1, 1 / 15))
    np.testing.assert_array_equal(shared, want[2])
    np.testing.assert_array_equal(weight, want[2] / (2.0 * (k + 1) - want[2]))
    assert np.all(weight >= 1 / 15) and np.all(i < j)


def test_snn_of_a_hub(engine_lib):
    """300 identical columns among 600, k = 20: every identical cell lists the 20 lowest of
    them, so all their pairs are edges, and the 21 lowest have the same set: weight 1."""
    n, k = 600, 20
    x = np.random.default_rng(6).random((5, n))
    x[:, ::2] = x[:, :1]
    idx, dist = engine_lib.graph_knn(x, k)
    assert not dist[::2].any() and np.all(idx[::2] % 2 == 0)
    got = engine_lib.graph_snn(idx, 1)
    want = oracle_snn(idx, 1)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    i, j, shared = got
    hub = (i % 2 == 0) & (j % 2 == 0)
    assert hub.sum() == 300 * 299 // 2 and np.all(shared[hub] >= k)  # the dense block, complete
    top = hub & (i <= 2 * k) & (j <= 2 * k)
    assert top.sum() == (k + 1) * k // 2 and np.all(shared[top] == k + 1)  # weight 1
    assert engine_lib.graph_snn(idx, k + 1)[2].tolist() == [k + 1] * int((shared == k + 1).sum())


def test_snn_capacity(engine_lib):
    x, _ = device_matrix(engine_lib, 2 * T + 2, 9)
    idx, _ = engine_lib.graph_knn(x, 5)
    want = oracle_snn(idx, 2)
    ne = len(want[0])
    lib = engine_lib.load_library()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for cap in (0, 1, ne - 1):
        out = [np.full(ne, -7, np.int32) for _ in range(3)]
        count = C.c_int64(-1)
        rc = lib.mgp_snn(0, p(idx), idx.shape[0], 5, 2, cap, C.byref(count), *map(p, out))
        assert rc == engine_lib.MGP_E_INVALID and count.value == ne
        assert f"{ne} edges, capacity {cap}" in lib.mgp_last_error().decode()
        assert all(np.all(a == -7) for a in out)  # nothing written
    out = [np.full(ne + 3, -7, np.int32) for _ in range(3)]
    count = C.c_int64(-1)
    assert lib.mgp_snn(0, p(idx), idx.shape[0], 5, 2, ne + 3, C.byref(count), *map(p, out)) == engine_lib.MGP_OK
    assert count.value == ne and all(np.all(a[ne:] == -7) for a in out)
    order = np.lexsort((out[1][:ne], out[0][:ne]))
    for a, b in zip(out, want):
        np.testing.assert_array_equal(a[:ne][order], b)


LOW = dict(call_variants=True, variant_min_cells=0, variant_min_strand_cor=-1.0, variant_min_vmr=0.0)


def test_pipeline_neighbors(tmp_path, engine_lib, monkeypatch):
    """run_pipeline(call_variants, neighbors=20) on the synth_run_h5 golden reads, the thresholds
    lowered as in test_gpu_variants so that variants pass: the three files equal the oracle on the
    heteroplasmy matrix the same run wrote (features in genomic order), a run sharded over two
    contexts writes the same bytes, every other file is what a run without the flag writes, and
    with the clustering both sets of files are written."""
    from test_cluster import CLUSTER_FILES

    from mgatk2_amd.analysis.neighbors import min_shared_for

    g, out = _pipeline(tmp_path, "graph", "txt", monkeypatch, neighbors=20, **LOW)
    _, plain = _pipeline(tmp_path, "plain", "txt", monkeypatch, **LOW)
    assert [f for f in _files(out) if f not in _files(plain)] == GRAPH_FILES
    assert [f for f in _files(out) if f not in GRAPH_FILES] == _files(plain)
    for rel in _files(plain):
        _same_file(out, plain, rel)
    _, af = written_matrix(out, g.whitelist)  # (the variants in genomic order: the graph's features)
    n = len(g.whitelist)
    assert af.shape[0] >= 2 and n >= 3
    k = min(19, n - 1)
    idx, dist = oracle_knn(engine_lib.cluster_pair_dist(af), k)
    check_graph_files(out / "variants", g.whitelist, idx, dist, oracle_snn(idx, min_shared_for(k + 1, 1 / 15)), k + 1)
    _, two = _pipeline(tmp_path, "two", "txt", monkeypatch, devices=[0, 0], neighbors=20, **LOW)
    for rel in GRAPH_FILES:
        assert (two / rel).read_bytes() == (out / rel).read_bytes(), rel
    _, both = _pipeline(tmp_path, "both", "txt", monkeypatch, neighbors=20, cluster=True, clones=3, **LOW)
    new = sorted(CLUSTER_FILES + ["variants/cell_clones.tsv"] + GRAPH_FILES)
    assert [f for f in _files(both) if f not in _files(plain)] == new
    for rel in GRAPH_FILES:
        assert (both / rel).read_bytes() == (out / rel).read_bytes(), rel
