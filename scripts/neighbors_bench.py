#!/usr/bin/env python
"""The cells' kNN and SNN graphs at the bench population: the synthetic
heteroplasmy-like matrix of scripts/cluster_bench.py, the kNN kernels' device time (HIP events,
MGP_VAR_PROF=1, printed by the library to stderr and collected here) with the automatic splits,
with one split and with k = 1 (the distances with next to no selection), beside the pair-distance
kernel's on the same matrix; the SNN passes' device times and the edge count; the wall time of
neighbor_graph; and scipy's cdist + argpartition on one core of the host as the reference point.
The device's indices of a subset are compared with the numpy oracle of tests/test_neighbors.py.

    python scripts/neighbors_bench.py [--cells 10000] [--variants 200] [--neighbors 20] [--reps 3]
                                      [--subset 1500] [--no-pair-dist] [--no-host] [--sweep 1,2,4,8,16,32,64]
"""

from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "scripts")]

from cluster_bench import FP64_VECTOR_PEAK, Stderr, synth_matrix  # noqa: E402


def knn_ms(err: Stderr) -> tuple[list[int], list[float]]:
    got = re.findall(r"kNN, splits (\d+): kernels ([0-9.]+) ms", err.text)
    return [int(s) for s, _ in got], [float(m) for _, m in got]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--variants", type=int, default=200)
    ap.add_argument("--neighbors", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--subset", type=int, default=1500)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-pair-dist", action="store_true", help="skip mgp_pair_dist (8 n^2 bytes) as the yardstick")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--sweep", type=str, default="", help="also time these MGP_KNN_SPLITS values (comma-separated)")
    args = ap.parse_args()
    os.environ["MGP_VAR_PROF"] = "1"
    os.environ.pop("MGP_KNN_SPLITS", None)

    from mgatk2_amd.analysis.clustering import pair_dist
    from mgatk2_amd.analysis.neighbors import knn, min_shared_for, neighbor_graph, snn

    af = synth_matrix(args.variants, args.cells, args.seed)
    n, f, k = args.cells, args.variants, args.neighbors - 1
    res = {"cells": n, "variants": f, "k_param": args.neighbors,
           "nonzero_fraction": round(float((af != 0).mean()), 4)}
    knn(af[:, :256], 5)  # (the first call loads the code objects)
    pairs2 = n * (n - 1)  # both triangles: what k_knn computes

    def timed(label, kk, splits=None):
        if splits is None:
            os.environ.pop("MGP_KNN_SPLITS", None)
        else:
            os.environ["MGP_KNN_SPLITS"] = str(splits)
        with Stderr() as err:
            for _ in range(args.reps):
                out = knn(af, kk)
        os.environ.pop("MGP_KNN_SPLITS", None)
        s, ms = knn_ms(err)
        res[f"knn_{label}_splits"], res[f"knn_{label}_kernels_ms"] = sorted(set(s)), ms
        res[f"knn_{label}_pair_features_per_s"] = round(pairs2 * f / (min(ms) * 1e-3), 0)
        return out

    idx, dist = timed("auto", k)
    one = timed("one_split", k, 1)
    assert one[0].tobytes() == idx.tobytes() and one[1].tobytes() == dist.tobytes()
    first = timed("k1", 1)
    np.testing.assert_array_equal(first[0][:, 0], idx[:, 0])
    sweep = {}
    for s in [int(v) for v in args.sweep.split(",") if v]:
        got = timed(f"sweep{s}", k, s)
        assert got[0].tobytes() == idx.tobytes() and got[1].tobytes() == dist.tobytes()
        sweep[s] = min(res.pop(f"knn_sweep{s}_kernels_ms"))
        del res[f"knn_sweep{s}_splits"], res[f"knn_sweep{s}_pair_features_per_s"]
    if sweep:
        res["knn_splits_sweep_best_ms"] = sweep
    best = min(res["knn_auto_kernels_ms"])
    res["knn_selection_share"] = round(1.0 - min(res["knn_k1_kernels_ms"]) / best, 4)
    # a pair and feature is one fp64 subtract and one fma: 3 FLOP of the peak's count
    res["knn_fraction_of_fp64_vector_peak"] = round(3 * pairs2 * f / (best * 1e-3) / FP64_VECTOR_PEAK, 4)
    if not args.no_pair_dist:
        pair_dist(af[:, :256])
        with Stderr() as err:
            for _ in range(args.reps):
                d = pair_dist(af)
        res["pair_dist_kernel_ms"] = err.kernel_ms("pair distances")
        res["pair_dist_pair_features_per_s"] = round(pairs2 / 2 * f / (min(res["pair_dist_kernel_ms"]) * 1e-3), 0)
        res["knn_over_pair_dist"] = round(best / min(res["pair_dist_kernel_ms"]), 3)
        rows = np.arange(n)[:, None]
        assert dist.tobytes() == d[rows, idx].tobytes()  # the matrix's own entries, bit for bit
        del d

    with Stderr() as err:
        for _ in range(args.reps):
            i, j, shared, weight = snn(idx)
    for key, what in (("check", "table check"), ("csr", "sorted sets and reverse lists"), ("count", "count pass"),
                      ("fill", "fill pass")):
        res[f"snn_{key}_kernels_ms"] = err.kernel_ms(what)  # (count and CSR run twice a call: capacity 0, then the size)
    res["snn_min_shared"], res["snn_edges"] = min_shared_for(k + 1, 1 / 15), int(i.size)
    res["snn_mean_degree"] = round(2.0 * i.size / n, 2)
    walls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        g = neighbor_graph(af, neighbors=args.neighbors)
        walls.append(round((time.perf_counter() - t0) * 1e3, 2))
    res["neighbor_graph_wall_ms"] = walls
    res["neighbor_graph_parts_s"] = {key: round(v, 4) for key, v in g.seconds.items()}
    assert g.idx.tobytes() == idx.tobytes() and np.array_equal(g.i, i) and np.array_equal(g.shared, shared)

    from test_neighbors import oracle_knn, oracle_snn

    m = min(args.subset, n)
    sub = knn(af[:, :m], min(k, m - 1))
    want = oracle_knn(pair_dist(af[:, :m]), min(k, m - 1))  # (on the device's own matrix: its fma chain)
    np.testing.assert_array_equal(sub[0], want[0])
    assert sub[1].tobytes() == want[1].tobytes()
    ms = min_shared_for(sub[0].shape[1] + 1, 1 / 15)
    for a, b in zip(snn(sub[0])[:3], oracle_snn(sub[0], ms)):
        np.testing.assert_array_equal(a, b)
    res["oracle_subset_cells"], res["subset_equals_oracle"] = m, True

    if not args.no_host:
        from scipy.spatial.distance import cdist

        pts = np.ascontiguousarray(af.T)
        t0 = time.perf_counter()
        full = cdist(pts, pts)  # (scipy's C loop: one core)
        t1 = time.perf_counter()
        np.fill_diagonal(full, np.inf)
        part = np.argpartition(full, k, axis=1)[:, :k]
        t2 = time.perf_counter()
        res["host_cdist_s"], res["host_argpartition_s"] = round(t1 - t0, 3), round(t2 - t1, 3)
        # the k-th distance agrees (the sets can differ among tied candidates)
        kth = np.take_along_axis(full, part, axis=1).max(axis=1)
        np.testing.assert_allclose(kth, dist[:, -1], rtol=1e-9, atol=1e-12)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
