#!/usr/bin/env python
"""The cells' clonotypes at the bench population: the synthetic heteroplasmy-like
matrix of scripts/cluster_bench.py with K planted clones, its SNN graph from neighbor_graph on the
device, then mgp_louvain on it: the device time of the build and of the loop of levels and passes
(HIP events, MGP_VAR_PROF=1, printed by the library to stderr and collected here; the loop's time
includes the waits for the host between passes), the wall time of the call, the levels and passes,
Q and the agreement with the planted clones; and networkx's louvain_communities on the same graph
on one core of the host as the reference point, its Q beside ours. The device's result of a subset
is compared with the plain-Python model of tests/louvain_model.py.

    python scripts/clonotypes_bench.py [--cells 10000] [--variants 200] [--clones 20] [--neighbors 20]
                                       [--reps 3] [--subset 1500] [--no-host] [--seeds 3]
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

from cluster_bench import Stderr, synth_matrix  # noqa: E402


def adjusted_rand(a, b) -> float:
    """The adjusted Rand index of two labellings (the contingency table's pair counts)."""
    a, b = np.unique(a, return_inverse=True)[1], np.unique(b, return_inverse=True)[1]
    table = np.zeros((a.max() + 1, b.max() + 1), np.int64)
    np.add.at(table, (a, b), 1)
    pairs = lambda x: float((x * (x - 1) // 2).sum())  # noqa: E731
    both, rows, cols, total = pairs(table), pairs(table.sum(1)), pairs(table.sum(0)), pairs(np.array([a.size]))
    expected = rows * cols / total
    return (both - expected) / ((rows + cols) / 2 - expected)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--variants", type=int, default=200)
    ap.add_argument("--clones", type=int, default=20)
    ap.add_argument("--neighbors", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--subset", type=int, default=1500)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--seeds", type=int, default=3, help="networkx seeds 0..seeds-1")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    os.environ["MGP_VAR_PROF"] = "1"
    for name in ("MGP_LOUVAIN_WAVE_ROW", "MGP_LOUVAIN_LDS_ROW"):
        os.environ.pop(name, None)

    from mgatk2_amd.analysis.clonotypes import communities, modularity, quantise
    from mgatk2_amd.analysis.neighbors import neighbor_graph

    n = args.cells
    af = synth_matrix(args.variants, n, args.seed, clones=args.clones)
    planted = np.random.default_rng(args.seed).integers(0, args.clones, n)  # synth_matrix's first draw
    g = neighbor_graph(af, neighbors=args.neighbors)
    wq = quantise(g.weight)
    deg = np.bincount(np.concatenate([g.i, g.j]), minlength=n)
    res = {"cells": n, "variants": args.variants, "planted_clones": args.clones, "k_param": args.neighbors,
           "snn_edges": int(g.i.size), "max_degree": int(deg.max()), "rows_over_64": int((deg > 64).sum()),
           "rows_over_2048": int((deg > 2048).sum())}
    communities(n, g.i, g.j, wq)  # (the first call loads the code objects)
    walls = []
    with Stderr() as err:
        for _ in range(args.reps):
            t0 = time.perf_counter()
            c = communities(n, g.i, g.j, wq)
            walls.append(round((time.perf_counter() - t0) * 1e3, 2))
    res["louvain_wall_ms"] = walls
    res["louvain_build_kernels_ms"] = err.kernel_ms("vertices, edges, build")
    res["louvain_loop_device_ms"] = [float(m) for m in re.findall(r"levels, passes: kernels ([0-9.]+) ms", err.text)]
    res["levels"] = c.levels
    res["passes"] = int(sum(lv[2] for lv in c.levels))
    res["clonotypes"], res["modularity"] = c.n_communities, c.modularity
    res["adjusted_rand_with_planted"] = round(adjusted_rand(c.labels, planted), 4)
    assert modularity(n, g.i, g.j, wq, c.labels) == c.modularity

    from louvain_model import louvain

    m = min(args.subset, n)
    keep = g.j < m
    sub = communities(m, g.i[keep], g.j[keep], wq[keep])
    want = louvain(m, g.i[keep], g.j[keep], wq[keep])
    assert sub.labels.tolist() == want.labels and sub.modularity == want.modularity and sub.levels == want.levels
    assert (sub.m2, sub.internal, sub.b) == (want.m2, want.internal, want.b)
    res["model_subset_cells"], res["subset_equals_model"] = m, True

    if not args.no_host:
        import networkx as nx

        t0 = time.perf_counter()
        graph = nx.Graph()
        graph.add_nodes_from(range(n))
        graph.add_weighted_edges_from(zip(g.i.tolist(), g.j.tolist(), (wq / float(1 << 20)).tolist()))
        res["networkx_graph_s"] = round(time.perf_counter() - t0, 3)
        secs, qs, counts, aris = [], [], [], []
        for seed in range(args.seeds):
            t0 = time.perf_counter()
            comms = nx.community.louvain_communities(graph, weight="weight", resolution=1.0, seed=seed)
            secs.append(round(time.perf_counter() - t0, 3))
            labels = np.zeros(n, np.int64)
            for k, members in enumerate(comms):
                labels[list(members)] = k
            qs.append(modularity(n, g.i, g.j, wq, labels))  # (the same expression as ours)
            counts.append(len(comms))
            aris.append(round(adjusted_rand(labels, planted), 4))
        res.update(networkx_louvain_s=secs, networkx_modularity=qs, networkx_communities=counts,
                   networkx_adjusted_rand_with_planted=aris)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
