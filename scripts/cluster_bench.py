#!/usr/bin/env python
"""Clustering by heteroplasmy at the bench population: a synthetic
heteroplasmy-like matrix (mostly zeros, a few clonal blocks, sparse noise), the pair-distance
kernel's and the linkage's device times (HIP events, MGP_VAR_PROF=1, printed by the library to
stderr and collected here), the wall time of cluster_heteroplasmy, and scipy's pdist + linkage on
the same matrix on one core of the host as the reference point. The device's trees of a subset
are compared with the numpy oracle of tests/test_cluster.py.

    python scripts/cluster_bench.py [--cells 10000] [--variants 200] [--reps 3] [--subset 1500] [--no-scipy]
"""

from __future__ import annotations

import argparse
import json
import os
import re
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

FP64_VECTOR_PEAK = 78.6e12  # MI355X, FLOP/s with an fma as two (half the 157.3 TFLOPS fp32 vector rate)


def synth_matrix(n_var: int, n_cells: int, seed: int, clones: int = 8) -> np.ndarray:
    """[n_var, n_cells]: each clone has its own few marker variants at a clone-wide level with
    per-cell spread; elsewhere zeros but for sparse low-level noise."""
    rng = np.random.default_rng(seed)
    af = np.zeros((n_var, n_cells))
    clone_of = rng.integers(0, clones, n_cells)
    markers = rng.permutation(n_var)[:clones * max(2, n_var // (4 * clones))].reshape(clones, -1)
    for c in range(clones):
        cells = np.flatnonzero(clone_of == c)
        for v in markers[c]:
            level = rng.uniform(0.1, 0.9)
            af[v, cells] = np.clip(rng.normal(level, 0.08, cells.size), 0.0, 1.0)
    noise = rng.random((n_var, n_cells)) < 0.01
    af[noise] = np.round(rng.uniform(0.0, 0.05, int(noise.sum())), 3)
    return af


class Stderr:
    """fd 2 into a file for the duration (the library's MGP_VAR_PROF lines), echoed afterwards."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        sys.stderr.write(self.text)

    def kernel_ms(self, what: str) -> list[float]:
        return [float(m) for m in re.findall(rf"{what}: kernels ([0-9.]+) ms", self.text)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--variants", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--subset", type=int, default=1500)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    os.environ["MGP_VAR_PROF"] = "1"

    from mgatk2_amd.analysis.clustering import cluster_heteroplasmy, hclust

    af = synth_matrix(args.variants, args.cells, args.seed)
    n, f = args.cells, args.variants
    res = {"cells": n, "variants": f, "nonzero_fraction": round(float((af != 0).mean()), 4)}
    hclust(x=af[:, :64])  # (the first call loads the code objects)
    with Stderr() as err:
        walls = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            tree = hclust(x=af)
            walls.append(round((time.perf_counter() - t0) * 1e3, 2))
    res["pair_dist_kernel_ms"] = err.kernel_ms("pair distances")
    res["linkage_kernels_ms"] = err.kernel_ms("linkage steps")
    res["hclust_cells_wall_ms"] = walls
    best = min(res["pair_dist_kernel_ms"]) * 1e-3
    pairs = n * (n - 1) // 2
    res["pair_features_per_s"] = round(pairs * f / best, 0)
    # a pair and feature is one fp64 subtract and one fma: 3 FLOP of the peak's count
    res["fraction_of_fp64_vector_peak"] = round(3 * pairs * f / best / FP64_VECTOR_PEAK, 4)
    with Stderr() as err:
        walls = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            both = cluster_heteroplasmy(af, clones=8)
            walls.append(round((time.perf_counter() - t0) * 1e3, 2))
    res["cluster_heteroplasmy_wall_ms"] = walls
    res["cluster_heteroplasmy_parts_s"] = {k: round(v, 4) for k, v in both.seconds.items()}
    res["clone_sizes"] = np.bincount(both.clones)[1:].tolist()
    np.testing.assert_array_equal(both.cells.merge, tree.merge)

    from test_cluster import oracle_dist, oracle_hclust

    m = min(args.subset, n)
    sub = hclust(x=af[:, :m])
    t0 = time.perf_counter()
    want = oracle_hclust(oracle_dist(af[:, :m]))
    res["oracle_subset_cells"], res["oracle_subset_s"] = m, round(time.perf_counter() - t0, 3)
    # (the oracle's distances have no fma: where they differ from the device's in the last place a
    # tie can fall the other way, so the subset is compared on the device's own matrix)
    from mgatk2_amd.analysis.clustering import pair_dist

    want = oracle_hclust(pair_dist(af[:, :m]))
    for a, b in zip((sub.merge, sub.height, sub.order), want):
        np.testing.assert_array_equal(a, b)
    res["subset_equals_oracle"] = True

    if not args.no_scipy:
        os.environ.setdefault("OMP_NUM_THREADS", "1")
        from scipy.cluster.hierarchy import linkage
        from scipy.spatial.distance import pdist

        t0 = time.perf_counter()
        cond = pdist(np.ascontiguousarray(af.T))
        t1 = time.perf_counter()
        z = linkage(cond, "complete")
        t2 = time.perf_counter()
        res["scipy_pdist_s"], res["scipy_linkage_s"] = round(t1 - t0, 3), round(t2 - t1, 3)
        res["scipy_top_height"], res["device_top_height"] = float(z[-1, 2]), float(tree.height[-1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
