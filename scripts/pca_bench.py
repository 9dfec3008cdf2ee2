#!/usr/bin/env python
"""The principal components of a heteroplasmy-shaped matrix: 90 % zeros, the rest uniform
noise, plus a planted low-rank part; the device time of each phase of mgp_pca (HIP events, MGP_VAR_PROF=1,
printed by the library to stderr and collected here: the means and the scaling, the covariance, the Jacobi
iteration with its sweeps, the scores), the wall time around the Python call, and, for the first case,
numpy.linalg.svd of the centred matrix on one core of the host as the reference point, with the two results
compared (eigenvalues, and the scores up to the vectors' signs).

    OMP_NUM_THREADS=1 python scripts/pca_bench.py [--cells 10000] [--variants 200] [--components 50] [--reps 3]
                                                  [--rank 8] [--scale] [--no-host] [--tiles 16,32,64]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "scripts")]

from cluster_bench import FP64_VECTOR_PEAK, Stderr  # noqa: E402

PHASES = (("means", "means and scaling"), ("covariance", r"covariance, tile \d+"), ("jacobi", "Jacobi"),
          ("scores", "scores"))


def planted_sparse(n_var: int, n_cells: int, rank: int, seed: int) -> np.ndarray:
    """[n_var, n_cells]: 90 % zeros and uniform (0, 0.05] elsewhere, plus a rank-`rank` part (a clone-like
    block structure: each factor lifts a tenth of the variants in a share of the cells)."""
    rng = np.random.default_rng(seed)
    x = np.where(rng.random((n_var, n_cells)) < 0.9, 0.0, 0.05 * (1.0 - rng.random((n_var, n_cells))))
    for r in range(rank):
        rows = rng.permutation(n_var)[:max(1, n_var // 10)]
        cells = rng.random(n_cells) < rng.uniform(0.05, 0.3)
        x[np.ix_(rows, np.flatnonzero(cells))] += rng.uniform(0.2, 0.8, (rows.size, 1)) * rng.uniform(
            0.5, 1.0, (1, int(cells.sum())))
    return np.clip(x, 0.0, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--variants", type=int, default=200)
    ap.add_argument("--components", type=int, default=50)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scale", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--tiles", type=str, default="", help="also time these MGP_PCA_TILE values (comma-separated)")
    args = ap.parse_args()
    os.environ["MGP_VAR_PROF"] = "1"
    os.environ.pop("MGP_PCA_TILE", None)

    from mgatk2_amd.analysis.pca import pca, variance_table

    n, m, k = args.cells, args.variants, args.components
    x = planted_sparse(m, n, args.rank, args.seed)
    res = {"cells": n, "variants": m, "components": k, "scale": bool(args.scale),
           "nonzero_fraction": round(float((x != 0).mean()), 4)}
    pca(x[:8, :256], 2)  # (the first call loads the code objects)
    walls = []
    with Stderr() as err:
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = pca(x, k, args.scale)
            walls.append(round((time.perf_counter() - t0) * 1e3, 2))
    for key, what in PHASES:
        res[f"{key}_kernels_ms"] = err.kernel_ms(what)
    res["sweeps"], res["pca_wall_ms"] = r.sweeps, walls
    res["jacobi_launches"] = (r.sweeps + 1) * (((m + 1) & ~1) - 1)  # (the last sweep rotates nothing)
    # a pair of variants and a cell is one fma: 2 FLOP of the peak's count, one triangle
    res["covariance_fraction_of_fp64_vector_peak"] = round(
        n * m * (m + 1) / (min(res["covariance_kernels_ms"]) * 1e-3) / FP64_VECTOR_PEAK, 4)
    _, frac, cum = variance_table(r.eigenvalues, r.n_comp)
    res["variance_first"], res["variance_cumulative_at_rank"] = round(frac[0], 4), round(cum[min(args.rank, k) - 1], 4)
    for tile in [int(v) for v in args.tiles.split(",") if v]:
        os.environ["MGP_PCA_TILE"] = str(tile)
        with Stderr() as err:
            for _ in range(args.reps):
                again = pca(x, k, args.scale)
        os.environ.pop("MGP_PCA_TILE", None)
        assert again.scores.tobytes() == r.scores.tobytes() and again.eigenvalues.tobytes() == r.eigenvalues.tobytes()
        res.setdefault("covariance_tile_best_ms", {})[tile] = min(err.kernel_ms(PHASES[1][1]))
    if not args.no_host:
        t0 = time.perf_counter()
        z = x - x.mean(axis=1, keepdims=True)
        if args.scale:
            sd = z.std(axis=1, ddof=1, keepdims=True)
            z = np.divide(z, sd, out=np.zeros_like(z), where=sd != 0)
        u, s, vt = np.linalg.svd(z.T, full_matrices=False)  # (cells x variants, as prcomp)
        host = time.perf_counter() - t0
        res["host_svd_s"] = round(host, 3)
        ev = s ** 2 / (n - 1)
        top = float(ev.max())
        res["eigenvalues_max_abs_diff_over_top"] = float(np.abs(ev - r.eigenvalues).max() / top)
        want = (u * s).T[:k]
        sign = np.sign(np.sum(want * r.scores, axis=1, keepdims=True))
        sep = np.flatnonzero(np.abs(np.diff(ev[:k + 1])) > 1e-6 * top)  # (a vector is defined where its value is apart)
        sep = sep[sep < k]
        res["scores_max_abs_diff_separated"] = float(np.abs(want * sign - r.scores)[sep].max()) if sep.size else None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
