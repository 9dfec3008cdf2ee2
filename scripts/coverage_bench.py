#!/usr/bin/env python
"""Coverage QC at bench density: the four device passes' kernel times (HIP events,
MGP_VAR_PROF=1, printed by the library to stderr) and their wall times over a resident synthetic
run, run_coverage's wall time (what CellProcessor reports as last_timing["coverage"]), and the
numpy oracle of tests/test_coverage.py on a subset of the cells as the host reference point
(its tables are compared with the device's on that subset).

    python scripts/coverage_bench.py [--reads 200000000] [--cells 10000] [--subset 1000] [--reps 3]
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
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def timed(fn, reps):
    out, secs = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        secs.append(round((time.perf_counter() - t0) * 1e3, 3))
    return out, secs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200_000_000)
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--subset", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    os.environ["MGP_VAR_PROF"] = "1"

    from mgatk2_amd.analysis import coverage as cov
    from mgatk2_amd.engine import Engine, EngineConfig
    from mgatk2_amd.synth import cell_cdf, ref_codes

    cfg = EngineConfig(n_cells=args.cells, min_baseq=20, min_mapq=30, min_distance_from_end=5,
                       dedup_mode="alignment_and_fragment_length", max_strand_bias=1.0, min_reads=1)
    res = {"reads": args.reads, "cells": args.cells}
    with Engine(cfg) as eng:
        eng.synth(args.seed, args.reads, cell_cdf(args.seed, args.cells), ref_codes(args.seed), rec_align=64, pack=True)
        eng.run()
        eng.sync()
        L = cfg.mito_len
        cell, res["cell_coverage_ms"] = timed(lambda: eng.cell_coverage(), args.reps)
        pos, res["position_coverage_ms"] = timed(lambda: eng.position_coverage(), args.reps)
        res["max_depth"] = int(pos["max_depth"].max())
        res["mean_depth"] = float(pos["s_depth"].sum() / (args.cells * L))
        zero = np.zeros(L, np.uint32)
        for shift in (8, 0):
            _, res[f"depth_hist_shift{shift}_ms"] = timed(lambda: eng.position_depth_hist(shift, zero), args.reps)
        _, res["depth_next_ms"] = timed(lambda: eng.position_depth_next(zero), args.reps)
        full, res["run_coverage_ms"] = timed(lambda: cov.run_coverage(eng), args.reps)
        res["run_coverage_parts_s"] = {k: round(v, 4) for k, v in full.seconds.items()}
        _, res["run_coverage_filtered_ms"] = timed(
            lambda: cov.run_coverage(eng, min_mean_coverage=10, min_coverage_breadth=0.5, recompute_reference=True),
            args.reps)
        m = min(args.subset, args.cells)
        sub = cov.run_coverage(eng, cells=np.arange(m))
        rows = eng.fetch_cells(0, m)
    from test_coverage import check_table, oracle_cell_table, oracle_position_tables

    t0 = time.perf_counter()
    want_cell = oracle_cell_table(rows.depth)
    want = oracle_position_tables(rows.counts, rows.tn5, rows.depth)
    res["oracle_subset_cells"] = m
    res["oracle_subset_s"] = round(time.perf_counter() - t0, 3)
    top = int(rows.depth.max())
    check_table(sub.cell, want_cell, L, top, "subset cell")
    check_table(sub.position, want[0], m, top, "subset position")
    check_table(sub.strand, want[1], 4 * m, top, "subset strand")
    check_table(sub.transposition, want[2], m, top, "subset tn5")
    res["subset_equals_oracle"] = True
    print(json.dumps(res))


if __name__ == "__main__":
    main()
