"""engine.rank_sums (mgp_rank_sums) on heteroplasmy-shaped matrices, and the first case against the only route
there was before it, a loop of scipy.stats.mannwhitneyu over every (variant, group) pair on one core
(profiles/rank/).

Two cases: (a) 10,000 cells x 200 variants x 20 groups, (b) 65,536 cells x 1,000 variants x 1,000 groups; about
90 % of every variant's values are 0, the rest multiples of 1/64 (many ties, as a heteroplasmy matrix has).
Each is timed three times: wall time around the Python call (upload, kernels, download) and the kernels' device
time between two events of the call's stream (MGP_VAR_PROF, read back from the library's stderr line). For
(a) the whole test follows both ways: group_tests' table here, the scipy loop there (its time is for
--scipy-pairs pairs, scaled to all), and U and p are compared. One JSON file.

    python scripts/rank_bench.py [--out FILE] [--scipy-pairs N]
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from mgatk2_amd import engine  # noqa: E402
from mgatk2_amd.analysis.group_tests import group_tests  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="rank_bench.json")
ap.add_argument("--scipy-pairs", type=int, default=400)
args = ap.parse_args()
out = {}


def say(*a):
    print("[rank_bench]", *a, flush=True)


def timed(fn):
    """(result, wall seconds, device milliseconds) of fn(): the device time is the sum of the library's
    "kernels X ms" lines, which it writes to stderr under MGP_VAR_PROF."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            got = fn()
            wall = time.perf_counter() - t0
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        ms = sum(float(x) for x in re.findall(rb"kernels ([0-9.]+) ms", tmp.read()))
    return got, wall, ms


def matrix(rng, n_var, n_cells):
    x = rng.integers(1, 64, (n_var, n_cells)) / 64.0
    x[rng.random((n_var, n_cells)) < 0.9] = 0.0
    return x


os.environ["MGP_VAR_PROF"] = "1"
rng = np.random.default_rng(20251021)
engine.rank_sums(np.zeros((1, 64)), np.zeros(64, np.int32), 1)  # the device's first call is not timed
for name, n_cells, n_var, n_groups in (("a_10000x200x20", 10_000, 200, 20), ("b_65536x1000x1000", 65_536, 1_000, 1_000)):
    x = matrix(rng, n_var, n_cells)
    labels = rng.permutation(np.arange(n_cells) % n_groups).astype(np.int32)
    rec = {"cells": n_cells, "variants": n_var, "groups": n_groups, "rank_sums": []}
    for k in range(3):
        got, wall, ms = timed(lambda: engine.rank_sums(x, labels, n_groups))
        rec["rank_sums"].append({"wall_s": wall, "device_ms": ms})
        say(name, "rank_sums", json.dumps(rec["rank_sums"][-1]))
    n = n_cells
    rec["sums_hold"] = bool((got["r2"].sum(axis=1, dtype=np.uint64) == n * (n + 1)).all()
                            and (got["pos"].sum(axis=1, dtype=np.uint64) == (x > 0).sum(axis=1)).all())
    if name.startswith("a_"):
        t0 = time.perf_counter()
        stats = group_tests(x, labels, n_groups)
        rec["group_tests_wall_s"] = time.perf_counter() - t0
        try:
            from scipy.stats import mannwhitneyu
        except ImportError:
            mannwhitneyu = None
            say("scipy is not installed: no host loop")
        if mannwhitneyu is not None:
            pairs = [(v, g) for v in range(n_var) for g in range(n_groups)]
            pick = [pairs[i] for i in rng.choice(len(pairs), min(args.scipy_pairs, len(pairs)), replace=False)]
            worst, equal_u = 0.0, True
            t0 = time.perf_counter()
            for v, g in pick:
                ref = mannwhitneyu(x[v, labels == g], x[v, labels != g], alternative="two-sided", method="asymptotic",
                                   use_continuity=True)
                equal_u = equal_u and float(ref.statistic) == float(stats["u"][v, g])
                worst = max(worst, abs(float(stats["p_value"][v, g]) - ref.pvalue) / ref.pvalue)
            loop = time.perf_counter() - t0
            rec["scipy"] = {"pairs_timed": len(pick), "wall_s": loop, "wall_s_scaled_to_all_pairs": loop * len(pairs) / len(pick),
                            "u_equal": equal_u, "p_largest_relative_difference": worst}
            say(name, "scipy loop", json.dumps(rec["scipy"]))
    out[name] = rec
    Path(args.out).write_text(json.dumps(out, indent=1))
    del x, got
say("done")
