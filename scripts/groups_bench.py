"""Engine.group_moments on a C4-shaped run (10,000 cells x 16,569 positions) against the only route there
was before it, a loop of Engine.variant_moments(cells=group) over the same groups, on the same engine in
the same process (profiles/groups/).

Two labellings: (a) 20 groups of about 500 cells, (b) 1,000 groups of about 10 cells. Each is timed three
times either way: wall time around the call(s), and the kernels' device time between two events of the
call's stream (MGP_VAR_PROF, read back from the library's stderr lines). The results of the two routes
are compared. One JSON file.

    python scripts/groups_bench.py [--reads N] [--cells N] [--out FILE]
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

from mgatk2_amd.engine import Engine, EngineConfig  # noqa: E402
from mgatk2_amd.synth import cell_cdf, ref_codes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=200_000_000)
ap.add_argument("--cells", type=int, default=10_000)
ap.add_argument("--out", default="groups_bench.json")
args = ap.parse_args()
READS, CELLS = args.reads, args.cells
out = {"reads": READS, "cells": CELLS}


def say(*a):
    print("[groups_bench]", *a, flush=True)


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


os.environ["MGP_VAR_PROF"] = "1"
seed = 20251015 + 4
cfg = EngineConfig(n_cells=CELLS, min_baseq=20, min_mapq=30, min_distance_from_end=5,
                   dedup_mode="alignment_and_fragment_length", max_strand_bias=1.0, min_reads=1)
rng = np.random.default_rng(seed)
with Engine(cfg) as eng:
    t0 = time.perf_counter()
    eng.synth(seed, READS, cell_cdf(seed, CELLS), ref_codes(seed), read_len=50, rec_align=64, pack=True)
    eng.run()
    eng.sync()
    say(f"run of {READS:,} reads done in {time.perf_counter() - t0:.1f}s")
    for name, n_groups in (("a_20_groups", 20), ("b_1000_groups", 1000)):
        labels = rng.permutation(np.arange(CELLS) % n_groups).astype(np.int32)
        members = [np.flatnonzero(labels == g).astype(np.int32) for g in range(n_groups)]
        rec = {"n_groups": n_groups, "grouped": [], "loop": []}
        for k in range(3):
            got, wall, ms = timed(lambda: eng.group_moments(labels, n_groups))
            rec["grouped"].append({"wall_s": wall, "device_ms": ms})
            say(name, "group_moments", json.dumps(rec["grouped"][-1]))
        for k in range(3):
            loop, wall, ms = timed(lambda: [eng.variant_moments(m) for m in members])
            rec["loop"].append({"wall_s": wall, "device_ms": ms})
            say(name, "variant_moments loop", json.dumps(rec["loop"][-1]))
        rec["equal"] = bool(all(
            np.array_equal(got["fwd"][g] + got["rev"][g], m["s_total"]) and np.array_equal(got["cov"][g], m["s_cov"])
            and np.array_equal(got["n_det"][g], m["n_det"]) and np.array_equal(got["n_conf"][g], m["n_conf"])
            for g, m in enumerate(loop)))
        del loop, got
        out[name] = rec
        Path(args.out).write_text(json.dumps(out, indent=1))
say("done")
