"""load_counts on a C4-shaped output (10,000 cells) against two host baselines, and
analyze --variants end to end (profiles/table_load/).

The count files are written from the synthetic C4 run's rows by the device HDF5 writer; then:
the device load three times, zlib.decompress of the same raw chunks over a 16-thread pool,
analyze_outputs(call_variants=True) twice, load_counts(host_inflate=True) once. One JSON file.

    python scripts/table_bench.py [--reads N] [--cells N] [--dir WORKDIR] [--out FILE]
"""
import argparse
import json
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from mgatk2_amd import h5lite  # noqa: E402
from mgatk2_amd.engine import H5_PLANES, Engine, EngineConfig  # noqa: E402
from mgatk2_amd.file_io.writers import ref_alleles  # noqa: E402
from mgatk2_amd.synth import barcode_names, cell_cdf, ref_codes  # noqa: E402
from mgatk2_amd.table import load_counts  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=200_000_000)
ap.add_argument("--cells", type=int, default=10_000)
ap.add_argument("--dir", default="table_bench_work", help="where the count files and the analyses' outputs go")
ap.add_argument("--out", default="table_bench.json")
args = ap.parse_args()
READS, CELLS = args.reads, args.cells
CHUNKS = (1000, 100)
out = {"reads": READS, "cells": CELLS}


def say(*a):
    print("[table_bench]", *a, flush=True)


def save():
    Path(args.out).write_text(json.dumps(out, indent=1))


seed = 20251015 + 4
d = Path(args.dir)
(d / "output").mkdir(parents=True, exist_ok=True)
t0 = time.perf_counter()
cfg = EngineConfig(n_cells=CELLS, min_baseq=20, min_mapq=30, min_distance_from_end=5,
                   dedup_mode="alignment_and_fragment_length", max_strand_bias=1.0, min_reads=1)
with Engine(cfg) as eng:
    eng.synth(seed, READS, cell_cdf(seed, CELLS), ref_codes(seed), read_len=50, rec_align=64, pack=True)
    eng.run()
    eng.sync()
    say(f"run of {READS:,} reads done in {time.perf_counter() - t0:.1f}s")
    res = eng.fetch(dense=False)
    refs = ref_alleles(res.ref_tally)
    t1 = time.perf_counter()
    tiles = eng.h5_tiles(np.arange(CELLS, dtype=np.int32), chunks=CHUNKS)
    out["h5_tiles_s"] = time.perf_counter() - t1
    say(f"h5_tiles {out['h5_tiles_s']:.2f}s")
    from mgatk2_amd.analysis.variants import run_variants

    t1 = time.perf_counter()
    vr = run_variants(eng, refs, min_cells=5, min_strand_cor=0.65, min_vmr=0.01)
    out["run_variants_on_run_s"] = time.perf_counter() - t1
    out["run_variants_n"] = len(vr.table)
    run_vmr, run_af = vr.table.vmr.copy(), vr.allele_freq
L = cfg.mito_len
names = barcode_names(CELLS, 5)
with h5lite.File(d / "output" / "counts.h5", "w", libver="latest") as f:
    f.create_dataset("barcode", data=np.array(names, dtype="S"))
    for p in H5_PLANES[:10]:
        f.create_dataset_from_chunks(p, (L, CELLS), np.uint16, CHUNKS, 4, tiles[p])
with h5lite.File(d / "output" / "metadata.h5", "w", libver="latest") as f:
    f.create_dataset_from_chunks("coverage", (L, CELLS), np.uint16, CHUNKS, 4, tiles["coverage"])
    f.create_dataset("reference", data=np.array(refs, dtype="S1"))
stored = sum(int(b.size) for p in H5_PLANES for b in tiles[p])
out["stored_bytes"] = stored
out["inflated_bytes"] = 11 * (-(-L // 1000)) * (-(-CELLS // 100)) * 200_000
out["n_chunks"] = sum(len(tiles[p]) for p in H5_PLANES)
del tiles
say(f"files written: {stored / 1e6:.1f} MB stored, {out['n_chunks']} chunks")
save()

# the device path, three times (the first pays the first touch of the files and the allocations)
out["device"] = []
for k in range(3):
    t1 = time.perf_counter()
    with load_counts(d) as t:
        out["device"].append({"wall_s": time.perf_counter() - t1, **t.seconds, "n_saturated": t.n_saturated})
    say("device load", json.dumps(out["device"][-1]))
save()

# (b) zlib.decompress of the same raw chunks over a 16-thread pool
with h5lite.File(d / "output" / "counts.h5", "r") as cf, h5lite.File(d / "output" / "metadata.h5", "r") as mf:
    ds = [cf[p] for p in H5_PLANES[:10]] + [mf["coverage"]]
    nrc, ncc = -(-L // 1000), -(-CELLS // 100)
    t1 = time.perf_counter()
    blobs = []
    for x in ds:
        for rc in range(nrc):
            for cc in range(ncc):
                n, _ = x.chunk_info((rc, cc))
                buf = np.empty(n, np.uint8)
                x.read_chunk((rc, cc), buf)
                blobs.append(buf)
    read_s = time.perf_counter() - t1
for k in range(2):
    t1 = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:
        total = sum(pool.map(lambda b: len(zlib.decompress(b)), blobs, chunksize=64))
    out.setdefault("zlib_pool16", []).append({"read_s": read_s, "inflate_s": time.perf_counter() - t1, "bytes": total})
    say("zlib pool", json.dumps(out["zlib_pool16"][-1]))
del blobs
save()

# analyze --variants end to end (mgatk's customary thresholds), twice
from mgatk2_amd.pipeline import analyze_outputs  # noqa: E402

out["analyze_variants"] = []
for k in range(2):
    t1 = time.perf_counter()
    r = analyze_outputs(d, d / f"an{k}", call_variants=True)
    out["analyze_variants"].append({"wall_s": time.perf_counter() - t1, "variants": r["variants"],
                                    **{k2: v for k2, v in r["timings"].items() if isinstance(v, float)}})
    say("analyze", json.dumps(out["analyze_variants"][-1]))
    res = r["result"]
    out["analyze_equals_run"] = bool(res.variants.vmr.tobytes() == run_vmr.tobytes()
                                     and res.allele_freq.tobytes() == run_af.tobytes())
save()

# (a) host_inflate=True: libhdf5's H5Dread (one thread inflates), once
t1 = time.perf_counter()
with load_counts(d, host_inflate=True) as t:
    out["host_inflate"] = {"wall_s": time.perf_counter() - t1, **t.seconds}
say("host inflate", json.dumps(out["host_inflate"]))
save()
say("done")
