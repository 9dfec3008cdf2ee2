"""The device BGZF inflate (mgp_inflate.hip) against the host pool's, on a
synthetic C4-density BAM (device generator + native writer, level 6):

(a) kernel   the inflate kernel alone on blocks resident in HBM (>= 1 GB inflated in one call,
             and per chunk of 800 blocks): HIP events around the kernel, three calls after a
             warm-up, inflated GB/s;
(b) chunk    one mgp_inflater_run round trip per 16 MiB compressed chunk (H2D, kernel, D2H,
             wait; pinned buffers) against the host pool's inflate of the same chunks on
             --threads threads (the prefetcher's t_inflate counter, MGP_HOST_PROFILE, from a
             streaming decode in a child process), and the same counter with the hook set;
(c) ingest   the pipeline (BamStream into the engine) with and without device_inflate,
             interleaved, three each: ingest and end-to-end seconds.

    python scripts/inflate_bench.py [--reads N] [--cells C] [--threads T] [--out DIR] [--legs a,b,c]

Prints one JSON line; the log goes to stderr.
"""

from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def log(*a):
    print("[inflate]", *a, file=sys.stderr, flush=True)


def make_bam(out: Path, reads: int, cells: int, threads: int):
    from mgatk2_amd.bam import write_bam
    from mgatk2_amd.engine import Engine, EngineConfig
    from mgatk2_amd.synth import barcode_names, cell_cdf, ref_codes

    seed = 20251015 + 3
    names = barcode_names(cells, seed)
    bam = out / f"inflate_{reads}_{cells}.bam"
    if not bam.exists():
        t = time.time()
        with Engine(EngineConfig(n_cells=cells), device=0) as eng:
            eng.synth(seed, reads, cell_cdf(seed, cells), ref_codes(seed), read_len=50)
            soa = eng.download_inputs()
        write_bam(bam, soa, names, level=6, n_threads=threads)
        del soa
        log(f"BAM {bam.stat().st_size / 1e9:.2f} GB written in {time.time() - t:.1f}s")
    return bam, names


def block_table(data: np.ndarray, max_inflated: int | None = None):
    """coff, clen, isize of the BGZF blocks of a file's bytes (up to max_inflated bytes)."""
    coff, clen, isize = [], [], []
    p, total, n = 0, 0, data.shape[0]
    while p + 18 <= n:
        xlen = int(data[p + 10]) | int(data[p + 11]) << 8
        bsize = (int(data[p + 16]) | int(data[p + 17]) << 8) + 1
        sz = int.from_bytes(data[p + bsize - 4:p + bsize].tobytes(), "little")
        if sz:
            coff.append(p + 12 + xlen)
            clen.append(bsize - 12 - xlen - 8)
            isize.append(sz)
            total += sz
        p += bsize
        if max_inflated is not None and total >= max_inflated:
            break
    return np.array(coff, np.uint64), np.array(clen, np.uint32), np.array(isize, np.uint32), p


def gbps(nbytes: int, ms: float) -> float:
    return round(nbytes / 1e6 / max(ms, 1e-9), 3)


def leg_kernel_and_chunk(bam: Path, threads: int) -> dict:
    from mgatk2_amd import engine

    res = {}
    raw = np.fromfile(bam, np.uint8, count=min(bam.stat().st_size, 700 << 20))
    coff, clen, isize, used = block_table(raw, max_inflated=1_050_000_000)
    ooff = np.concatenate([[0], np.cumsum(isize[:-1], dtype=np.uint64)]).astype(np.uint64)
    total = int(isize.sum(dtype=np.uint64))
    log(f"{coff.shape[0]} blocks, {used / 1e6:.1f} MB compressed, {total / 1e6:.1f} MB inflated")
    pin_src = engine.PinnedBuffer(used)
    pin_out = engine.PinnedBuffer(total)
    src = pin_src.array(used, np.uint8)
    src[:] = raw[:used]
    out = pin_out.array(total, np.uint8)

    def kernel_ms(inf, *args, calls=3):
        inf.run(*args)  # warm-up
        ms = []
        for _ in range(calls):
            t0 = inf.times()
            st = inf.run(*args)
            assert not st.any(), "a block was refused"
            t1 = inf.times()
            ms.append({k: t1[k] - t0[k] for k in ("h2d_ms", "kernel_ms", "d2h_ms")})
        return ms

    # (a) everything in one call: the kernel's own time over >= 1 GB inflated
    with engine.Inflater(0, used, total) as inf:
        ms = kernel_ms(inf, src, coff, clen, isize, ooff, out)
        res["a_whole"] = {"blocks": int(coff.shape[0]), "inflated_bytes": total, "compressed_bytes": used,
                          "kernel_ms": [round(m["kernel_ms"], 3) for m in ms],
                          "kernel_GBps_inflated": [gbps(total, m["kernel_ms"]) for m in ms]}
        log("a_whole", res["a_whole"])
        # check a sample against zlib
        import zlib

        for i in (0, coff.shape[0] // 2, coff.shape[0] - 1):
            a, b = int(coff[i]), int(ooff[i])
            assert zlib.decompress(src[a:a + int(clen[i])].tobytes(), -15) == out[b:b + int(isize[i])].tobytes()
    # (a) per chunk of 800 blocks, (b) per 16 MiB compressed chunk: round trips from pinned memory
    for key, pick in (("a_800_blocks", lambda i0: min(i0 + 800, coff.shape[0])),
                      ("b_16MiB_chunk", lambda i0: int(np.searchsorted(coff, coff[i0] + np.uint64(16 << 20))))):
        rows = []
        with engine.Inflater(0, 17 << 20, 256 << 20) as inf:
            i0, k = 0, 0
            while i0 < coff.shape[0] and k < 6:
                i1 = max(pick(i0), i0 + 1)
                lo = int(coff[i0]) - 18
                hi = int(coff[i1 - 1]) + int(clen[i1 - 1]) + 8
                if hi - lo > 17 << 20:
                    break
                c_coff = coff[i0:i1] - np.uint64(lo)
                c_ooff = ooff[i0:i1] - ooff[i0]
                nb = int(isize[i0:i1].sum(dtype=np.uint64))
                args = (src[lo:hi], c_coff, clen[i0:i1], isize[i0:i1], c_ooff, out[:nb])
                ms = kernel_ms(inf, *args, calls=3)
                walls = []
                for _ in range(3):
                    t = time.perf_counter()
                    inf.run(*args)
                    walls.append((time.perf_counter() - t) * 1e3)
                best = min(ms, key=lambda m: m["kernel_ms"])
                rows.append({"blocks": i1 - i0, "compressed_bytes": hi - lo, "inflated_bytes": nb,
                             "h2d_ms": round(best["h2d_ms"], 3), "kernel_ms": round(best["kernel_ms"], 3),
                             "d2h_ms": round(best["d2h_ms"], 3), "round_trip_wall_ms": round(min(walls), 3),
                             "kernel_GBps_inflated": gbps(nb, best["kernel_ms"]),
                             "round_trip_GBps_inflated": gbps(nb, min(walls))})
                i0, k = i1, k + 1
        res[key] = rows
        log(key, rows)
    del src, out
    # (b) the host pool on the same file: the prefetcher's inflate counter of a streaming decode,
    # host inflate and hook, each in a child process of its own
    for flag in ("0", "1", "0", "1"):
        env = dict(os.environ, MGP_HOST_PROFILE="1")
        r = subprocess.run([sys.executable, __file__, "--leg-stream", str(bam), "--threads", str(threads),
                            "--device-inflate", flag], env=env, capture_output=True, text=True, timeout=900)
        m = re.search(r"prefetch: read ([0-9.]+), inflate ([0-9.]+), walk ([0-9.]+); (\d+) \+ (\d+) chunks", r.stderr)
        line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "{}"
        row = json.loads(line)
        if m:
            chunks = int(m.group(4)) + int(m.group(5))
            row.update(prefetch_read_s=float(m.group(1)), prefetch_inflate_s=float(m.group(2)),
                       prefetch_walk_s=float(m.group(3)), chunks=chunks,
                       inflate_ms_per_chunk=round(float(m.group(2)) * 1e3 / max(chunks, 1), 3))
        else:
            row["stderr"] = r.stderr[-2000:]
        res.setdefault("b_stream_" + ("device" if flag == "1" else "host"), []).append(row)
        log("b_stream", flag, row)
    return res


def leg_stream(bam: str, threads: int, device_inflate: bool):
    """A streaming decode of the whole file into one slot (decode_bench.py's loop); with the
    flag the blocks go through the device. Prints the seconds and the inflater's device times."""
    from mgatk2_amd.bam import BamFile, StreamSlot
    from mgatk2_amd.synth import barcode_names

    m = re.search(r"inflate_(\d+)_(\d+)\.bam", bam)
    names = barcode_names(int(m.group(2)), 20251015 + 3)
    slot = StreamSlot(4_000_000, 4_000_000 * 64 + (64 << 20))
    t = time.time()
    n = 0
    with BamFile(bam, n_threads=threads) as bf:
        if device_inflate:
            bf.set_device_inflate(0)
        with bf.stream("chrM", names, paired=False) as st:
            while st.next_into(slot):
                n += slot.n
        times = bf._inflater.times() if device_inflate else {}
    print(json.dumps({"reads": n, "seconds": round(time.time() - t, 3), "device_inflate": device_inflate,
                      **{k: round(v, 2) if isinstance(v, float) else v for k, v in times.items()}}))


def leg_ingest(bam: Path, names, threads: int, out: Path, fmt: str) -> dict:
    import shutil

    from mgatk2_amd.config import PipelineConfig
    from mgatk2_amd.pipeline import MtDNAPipeline

    rows = {"host": [], "device": []}
    for rep in range(3):
        for flag in (False, True):
            cfg = PipelineConfig(min_baseq=20, min_mapq=30, max_strand_bias=1.0, min_reads_per_cell=1,
                                 n_cores=threads, device_inflate=flag, inflate_device=0)
            od = out / f"run_{int(flag)}"
            t = time.time()
            p = MtDNAPipeline(str(bam), names, od, config=cfg, output_format=fmt, stream=True)
            p.run()
            wall = time.time() - t
            row = {"wall_s": round(wall, 3), **{k: round(v, 3) for k, v in p.timings.items() if isinstance(v, float)}}
            rows["device" if flag else "host"].append(row)
            log("c", "device" if flag else "host", row)
            shutil.rmtree(od, ignore_errors=True)
    return {"c_ingest_" + fmt: rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--cells", type=int, default=1_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default="/tmp/mgp_inflate_bench")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--format", default="hdf5")
    ap.add_argument("--leg-stream", default=None, help="(internal) the streaming decode of this BAM, then exit")
    ap.add_argument("--device-inflate", default="0")
    args = ap.parse_args()
    if args.leg_stream:
        return leg_stream(args.leg_stream, args.threads, args.device_inflate == "1")
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    bam, names = make_bam(out, args.reads, args.cells, args.threads)
    res = {"reads": args.reads, "cells": args.cells, "threads": args.threads, "bam_bytes": bam.stat().st_size}
    legs = args.legs.split(",")
    if "a" in legs or "b" in legs:
        res.update(leg_kernel_and_chunk(bam, args.threads))
    if "c" in legs:
        res.update(leg_ingest(bam, names, args.threads, out, args.format))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
