"""The streamed headline's H2D copies per batch, from one
`rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -o run -- python bench.py ...`
run: each copy's duration and rate, split by whether a rows kernel (k_rows_to_host /
k_rows_to_host8) ran beside it.

    python scripts/h2d_table.py DIR/run [--batch-reads 16000000] [--steps 5] > profiles/.../h2d_table.txt

The copy trace carries no byte counts: a batch is the bench's four column copies (2, 2, 2
and 1 byte per read, mgp_push_batch16) and its record copy (64 bytes per read); the run's last
batch may be short, its reads are taken from --reads.
"""

from __future__ import annotations

import argparse
import csv
import statistics


def load(path, pred, key):
    out = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if pred(r[key]):
                out.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    return sorted(out)


def overlap(a, spans):
    return sum(max(0, min(a[1], s[1]) - max(a[0], s[0])) for s in spans)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("prefix", help="DIR/run: the prefix of run_kernel_trace.csv and run_memory_copy_trace.csv")
    ap.add_argument("--batch-reads", type=int, default=16_000_000)
    ap.add_argument("--reads", type=int, default=200_000_000)
    ap.add_argument("--steps", type=int, default=5, help="timed steps: the trace's last steps are tabulated")
    args = ap.parse_args()
    h2d = load(args.prefix + "_memory_copy_trace.csv", lambda d: d.endswith("HOST_TO_DEVICE"), "Direction")
    rows = load(args.prefix + "_kernel_trace.csv", lambda n: n.startswith("k_rows_to_host"), "Kernel_Name")
    nb = -(-args.reads // args.batch_reads)
    # a record copy is by far the longest of its batch: every copy of at least a quarter of the longest
    big = max(e - s for s, e in h2d)
    rec_idx = [i for i, (s, e) in enumerate(h2d) if e - s >= big // 4][-nb * args.steps:]
    assert len(rec_idx) == nb * args.steps, "fewer record copies in the trace than steps x batches"
    per_read = (2, 2, 2, 1, 64)
    names = ("col0", "col1", "col2", "col3", "records")
    print(f"{len(rows)} rows kernels, mean {statistics.mean(e - s for s, e in rows) / 1e6:.3f} ms; "
          f"last {args.steps} steps x {nb} batches of {args.batch_reads} reads")
    print("step batch  " + "  ".join(f"{n:>7s}_ms  GB/s rows_ms" for n in names) + "   batch_ms  GB/s")
    beside = {n: [] for n in names}
    alone = {n: [] for n in names}
    batch_rate = []
    step_ms = []
    for k, i in enumerate(rec_idx):
        step, b = divmod(k, nb)
        reads = args.batch_reads if b < nb - 1 else args.reads - args.batch_reads * (nb - 1)
        line = f"{step:4d} {b:5d}  "
        for j, n in enumerate(names):
            c = h2d[i - 4 + j]
            dur = c[1] - c[0]
            gbs = per_read[j] * reads / dur
            ov = overlap(c, rows)
            (beside if ov > 0.5 * dur or (n == "records" and ov > 0) else alone)[n].append(gbs)
            line += f"{dur / 1e6:10.3f} {gbs:5.1f} {ov / 1e6:7.3f}  "
        span = h2d[i][1] - h2d[i - 4][0]
        batch_rate.append(71 * reads / span)
        line += f" {span / 1e6:9.3f} {batch_rate[-1]:5.1f}"
        print(line)
        if b == nb - 1:
            first = h2d[rec_idx[k - nb + 1] - 4][0]
            step_ms.append((h2d[i][1] - first) / 1e6)
    print()
    print("rate of a copy by what ran beside it (GB/s: median, min-max, copies); a column copy counts as beside")
    print("the rows kernel when more than half of it was, a record copy when any of it was")
    for n in names:
        for what, d in (("alone", alone[n]), ("beside rows", beside[n])):
            if d:
                print(f"  {n:8s} {what:12s} {statistics.median(d):5.1f}  {min(d):5.1f}-{max(d):5.1f}  {len(d)}")
    print(f"whole batches (first column copy's start to the record copy's end): median {statistics.median(batch_rate):.1f} GB/s")
    print("first copy's start to last copy's end per step, ms: " + " ".join(f"{x:.2f}" for x in step_ms))


if __name__ == "__main__":
    main()
