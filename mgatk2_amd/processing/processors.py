"""Cell processing (mirror of src/processing/processors.py).

The reference dispatches one Python call per cell, sequentially or over a
spawn pool (processors.py:63-144). Here every cell goes through the GPU engine
in one run:

* :meth:`CellProcessor.process_soa` — production path: the whole chrM read set
  (engine SoA, BAM order) in, dedup + pileup + filters + statistics on the GPU,
  results streamed to the writer in first-seen cell order.
* :meth:`CellProcessor.process_cells_progressive` / :func:`process_barcode_worker`
  — the reference's dict API (already-deduplicated ``SimpleRead`` lists per
  barcode). The lists are merged into one coordinate-sorted batch and run with
  dedup off, so each cell sees exactly its own reads.
"""

from __future__ import annotations

import gc
import logging
import os
import threading
import time
from functools import partialmethod
from queue import Queue

import numpy as np

from ..engine import Engine, EngineResult, PinnedBuffer, Rows16
from ..exceptions import InvalidInputError
from ..shard import (DeviceParts, copy_part, merge_results, merged_stats, partition_cells, reads_per_cell,
                     shard_soa)
from ..synth import ReadSoA, pack_reads
from .device_writers import write_h5, write_txt
from .pileup import result_dict, simple_reads_to_dicts

logger = logging.getLogger(__name__)

MP_CONTEXT = "spawn"  # kept for API compatibility (processors.py:17); no process pool is used

# streamed runs: reads per decoded batch and batches in flight (MGP_STREAM_BATCH /
# MGP_STREAM_SLOTS override them, read at each run)
STREAM_BATCH_READS = 4_000_000
STREAM_SLOTS = 3


def _engine_config_for(config, n_cells: int, dedup: bool):
    ec = config.engine_config(n_cells)
    if not dedup:
        ec.dedup_mode = "none"
    return ec


def run_cells_from_reads(config, reads_by_barcode: dict, device: int = 0) -> tuple[EngineResult, list[str]]:
    """Engine run over already-deduplicated per-barcode read lists."""
    barcodes = list(reads_by_barcode)
    dicts = []
    for i, bc in enumerate(barcodes):
        dicts.extend(simple_reads_to_dicts(reads_by_barcode[bc], bc=i))
    dicts.sort(key=lambda d: d["reference_start"])  # stable: per-cell order is kept
    soa = pack_reads(dicts)
    with Engine(_engine_config_for(config, len(barcodes), dedup=False), device=device) as eng:
        eng.push(soa)
        res = eng.finish()
    return res, barcodes


def process_barcode_worker(args):
    """processors.py:20-55: one barcode's reads -> result dict or None."""
    barcode, reads, config = args
    if not reads or len(reads) < config.min_reads_per_cell:
        return None
    res, _ = run_cells_from_reads(config, {barcode: reads})
    if not res.passed[0]:
        return None
    return result_dict(res, 0, barcode, config.mito_length)


def _pinned_alloc(nbytes: int):
    """alloc(m, dtype) -> consecutive 64-byte aligned views of one pinned buffer."""
    pb = PinnedBuffer(nbytes)
    off = [0]

    def alloc(m, dt):
        a = pb.array(m, dt, off[0])
        off[0] = (off[0] + m * np.dtype(dt).itemsize + 63) & ~63
        return a

    return alloc


def _link_bytes(soa: ReadSoA) -> int:
    """Host-to-device bytes of a pushed batch (its columns and payload)."""
    return sum(int(a.nbytes) for a in (soa.start, soa.bc, soa.tlen, soa.flag, soa.mapq, soa.span, soa.rec_off,
                                       soa.payload) if a is not None)


def _payload_hint(n_reads: int, n_cells: int = 0, batch_reads: int = STREAM_BATCH_READS) -> int:
    """Device payload bytes a streamed run of n_reads needs at once (no regrowth, which
    waits for the queued segments): 64-byte records plus what the on-device pairing
    reserves (mgp_push_batch: one half-empty line per cell and key range of 2^18 reads,
    per batch), or 32-byte records four per line plus their lines."""
    if os.environ.get("MGP_RECORDS", "64") == "32":
        return int(n_reads) * 40 + (64 << 20)
    ranges = -(-int(n_reads) // (1 << 18)) + -(-int(n_reads) // max(1, int(batch_reads))) + 1
    return int(n_reads) * 64 + ranges * (int(n_cells) + 2) * 64 + (64 << 20)


def _rows_slice(r: Rows16, lo: int, hi: int) -> Rows16:
    """The cells [lo, hi) of 16-bit rows, as views."""
    return Rows16(r.counts[lo:hi], r.tn5[lo:hi], r.depth[lo:hi], r.wide[lo:hi], r.window_width)


class _RowsTarget:
    """The rows target of a streamed run: pinned 16-bit result rows for all n_cells cells
    (GBs of pinned memory: ~0.25 s per GB to pin), allocated on a thread of its own while the
    first batches go in. The engine copies the rows of the windows piled before its target is
    set when it is set (ABI 4). `windows`: the engine's windows()."""

    def __init__(self, n_cells: int, L: int, windows: tuple[int, int]):
        self._rows, self._err = None, None
        self._thread = threading.Thread(target=self._alloc, args=(n_cells, L, *windows), name="mgp-rows-alloc",
                                        daemon=True)
        self._thread.start()

    def _alloc(self, n_cells, L, nw, W):
        try:
            if n_cells > 0:
                rb = PinnedBuffer(n_cells * L * 22 + n_cells * nw + 4096)
                self._rows = Rows16(
                    rb.array((n_cells, L, 8), np.uint16, 0), rb.array((n_cells, L, 2), np.uint16, n_cells * L * 16),
                    rb.array((n_cells, L), np.uint16, n_cells * L * 20),
                    rb.array((n_cells, nw), np.uint8, n_cells * L * 22), W)
        except BaseException as e:  # noqa: BLE001 - re-raised by take
            self._err = e

    def ready(self) -> bool:
        """Whether take() would return at once (never blocks)."""
        return not self._thread.is_alive()

    def take(self) -> Rows16 | None:
        """The rows once allocated (None without cells); the allocation's exception raised here."""
        self._thread.join()
        if self._err is not None:
            raise self._err
        return self._rows


class CellProcessor:
    def __init__(self, config, output_dir, device: int = 0, devices: list[int] | None = None):
        self.config = config
        self.output_dir = output_dir
        self.device = device
        self.devices = list(devices) if devices else [device]
        self.last_result: EngineResult | None = None
        self.last_stats: dict = {}
        self.last_timing: dict = {}
        self.txt_out = None
        self.h5_out = None
        self.variants_opt: dict | None = None
        self.coverage_opt: dict | None = None
        self.groups_opt: dict | None = None
        self.pca_opt: dict | None = None
        self.stage_opt: dict[str, dict] = {}  # the analyses turned on (enable), by stage key
        # what a loaded table sets (analyze_outputs): the file's reference alleles in place of the
        # tally's, and the population in place of every cell (a subset of the file's columns)
        self.reference: list[str] | None = None
        self.population: np.ndarray | None = None

    # txt output on the device ----------------------------------------------
    def enable_device_txt(self, prefix, names: list[str]):
        """Write the txt count files (`prefix`.{coverage,A,C,G,T}.txt.gz, appended) from
        the devices' rows before their contexts close: each passing cell's lines
        formatted and deflated on its device (mgp_txt_gz, writers.py:430-486), only the
        gzip members cross the link. The run's result then carries `txt_gz_cells`, the
        cells written, and IncrementalTextWriter.write_cells writes only the rest
        (stats, depth table, reference alleles). MGP_TXT_DEVICE=0, or a gzip level other
        than the reference's 9 (MGP_GZIP_LEVEL), keeps the host formatter."""
        self.txt_out = (str(prefix), list(names))

    def enable_device_h5(self, names: list[str]):
        """Deflate the HDF5 count datasets' chunks (writers.py:60-131) on the devices before
        their contexts close (mgp_h5_tiles): the run's result then carries `h5_tiles`, which
        IncrementalHDF5Writer.finalize writes instead of deflating the planes on the host.
        `names`: the writer's barcodes (its columns). MGP_H5_DEVICE=0 keeps the host deflate."""
        self.h5_out = list(names)

    def enable_variants(self, min_cells: int = 0, min_strand_cor: float = 0, min_vmr: float = 0,
                        stabilize_variance: bool = False, low_coverage_threshold: int = 10, min_coverage: int = 1):
        """Call variants from the devices' rows before their contexts close (mgp_variant_*,
        mgp_allele_freq_*; analysis/variants.py): the run's result then carries `variants`,
        the table of identify_variants over every cell of the run (cells that did not pass
        count as all-zero rows, the zero columns of counts.h5), and `allele_freq`, the
        heteroplasmy matrix [n_variants, n_cells] of the variants that pass. The defaults
        are R's (no filtering)."""
        self.variants_opt = dict(min_cells=min_cells, min_strand_cor=min_strand_cor, min_vmr=min_vmr,
                                 stabilize_variance=stabilize_variance,
                                 low_coverage_threshold=low_coverage_threshold, min_coverage=min_coverage)

    def _call_variants(self, res: EngineResult, parts: DeviceParts) -> None:
        """Pass 1 on every part (the devices concurrently), the host merge, pass 2, the
        table, then the matrix of the passing variants, each part filling its own columns."""
        from ..analysis.variants import run_variants

        pop, ref = self._analysis_population(res), self.run_reference(res)
        cov = res.coverage
        if self.coverage_opt is not None and cov is not None:
            # the vignette's order: the variants of the kept cells, with their own reference
            res.variant_cells = np.flatnonzero(cov.kept)
            pop = cov.kept_cells
            if cov.ref_alleles is not None:
                ref = cov.ref_alleles
        vr = run_variants(parts, ref, cells=pop, **self.variants_opt)
        res.variants, res.allele_freq, res.variant_seconds = vr.table, vr.allele_freq, vr.seconds

    def enable(self, key: str, **options):
        """Turn on the analysis `key` of the run's heteroplasmy matrix (analysis/stages.py), made by stage_result.
        The stage it needs must be on and every option passes its analysis's own checker (InvalidInputError)."""
        from ..analysis.stages import STAGES

        stage = STAGES[key]
        if (self.variants_opt if stage.needs == "variants" else self.stage_opt.get(stage.needs)) is None:
            raise InvalidInputError(stage.refusal)
        self.stage_opt[key] = {name: check(options.get(name, default)) for name, default, check in stage.options}

    def stage_result(self, key: str, res: EngineResult):
        """The analysis `key` of a finished run's matrix (res.allele_freq, host-merged from every part), on
        the first device, after the run's engine contexts have closed; the stages in their declared order.
        Sets the stage's field of res and last_timing[key]; returns the result (None when not enabled)."""
        if key not in self.stage_opt:
            return None
        from ..analysis.stages import STAGES

        t0 = time.perf_counter()
        try:
            setattr(res, STAGES[key].field, STAGES[key].compute(res, self.devices[0], **self.stage_opt[key]))
        finally:
            self.last_timing[key] = time.perf_counter() - t0
        return getattr(res, STAGES[key].field)

    def enable_clustering(self, clones: int | None = None):
        self.enable("cluster", clones=clones)

    def enable_neighbors(self, neighbors: int = 20, prune: float = 1.0 / 15.0):
        self.enable("neighbors", neighbors=neighbors, prune=prune)

    def enable_clonotypes(self, resolution: float = 1.0):
        self.enable("clonotypes", resolution=resolution)

    def enable_pca(self, n_comp: int, scale: bool = False):
        """The principal components of the run's heteroplasmy matrix (mgp_pca; analysis/pca.py), made by
        pca_result: the first n_comp (1..50, clipped to what the matrix has), the variants scaled to unit
        variance with `scale`. Needs enable_variants (InvalidInputError otherwise)."""
        from ..analysis.pca import check_pca

        if self.variants_opt is None:
            raise InvalidInputError("pca requires call_variants")
        self.pca_opt = dict(n_comp=check_pca(n_comp), scale=bool(scale))

    def pca_result(self, res: EngineResult):
        """The principal components of a finished run's matrix (res.allele_freq with res.variants' names), on
        the first device, after the run's engine contexts have closed, as stage_result. Sets res.pca and
        last_timing["pca"]; returns the PcaResult (None when not enabled)."""
        if self.pca_opt is None:
            return None
        from ..analysis.pca import principal_components

        t0 = time.perf_counter()
        try:
            res.pca = principal_components(res.allele_freq, table=res.variants, device=self.devices[0], **self.pca_opt)
        finally:
            self.last_timing["pca"] = time.perf_counter() - t0
        return res.pca

    cluster_result = partialmethod(stage_result, "cluster")
    neighbor_result = partialmethod(stage_result, "neighbors")
    clonotype_result = partialmethod(stage_result, "clonotypes")
    cluster_opt = property(lambda self: self.stage_opt.get("cluster"))
    neighbors_opt = property(lambda self: self.stage_opt.get("neighbors"))
    clonotypes_opt = property(lambda self: self.stage_opt.get("clonotypes"))

    @staticmethod
    def _population(res: EngineResult) -> np.ndarray:
        """The run's default population: every cell, -1 (an all-zero row) for those that did
        not pass, the zero columns of counts.h5."""
        n_cells = int(res.passed.shape[0])
        return np.where(res.passed.astype(bool), np.arange(n_cells, dtype=np.int64), -1)

    def _analysis_population(self, res: EngineResult) -> np.ndarray:
        return self._population(res) if self.population is None else self.population

    def run_reference(self, res: EngineResult) -> list[str]:
        """The reference alleles the analyses of `res` go by: the tally's, or a loaded table's file's."""
        from ..file_io.writers import ref_alleles

        return ref_alleles(res.ref_tally) if self.reference is None else list(self.reference)

    def enable_coverage(self, min_mean_coverage: float = 0.0, min_coverage_breadth: float = 0.0,
                        recompute_reference: bool = False):
        """Coverage QC from the devices' rows before their contexts close (mgp_cell_coverage_*,
        mgp_position_*; analysis/coverage.py): the run's result then carries `coverage`, a
        CoverageResult with the cell table over every cell of the run (cells that did not
        pass count as all-zero rows), the kept mask of filter_cells_by_coverage (both
        thresholds inclusive; at 0 every cell is kept), the position, strand and
        transposition tables of the kept cells and, with recompute_reference, their
        reference alleles. With enable_variants too, the variants are called over the kept
        cells (allele_freq has one column per kept cell, `variant_cells` their indices), with
        the recomputed reference when there is one."""
        self.coverage_opt = dict(min_mean_coverage=float(min_mean_coverage),
                                 min_coverage_breadth=float(min_coverage_breadth),
                                 recompute_reference=bool(recompute_reference))

    def _call_coverage(self, res: EngineResult, parts: DeviceParts) -> None:
        from ..analysis.coverage import run_coverage

        res.coverage = run_coverage(parts, cells=self._analysis_population(res), **self.coverage_opt)

    def enable_groups(self, labels, group_names: list[str], min_cells: int = 2, min_af: float = 0.01,
                      group_test: bool = False, group_test_max_p: float = 0.01):
        """Pseudobulk counts and marker variants per cell group from the devices' rows before their contexts
        close (mgp_group_moments; analysis/groups.py): the run's result then carries `groups`, a GroupResult.
        labels[c]: the group number of the run's cell c (of a loaded table's column c), 0 .. len(group_names)
        - 1, or -1 for a cell in no group. The population is the variants': every cell of the run (one that
        did not pass is an all-zero row and counts in its group's n_cells only), or the coverage filter's
        kept cells, with the recomputed reference when there is one. The thresholds of the marker variants
        are this project's choice; mgatk defines none. group_test: also the rank-sum test of each tested
        variant, every group against the rest of the population (mgp_rank_sums; analysis/group_tests.py), the
        pairs with a p-value up to group_test_max_p kept: the GroupResult's `tests`."""
        from ..analysis.group_tests import check_group_test_max_p
        from ..analysis.groups import check_group_min_af, check_group_min_cells

        labels = np.ascontiguousarray(labels, np.int32)
        if not group_names or (labels.size and (labels.min() < -1 or labels.max() >= len(group_names))):
            raise InvalidInputError("enable_groups: a label is outside the group names")
        self.groups_opt = dict(labels=labels, group_names=list(group_names), min_cells=check_group_min_cells(min_cells),
                               min_af=check_group_min_af(min_af), test=bool(group_test),
                               test_max_p=check_group_test_max_p(group_test_max_p))

    def _call_groups(self, res: EngineResult, parts: DeviceParts) -> None:
        from ..analysis.groups import group_result

        opt = self.groups_opt
        pop, ref = self._analysis_population(res), self.run_reference(res)
        # the cell (or column) each entry of the population is, whether it has rows or not
        ids = np.arange(pop.size, dtype=np.int64) if self.population is None else np.asarray(self.population, np.int64)
        cov = res.coverage
        if self.coverage_opt is not None and cov is not None:  # (as _call_variants)
            pop, ids = cov.kept_cells, ids[cov.kept]
            if cov.ref_alleles is not None:
                ref = cov.ref_alleles
        if ids.size and int(ids.max()) >= opt["labels"].size:
            raise InvalidInputError(f"enable_groups: {opt['labels'].size} labels for a run of more cells")
        labels = np.where(ids >= 0, opt["labels"][np.maximum(ids, 0)], -1)
        res.groups = group_result(parts, labels, opt["group_names"], ref, cells=pop, min_cells=opt["min_cells"],
                                  min_af=opt["min_af"], variants=res.variants)
        if opt["test"]:
            # the marker variants and the run's called ones, ranked over the same population on the first device;
            # their matrix by the route (and with the minimum coverage) of the variants' own
            from ..analysis.group_tests import run_group_tests

            t0 = time.perf_counter()
            min_cov = 1 if self.variants_opt is None else self.variants_opt["min_coverage"]
            res.groups.tests = run_group_tests(parts, res.groups.markers, labels, len(opt["group_names"]), ref,
                                               cells=pop, variants=res.variants, min_coverage=min_cov,
                                               max_p=opt["test_max_p"], device=self.devices[0])
            res.groups.seconds["tests"] = time.perf_counter() - t0

    def _h5_device_on(self) -> bool:
        return self.h5_out is not None and os.environ.get("MGP_H5_DEVICE", "1") != "0"

    def _txt_device_on(self) -> bool:
        if self.txt_out is None or os.environ.get("MGP_TXT_DEVICE", "1") == "0":
            return False
        return os.environ.get("MGP_GZIP_LEVEL", "9") == "9"

    def _write_txt(self, res: EngineResult, parts) -> None:
        write_txt(res, DeviceParts(parts), *self.txt_out)

    def _write_h5(self, res: EngineResult, parts) -> None:
        write_h5(res, DeviceParts(parts), self.h5_out, self.config.mito_length)

    def _after_run(self, res: EngineResult, parts: list, writers: bool = True) -> dict:
        """What is made of the devices' rows while their contexts are open, over parts =
        [(engine, lo, hi)] (shard.DeviceParts): the device txt writer, the device HDF5 writer,
        the coverage pass, then the variants (which use its kept cells), then the groups (which
        use both), each when enabled. Returns the seconds of each under its last_timing key:
        txt_device and h5_device always (writers=False: neither is run nor reported), coverage,
        variants and groups when enabled. A run without cells has no parts and makes nothing."""
        steps = [("coverage", self.coverage_opt is not None, self._call_coverage),
                 ("variants", self.variants_opt is not None, self._call_variants),
                 ("groups", self.groups_opt is not None, self._call_groups)]
        seconds = {}
        if writers:
            steps = [("txt_device", self._txt_device_on(), self._write_txt),
                     ("h5_device", self._h5_device_on(), self._write_h5)] + steps
            seconds = {"txt_device": 0.0, "h5_device": 0.0}
        live = DeviceParts(parts) if parts else None
        for key, on, step in steps:
            if on:
                t0 = time.perf_counter()
                if live is not None:
                    step(res, live)
                seconds[key] = time.perf_counter() - t0
        return seconds

    # production path ------------------------------------------------------
    def run_soa(self, soa_batches, n_cells: int) -> EngineResult:
        """Whole read set (one or more BAM-order batches) through the engine:
        filters, dedup, pileup, strand filter, per-cell statistics, tallies."""
        if isinstance(soa_batches, ReadSoA):
            soa_batches = [soa_batches]
        if len(self.devices) > 1:
            return self._run_sharded(soa_batches, n_cells)
        n = sum(b.n for b in soa_batches)
        pay = sum(int(b.payload.shape[0]) for b in soa_batches)
        ec = self.config.engine_config(n_cells, reserve_reads=n, reserve_payload=pay + 256 * len(soa_batches))
        t0 = time.perf_counter()
        with Engine(ec, device=self.device) as eng:
            t1 = time.perf_counter()
            for b in soa_batches:
                eng.push(b)
            eng.run()
            eng.sync()
            t2 = time.perf_counter()
            res = eng.fetch_compact()  # exact 16-bit rows: half the device-to-host bytes
            t3 = time.perf_counter()
            self.last_stats = eng.kernel_times()
            tail = self._after_run(res, [(eng, 0, n_cells)])
        t4 = time.perf_counter()
        # where the engine leg goes (pipeline timings): context + allocation, H2D of
        # the batches + the run, D2H of the results, teardown
        self.last_timing = {"engine_open": t1 - t0, "engine_h2d_run": t2 - t1, "engine_d2h": t3 - t2,
                            "engine_close": t4 - t3 - sum(tail.values()), **tail}
        self.last_result = res
        return res

    def _stream_producer(self, reader, n_cells: int, batch_reads: int | None, pinned: bool = True):
        """The decode side of a streamed run: the native streaming decoder filling a
        ring of batches (pinned: the engine copies from them; pinned=False: the router
        reads them on the host) on a producer thread. Returns (bam, stream, expected
        reads, free queue, full queue, thread, times); the consumer takes filled slots
        from `full` (None at the end, an exception on error) and hands them back
        through `free` (None stops the producer)."""
        from ..bam import StreamSlot

        bam, st, expected = reader.open_stream()
        n_hint = expected if expected > 0 else max(1, os.path.getsize(reader.bam_path) // 30)
        batch_reads = batch_reads or int(os.environ.get("MGP_STREAM_BATCH", STREAM_BATCH_READS))
        n_slots = max(2, int(os.environ.get("MGP_STREAM_SLOTS", STREAM_SLOTS)))
        cap_reads = max(1, min(int(batch_reads), n_hint + 1))
        cap_payload = cap_reads * 48 + 256 * (n_cells + 1) + (1 << 20)
        slot_bytes = StreamSlot.nbytes(cap_reads, cap_payload)
        free: Queue = Queue()
        full: Queue = Queue()
        for _ in range(n_slots):
            free.put(StreamSlot(cap_reads, cap_payload, _pinned_alloc(slot_bytes) if pinned else None))
        times = {"cap_reads": cap_reads, "cap_payload": cap_payload}

        def produce():
            try:
                while True:
                    sl = free.get()
                    if sl is None:
                        return
                    n = st.next_into(sl)
                    full.put(sl if n else None)
                    if not n:
                        times["decode_end"] = time.perf_counter()
                        return
            except BaseException as e:  # noqa: BLE001 - handed to the consumer
                full.put(e)

        producer = threading.Thread(target=produce, name="mgp-bam-decode", daemon=True)
        producer.start()
        return bam, st, n_hint, free, full, producer, times

    @staticmethod
    def _push_view(item, n_cells: int) -> ReadSoA:
        """A decoded batch as pushed. Records dense in BAM order at one stride (every
        offset checked: a paired placement can give the same payload size with its
        records permuted) go without their rec_off / start / span columns (ABI 4: the
        engine places and pairs them on the device and takes start and span from the
        records), and with 16-bit barcode and |tlen| columns when every key fits
        (mgp_push_batch16, ABI 5: 7 bytes of columns per read over the link instead of
        11; MGP_COLUMNS16=0 keeps the 32-bit ones); any other batch with its offsets."""
        from ..bam import batch_columns16

        soa = item.soa()
        n = soa.n
        if not n:
            return soa
        rc = batch_columns16(soa, n_cells, item.bc16, item.tlen16)
        if rc == 3 and os.environ.get("MGP_COLUMNS16", "1") != "0":
            return ReadSoA(None, item.bc16[:n], item.tlen16[:n], soa.flag, soa.mapq, None, None, soa.payload)
        if rc & 1:
            return ReadSoA(None, soa.bc, soa.tlen, soa.flag, soa.mapq, None, None, soa.payload)
        return soa

    def run_stream(self, reader, n_cells: int, batch_reads: int | None = None,
                   rows_target: bool | None = None) -> EngineResult:
        """The production path, streamed (readers.py:84-93's one pass, overlapped with
        the device): the native decoder fills a ring of pinned batches on a producer
        thread while this thread pushes each finished batch to a streaming engine
        context (MGP_CFG_STREAM: its H2D copies, then the hot path of the position
        windows it completes, run behind the next batches' decode); the 16-bit result
        rows are fetched after the run. With a rows target (rows_target=True or
        MGP_ROWS_TARGET=1), each window's rows leave the device as soon as it is piled,
        into pinned host memory the writers read. Results are those of a
        resident run of the same reads (reads a segment cannot serve rerun it).
        Several devices: see :meth:`_run_stream_sharded`."""
        if rows_target is None:
            # the rows fetched after the run by default: pinning a rows target during the
            # decode (GBs at ~0.25 s per GB, on a thread) slowed the decode more than the
            # fetch costs (C4 txt end to end 5.38-5.43 s with the target, 4.72-5.26 s
            # without, fetch 0.16 s; profiles/r05/e2e_rows_*.log); MGP_ROWS_TARGET=1 keeps it
            rows_target = os.environ.get("MGP_ROWS_TARGET", "0") == "1"
        if len(self.devices) > 1:
            return self._run_stream_sharded(reader, n_cells, batch_reads, rows_target)
        t0 = time.perf_counter()
        bam, st, n_hint, free, full, producer, times = self._stream_producer(reader, n_cells, batch_reads)
        try:
            ec = self.config.engine_config(n_cells, reserve_reads=n_hint,
                                           reserve_payload=_payload_hint(n_hint, n_cells, times["cap_reads"]))
            ec.stream = True
            eng = Engine(ec, device=self.device)
            try:
                # the rows target is pinned while the first batches go in, and set when it is ready
                target = _RowsTarget(n_cells, self.config.mito_length, eng.windows()) \
                    if rows_target and n_cells > 0 else None
                rows = None

                def settle(wait: bool):
                    nonlocal rows, target
                    if target is None or not (wait or target.ready()):
                        return
                    rows, target = target.take(), None
                    if rows is not None:
                        eng.set_rows16_target(rows)

                t1 = time.perf_counter()
                n_batches, h2d = 0, 0
                while True:
                    item = full.get()
                    if item is None:
                        break
                    if isinstance(item, BaseException):
                        raise item
                    if n_batches == 0:
                        times["first_batch"] = time.perf_counter()
                    settle(False)
                    view = self._push_view(item, n_cells)
                    eng.push(view)
                    h2d += _link_bytes(view)
                    eng.copy_wait()  # its pinned arrays may be refilled now
                    free.put(item)
                    n_batches += 1
                settle(True)
                t2 = time.perf_counter()
                eng.run()
                eng.sync()
                t3 = time.perf_counter()
                res = eng.fetch(dense=False)
                if rows is not None and not rows.wide.any():
                    res.counts, res.tn5, res.depth = rows.counts, rows.tn5, rows.depth
                elif rows is not None:
                    res = eng.fetch(dense=True)  # a drained window: the exact u32 arrays
                else:
                    res = eng.fetch_compact()
                t4 = time.perf_counter()
                self.last_stats = eng.kernel_times()
                _, last_streamed = eng.stream_info()
                tail = self._after_run(res, [(eng, 0, n_cells)])
            finally:
                free.put(None)
                eng.close()
            producer.join()
        finally:
            st.close()
            bam.close()
        te = time.perf_counter()
        # where the streamed engine leg goes: setup (pinned ring + rows target, context),
        # the pushes (behind the decode), the run's tail after the last batch, results
        dec_end = times.get("decode_end", t2)
        self.last_timing = {"stream_setup": t1 - t0, "stream_first_batch": times.get("first_batch", t1) - t0,
                            "stream_decode_end": dec_end - t0, "stream_push_end": t2 - t0,
                            "engine_tail": t3 - t2, "engine_fetch": t4 - t3,
                            "engine_close": te - t4 - sum(tail.values()), **tail,
                            "stream_batches": n_batches, "stream_batch_reads": times["cap_reads"],
                            "streamed_run": bool(last_streamed), "rows_target": rows is not None,
                            "h2d_bytes": int(h2d)}
        self.last_result = res
        return res

    def _run_stream_sharded(self, reader, n_cells: int, batch_reads: int | None, rows_target: bool) -> EngineResult:
        """The streamed path over several devices: one streaming
        context per device, each owning a contiguous whitelist range of cells and fed by
        a thread of its own. The host routes every decoded batch (mgp_route_batch, the
        reference's split of the barcodes over its pool, processors.py:112-144, as a
        split over devices): each kept read's columns and record go to its cell's
        device's pinned batch, in BAM order, the barcode rebased to the device's range;
        reads without a whitelisted barcode, or that readers.py:96 skips, go nowhere
        (they count only toward total_reads, which the decoder counts). So each link
        carries, and each device holds, only its own cells' reads. The ranges are
        read-balanced by the first batch's reads per cell (a cell's reads are spread
        over all of chrM, so the first batch is a fair sample of the whole set). The
        cells' first-seen order (readers.py:104-163) comes from the router: each cell's
        first routed read's index in the stream. Every device's rows go into its cell
        range of one result array, so nothing is concatenated; the tallies are summed
        on the host."""
        from queue import Empty

        from ..bam import RoutePart, host_threads, route_batch
        from ..exceptions import ProcessingError
        devs = list(self.devices)
        D = len(devs)
        t0 = time.perf_counter()
        bam, st, n_hint, free, full, producer, times = self._stream_producer(reader, n_cells, batch_reads,
                                                                            pinned=False)
        engines, rings, queues, workers, errors = {}, {}, {}, {}, []
        parts: list[tuple[int, int, int]] = []
        rows = None
        first_seen = np.full(max(1, n_cells), 0xFFFFFFFF, np.uint32)
        n_threads = host_threads()
        n_slots = max(2, int(os.environ.get("MGP_STREAM_SLOTS", STREAM_SLOTS)))
        link_bytes = {}
        try:
            first = full.get()
            if isinstance(first, BaseException):
                raise first
            if first is not None:
                times["first_batch"] = time.perf_counter()
                bc = first.soa().bc
                w = np.bincount(bc[(bc >= 0) & (bc < n_cells)], minlength=n_cells).astype(np.float64) + 1e-3
            else:
                w = np.ones(n_cells)
            bounds = partition_cells(w, D)
            parts = [(d, int(bounds[d]), int(bounds[d + 1])) for d in range(D) if bounds[d + 1] > bounds[d]]
            wsum = float(w.sum()) or 1.0
            share = {d: float(w[lo:hi].sum()) / wsum for d, lo, hi in parts}
            for d, lo, hi in parts:
                m = int(n_hint * share[d] * 1.1) + 65536  # the device's share of the reads, with headroom
                ec = self.config.engine_config(hi - lo, reserve_reads=m,
                                               reserve_payload=_payload_hint(m, hi - lo, times["cap_reads"] * share[d]))
                ec.stream = True
                engines[d] = Engine(ec, device=devs[d])
                rings[d], queues[d] = Queue(), Queue()
                link_bytes[d] = 0
            route_bounds = np.array([lo for _, lo, _ in parts] + ([parts[-1][2]] if parts else [0]), np.int32)
            # a device's batch: its share of a decoded batch with headroom (a batch that
            # does not fit is routed in halves)
            cap_r, cap_p = times["cap_reads"], times["cap_payload"]

            def part_caps(d):
                f = min(1.0, share[d] * 1.5 + 0.02)
                return int(cap_r * f) + 65536, int(cap_p * f) + (1 << 20)

            # the rows target (all cells, one pinned array) is pinned while the first batches go
            # in; each device thread sets its view of it when it is ready
            target = _RowsTarget(n_cells, self.config.mito_length, engines[parts[0][0]].windows()) \
                if rows_target and parts else None

            def work(d, lo, hi):
                # the device's pinned batches (pinned here, beside the other devices'), then
                # every routed batch pushed, its copy awaited, its arrays back to the ring
                eng = engines[d]
                view_set = target is None

                def set_view(wait: bool):
                    nonlocal view_set
                    if view_set or not (wait or target.ready()):
                        return
                    view_set = True
                    r = target.take()
                    if r is not None:
                        eng.set_rows16_target(_rows_slice(r, lo, hi))

                try:
                    cr, cp = part_caps(d)
                    for _ in range(n_slots):
                        rings[d].put(RoutePart(cr, cp, _pinned_alloc(RoutePart.nbytes(cr, cp))))
                    while True:
                        set_view(False)
                        pt = queues[d].get()
                        if pt is None:
                            break
                        try:
                            sub = pt.soa()
                            eng.push(sub)
                            link_bytes[d] += _link_bytes(sub)
                            eng.copy_wait()
                        finally:
                            rings[d].put(pt)
                    set_view(True)
                    eng.run()
                    eng.sync()
                except BaseException as e:  # noqa: BLE001 - re-raised by the router
                    errors.append(e)
                    while True:  # drain (handing back the batches it was dealt)
                        pt = queues[d].get()
                        if pt is None:
                            break
                        rings[d].put(pt)

            def take(d):
                while True:
                    if errors:
                        raise errors[0]
                    try:
                        return rings[d].get(timeout=0.2)
                    except Empty:
                        continue

            def route(soa, a, b, base):
                """Reads [a, b) of a decoded batch to their devices (halves when a device's
                batch cannot hold its share)."""
                sub = soa if (a, b) == (0, soa.n) else ReadSoA(None, soa.bc[a:b], soa.tlen[a:b], soa.flag[a:b],
                                                               soa.mapq[a:b], None, soa.rec_off[a:b], soa.payload)
                got = [take(d) for d, _, _ in parts]
                if not route_batch(sub, route_bounds, got, base + a, first_seen, n_threads):
                    for (d, _, _), pt in zip(parts, got):
                        rings[d].put(pt)
                    if b - a <= 1:
                        raise ProcessingError("a read's record does not fit a device batch")
                    mid = (a + b) // 2
                    route(soa, a, mid, base)
                    route(soa, mid, b, base)
                    return
                for (d, _, _), pt in zip(parts, got):
                    (queues[d] if pt.n else rings[d]).put(pt)

            for d, lo, hi in parts:
                workers[d] = threading.Thread(target=work, args=(d, lo, hi), name=f"mgp-dev{d}", daemon=True)
                workers[d].start()
            t1 = time.perf_counter()
            n_batches, base, t_route = 0, 0, 0.0
            try:
                item = first
                while item is not None:
                    if isinstance(item, BaseException):
                        raise item
                    if errors:
                        raise errors[0]
                    soa = item.soa()
                    if parts and soa.n:
                        tr = time.perf_counter()
                        route(soa, 0, soa.n, base)
                        t_route += time.perf_counter() - tr
                    base += soa.n
                    free.put(item)
                    n_batches += 1
                    item = full.get()
            finally:
                for d, _, _ in parts:
                    queues[d].put(None)
                for d, _, _ in parts:
                    workers[d].join()
            if errors:
                raise errors[0]
            rows = target.take() if target is not None else None
            t2 = time.perf_counter()
            L = self.config.mito_length
            # without a rows target: every device's exact 16-bit rows fetched into its cell
            # range of one host array (the u32 arrays only when a window was drained)
            src = rows
            if rows is None and parts:
                nw, W = engines[parts[0][0]].windows()
                src = Rows16(np.empty((n_cells, L, 8), np.uint16), np.empty((n_cells, L, 2), np.uint16),
                             np.empty((n_cells, L), np.uint16), np.zeros((n_cells, nw), np.uint8), W)
                for d, lo, hi in parts:
                    engines[d].fetch_rows16(lo=0, hi=hi - lo, out=_rows_slice(src, lo, hi))
            wide = src is None or bool(src.wide.any())
            res = EngineResult.alloc(n_cells, L, dense=wide)
            res.stats = merged_stats(st.records)  # (the decoder counts every read, routed or not)
            for d, lo, hi in parts:
                r = engines[d].fetch(dense=wide)
                copy_part(res, r, lo, hi, dense=wide)
                res.ref_tally += r.ref_tally
                res.stats["error_bits"] |= int(r.stats["error_bits"])
            # each cell's first read in the BAM (the router's index over the whole stream)
            res.first_read[:] = first_seen[:n_cells]
            if np.any((res.n_reads > 0) != (res.first_read != 0xFFFFFFFF)):
                raise ProcessingError("routed reads and per-cell read counts disagree")
            if not wide:
                res.counts, res.tn5, res.depth = src.counts, src.tn5, src.depth
            t3 = time.perf_counter()
            self.last_stats = engines[parts[0][0]].kernel_times() if parts else {}
            tail = self._after_run(res, [(engines[d], lo, hi) for d, lo, hi in parts])
        finally:
            free.put(None)
            for eng in engines.values():
                eng.close()
            producer.join()
            st.close()
            bam.close()
        te = time.perf_counter()
        self.last_timing = {"stream_setup": t1 - t0, "stream_first_batch": times.get("first_batch", t1) - t0,
                            "stream_decode_end": times.get("decode_end", t2) - t0, "stream_push_end": t2 - t0,
                            "engine_tail": 0.0, "engine_fetch": t3 - t2,
                            "engine_close": te - t3 - sum(tail.values()), **tail,
                            "stream_batches": n_batches, "stream_batch_reads": times["cap_reads"],
                            "stream_devices": len(parts), "rows_target": rows is not None, "route_s": t_route,
                            "h2d_bytes": int(sum(link_bytes.values())),
                            "cell_bounds": [lo for _, lo, _ in parts] + ([parts[-1][2]] if parts else [])}
        self.last_result = res
        return res

    def _run_sharded(self, soa_batches, n_cells: int) -> EngineResult:
        """Cells split into contiguous read-balanced ranges, one engine per device,
        run concurrently (ctypes releases the GIL); results concatenated along
        cells and tallies summed on the host."""
        from concurrent.futures import ThreadPoolExecutor

        from ..synth import concat_soa

        soa = soa_batches[0] if len(soa_batches) == 1 else concat_soa(soa_batches)
        b = partition_cells(reads_per_cell(soa, n_cells), len(self.devices))
        shards = [(int(lo), int(hi)) + shard_soa(soa, int(lo), int(hi)) for lo, hi in zip(b[:-1], b[1:])]

        # (the engines stay open only for the coverage and variant passes to read their rows)
        keep_open = self.variants_opt is not None or self.coverage_opt is not None
        engines: list = [None] * len(self.devices)

        def one(i):
            lo, hi, sub, idx = shards[i]
            ec = self.config.engine_config(hi - lo, reserve_reads=sub.n, reserve_payload=sub.payload.shape[0] + 256)
            eng = engines[i] = Engine(ec, device=self.devices[i])
            try:
                if sub.n:
                    eng.push(sub)
                eng.run()
                return eng.fetch_compact(), lo, hi, idx
            finally:
                if not keep_open:
                    eng.close()

        try:
            with ThreadPoolExecutor(len(self.devices)) as ex:
                parts = list(ex.map(one, range(len(self.devices))))
            res = merge_results(parts, n_cells, soa.n)
            live = [(engines[i], lo, hi) for i, (_, lo, hi, _) in enumerate(parts) if hi > lo]
            self.last_timing = self._after_run(res, live, writers=False)  # (this path has no device writers)
        finally:
            for eng in engines:
                if eng is not None:
                    eng.close()
        self.last_result = res
        return res

    def write_results(self, res: EngineResult, barcodes: list[str], incremental_writer=None) -> list[dict]:
        """Passing cells in first-seen order to the writer; returns the reference's
        slim result list ({"barcode", "n_reads"} per written cell, processors.py:75)."""
        order = res.cell_order()
        written = order[res.passed[order].astype(bool)]
        failed = int(order.size - written.size)
        if failed:
            logger.warning(f"{failed} cells failed")
        if incremental_writer is not None:
            incremental_writer.write_cells(res, written, barcodes=barcodes, tally=res.ref_tally)
        return [{"barcode": barcodes[int(c)], "n_reads": int(res.n_reads[c])} for c in written]

    def process_soa(self, soa_batches, barcodes: list[str], incremental_writer=None) -> list[dict]:
        res = self.run_soa(soa_batches, len(barcodes))
        return self.write_results(res, barcodes, incremental_writer)

    # reference dict API (processors.py:63-144) ------------------------------
    def process_cells_direct(self, reads_by_barcode, incremental_writer=None):
        res, barcodes = run_cells_from_reads(self.config, reads_by_barcode, self.device)
        self.last_result = res
        reads_by_barcode.clear()
        results, failed = [], 0
        for c, bc in enumerate(barcodes):
            if not res.passed[c]:
                failed += 1
                continue
            r = result_dict(res, c, bc, self.config.mito_length)
            if incremental_writer:
                incremental_writer.write_cell(r)
                results.append({"barcode": bc, "n_reads": r["n_reads"]})
            else:
                results.append(r)
        if failed > 0:
            logger.warning(f"{failed} cells failed")
        gc.collect()
        return results

    def process_cells_progressive(self, reads_by_barcode, incremental_writer=None):
        n_cells = len(reads_by_barcode)
        total = sum(len(r) for r in reads_by_barcode.values())
        avg = total / n_cells if n_cells > 0 else 0
        logger.info(f"Processing {n_cells} cells at an average of {avg:.0f} reads/cell")
        return self.process_cells_direct(reads_by_barcode, incremental_writer)

