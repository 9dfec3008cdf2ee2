"""Pipeline orchestration (mirror of src/core/pipeline.py:23-269).

Same entry points as the reference (``MtDNAPipeline(...).run()`` and
``run_pipeline(...)``). The flow is the reference's; the work inside is the
build's:

1. native BAM ingest of the chrM records in batches on a producer thread
   (:meth:`BAMReader.open_stream`), each batch pushed to the GPU as soon as it is
   decoded;
2. one streamed engine run: every position window goes through filters, dedup,
   pileup, strand filter and per-cell statistics as soon as its reads have all
   arrived, and its result rows come back while later batches are still decoded
   (:meth:`CellProcessor.run_stream`; ``stream=False`` or ``MGP_STREAM=0``: the whole
   set decoded first, then one run, :meth:`CellProcessor.run_soa`);
3. the writers format the passing cells, in first-seen order, from the
   engine's arrays;
4. ``qc/summary.txt`` and, for HDF5 output, the HTML report.

``self.timings`` records the wall time of each stage (seconds).
"""

from __future__ import annotations

import gc
import logging
import os
import threading
import time
from pathlib import Path
from types import SimpleNamespace
from typing import Any

import numpy as np

from .analysis.clonotypes import check_resolution
from .analysis.clustering import check_clones
from .analysis.neighbors import check_neighbors, check_prune
from .analysis.qc import QCCalculator
from .bam import BamFile
from .config import PipelineConfig
from .exceptions import InvalidInputError
from .file_io import IncrementalHDF5Writer, IncrementalTextWriter, write_run_summary
from .options import AnalysisOptions
from .processing.processors import CellProcessor
from .processing.readers import MITO_NAMES, BAMReader

logger = logging.getLogger(__name__)


def _release_in_background(box: list) -> None:
    """Drop the objects in `box` (holding their last references) on a daemon thread:
    their native free releases the GIL, so the unmapping overlaps the caller's next
    stage."""
    import threading

    threading.Thread(target=box.clear, name="mgp-free-inputs", daemon=True).start()


class _Background:
    """fn(*args) on a thread; result() joins and returns its value or raises its error."""

    def __init__(self, fn, *args):
        self._out = self._err = None
        self._t = threading.Thread(target=self._run, args=(fn, args), name="mgp-report-plots", daemon=True)
        self._t.start()

    def _run(self, fn, args):
        try:
            self._out = fn(*args)
        except BaseException as e:  # handed to result()
            self._err = e

    def result(self):
        self._t.join()
        if self._err is not None:
            raise self._err
        return self._out


def analysis_settings(call_variants=False, variant_min_cells=5, variant_min_strand_cor=0.65, variant_min_vmr=0.01,
                      variant_stabilize=False, variant_low_coverage=10, variant_min_coverage=1, coverage_stats=False,
                      cell_min_mean_coverage=0.0, cell_min_coverage_breadth=0.0, recompute_reference=False,
                      cluster=False, clones=None, neighbors=None, snn_prune=1.0 / 15.0, clonotypes=False,
                      clonotype_resolution=1.0, group_test=False, group_test_max_p=0.01, groups=None,
                      group_min_cells=2, group_min_af=0.01) -> dict:
    """The analysis keywords of run_pipeline / analyze_outputs checked (options.REQUIRES and each
    analysis's own range, InvalidInputError) and in the form enable_analyses and the writers take."""
    s: dict[str, Any] = {}
    # variant calling from the devices' rows (off unless asked for): variants/ in the output
    s["call_variants"] = bool(call_variants)
    s["variant_options"] = dict(min_cells=variant_min_cells, min_strand_cor=variant_min_strand_cor,
                                min_vmr=variant_min_vmr, stabilize_variance=bool(variant_stabilize),
                                low_coverage_threshold=variant_low_coverage, min_coverage=variant_min_coverage)
    # coverage QC from the devices' rows (off unless asked for): coverage/ in the output; the
    # cell filter and the recomputed reference also set the variants' population and reference
    s["coverage_stats"] = bool(coverage_stats)
    s["coverage_options"] = dict(min_mean_coverage=float(cell_min_mean_coverage),
                                 min_coverage_breadth=float(cell_min_coverage_breadth),
                                 recompute_reference=bool(recompute_reference))
    s["coverage_on"] = (s["coverage_stats"] or bool(recompute_reference) or cell_min_mean_coverage > 0
                        or cell_min_coverage_breadth > 0)
    # the analyses of the heteroplasmy matrix (analysis/stages.py), each off unless asked for
    s["cluster"], s["clonotypes"] = bool(cluster), bool(clonotypes)
    # (a float default cannot say "not given": snn_prune passes without neighbors, a resolution != 1.0 is given)
    AnalysisOptions(s["call_variants"], s["cluster"], clones, neighbors, None, s["clonotypes"],
                    None if clonotype_resolution == 1.0 else clonotype_resolution).check(InvalidInputError, True)
    s["clones"] = check_clones(clones)
    s["neighbors"] = None if neighbors is None else check_neighbors(neighbors)
    s["snn_prune"] = check_prune(snn_prune)
    s["clonotype_resolution"] = check_resolution(clonotype_resolution)
    # pseudobulk counts and marker variants per cell group (off unless asked for): groups/ in the output;
    # `groups` is a groups file or a {barcode: group} mapping, resolved over the run's cells before the run
    s["groups"] = groups
    if groups is not None:
        from .analysis.groups import check_group_min_af, check_group_min_cells

        group_min_cells, group_min_af = check_group_min_cells(group_min_cells), check_group_min_af(group_min_af)
    s["group_min_cells"], s["group_min_af"] = group_min_cells, group_min_af
    # the rank-sum test of each tested variant, every group against the rest (off unless asked for):
    # groups/group_tests.tsv
    s["group_test"] = bool(group_test)
    if s["group_test"]:
        from .analysis.group_tests import check_group_test_max_p

        if groups is None:
            raise InvalidInputError("group_test requires groups")
        group_test_max_p = check_group_test_max_p(group_test_max_p)
    s["group_test_max_p"] = group_test_max_p
    return s


def pca_settings(call_variants=False, pca=None, pca_scale=False) -> dict:
    """The PCA keywords of run_pipeline / analyze_outputs checked (InvalidInputError), beside analysis_settings
    (whose own keywords end with the groups'): the principal components of the heteroplasmy matrix, off unless
    asked for; variants/cell_pca.tsv, variant_loadings.tsv and pca_variance.tsv in the output."""
    s: dict[str, Any] = {"pca": None, "pca_scale": bool(pca_scale)}
    if pca is not None:
        from .analysis.pca import check_pca

        if not call_variants:
            raise InvalidInputError("pca requires call_variants")
        s["pca"] = check_pca(pca)
    elif s["pca_scale"]:
        raise InvalidInputError("pca_scale requires pca")
    return s


def enable_analyses(processor, s, names=None) -> None:
    """Turn on, on a CellProcessor, the analyses that `s` (an object with analysis_settings' names) asks for.
    names: the barcode of each cell of the run (of each column of a loaded table), for the groups."""
    if s.call_variants:
        processor.enable_variants(**s.variant_options)
    if s.coverage_on:
        processor.enable_coverage(**s.coverage_options)
    if s.cluster:
        processor.enable_clustering(s.clones)
    if s.neighbors is not None:
        processor.enable_neighbors(s.neighbors, s.snn_prune)
    if s.clonotypes:
        processor.enable_clonotypes(s.clonotype_resolution)
    if getattr(s, "groups", None) is not None:
        from .analysis.groups import resolve_groups

        processor.enable_groups(*resolve_groups(s.groups, list(names or [])), s.group_min_cells, s.group_min_af,
                                getattr(s, "group_test", False), getattr(s, "group_test_max_p", 0.01))
    if getattr(s, "pca", None) is not None:
        processor.enable_pca(s.pca, getattr(s, "pca_scale", False))


def write_table_outputs(processor, res, names: list[str], output_dir, output_format: str, coverage_on: bool,
                        coverage_stats: bool, call_variants: bool) -> list[str]:
    """coverage/ and variants/ of a result whose population's cells are named `names` (a run's
    whitelist, a loaded table's columns or subset). Returns the barcodes of the heteroplasmy
    matrix's columns (the coverage filter's kept cells, if it ran)."""
    cov = res.coverage if coverage_on else None
    if cov is not None and (coverage_stats or cov.ref_alleles is not None):
        from .analysis.coverage import write_coverage_outputs

        write_coverage_outputs(cov, names, output_dir, processor.run_reference(res), tables=coverage_stats)
        logger.info("%d of %d cells kept by the coverage filter", int(cov.kept.sum()), int(cov.kept.size))
    af_names = names if res.variant_cells is None else [names[int(i)] for i in res.variant_cells]
    if call_variants and res.variants is not None:
        from .analysis.variants import write_variant_outputs

        write_variant_outputs(res.variants, res.allele_freq, af_names, output_dir, output_format)
        logger.info("%d variants called", len(res.variants))
    return af_names


def write_group_outputs(res, output_dir) -> None:
    """groups/ of a result whose run had the groups on (analysis/groups.py)."""
    if res.groups is None:
        return
    from .analysis.groups import write_group_result

    write_group_result(res.groups, output_dir)
    logger.info("%d groups, %d marker variants", len(res.groups.group_names), len(res.groups.markers))
    tests = res.groups.tests
    if tests is not None:
        logger.info("Rank-sum tests: %d variants tested over %d groups, %d lines with p <= %s", tests.n_tested,
                    tests.n_groups, len(tests), tests.max_p)


def write_stage_outputs(processor, res, af_names: list[str], output_dir) -> None:
    """The analyses of the heteroplasmy matrix that are on (analysis/stages.py), each made and
    written to variants/ in the declared order."""
    if not (processor.stage_opt and res.variants is not None):
        return
    from .analysis.stages import STAGES

    for stage in STAGES.values():
        result = processor.stage_result(stage.key, res)
        if result is not None:
            stage.write(result, af_names, res.variants, output_dir)
            if line := stage.log(result):
                logger.info(*line)


def write_pca_outputs(processor, res, af_names: list[str], output_dir) -> None:
    """The principal components of the heteroplasmy matrix, when on (analysis/pca.py): made on the first
    device and written to variants/."""
    if processor.pca_opt is None or res.variants is None:
        return
    from .analysis.pca import write_pca_outputs as write_files

    result = processor.pca_result(res)
    write_files(result, af_names, res.variants, output_dir)
    if result.scores is not None:
        logger.info("PCA: %d cells x %d variants, %d components, %d Jacobi sweeps", result.n,
                    result.loadings.shape[1], result.n_comp, result.sweeps)


class MtDNAPipeline:
    """Single-pass mtDNA genotyping pipeline (pipeline.py:23-74)."""

    def __init__(
        self,
        bam_path: str,
        barcodes: list[str],
        output_dir: Path,
        config: PipelineConfig | None = None,
        output_format: str = "standard",
        barcode_metadata=None,
        sample_name: str = "mgatk2",
        report_title: str | None = None,
        report_subtitle: str | None = None,
        working_directory: str | None = None,
        device: int = 0,
        devices: list[int] | None = None,
        stream: bool | None = None,
        call_variants: bool = False,
        variant_min_cells: int = 5,
        variant_min_strand_cor: float = 0.65,
        variant_min_vmr: float = 0.01,
        variant_stabilize: bool = False,
        variant_low_coverage: int = 10,
        variant_min_coverage: int = 1,
        coverage_stats: bool = False,
        cell_min_mean_coverage: float = 0.0,
        cell_min_coverage_breadth: float = 0.0,
        recompute_reference: bool = False,
        cluster: bool = False,
        clones: int | None = None,
        neighbors: int | None = None,
        snn_prune: float = 1.0 / 15.0,
        clonotypes: bool = False,
        clonotype_resolution: float = 1.0,
        groups=None,
        group_min_cells: int = 2,
        group_min_af: float = 0.01,
        group_test: bool = False,
        group_test_max_p: float = 0.01,
        pca: int | None = None,
        pca_scale: bool = False,
    ):
        self.bam_path = Path(bam_path)
        # streamed ingest (default; MGP_STREAM=0 decodes the whole chrM set first)
        self.stream = (os.environ.get("MGP_STREAM", "1") != "0") if stream is None else bool(stream)
        self.barcodes = set(barcodes)
        self.barcode_list = list(barcodes)
        self.output_dir = Path(output_dir)
        self.config = config or PipelineConfig()
        self.output_format = output_format.lower()
        self.barcode_metadata = barcode_metadata
        self.sample_name = sample_name
        self.report_title = report_title or sample_name
        self.report_subtitle = report_subtitle or "mgatk2 output analysis"
        self.working_directory = working_directory
        self.device = device
        self.devices = list(devices) if devices else [device]
        vars(self).update(analysis_settings(
            call_variants, variant_min_cells, variant_min_strand_cor, variant_min_vmr, variant_stabilize,
            variant_low_coverage, variant_min_coverage, coverage_stats, cell_min_mean_coverage,
            cell_min_coverage_breadth, recompute_reference, cluster, clones, neighbors, snn_prune, clonotypes,
            clonotype_resolution, group_test, group_test_max_p, groups, group_min_cells, group_min_af))
        vars(self).update(pca_settings(call_variants, pca, pca_scale))
        self.timings: dict[str, float] = {}
        self.engine_result = None
        self.read_stats: dict = {}

        if not self.bam_path.exists():
            raise InvalidInputError(f"BAM file not found: {bam_path}")
        with BamFile(self.bam_path) as bam:
            refs = list(bam.references)
        if self.config.mito_chr not in refs:
            for alt in MITO_NAMES:
                if alt in refs:
                    logger.warning(f"Using '{alt}' instead of '{self.config.mito_chr}'")
                    self.config.mito_chr = alt
                    break
            else:
                raise InvalidInputError(
                    f"Mitochondrial chromosome '{self.config.mito_chr}' not found. Available: {', '.join(refs[:10])}"
                )
        self.output_dir.mkdir(parents=True, exist_ok=True)

    def _render_plots(self, arrays):
        from .analysis.report import render_plots

        return render_plots(arrays, scatac=self.barcode_metadata is not None)

    def run(self) -> dict[str, Any]:
        t0 = time.time()
        if self.output_format == "hdf5":
            # the report's pyplot import and package listing, under the decode
            try:
                from .analysis.report import prewarm

                prewarm()
            except ImportError:  # pragma: no cover
                pass
        logger.info("Collecting reads from BAM by barcode...")
        reader = BAMReader(str(self.bam_path), self.config, self.barcode_list)
        processor = CellProcessor(self.config, self.output_dir, device=self.device, devices=self.devices)
        txt_writer = None
        if self.output_format != "hdf5":
            # the count files are written from the devices' rows at the end of the run
            # (mgp_txt_gz): the writer's files exist before it
            txt_writer = IncrementalTextWriter(self.output_dir, self.config, self.barcode_list)
            processor.enable_device_txt(txt_writer.prefix, self.barcode_list)
        else:
            # the HDF5 chunks are deflated on the device at the end of the run (mgp_h5_tiles)
            processor.enable_device_h5(self.barcode_list)
        enable_analyses(processor, self, self.barcode_list)
        if self.stream:
            # one pass: batches decoded on a producer thread, each pushed to the device as
            # it is ready, the windows piled as their reads arrive (readers.py:84-93)
            res = processor.run_stream(reader, len(self.barcode_list))
            stats = {"total_reads": int(res.stats["total_reads"])}
            t1 = ta = t0 + processor.last_timing.get("stream_decode_end", time.time() - t0)
            tb = t2 = time.time()
        else:
            soa, stats = reader.read_soa()
            t1 = time.time()
            ta = time.time()
            res = processor.run_soa(soa, len(self.barcode_list))
            tb = time.time()
            # the decoded batch (GBs of malloc'd columns and records) is unmapped on a
            # background thread while the writers run: its free took 0.36 s at C3
            box = [soa]
            del soa
            _release_in_background(box)
            t2 = time.time()
        self.engine_result = res
        self.read_stats = {**res.stats, **stats}
        st = self.read_stats
        if not self.config.dedup.skip and st["total_reads"]:
            removed = st["duplicate_reads_with_length"] if self.config.dedup.use_fragment_length \
                else st["duplicate_reads_position_only"]
            logger.info("%d duplicate reads removed (%.1f%%)", removed, removed / st["total_reads"] * 100)
        n_cells_input = int((res.n_reads > 0).sum())  # len(reads_by_barcode)
        if n_cells_input == 0:
            logger.error("No reads found for any barcodes!")
            return {}
        logger.info(f"Kept {st['filtered_reads']:,} reads from {n_cells_input:,} barcodes")

        if self.output_format == "hdf5":
            writer = IncrementalHDF5Writer(self.output_dir, self.config, self.barcode_list,
                                           barcode_metadata=self.barcode_metadata)
        else:
            writer = txt_writer
        cell_results = processor.write_results(res, self.barcode_list, writer)
        if not cell_results:
            logger.error("No cells passed quality filters")
            return {}

        logger.info("Cleaning up...")
        qc_dir = self.output_dir / "qc"
        plots = None
        if self.output_format == "hdf5" and hasattr(writer, "prepare_report_arrays"):
            # the report's figures are rendered from memory while finalize deflates and
            # writes the planes (native code, GIL released)
            plots = _Background(self._render_plots, writer.prepare_report_arrays())
        writer.finalize(qc_dir)
        meta = QCCalculator(self.config).collect_run_metadata(
            str(self.bam_path), str(self.output_dir), n_cells_input, len(cell_results))
        write_run_summary(meta, qc_dir / "summary.txt")
        af_names = write_table_outputs(processor, res, self.barcode_list, self.output_dir, self.output_format,
                                       self.coverage_on, self.coverage_stats, self.call_variants)
        write_group_outputs(res, self.output_dir)
        t3 = time.time()
        gc.collect()

        if self.output_format == "hdf5":
            logger.info("Generating HTML QC report...")
            try:
                from .analysis.report import generate_html_report, generate_scrna_html_report

                gen = generate_html_report if self.barcode_metadata is not None else generate_scrna_html_report
                gen(self.output_dir, self.sample_name, title=self.report_title, subtitle=self.report_subtitle,
                    working_directory=self.working_directory, input_dir=str(self.bam_path.parent),
                    arrays=getattr(writer, "report_arrays", None), plots=plots.result() if plots else None)
            except ImportError:
                logger.warning("matplotlib not installed, skipping HTML report generation")
            except Exception as e:
                logger.warning("Failed to generate HTML report: %s", e)
        t4 = time.time()
        # last, so that a population above an analysis's bound raises with every other output
        # written; the run's engine contexts closed long ago
        write_stage_outputs(processor, res, af_names, self.output_dir)
        write_pca_outputs(processor, res, af_names, self.output_dir)
        t5 = time.time()
        # streamed: bam_ingest ends with the last decoded batch and `engine` is only what the
        # device still did after it (the rest ran under the decode)
        self.timings = {"bam_ingest": t1 - t0, "engine": t2 - t1, "write": t3 - t2, "report": t4 - t3,
                        "total": t5 - t0, "engine_setup": ta - t1, "engine_run_soa": tb - ta,
                        "engine_free_inputs": t2 - tb, "streamed": bool(self.stream),
                        **processor.last_timing}
        logger.info("Pipeline complete")
        logger.info("Elapsed time: %.1fs (ingest %.1fs, engine %.1fs, write %.1fs)", t5 - t0, t1 - t0, t2 - t1,
                    t3 - t2)
        return {
            "cells_processed": n_cells_input,
            "cells_passed_qc": len(cell_results),
            "mean_reads": sum(r["n_reads"] for r in cell_results) / len(cell_results),
        }


def run_pipeline(
    bam_path: str,
    barcode_file: str | None = None,
    output_dir: str = "",
    sample_name: str = "mgatk",
    min_baseq: int = 20,
    min_mapq: int = 30,
    min_reads_per_cell: int = 1,
    max_strand_bias: float = 1.0,
    min_distance_from_end: int = 5,
    skip_deduplication: bool = False,
    use_fragment_length_dedup: bool = True,
    write_cell_bams: bool = False,
    barcode_tag: str = "CB",
    min_barcode_reads: int = 1,
    mito_chr: str = "chrM",
    n_cores: int = 16,
    worker_batch_size: int | None = None,
    io_batch_size: int | None = None,
    max_memory_gb: float = 128.0,
    output_format: str = "standard",
    sequential: bool = False,
    report_title: str | None = None,
    report_subtitle: str | None = None,
    working_directory: str | None = None,
    device: int = 0,
    devices: list[int] | None = None,
    call_variants: bool = False,
    variant_min_cells: int = 5,
    variant_min_strand_cor: float = 0.65,
    variant_min_vmr: float = 0.01,
    variant_stabilize: bool = False,
    variant_low_coverage: int = 10,
    variant_min_coverage: int = 1,
    coverage_stats: bool = False,
    cell_min_mean_coverage: float = 0.0,
    cell_min_coverage_breadth: float = 0.0,
    recompute_reference: bool = False,
    cluster: bool = False,
    clones: int | None = None,
    neighbors: int | None = None,
    snn_prune: float = 1.0 / 15.0,
    clonotypes: bool = False,
    clonotype_resolution: float = 1.0,
    device_inflate: bool = False,
    groups=None,
    group_min_cells: int = 2,
    group_min_af: float = 0.01,
    group_test: bool = False,
    group_test_max_p: float = 0.01,
    pca: int | None = None,
    pca_scale: bool = False,
) -> dict[str, Any]:
    """pipeline.py:183-269. ``min_distance_from_end`` is accepted and, as in the
    reference, not passed on (the engine uses 5). ``call_variants``
    (not in the reference's pipeline: its R step on counts.h5) writes variants/ with
    mgatk's customary thresholds as defaults. ``coverage_stats`` writes coverage/ (the front
    half of that R workflow: cell, position, strand and transposition tables);
    ``cell_min_mean_coverage`` / ``cell_min_coverage_breadth`` filter the cells those position
    tables and the variants are made of, ``recompute_reference`` gives the variants the kept
    cells' own reference alleles (and writes coverage/reference_alleles.tsv). ``cluster`` (needs
    ``call_variants``) clusters the cells and the variants of the heteroplasmy matrix on the
    device (the vignette's pheatmap step: Euclidean distances, complete linkage) and writes the
    trees and the heatmap orders to variants/; ``clones`` = K (needs ``cluster``) also writes the
    cell tree cut into K clones. ``neighbors`` = K (needs ``call_variants``; Seurat's k.param, 2..GRAPH_MAX_K + 1)
    builds the cells' kNN graph over the variants and its SNN graph (Jaccard weights, ``snn_prune``
    as Seurat's prune.SNN) on the device and writes variants/cell_knn.tsv, cell_snn.mtx and
    cell_snn_barcodes.tsv. ``clonotypes`` (needs ``neighbors``) finds the Louvain communities of that
    SNN graph on the device, the same on every run (``clonotype_resolution`` as Seurat's resolution),
    and writes variants/cell_clonotypes.tsv and clonotypes.tsv. ``device_inflate`` inflates the BAM's
    BGZF blocks on the device (the first of ``devices``) instead of the host pool; the outputs are the
    same bytes. ``groups`` (a groups file: barcode, group; or a {barcode: group} mapping) writes groups/: the
    pseudobulk counts of every group at all positions and bases and its marker variants, those with at least
    ``group_min_cells`` confident cells and a pseudobulk heteroplasmy of at least ``group_min_af`` that
    exceeds the rest of the population's (this project's thresholds; mgatk defines none). ``group_test`` (needs
    ``groups``) adds groups/group_tests.tsv: the Wilcoxon rank-sum test of each marker or called variant's
    heteroplasmy over the cells, every group against the rest (Seurat's FindAllMarkers; the ranks on the device),
    the pairs higher in the group with a p-value up to ``group_test_max_p``. ``pca`` = N (needs ``call_variants``;
    1..50, clipped to what the matrix has) writes the first N principal components of the heteroplasmy matrix,
    R's prcomp(t(af)) on the device with a fixed operation order: variants/cell_pca.tsv, variant_loadings.tsv and
    pca_variance.tsv; ``pca_scale`` (needs ``pca``) scales each variant to unit variance first."""
    barcode_metadata = None
    if barcode_file is None:
        from .file_io.barcode_extraction import extract_barcodes_from_bam

        logger.info("No barcode file provided - extracting barcodes from BAM")
        barcodes = extract_barcodes_from_bam(bam_path, barcode_tag=barcode_tag, mito_chr=mito_chr,
                                             min_reads=min_barcode_reads)
        if not barcodes:
            raise InvalidInputError(
                f"No barcodes found in BAM file with tag '{barcode_tag}' and minimum {min_barcode_reads} reads")
    elif barcode_file.endswith(".csv"):
        from .utils import load_singlecell_csv

        barcodes, barcode_metadata = load_singlecell_csv(barcode_file)
    else:
        from .utils import load_barcode_list

        barcodes = load_barcode_list(barcode_file)

    if worker_batch_size is None:
        worker_batch_size = n_cores
    if io_batch_size is None:
        io_batch_size = max(50, min(int(0.1 * len(barcodes)), 1000))
    config = PipelineConfig(
        min_baseq=min_baseq, min_mapq=min_mapq, max_strand_bias=max_strand_bias,
        skip_deduplication=skip_deduplication, use_fragment_length_dedup=use_fragment_length_dedup,
        n_cores=n_cores, worker_batch_size=worker_batch_size, io_batch_size=io_batch_size,
        max_memory_gb=max_memory_gb, sequential=sequential, min_reads_per_cell=min_reads_per_cell,
        barcode_tag=barcode_tag, mito_chr=mito_chr, write_cell_bams=write_cell_bams,
        device_inflate=device_inflate, inflate_device=devices[0] if devices else device,
    )
    pipeline = MtDNAPipeline(
        bam_path=bam_path, barcodes=barcodes, output_dir=Path(output_dir), config=config,
        output_format=output_format, barcode_metadata=barcode_metadata, sample_name=sample_name,
        report_title=report_title, report_subtitle=report_subtitle, working_directory=working_directory,
        device=device, devices=devices, call_variants=call_variants, variant_min_cells=variant_min_cells,
        variant_min_strand_cor=variant_min_strand_cor, variant_min_vmr=variant_min_vmr,
        variant_stabilize=variant_stabilize, variant_low_coverage=variant_low_coverage,
        variant_min_coverage=variant_min_coverage, coverage_stats=coverage_stats,
        cell_min_mean_coverage=cell_min_mean_coverage, cell_min_coverage_breadth=cell_min_coverage_breadth,
        recompute_reference=recompute_reference, cluster=cluster, clones=clones,
        neighbors=neighbors, snn_prune=snn_prune, clonotypes=clonotypes, clonotype_resolution=clonotype_resolution,
        groups=groups, group_min_cells=group_min_cells, group_min_af=group_min_af, group_test=group_test,
        group_test_max_p=group_test_max_p, pca=pca, pca_scale=pca_scale,
    )
    return pipeline.run()


def _subset_columns(file_barcodes: list[str], barcodes) -> tuple[Any, list[str]]:
    """subset_mgatk_barcodes (R/mgatk2_functions.R:98-136): the file's columns whose barcode is in
    `barcodes` (a barcode file or a list), in file order, and their names."""
    if isinstance(barcodes, (str, os.PathLike)):
        from .utils import load_barcode_list

        barcodes = load_barcode_list(str(barcodes))
    want = set(barcodes)
    keep = [i for i, b in enumerate(file_barcodes) if b in want]
    missing = sorted(want - set(file_barcodes))
    if missing:
        logger.warning("%d of %d barcodes are not in the count files: %s%s", len(missing), len(want),
                       ", ".join(missing[:5]), ", ..." if len(missing) > 5 else "")
    if not keep:
        raise InvalidInputError("No matching barcodes found")
    logger.info("Found %d matching barcodes (%.1f%%)", len(keep), 100.0 * len(keep) / len(file_barcodes))
    return np.array(keep, np.int64), [file_barcodes[i] for i in keep]


def analyze_outputs(input_dir, output_dir=None, barcodes=None, device: int = 0, host_inflate: bool = False,
                    pca=None, pca_scale=False, **analysis) -> dict[str, Any]:
    """The analyses of a run (``analysis``: run_pipeline's keywords from call_variants to
    clonotype_resolution, with its defaults and rules) from the count files a run left in
    ``input_dir`` (output/counts.h5 and output/metadata.h5, ours or the reference tool's): the
    R workflow's read_mgatk_hdf5, optionally subset_mgatk_barcodes (``barcodes``: a file or a
    list; the population is those columns in file order), then the rest, on the device. Every
    column of the files is a cell, the reference alleles are the files', and the values are
    the stored min(count, 65535): the results equal R's on the files exactly, and a run's own
    wherever no count saturates. ``groups`` (with ``group_min_cells``, ``group_min_af``, ``group_test``,
    ``group_test_max_p``) labels the files' columns; ``pca`` / ``pca_scale`` as run_pipeline's.
    Writes coverage/, variants/ and groups/ into ``output_dir`` (default:
    ``input_dir``); the count files are never rewritten. ``host_inflate``: libhdf5 inflates
    the chunks instead of the device (the same results)."""
    from .engine import EngineResult
    from .table import load_counts

    s = SimpleNamespace(**analysis_settings(**analysis),
                        **pca_settings(analysis.get("call_variants", False), pca, pca_scale))
    t0 = time.time()
    out_dir = Path(output_dir) if output_dir else Path(input_dir)
    with load_counts(input_dir, device=device, host_inflate=host_inflate) as loaded:
        t1 = time.time()
        n, L = loaded.n_cells, len(loaded.ref_alleles)
        names, pop = loaded.barcodes, None
        if barcodes is not None:
            pop, names = _subset_columns(loaded.barcodes, barcodes)
        processor = CellProcessor(PipelineConfig(), out_dir, device=device)
        processor.reference, processor.population = loaded.ref_alleles, pop
        enable_analyses(processor, s, loaded.barcodes)
        # the minimal result of a run: every column of the files is a cell that passed
        res = EngineResult.alloc(n, L, dense=False)
        res.passed[:] = 1
        tail = processor._after_run(res, [(loaded.engine, 0, n)] if n else [], writers=False)
    t2 = time.time()
    out_dir.mkdir(parents=True, exist_ok=True)
    af_names = write_table_outputs(processor, res, names, out_dir, "hdf5", s.coverage_on, s.coverage_stats,
                                   s.call_variants)
    write_group_outputs(res, out_dir)
    write_stage_outputs(processor, res, af_names, out_dir)
    write_pca_outputs(processor, res, af_names, out_dir)
    t3 = time.time()
    timings = {"load": t1 - t0, **{"load_" + k: v for k, v in loaded.seconds.items()}, "analyses": t2 - t1,
               "write": t3 - t2, "total": t3 - t0, **tail, **processor.last_timing}
    logger.info("Analyses complete: %d cells of %d columns, load %.2fs, analyses %.2fs, write %.2fs", len(names), n,
                t1 - t0, t2 - t1, t3 - t2)
    return {"cells": len(names), "columns": n, "n_saturated": loaded.n_saturated,
            "variants": None if res.variants is None else len(res.variants), "timings": timings, "result": res}
