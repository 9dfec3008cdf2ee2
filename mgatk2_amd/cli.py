"""Command line (mirror of src/cli: base.py, options.py, utils.py, commands/{run,tenx,call}.py).

Same commands, option names, short flags and defaults as the reference, so a
reference command line runs unchanged (``python -m mgatk2_amd run -i ...``).
Added: ``--device`` (HIP device ordinal for the engine), ``--variants`` with its
``--variant-*`` thresholds (variant calling from the device's rows, variants/ in the output),
and ``--coverage-stats`` / ``--cell-min-mean-coverage`` / ``--cell-min-coverage-breadth`` /
``--recompute-reference`` (coverage QC and the cell filter from the device's rows, coverage/),
and ``--cluster`` / ``--clones K`` (the heteroplasmy matrix's cells and variants clustered on
the device, the trees and heatmap orders in variants/), and ``--neighbors K`` / ``--snn-prune P``
(the cells' kNN and SNN graphs by heteroplasmy on the device, in variants/), and ``--clonotypes`` /
``--clonotype-resolution R`` (the Louvain communities of that SNN graph on the device: each cell's
clonotype, in variants/), and ``--groups FILE`` / ``--group-min-cells N`` / ``--group-min-af F`` (the
pseudobulk counts and marker variants of every cell group of FILE from the device's rows, groups/), and
``--group-test`` / ``--group-test-max-p P`` (the rank-sum test of each variant, every group against the rest
of the cells, ranked on the device: groups/group_tests.tsv), and ``--pca N`` / ``--pca-scale`` (the first N
principal components of the heteroplasmy matrix on the device, in variants/).
Not carried over: ``hardmask-fasta`` (FASTA masking utility, outside the hot path).
"""

from __future__ import annotations

import csv
import logging
import multiprocessing
import os
import sys
from datetime import datetime
from pathlib import Path

import click

from . import __version__
from .exceptions import InvalidInputError, ProcessingError

logger = logging.getLogger(__name__)

DEDUP_CHOICES = ["alignment_and_fragment_length", "alignment_start", "none"]


# ---------------------------------------------------------------------------
# options (options.py:6-306)
# ---------------------------------------------------------------------------
def _analysis_option_list() -> list:
    """--variants and its thresholds, the coverage options and the analyses of the heteroplasmy
    matrix: what `run`, `tenx`, `call` and `analyze` share."""
    return [
        click.option("--variants", "call_variants", is_flag=True,
                     help="Call variants on the device: variants/variant_stats.tsv and the heteroplasmy matrix"),
        click.option("--variant-min-cells", default=5, type=int, show_default=True,
                     help="Minimum cells with >= 2 reads of the allele on each strand"),
        click.option("--variant-min-strand-cor", default=0.65, type=float, show_default=True,
                     help="Minimum strand correlation"),
        click.option("--variant-min-vmr", default=0.01, type=float, show_default=True,
                     help="Variance-to-mean ratio a variant must exceed"),
        click.option("--variant-stabilize", is_flag=True,
                     help="Variance stabilisation: low-coverage cells take the bulk allele frequency"),
        click.option("--variant-low-coverage", default=10, type=int, show_default=True,
                     help="Depth below which a cell is low-coverage (with --variant-stabilize)"),
        click.option("--variant-min-coverage", default=1, type=int, show_default=True,
                     help="Depth below which the heteroplasmy matrix is 0"),
        click.option("--coverage-stats", is_flag=True,
                     help="Coverage QC on the device: coverage/ with the cell, position, strand and Tn5 tables"),
        click.option("--cell-min-mean-coverage", default=0.0, type=float, show_default=True,
                     help="Keep cells with at least this mean depth (for the position tables and --variants)"),
        click.option("--cell-min-coverage-breadth", default=0.0, type=float, show_default=True,
                     help="Keep cells with at least this fraction of positions covered"),
        click.option("--recompute-reference", is_flag=True,
                     help="Reference alleles from the kept cells (coverage/reference_alleles.tsv; used by --variants)"),
        click.option("--cluster", is_flag=True,
                     help="Cluster cells and variants by heteroplasmy on the device (Euclidean, complete linkage): "
                          "variants/{cell,variant}_{hclust,order}.tsv; needs --variants"),
        click.option("--clones", default=None, type=click.IntRange(min=1), metavar="K",
                     help="Cut the cell tree into K clones (variants/cell_clones.tsv); needs --cluster"),
        click.option("--neighbors", default=None, type=click.IntRange(min=2, max=65), metavar="K",  # (GRAPH_MAX_K + 1)
                     help="kNN and SNN graphs of the cells by heteroplasmy on the device, K as Seurat's k.param "
                          "(the cell and its K - 1 nearest others): variants/cell_knn.tsv, cell_snn.mtx, "
                          "cell_snn_barcodes.tsv; needs --variants"),
        click.option("--snn-prune", default=None, type=click.FloatRange(min=0.0, max=1.0), metavar="P",
                     help="Drop SNN edges of Jaccard weight below P (Seurat's prune.SNN)  [default: 1/15]; "
                          "needs --neighbors"),
        click.option("--clonotypes", is_flag=True,
                     help="Clonotypes of the cells: Louvain communities of the SNN graph on the device, the same "
                          "on every run (variants/cell_clonotypes.tsv, clonotypes.tsv); needs --neighbors"),
        click.option("--clonotype-resolution", default=None, type=float, metavar="R",
                     help="Resolution of the communities, as Seurat's: above 1 more and smaller clonotypes  "
                          "[default: 1.0]; needs --clonotypes"),
    ]


def _group_option_list() -> list:
    """--groups and its thresholds, on `run`, `tenx`, `call` and `analyze`: declared before the shared block."""
    return [
        click.option("--groups", "groups", default=None, type=click.Path(exists=True, dir_okay=False), metavar="FILE",
                     help="Pseudobulk counts and marker variants per cell group on the device (groups/); FILE: "
                          "barcode<TAB>group lines, e.g. a run's variants/cell_clonotypes.tsv or cell_clones.tsv"),
        click.option("--group-min-cells", default=None, type=click.IntRange(min=0), metavar="N",
                     help="Cells of the group with >= 2 reads of the allele on each strand a marker variant needs  "
                          "[default: 2]; needs --groups"),
        click.option("--group-min-af", default=None, type=click.FloatRange(min=0.0, max=1.0), metavar="F",
                     help="Pseudobulk heteroplasmy in the group a marker variant needs  [default: 0.01]; "
                          "needs --groups"),
        click.option("--group-test", "group_test", is_flag=True,
                     help="Wilcoxon rank-sum test of each marker or called variant's heteroplasmy, every group "
                          "against the rest of the cells, ranked on the device (groups/group_tests.tsv, as Seurat's "
                          "FindAllMarkers); needs --groups"),
        click.option("--group-test-max-p", default=None, type=click.FloatRange(min=0.0, max=1.0), metavar="P",
                     help="Largest p-value of a written line (Seurat's return.thresh)  [default: 0.01]; needs "
                          "--group-test"),
    ]


def _pca_option_list() -> list:
    """--pca and --pca-scale, on `run`, `tenx`, `call` and `analyze`: declared beside the group options."""
    return [
        click.option("--pca", "pca", default=None, type=click.IntRange(min=1, max=50), metavar="N",
                     help="The first N principal components of the heteroplasmy matrix on the device, as R's "
                          "prcomp (variants/cell_pca.tsv, variant_loadings.tsv, pca_variance.tsv); needs --variants"),
        click.option("--pca-scale", "pca_scale", is_flag=True,
                     help="Scale each variant to unit variance before the components (prcomp's scale.); needs --pca"),
    ]


def _analysis_options(f):
    """The group and PCA options and the analysis options alone (`analyze`: there is no BAM)."""
    for o in reversed(_group_option_list() + _pca_option_list() + _analysis_option_list()):
        f = o(f)
    return f


def _variant_options(f):
    """The group options, the analysis options (after every reference option) and --device-inflate."""
    opts = _group_option_list() + _pca_option_list() + _analysis_option_list() + [
        click.option("--device-inflate", "device_inflate", is_flag=True,
                     help="Inflate the BAM's BGZF blocks on the device (the first of --devices); CRC32 stays on "
                          "the host. Off by default"),
    ]
    for o in reversed(opts):
        f = o(f)
    return f


def _variant_args(call_variants, variant_min_cells, variant_min_strand_cor, variant_min_vmr, variant_stabilize,
                  variant_low_coverage, variant_min_coverage, coverage_stats=False, cell_min_mean_coverage=0.0,
                  cell_min_coverage_breadth=0.0, recompute_reference=False, cluster=False, clones=None, neighbors=None,
                  snn_prune=None, clonotypes=False, clonotype_resolution=None, device_inflate=False, groups=None,
                  group_min_cells=None, group_min_af=None, group_test=False, group_test_max_p=None, pca=None,
                  pca_scale=False) -> dict:
    """The options run_pipeline gets beyond the reference's, each only when asked for: the variant
    options with --variants; the four coverage options with --coverage-stats, otherwise the filter
    thresholds and --recompute-reference that were given; the analysis options that were given (one
    that lacks what it needs, options.REQUIRES, or is out of range: a usage error); --device-inflate; --groups
    and the thresholds given with it (one given without --groups: a usage error); --group-test (without --groups:
    a usage error) and --group-test-max-p when given (without --group-test: a usage error); --pca (without
    --variants: a usage error) and --pca-scale (without --pca: a usage error)."""
    from .options import AnalysisOptions

    opts = AnalysisOptions(call_variants, cluster, clones, neighbors, snn_prune, clonotypes, clonotype_resolution)
    opts.check(click.UsageError)
    out = opts.given()
    if "clonotype_resolution" in out:  # (a plain float to click; the analyses load only now)
        from .analysis.clonotypes import check_resolution

        try:
            check_resolution(clonotype_resolution)
        except InvalidInputError as e:
            raise click.UsageError(f"--clonotype-resolution: {e}") from None
    if call_variants:
        out.update(variant_min_cells=variant_min_cells,
                   variant_min_strand_cor=variant_min_strand_cor, variant_min_vmr=variant_min_vmr,
                   variant_stabilize=variant_stabilize, variant_low_coverage=variant_low_coverage,
                   variant_min_coverage=variant_min_coverage)
    cov = dict(cell_min_mean_coverage=float(cell_min_mean_coverage),
               cell_min_coverage_breadth=float(cell_min_coverage_breadth),
               recompute_reference=bool(recompute_reference))
    if coverage_stats:
        out.update(coverage_stats=True, **cov)
    else:
        out.update({k: v for k, v in cov.items() if v})
    if device_inflate:
        out.update(device_inflate=True)
    for flag, value in (("--group-min-cells", group_min_cells), ("--group-min-af", group_min_af)):
        if value is not None and groups is None:
            raise click.UsageError(f"{flag} requires --groups")
    if group_test and groups is None:
        raise click.UsageError("--group-test requires --groups")
    if group_test_max_p is not None and not group_test:
        raise click.UsageError("--group-test-max-p requires --group-test")
    if group_test:
        out.update(group_test=True)
        if group_test_max_p is not None:
            out.update(group_test_max_p=group_test_max_p)
    if groups is not None:
        out.update(groups=str(groups))
        out.update({k: v for k, v in (("group_min_cells", group_min_cells), ("group_min_af", group_min_af))
                    if v is not None})
    if pca is not None and not call_variants:
        raise click.UsageError("--pca requires --variants")
    if pca_scale and pca is None:
        raise click.UsageError("--pca-scale requires --pca")
    if pca is not None:
        out.update(pca=int(pca))
        if pca_scale:
            out.update(pca_scale=True)
    return out


def _options(defaults: dict, helps: dict | None = None):
    d = defaults

    def deco(f):
        opts = [
            click.option("--input", "-i", "bam_path", default=".", type=click.Path(exists=True),
                         help="Input BAM file or 10x outs/ directory"),
            click.option("--genome", "-g", "mito_genome", default="chrM", show_default=True,
                         help="Mitochondrial chromosome name (e.g chrM, MT, or M)"),
            click.option("--barcodes", "-b", "barcode_file", default=None, type=click.Path(exists=True),
                         help="Barcode file (singlecell.csv, barcodes.tsv/csv, or auto-detect from BAM)"),
            click.option("--barcode-tag", "-bt", default="CB", show_default=True, help="BAM tag for cell barcode"),
            click.option("--min-barcode-reads", default=10, type=int, show_default=True,
                         help="Minimum reads per barcode when auto-detecting from BAM"),
            click.option("--output", "-o", "output_dir", default=d["output"], type=click.Path(),
                         show_default=True, help="Output directory for analysis results"),
            click.option("--threads", "-t", "ncores", default=None, type=int,
                         help="Number of threads (host side; the pileup runs on the GPU)"),
            click.option("--verbose", "-v", is_flag=True, default=d["verbose"], help="Enable verbose logging"),
            click.option("--batch-size", "batch_size", default=None, type=int,
                         help="Worker batch size (accepted for compatibility)"),
            click.option("--memory", "-m", "max_memory", default=d["memory"], type=float,
                         help="Maximum memory usage in GB"),
            click.option("--quality", "-q", "base_qual", default=d["quality"], type=int, show_default=True,
                         help="Minimum base quality (Phred score)"),
            click.option("--mapq", "min_mapq", default=d["mapq"], type=int, show_default=True,
                         help="Minimum alignment/mapping quality"),
            click.option("--min-reads", "-c", "min_reads", default=d["min_reads"], type=int, show_default=True,
                         help="Minimum deduplicated reads per cell to include in analysis"),
            click.option("--max-strand-bias", "-s", "max_strand_bias", default=1.0, type=float, show_default=True,
                         help="Maximum strand bias (0-1)"),
            click.option("--min-distance-from-end", "-e", "min_distance_from_end", default=d["dist"], type=int,
                         show_default=True, help="Minimum distance from read ends (bp)"),
            click.option("--deduplication", "-d", "dedup_mode",
                         type=click.Choice(DEDUP_CHOICES, case_sensitive=False), default=d["dedup"],
                         show_default=True, help="Deduplication strategy"),
            click.option("--format", "-f", "output_format", type=click.Choice(["txt", "hdf5"], case_sensitive=False),
                         default=d["format"], show_default=True, help="Output format"),
            click.option("--dry-run", is_flag=True, help="Show configuration and exit without processing"),
            click.option("--device", "device", default=0, type=int, show_default=True,
                         help="HIP device ordinal for the pileup engine"),
            click.option("--devices", "devices", default=None,
                         help="Comma-separated HIP devices to shard cells over (e.g. 0,1,2,3)"),
        ]
        for o in reversed(opts):
            f = o(f)
        return f

    return deco


RUN_DEFAULTS = dict(output="mgatk2/", verbose=True, memory=128, quality=20, mapq=30, min_reads=1, dist=5,
                    dedup="alignment_and_fragment_length", format="hdf5")
TENX_DEFAULTS = dict(output="mgatk2", verbose=False, memory=None, quality=0, mapq=0, min_reads=0, dist=0,
                     dedup="alignment_start", format="txt")


# ---------------------------------------------------------------------------
# helpers (cli/utils.py)
# ---------------------------------------------------------------------------
def _find_barcode_file(directory: Path) -> str | None:
    singlecell = directory / "singlecell.csv"
    if singlecell.exists():
        return str(singlecell)
    for pattern in ["filtered_peak_bc_matrix/barcodes.tsv", "filtered_tf_bc_matrix/barcodes.tsv.gz"]:
        if (directory / pattern).exists():
            return str(directory / pattern)
    logger.warning("No barcode file found")
    return None


def auto_detect_10x_structure(bam_path: str, barcode_file: str | None = None) -> tuple[str, str | None]:
    """cli/utils.py:18-52."""
    path = Path(bam_path)
    if path.is_dir():
        bam_file: Path | None = None
        if path.name == "outs" or "outs" in str(path):
            bam_file = path / "possorted_bam.bam"
            if not bam_file.exists():
                bam_file = path.parent / "outs" / "possorted_bam.bam"
        else:
            outs_dir = path / "outs"
            bam_file = outs_dir / "possorted_bam.bam" if outs_dir.exists() else None
        if bam_file and bam_file.exists():
            bam_path = str(bam_file)
            if not barcode_file:
                barcode_file = _find_barcode_file(bam_file.parent)
        else:
            logger.warning(f"No possorted_bam.bam found in {path}")
    elif path.is_file() and not barcode_file and path.parent.name == "outs":
        logger.info("Detected 10x BAM in outs directory")
        barcode_file = _find_barcode_file(path.parent)
    return str(Path(bam_path).resolve()), barcode_file


def normalise_mito_chr(mito_genome: str) -> str:
    """cli/utils.py:76-83."""
    if mito_genome.upper() in ["M", "MT"]:
        return "chrM"
    if mito_genome in ["chrM", "chrMT"]:
        return mito_genome
    logger.warning("Unusual mitochondrial chromosome name: %s", mito_genome)
    return mito_genome


def get_10x_parent_directory_name(bam_path: str) -> str:
    """cli/utils.py:86-108."""
    p = Path(bam_path)
    if p.parent.name == "outs":
        return p.parent.parent.name
    if "outs" in str(p.parent):
        cur = p.parent
        while cur.parent != cur:
            if cur.name == "outs":
                return cur.parent.name
            cur = cur.parent
    return p.parent.name if p.parent.name != "." else "mgatk2"


def setup_file_logging(log_file_path):
    handler = logging.FileHandler(log_file_path, mode="w")
    handler.setLevel(logging.INFO)
    handler.setFormatter(logging.Formatter("%(asctime)s - %(name)s - %(levelname)s - %(message)s"))
    logging.getLogger("mgatk2_amd").addHandler(handler)


def _determine_cores(ncores):
    if ncores is not None:
        return ncores
    for var in ("SLURM_CPUS_PER_TASK", "SLURM_NTASKS"):
        v = os.environ.get(var)
        if v:
            try:
                return int(v)
            except ValueError:
                break
    return max(1, multiprocessing.cpu_count())


def _count_barcodes(barcode_file: str | None) -> str:
    if not barcode_file:
        return "auto-detect from BAM"
    if barcode_file.endswith(".csv"):
        with open(barcode_file) as f:
            reader = csv.DictReader(f)
            headers = reader.fieldnames or []
            col = next((c for c in ("is__cell_barcode", "is_cell_barcode", "is_cell") if c in headers), None)
            return str(sum(1 for row in reader if col and row.get(col, "0") in ("1", "1.0", "True", "true", "TRUE")))
    with open(barcode_file) as f:
        return str(sum(1 for line in f if line.strip()))


def run_pipeline_command(bam_path, output_dir, barcode_file, barcode_tag, min_barcode_reads, mito_genome, ncores,
                         verbose, batch_size, max_memory, base_qual, min_mapq, min_reads, max_strand_bias,
                         min_distance_from_end, dedup_mode, output_format, sequential, dry_run=False,
                         original_bam_path=None, report_title=None, report_subtitle=None, working_directory=None,
                         device=0, devices=None, variant_args: dict | None = None) -> int:
    """cli/utils.py:124-289: returns 0 on success, 1 on a handled error."""
    from .pipeline import run_pipeline
    from .utils import validate_bam_file, validate_barcode_file

    if verbose:
        logging.getLogger("mgatk2_amd").setLevel(logging.DEBUG)
    logger.info("mgatk2 (MI355X engine) version %s", __version__)
    if barcode_file != "bulk":
        bam_path, barcode_file = auto_detect_10x_structure(bam_path, barcode_file)
    skip_dedup = dedup_mode.lower() == "none"
    use_fragment_length_dedup = dedup_mode.lower() in ["alignment_and_fragment_length", "fragment-length", "hybrid"]
    if not dry_run:
        log_file = Path(output_dir) / "output.log"
        log_file.parent.mkdir(parents=True, exist_ok=True)
        setup_file_logging(log_file)
        logger.info("Command executed: %s %s", os.path.realpath(sys.argv[0]) if sys.argv else "mgatk2",
                    " ".join(sys.argv[1:]))
        logger.info("Working directory: %s", os.getcwd())
        logger.info("Execution time: %s", datetime.now().strftime("%Y-%m-%d %H:%M:%S"))
    try:
        validate_bam_file(bam_path)
        if barcode_file:
            validate_barcode_file(barcode_file)
        os.makedirs(output_dir, exist_ok=True)
        mito_chr = normalise_mito_chr(mito_genome)
        cores = _determine_cores(ncores)
        logger.info("  Input BAM:              %s", os.path.realpath(bam_path))
        logger.info("  Input barcodes:         %s",
                    os.path.realpath(barcode_file) if barcode_file else "None (auto-detect from BAM)")
        logger.info("  Output directory:       %s", os.path.realpath(output_dir))
        logger.info("  Mitochondrial chr:      %s", mito_chr)
        logger.info("  Min base quality:       %s", base_qual)
        logger.info("  Min mapping quality:    %s", min_mapq)
        logger.info("  Min reads per cell:     %s", min_reads)
        logger.info("  Max strand bias:        %s", max_strand_bias)
        logger.info("  Deduplication:          %s", dedup_mode)
        logger.info("  Output format:          %s", output_format)
        logger.info("  Barcodes:               %s", _count_barcodes(barcode_file))
        logger.info("  HIP device:             %s", device)
        if variant_args and variant_args.get("call_variants"):
            logger.info("  Variant calling:        min cells %s, min strand cor %s, min vmr %s",
                        variant_args["variant_min_cells"], variant_args["variant_min_strand_cor"],
                        variant_args["variant_min_vmr"])
        if variant_args and any(k.startswith(("coverage_", "cell_min_", "recompute_")) for k in variant_args):
            logger.info("  Coverage QC:            tables %s, min mean coverage %s, min breadth %s, recompute reference %s",
                        variant_args.get("coverage_stats", False), variant_args.get("cell_min_mean_coverage", 0.0),
                        variant_args.get("cell_min_coverage_breadth", 0.0),
                        variant_args.get("recompute_reference", False))
        if variant_args and variant_args.get("cluster"):
            logger.info("  Clustering:             complete linkage, clones %s", variant_args.get("clones"))
        if variant_args and variant_args.get("neighbors") is not None:
            logger.info("  Neighbour graph:        k.param %s, SNN prune %s", variant_args["neighbors"],
                        variant_args.get("snn_prune", "1/15"))
        if variant_args and variant_args.get("clonotypes"):
            logger.info("  Clonotypes:             Louvain on the SNN graph, resolution %s",
                        variant_args.get("clonotype_resolution", 1.0))
        if variant_args and variant_args.get("groups") is not None:
            logger.info("  Cell groups:            %s, min cells %s, min heteroplasmy %s", variant_args["groups"],
                        variant_args.get("group_min_cells", 2), variant_args.get("group_min_af", 0.01))
        if variant_args and variant_args.get("group_test"):
            logger.info("  Group rank-sum tests:   max p %s", variant_args.get("group_test_max_p", 0.01))
        if variant_args and variant_args.get("pca") is not None:
            logger.info("  Principal components:   %s, scaled %s", variant_args["pca"],
                        variant_args.get("pca_scale", False))
        if variant_args and variant_args.get("device_inflate"):
            logger.info("  BGZF inflate:           on the device")
        if dry_run:
            return 0
        if report_title is None:
            report_title = get_10x_parent_directory_name(original_bam_path or bam_path)
        run_args = dict(
            bam_path=bam_path, barcode_file=barcode_file, output_dir=output_dir, sample_name="output_",
            min_baseq=base_qual, min_mapq=min_mapq, min_reads_per_cell=min_reads, output_format=output_format.lower(),
            max_strand_bias=max_strand_bias, min_distance_from_end=min_distance_from_end, barcode_tag=barcode_tag,
            min_barcode_reads=min_barcode_reads, mito_chr=mito_chr, n_cores=cores,
            worker_batch_size=batch_size if batch_size is not None else cores, io_batch_size=None,
            skip_deduplication=skip_dedup, use_fragment_length_dedup=use_fragment_length_dedup,
            sequential=sequential, report_title=report_title, report_subtitle=report_subtitle or
            "mgatk2 output analysis", working_directory=working_directory, device=device,
            devices=[int(x) for x in devices.split(",")] if devices else None,
        )
        if max_memory is not None:
            run_args["max_memory_gb"] = max_memory
        if variant_args:
            run_args.update(variant_args)
        run_pipeline(**run_args)
        return 0
    except InvalidInputError as e:
        logger.error("Input validation failed: %s", e)
        return 1
    except ProcessingError as e:
        logger.error("Processing failed: %s", e)
        return 1
    except Exception as e:
        logger.error("Unexpected error: %s", e)
        if verbose:
            import traceback

            traceback.print_exc()
        return 1


# ---------------------------------------------------------------------------
# commands
# ---------------------------------------------------------------------------
class OrderedGroup(click.Group):
    def list_commands(self, ctx):
        return list(self.commands)


@click.group(cls=OrderedGroup)
@click.version_option(version=__version__)
def cli():
    """mgatk2 (MI355X engine): per-cell mitochondrial pileup on AMD Instinct GPUs."""


@cli.command()
@_options(RUN_DEFAULTS)
@_variant_options
def run(bam_path, mito_genome, barcode_file, barcode_tag, min_barcode_reads, output_dir, ncores, verbose, batch_size,
        max_memory, base_qual, min_mapq, min_reads, max_strand_bias, min_distance_from_end, dedup_mode,
        output_format, dry_run, device, devices, **variant_kw):
    """Run mgatk2 with optimised defaults"""
    try:
        rc = run_pipeline_command(
            bam_path, output_dir, barcode_file, barcode_tag, min_barcode_reads, mito_genome, ncores, verbose,
            batch_size, max_memory, base_qual, min_mapq, min_reads, max_strand_bias, min_distance_from_end,
            dedup_mode, output_format, ncores == 1, dry_run=dry_run, original_bam_path=bam_path,
            report_title=get_10x_parent_directory_name(bam_path), report_subtitle="mgatk2 output analysis",
            working_directory=os.getcwd(), device=device, devices=devices, variant_args=_variant_args(**variant_kw))
    except KeyboardInterrupt:
        raise SystemExit(130) from None
    if rc:
        raise SystemExit(rc)


@cli.command()
@_options(TENX_DEFAULTS)
@_variant_options
def tenx(bam_path, mito_genome, barcode_file, barcode_tag, min_barcode_reads, output_dir, ncores, verbose, batch_size,
         max_memory, base_qual, min_mapq, min_reads, max_strand_bias, min_distance_from_end, dedup_mode,
         output_format, dry_run, device, devices, **variant_kw):
    """Run mgatk2 with original mgatk package behaviour"""
    rc = run_pipeline_command(
        bam_path, output_dir, barcode_file, barcode_tag, min_barcode_reads, mito_genome, ncores, verbose,
        batch_size, max_memory, base_qual, min_mapq, min_reads, max_strand_bias, min_distance_from_end, dedup_mode,
        output_format, ncores == 1, dry_run=dry_run, device=device, devices=devices,
        variant_args=_variant_args(**variant_kw))
    if rc:
        raise SystemExit(rc)


@cli.command()
@click.option("--input", "-i", "bam_path", type=click.Path(exists=True), required=True,
              help="Directory of BAM files (one BAM per cell)")
@click.option("--genome", "-g", "mito_genome", default="chrM", show_default=True)
@click.option("--output", "-o", "output_dir", default="mgatk2/", type=click.Path(), show_default=True)
@click.option("--threads", "-t", "ncores", default=None, type=int)
@click.option("--verbose", "-v", is_flag=True, default=True)
@click.option("--memory", "-m", "max_memory", default=128, type=float, show_default=True)
@click.option("--quality", "-q", "base_qual", default=20, type=int, show_default=True)
@click.option("--mapq", "min_mapq", default=30, type=int, show_default=True)
@click.option("--max-strand-bias", "-s", "max_strand_bias", default=1.0, type=float, show_default=True)
@click.option("--min-distance-from-end", "-e", "min_distance_from_end", default=5, type=int, show_default=True)
@click.option("--deduplication", "-d", "dedup_mode", type=click.Choice(DEDUP_CHOICES, case_sensitive=False),
              default="alignment_and_fragment_length", show_default=True)
@click.option("--format", "-f", "output_format", type=click.Choice(["txt", "hdf5"], case_sensitive=False),
              default="hdf5", show_default=True)
@click.option("--dry-run", is_flag=True)
@click.option("--device", "device", default=0, type=int, show_default=True)
@_variant_options
def call(bam_path, mito_genome, output_dir, ncores, verbose, max_memory, base_qual, min_mapq, max_strand_bias,
         min_distance_from_end, dedup_mode, output_format, dry_run, device, **variant_kw):
    """Run mgatk2 and treat each bam file as a single cell (commands/call.py)"""
    variant_args = _variant_args(**variant_kw)
    bam_files = sorted(Path(bam_path).glob("*.bam"))
    if not bam_files:
        logger.error(f"No BAM files (*.bam) found in directory: {bam_path}")
        raise SystemExit(1)
    mito_chr = normalise_mito_chr(mito_genome)
    logger.info("Auto-detected %s BAM files", len(bam_files))
    if dry_run:
        return
    for i, bam_file in enumerate(bam_files, 1):
        out = Path(output_dir) / bam_file.stem
        out.mkdir(parents=True, exist_ok=True)
        logger.info(f"[{i}/{len(bam_files)}] Processing: {bam_file.name} -> {out}")
        run_pipeline_command(str(bam_file), str(out), None, "CB", 10, mito_chr, ncores, verbose, 1, max_memory,
                             base_qual, min_mapq, 0, max_strand_bias, min_distance_from_end, dedup_mode, output_format,
                             ncores == 1, dry_run=False, device=device, variant_args=variant_args)
    logger.info("Analysis completed for all %s BAM files", len(bam_files))


@cli.command()
@click.option("--input", "-i", "input_dir", required=True, type=click.Path(exists=True, file_okay=False),
              help="Output directory of a finished run (holds output/counts.h5 and output/metadata.h5)")
@click.option("--output", "-o", "output_dir", default=None, type=click.Path(),
              help="Where coverage/, variants/ and groups/ are written  [default: the input directory]")
@click.option("--barcodes", "-b", "barcode_file", default=None, type=click.Path(exists=True),
              help="Analyse only the cells whose barcode is in this file (one per line)")
@click.option("--host-inflate", is_flag=True,
              help="Inflate the HDF5 chunks with libhdf5 on the host instead of the device (the same results)")
@click.option("--verbose", "-v", is_flag=True, help="Enable verbose logging")
@click.option("--device", "device", default=0, type=int, show_default=True, help="HIP device ordinal")
@_analysis_options
def analyze(input_dir, output_dir, barcode_file, host_inflate, verbose, device, **analysis_kw):
    """Run the analyses on the count files of a finished run (no BAM is read)"""
    args = _variant_args(**analysis_kw)
    from .pipeline import analyze_outputs

    if verbose:
        logging.getLogger("mgatk2_amd").setLevel(logging.DEBUG)
    try:
        analyze_outputs(input_dir, output_dir, barcodes=barcode_file, device=device, host_inflate=host_inflate, **args)
    except InvalidInputError as e:
        logger.error("Input validation failed: %s", e)
        raise SystemExit(1) from None
    except ProcessingError as e:
        logger.error("Processing failed: %s", e)
        raise SystemExit(1) from None


def main():
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    cli()


if __name__ == "__main__":
    main()
