"""The analyses of a finished run's heteroplasmy matrix, declared once, by key and in the order they
run: CellProcessor.enable / stage_result and MtDNAPipeline.run are driven by STAGES."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

from . import clonotypes, clustering, neighbors


@dataclass(frozen=True)
class Stage:
    key: str            # the stage's name, and its key in CellProcessor.last_timing
    field: str          # the EngineResult field its result is set on
    needs: str          # what must be on before it: "variants", or an earlier stage's key
    refusal: str        # the error when that is off
    options: tuple      # (name, default, checker) of each option
    compute: Callable   # (res, device, **options) -> the result
    write: Callable     # (result, barcodes, table, output_dir): the stage's files in variants/
    log: Callable       # result -> the arguments of the run's log line, None with nothing to report


STAGES = {s.key: s for s in (
    Stage("cluster", "clusters", "variants", "clustering needs the variants (enable_variants first)",
          (("clones", None, clustering.check_clones),),
          lambda r, dev, **o: clustering.cluster_heteroplasmy(r.allele_freq, table=r.variants, device=dev, **o),
          clustering.write_cluster_outputs,
          lambda c: None if c.cells is None else ("Clustered %d cells and %d variants", c.cells.n, c.variants.n)),
    Stage("neighbors", "neighbors", "variants", "the neighbour graph needs the variants (enable_variants first)",
          (("neighbors", 20, neighbors.check_neighbors), ("prune", neighbors.DEFAULT_PRUNE, neighbors.check_prune)),
          lambda r, dev, **o: neighbors.neighbor_graph(r.allele_freq, table=r.variants, device=dev, **o),
          lambda g, barcodes, table, output_dir: neighbors.write_neighbor_outputs(g, barcodes, output_dir),
          lambda g: None if g.idx is None else ("Neighbour graph: %d cells, k.param %d, %d SNN edges", g.n, g.k_param,
                                                int(g.i.size))),
    Stage("clonotypes", "clonotypes", "neighbors", "the clonotypes need the neighbour graph (enable_neighbors first)",
          (("resolution", 1.0, clonotypes.check_resolution),),
          lambda r, dev, **o: clonotypes.find_clonotypes(r.neighbors, r.allele_freq, table=r.variants, device=dev, **o),
          lambda c, barcodes, table, output_dir: clonotypes.write_clonotype_outputs(c, barcodes, output_dir),
          lambda c: None if c.result is None else (
              "Clonotypes: %d of %d cells, modularity %.6f (resolution %s, %d levels)", c.result.n_communities, c.n,
              c.result.modularity, c.resolution, len(c.result.levels))),
)}
