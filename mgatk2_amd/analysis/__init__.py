"""QC metrics and report (mirror of src/analysis), and the analyses made on the device."""

from .clustering import HClust, cluster_heteroplasmy, hclust, pair_dist, write_cluster_outputs
from .neighbors import NeighborGraph, knn, min_shared_for, neighbor_graph, snn, write_neighbor_outputs
from .qc import QCCalculator

__all__ = ["QCCalculator", "HClust", "cluster_heteroplasmy", "hclust", "pair_dist", "write_cluster_outputs",
           "NeighborGraph", "knn", "min_shared_for", "neighbor_graph", "snn", "write_neighbor_outputs"]
