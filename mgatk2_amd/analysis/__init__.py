"""QC metrics and report (mirror of src/analysis), and the analyses made on the device."""

from .clonotypes import Clonotypes, Communities, communities, find_clonotypes, modularity, write_clonotype_outputs
from .clustering import HClust, cluster_heteroplasmy, hclust, pair_dist, write_cluster_outputs
from .neighbors import NeighborGraph, knn, min_shared_for, neighbor_graph, snn, write_neighbor_outputs
from .pca import PcaResult, principal_components, write_pca_outputs
from .qc import QCCalculator

__all__ = ["QCCalculator", "HClust", "cluster_heteroplasmy", "hclust", "pair_dist", "write_cluster_outputs",
           "NeighborGraph", "knn", "min_shared_for", "neighbor_graph", "snn", "write_neighbor_outputs",
           "Clonotypes", "Communities", "communities", "find_clonotypes", "modularity", "write_clonotype_outputs",
           "PcaResult", "principal_components", "write_pca_outputs"]
