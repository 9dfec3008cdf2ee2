"""QC metrics and report (mirror of src/analysis), and the analyses made on the device."""

from .clustering import HClust, cluster_heteroplasmy, hclust, pair_dist, write_cluster_outputs
from .qc import QCCalculator

__all__ = ["QCCalculator", "HClust", "cluster_heteroplasmy", "hclust", "pair_dist", "write_cluster_outputs"]
