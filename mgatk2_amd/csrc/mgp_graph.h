// mgp_graph.h — the cells' k-nearest-neighbour graph and its shared-nearest-neighbour graph on
// the device (internal interface between mgp_jobs.hip and mgp_graph.hip; the C-ABI is mgp_knn /
// mgp_snn in include/mgpileup.h).
//
// The step of mgatk's vignette after the heatmap, "Integration with Seurat/Signac": Signac's
// FindClonotypes first calls FindNeighbors on the heteroplasmy matrix, a kNN graph of the cells
// over the variants and Seurat's ComputeSNN on it, and hands the SNN graph to a graph clusterer.
// Items are the columns of x [n_feat][n_items], as in mgp_cluster.h.
//
//   knn():        per item the k others smallest under (distance, index), no n^2 storage
//   knn_check():  a caller's table is in range, names no row itself, repeats no entry
//   snn_*():      S_i = {i} + knn[i] sorted, the reverse lists as CSR, the pairs i < j counted and
//                 written with shared = |S_i & S_j| >= min_shared
//
// Distance. The number mgp_pair_dist returns for the pair: one thread's chain s = fma(d, d, s),
// k ascending, d = x[k][i] - x[k][j], then one sqrt (k_knn stages and walks the features as
// k_pair_dist does). Symmetric, equal columns at exactly 0.
//
// Order. A key is (the distance's bits as u64, the index): distances are >= +0, so their bits
// order as integers and the order is strict and total. Row i of the result is "row i of the
// matrix sorted by (value, index), i dropped, the first k". Since the order is strict, the result
// depends on neither the tiling, nor the splits of the candidate range, nor the launch shape.
//
// k_knn. A workgroup owns 64 query items and walks the 64-wide candidate tiles of its split
// of the candidate range; per tile it makes the 64 x 64 distances (staged through LDS, 4 x 4
// pairs a thread), leaves them in LDS (over the staging buffers) and each of its four waves
// offers the tile to its 16 rows: a lane takes one candidate, a ballot tells whether any key is
// below the row's k-th key so far, and only then the wave sorts the 64 candidates (a bitonic
// network over the lanes) and merges them with the row's list, one entry per lane. The lists
// are the call's partial output [S][n][k] in HBM (lane p reads and writes entry p only); the
// rows' k-th keys stay in LDS. k_knn_merge then merges the S lists of a row, a wave per row.
//
// Waiting. No kernel here waits on another workgroup, spins on a flag or syncs a grid. Every
// loop's trip count is bounded by n, k, n_feat, the number of splits or the length of a CSR
// list fixed before the launch; none ends on a data value (the list intersections run 2K fixed
// steps). The caller checks `bad` before it trusts a result.
//
// Device memory (bytes, each buffer rounded up to 256):
//   knn: 8 n f (x) + 12 S n k (the partial lists) + 12 n k (the result) + 4
//   snn: 4 n k (the table) + 4 n K (the sorted sets) + 4 n K (the reverse lists) + 28 n (degrees,
//        offsets, cursors, row counts, edge offsets) + 12 E (the triples), K = k + 1
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mgp {
namespace graph {

constexpr int64_t kMaxItems = 1 << 20;  // items of one call (no n^2 term is left to bound it lower)
constexpr int64_t kMaxFeat = 1 << 24;   // features of one call
constexpr int kMaxK = 64;               // neighbours per item: a row's list is one entry per lane
constexpr int64_t kMaxEdges = (int64_t)1 << 30;  // SNN edges of one call
constexpr int kTile = 64;               // query and candidate tile edge (items)
constexpr int kChunk = 32;              // features staged through LDS at a time

enum Bad { BAD_VALUE = 1, BAD_TABLE = 2 };

// the number of candidate splits of a call: `want` > 0 as asked for (at most the candidate
// tiles), otherwise enough workgroups to fill the device twice over
int knn_splits(int n, int want);
// x [nf][n] on the device; part_dist / part_idx [splits][n][k] (scratch), out_dist / out_idx
// [n][k]; bad: one word, zeroed by the caller, BAD_VALUE ORed in when a value of x is not finite.
int knn(const double* x, int n, int nf, int k, int splits, double* part_dist, int32_t* part_idx, double* out_dist,
        int32_t* out_idx, uint32_t* bad, hipStream_t s);
// idx [n][k]: BAD_TABLE when an entry is outside [0, n), is its own row or repeats in its row
int knn_check(const int32_t* idx, int n, int k, uint32_t* bad, hipStream_t s);
// sets [n][k + 1]: {i} + idx[i] ascending; deg [n] (zeroed here): the rows whose set holds m
int snn_sets(const int32_t* idx, int n, int k, int32_t* sets, int32_t* deg, hipStream_t s);
// off [n + 1] = the exclusive sums of v [n], off[n] the total (one workgroup)
int scan(const int32_t* v, int n, int64_t* off, hipStream_t s);
// rev [off[n]]: the rows of each m's reverse list, in no particular order; cur [n] scratch
int snn_reverse(const int32_t* sets, int n, int k, const int64_t* off, int32_t* cur, int32_t* rev, hipStream_t s);
// The pairs i < j with shared >= min_shared. eoff == nullptr: cnt [n] = the pairs of row i;
// otherwise the triples of row i from eoff[i] on.
int snn_edges(const int32_t* sets, int n, int k, const int64_t* off, const int32_t* rev, int min_shared,
              int32_t* cnt, const int64_t* eoff, int32_t* ei, int32_t* ej, int32_t* es, hipStream_t s);

}  // namespace graph
}  // namespace mgp
