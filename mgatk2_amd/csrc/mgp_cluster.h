// mgp_cluster.h — Euclidean pair distances and complete-linkage clustering on the device
// (internal interface between mgp_jobs.hip and mgp_cluster.hip; the C-ABI is mgp_pair_dist /
// mgp_hclust_dist / mgp_hclust in include/mgpileup.h).
//
// The step of mgatk's vignette after calculate_allele_freq: pheatmap's dist() over the cells
// and over the variants of the heteroplasmy matrix and hclust(..., "complete") on each
// (R/mgatk2_qc_plots.R:121-139). Items are the columns of x [n_feat][n_items] (feature-major:
// the loads over items are contiguous).
//
//   pair_dist():  D[i][j] = sqrt(sum_k (x[k][i] - x[k][j])^2), the full symmetric matrix
//   check_dist(): a caller's matrix is finite, >= 0 and symmetric (flags in `bad`)
//   linkage():    the n - 1 raw merge steps (i, j, height) of complete linkage on D
//
// Determinism. One thread makes a pair's whole sum, k ascending, s = fma(d, d, s) with
// d = x[k][i] - x[k][j] (the fma is explicit, so no compiler flag changes it; (-d)^2 == d^2
// exactly, so a diagonal tile's two halves agree), then one correctly rounded sqrt. The value
// depends on neither the tiling nor the launch shape; tiles above the diagonal are computed
// once and stored twice, so D[i][j] and D[j][i] are the same bytes; equal columns give d == 0
// in every term and a distance of exactly 0. The linkage only compares and selects: its
// output is a function of the matrix alone.
//
// Linkage rule (R's hclust.f for method "complete"). Clusters are named by their lowest
// member. Each step takes the smallest D over the active pairs i < j, ties to the smallest i
// then the smallest j, records (i, j, D), makes j inactive and sets D(i, k) = max(D(i, k),
// D(j, k)) for every active k. nn[r] is the first active k > r at row r's minimum and dnn[r]
// that minimum: since complete-linkage distances only grow, a row's list entry stays valid
// unless it pointed at i or j, and only those rows are scanned again.
//
// Waiting. linkage() is one workgroup of kLinkBlock threads that loops over the n - 1 steps
// with workgroup barriers only; no kernel here waits on another workgroup, spins on a flag
// or syncs a grid. Every loop's trip count is bounded by n alone (the rows to scan again are
// a list of at most n entries); no loop ends on a value of the matrix. The caller checks
// `bad` before it launches the linkage, so no comparison ever sees a NaN.
//
// Device memory of a call over n items and f features (bytes):
//   8 n^2 (D) + 8 n f (x; not for a caller's matrix) + 33 n (nn, dnn, active, scan list,
//   steps) + 4, each buffer rounded up to 256. n <= kMaxItems: 32 GiB of D at the bound.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mgp {
namespace cluster {

constexpr int64_t kMaxItems = 1 << 16;  // items of one call (the bound of every other job)
constexpr int64_t kMaxFeat = 1 << 24;   // features of one call
constexpr int kTile = 64;               // pair tile edge (items)
constexpr int kChunk = 32;              // features staged through LDS at a time
constexpr int kLinkBlock = 1024;        // the linkage workgroup (its stride over rows and columns)

enum Bad { BAD_VALUE = 1, BAD_ASYMMETRIC = 2 };

// x [nf][n] on the device; dist [n][n]; bad: one word, zeroed by the caller, BAD_VALUE ORed in
// when a value of x is not finite.
int pair_dist(const double* x, int n, int nf, double* dist, uint32_t* bad, hipStream_t s);
// bad: BAD_VALUE when an entry is not finite or is negative, BAD_ASYMMETRIC when
// dist[i][j] != dist[j][i].
int check_dist(const double* dist, int n, uint32_t* bad, hipStream_t s);
// dist [n][n] symmetric, finite, >= 0 (overwritten). nn, list, si, sj: n int32 each; dnn,
// sh: n doubles; act: n bytes. Steps 0..n-2 come out in si, sj, sh (i < j, the height).
int linkage(double* dist, int n, int32_t* nn, double* dnn, uint8_t* act, int32_t* list, int32_t* si, int32_t* sj,
            double* sh, hipStream_t s);

}  // namespace cluster
}  // namespace mgp
