// mgp_pca.h — principal components of the heteroplasmy matrix on the device (internal interface
// between mgp_jobs.hip and mgp_pca.hip; the C-ABI is mgp_pca / mgp_sym_eig in include/mgpileup.h).
//
// The first use mgatk's vignette names for the matrix, dimensionality reduction: R's
// prcomp(t(af), center = TRUE, scale. = <flag>). Items are the columns of x [n_feat = m][n_items = n],
// as in mgp_cluster.h. Every number is a chain of fp64 operations in an order fixed by the input's
// shape alone, so the bytes depend on neither the tile, nor the grid, nor the
// device. No float atomics; fp contraction is off in mgp_pca.hip and every fma is written out.
//
// A slab is kSlab = 1,024 consecutive items (the last may be short); the slab is part of the
// definition. S = the number of slabs.
//   mean[f]    per slab s = s + x from 0.0 in ascending i; the slab sums added in ascending slab
//              order from 0.0; one division by n
//   xc         x - mean, one rounding
//   var[f]     per slab s = fma(xc, xc, s); the slab sums added in order; / (n - 1); sd = sqrt(var)
//   z          xc, or with scale xc / sd (0 where sd == 0)
//   cov[a][b]  per slab s = fma(z[a][i], z[b][i], s); the slab sums added in order; / (n - 1).
//              One triangle is computed and mirrored: exactly symmetric
//   scores     score[c][i]: s = fma(z[f][i], vec[c][f], s) in ascending f from 0.0
//
// Kernels.
//   k_slab_sums    a workgroup owns 64 features of one slab: chunks of 32 items are staged through
//                  LDS by all 256 threads (coalesced along items), then thread t < 64 walks feature
//                  t's chunk in ascending order: one thread owns a (feature, slab) chain
//   k_slab_reduce  one thread per feature adds the S partial sums in order and divides
//   k_standardize  z to HBM (8 n m bytes)
//   k_cov          a workgroup per (tile of a, tile of b >= a, slab); chunks of 32 items of both
//                  tiles staged through LDS item-major, an R x R register tile per thread (tile edge
//                  16 R, R = 1, 2, 4) accumulates in ascending i; partials [S][m][m]
//   k_cov_reduce   one thread per a <= b adds the slabs in order, divides and writes both places
//   k_sym_check    finite, a[i][j] == a[j][i], and the largest |a[i][j]| (an integer atomicMax on
//                  the bits of a non-negative double)
//   k_jacobi_step  one step of the round-robin order (below), A and V ping-ponged in HBM
//   k_order_vec    the chosen eigenvectors in the output order with the sign rule applied
//   k_scores       a workgroup owns 256 items and 8 components; the loadings go through LDS in
//                  chunks of 256 features, z is read coalesced along items
//
// Jacobi. Cyclic two-sided Jacobi in the round-robin (tournament) order: m' = m rounded up to
// even, a sweep is m' - 1 steps, step r pairs m' - 1 with r and every other i with
// (2 r - i) mod (m' - 1); a pair that holds the padding index m is skipped. The m' / 2 rotations
// of a step are disjoint and all computed from the same snapshot A; A' = J^T A J and V' = V J are
// written to the other buffers. For the pair p < q with pivot a_pq:
//   tau = (a_qq - a_pp) / (2 a_pq), t = sign(tau) / (|tau| + sqrt(1 + tau^2))  (sign(0) = +1),
//   c = 1 / sqrt(1 + t^2), s = t c.
// Row p has (alpha, beta) = (c, -s), row q (c, s); a row outside a rotated pair (1, 0). With i', j'
// the partners of i and j,
//   a'_ij = (alpha_i alpha_j a_ij + beta_i beta_j a_i'j') + (beta_i alpha_j a_i'j + alpha_i beta_j a_ij'),
// every product grouped as (coefficient product) * entry: the expression is the same under i <-> j,
// so A stays exactly symmetric. The rotated pair's own places are the usual closed forms:
// a'_pq = a'_qp = 0, a'_pp = a_pp - t a_pq, a'_qq = a_qq + t a_pq. V is kept transposed (row c is
// vector c): vt'_i. = alpha_i vt_i. + beta_i vt_i'. .
// Skipped pairs. A pair rotates only if |a_pq| > 2^-53 sqrt(|a_pp|) sqrt(|a_qq|) (the relative
// threshold: below it the rotation changes neither diagonal entry's last bit by more than one) and
// |a_pq| > 2^-63 max|a_ij| of the input (the absolute threshold: it ends the iteration where the
// diagonal is zero, e.g. inside the null space of a singular matrix; at 2^-63 it adds less than
// m 2^-63 |A| to any eigenvalue). An exactly zero pivot never rotates, so a diagonal matrix, the zero
// matrix and a zero row / column take no rotation at all. The loop ends after the first sweep in
// which no pair rotated; the count returned is the sweeps in which one did. kMaxSweeps sweeps that
// all rotated are an error, never a partial result.
//
// Waiting. No kernel waits on another workgroup; every loop's trip count is fixed by n, m or k
// before the launch. The only value read back during the iteration is the "rotated" word, once a
// sweep.
//
// Device memory (bytes, each buffer rounded up to 256), S = ceil(n / 1024):
//   pca:     16 n m (x and z) + 8 S m^2 (the covariance's slab partials) + 8 S m + 40 m^2 (cov, A and
//            V twice) + 8 k (m + n) + 24 m
//   sym_eig: 48 m^2 (the input, A and V twice, the ordered vectors) + 12 m
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mgp {
namespace pca {

constexpr int64_t kMaxItems = 1 << 20;  // items of one call
constexpr int64_t kMaxFeat = 2048;      // features of one call (A and V are 8 m^2 bytes each, twice)
constexpr int kSlab = 1024;             // items of a slab: part of the definition
constexpr int kMaxSweeps = 60;          // Jacobi sweeps before the call gives up (an error)

enum Bad { BAD_VALUE = 1, BAD_ASYMMETRIC = 2 };

inline int slabs(int64_t n) { return (int)((n + kSlab - 1) / kSlab); }
// the covariance's tile edge: `want` if it is 16, 32 or 64, otherwise by m
int cov_tile(int m, int want);

// part [S][m]: per (slab, feature) the sum of x (mean == nullptr; BAD_VALUE ORed into bad when a
// value of x is not finite) or of (x - mean[f])^2 as the fma chain
int slab_sums(const double* x, const double* mean, int n, int m, double* part, uint32_t* bad, hipStream_t s);
// out[f] = (part[0][f] + part[1][f] + ...) / div; out_sqrt (may be null) its square root
int slab_reduce(const double* part, int m, int S, double div, double* out, double* out_sqrt, hipStream_t s);
// z [m][n] = x - mean, divided by sd when sd != nullptr (0 where sd == 0)
int standardize(const double* x, const double* mean, const double* sd, int n, int m, double* z, hipStream_t s);
// cov [m][m] from z [m][n]; part [S][m][m] scratch
int covariance(const double* z, int n, int m, int tile, double* part, double* cov, hipStream_t s);
// bad: BAD_VALUE / BAD_ASYMMETRIC; maxabs: the bits of the largest |a[i][j]| (both zeroed by the caller)
int sym_check(const double* a, int m, uint32_t* bad, unsigned long long* maxabs, hipStream_t s);
// vt [m][m] = the identity
int identity(double* vt, int m, hipStream_t s);
// step `step` (0 .. m' - 2) from (a, vt) into (a2, vt2); *flag = 1 when a pair rotated
int jacobi_step(const double* a, const double* vt, double* a2, double* vt2, int m, int step,
                const unsigned long long* maxabs, uint32_t* flag, hipStream_t s);
// out [k][m]: row c = row perm[c] of vt, negated when its entry of largest magnitude (the lowest
// index among equals) is negative
int order_vectors(const double* vt, const int32_t* perm, int m, int k, double* out, hipStream_t s);
// out [k][n]: the scores of z [m][n] on vec [k][m]
int scores(const double* z, const double* vec, int n, int m, int k, double* out, hipStream_t s);

}  // namespace pca
}  // namespace mgp
