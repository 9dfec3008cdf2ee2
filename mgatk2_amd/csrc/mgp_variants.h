// mgp_variants.h — variant statistics and heteroplasmy on the device (internal interface
// between mgp_jobs.hip and mgp_variants.hip; the C-ABI is mgp_variant_* / mgp_allele_freq_*
// in include/mgpileup.h).
//
// mgatk's variant calling (identify_variants / calculate_allele_freq, R over counts.h5)
// reduces, for every (position, base), the cells' fwd / rev counts of the base and their
// filtered depth. The count rows are still resident in HBM when a run ends, so the
// reductions read them there, through the writers' txtgz::Rows description:
//   pass 1  moments():  the integer moments below and the sum of the per-cell allele
//                       frequencies, all 4 bases from one row load per (cell, position)
//   pass 2  dev2():     the sum of squared deviations from a mean the host made of pass 1
//   gather  gather():   the cells x variants allele-frequency matrix of listed variants
//
// Exactness. Every integer moment is an exact sum while
//   * every fwd and rev count that enters a call is below kMaxCount = 2^24, and
//   * a call covers at most kMaxCells = 2^16 cells:
// the largest terms are f^2, r^2 and f r < 2^48, and 2^16 of them stay below 2^64 (the
// depth sums: 2^16 x 2^32 = 2^48). moments() reports a count at or above 2^24 through
// `bad`; the caller rejects more cells than 2^16. A larger population goes in several
// calls whose moments the host adds (analysis/variants.py: merge_moments).
//
// Determinism. The integer moments are integer atomics (order-free). The fp64 sums never
// are: a thread adds its slab's cells in list order, the slabs' partials are then added in
// slab order by k_combine, and the slab size depends on the cell count alone. Two calls on
// the same rows return the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgp_txtgz.h"

namespace mgp {
namespace variants {

constexpr uint32_t kMaxCount = 1u << 24;  // fwd / rev counts below this are summed exactly
constexpr int64_t kMaxCells = 1 << 16;    // cells of one call

// u64 planes of moments()' accumulator `acc`, each [L][4] (position-major, bases A, C, G, T):
// cells with fwd + rev > 0; cells with fwd >= 2 and rev >= 2; sum of fwd + rev; then over
// the cells with fwd > 0: their number, and the sums of fwd, rev, fwd^2, rev^2, fwd x rev.
enum Field { F_NDET, F_NCONF, F_STOTAL, F_M, F_SF, F_SR, F_SFF, F_SRR, F_SFR, F_N };
// then two [L] planes: the depth sum, and the cells with depth < thr
inline size_t acc_words(int L) { return (size_t)L * (4 * F_N + 2); }
inline size_t acc_scov(int L) { return (size_t)L * 4 * F_N; }
inline size_t acc_nlow(int L) { return (size_t)L * (4 * F_N + 1); }

// cell slabs of a call over n cells (grid.y; the fp64 partials are [slabs][L][4])
int slabs(int64_t n);

// cells: device list of row indices (-1: an all-zero row), n of them, or null = rows 0..n-1.
// thr: cells of depth < thr are "low" (0: none). acc: acc_words(L) u64, zeroed here.
// part: slabs(n) x L x 4 doubles. s_af [L][4]: sum of af over the cells that are not low.
// bad: one word, set nonzero when a count reaches kMaxCount.
int moments(const txtgz::Rows& rows, const int32_t* cells, int64_t n, uint32_t thr, unsigned long long* acc,
            double* part, double* s_af, uint32_t* bad, hipStream_t s);
// out [L][4]: sum over the cells that are not low of (af - mu[p][b])^2
int dev2(const txtgz::Rows& rows, const int32_t* cells, int64_t n, uint32_t thr, const double* mu, double* part,
         double* out, hipStream_t s);
// out [n_var][n]: (fwd + rev) / depth of base[v] at pos[v] where depth >= max(min_cov, 1), else 0
int gather(const txtgz::Rows& rows, const int32_t* cells, int64_t n, const int32_t* pos, const int32_t* base,
           int64_t n_var, uint32_t min_cov, double* out, hipStream_t s);

}  // namespace variants
}  // namespace mgp
