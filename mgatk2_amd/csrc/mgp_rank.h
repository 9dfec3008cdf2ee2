// mgp_rank.h — the rank sums of every feature's items per group on the device (internal
// interface between mgp_jobs.hip and mgp_rank.hip; the C-ABI is mgp_rank_sums in
// include/mgpileup.h).
//
// The step after FindClonotypes in the vignette's Seurat half: FindAllMarkers on the alleles
// assay, whose default test is the Wilcoxon rank-sum test of each variant, a group against the
// rest. Items are the columns of x [n_feat][n_items], as in mgp_cluster.h and mgp_graph.h (the
// orientation of the heteroplasmy matrix: each variant's cells contiguous).
//
// Per feature f the items are ordered by value (-0.0 equals +0.0). A tie class is a maximal run
// of equal values at the 0-based sorted positions lo..hi; each of its members has the midrank
// (lo + hi + 2) / 2. The device returns integers only:
//   r2[f][g]   the sum over the items of group g of lo + hi + 2 (twice the midrank sum; <= 2^41)
//   pos[f][g]  the items of group g with a value > 0
//   ties[f]    the sum over the tie classes of t^3 - t, t = hi - lo + 1 (<= 2^60)
// Integer adds, exact and independent of their order; the order inside a tie class changes no
// member's lo or hi, so the sort need not be stable and the result is a function of the input
// alone: not of the tile, the batch or the launch shape. U, AUC, z and p are host arithmetic on
// these (analysis/group_tests.py).
//
// Keys. The order-preserving u64 of v = x + 0.0: sign set -> ~bits, else bits | 1 << 63. The
// payload is the item's group (u32). A row is padded to P = the next power of two >= n with the
// all-ones key, which no finite value maps to, and the payload kPadGroup.
//
// Sort. A bitonic network per row. The steps with a stride below the tile (T elements, at most
// 4,096: 8 + 4 bytes each as two arrays, 48 KiB of LDS) run in LDS, one workgroup per tile:
// sort_tiles() makes the keys and runs every stage up to T; for each larger stage, cx_global()
// is one compare-exchange pass over all rows of the batch per stride >= T and merge_tiles() then
// finishes the stage's strides below T. At n = 2^20 and T = 4,096 that is 36 global passes.
//
// Ranks. rank_sums(): a workgroup walks kSpan consecutive sorted positions of one row, 256 at a
// time. A position's lo is the running maximum of the class starts before it and its hi the
// running minimum of the class ends after it (a scan over the 256); a class that begins before
// the span or ends after the 256 is found by a binary search of the row, log2 P + 1 fixed steps.
// The sums go to a table in LDS while n_groups <= kLdsGroups, and from there (or directly, above
// that) to the result by atomic adds; the position at lo adds t^3 - t.
//
// Waiting. No kernel here waits on another workgroup, spins on a flag or syncs a grid; every
// loop's trip count is fixed by n, the tile and n_groups before the launch, none ends on a data
// value. `bad` is checked by the caller before it trusts a result: BAD_LABEL after check_labels()
// and before any kernel that indexes by a label, BAD_VALUE after each batch.
//
// Device memory (bytes, each buffer rounded up to 256): 4 n (the labels) + 4, and per feature of
// a batch 8 n (x) + 12 P (keys and payloads) + 12 n_groups + 8 (the results). A batch is
// batch_features() = kBudget / that, at least 1 and at most n_feat (MGP_RANK_BATCH overrides it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mgp {
namespace rank {

constexpr int64_t kMaxItems = 1 << 20;   // items of one call
constexpr int64_t kMaxFeat = 1 << 24;    // features of one call
constexpr int32_t kMaxGroups = 1 << 16;  // groups of one call
constexpr int kMaxTile = 4096;           // elements of an LDS tile (MGP_RANK_TILE lowers it)
constexpr int kMinTile = 64;
constexpr int kLdsGroups = 2048;         // n_groups up to here: the rank kernel's table is in LDS
constexpr int kSpan = 4096;              // sorted positions of one rank workgroup
constexpr int64_t kBudget = (int64_t)1 << 30;  // device bytes of one batch of features
constexpr uint32_t kPadGroup = 0xffffffffu;

enum Bad { BAD_VALUE = 1, BAD_LABEL = 2 };

// the padded row length: the next power of two >= n (n >= 1)
int64_t padded(int64_t n);
// the tile of a call: `want` when it is a power of two in kMinTile..kMaxTile, else kMaxTile
int tile_of(int want);
// the features of one batch: `want` > 0 as asked for, otherwise what kBudget holds; 1..n_feat
int64_t batch_features(int64_t n, int64_t n_feat, int32_t n_groups, int64_t want);

// group [n]: BAD_LABEL ORed into *bad when a label is outside [0, n_groups)
int check_labels(const int32_t* group, int n, int32_t n_groups, uint32_t* bad, hipStream_t s);
// x [rows][n] on the device, group [n] checked; keys / pay [rows][P] (scratch, left sorted by key);
// r2 [rows][n_groups], pos [rows][n_groups], ties [rows]: zeroed here, then the sums. BAD_VALUE
// is ORed into *bad when a value of x is not finite (the results are then not to be used).
int sums(const double* x, const int32_t* group, int n, int64_t rows, int32_t n_groups, int tile, uint64_t* keys,
         uint32_t* pay, uint64_t* r2, uint32_t* pos, uint64_t* ties, uint32_t* bad, hipStream_t s);

}  // namespace rank
}  // namespace mgp
