// mgp_qc.h — coverage QC on the device (internal interface between mgp_jobs.hip and
// mgp_qc.hip; the C-ABI is mgp_cell_coverage_* / mgp_position_* in include/mgpileup.h).
//
// The front half of mgatk's downstream workflow (calculate_cell_coverage_stats,
// calculate_position_coverage_stats, calculate_strand_coverage_stats,
// calculate_transposition_stats; R over counts.h5) is dense passes over the cells x
// positions matrix. The rows are still in HBM when a run ends, so the passes read them
// there, through txtgz::Rows plus the Tn5 planes:
//   cell_stats()      per population cell, over all L positions: the depth's sum, sum of
//                     squares, max, the counts d > 0, d >= 10, d >= 50 and the two middle
//                     order statistics (a radix select over the cell's depths)
//   pos_stats()       per position, over the population: the same sums and counts, the
//                     fwd / rev / Tn5 sums, the cells with a Tn5 cut and the base tallies
//   pos_depth_hist()  one round of the per-position radix select over cells, and
//   pos_depth_next()  its last step; the host drives them (analysis/coverage.py), so that
//                     several contexts and several calls merge exactly
// The device makes integers only; every floating-point column is one host division.
//
// Exactness, as for the variant moments: the sum passes are exact while every depth and
// count is below variants::kMaxCount = 2^24, a call covers at most variants::kMaxCells =
// 2^16 cells and L <= 2^16 (2^16 terms below 2^48). They report a larger value through
// `bad`; the caller rejects the other two. The histogram and `next` passes have no bound on
// the values.
//
// Determinism: every combination is an integer atomic add, max or min (order-free); two
// calls on the same rows return the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgp_sweep.h"
#include "mgp_txtgz.h"
#include "mgp_variants.h"

namespace mgp {
namespace qc {

using sweep_detail::Tn5;

constexpr int kMaxL = 1 << 16;  // positions of a cell_stats() / pos_stats() call

// cell_stats(): per cell, 2 u64 (CELL64_*) and 6 u32 (CELL32_*), cell-major
enum { CELL64_SD, CELL64_SD2, CELL64_N };
enum { CELL32_MAX, CELL32_NPOS, CELL32_N10, CELL32_N50, CELL32_MIDLO, CELL32_MIDHI, CELL32_N };
// pos_stats(): u64 planes [L] (then the tallies [L][4]) and u32 planes [L]
enum { POS64_SD, POS64_SD2, POS64_FWD, POS64_REV, POS64_TF, POS64_TR, POS64_TALLY, POS64_N = POS64_TALLY + 4 };
enum { POS32_NPOS, POS32_N10, POS32_N50, POS32_NTN5, POS32_MAX, POS32_N };

// cells: device list of row indices (-1: an all-zero row), n of them, or null = rows 0..n-1.
// out64 [n][CELL64_N], out32 [n][CELL32_N] (written, not accumulated); bad: one word,
// zeroed here, set nonzero when a depth reaches kMaxCount.
int cell_stats(const txtgz::Rows& rows, const int32_t* cells, int64_t n, unsigned long long* out64, uint32_t* out32,
               uint32_t* bad, hipStream_t s);
// acc64 [POS64_N][L] and acc32 [POS32_N][L], zeroed here; bad as above (depths and counts)
int pos_stats(const txtgz::Rows& rows, const Tn5& tn5, const int32_t* cells, int64_t n, unsigned long long* acc64,
              uint32_t* acc32, uint32_t* bad, hipStream_t s);
// hist [L][256], zeroed here: per position, the cells with d >> (shift + 8) == prefix[p]
// (shift = 24: every cell) by (d >> shift) & 255. shift in {0, 8, 16, 24}.
int pos_depth_hist(const txtgz::Rows& rows, const int32_t* cells, int64_t n, int shift, const uint32_t* prefix,
                   uint32_t* hist, hipStream_t s);
// n_le [L]: cells with d <= v[p]; next [L]: the smallest d > v[p], 0xFFFFFFFF if none
int pos_depth_next(const txtgz::Rows& rows, const int32_t* cells, int64_t n, const uint32_t* v, uint32_t* n_le,
                   uint32_t* next, hipStream_t s);

}  // namespace qc
}  // namespace mgp
