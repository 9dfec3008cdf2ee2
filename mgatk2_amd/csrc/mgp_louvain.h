// mgp_louvain.h — Louvain communities of an integer-weighted graph on the device (internal
// interface between mgp_jobs.hip and mgp_louvain.hip; the C-ABI is mgp_louvain in
// include/mgpileup.h, which pins the definition).
//
// The second half of Signac's FindClonotypes: FindClusters on the SNN graph that mgp_snn makes.
// The CPU tools visit the vertices one after the other in a random order; here every vertex of
// a pass decides from one snapshot of the labels and the community totals, and every sum is an
// integer sum (edge weights are integers in units of 2^-20), so 64-bit integer atomics may add
// in any order and the result is a function of the input alone.
//
//   build:      edges checked, degrees counted, scanned, the symmetric CSR filled; a repeated
//               pair is found by inserting each row's forward entries into the row's table
//   move:       per vertex the weights into each neighbouring community, then the best gain.
//               Three shapes by row length: a wave per row (one entry per lane, matched across
//               the lanes), a workgroup per row with an open-addressed community -> sum table in
//               LDS, and the same with the table in the row's slice of a global scratch
//   apply:      the moved count and the new totals (integer atomics)
//   score:      I (the internal weight) and the exact partial sums of tot_c^2 as (hi, lo) pairs
//   aggregate:  the non-empty communities renumbered (flag, scan), the coarse edges summed in
//               per-row hash tables with integer atomics, counted, scanned and compacted
//
// Waiting. No kernel here waits on another workgroup, spins on a flag or syncs a grid. Every
// loop's trip count is bounded by the number of vertices or entries, a row's length or a table's
// capacity, all fixed before the launch; a probe sequence ends after `capacity` steps and a full
// table is a BAD_TABLE status, not a spin. The caller checks `bad` before it trusts a result.
//
// Device memory (bytes, each buffer rounded up to 256), m = 2 * edges (the directed entries):
//   12 edges (the edge list) + 2 * 16 m (two CSRs: neighbour, source, weight) + 12 * 2 m (the
//   tables: key, sum) + about 120 n (offsets, degrees, labels, totals, lists, maps) + 4 KiB
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mgp {
namespace louvain {

constexpr int64_t kMaxVertices = 1 << 20;
constexpr int64_t kMaxEdges = (int64_t)1 << 30;
constexpr int32_t kMaxWeight = 1 << 20;  // an edge's weight, in units of 2^-20
constexpr int kMaxLevels = 64;           // the cap on `max_levels`
constexpr int kMaxPasses = 1 << 16;      // the cap on `max_passes`
constexpr int kWaveRow = 64;             // rows up to here: a wave, one entry per lane
constexpr int kLdsRow = 2048;            // rows up to here: a workgroup and the LDS table
constexpr int kLdsSlots = 2 * kLdsRow;   // 48 KiB of (key, sum): three workgroups a compute unit
constexpr int kScoreBlocks = 256;        // partial (hi, lo) pairs of sum tot^2 per pass

enum Bad { BAD_EDGE = 1, BAD_WEIGHT = 2, BAD_REPEAT = 4, BAD_TABLE = 8 };

// a level's graph: row v is entries off[v] .. off[v + 1], src[e] = v for them
struct Csr {
    int64_t* off;
    int32_t* nbr;
    int32_t* src;
    uint64_t* w;
};

// off [n + 1] = the exclusive sums of v [n], off[n] the total (one workgroup)
int scan32(const int32_t* v, int64_t n, int64_t* off, hipStream_t s);
int scan64(const int64_t* v, int64_t n, int64_t* off, hipStream_t s);

// deg [n] and d [n] (both zeroed here) from the edges that pass the checks; the others set bad
int build_degrees(const int32_t* ei, const int32_t* ej, const int32_t* wq, int64_t ne, int n, int32_t* deg,
                  uint64_t* d, uint32_t* bad, hipStream_t s);
// the CSR of the same edges; cur [n] scratch
int build_fill(const int32_t* ei, const int32_t* ej, const int32_t* wq, int64_t ne, int n, int32_t* cur, Csr g,
               hipStream_t s);
// BAD_REPEAT when a pair occurs twice; tkeys [2 m] scratch
int build_repeats(Csr g, int64_t m, int32_t* tkeys, uint32_t* bad, hipStream_t s);

// c[v] = v, tot[v] = d[v]; the rows longer than wave_row into list_mid (up to lds_row) or
// list_long, counts [2] (zeroed here) their numbers
int level_start(Csr g, int n, const uint64_t* d, int32_t* c, uint64_t* tot, int wave_row, int lds_row,
                int32_t* list_mid, int32_t* list_long, int32_t* counts, hipStream_t s);
// next[v] for every vertex with an entry (the others keep next[v] as the caller set it)
int move(Csr g, int n, const int32_t* c, const uint64_t* tot, const uint64_t* d, uint64_t m2, double gamma, int odd,
         int wave_row, const int32_t* list_mid, int n_mid, const int32_t* list_long, int n_long, int32_t* tkeys,
         uint64_t* tvals, int32_t* next, uint32_t* bad, hipStream_t s);
// tot_next [n] (zeroed here) and *moved (zeroed here)
int apply(int n, const int32_t* c, const int32_t* next, const uint64_t* d, uint64_t* tot_next, int32_t* moved,
          hipStream_t s);
// *internal (zeroed here) = I; partial [kScoreBlocks][2] = (hi, lo) sums of tot^2 (unused pairs 0)
int score(Csr g, int64_t m, int n, const int32_t* c, const uint64_t* self, const uint64_t* tot, uint64_t* internal,
          uint64_t* partial, hipStream_t s);

// flag [n] (zeroed here) = 1 for the labels in use
int agg_flag(int n, const int32_t* c, int32_t* flag, hipStream_t s);
// map[u] = ren[c[map[u]]] for the n0 input vertices
int agg_map(int n0, int32_t* map, const int32_t* c, const int64_t* ren, hipStream_t s);
// The next level's d2, self2 [n2] and the count cap [n2] of each coarse row's cross entries (all
// zeroed here)
int agg_vertices(Csr g, int64_t m, int n, int n2, const int32_t* c, const int64_t* ren, const int32_t* flag,
                 const uint64_t* tot, const uint64_t* self, uint64_t* d2, uint64_t* self2, int64_t* cap,
                 hipStream_t s);
// the coarse rows' tables (row r: 2 cap[r] slots from 2 slot[r]), filled from the cross entries
int agg_insert(Csr g, int64_t m, const int32_t* c, const int64_t* ren, const int64_t* slot, int32_t* tkeys,
               uint64_t* tvals, uint32_t* bad, hipStream_t s);
// g2 == nullptr: deg2 [n2] = the keys of each row's table; otherwise the rows written from g2->off
int agg_rows(int n2, const int64_t* slot, const int32_t* tkeys, const uint64_t* tvals, int32_t* deg2, const Csr* g2,
             hipStream_t s);

}  // namespace louvain
}  // namespace mgp
