// mgp_groups.h — pseudobulk counts per cell group on the device (internal interface between
// mgp_jobs.hip and mgp_groups.hip; the C-ABI is mgp_group_moments_run / mgp_rows_group_moments
// in include/mgpileup.h).
//
// Every cell of a population carries a group label; per group g, position p and base b the
// sweep returns the sums of the cells' fwd and rev counts and of their filtered depth, and the
// cells with fwd + rev > 0 and with fwd >= 2 and rev >= 2: the evidence for a group's private
// variants at all (position, base) pairs, which the population-wide variant filter drops by
// construction when the group is small. One launch covers every group of a call: the host
// sorts the population by group and cuts each group's run into items of consecutive entries;
// a workgroup takes one (position block, item) and sweeps it with sweep() of mgp_sweep.h.
//
// Exactness, as mgp_variants.h: at most kMaxCells cells per call and every fwd / rev count
// below kMaxCount, so every sum stays below 2^40 (the depth sums below 2^48). A count at or
// above kMaxCount is reported through `bad`.
//
// Determinism. Integer adds only: the result does not depend on the item size, the items'
// order or the sort. An item that is its group's only one owns its output words and stores
// them plainly; the others add atomically into words the driver zeroed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mgpileup.h"
#include "mgp_txtgz.h"

namespace mgp {
namespace groups {

constexpr int kMaxGroups = MGP_GROUP_MAX_GROUPS;

// entries [k0, k1) of the sorted population belong to group g; excl: g's only item
struct Item {
    int32_t k0, k1, g, excl;
};

// One call's accumulators, [G] groups each: 104 bytes per (group, position)
struct Acc {
    unsigned long long *fwd, *rev;  // [G][L][4]
    unsigned long long* cov;        // [G][L]
    uint32_t *n_det, *n_conf;       // [G][L][4]
};
inline size_t acc_bytes(int G, int L) { return (size_t)G * (size_t)L * 104; }
// the planes of a buffer of acc_bytes(G, L)
inline Acc acc_of(void* base, int G, int L) {
    const size_t gl = (size_t)G * (size_t)L;
    unsigned long long* q = static_cast<unsigned long long*>(base);
    uint32_t* w = reinterpret_cast<uint32_t*>(q + gl * 9);
    return Acc{q, q + gl * 4, q + gl * 8, w, w + gl * 4};
}

// cells of an item when the caller sets none: n labelled entries in all fill the device with
// at least 32 cells each (the slabs of mgp_variants.hip), never across a group boundary
int64_t item_cells(int64_t n, int L);

// cells: device list of row indices sorted by group (-1: an all-zero row). items: device,
// n_items of them (> 0). acc: zeroed by the caller. bad: one word, zeroed by the caller, set
// nonzero when a count reaches kMaxCount.
int moments(const txtgz::Rows& rows, const int32_t* cells, const Item* items, int64_t n_items, const Acc& acc,
            uint32_t* bad, hipStream_t s);

}  // namespace groups
}  // namespace mgp
