// mgp_groups.hip — pseudobulk counts per cell group from the count rows in HBM (gfx950,
// wave64). See mgp_groups.h for what is computed, the exactness bound and the determinism.
//
// One position per lane and kBlock positions per workgroup, as the other sweeps over cells
// (mgp_sweep.h). grid.x = position blocks, grid.y = items, strided where a call has more
// items than grid.y holds. A thread keeps its position's sums of one item in registers and
// flushes them once per item. The outputs are [group][position][base], so a thread's four
// bases are 32 (u64) or 16 (u32) contiguous bytes and a wave's flush of one base would touch
// 64 separate 8-byte words: the workgroup turns each field through LDS instead, so that every
// store or atomic wave-instruction covers 512 (u64) or 256 (u32) contiguous bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mgp_groups.h"
#include "mgp_sweep.h"
#include "mgp_variants.h"

namespace mgp {
namespace groups {

using sweep_detail::Cnt;
using sweep_detail::kBlock;
using sweep_detail::sweep;
using txtgz::Rows;
using variants::kMaxCount;

constexpr int kTargetGroups = 1024;  // ~4 workgroups per CU, as mgp_variants.hip
constexpr int kMaxGridY = 65535;

struct GroupAcc {
    unsigned long long fwd[4] = {0, 0, 0, 0}, rev[4] = {0, 0, 0, 0}, cov = 0;
    uint32_t n_det[4] = {0, 0, 0, 0}, n_conf[4] = {0, 0, 0, 0}, big = 0;
    __device__ __forceinline__ void cell(const Cnt& x) {
        cov += x.cov;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t f = x.f[b], r = x.r[b];
            big |= f | r;
            fwd[b] += f;
            rev[b] += r;
            n_det[b] += (f + r) != 0;
            n_conf[b] += (f >= 2 && r >= 2);
        }
    }
};

// One field of the workgroup's positions [p0, p0 + kBlock) x 4 bases, contiguous in `out`
// from word p0 * 4: v[b] of every thread goes through `stage` so that consecutive lanes
// write consecutive words. count = the words of this block that exist (positions below L).
template <class T>
__device__ __forceinline__ void flush4(T* __restrict__ out, T* stage, const T (&v)[4], int count, bool excl) {
    __syncthreads();  // (the previous field's readers are done)
#pragma unroll
    for (int b = 0; b < 4; ++b) stage[threadIdx.x * 4 + b] = v[b];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = j * kBlock + (int)threadIdx.x;
        if (i >= count) continue;
        const T x = stage[i];
        if (excl)
            out[i] = x;
        else if (x)
            atomicAdd(out + i, x);
    }
}

__global__ void __launch_bounds__(kBlock) k_groups(Rows R, const int32_t* __restrict__ cells,
                                                   const Item* __restrict__ items, int64_t n_items, Acc acc,
                                                   uint32_t* __restrict__ bad) {
    __shared__ unsigned long long stage[kBlock * 4];
    const int p0 = blockIdx.x * kBlock, p = p0 + (int)threadIdx.x;
    const int count = min(kBlock, R.L - p0) * 4;
    uint32_t big = 0;
    for (int64_t it = blockIdx.y; it < n_items; it += gridDim.y) {
        const Item item = items[it];
        GroupAcc a;
        sweep(R, cells, item.k0, item.k1, a);
        big |= a.big;
        const bool excl = item.excl != 0;
        const size_t row = (size_t)item.g * R.L + p0;  // this block's first (group, position)
        flush4(acc.fwd + row * 4, stage, a.fwd, count, excl);
        flush4(acc.rev + row * 4, stage, a.rev, count, excl);
        flush4(acc.n_det + row * 4, reinterpret_cast<uint32_t*>(stage), a.n_det, count, excl);
        flush4(acc.n_conf + row * 4, reinterpret_cast<uint32_t*>(stage), a.n_conf, count, excl);
        if (p < R.L) {
            if (excl)
                acc.cov[row + threadIdx.x] = a.cov;
            else if (a.cov)
                atomicAdd(acc.cov + row + threadIdx.x, a.cov);
        }
    }
    if (big >= kMaxCount) atomicOr(bad, 1u);
}

int64_t item_cells(int64_t n, int L) {
    n = std::max<int64_t>(n, 1);
    const int gx = (L + kBlock - 1) / kBlock;
    const int64_t want = std::max<int64_t>(1, kTargetGroups / gx);
    const int64_t ns = std::max<int64_t>(1, std::min<int64_t>(want, (n + 31) / 32));
    return (n + ns - 1) / ns;
}

int moments(const Rows& rows, const int32_t* cells, const Item* items, int64_t n_items, const Acc& acc, uint32_t* bad,
            hipStream_t s) {
    const dim3 grid((rows.L + kBlock - 1) / kBlock, (unsigned)std::min<int64_t>(n_items, kMaxGridY));
    k_groups<<<grid, kBlock, 0, s>>>(rows, cells, items, n_items, acc, bad);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace groups
}  // namespace mgp
