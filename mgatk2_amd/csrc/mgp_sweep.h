// mgp_sweep.h — the loop over a population's cells at one position per lane, shared by the
// reductions over cells (mgp_variants.hip, mgp_qc.hip). Device code only.
//
// One position per lane, so a wave reads 64 consecutive positions of a cell (1 KB of its
// uint4 rows), and a loop over a slab of the population's cells: grid.x = ceil(L / 256)
// position blocks, grid.y = cell slabs. Every workgroup stages, per chunk of kChunk cells,
// their row indices and the wide flags of the windows its positions touch in LDS (the rows
// are txtgz::Rows: 16-bit rows, with the exact u32 rows where a (cell, window) was drained).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mgp_txtgz.h"

namespace mgp {
namespace sweep_detail {

using txtgz::Rows;

constexpr int kBlock = 256;  // positions per workgroup
constexpr int kChunk = 128;  // cells whose indices and wide flags are staged at once
constexpr int kWB = 4;       // windows a workgroup's positions may touch with staged flags
constexpr int kUnroll = 4;   // rows in flight per thread

// The Tn5 planes that go with a Rows: the 16-bit rows' packed fwd | rev << 16, and the
// exact u32 (fwd, rev) pairs of the drained windows (or of plain u32 rows, t16 == nullptr).
struct Tn5 {
    const uint32_t* t16;  // [cells][L]
    const uint32_t* t32;  // [cells][L][2]
};

struct Cnt {
    uint32_t f[4], r[4], cov;
};

__device__ __forceinline__ bool wide_at(const Rows& r, int c, int win) {
    return r.c16 == nullptr || (r.wide && r.wide[(size_t)c * r.nwin + win]);
}

// the filtered depth of position p of row c (c < 0: 0)
__device__ __forceinline__ uint32_t depth_at(const Rows& r, int c, int p) {
    if (c < 0) return 0u;
    const size_t P = (size_t)c * r.L + p;
    return wide_at(r, c, p / r.W) ? r.d32[P] : (uint32_t)r.d16[P];
}

// the counts of position p of row c (c < 0: zeros); u16: its window has exact 16-bit rows
__device__ __forceinline__ void load_row(const Rows& r, int c, int p, bool u16, Cnt& x) {
    if (c < 0) {
#pragma unroll
        for (int b = 0; b < 4; ++b) x.f[b] = x.r[b] = 0;
        x.cov = 0;
        return;
    }
    const size_t P = (size_t)c * r.L + p;
    if (u16) {
        const uint4 q = r.c16[P];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            x.f[b] = w[b] & 0xFFFFu;
            x.r[b] = w[b] >> 16;
        }
        x.cov = r.d16[P];
    } else {
        const uint4* q = reinterpret_cast<const uint4*>(r.c32 + P * 8);
        const uint4 a = q[0], b2 = q[1];
        x.f[0] = a.x, x.r[0] = a.y, x.f[1] = a.z, x.r[1] = a.w;
        x.f[2] = b2.x, x.r[2] = b2.y, x.f[3] = b2.z, x.r[3] = b2.w;
        x.cov = r.d32[P];
    }
}

// its Tn5 cuts (fwd, rev)
__device__ __forceinline__ uint2 load_tn5(const Rows& r, const Tn5& t, int c, int p, bool u16) {
    if (c < 0) return make_uint2(0u, 0u);
    const size_t P = (size_t)c * r.L + p;
    if (u16) {
        const uint32_t v = t.t16[P];
        return make_uint2(v & 0xFFFFu, v >> 16);
    }
    return reinterpret_cast<const uint2*>(t.t32)[P];
}

// Cells [k0, k1) of the population at this thread's position: acc.cell(x) for each, in
// list order (kUnroll rows loaded ahead of their use); with kTn5, acc.cell(x, tn5 fwd, tn5
// rev). All threads of the workgroup call it.
template <bool kTn5 = false, class Acc>
__device__ __forceinline__ void sweep(const Rows& R, const int32_t* __restrict__ cells, int64_t k0, int64_t k1,
                                      Acc& acc, const Tn5 t = Tn5{nullptr, nullptr}) {
    __shared__ int32_t cs[kChunk + kUnroll];
    __shared__ uint8_t wf[kChunk * kWB];
    const int p0 = blockIdx.x * kBlock, p = p0 + (int)threadIdx.x;
    const bool active = p < R.L;
    const int w0 = p0 / R.W, w1 = min(R.L - 1, p0 + kBlock - 1) / R.W, nwb = w1 - w0 + 1;
    const bool staged = nwb <= kWB;
    const int myw = active ? p / R.W - w0 : 0;
    for (int64_t kc = k0; kc < k1; kc += kChunk) {
        const int m = (int)min((int64_t)kChunk, k1 - kc);
        __syncthreads();  // (the previous chunk's readers are done)
        for (int q = threadIdx.x; q < m + kUnroll; q += kBlock) cs[q] = q < m ? (cells ? cells[kc + q] : (int32_t)(kc + q)) : -1;
        __syncthreads();
        if (staged) {
            for (int q = threadIdx.x; q < m * nwb; q += kBlock) {
                const int i = q / nwb, w = q - i * nwb, c = cs[i];
                wf[i * kWB + w] = (c >= 0 && wide_at(R, c, w0 + w)) ? 1 : 0;
            }
            __syncthreads();
        }
        if (!active) continue;
        for (int i = 0; i < m; i += kUnroll) {
            Cnt x[kUnroll];
            uint2 tn[kUnroll];
#pragma unroll
            for (int j = 0; j < kUnroll; ++j) {
                const int c = cs[i + j];  // (-1 past the chunk's end)
                const bool u16 = c >= 0 && (staged ? !wf[min(i + j, kChunk - 1) * kWB + myw] : !wide_at(R, c, w0 + myw));
                load_row(R, c, p, u16, x[j]);
                if constexpr (kTn5) tn[j] = load_tn5(R, t, c, p, u16);
            }
#pragma unroll
            for (int j = 0; j < kUnroll; ++j) {
                if (i + j >= m) continue;
                if constexpr (kTn5)
                    acc.cell(x[j], tn[j].x, tn[j].y);
                else
                    acc.cell(x[j]);
            }
        }
    }
}

}  // namespace sweep_detail
}  // namespace mgp
