// mgp_qc.hip — coverage QC from the count rows in HBM (gfx950, wave64). See mgp_qc.h for
// what is computed, the exactness bound and why the results are order-free.
//
//   k_cell_stats  one workgroup per population cell. The cell's L depths (33 KB of u16 at
//                 chrM) are read once from HBM; the select's rounds read them again from
//                 the caches (a cell of 2^16 positions of u32 would not fit the LDS, so the
//                 rows are not staged there). Radix select from the highest byte the
//                 cell's max makes necessary: one 256-bin LDS histogram per round.
//   k_pos_stats   the sweep of mgp_sweep.h (one position per lane, cell slabs on grid.y),
//                 with the Tn5 planes loaded next to the counts.
//   k_pos_hist    a workgroup owns 64 positions with an LDS histogram [64][257] (the odd
//                 row stride puts the 64 lanes' equal bins on different banks); its 4 waves
//                 take the slab's cells in turn, 4 cells in flight each.
//   k_pos_next    the same shape, two registers per lane instead of the histogram.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mgp_qc.h"

namespace mgp {
namespace qc {

using sweep_detail::Cnt;
using sweep_detail::depth_at;
using sweep_detail::kBlock;
using sweep_detail::sweep;
using txtgz::Rows;
using variants::kMaxCount;

constexpr int kTargetGroups = 1024;  // ~4 workgroups per CU (k_pos_stats)
constexpr int kHistPos = 64;         // positions of a k_pos_hist / k_pos_next workgroup (one per lane)
constexpr int kHistStride = 257;     // words of a position's LDS histogram row (odd: see above)
constexpr int kHistWaves = kBlock / 64;
constexpr int kHistFlight = 4;       // cells in flight per wave
constexpr int kHistTargetGroups = 2048;

// ---- per cell ------------------------------------------------------------------------

// One more of `bin` in the workgroup's histogram for every lane that is `on`. Depths repeat
// (zeros above all): the bin of the wave's first lane is counted once for all its lanes.
__device__ __forceinline__ void hist_add(uint32_t* h, bool on, uint32_t bin) {
    const unsigned long long act = __ballot(on);
    if (!act) return;
    const int lane = (int)(threadIdx.x & 63u), first = __ffsll((long long)act) - 1;
    const uint32_t b0 = (uint32_t)__shfl((int)bin, first);
    const unsigned long long same = __ballot(on && bin == b0);
    if (lane == first)
        atomicAdd(&h[b0], (uint32_t)__popcll(same));
    else if (on && bin != b0)
        atomicAdd(&h[bin], 1u);
}

__global__ void __launch_bounds__(kBlock) k_cell_stats(Rows R, const int32_t* __restrict__ cells, int64_t n,
                                                       unsigned long long* __restrict__ out64,
                                                       uint32_t* __restrict__ out32, uint32_t* __restrict__ bad) {
    __shared__ unsigned long long s64[CELL64_N];
    __shared__ uint32_t s32[CELL32_N];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sel[3];  // the round's bin, the elements of the prefix below it, the bin's count
    const int64_t k = blockIdx.x;
    const int tid = (int)threadIdx.x;
    const int c = cells ? cells[k] : (int)k;
    unsigned long long* o64 = out64 + k * CELL64_N;
    uint32_t* o32 = out32 + k * CELL32_N;
    if (c < 0) {  // an all-zero row
        if (tid < CELL64_N) o64[tid] = 0;
        if (tid < CELL32_N) o32[tid] = 0;
        return;
    }
    if (tid < CELL64_N) s64[tid] = 0;
    if (tid < CELL32_N) s32[tid] = 0;
    __syncthreads();
    const int L = R.L;
    {
        unsigned long long sd = 0, sd2 = 0;
        uint32_t mx = 0, npos = 0, n10 = 0, n50 = 0;
        for (int p = tid; p < L; p += kBlock) {
            const uint32_t d = depth_at(R, c, p);
            sd += d;
            sd2 += (unsigned long long)d * d;
            mx = max(mx, d);
            npos += d > 0;
            n10 += d >= 10;
            n50 += d >= 50;
        }
        if (sd) {
            atomicAdd(&s64[CELL64_SD], sd);
            atomicAdd(&s64[CELL64_SD2], sd2);
            atomicMax(&s32[CELL32_MAX], mx);
            atomicAdd(&s32[CELL32_NPOS], npos);
            if (n10) atomicAdd(&s32[CELL32_N10], n10);
            if (n50) atomicAdd(&s32[CELL32_N50], n50);
        }
    }
    __syncthreads();
    const uint32_t mx = s32[CELL32_MAX];
    // the lower middle (rank (L - 1) / 2 of the L depths, zeros included), byte by byte
    uint32_t prefix = 0, rank = (uint32_t)(L - 1) / 2, below = 0, at = 0;
    for (int shift = mx >> 24 ? 24 : mx >> 16 ? 16 : mx >> 8 ? 8 : 0; shift >= 0; shift -= 8) {
        hist[tid] = 0;  // (kBlock == 256)
        __syncthreads();
        for (int p0 = 0; p0 < L; p0 += kBlock) {  // (whole waves reach hist_add)
            const int p = p0 + tid;
            const uint32_t d = p < L ? depth_at(R, c, p) : 0u;
            const bool on = p < L && (shift == 24 || (d >> (shift + 8)) == prefix);
            hist_add(hist, on, (d >> shift) & 255u);
        }
        __syncthreads();
        if (tid < 64) {  // wave 0: 4 bins per lane, a scan over the lanes, the bin that holds the rank
            uint32_t h[4], t = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) t += h[j] = hist[4 * tid + j];
            uint32_t inc = t;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = (uint32_t)__shfl_up((int)inc, o);
                if (tid >= o) inc += v;
            }
            uint32_t cum = inc - t;
            if (cum <= rank && rank < inc) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (rank >= cum && rank < cum + h[j]) {
                        sel[0] = 4 * tid + j;
                        sel[1] = cum;
                        sel[2] = h[j];
                    }
                    cum += h[j];
                }
            }
        }
        __syncthreads();
        prefix = prefix << 8 | sel[0];
        rank -= sel[1];
        below += sel[1];
        at = sel[2];
        __syncthreads();  // (sel and hist are free for the next round)
    }
    const uint32_t lo = prefix;
    uint32_t hi = lo;
    if ((uint64_t)below + at <= (uint32_t)L / 2) {  // the upper middle is the next larger depth
        if (tid == 0) sel[0] = 0xFFFFFFFFu;
        __syncthreads();
        uint32_t nx = 0xFFFFFFFFu;
        for (int p = tid; p < L; p += kBlock) {
            const uint32_t d = depth_at(R, c, p);
            if (d > lo) nx = min(nx, d);
        }
        if (nx != 0xFFFFFFFFu) atomicMin(&sel[0], nx);
        __syncthreads();
        hi = sel[0];
    }
    if (tid < CELL64_N) o64[tid] = s64[tid];
    if (tid < CELL32_MIDLO) o32[tid] = s32[tid];
    if (tid == 0) {
        o32[CELL32_MIDLO] = lo;
        o32[CELL32_MIDHI] = hi;
        if (mx >= kMaxCount) atomicOr(bad, 1u);
    }
}

// ---- per position: the sums ------------------------------------------------------------

struct PosAcc {
    unsigned long long sd = 0, sd2 = 0, fwd = 0, rev = 0, tf = 0, tr = 0, tal[4] = {0, 0, 0, 0};
    uint32_t npos = 0, n10 = 0, n50 = 0, ntn5 = 0, mx = 0, big = 0;
    __device__ __forceinline__ void cell(const Cnt& x, uint32_t t_f, uint32_t t_r) {
        const uint32_t d = x.cov;
        sd += d;
        sd2 += (unsigned long long)d * d;
        mx = max(mx, d);
        npos += d > 0;
        n10 += d >= 10;
        n50 += d >= 50;
        big |= d;
        uint32_t f = 0, r = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            big |= x.f[b] | x.r[b];
            f += x.f[b];  // (four counts below 2^24, checked through big)
            r += x.r[b];
            tal[b] += (unsigned long long)x.f[b] + x.r[b];
        }
        fwd += f;
        rev += r;
        tf += t_f;
        tr += t_r;
        ntn5 += (t_f | t_r) != 0;
    }
};

__device__ __forceinline__ void add64(unsigned long long* a, unsigned long long v) {
    if (v) atomicAdd(a, v);
}
__device__ __forceinline__ void add32(uint32_t* a, uint32_t v) {
    if (v) atomicAdd(a, v);
}

__global__ void __launch_bounds__(kBlock) k_pos_stats(Rows R, Tn5 T, const int32_t* __restrict__ cells, int64_t n,
                                                      int64_t slab, unsigned long long* __restrict__ acc64,
                                                      uint32_t* __restrict__ acc32, uint32_t* __restrict__ bad) {
    PosAcc a;
    const int64_t k0 = (int64_t)blockIdx.y * slab, k1 = min(n, k0 + slab);
    sweep<true>(R, cells, k0, k1, a, T);
    const int p = blockIdx.x * kBlock + (int)threadIdx.x;
    if (p >= R.L) return;
    const size_t L = (size_t)R.L;
    add64(acc64 + POS64_SD * L + p, a.sd);
    add64(acc64 + POS64_SD2 * L + p, a.sd2);
    add64(acc64 + POS64_FWD * L + p, a.fwd);
    add64(acc64 + POS64_REV * L + p, a.rev);
    add64(acc64 + POS64_TF * L + p, a.tf);
    add64(acc64 + POS64_TR * L + p, a.tr);
#pragma unroll
    for (int b = 0; b < 4; ++b) add64(acc64 + POS64_TALLY * L + (size_t)p * 4 + b, a.tal[b]);
    add32(acc32 + POS32_NPOS * L + p, a.npos);
    add32(acc32 + POS32_N10 * L + p, a.n10);
    add32(acc32 + POS32_N50 * L + p, a.n50);
    add32(acc32 + POS32_NTN5 * L + p, a.ntn5);
    if (a.mx) atomicMax(acc32 + POS32_MAX * L + p, a.mx);
    if (a.big >= kMaxCount) atomicOr(bad, 1u);
}

// ---- per position: the median's two primitives -----------------------------------------

// fn(d) for the depth at position p of the cells [k0, k1) this wave takes: the workgroup's
// waves take groups of kHistFlight consecutive cells in turn
template <class Fn>
__device__ __forceinline__ void depth_cells(const Rows& R, const int32_t* __restrict__ cells, int64_t k0, int64_t k1,
                                            int p, bool active, Fn fn) {
    const int wave = (int)(threadIdx.x >> 6);
    for (int64_t k = k0 + wave * kHistFlight; k < k1; k += kHistWaves * kHistFlight) {
        uint32_t d[kHistFlight];
#pragma unroll
        for (int j = 0; j < kHistFlight; ++j) {
            const bool on = active && k + j < k1;
            const int c = on ? (cells ? cells[k + j] : (int)(k + j)) : -1;
            d[j] = depth_at(R, c, p);
        }
#pragma unroll
        for (int j = 0; j < kHistFlight; ++j)
            if (active && k + j < k1) fn(d[j]);
    }
}

__global__ void __launch_bounds__(kBlock) k_pos_hist(Rows R, const int32_t* __restrict__ cells, int64_t n, int64_t slab,
                                                     int shift, const uint32_t* __restrict__ prefix,
                                                     uint32_t* __restrict__ hist) {
    extern __shared__ uint32_t lh[];  // [kHistPos][kHistStride]
    const int tid = (int)threadIdx.x, lane = tid & 63;
    for (int i = tid; i < kHistPos * kHistStride; i += kBlock) lh[i] = 0;
    __syncthreads();
    const int p0 = blockIdx.x * kHistPos, p = p0 + lane;
    const bool active = p < R.L;
    const uint32_t pre = (active && shift < 24) ? prefix[p] : 0u;
    const int64_t k0 = (int64_t)blockIdx.y * slab, k1 = min(n, k0 + slab);
    uint32_t* row = lh + lane * kHistStride;
    depth_cells(R, cells, k0, k1, p, active, [&](uint32_t d) {
        if (shift == 24 || (d >> (shift + 8)) == pre) atomicAdd(&row[(d >> shift) & 255u], 1u);
    });
    __syncthreads();
    for (int i = tid; i < kHistPos * 256; i += kBlock) {
        const int q = i >> 8, b = i & 255;
        const uint32_t v = lh[q * kHistStride + b];
        if (v && p0 + q < R.L) atomicAdd(&hist[(size_t)(p0 + q) * 256 + b], v);
    }
}

__global__ void __launch_bounds__(kBlock) k_pos_next(Rows R, const int32_t* __restrict__ cells, int64_t n, int64_t slab,
                                                     const uint32_t* __restrict__ v, uint32_t* __restrict__ n_le,
                                                     uint32_t* __restrict__ next) {
    const int p = blockIdx.x * kHistPos + (int)(threadIdx.x & 63u);
    const bool active = p < R.L;
    const uint32_t at = active ? v[p] : 0u;
    const int64_t k0 = (int64_t)blockIdx.y * slab, k1 = min(n, k0 + slab);
    uint32_t le = 0, nx = 0xFFFFFFFFu;
    depth_cells(R, cells, k0, k1, p, active, [&](uint32_t d) {
        le += d <= at;
        if (d > at) nx = min(nx, d);
    });
    if (!active) return;
    if (le) atomicAdd(&n_le[p], le);
    if (nx != 0xFFFFFFFFu) atomicMin(&next[p], nx);
}

// ---- launches ------------------------------------------------------------------------

static int launch_ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

// cells of a slab: `groups` workgroups over gx position blocks, at least `least` cells each
static int64_t slab_cells(int64_t n, int gx, int groups, int least) {
    n = std::max<int64_t>(n, 1);
    const int64_t want = std::max<int64_t>(1, groups / gx);
    const int64_t ns = std::max<int64_t>(1, std::min<int64_t>(want, (n + least - 1) / least));
    return (n + ns - 1) / ns;
}

int cell_stats(const Rows& rows, const int32_t* cells, int64_t n, unsigned long long* out64, uint32_t* out32,
               uint32_t* bad, hipStream_t s) {
    if (hipMemsetAsync(bad, 0, 4, s) != hipSuccess) return -1;
    if (n <= 0) return 0;
    k_cell_stats<<<(unsigned)n, kBlock, 0, s>>>(rows, cells, n, out64, out32, bad);
    return launch_ok();
}

int pos_stats(const Rows& rows, const Tn5& tn5, const int32_t* cells, int64_t n, unsigned long long* acc64,
              uint32_t* acc32, uint32_t* bad, hipStream_t s) {
    const int L = rows.L;
    if (hipMemsetAsync(acc64, 0, (size_t)POS64_N * L * 8, s) != hipSuccess) return -1;
    if (hipMemsetAsync(acc32, 0, (size_t)POS32_N * L * 4, s) != hipSuccess) return -1;
    if (hipMemsetAsync(bad, 0, 4, s) != hipSuccess) return -1;
    if (n <= 0) return 0;
    const int gx = (L + kBlock - 1) / kBlock;
    const int64_t slab = slab_cells(n, gx, kTargetGroups, 32);
    const dim3 grid(gx, (unsigned)((n + slab - 1) / slab));
    k_pos_stats<<<grid, kBlock, 0, s>>>(rows, tn5, cells, n, slab, acc64, acc32, bad);
    return launch_ok();
}

int pos_depth_hist(const Rows& rows, const int32_t* cells, int64_t n, int shift, const uint32_t* prefix, uint32_t* hist,
                   hipStream_t s) {
    const int L = rows.L;
    if (hipMemsetAsync(hist, 0, (size_t)L * 256 * 4, s) != hipSuccess) return -1;
    if (n <= 0) return 0;
    constexpr size_t lds = (size_t)kHistPos * kHistStride * 4;  // 65,792 B: above the 64 KiB a launch gets unasked
    if (hipFuncSetAttribute((const void*)k_pos_hist, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -1;
    const int gx = (L + kHistPos - 1) / kHistPos;
    const int64_t slab = slab_cells(n, gx, kHistTargetGroups, 64);
    const dim3 grid(gx, (unsigned)((n + slab - 1) / slab));
    k_pos_hist<<<grid, kBlock, lds, s>>>(rows, cells, n, slab, shift, prefix, hist);
    return launch_ok();
}

int pos_depth_next(const Rows& rows, const int32_t* cells, int64_t n, const uint32_t* v, uint32_t* n_le, uint32_t* next,
                   hipStream_t s) {
    const int L = rows.L;
    if (hipMemsetAsync(n_le, 0, (size_t)L * 4, s) != hipSuccess) return -1;
    if (hipMemsetAsync(next, 0xFF, (size_t)L * 4, s) != hipSuccess) return -1;
    if (n <= 0) return 0;
    const int gx = (L + kHistPos - 1) / kHistPos;
    const int64_t slab = slab_cells(n, gx, kHistTargetGroups, 64);
    const dim3 grid(gx, (unsigned)((n + slab - 1) / slab));
    k_pos_next<<<grid, kBlock, 0, s>>>(rows, cells, n, slab, v, n_le, next);
    return launch_ok();
}

}  // namespace qc
}  // namespace mgp
