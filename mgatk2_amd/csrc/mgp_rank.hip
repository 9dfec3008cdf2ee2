// mgp_rank.hip — the kernels of mgp_rank.h: the rows' keys sorted by a bitonic network (tiles in
// LDS, the wider strides one pass each over the batch), then every group's rank sums and the tie
// term from the sorted rows.
#include "mgp_rank.h"

#include <algorithm>
#include <climits>

namespace mgp {
namespace rank {

constexpr int kSortBlock = 512;   // threads of a tile's workgroup at most: 4 pairs each at 4,096 elements
constexpr int kRankBlock = 256;   // sorted positions a rank workgroup takes at a time, one a thread
constexpr int kRankWaves = kRankBlock / 64;
constexpr uint64_t kPadKey = ~0ull;         // above every finite value's key
constexpr uint64_t kZeroKey = 1ull << 63;   // the key of 0.0; a value > 0 has a key above it
#define MGP_INF __builtin_huge_val()

static_assert(kSpan % kRankBlock == 0, "a span is whole blocks of positions");
static_assert(kMaxTile * 12 <= 48 * 1024, "the tile's keys and payloads fit 48 KiB of LDS");

// ---------------------------------------------------------------------------
// the sort
// ---------------------------------------------------------------------------
// The steps of stage `size` with the strides from, from / 2, .. 1 on a tile of te elements in
// LDS (keys sk, payloads sp; struct of arrays: a wave's 8-byte reads of consecutive pairs cover
// consecutive banks). g0: the tile's first index in its row, which with `size` gives the
// direction. Equal keys are never exchanged.
static __device__ __forceinline__ void lds_steps(uint64_t* sk, uint32_t* sp, int te, int g0, int size, int from) {
    for (int j = from; j > 0; j >>= 1) {
        for (int q = threadIdx.x; q < (te >> 1); q += blockDim.x) {
            const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
            const int l = i | j;
            const bool up = ((g0 + i) & size) == 0;
            const uint64_t a = sk[i], b = sk[l];
            if (up ? a > b : a < b) {
                sk[i] = b;
                sk[l] = a;
                const uint32_t pa = sp[i], pb = sp[l];
                sp[i] = pb;
                sp[l] = pa;
            }
        }
        __syncthreads();
    }
}

// Workgroup (row, tile): the tile's keys made of x and the labels (the padding beyond n), every
// stage up to te run in LDS, the tile stored. te = min(tile, P) elements, P / te tiles a row.
__global__ void __launch_bounds__(kSortBlock) k_sort_tiles(const double* __restrict__ x,
                                                           const int32_t* __restrict__ group, int n, int64_t P, int te,
                                                           int tiles, uint64_t* __restrict__ keys,
                                                           uint32_t* __restrict__ pay, uint32_t* __restrict__ bad) {
    __shared__ uint64_t sk[kMaxTile];
    __shared__ uint32_t sp[kMaxTile];
    const int64_t row = blockIdx.x / (unsigned)tiles;
    const int g0 = (int)(blockIdx.x % (unsigned)tiles) * te;
    const double* xr = x + (size_t)row * (size_t)n;
    bool wrong = false;
    for (int i = threadIdx.x; i < te; i += blockDim.x) {
        const int gi = g0 + i;
        uint64_t k = kPadKey;
        uint32_t p = kPadGroup;
        if (gi < n) {
            const double v = xr[gi] + 0.0;  // -0.0 -> +0.0
            wrong = wrong || !(fabs(v) < MGP_INF);
            const uint64_t b = (uint64_t)__double_as_longlong(v);
            k = (b >> 63) ? ~b : (b | kZeroKey);
            p = (uint32_t)group[gi];
        }
        sk[i] = k;
        sp[i] = p;
    }
    if (wrong) atomicOr(bad, (uint32_t)BAD_VALUE);
    __syncthreads();
    for (int size = 2; size <= te; size <<= 1) lds_steps(sk, sp, te, g0, size, size >> 1);
    const size_t at = (size_t)row * (size_t)P + (size_t)g0;
    for (int i = threadIdx.x; i < te; i += blockDim.x) {
        keys[at + i] = sk[i];
        pay[at + i] = sp[i];
    }
}

// Workgroup (row, tile): the strides te / 2 .. 1 of stage `size` > te, in LDS
__global__ void __launch_bounds__(kSortBlock) k_merge_tiles(uint64_t* __restrict__ keys, uint32_t* __restrict__ pay,
                                                            int64_t P, int te, int tiles, int size) {
    __shared__ uint64_t sk[kMaxTile];
    __shared__ uint32_t sp[kMaxTile];
    const int64_t row = blockIdx.x / (unsigned)tiles;
    const int g0 = (int)(blockIdx.x % (unsigned)tiles) * te;
    const size_t at = (size_t)row * (size_t)P + (size_t)g0;
    for (int i = threadIdx.x; i < te; i += blockDim.x) {
        sk[i] = keys[at + i];
        sp[i] = pay[at + i];
    }
    __syncthreads();
    lds_steps(sk, sp, te, g0, size, te >> 1);
    for (int i = threadIdx.x; i < te; i += blockDim.x) {
        keys[at + i] = sk[i];
        pay[at + i] = sp[i];
    }
}

// A thread per pair of every row of the batch: the compare-exchange of stage `size` at stride j
// (a power of two >= the tile). P = 1 << lg, total = rows * P / 2 pairs.
__global__ void __launch_bounds__(256) k_cx_global(uint64_t* __restrict__ keys, uint32_t* __restrict__ pay, int lg,
                                                   int size, int j, size_t total) {
    const size_t half_mask = ((size_t)1 << (lg - 1)) - 1;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (size_t)gridDim.x * 256) {
        const size_t row = q >> (lg - 1);
        const int qq = (int)(q & half_mask);
        const int i = ((qq & ~(j - 1)) << 1) | (qq & (j - 1));
        const int l = i | j;
        const bool up = (i & size) == 0;
        const size_t at = row << lg;
        const uint64_t a = keys[at + i], b = keys[at + l];
        if (up ? a > b : a < b) {
            keys[at + i] = b;
            keys[at + l] = a;
            const uint32_t pa = pay[at + i], pb = pay[at + l];
            pay[at + i] = pb;
            pay[at + l] = pa;
        }
    }
}

// ---------------------------------------------------------------------------
// the ranks
// ---------------------------------------------------------------------------
// the first index of [0, end) whose key is not below k, in `steps` fixed steps (2^steps > end)
static __device__ __forceinline__ int lower_bound(const uint64_t* __restrict__ rk, int end, uint64_t k, int steps) {
    int lo = 0, hi = end;
    for (int t = 0; t < steps; ++t)
        if (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (rk[mid] < k) lo = mid + 1;
            else hi = mid;
        }
    return lo;
}

// the first index of [from, end) whose key is above k (end when there is none)
static __device__ __forceinline__ int upper_bound(const uint64_t* __restrict__ rk, int from, int end, uint64_t k,
                                                  int steps) {
    int lo = from, hi = end;
    for (int t = 0; t < steps; ++t)
        if (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (rk[mid] <= k) lo = mid + 1;
            else hi = mid;
        }
    return lo;
}

// the maximum of v over the lanes up to this one
static __device__ __forceinline__ int wave_scan_max(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v = max(v, o);
    }
    return v;
}

// the minimum of v over the lanes from this one on
static __device__ __forceinline__ int wave_rscan_min(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_down(v, d, 64);
        if (lane + d < 64) v = min(v, o);
    }
    return v;
}

static __device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
    return v;
}

// Workgroup (row, span): the sorted positions [span * kSpan, min(n, (span + 1) * kSpan)) of the
// row, kRankBlock at a time. Position e of the class lo..hi adds lo + hi + 2 to its group's sum
// and, with a value > 0, 1 to its count; the position at lo adds t^3 - t to the row's tie term.
// in_lds: the table is t_r2 / t_pos, added to the result at the end; otherwise the result itself.
__global__ void __launch_bounds__(kRankBlock) k_rank_sums(const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ pay, int n, int64_t P, int steps,
                                                          int spans, int32_t n_groups, int in_lds,
                                                          uint64_t* __restrict__ r2, uint32_t* __restrict__ pos,
                                                          uint64_t* __restrict__ ties) {
    __shared__ uint64_t t_r2[kLdsGroups];
    __shared__ uint32_t t_pos[kLdsGroups];
    __shared__ uint64_t w_tie[kRankWaves];
    __shared__ int w_lo[kRankWaves], w_hi[kRankWaves];
    __shared__ int s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x / (unsigned)spans;
    const int e0 = (int)(blockIdx.x % (unsigned)spans) * kSpan, e1 = min(n, e0 + kSpan);
    const uint64_t* rk = keys + (size_t)row * (size_t)P;
    const uint32_t* rp = pay + (size_t)row * (size_t)P;
    unsigned long long* out_r2 = reinterpret_cast<unsigned long long*>(r2) + (size_t)row * (size_t)n_groups;
    uint32_t* out_pos = pos + (size_t)row * (size_t)n_groups;
    if (in_lds)
        for (int g = tid; g < n_groups; g += kRankBlock) {
            t_r2[g] = 0;
            t_pos[g] = 0;
        }
    __syncthreads();
    uint64_t tie = 0;
    for (int c0 = e0; c0 < e1; c0 += kRankBlock) {
        const int e = c0 + tid;
        const bool live = e < e1;
        uint64_t k = 0;
        bool start = false, end = false;
        if (live) {
            k = rk[e];
            start = e == 0 || rk[e - 1] != k;
            end = e == n - 1 || rk[e + 1] != k;
        }
        // a class that began before these positions: the last block's (carried), or searched for
        int slo = start ? e : -1;
        if (tid == 0 && !start) slo = c0 > e0 ? s_carry : lower_bound(rk, e, k, steps);
        // one that ends after them (e1 < n then, and the block is full)
        int shi = end ? e : INT_MAX;
        if (tid == kRankBlock - 1 && live && !end) shi = upper_bound(rk, e + 1, n, k, steps) - 1;
        int lo = wave_scan_max(slo, lane), hi = wave_rscan_min(shi, lane);
        if (lane == 63) w_lo[wave] = lo;
        if (lane == 0) w_hi[wave] = hi;
        __syncthreads();
        for (int w = 0; w < kRankWaves; ++w) {
            if (w < wave) lo = max(lo, w_lo[w]);
            if (w > wave) hi = min(hi, w_hi[w]);
        }
        if (tid == kRankBlock - 1) s_carry = lo;
        if (live) {
            const uint32_t g = rp[e];
            if (g < (uint32_t)n_groups) {  // (a padding entry can stand here only beside a value that is not finite)
                const unsigned long long val = (unsigned long long)(lo + hi + 2);
                if (in_lds) {
                    atomicAdd(reinterpret_cast<unsigned long long*>(&t_r2[g]), val);
                    if (k > kZeroKey) atomicAdd(&t_pos[g], 1u);
                } else {
                    atomicAdd(&out_r2[g], val);
                    if (k > kZeroKey) atomicAdd(&out_pos[g], 1u);
                }
            }
            if (start) {
                const uint64_t t = (uint64_t)(hi - lo + 1);
                tie += t * t * t - t;
            }
        }
        __syncthreads();
    }
    tie = wave_sum(tie);
    if (lane == 0) w_tie[wave] = tie;
    __syncthreads();
    if (tid == 0) {
        uint64_t sum = 0;
        for (int w = 0; w < kRankWaves; ++w) sum += w_tie[w];
        if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(ties) + row, (unsigned long long)sum);
    }
    if (in_lds)
        for (int g = tid; g < n_groups; g += kRankBlock) {
            if (t_r2[g]) atomicAdd(&out_r2[g], (unsigned long long)t_r2[g]);
            if (t_pos[g]) atomicAdd(&out_pos[g], t_pos[g]);
        }
}

__global__ void __launch_bounds__(256) k_check_labels(const int32_t* __restrict__ group, int n, int32_t n_groups,
                                                      uint32_t* __restrict__ bad) {
    bool wrong = false;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        wrong = wrong || group[i] < 0 || group[i] >= n_groups;
    if (wrong) atomicOr(bad, (uint32_t)BAD_LABEL);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
static int launch_ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

int64_t padded(int64_t n) {
    int64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

int tile_of(int want) {
    const bool ok = want >= kMinTile && want <= kMaxTile && (want & (want - 1)) == 0;
    return ok ? want : kMaxTile;
}

int64_t batch_features(int64_t n, int64_t n_feat, int32_t n_groups, int64_t want) {
    const int64_t P = padded(n);
    const int64_t per = 8 * n + 12 * P + 12 * (int64_t)n_groups + 8;
    // (a batch asked for stays below 2^28 padded elements: 3 GiB of keys and payloads, a grid below 2^31)
    const int64_t b = want > 0 ? std::min(want, std::max<int64_t>(1, ((int64_t)1 << 28) / P)) : kBudget / per;
    return std::max<int64_t>(1, std::min(b, n_feat));
}

int check_labels(const int32_t* group, int n, int32_t n_groups, uint32_t* bad, hipStream_t s) {
    if (n <= 0) return 0;
    k_check_labels<<<(unsigned)std::min((n + 255) / 256, 1024), 256, 0, s>>>(group, n, n_groups, bad);
    return launch_ok();
}

int sums(const double* x, const int32_t* group, int n, int64_t rows, int32_t n_groups, int tile, uint64_t* keys,
         uint32_t* pay, uint64_t* r2, uint32_t* pos, uint64_t* ties, uint32_t* bad, hipStream_t s) {
    if (n <= 0 || rows <= 0) return 0;
    const int64_t P = padded(n);
    int lg = 0;
    while (((int64_t)1 << lg) < P) ++lg;
    const int te = (int)std::min<int64_t>(tile, P);
    const int tiles = (int)(P / te);
    const size_t cells = (size_t)rows * (size_t)n_groups;
    if (hipMemsetAsync(r2, 0, cells * 8, s) != hipSuccess || hipMemsetAsync(pos, 0, cells * 4, s) != hipSuccess ||
        hipMemsetAsync(ties, 0, (size_t)rows * 8, s) != hipSuccess)
        return -1;
    const unsigned sort_block = (unsigned)std::min(std::max(te / 2, 64), kSortBlock);
    const unsigned sort_grid = (unsigned)(rows * tiles);
    k_sort_tiles<<<sort_grid, sort_block, 0, s>>>(x, group, n, P, te, tiles, keys, pay, bad);
    if (launch_ok() != 0) return -1;
    const size_t pairs = (size_t)rows * (size_t)(P / 2);
    for (int64_t size = 2 * (int64_t)te; size <= P; size <<= 1) {
        for (int64_t j = size >> 1; j >= te; j >>= 1) {
            const unsigned blocks = (unsigned)std::min<size_t>((pairs + 255) / 256, (size_t)1 << 20);
            k_cx_global<<<blocks, 256, 0, s>>>(keys, pay, lg, (int)size, (int)j, pairs);
            if (launch_ok() != 0) return -1;
        }
        k_merge_tiles<<<sort_grid, sort_block, 0, s>>>(keys, pay, P, te, tiles, (int)size);
        if (launch_ok() != 0) return -1;
    }
    const int spans = (n + kSpan - 1) / kSpan;
    k_rank_sums<<<(unsigned)(rows * spans), kRankBlock, 0, s>>>(keys, pay, n, P, lg + 1, spans, n_groups,
                                                                  n_groups <= kLdsGroups ? 1 : 0, r2, pos, ties);
    return launch_ok();
}

}  // namespace rank
}  // namespace mgp
