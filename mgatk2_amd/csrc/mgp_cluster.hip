// mgp_cluster.hip — the kernels of mgp_cluster.h: tiled Euclidean pair distances in fp64
// and the single-workgroup complete linkage over the matrix in HBM.
#include "mgp_cluster.h"

#include <algorithm>
#include <cmath>

namespace mgp {
namespace cluster {

constexpr int kPairBlock = 256;  // 16 x 16 threads, a 4 x 4 block of pairs each
constexpr int kRowsPerBlock = 4; // k_nn_init: one wave per row
#define MGP_INF __builtin_huge_val()

static __device__ __forceinline__ bool finite_f64(double v) { return fabs(v) < MGP_INF; }

// ---------------------------------------------------------------------------
// pair distances
// ---------------------------------------------------------------------------
// One workgroup per 64 x 64 tile (bi, bj) with bj >= bi; the tiles below the diagonal leave
// at once. Per chunk of kChunk features, the tile's two item ranges are staged through LDS
// (coalesced over items); a thread then walks the chunk's features in ascending order for
// its 4 x 4 pairs: rows ty*4.., columns tx*4.., so its LDS reads are two 32-byte runs and
// its stores four 32-byte runs, both ways round.
__global__ void __launch_bounds__(kPairBlock) k_pair_dist(const double* __restrict__ x, int n, int nf,
                                                          double* __restrict__ dist, uint32_t* __restrict__ bad) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;
    __shared__ double A[kChunk][kTile];
    __shared__ double B[kChunk][kTile];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = bi * kTile, j0 = bj * kTile;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    bool ok = true;
    for (int k0 = 0; k0 < nf; k0 += kChunk) {
        const int kc = min(kChunk, nf - k0);
        for (int m = tid; m < kc * kTile; m += kPairBlock) {
            const int kk = m / kTile, c = m % kTile;
            const double* row = x + (size_t)(k0 + kk) * (size_t)n;
            const double a = i0 + c < n ? row[i0 + c] : 0.0;
            const double b = j0 + c < n ? row[j0 + c] : 0.0;
            ok = ok && finite_f64(a) && finite_f64(b);
            A[kk][c] = a;
            B[kk][c] = b;
        }
        __syncthreads();
        for (int kk = 0; kk < kc; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = A[kk][ty * 4 + r];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = B[kk][tx * 4 + c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double d = a[r] - b[c];
                    acc[r][c] = __builtin_fma(d, d, acc[r][c]);
                }
        }
        __syncthreads();
    }
    if (!ok) atomicOr(bad, (uint32_t)BAD_VALUE);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty * 4 + r;
        if (i >= n) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + tx * 4 + c;
            if (j >= n) continue;
            const double v = sqrt(acc[r][c]);
            dist[(size_t)i * n + j] = v;
            if (bi != bj) dist[(size_t)j * n + i] = v;
        }
    }
}

__global__ void __launch_bounds__(256) k_check_dist(const double* __restrict__ dist, int n, uint32_t* __restrict__ bad) {
    const size_t total = (size_t)n * (size_t)n;
    uint32_t f = 0;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t i = idx / (size_t)n, j = idx % (size_t)n;
        const double v = dist[idx];
        if (!(v >= 0.0 && v < MGP_INF)) f |= BAD_VALUE;
        if (j > i && !(v == dist[j * (size_t)n + i])) f |= BAD_ASYMMETRIC;
    }
    if (f) atomicOr(bad, f);
}

// ---------------------------------------------------------------------------
// complete linkage
// ---------------------------------------------------------------------------
// (d, k) of every lane -> the smallest d, ties to the smallest k, in all lanes
static __device__ __forceinline__ void wave_argmin(double& d, int& k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(d, off, 64);
        const int ok = __shfl_xor(k, off, 64);
        if (od < d || (od == d && ok < k)) {
            d = od;
            k = ok;
        }
    }
}

// the same over the workgroup's kLinkBlock threads (16 waves); every thread gets the result
static __device__ __forceinline__ void block_argmin(double& d, int& k, double* s_d, int* s_k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wave_argmin(d, k);
    if (lane == 0) {
        s_d[wave] = d;
        s_k[wave] = k;
    }
    __syncthreads();
    d = s_d[lane & (kLinkBlock / 64 - 1)];
    k = s_k[lane & (kLinkBlock / 64 - 1)];
    wave_argmin(d, k);
    __syncthreads();
}

// row r's list entry, by one wave: the first active k > r at the row's minimum (k = n and
// +inf when no active k > r is left); all lanes get it
static __device__ __forceinline__ void wave_scan_row(const double* dist, const uint8_t* act,
                                                     int n, int r, double& bd, int& bk) {
    const int lane = threadIdx.x & 63;
    const double* row = dist + (size_t)r * (size_t)n;
    bd = MGP_INF;
    bk = n;
#pragma unroll 4
    for (int k = r + 1 + lane; k < n; k += 64) {
        const double d = row[k];
        if (act[k] && d < bd) {  // (k ascending in a lane: strict < keeps its first minimum)
            bd = d;
            bk = k;
        }
    }
    wave_argmin(bd, bk);
}

__global__ void __launch_bounds__(64 * kRowsPerBlock) k_nn_init(const double* __restrict__ dist,
                                                                const uint8_t* __restrict__ act, int n,
                                                                int32_t* __restrict__ nn, double* __restrict__ dnn) {
    const int r = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (r >= n) return;
    double bd;
    int bk;
    wave_scan_row(dist, act, n, r, bd, bk);
    if ((threadIdx.x & 63) == 0) {
        nn[r] = bk;
        dnn[r] = bd;
    }
}

// One workgroup, n - 1 steps. Per step: (1) argmin over dnn, ties to the smallest row; (2) the
// max-update of row and column i over the active k, which also gives row i's new list entry
// and collects the rows whose entry pointed at i or j; (3) those rows scanned again, a wave
// each. Global writes of one phase are read by other waves only after a workgroup barrier.
__global__ void __launch_bounds__(kLinkBlock) k_link(double* dist, int n, int32_t* nn,
                                                     double* dnn, uint8_t* act,
                                                     int32_t* list, int32_t* si,
                                                     int32_t* sj, double* sh) {
    __shared__ double s_d[kLinkBlock / 64];
    __shared__ int s_k[kLinkBlock / 64];
    __shared__ int s_cnt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int step = 0; step < n - 1; ++step) {
        double bd = MGP_INF;
        int bi = n;
        for (int r = tid; r < n; r += kLinkBlock) {
            const double d = dnn[r];
            if (d < bd) {
                bd = d;
                bi = r;
            }
        }
        block_argmin(bd, bi, s_d, s_k);
        const int i = bi;
        const int j = i < n ? nn[i] : n;
        // (always true on a finite matrix: at least two clusters are active)
        const bool ok = i >= 0 && i < n && j > i && j < n;
        if (tid == 0) {
            si[step] = ok ? i : 0;
            sj[step] = ok ? j : 0;
            sh[step] = bd;
            if (ok) {
                act[j] = 0;
                dnn[j] = MGP_INF;
            }
            s_cnt = 0;
        }
        __syncthreads();
        if (!ok) continue;  // (the same in every thread)
        double* ri = dist + (size_t)i * (size_t)n;
        const double* rj = dist + (size_t)j * (size_t)n;
        double md = MGP_INF;
        int mk = n;
        for (int k = tid; k < n; k += kLinkBlock) {
            if (k == i || k == j || !act[k]) continue;
            const double a = ri[k], b = rj[k];
            const double v = a > b ? a : b;
            ri[k] = v;
            dist[(size_t)k * (size_t)n + i] = v;
            if (k > i && v < md) {
                md = v;
                mk = k;
            }
            const int t = nn[k];
            if (t == i || t == j) list[atomicAdd(&s_cnt, 1)] = k;  // (at most n - 2 entries)
        }
        block_argmin(md, mk, s_d, s_k);  // (its barriers also close the update and the list)
        if (tid == 0) {
            nn[i] = mk;
            dnn[i] = md;
        }
        const int cnt = min(s_cnt, n);
        for (int e = wave; e < cnt; e += kLinkBlock / 64) {
            const int r = list[e];
            double d;
            int k;
            wave_scan_row(dist, act, n, r, d, k);
            if (lane == 0) {
                nn[r] = k;
                dnn[r] = d;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
static int launch_ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

int pair_dist(const double* x, int n, int nf, double* dist, uint32_t* bad, hipStream_t s) {
    if (n <= 0) return 0;
    const unsigned nt = (unsigned)((n + kTile - 1) / kTile);
    k_pair_dist<<<dim3(nt, nt), kPairBlock, 0, s>>>(x, n, nf, dist, bad);
    return launch_ok();
}

int check_dist(const double* dist, int n, uint32_t* bad, hipStream_t s) {
    if (n <= 0) return 0;
    const size_t total = (size_t)n * (size_t)n;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 1u << 16);
    k_check_dist<<<blocks, 256, 0, s>>>(dist, n, bad);
    return launch_ok();
}

int linkage(double* dist, int n, int32_t* nn, double* dnn, uint8_t* act, int32_t* list, int32_t* si, int32_t* sj,
            double* sh, hipStream_t s) {
    if (n < 2) return 0;
    if (hipMemsetAsync(act, 1, (size_t)n, s) != hipSuccess) return -1;
    k_nn_init<<<(unsigned)((n + kRowsPerBlock - 1) / kRowsPerBlock), 64 * kRowsPerBlock, 0, s>>>(dist, act, n, nn, dnn);
    if (launch_ok() != 0) return -1;
    k_link<<<1, kLinkBlock, 0, s>>>(dist, n, nn, dnn, act, list, si, sj, sh);
    return launch_ok();
}

}  // namespace cluster
}  // namespace mgp
