// mgp_graph.hip — the kernels of mgp_graph.h: the fused distance and k-smallest selection of
// the kNN graph, and the passes of the shared-nearest-neighbour graph over a kNN table.
#include "mgp_graph.h"

#include <algorithm>

namespace mgp {
namespace graph {

constexpr int kKnnBlock = 256;      // 16 x 16 threads, a 4 x 4 block of pairs each; 4 waves of 16 rows
constexpr int kRowsPerBlock = 4;    // the wave-per-row kernels
constexpr int kScanBlock = 1024;    // the single scan workgroup
constexpr uint64_t kPadDist = ~0ull;  // the key of an empty list entry: above every distance's bits
constexpr int32_t kPadIdx = 0x7fffffff;
#define MGP_INF __builtin_huge_val()

static __device__ __forceinline__ bool finite_f64(double v) { return fabs(v) < MGP_INF; }

// ---------------------------------------------------------------------------
// keys over the lanes of a wave
// ---------------------------------------------------------------------------
static __device__ __forceinline__ bool key_less(uint64_t ad, int32_t aj, uint64_t bd, int32_t bj) {
    return ad < bd || (ad == bd && aj < bj);
}

// one compare-exchange with the lane `stride` away: the smaller key stays when take_min
static __device__ __forceinline__ void key_cx(uint64_t& d, int32_t& j, int stride, bool take_min) {
    const uint64_t od = __shfl_xor((unsigned long long)d, stride, 64);
    const int32_t oj = __shfl_xor(j, stride, 64);
    if (key_less(od, oj, d, j) == take_min) {
        d = od;
        j = oj;
    }
}

// the wave's 64 keys ascending over the lanes (a bitonic network, 21 exchanges)
static __device__ __forceinline__ void wave_sort(uint64_t& d, int32_t& j, int lane) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1)
            key_cx(d, j, stride, ((lane & stride) == 0) == ((lane & size) == 0));
}

// (ld, lj) and (d, j) both ascending over the lanes: (ld, lj) becomes the 64 smallest of the 128,
// ascending. min(L[p], C[63 - p]) holds them as a bitonic sequence; 6 exchanges sort it.
static __device__ __forceinline__ void wave_merge(uint64_t& ld, int32_t& lj, uint64_t d, int32_t j, int lane) {
    const uint64_t rd = __shfl((unsigned long long)d, 63 - lane, 64);
    const int32_t rj = __shfl(j, 63 - lane, 64);
    if (key_less(rd, rj, ld, lj)) {
        ld = rd;
        lj = rj;
    }
#pragma unroll
    for (int stride = 32; stride > 0; stride >>= 1) key_cx(ld, lj, stride, (lane & stride) == 0);
}

// ---------------------------------------------------------------------------
// kNN
// ---------------------------------------------------------------------------
// Workgroup (bi, sp): query items bi*64.., the candidate tiles [sp*per, (sp + 1)*per) of the nt.
// Per tile the distances are made as in k_pair_dist (the same staging, the same chain), left in
// LDS over the staging buffers and offered to the rows, 16 rows a wave, a candidate a lane. A
// row's list is part_*[sp][i][0..k), entry p read and written by lane p alone; thr_* its k-th key.
__global__ void __launch_bounds__(kKnnBlock) k_knn(const double* __restrict__ x, int n, int nf, int k, int nt, int per,
                                                   uint64_t* __restrict__ part_dist, int32_t* __restrict__ part_idx,
                                                   uint32_t* __restrict__ bad) {
    __shared__ double sm[2 * kChunk * kTile];  // A and B [kChunk][kTile]; then D [kTile][kTile]
    __shared__ uint64_t thr_d[kTile];
    __shared__ int32_t thr_j[kTile];
    double* A = sm;
    double* B = sm + kChunk * kTile;
    const int bi = blockIdx.x, sp = blockIdx.y;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, wave = tid >> 6;
    const int i0 = bi * kTile;
    const size_t base = (size_t)sp * (size_t)n * (size_t)k;
    uint64_t* pd = part_dist + base;
    int32_t* pi = part_idx + base;
    if (tid < kTile) {
        thr_d[tid] = kPadDist;
        thr_j[tid] = kPadIdx;
    }
    for (int rr = 0; rr < kTile / 4; ++rr) {
        const int i = i0 + wave * (kTile / 4) + rr;
        if (i < n && lane < k) {
            pd[(size_t)i * k + lane] = kPadDist;
            pi[(size_t)i * k + lane] = kPadIdx;
        }
    }
    __syncthreads();
    bool ok = true;
    const int t_lo = sp * per, t_hi = min(nt, t_lo + per);
    for (int bj = t_lo; bj < t_hi; ++bj) {
        const int j0 = bj * kTile;
        double acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
        for (int k0 = 0; k0 < nf; k0 += kChunk) {
            const int kc = min(kChunk, nf - k0);
            for (int m = tid; m < kc * kTile; m += kKnnBlock) {
                const int kk = m / kTile, c = m % kTile;
                const double* row = x + (size_t)(k0 + kk) * (size_t)n;
                const double a = i0 + c < n ? row[i0 + c] : 0.0;
                const double b = j0 + c < n ? row[j0 + c] : 0.0;
                ok = ok && finite_f64(a) && finite_f64(b);
                A[kk * kTile + c] = a;
                B[kk * kTile + c] = b;
            }
            __syncthreads();
            for (int kk = 0; kk < kc; ++kk) {
                double a[4], b[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) a[r] = A[kk * kTile + ty * 4 + r];
#pragma unroll
                for (int c = 0; c < 4; ++c) b[c] = B[kk * kTile + tx * 4 + c];
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
        // (the staging buffers are free: the last chunk's barrier, or the last tile's, is behind)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) sm[(ty * 4 + r) * kTile + tx * 4 + c] = sqrt(acc[r][c]);
        __syncthreads();
        for (int rr = 0; rr < kTile / 4; ++rr) {
            const int row = wave * (kTile / 4) + rr, i = i0 + row;
            if (i >= n) continue;  // (the same in every lane)
            const int j = j0 + lane;
            uint64_t cd = (uint64_t)__double_as_longlong(sm[row * kTile + lane]);
            int32_t cj = j;
            if (j >= n || j == i) {
                cd = kPadDist;
                cj = kPadIdx;
            }
            if (__ballot(key_less(cd, cj, thr_d[row], thr_j[row])) == 0) continue;
            uint64_t ld = kPadDist;
            int32_t lj = kPadIdx;
            if (lane < k) {
                ld = pd[(size_t)i * k + lane];
                lj = pi[(size_t)i * k + lane];
            }
            wave_sort(cd, cj, lane);
            wave_merge(ld, lj, cd, cj, lane);
            if (lane < k) {
                pd[(size_t)i * k + lane] = ld;
                pi[(size_t)i * k + lane] = lj;
            }
            if (lane == k - 1) {
                thr_d[row] = ld;
                thr_j[row] = lj;
            }
        }
        __syncthreads();
    }
    if (!ok) atomicOr(bad, (uint32_t)BAD_VALUE);
}

// a wave per row: the row's `splits` partial lists (each ascending, the empty entries last) merged
__global__ void __launch_bounds__(64 * kRowsPerBlock) k_knn_merge(const uint64_t* __restrict__ part_dist,
                                                                  const int32_t* __restrict__ part_idx, int n, int k,
                                                                  int splits, double* __restrict__ out_dist,
                                                                  int32_t* __restrict__ out_idx) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n) return;
    uint64_t ld = kPadDist;
    int32_t lj = kPadIdx;
    for (int sp = 0; sp < splits; ++sp) {
        const size_t at = ((size_t)sp * (size_t)n + (size_t)row) * (size_t)k + lane;
        uint64_t cd = kPadDist;
        int32_t cj = kPadIdx;
        if (lane < k) {
            cd = part_dist[at];
            cj = part_idx[at];
        }
        wave_merge(ld, lj, cd, cj, lane);
    }
    if (lane < k) {
        out_dist[(size_t)row * k + lane] = __longlong_as_double((long long)ld);
        out_idx[(size_t)row * k + lane] = lj;
    }
}

// ---------------------------------------------------------------------------
// SNN
// ---------------------------------------------------------------------------
// a wave per row, an entry a lane
__global__ void __launch_bounds__(64 * kRowsPerBlock) k_knn_check(const int32_t* __restrict__ idx, int n, int k,
                                                                  uint32_t* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n) return;
    const int32_t e = lane < k ? idx[(size_t)row * k + lane] : -1;
    bool wrong = lane < k && (e < 0 || e >= n || e == row);
    for (int t = 0; t < k; ++t) {
        const int32_t v = __shfl(e, t, 64);
        wrong = wrong || (lane < k && lane != t && v == e);
    }
    if (wrong) atomicOr(bad, (uint32_t)BAD_TABLE);
}

// a wave per row of a checked table: S_i ascending and the in-degrees
__global__ void __launch_bounds__(64 * kRowsPerBlock) k_snn_sets(const int32_t* __restrict__ idx, int n, int k,
                                                                 int32_t* __restrict__ sets, int32_t* __restrict__ deg) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n) return;
    uint64_t e = lane < k ? (uint64_t)idx[(size_t)row * k + lane] : kPadDist;
    int32_t zero = 0;
    wave_sort(e, zero, lane);
    const bool have = lane < k;  // (the k entries are below the padding)
    const int below = __popcll(__ballot(have && (int64_t)e < row));
    int32_t* out = sets + (size_t)row * (size_t)(k + 1);
    if (have) {
        out[lane + ((int64_t)e > row ? 1 : 0)] = (int32_t)e;
        atomicAdd(&deg[(int32_t)e], 1);
    }
    if (lane == 0) {
        out[below] = row;
        atomicAdd(&deg[row], 1);
    }
}

// one workgroup: thread t sums its run of ceil(n / 1024) values, the 1024 sums are scanned in LDS
__global__ void __launch_bounds__(kScanBlock) k_scan(const int32_t* __restrict__ v, int n, int64_t* __restrict__ off) {
    __shared__ int64_t sh[kScanBlock];
    const int tid = threadIdx.x;
    const int per = (n + kScanBlock - 1) / kScanBlock;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    int64_t sum = 0;
    for (int e = lo; e < hi; ++e) sum += v[e];
    sh[tid] = sum;
    __syncthreads();
    for (int d = 1; d < kScanBlock; d <<= 1) {
        const int64_t t = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    int64_t run = sh[tid] - sum;
    for (int e = lo; e < hi; ++e) {
        off[e] = run;
        run += v[e];
    }
    if (tid == kScanBlock - 1) off[n] = sh[tid];
}

// a thread per entry of the sets: row i joins the reverse list of m
__global__ void __launch_bounds__(256) k_snn_reverse(const int32_t* __restrict__ sets, size_t total, int kk,
                                                     const int64_t* __restrict__ off, int32_t* __restrict__ cur,
                                                     int32_t* __restrict__ rev) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int32_t m = sets[e];
        rev[off[m] + atomicAdd(&cur[m], 1)] = (int32_t)(e / (size_t)kk);
    }
}

// A wave per row i: for each m of S_i, the rows j > i of R(m), a lane each; S_i and S_j are
// intersected in 2K fixed steps and the pair belongs to the m that is their smallest common
// member. eoff == nullptr counts the row's pairs; otherwise they are written from eoff[i] on,
// placed by the ballot's prefix.
__global__ void __launch_bounds__(64 * kRowsPerBlock) k_snn_edges(const int32_t* __restrict__ sets, int n, int kk,
                                                                  const int64_t* __restrict__ off,
                                                                  const int32_t* __restrict__ rev, int min_shared,
                                                                  int32_t* __restrict__ cnt,
                                                                  const int64_t* __restrict__ eoff,
                                                                  int32_t* __restrict__ ei, int32_t* __restrict__ ej,
                                                                  int32_t* __restrict__ es) {
    __shared__ int32_t s_set[kRowsPerBlock][kMaxK + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * kRowsPerBlock + wave;
    const bool live = i < n;
    int32_t* si = s_set[wave];
    for (int a = lane; a < kk; a += 64) si[a] = live ? sets[(size_t)i * kk + a] : 0;
    __syncthreads();
    if (!live) return;
    const int64_t at = eoff ? eoff[i] : 0;
    int32_t run = 0;
    for (int a = 0; a < kk; ++a) {
        const int32_t m = si[a];
        const int64_t lo = off[m], hi = off[m + 1];
        for (int64_t e0 = lo; e0 < hi; e0 += 64) {
            const int64_t e = e0 + lane;
            bool keep = false;
            int32_t j = -1, shared = 0;
            if (e < hi) {
                j = rev[e];
                if (j > i) {
                    const int32_t* sj = sets + (size_t)j * kk;
                    int pa = 0, pb = 0;
                    int32_t first = -1;
                    for (int t = 0; t < 2 * kk; ++t) {
                        if (pa < kk && pb < kk) {
                            const int32_t va = si[pa], vb = sj[pb];
                            if (va == vb && shared == 0) first = va;
                            shared += va == vb;
                            pa += va <= vb;
                            pb += vb <= va;
                        }
                    }
                    keep = first == m && shared >= min_shared;
                }
            }
            const uint64_t mask = __ballot(keep);
            if (eoff && keep) {
                const int64_t p = at + run + __popcll(mask & (((uint64_t)1 << lane) - 1));
                ei[p] = i;
                ej[p] = j;
                es[p] = shared;
            }
            run += __popcll(mask);
        }
    }
    if (!eoff && lane == 0) cnt[i] = run;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
static int launch_ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }
static unsigned row_blocks(int n) { return (unsigned)((n + kRowsPerBlock - 1) / kRowsPerBlock); }

int knn_splits(int n, int want) {
    const int nt = std::max(1, (n + kTile - 1) / kTile);
    if (want > 0) return std::min(want, nt);
    // 8 x 256 workgroups: two rounds of the 4 that fit a compute unit, on the 256 of the device
    // this was written for (measured: DESIGN 7.8; fewer leave units idle, more only add merges)
    return std::max(1, std::min({(2048 + nt - 1) / nt, nt, 64}));
}

int knn(const double* x, int n, int nf, int k, int splits, double* part_dist, int32_t* part_idx, double* out_dist,
        int32_t* out_idx, uint32_t* bad, hipStream_t s) {
    if (n <= 0) return 0;
    const int nt = (n + kTile - 1) / kTile;
    const int per = (nt + splits - 1) / splits;
    uint64_t* pd = reinterpret_cast<uint64_t*>(part_dist);
    k_knn<<<dim3((unsigned)nt, (unsigned)splits), kKnnBlock, 0, s>>>(x, n, nf, k, nt, per, pd, part_idx, bad);
    if (launch_ok() != 0) return -1;
    k_knn_merge<<<row_blocks(n), 64 * kRowsPerBlock, 0, s>>>(pd, part_idx, n, k, splits, out_dist, out_idx);
    return launch_ok();
}

int knn_check(const int32_t* idx, int n, int k, uint32_t* bad, hipStream_t s) {
    if (n <= 0) return 0;
    k_knn_check<<<row_blocks(n), 64 * kRowsPerBlock, 0, s>>>(idx, n, k, bad);
    return launch_ok();
}

int snn_sets(const int32_t* idx, int n, int k, int32_t* sets, int32_t* deg, hipStream_t s) {
    if (n <= 0) return 0;
    if (hipMemsetAsync(deg, 0, (size_t)n * 4, s) != hipSuccess) return -1;
    k_snn_sets<<<row_blocks(n), 64 * kRowsPerBlock, 0, s>>>(idx, n, k, sets, deg);
    return launch_ok();
}

int scan(const int32_t* v, int n, int64_t* off, hipStream_t s) {
    k_scan<<<1, kScanBlock, 0, s>>>(v, std::max(n, 0), off);
    return launch_ok();
}

int snn_reverse(const int32_t* sets, int n, int k, const int64_t* off, int32_t* cur, int32_t* rev, hipStream_t s) {
    if (n <= 0) return 0;
    if (hipMemsetAsync(cur, 0, (size_t)n * 4, s) != hipSuccess) return -1;
    const size_t total = (size_t)n * (size_t)(k + 1);
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 1u << 16);
    k_snn_reverse<<<blocks, 256, 0, s>>>(sets, total, k + 1, off, cur, rev);
    return launch_ok();
}

int snn_edges(const int32_t* sets, int n, int k, const int64_t* off, const int32_t* rev, int min_shared,
              int32_t* cnt, const int64_t* eoff, int32_t* ei, int32_t* ej, int32_t* es, hipStream_t s) {
    if (n <= 0) return 0;
    k_snn_edges<<<row_blocks(n), 64 * kRowsPerBlock, 0, s>>>(sets, n, k + 1, off, rev, min_shared, cnt, eoff, ei, ej,
                                                              es);
    return launch_ok();
}

}  // namespace graph
}  // namespace mgp
