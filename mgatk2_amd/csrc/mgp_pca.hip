// mgp_pca.hip — the kernels of mgp_pca.h: slab sums, centring and scaling, the tiled covariance,
// the round-robin Jacobi step over A and V in HBM, the ordered eigenvectors and the scores. All in
// vector fp64: the results are defined as chains of single operations (mgp_pca.h), so nothing here
// may be contracted by the compiler; every fma is spelled out.
#include "mgp_pca.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace mgp {
namespace pca {

constexpr int kChunk = 32;     // items staged through LDS at a time (slab sums and covariance)
constexpr int kSumFeat = 64;   // features of a k_slab_sums workgroup
constexpr int kJTile = 16;     // k_jacobi_step: a 16 x 16 tile of A and of V a workgroup
constexpr int kScoreComp = 8;  // k_scores: components of a workgroup
constexpr int kScoreFeat = 256;  // k_scores: loadings staged through LDS at a time (per component)
#define MGP_INF __builtin_huge_val()

static __device__ __forceinline__ bool finite_f64(double v) { return fabs(v) < MGP_INF; }

// ---------------------------------------------------------------------------
// means and variances
// ---------------------------------------------------------------------------
// grid (S, ceil(m / 64)). tile[f][c]: a row is 33 doubles, so the 64 chain threads (the wave's
// two halves of 32 lanes are served apart) read 32 distinct bank pairs.
__global__ void __launch_bounds__(256) k_slab_sums(const double* __restrict__ x, const double* __restrict__ mean, int n,
                                                   int m, double* __restrict__ part, uint32_t* __restrict__ bad) {
    __shared__ double tile[kSumFeat][kChunk + 1];
    const int tid = threadIdx.x, slab = blockIdx.x, f0 = blockIdx.y * kSumFeat;
    const int i_lo = slab * kSlab, i_hi = min(n, i_lo + kSlab);
    const double mu = (mean && tid < kSumFeat && f0 + tid < m) ? mean[f0 + tid] : 0.0;
    double sum = 0.0;
    bool ok = true;
    for (int i0 = i_lo; i0 < i_hi; i0 += kChunk) {
        for (int e = tid; e < kSumFeat * kChunk; e += 256) {
            const int r = e / kChunk, c = e % kChunk;
            double v = 0.0;
            if (f0 + r < m && i0 + c < i_hi) v = x[(size_t)(f0 + r) * (size_t)n + (size_t)(i0 + c)];
            ok = ok && finite_f64(v);
            tile[r][c] = v;
        }
        __syncthreads();
        if (tid < kSumFeat) {
            const int lim = min(kChunk, i_hi - i0);
            if (mean) {
                for (int c = 0; c < lim; ++c) {
                    const double d = tile[tid][c] - mu;
                    sum = __builtin_fma(d, d, sum);
                }
            } else {
                for (int c = 0; c < lim; ++c) sum = sum + tile[tid][c];
            }
        }
        __syncthreads();
    }
    if (!ok && !mean) atomicOr(bad, (uint32_t)BAD_VALUE);
    if (tid < kSumFeat && f0 + tid < m) part[(size_t)slab * (size_t)m + (size_t)(f0 + tid)] = sum;
}

__global__ void __launch_bounds__(256) k_slab_reduce(const double* __restrict__ part, int m, int S, double div,
                                                     double* __restrict__ out, double* __restrict__ out_sqrt) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= m) return;
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum = sum + part[(size_t)s * (size_t)m + (size_t)f];
    const double v = sum / div;
    out[f] = v;
    if (out_sqrt) out_sqrt[f] = sqrt(v);
}

// grid (ceil(n / 256), m)
__global__ void __launch_bounds__(256) k_standardize(const double* __restrict__ x, const double* __restrict__ mean,
                                                     const double* __restrict__ sd, int n, int m,
                                                     double* __restrict__ z) {
    const int f = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (f >= m || i >= n) return;
    const size_t at = (size_t)f * (size_t)n + (size_t)i;
    const double d = x[at] - mean[f];
    if (!sd) {
        z[at] = d;
    } else {
        const double q = sd[f];
        z[at] = q == 0.0 ? 0.0 : d / q;
    }
}

// ---------------------------------------------------------------------------
// covariance
// ---------------------------------------------------------------------------
// grid (nt (nt + 1) / 2, S), nt = ceil(m / T), T = 16 R. A[c][f], B[c][f]: item-major, a row is
// T + 1 doubles: a thread's reads of B are contiguous over tx, those of A a broadcast; the
// transposed stores of the staging (lanes along items) fall on distinct banks.
template <int R>
__global__ void __launch_bounds__(256) k_cov(const double* __restrict__ z, int n, int m, int nt,
                                             double* __restrict__ part) {
    constexpr int T = 16 * R;
    __shared__ double A[kChunk][T + 1];
    __shared__ double B[kChunk][T + 1];
    int ta = 0, rem = blockIdx.x;
    while (ta < nt && rem >= nt - ta) {  // the pair (ta, tb >= ta) number blockIdx.x, row by row
        rem -= nt - ta;
        ++ta;
    }
    if (ta >= nt) return;
    const int tb = ta + rem;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int a0 = ta * T, b0 = tb * T;
    const int slab = blockIdx.y, i_lo = slab * kSlab, i_hi = min(n, i_lo + kSlab);
    double acc[R][R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < R; ++q) acc[r][q] = 0.0;
    for (int i0 = i_lo; i0 < i_hi; i0 += kChunk) {
        for (int e = tid; e < T * kChunk; e += 256) {
            const int r = e / kChunk, c = e % kChunk;
            const bool in = i0 + c < i_hi;
            A[c][r] = (in && a0 + r < m) ? z[(size_t)(a0 + r) * (size_t)n + (size_t)(i0 + c)] : 0.0;
            B[c][r] = (in && b0 + r < m) ? z[(size_t)(b0 + r) * (size_t)n + (size_t)(i0 + c)] : 0.0;
        }
        __syncthreads();
        const int lim = min(kChunk, i_hi - i0);
        for (int c = 0; c < lim; ++c) {
            double va[R], vb[R];
#pragma unroll
            for (int r = 0; r < R; ++r) va[r] = A[c][ty + 16 * r];
#pragma unroll
            for (int q = 0; q < R; ++q) vb[q] = B[c][tx + 16 * q];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int q = 0; q < R; ++q) acc[r][q] = __builtin_fma(va[r], vb[q], acc[r][q]);
        }
        __syncthreads();
    }
    double* out = part + (size_t)slab * (size_t)m * (size_t)m;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int a = a0 + ty + 16 * r;
        if (a >= m) continue;
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int b = b0 + tx + 16 * q;
            if (b < m) out[(size_t)a * (size_t)m + (size_t)b] = acc[r][q];
        }
    }
}

// one thread per (a, b), a <= b (the partial of such a place is always written: tile(a) <= tile(b))
__global__ void __launch_bounds__(256) k_cov_reduce(const double* __restrict__ part, int m, int S, double div,
                                                    double* __restrict__ cov) {
    const size_t mm = (size_t)m * (size_t)m;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= mm) return;
    const size_t a = idx / (size_t)m, b = idx % (size_t)m;
    if (a > b) return;
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum = sum + part[(size_t)s * mm + idx];
    const double v = sum / div;
    cov[idx] = v;
    cov[b * (size_t)m + a] = v;
}

// ---------------------------------------------------------------------------
// the symmetric eigensolver
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sym_check(const double* __restrict__ a, int m, uint32_t* __restrict__ bad,
                                                   unsigned long long* __restrict__ maxabs) {
    const size_t total = (size_t)m * (size_t)m;
    uint32_t f = 0;
    unsigned long long big = 0;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t i = idx / (size_t)m, j = idx % (size_t)m;
        const double v = a[idx];
        if (!finite_f64(v)) {
            f |= BAD_VALUE;
        } else {
            // (a non-negative double's bits order as an integer)
            big = max(big, (unsigned long long)__double_as_longlong(fabs(v)));
        }
        if (j > i && !(v == a[j * (size_t)m + i])) f |= BAD_ASYMMETRIC;
    }
    if (f) atomicOr(bad, f);
    if (big) atomicMax(maxabs, big);
}

__global__ void __launch_bounds__(256) k_identity(double* __restrict__ vt, int m) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)m * (size_t)m) return;
    vt[idx] = idx / (size_t)m == idx % (size_t)m ? 1.0 : 0.0;
}

// grid (ceil(m / 16), ceil(m / 16)). Threads 0..31 derive the rotations of the tile's 16 row
// indices and 16 column indices into LDS from the snapshot (each from its pair's three entries);
// then a thread writes its element of A' and of V' (mgp_pca.h has the expressions).
__global__ void __launch_bounds__(256) k_jacobi_step(const double* __restrict__ a, const double* __restrict__ vt,
                                                     double* __restrict__ a2, double* __restrict__ vt2, int m, int step,
                                                     const unsigned long long* __restrict__ maxabs,
                                                     uint32_t* __restrict__ flag) {
    __shared__ double s_alpha[2 * kJTile], s_beta[2 * kJTile], s_t[2 * kJTile];
    __shared__ int s_partner[2 * kJTile], s_rot[2 * kJTile];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * kJTile, j0 = blockIdx.x * kJTile;
    const size_t M = (size_t)m;
    if (tid < 2 * kJTile) {
        const int idx = tid < kJTile ? i0 + tid : j0 + tid - kJTile;
        double alpha = 1.0, beta = 0.0, t = 0.0;
        int partner = idx, rot = 0;
        if (idx < m) {
            const int last = ((m + 1) & ~1) - 1;  // m' - 1: the index that stays in place
            int pr;
            if (idx == last) {
                pr = step;
            } else if (idx == step) {
                pr = last;
            } else {
                pr = (2 * step - idx) % last;
                if (pr < 0) pr += last;
            }
            if (pr < m && pr != idx) {
                const int p = min(idx, pr), q = max(idx, pr);
                const double apq = a[(size_t)p * M + (size_t)q];
                const double app = a[(size_t)p * M + (size_t)p], aqq = a[(size_t)q * M + (size_t)q];
                const double big = __longlong_as_double((long long)*maxabs);
                const double rel = 0x1p-53 * (sqrt(fabs(app)) * sqrt(fabs(aqq)));
                if (fabs(apq) > rel && fabs(apq) > 0x1p-63 * big) {
                    const double tau = (aqq - app) / (2.0 * apq);
                    t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    const double c = 1.0 / sqrt(1.0 + t * t);
                    const double sn = t * c;
                    alpha = c;
                    beta = idx == p ? -sn : sn;
                    partner = pr;
                    rot = 1;
                }
            }
        }
        s_alpha[tid] = alpha;
        s_beta[tid] = beta;
        s_t[tid] = t;
        s_partner[tid] = partner;
        s_rot[tid] = rot;
        if (rot && tid < kJTile && blockIdx.x == 0 && idx < partner) *flag = 1u;  // (every writer stores 1)
    }
    __syncthreads();
    const int i = i0 + ty, j = j0 + tx;
    if (i >= m || j >= m) return;
    const size_t at = (size_t)i * M + (size_t)j;
    const int ri = s_rot[ty], rj = s_rot[kJTile + tx];
    const int ip = s_partner[ty], jp = s_partner[kJTile + tx];
    const double ai = s_alpha[ty], bi = s_beta[ty], aj = s_alpha[kJTile + tx], bj = s_beta[kJTile + tx];
    double v;
    if (!ri && !rj) {
        v = a[at];
    } else if (ri && j == ip) {
        v = 0.0;
    } else if (ri && i == j) {
        const int p = min(i, ip), q = max(i, ip);
        const double w = s_t[ty] * a[(size_t)p * M + (size_t)q];
        v = i == p ? a[at] - w : a[at] + w;
    } else {
        const double t1 = (ai * aj) * a[at];
        const double t2 = (bi * aj) * a[(size_t)ip * M + (size_t)j];
        const double t3 = (ai * bj) * a[(size_t)i * M + (size_t)jp];
        const double t4 = (bi * bj) * a[(size_t)ip * M + (size_t)jp];
        v = (t1 + t4) + (t2 + t3);
    }
    a2[at] = v;
    vt2[at] = ri ? ai * vt[at] + bi * vt[(size_t)ip * M + (size_t)j] : vt[at];
}

// one workgroup per output vector
__global__ void __launch_bounds__(256) k_order_vec(const double* __restrict__ vt, const int32_t* __restrict__ perm,
                                                   int m, double* __restrict__ out) {
    __shared__ double s_mag[256];
    __shared__ int s_idx[256];
    const int tid = threadIdx.x;
    const double* src = vt + (size_t)perm[blockIdx.x] * (size_t)m;
    double mag = -1.0;
    int at = m;
    for (int f = tid; f < m; f += 256) {  // (f ascending in a thread: strict > keeps its lowest index)
        const double v = fabs(src[f]);
        if (v > mag) {
            mag = v;
            at = f;
        }
    }
    s_mag[tid] = mag;
    s_idx[tid] = at;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            const double om = s_mag[tid + off];
            const int oi = s_idx[tid + off];
            if (om > s_mag[tid] || (om == s_mag[tid] && oi < s_idx[tid])) {
                s_mag[tid] = om;
                s_idx[tid] = oi;
            }
        }
        __syncthreads();
    }
    const int lead = s_idx[0];
    const bool flip = lead < m && src[lead] < 0.0;
    double* dst = out + (size_t)blockIdx.x * (size_t)m;
    for (int f = tid; f < m; f += 256) dst[f] = flip ? -src[f] : src[f];
}

// ---------------------------------------------------------------------------
// scores
// ---------------------------------------------------------------------------
// grid (ceil(n / 256), ceil(k / 8)): a thread owns one item and the workgroup's 8 components
__global__ void __launch_bounds__(256) k_scores(const double* __restrict__ z, const double* __restrict__ vec, int n,
                                                int m, int k, double* __restrict__ out) {
    __shared__ double L[kScoreComp][kScoreFeat];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid, c0 = blockIdx.y * kScoreComp;
    double acc[kScoreComp];
#pragma unroll
    for (int c = 0; c < kScoreComp; ++c) acc[c] = 0.0;
    for (int f0 = 0; f0 < m; f0 += kScoreFeat) {
        for (int e = tid; e < kScoreComp * kScoreFeat; e += 256) {
            const int c = e / kScoreFeat, f = e % kScoreFeat;
            L[c][f] = (c0 + c < k && f0 + f < m) ? vec[(size_t)(c0 + c) * (size_t)m + (size_t)(f0 + f)] : 0.0;
        }
        __syncthreads();
        if (i < n) {
            const int lim = min(kScoreFeat, m - f0);
            for (int f = 0; f < lim; ++f) {
                const double zv = z[(size_t)(f0 + f) * (size_t)n + (size_t)i];
#pragma unroll
                for (int c = 0; c < kScoreComp; ++c) acc[c] = __builtin_fma(zv, L[c][f], acc[c]);
            }
        }
        __syncthreads();
    }
    if (i >= n) return;
#pragma unroll
    for (int c = 0; c < kScoreComp; ++c)
        if (c0 + c < k) out[(size_t)(c0 + c) * (size_t)n + (size_t)i] = acc[c];
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
static int launch_ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }
static unsigned blocks_of(size_t total) { return (unsigned)((total + 255) / 256); }

int cov_tile(int m, int want) {
    if (want == 16 || want == 32 || want == 64) return want;
    return m <= 256 ? 32 : 64;
}

int slab_sums(const double* x, const double* mean, int n, int m, double* part, uint32_t* bad, hipStream_t s) {
    if (n <= 0 || m <= 0) return 0;
    k_slab_sums<<<dim3((unsigned)slabs(n), (unsigned)((m + kSumFeat - 1) / kSumFeat)), 256, 0, s>>>(x, mean, n, m, part,
                                                                                                   bad);
    return launch_ok();
}

int slab_reduce(const double* part, int m, int S, double div, double* out, double* out_sqrt, hipStream_t s) {
    if (m <= 0) return 0;
    k_slab_reduce<<<blocks_of((size_t)m), 256, 0, s>>>(part, m, S, div, out, out_sqrt);
    return launch_ok();
}

int standardize(const double* x, const double* mean, const double* sd, int n, int m, double* z, hipStream_t s) {
    if (n <= 0 || m <= 0) return 0;
    k_standardize<<<dim3(blocks_of((size_t)n), (unsigned)m), 256, 0, s>>>(x, mean, sd, n, m, z);
    return launch_ok();
}

int covariance(const double* z, int n, int m, int tile, double* part, double* cov, hipStream_t s) {
    if (n <= 1 || m <= 0) return 0;
    const int S = slabs(n), nt = (m + tile - 1) / tile;
    const dim3 grid((unsigned)(nt * (nt + 1) / 2), (unsigned)S);
    if (tile == 16)
        k_cov<1><<<grid, 256, 0, s>>>(z, n, m, nt, part);
    else if (tile == 32)
        k_cov<2><<<grid, 256, 0, s>>>(z, n, m, nt, part);
    else if (tile == 64)
        k_cov<4><<<grid, 256, 0, s>>>(z, n, m, nt, part);
    else
        return -1;
    if (launch_ok() != 0) return -1;
    k_cov_reduce<<<blocks_of((size_t)m * (size_t)m), 256, 0, s>>>(part, m, S, (double)(n - 1), cov);
    return launch_ok();
}

int sym_check(const double* a, int m, uint32_t* bad, unsigned long long* maxabs, hipStream_t s) {
    if (m <= 0) return 0;
    const unsigned blocks = std::min(blocks_of((size_t)m * (size_t)m), 1u << 12);
    k_sym_check<<<blocks, 256, 0, s>>>(a, m, bad, maxabs);
    return launch_ok();
}

int identity(double* vt, int m, hipStream_t s) {
    if (m <= 0) return 0;
    k_identity<<<blocks_of((size_t)m * (size_t)m), 256, 0, s>>>(vt, m);
    return launch_ok();
}

int jacobi_step(const double* a, const double* vt, double* a2, double* vt2, int m, int step,
                const unsigned long long* maxabs, uint32_t* flag, hipStream_t s) {
    if (m < 2 || step < 0 || step >= ((m + 1) & ~1) - 1) return -1;
    const unsigned nt = (unsigned)((m + kJTile - 1) / kJTile);
    k_jacobi_step<<<dim3(nt, nt), 256, 0, s>>>(a, vt, a2, vt2, m, step, maxabs, flag);
    return launch_ok();
}

int order_vectors(const double* vt, const int32_t* perm, int m, int k, double* out, hipStream_t s) {
    if (m <= 0 || k <= 0) return 0;
    k_order_vec<<<(unsigned)k, 256, 0, s>>>(vt, perm, m, out);
    return launch_ok();
}

int scores(const double* z, const double* vec, int n, int m, int k, double* out, hipStream_t s) {
    if (n <= 0 || m <= 0 || k <= 0) return 0;
    k_scores<<<dim3(blocks_of((size_t)n), (unsigned)((k + kScoreComp - 1) / kScoreComp)), 256, 0, s>>>(z, vec, n, m, k,
                                                                                                      out);
    return launch_ok();
}

}  // namespace pca
}  // namespace mgp
