// mgp_variants.hip — variant statistics and heteroplasmy from the count rows in HBM
// (gfx950, wave64). See mgp_variants.h for what is computed and the exactness bound.
//
// The reductions run over cells, not positions: one position per lane, so a wave reads 64
// consecutive positions of a cell (1 KB of its uint4 rows), and a loop over a slab of the
// population's cells. grid.x = ceil(L / 256) position blocks, grid.y = cell slabs: chrM's
// 16,569 positions alone are 65 workgroups, the slabs bring the grid to ~1000.
// The loop over the cells is sweep() of mgp_sweep.h, which mgp_qc.hip shares.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mgp_sweep.h"
#include "mgp_variants.h"

namespace mgp {
namespace variants {

using sweep_detail::Cnt;
using sweep_detail::kBlock;
using sweep_detail::load_row;
using sweep_detail::sweep;
using sweep_detail::wide_at;
using txtgz::Rows;

constexpr int kTargetGroups = 1024;  // ~4 workgroups per CU

struct MomentAcc {
    uint32_t thr;
    uint32_t n_det[4] = {0, 0, 0, 0}, n_conf[4] = {0, 0, 0, 0}, m[4] = {0, 0, 0, 0};
    unsigned long long s_total[4] = {0, 0, 0, 0}, sf[4] = {0, 0, 0, 0}, sr[4] = {0, 0, 0, 0}, sff[4] = {0, 0, 0, 0},
                       srr[4] = {0, 0, 0, 0}, sfr[4] = {0, 0, 0, 0};
    unsigned long long s_cov = 0;
    uint32_t n_low = 0, big = 0;
    double s_af[4] = {0, 0, 0, 0};
    __device__ __forceinline__ void cell(const Cnt& x) {
        const bool low = x.cov < thr;
        n_low += low;
        s_cov += x.cov;
        const double dc = (double)x.cov;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t f = x.f[b], r = x.r[b], t = f + r;
            big |= f | r;
            if (t) {
                ++n_det[b];
                n_conf[b] += (f >= 2 && r >= 2);
                s_total[b] += t;
                if (f) {
                    ++m[b];
                    sf[b] += f;
                    sr[b] += r;
                    sff[b] += (unsigned long long)f * f;
                    srr[b] += (unsigned long long)r * r;
                    sfr[b] += (unsigned long long)f * r;
                }
                if (!low && x.cov) s_af[b] += (double)t / dc;
            }
        }
    }
};

__device__ __forceinline__ void add64(unsigned long long* a, unsigned long long v) {
    if (v) atomicAdd(a, v);
}

__global__ void __launch_bounds__(kBlock) k_moments(Rows R, const int32_t* __restrict__ cells, int64_t n, int64_t slab,
                                                    uint32_t thr, unsigned long long* __restrict__ acc,
                                                    double* __restrict__ part, uint32_t* __restrict__ bad) {
    MomentAcc a;
    a.thr = thr;
    const int64_t k0 = (int64_t)blockIdx.y * slab, k1 = min(n, k0 + slab);
    sweep(R, cells, k0, k1, a);
    const int p = blockIdx.x * kBlock + (int)threadIdx.x;
    if (p >= R.L) return;
    const size_t plane = (size_t)R.L * 4;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        unsigned long long* q = acc + (size_t)p * 4 + b;
        add64(q + F_NDET * plane, a.n_det[b]);
        add64(q + F_NCONF * plane, a.n_conf[b]);
        add64(q + F_STOTAL * plane, a.s_total[b]);
        add64(q + F_M * plane, a.m[b]);
        add64(q + F_SF * plane, a.sf[b]);
        add64(q + F_SR * plane, a.sr[b]);
        add64(q + F_SFF * plane, a.sff[b]);
        add64(q + F_SRR * plane, a.srr[b]);
        add64(q + F_SFR * plane, a.sfr[b]);
        part[((size_t)blockIdx.y * R.L + p) * 4 + b] = a.s_af[b];
    }
    add64(acc + F_N * plane + p, a.s_cov);
    add64(acc + F_N * plane + R.L + p, a.n_low);
    if (a.big >= kMaxCount) atomicOr(bad, 1u);
}

struct Dev2Acc {
    uint32_t thr;
    double mu[4];
    double s[4] = {0, 0, 0, 0};
    __device__ __forceinline__ void cell(const Cnt& x) {
        if (x.cov < thr) return;
        const double dc = (double)x.cov;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t t = x.f[b] + x.r[b];
            const double af = (t && x.cov) ? (double)t / dc : 0.0;
            const double d = af - mu[b];
            s[b] += d * d;
        }
    }
};

__global__ void __launch_bounds__(kBlock) k_dev2(Rows R, const int32_t* __restrict__ cells, int64_t n, int64_t slab,
                                                 uint32_t thr, const double* __restrict__ mu, double* __restrict__ part) {
    Dev2Acc a;
    a.thr = thr;
    const int p = blockIdx.x * kBlock + (int)threadIdx.x;
#pragma unroll
    for (int b = 0; b < 4; ++b) a.mu[b] = p < R.L ? mu[(size_t)p * 4 + b] : 0.0;
    const int64_t k0 = (int64_t)blockIdx.y * slab, k1 = min(n, k0 + slab);
    sweep(R, cells, k0, k1, a);
    if (p >= R.L) return;
#pragma unroll
    for (int b = 0; b < 4; ++b) part[((size_t)blockIdx.y * R.L + p) * 4 + b] = a.s[b];
}

// out[i] = part[0][i] + part[1][i] + ... in slab order
__global__ void __launch_bounds__(kBlock) k_combine(const double* __restrict__ part, int nslab, size_t count,
                                                    double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    double s = 0.0;
    for (int k = 0; k < nslab; ++k) s += part[(size_t)k * count + i];
    out[i] = s;
}

__global__ void __launch_bounds__(kBlock) k_gather(Rows R, const int32_t* __restrict__ cells, int64_t n,
                                                   const int32_t* __restrict__ pos, const int32_t* __restrict__ base,
                                                   uint32_t min_cov, double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const int64_t v = blockIdx.y;
    const int p = pos[v], b = base[v];
    const int c = cells ? cells[j] : (int)j;
    Cnt x;
    load_row(R, c, p, c >= 0 && !wide_at(R, c, p / R.W), x);
    const uint32_t t = b == 0 ? x.f[0] + x.r[0] : b == 1 ? x.f[1] + x.r[1] : b == 2 ? x.f[2] + x.r[2] : x.f[3] + x.r[3];
    out[v * n + j] = (x.cov && x.cov >= min_cov) ? (double)t / (double)x.cov : 0.0;
}

static int64_t slab_cells(int64_t n, int L) {
    const int gx = (L + kBlock - 1) / kBlock;
    const int64_t want = std::max<int64_t>(1, kTargetGroups / gx);  // slabs that fill the device
    const int64_t ns = std::max<int64_t>(1, std::min<int64_t>(want, (n + 31) / 32));  // at least 32 cells each
    return (n + ns - 1) / ns;
}

// (L enters only through the slab count's cap: slabs(n) is an upper bound for every L)
int slabs(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(kTargetGroups, (n + 31) / 32)); }

static int launch_ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

int moments(const Rows& rows, const int32_t* cells, int64_t n, uint32_t thr, unsigned long long* acc, double* part,
            double* s_af, uint32_t* bad, hipStream_t s) {
    const int L = rows.L;
    if (hipMemsetAsync(acc, 0, acc_words(L) * 8, s) != hipSuccess) return -1;
    if (hipMemsetAsync(bad, 0, 4, s) != hipSuccess) return -1;
    const int64_t slab = slab_cells(std::max<int64_t>(n, 1), L);
    const int ns = (int)std::max<int64_t>(1, (n + slab - 1) / slab);
    const dim3 grid((L + kBlock - 1) / kBlock, ns);
    k_moments<<<grid, kBlock, 0, s>>>(rows, cells, n, slab, thr, acc, part, bad);
    if (launch_ok() != 0) return -1;
    const size_t count = (size_t)L * 4;
    k_combine<<<(unsigned)((count + kBlock - 1) / kBlock), kBlock, 0, s>>>(part, ns, count, s_af);
    return launch_ok();
}

int dev2(const Rows& rows, const int32_t* cells, int64_t n, uint32_t thr, const double* mu, double* part, double* out,
         hipStream_t s) {
    const int L = rows.L;
    const int64_t slab = slab_cells(std::max<int64_t>(n, 1), L);
    const int ns = (int)std::max<int64_t>(1, (n + slab - 1) / slab);
    const dim3 grid((L + kBlock - 1) / kBlock, ns);
    k_dev2<<<grid, kBlock, 0, s>>>(rows, cells, n, slab, thr, mu, part);
    if (launch_ok() != 0) return -1;
    const size_t count = (size_t)L * 4;
    k_combine<<<(unsigned)((count + kBlock - 1) / kBlock), kBlock, 0, s>>>(part, ns, count, out);
    return launch_ok();
}

int gather(const Rows& rows, const int32_t* cells, int64_t n, const int32_t* pos, const int32_t* base, int64_t n_var,
           uint32_t min_cov, double* out, hipStream_t s) {
    if (n <= 0 || n_var <= 0) return 0;
    for (int64_t v0 = 0; v0 < n_var; v0 += 65535) {  // (grid.y's limit)
        const int64_t nv = std::min<int64_t>(65535, n_var - v0);
        const dim3 grid((unsigned)((n + kBlock - 1) / kBlock), (unsigned)nv);
        k_gather<<<grid, kBlock, 0, s>>>(rows, cells, n, pos + v0, base + v0, min_cov, out + v0 * n);
        if (launch_ok() != 0) return -1;
    }
    return 0;
}

}  // namespace variants
}  // namespace mgp
