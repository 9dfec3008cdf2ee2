// mgp_louvain.hip — the kernels of mgp_louvain (mgp_louvain.h states the stages, the shapes of
// the move kernel, the rule on waiting and the device memory; include/mgpileup.h the definition).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mgp_louvain.h"

namespace mgp {
namespace louvain {

namespace {

typedef unsigned long long ull;
constexpr int kBlock = 256;
constexpr int kRowsPerBlock = 4;  // waves (rows) of a wave-per-row workgroup
constexpr int kScanBlock = 1024;
constexpr int32_t kEmpty = -1;

__device__ __forceinline__ void add64(uint64_t* p, uint64_t v) { atomicAdd(reinterpret_cast<ull*>(p), (ull)v); }

// the first slot a key probes in a table of `cap` slots (cap <= 2^32)
__device__ __forceinline__ int64_t first_slot(int32_t key, int64_t cap) {
    const uint32_t h = (uint32_t)key * 2654435761u;
    return (int64_t)(((uint64_t)h * (uint64_t)cap) >> 32);
}

// keys[slot] becomes `key` in the first free slot of its probe sequence (or is it already):
// the slot, or -1 when `cap` probes found neither (*fresh: this call took the slot)
__device__ __forceinline__ int64_t tab_slot(int32_t* keys, int64_t cap, int32_t key, bool* fresh) {
    int64_t at = first_slot(key, cap);
    for (int64_t t = 0; t < cap; ++t) {
        const int32_t prev = atomicCAS(&keys[at], kEmpty, key);
        if (prev == kEmpty || prev == key) {
            *fresh = prev == kEmpty;
            return at;
        }
        at = at + 1 == cap ? 0 : at + 1;
    }
    return -1;
}

// the gain's two products and their difference, each rounded on its own (no fma)
__device__ __forceinline__ double gain(uint64_t k, double m2, double g1, uint64_t t) {
    return __dsub_rn(__dmul_rn((double)k, m2), __dmul_rn(g1, (double)t));
}

// is (go, b) before (best_go, best_b) in the order (largest gain, then smallest community)
__device__ __forceinline__ bool before(double go, int32_t b, double best_go, int32_t best_b) {
    return go > best_go || (go == best_go && b < best_b);
}

template <typename T>
__global__ void __launch_bounds__(kScanBlock) k_scan(const T* __restrict__ v, int64_t n, int64_t* __restrict__ off) {
    __shared__ int64_t sh[kScanBlock];
    const int tid = threadIdx.x;
    const int64_t per = (n + kScanBlock - 1) / kScanBlock;
    const int64_t lo = min((int64_t)tid * per, n), hi = min(lo + per, n);
    int64_t sum = 0;
    for (int64_t e = lo; e < hi; ++e) sum += (int64_t)v[e];
    sh[tid] = sum;
    __syncthreads();
    for (int d = 1; d < kScanBlock; d <<= 1) {
        const int64_t t = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    int64_t run = sh[tid] - sum;
    for (int64_t e = lo; e < hi; ++e) {
        off[e] = run;
        run += (int64_t)v[e];
    }
    if (tid == kScanBlock - 1) off[n] = sh[tid];
}

// ---- build ---------------------------------------------------------------------------
__device__ __forceinline__ bool edge_ok(int32_t i, int32_t j, int32_t w, int n, uint32_t* bad) {
    uint32_t b = 0;
    if (i < 0 || j >= n || i >= j) b |= BAD_EDGE;
    if (w < 1 || w > kMaxWeight) b |= BAD_WEIGHT;
    if (b && bad) atomicOr(bad, b);
    return b == 0;
}

__global__ void __launch_bounds__(kBlock) k_build_degrees(const int32_t* __restrict__ ei, const int32_t* __restrict__ ej,
                                                          const int32_t* __restrict__ wq, int64_t ne, int n,
                                                          int32_t* __restrict__ deg, uint64_t* __restrict__ d,
                                                          uint32_t* __restrict__ bad) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < ne; e += (int64_t)gridDim.x * kBlock) {
        const int32_t i = ei[e], j = ej[e], w = wq[e];
        if (!edge_ok(i, j, w, n, bad)) continue;
        atomicAdd(&deg[i], 1);
        atomicAdd(&deg[j], 1);
        add64(&d[i], (uint64_t)w);
        add64(&d[j], (uint64_t)w);
    }
}

__global__ void __launch_bounds__(kBlock) k_build_fill(const int32_t* __restrict__ ei, const int32_t* __restrict__ ej,
                                                       const int32_t* __restrict__ wq, int64_t ne, int n,
                                                       int32_t* __restrict__ cur, Csr g) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < ne; e += (int64_t)gridDim.x * kBlock) {
        const int32_t i = ei[e], j = ej[e], w = wq[e];
        if (!edge_ok(i, j, w, n, nullptr)) continue;  // (the edges k_build_degrees counted)
        const int64_t pi = g.off[i] + atomicAdd(&cur[i], 1);
        const int64_t pj = g.off[j] + atomicAdd(&cur[j], 1);
        g.nbr[pi] = j, g.src[pi] = i, g.w[pi] = (uint64_t)w;
        g.nbr[pj] = i, g.src[pj] = j, g.w[pj] = (uint64_t)w;
    }
}

// a thread per forward entry (src < nbr): its neighbour into the row's table (2 x the row's
// length from 2 x the row's offset); a key that is already there is a repeated pair
__global__ void __launch_bounds__(kBlock) k_build_repeats(Csr g, int64_t m, int32_t* __restrict__ tkeys,
                                                          uint32_t* __restrict__ bad) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m; e += (int64_t)gridDim.x * kBlock) {
        const int32_t v = g.src[e], u = g.nbr[e];
        if (v >= u) continue;
        const int64_t lo = g.off[v], cap = 2 * (g.off[v + 1] - lo);
        bool fresh = false;
        const int64_t at = tab_slot(tkeys + 2 * lo, cap, u, &fresh);
        if (at < 0) atomicOr(bad, (uint32_t)BAD_TABLE);
        else if (!fresh) atomicOr(bad, (uint32_t)BAD_REPEAT);
    }
}

// ---- a level -------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_level_start(Csr g, int n, const uint64_t* __restrict__ d,
                                                        int32_t* __restrict__ c, uint64_t* __restrict__ tot,
                                                        int wave_row, int lds_row, int32_t* __restrict__ list_mid,
                                                        int32_t* __restrict__ list_long, int32_t* __restrict__ counts) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= n) return;
    c[v] = v;
    tot[v] = d[v];
    const int64_t deg = g.off[v + 1] - g.off[v];
    if (deg > wave_row) {
        if (deg <= lds_row) list_mid[atomicAdd(&counts[0], 1)] = v;
        else list_long[atomicAdd(&counts[1], 1)] = v;
    }
}

// A wave per row of at most 64 entries, an entry per lane: every lane sums the weights of the
// lanes that name its community (64 fixed steps), then the wave takes the best candidate.
__global__ void __launch_bounds__(64 * kRowsPerBlock) k_move_wave(Csr g, int n, const int32_t* __restrict__ c,
                                                                  const uint64_t* __restrict__ tot,
                                                                  const uint64_t* __restrict__ d, double m2,
                                                                  double gamma, int odd, int wave_row,
                                                                  int32_t* __restrict__ next) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n) return;
    const int64_t lo = g.off[row], deg = g.off[row + 1] - lo;
    if (deg == 0 || deg > wave_row || deg > 64) return;
    const bool have = lane < deg;
    const int32_t cu = have ? c[g.nbr[lo + lane]] : kEmpty;
    const ull wt = have ? (ull)g.w[lo + lane] : 0;
    ull k = 0;
    for (int t = 0; t < 64; ++t) {
        const int32_t ct = __shfl(cu, t, 64);
        const ull wo = __shfl(wt, t, 64);
        k += ct == cu ? wo : 0;
    }
    const int32_t a = c[row];
    const uint64_t dv = d[row];
    const double g1 = __dmul_rn(gamma, (double)dv);
    ull ka = have && cu == a ? k : 0;  // (every lane of community a holds the same sum)
    bool cand = have && cu != a && (odd ? cu > a : cu < a);
    double go = cand ? gain(k, m2, g1, tot[cu]) : 0.0;
    int32_t b = cand ? cu : kEmpty;
    for (int o = 32; o >= 1; o >>= 1) {
        const ull oka = __shfl_xor(ka, o, 64);
        const double ogo = __shfl_xor(go, o, 64);
        const int32_t ob = __shfl_xor(b, o, 64);
        const int oc = __shfl_xor((int)cand, o, 64);
        ka = oka > ka ? oka : ka;
        if (oc && (!cand || before(ogo, ob, go, b))) go = ogo, b = ob, cand = true;
    }
    if (lane == 0) {
        const double stay = gain(ka, m2, g1, tot[a] - dv);
        next[row] = cand && go > stay ? b : a;
    }
}

// A workgroup per listed row: the row's entries summed by community in an open-addressed table,
// in LDS (kLdsSlots slots; rows of at most kLdsRow entries) or in the row's slice of the global
// scratch (twice the row's length), then the table's slots scanned for the best candidate.
template <bool LDS>
__global__ void __launch_bounds__(kBlock) k_move_table(const int32_t* __restrict__ list, Csr g,
                                                       const int32_t* __restrict__ c, const uint64_t* __restrict__ tot,
                                                       const uint64_t* __restrict__ d, double m2, double gamma, int odd,
                                                       int32_t* __restrict__ tkeys, uint64_t* __restrict__ tvals,
                                                       int32_t* __restrict__ next, uint32_t* __restrict__ bad) {
    __shared__ int32_t s_keys[LDS ? kLdsSlots : 1];
    __shared__ uint64_t s_vals[LDS ? kLdsSlots : 1];
    __shared__ double s_go[kBlock];
    __shared__ int32_t s_b[kBlock];
    __shared__ ull s_ka;
    const int tid = threadIdx.x;
    const int32_t v = list[blockIdx.x];
    const int64_t lo = g.off[v], deg = g.off[v + 1] - lo;
    if (LDS && deg > kLdsRow) {  // (not reached: the list holds rows of at most lds_row <= kLdsRow)
        if (tid == 0) atomicOr(bad, (uint32_t)BAD_TABLE);
        return;
    }
    int32_t* keys = LDS ? s_keys : tkeys + 2 * lo;
    uint64_t* vals = LDS ? s_vals : tvals + 2 * lo;
    const int64_t cap = LDS ? (int64_t)kLdsSlots : 2 * deg;
    for (int64_t q = tid; q < cap; q += kBlock) keys[q] = kEmpty, vals[q] = 0;
    if (tid == 0) s_ka = 0;
    if (!LDS) __threadfence();
    __syncthreads();
    for (int64_t e = tid; e < deg; e += kBlock) {
        bool fresh = false;
        const int64_t at = tab_slot(keys, cap, c[g.nbr[lo + e]], &fresh);
        if (at < 0) atomicOr(bad, (uint32_t)BAD_TABLE);
        else add64(&vals[at], g.w[lo + e]);
    }
    if (!LDS) __threadfence();
    __syncthreads();
    const int32_t a = c[v];
    const uint64_t dv = d[v];
    const double g1 = __dmul_rn(gamma, (double)dv);
    double go = 0.0;
    int32_t b = kEmpty;
    for (int64_t q = tid; q < cap; q += kBlock) {
        // (the global table was written by atomics of other waves: read it past this unit's cache)
        const int32_t key = LDS ? keys[q] : __hip_atomic_load(&keys[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (key == kEmpty) continue;
        const uint64_t k = LDS ? vals[q] : __hip_atomic_load(&vals[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (key == a) {
            s_ka = (ull)k;  // (one slot holds a)
            continue;
        }
        if (odd ? key < a : key > a) continue;
        const double cgo = gain(k, m2, g1, tot[key]);
        if (b == kEmpty || before(cgo, key, go, b)) go = cgo, b = key;
    }
    s_go[tid] = go;
    s_b[tid] = b;
    __syncthreads();
    for (int o = kBlock / 2; o >= 1; o >>= 1) {
        if (tid < o && s_b[tid + o] != kEmpty &&
            (s_b[tid] == kEmpty || before(s_go[tid + o], s_b[tid + o], s_go[tid], s_b[tid]))) {
            s_go[tid] = s_go[tid + o];
            s_b[tid] = s_b[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double stay = gain((uint64_t)s_ka, m2, g1, tot[a] - dv);
        next[v] = s_b[0] != kEmpty && s_go[0] > stay ? s_b[0] : a;
    }
}

__global__ void __launch_bounds__(kBlock) k_apply(int n, const int32_t* __restrict__ c, const int32_t* __restrict__ next,
                                                  const uint64_t* __restrict__ d, uint64_t* __restrict__ tot_next,
                                                  int32_t* __restrict__ moved) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    const bool mv = v < n && next[v] != c[v];
    if (v < n) add64(&tot_next[next[v]], d[v]);
    const int cnt = __popcll(__ballot(mv));
    if (cnt && (threadIdx.x & 63) == 0) atomicAdd(moved, cnt);
}

// I: the entries whose ends share a label, and the vertices' self weights
__global__ void __launch_bounds__(kBlock) k_score_internal(Csr g, int64_t m, int n, const int32_t* __restrict__ c,
                                                           const uint64_t* __restrict__ self,
                                                           uint64_t* __restrict__ internal) {
    __shared__ uint64_t sh[kBlock];
    uint64_t sum = 0;
    const int64_t at = (int64_t)blockIdx.x * kBlock + threadIdx.x, step = (int64_t)gridDim.x * kBlock;
    for (int64_t e = at; e < m; e += step) sum += c[g.src[e]] == c[g.nbr[e]] ? g.w[e] : 0;
    for (int64_t v = at; v < n; v += step) sum += self[v];
    sh[threadIdx.x] = sum;
    __syncthreads();
    for (int o = kBlock / 2; o >= 1; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0]) add64(internal, sh[0]);
}

// B: a workgroup's exact 128-bit sum of tot^2 as (hi, lo)
__global__ void __launch_bounds__(kBlock) k_score_b(int n, const uint64_t* __restrict__ tot,
                                                    uint64_t* __restrict__ partial) {
    __shared__ uint64_t s_hi[kBlock], s_lo[kBlock];
    uint64_t hi = 0, lo = 0;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const uint64_t t = tot[v], l = t * t;
        lo += l;
        hi += __umul64hi(t, t) + (lo < l ? 1 : 0);
    }
    s_hi[threadIdx.x] = hi;
    s_lo[threadIdx.x] = lo;
    __syncthreads();
    for (int o = kBlock / 2; o >= 1; o >>= 1) {
        if (threadIdx.x < o) {
            const uint64_t l = s_lo[threadIdx.x + o];
            s_lo[threadIdx.x] += l;
            s_hi[threadIdx.x] += s_hi[threadIdx.x + o] + (s_lo[threadIdx.x] < l ? 1 : 0);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[2 * blockIdx.x] = s_hi[0], partial[2 * blockIdx.x + 1] = s_lo[0];
}

// ---- aggregation ---------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_agg_flag(int n, const int32_t* __restrict__ c, int32_t* __restrict__ flag) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v < n) flag[c[v]] = 1;
}

__global__ void __launch_bounds__(kBlock) k_agg_vertices(int n, const int32_t* __restrict__ c,
                                                         const int64_t* __restrict__ ren,
                                                         const int32_t* __restrict__ flag,
                                                         const uint64_t* __restrict__ tot,
                                                         const uint64_t* __restrict__ self, uint64_t* __restrict__ d2,
                                                         uint64_t* __restrict__ self2) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= n) return;
    if (flag[v]) d2[ren[v]] = tot[v];
    if (self[v]) add64(&self2[ren[c[v]]], self[v]);
}

__global__ void __launch_bounds__(kBlock) k_agg_map(int n0, int32_t* __restrict__ map, const int32_t* __restrict__ c,
                                                    const int64_t* __restrict__ ren) {
    const int u = blockIdx.x * kBlock + threadIdx.x;
    if (u < n0) map[u] = (int32_t)ren[c[map[u]]];
}

// an entry inside a community adds to the coarse vertex's self weight, one across to its row's count
__global__ void __launch_bounds__(kBlock) k_agg_entries(Csr g, int64_t m, const int32_t* __restrict__ c,
                                                        const int64_t* __restrict__ ren, uint64_t* __restrict__ self2,
                                                        int64_t* __restrict__ cap) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m; e += (int64_t)gridDim.x * kBlock) {
        const int32_t cv = c[g.src[e]], cu = c[g.nbr[e]];
        if (cv == cu) add64(&self2[ren[cv]], g.w[e]);
        else atomicAdd(reinterpret_cast<ull*>(&cap[ren[cv]]), (ull)1);
    }
}

__global__ void __launch_bounds__(kBlock) k_agg_insert(Csr g, int64_t m, const int32_t* __restrict__ c,
                                                       const int64_t* __restrict__ ren, const int64_t* __restrict__ slot,
                                                       int32_t* __restrict__ tkeys, uint64_t* __restrict__ tvals,
                                                       uint32_t* __restrict__ bad) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m; e += (int64_t)gridDim.x * kBlock) {
        const int32_t cv = c[g.src[e]], cu = c[g.nbr[e]];
        if (cv == cu) continue;
        const int64_t r = ren[cv], lo = 2 * slot[r], cap = 2 * (slot[r + 1] - slot[r]);
        bool fresh = false;
        const int64_t at = tab_slot(tkeys + lo, cap, (int32_t)ren[cu], &fresh);
        if (at < 0) atomicOr(bad, (uint32_t)BAD_TABLE);
        else add64(&tvals[lo + at], g.w[e]);
    }
}

// a wave per coarse row: the keys of its table counted, or written from off[row] on in slot order
__global__ void __launch_bounds__(64 * kRowsPerBlock) k_agg_rows(int n2, const int64_t* __restrict__ slot,
                                                                 const int32_t* __restrict__ tkeys,
                                                                 const uint64_t* __restrict__ tvals,
                                                                 int32_t* __restrict__ deg2, bool fill, Csr g2) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n2) return;
    const int64_t lo = 2 * slot[row], cap = 2 * (slot[row + 1] - slot[row]);
    const int64_t at = fill ? g2.off[row] : 0;
    int64_t run = 0;
    for (int64_t q0 = 0; q0 < cap; q0 += 64) {
        const int64_t q = q0 + lane;
        const int32_t key = q < cap ? tkeys[lo + q] : kEmpty;
        const uint64_t mask = __ballot(key != kEmpty);
        if (fill && key != kEmpty) {
            const int64_t p = at + run + __popcll(mask & (((uint64_t)1 << lane) - 1));
            g2.nbr[p] = key;
            g2.src[p] = row;
            g2.w[p] = tvals[lo + q];
        }
        run += __popcll(mask);
    }
    if (!fill && lane == 0) deg2[row] = (int32_t)run;
}

int launch_ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }
unsigned blocks_for(int64_t items) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kBlock - 1) / kBlock, 1 << 16));
}
unsigned row_blocks(int n) { return (unsigned)((n + kRowsPerBlock - 1) / kRowsPerBlock); }
bool zero(void* p, size_t bytes, hipStream_t s) { return bytes == 0 || hipMemsetAsync(p, 0, bytes, s) == hipSuccess; }

}  // namespace

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
int scan32(const int32_t* v, int64_t n, int64_t* off, hipStream_t s) {
    k_scan<int32_t><<<1, kScanBlock, 0, s>>>(v, std::max<int64_t>(n, 0), off);
    return launch_ok();
}

int scan64(const int64_t* v, int64_t n, int64_t* off, hipStream_t s) {
    k_scan<int64_t><<<1, kScanBlock, 0, s>>>(v, std::max<int64_t>(n, 0), off);
    return launch_ok();
}

int build_degrees(const int32_t* ei, const int32_t* ej, const int32_t* wq, int64_t ne, int n, int32_t* deg,
                  uint64_t* d, uint32_t* bad, hipStream_t s) {
    if (!zero(deg, (size_t)n * 4, s) || !zero(d, (size_t)n * 8, s)) return -1;
    if (ne <= 0) return 0;
    k_build_degrees<<<blocks_for(ne), kBlock, 0, s>>>(ei, ej, wq, ne, n, deg, d, bad);
    return launch_ok();
}

int build_fill(const int32_t* ei, const int32_t* ej, const int32_t* wq, int64_t ne, int n, int32_t* cur, Csr g,
               hipStream_t s) {
    if (!zero(cur, (size_t)n * 4, s)) return -1;
    if (ne <= 0) return 0;
    k_build_fill<<<blocks_for(ne), kBlock, 0, s>>>(ei, ej, wq, ne, n, cur, g);
    return launch_ok();
}

int build_repeats(Csr g, int64_t m, int32_t* tkeys, uint32_t* bad, hipStream_t s) {
    if (m <= 0) return 0;
    if (hipMemsetAsync(tkeys, 0xFF, (size_t)m * 2 * 4, s) != hipSuccess) return -1;
    k_build_repeats<<<blocks_for(m), kBlock, 0, s>>>(g, m, tkeys, bad);
    return launch_ok();
}

int level_start(Csr g, int n, const uint64_t* d, int32_t* c, uint64_t* tot, int wave_row, int lds_row,
                int32_t* list_mid, int32_t* list_long, int32_t* counts, hipStream_t s) {
    if (!zero(counts, 8, s)) return -1;
    k_level_start<<<blocks_for(n), kBlock, 0, s>>>(g, n, d, c, tot, wave_row, lds_row, list_mid, list_long, counts);
    return launch_ok();
}

int move(Csr g, int n, const int32_t* c, const uint64_t* tot, const uint64_t* d, uint64_t m2, double gamma, int odd,
         int wave_row, const int32_t* list_mid, int n_mid, const int32_t* list_long, int n_long, int32_t* tkeys,
         uint64_t* tvals, int32_t* next, uint32_t* bad, hipStream_t s) {
    const double fm2 = (double)m2;
    if (wave_row > 0) {
        k_move_wave<<<row_blocks(n), 64 * kRowsPerBlock, 0, s>>>(g, n, c, tot, d, fm2, gamma, odd, wave_row, next);
        if (launch_ok() != 0) return -1;
    }
    if (n_mid > 0) {
        k_move_table<true><<<(unsigned)n_mid, kBlock, 0, s>>>(list_mid, g, c, tot, d, fm2, gamma, odd, tkeys, tvals,
                                                              next, bad);
        if (launch_ok() != 0) return -1;
    }
    if (n_long > 0) {
        k_move_table<false><<<(unsigned)n_long, kBlock, 0, s>>>(list_long, g, c, tot, d, fm2, gamma, odd, tkeys, tvals,
                                                                next, bad);
        if (launch_ok() != 0) return -1;
    }
    return 0;
}

int apply(int n, const int32_t* c, const int32_t* next, const uint64_t* d, uint64_t* tot_next, int32_t* moved,
          hipStream_t s) {
    if (!zero(tot_next, (size_t)n * 8, s) || !zero(moved, 4, s)) return -1;
    k_apply<<<blocks_for(n), kBlock, 0, s>>>(n, c, next, d, tot_next, moved);
    return launch_ok();
}

int score(Csr g, int64_t m, int n, const int32_t* c, const uint64_t* self, const uint64_t* tot, uint64_t* internal,
          uint64_t* partial, hipStream_t s) {
    if (!zero(internal, 8, s) || !zero(partial, (size_t)kScoreBlocks * 16, s)) return -1;
    const unsigned nb = (unsigned)std::min<int64_t>(blocks_for(std::max<int64_t>(m, n)), 4096);
    k_score_internal<<<nb, kBlock, 0, s>>>(g, m, n, c, self, internal);
    if (launch_ok() != 0) return -1;
    k_score_b<<<std::min<unsigned>(blocks_for(n), kScoreBlocks), kBlock, 0, s>>>(n, tot, partial);
    return launch_ok();
}

int agg_flag(int n, const int32_t* c, int32_t* flag, hipStream_t s) {
    if (!zero(flag, (size_t)n * 4, s)) return -1;
    k_agg_flag<<<blocks_for(n), kBlock, 0, s>>>(n, c, flag);
    return launch_ok();
}

int agg_map(int n0, int32_t* map, const int32_t* c, const int64_t* ren, hipStream_t s) {
    if (n0 <= 0) return 0;
    k_agg_map<<<blocks_for(n0), kBlock, 0, s>>>(n0, map, c, ren);
    return launch_ok();
}

int agg_vertices(Csr g, int64_t m, int n, int n2, const int32_t* c, const int64_t* ren, const int32_t* flag,
                 const uint64_t* tot, const uint64_t* self, uint64_t* d2, uint64_t* self2, int64_t* cap,
                 hipStream_t s) {
    if (!zero(d2, (size_t)n2 * 8, s) || !zero(self2, (size_t)n2 * 8, s) || !zero(cap, (size_t)n2 * 8, s)) return -1;
    k_agg_vertices<<<blocks_for(n), kBlock, 0, s>>>(n, c, ren, flag, tot, self, d2, self2);
    if (launch_ok() != 0) return -1;
    if (m <= 0) return 0;
    k_agg_entries<<<blocks_for(m), kBlock, 0, s>>>(g, m, c, ren, self2, cap);
    return launch_ok();
}

int agg_insert(Csr g, int64_t m, const int32_t* c, const int64_t* ren, const int64_t* slot, int32_t* tkeys,
               uint64_t* tvals, uint32_t* bad, hipStream_t s) {
    if (m <= 0) return 0;
    // (the rows' tables lie within the first 2 m slots: the cross entries are at most m)
    if (hipMemsetAsync(tkeys, 0xFF, (size_t)m * 2 * 4, s) != hipSuccess || !zero(tvals, (size_t)m * 2 * 8, s))
        return -1;
    k_agg_insert<<<blocks_for(m), kBlock, 0, s>>>(g, m, c, ren, slot, tkeys, tvals, bad);
    return launch_ok();
}

int agg_rows(int n2, const int64_t* slot, const int32_t* tkeys, const uint64_t* tvals, int32_t* deg2, const Csr* g2,
             hipStream_t s) {
    if (n2 <= 0) return 0;
    k_agg_rows<<<row_blocks(n2), 64 * kRowsPerBlock, 0, s>>>(n2, slot, tkeys, tvals, deg2, g2 != nullptr,
                                                             g2 ? *g2 : Csr{});
    return launch_ok();
}

}  // namespace louvain
}  // namespace mgp
