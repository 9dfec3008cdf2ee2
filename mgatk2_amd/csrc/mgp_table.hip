// mgp_table.hip — a finished run's count files loaded into a table context:
// the HDF5 chunks of counts.h5 / metadata.h5 (11 u16 planes [mito_len][n_cols], chunks of
// chunk_rows x chunk_cols, each one zlib stream) are inflated on the device, one wave per
// chunk over the streaming decoder of mgp_inflate_core.h (inflate_chunks), and their tiles
// transposed into the 16-bit cell rows every row job reads (tiles_to_rows). The C-ABI
// (include/mgpileup.h): mgp_table_load, mgp_table_load_planes, mgp_table_check and the
// detached probe mgp_zlib_inflate. The context itself (mgp_open_table, mgp_table_ready) is
// mgp_engine.hip's; this file reaches it through table_planes (mgp_jobs.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mgpileup.h"
#include "mgp_host.h"
#include "mgp_inflate_core.h"
#include "mgp_jobs.h"

namespace {

using namespace mgp_inflate;

constexpr int kPlanes = 11;  // engine.H5_PLANES: 8 count planes, tn5 fwd and rev, coverage

// The wave of inflate_chunks: a workgroup is one wave of 64 lanes, so the workgroup barrier
// is the wave's own (it orders the LDS and global accesses of its lanes).
struct DeviceWave {
    __device__ uint32_t lane() const { return threadIdx.x; }
    __device__ uint32_t width() const { return 64; }
    __device__ bool leader() const { return threadIdx.x == 0; }
    __device__ void sync() const { __syncthreads(); }
};

enum : uint8_t { CH_ZLIB = 0, CH_RAW = 1, CH_ABSENT = 2 };  // mgp_table_chunks.raw

// Stream b = blockIdx.x: the zlib stream src[coff[b], + clen[b]) into out[out_off[b], +
// isize[b]) through the LDS ring (Scratch + 64 KiB: two workgroups on a CU). A chunk whose
// filter mask says "deflate skipped" (CH_RAW) is copied (clen == isize, else ST_SIZE), an
// unallocated one (CH_ABSENT) is zeros. A refused stream may have written a part of its own
// range. The host checked every range against src and out before the launch.
__global__ __launch_bounds__(64) void inflate_chunks(const uint8_t* __restrict__ src, const uint64_t* __restrict__ coff,
                                                     const uint32_t* __restrict__ clen,
                                                     const uint32_t* __restrict__ isize,
                                                     const uint64_t* __restrict__ out_off,
                                                     const uint8_t* __restrict__ raw, uint8_t* __restrict__ out,
                                                     int32_t* __restrict__ status, uint32_t n_streams) {
    __shared__ Scratch sc;
    __shared__ alignas(16) uint8_t ring[kRing];
    const uint32_t b = blockIdx.x;
    if (b >= n_streams) return;
    const DeviceWave w;
    const uint32_t n = isize[b];
    uint8_t* dst = out + out_off[b];
    const uint8_t kind = raw ? raw[b] : (uint8_t)CH_ZLIB;
    int32_t st;
    if (kind == CH_ZLIB) {
        st = inflate_zlib(w, src + coff[b], clen[b], ring, dst, n, &sc);
    } else if (kind == CH_RAW) {
        st = clen[b] == n ? ST_OK : ST_SIZE;
        if (st == ST_OK) flush(w, src + coff[b], n, dst);
    } else {
        st = ST_OK;
        for (uint32_t i = w.lane(); i < n; i += w.width()) dst[i] = 0;
    }
    if (w.leader()) status[b] = st;
}

// tiles_to_rows: the sub-tile of a workgroup is kTP positions x kTC cells of one chunk, for
// all 11 planes, through an LDS tile of 8 planes (the counts, then tn5's two, then the
// coverage). A wave reads a plane in runs of 64 cells (128 bytes) at one position, and
// writes one cell's run of 64 positions (1 KiB of c16, 256 bytes of t16, 128 of d16).
// The LDS row pitch kTCP = 66 u16 = 33 dwords: the readers' lanes differ in the position,
// 33 dwords apart, so the 32 lanes of an LDS lane group fall on 32 different banks.
constexpr int kTP = 64, kTC = 64, kTCP = 66, kTBlock = 256;

struct TileJob {
    const uint8_t* tiles;  // tile t = (plane * nrc + rc) * ncc + cc at t * stride: [chunk_rows][chunk_cols] u16
    uint64_t stride;
    int crow, ccol, nrc, ncc, nsc;  // nsc: sub-tiles of cells per chunk
    int L;
    int64_t cols_left;   // the datasets' columns from the batch's first on (n_cols - lo * chunk_cols)
    int64_t first_cell;  // the table row of the batch's first column
    uint4* c16;
    uint32_t* t16;
    uint16_t* d16;
    unsigned long long* n_sat;
};

__global__ __launch_bounds__(kTBlock) void tiles_to_rows(TileJob j) {
    __shared__ uint16_t t[8][kTP][kTCP];
    __shared__ uint32_t wsat[kTBlock / 64];
    const int nsp = (j.crow + kTP - 1) / kTP;
    const int rc = (int)(blockIdx.x / nsp), sp = (int)(blockIdx.x % nsp);
    const int cc = (int)(blockIdx.y / j.nsc), sc = (int)(blockIdx.y % j.nsc);
    if (rc >= j.nrc || cc >= j.ncc) return;
    const int pr0 = sp * kTP, cl0 = sc * kTC;             // the sub-tile's first row and column in its chunk
    const int64_t p0 = (int64_t)rc * j.crow + pr0;        // its first position
    const int64_t col0 = (int64_t)cc * j.ccol + cl0;      // its first column, from the batch's first
    // the padding of edge chunks is dropped: positions >= L, columns >= n_cols
    const int np = (int)min((int64_t)min(kTP, j.crow - pr0), (int64_t)j.L - p0);
    const int ncell = (int)min((int64_t)min(kTC, j.ccol - cl0), j.cols_left - col0);
    if (np <= 0 || ncell <= 0) return;  // (the same in every thread)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t sat = 0;
    auto stage = [&](int pl0, int npl) {
        __syncthreads();  // (the tile's earlier readers are done)
        for (int pl = 0; pl < npl; ++pl) {
            const uint64_t tile = ((uint64_t)(pl0 + pl) * j.nrc + rc) * j.ncc + cc;
            const uint16_t* src = reinterpret_cast<const uint16_t*>(j.tiles + tile * j.stride);
            for (int r = wv; r < np; r += kTBlock / 64) {
                if (lane < ncell) {
                    const uint16_t v = src[(size_t)(pr0 + r) * j.ccol + cl0 + lane];
                    sat += v == 0xFFFFu;
                    t[pl][r][lane] = v;
                }
            }
        }
        __syncthreads();
    };
    const size_t row0 = (size_t)(j.first_cell + col0) * (size_t)j.L + (size_t)p0;
    stage(0, 8);
    for (int k = wv; k < ncell; k += kTBlock / 64) {
        if (lane < np) {
            uint4 q;
            q.x = (uint32_t)t[0][lane][k] | (uint32_t)t[1][lane][k] << 16;
            q.y = (uint32_t)t[2][lane][k] | (uint32_t)t[3][lane][k] << 16;
            q.z = (uint32_t)t[4][lane][k] | (uint32_t)t[5][lane][k] << 16;
            q.w = (uint32_t)t[6][lane][k] | (uint32_t)t[7][lane][k] << 16;
            j.c16[row0 + (size_t)k * j.L + lane] = q;
        }
    }
    stage(8, 2);
    for (int k = wv; k < ncell; k += kTBlock / 64)
        if (lane < np) j.t16[row0 + (size_t)k * j.L + lane] = (uint32_t)t[0][lane][k] | (uint32_t)t[1][lane][k] << 16;
    stage(10, 1);
    for (int k = wv; k < ncell; k += kTBlock / 64)
        if (lane < np) j.d16[row0 + (size_t)k * j.L + lane] = t[0][lane][k];
    // the values equal to 65,535: the wave's sum, the workgroup's, one atomic add
    for (int o = 32; o > 0; o >>= 1) sat += __shfl_down(sat, o, 64);
    if (lane == 0) wsat[wv] = sat;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int i = 0; i < kTBlock / 64; ++i) s += wsat[i];
        if (s) atomicAdd(j.n_sat, (unsigned long long)s);
    }
}

// The batch of `job` over a table of n_cells x mito_len, derived after table_check
struct Batch {
    int nrc, ncc;
    int64_t nch;         // 11 * nrc * ncc
    uint64_t tile_bytes; // chunk_rows * chunk_cols * 2
    uint64_t stride;     // a tile's place in the device buffer (16-byte multiple)
};

Batch batch_of(const mgp_table_chunks* job, int32_t mito_len) {
    Batch b;
    b.nrc = (mito_len + job->chunk_rows - 1) / job->chunk_rows;
    b.ncc = job->col_chunk_hi - job->col_chunk_lo;
    b.nch = (int64_t)kPlanes * b.nrc * b.ncc;
    b.tile_bytes = (uint64_t)job->chunk_rows * job->chunk_cols * 2;
    b.stride = (b.tile_bytes + 15) & ~uint64_t(15);
    return b;
}

// Every refusal of a batch's arguments, before any allocation or launch. planes: the batch
// is inflated tiles (mgp_table_load_planes), not streams.
int table_check(const char* who, int32_t n_cells, int32_t mito_len, const mgp_table_chunks* job, bool planes) {
    const std::string w(who);
    if (!job) return set_err(MGP_E_INVALID, w + ": null job");
    if (n_cells < 0 || mito_len <= 0 || mito_len > (1 << 24)) return set_err(MGP_E_INVALID, w + ": table shape out of range");
    if (job->n_cols < 0 || job->n_cols > 0x7FFFFFFF) return set_err(MGP_E_INVALID, w + ": n_cols out of range");
    if (job->chunk_rows <= 0 || job->chunk_cols <= 0) return set_err(MGP_E_INVALID, w + ": chunk shape not positive");
    if ((int64_t)job->chunk_rows * job->chunk_cols * 2 >= ((int64_t)1 << 31))
        return set_err(MGP_E_INVALID, w + ": a chunk of 2^31 bytes or more");
    const int64_t ncc_all = (job->n_cols + job->chunk_cols - 1) / job->chunk_cols;
    const int64_t lo = job->col_chunk_lo, hi = job->col_chunk_hi;
    if (lo < 0 || hi < lo || hi > ncc_all) return set_err(MGP_E_INVALID, w + ": column chunks out of range");
    const Batch b = batch_of(job, mito_len);
    if (b.nch > ((int64_t)1 << 20)) return set_err(MGP_E_INVALID, w + ": too many chunks for one call");
    if ((int64_t)b.ncc * ((job->chunk_cols + kTC - 1) / kTC) > 65535)
        return set_err(MGP_E_INVALID, w + ": too many column chunks for one call");
    const int64_t cols = std::min<int64_t>(job->n_cols, hi * job->chunk_cols) - lo * job->chunk_cols;
    if (job->first_cell < 0 || (int64_t)job->first_cell + std::max<int64_t>(cols, 0) > n_cells)
        return set_err(MGP_E_INVALID, w + ": columns outside the table's cells");
    if (job->src_bytes < 0 || (job->src_bytes > 0 && !job->src)) return set_err(MGP_E_INVALID, w + ": null or negative src");
    if (b.nch == 0) return MGP_OK;
    if (planes) {
        if ((uint64_t)job->src_bytes != (uint64_t)b.nch * b.tile_bytes)
            return set_err(MGP_E_INVALID, w + ": src_bytes is not the batch's tiles");
        return MGP_OK;
    }
    if (!job->chunk_bytes || !job->raw) return set_err(MGP_E_INVALID, w + ": null chunk_bytes or raw");
    uint64_t sum = 0;
    for (int64_t k = 0; k < b.nch; ++k) {
        const std::string at = " (chunk " + std::to_string(k) + ")";
        const int64_t cb = job->chunk_bytes[k];
        if (job->raw[k] > CH_ABSENT) return set_err(MGP_E_INVALID, w + ": unknown raw flag" + at);
        if (cb < 0 || cb >= ((int64_t)1 << 31)) return set_err(MGP_E_INVALID, w + ": chunk size out of range" + at);
        if (job->raw[k] == CH_ABSENT && cb != 0) return set_err(MGP_E_INVALID, w + ": an absent chunk with bytes" + at);
        sum += (uint64_t)cb;
    }
    if (sum != (uint64_t)job->src_bytes) return set_err(MGP_E_INVALID, w + ": chunk sizes do not add up to src_bytes");
    return MGP_OK;
}

}  // namespace

// A table context's loader: the events and buffers of mgp_table_load, kept across the calls
struct TableLoad {
    DevBuf src, tiles, meta, status, nsat;
    uint8_t* pin = nullptr;  // pinned: the streams and their tables on their way up, the statuses back
    size_t pin_cap = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // before H2D, before inflate, before and after transpose
    void release() {
        for (DevBuf* b : {&src, &tiles, &meta, &status, &nsat}) b->release();
        if (pin) (void)hipHostFree(pin);
        pin = nullptr;
        pin_cap = 0;
    }
    ~TableLoad() {
        release();
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

TableLoad* table_load_new() { return new TableLoad(); }
void table_load_free(TableLoad* t) { delete t; }

namespace {

int ensure_pin(TableLoad& t, size_t need) {
    if (need <= t.pin_cap) return MGP_OK;
    if (t.pin) (void)hipHostFree(t.pin);
    t.pin = nullptr;
    t.pin_cap = 0;
    const size_t cap = need + need / 4 + 4096;
    HIP_TRY(hipHostMalloc((void**)&t.pin, cap, hipHostMallocDefault));
    t.pin_cap = cap;
    return MGP_OK;
}

int launch_tiles(const TablePlanes& tp, const mgp_table_chunks* job, const Batch& b, const uint8_t* tiles,
                 uint64_t stride, unsigned long long* n_sat) {
    TileJob j;
    j.tiles = tiles;
    j.stride = stride;
    j.crow = job->chunk_rows;
    j.ccol = job->chunk_cols;
    j.nrc = b.nrc;
    j.ncc = b.ncc;
    j.nsc = (job->chunk_cols + kTC - 1) / kTC;
    j.L = tp.mito_len;
    j.cols_left = job->n_cols - (int64_t)job->col_chunk_lo * job->chunk_cols;
    j.first_cell = job->first_cell;
    j.c16 = tp.c16;
    j.t16 = tp.t16;
    j.d16 = tp.d16;
    j.n_sat = n_sat;
    const int nsp = (job->chunk_rows + kTP - 1) / kTP;
    const dim3 grid((unsigned)((int64_t)b.nrc * nsp), (unsigned)(b.ncc * j.nsc));  // (x < 2^24, y <= 65535: table_check)
    hipLaunchKernelGGL(tiles_to_rows, grid, dim3(kTBlock), 0, tp.stream, j);
    if (hipGetLastError() != hipSuccess) return set_err(MGP_E_HIP, "tiles_to_rows: kernel launch failed");
    return MGP_OK;
}

// One batch: streams (planes false) or inflated tiles (true)
int table_load(mgp_ctx* ctx, mgp_table_chunks* job, bool planes) {
    const char* who = planes ? "mgp_table_load_planes" : "mgp_table_load";
    TablePlanes tp;
    MGP_TRY(table_planes(ctx, who, &tp));
    MGP_TRY(table_check(who, tp.n_cells, tp.mito_len, job, planes));
    job->n_saturated = 0;
    job->ms[0] = job->ms[1] = job->ms[2] = 0.0;
    const Batch b = batch_of(job, tp.mito_len);
    if (b.nch == 0) return MGP_OK;
    TableLoad& t = *tp.load;
    const size_t n = (size_t)b.nch, nsrc = (size_t)job->src_bytes;
    // the pinned buffer: src, then coff, out_off (8 each), clen, isize (4 each), raw (1), then the statuses
    const size_t src_pad = (nsrc + 15) & ~size_t(15), mb = planes ? 0 : n * 25, mb_pad = (mb + 15) & ~size_t(15);
    for (hipEvent_t& e : t.ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    int rc = ensure_pin(t, src_pad + mb_pad + n * 4 + 16);
    if (rc == MGP_OK) rc = t.src.ensure(src_pad + 64);
    if (rc == MGP_OK && !planes) rc = t.tiles.ensure(n * b.stride + 64);
    if (rc == MGP_OK && !planes) rc = t.meta.ensure(mb_pad + 64);
    if (rc == MGP_OK && !planes) rc = t.status.ensure(n * 4);
    if (rc == MGP_OK) rc = t.nsat.ensure(8);
    if (rc != MGP_OK) {
        t.release();  // (nothing of the loader's stays allocated)
        return rc;
    }
    hipStream_t s = tp.stream;
    uint8_t* p = t.pin;
    if (nsrc) std::memcpy(p, job->src, nsrc);
    uint8_t* m = p + src_pad;
    if (!planes) {
        uint64_t* coff = reinterpret_cast<uint64_t*>(m);
        uint64_t* ooff = coff + n;
        uint32_t* clen = reinterpret_cast<uint32_t*>(m + n * 16);
        uint32_t* isz = clen + n;
        uint8_t* raw = m + n * 24;
        uint64_t at = 0;
        for (size_t k = 0; k < n; ++k) {
            coff[k] = at;
            clen[k] = (uint32_t)job->chunk_bytes[k];
            at += clen[k];
            ooff[k] = (uint64_t)k * b.stride;
            isz[k] = (uint32_t)b.tile_bytes;
            raw[k] = job->raw[k];
        }
    }
    HIP_TRY(hipMemsetAsync(t.nsat.p, 0, 8, s));
    HIP_TRY(hipEventRecord(t.ev[0], s));
    if (nsrc) HIP_TRY(hipMemcpyAsync(t.src.p, p, nsrc, hipMemcpyHostToDevice, s));
    if (!planes) HIP_TRY(hipMemcpyAsync(t.meta.p, m, mb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(t.ev[1], s));
    int32_t* hst = reinterpret_cast<int32_t*>(p + src_pad + mb_pad);
    if (!planes) {
        const uint8_t* dm = t.meta.as<uint8_t>();
        hipLaunchKernelGGL(inflate_chunks, dim3((uint32_t)n), dim3(64), 0, s, t.src.as<uint8_t>(), (const uint64_t*)dm,
                           (const uint32_t*)(dm + n * 16), (const uint32_t*)(dm + n * 20),
                           (const uint64_t*)(dm + n * 8), dm + n * 24, t.tiles.as<uint8_t>(), t.status.as<int32_t>(),
                           (uint32_t)n);
        if (hipGetLastError() != hipSuccess) return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
        HIP_TRY(hipMemcpyAsync(hst, t.status.p, n * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipEventRecord(t.ev[2], s));
    if (!planes) {  // the tiles are used only when every stream inflated
        HIP_TRY(hipStreamSynchronize(s));
        for (size_t k = 0; k < n; ++k)
            if (hst[k] != ST_OK) {
                const size_t per = (size_t)b.nrc * b.ncc;
                return set_err(MGP_E_INVALID,
                               std::string(who) + ": chunk (plane " + std::to_string(k / per) + ", row chunk " +
                                   std::to_string(k % per / b.ncc) + ", column chunk " +
                                   std::to_string(job->col_chunk_lo + (int64_t)(k % b.ncc)) + ") did not inflate: status " +
                                   std::to_string(hst[k]) + "; the table's rows of this batch stay zero");
            }
    }
    MGP_TRY(launch_tiles(tp, job, b, planes ? t.src.as<uint8_t>() : t.tiles.as<uint8_t>(),
                         planes ? b.tile_bytes : b.stride, t.nsat.as<unsigned long long>()));
    HIP_TRY(hipEventRecord(t.ev[3], s));
    unsigned long long* hsat = reinterpret_cast<unsigned long long*>(p + ((src_pad + mb_pad + n * 4 + 7) & ~size_t(7)));
    HIP_TRY(hipMemcpyAsync(hsat, t.nsat.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    job->n_saturated = (int64_t)*hsat;
    for (int k = 0; k < 3; ++k) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, t.ev[k], t.ev[k + 1]) == hipSuccess) job->ms[k] = ms;
    }
    if (planes) job->ms[1] = 0.0;  // (nothing was inflated)
    return MGP_OK;
}

struct ZArgs {
    const uint8_t* src;
    int64_t src_bytes, n;
    const uint64_t* coff;
    const uint32_t* clen;
    const uint32_t* isize;
    const uint64_t* out_off;
    uint8_t* out;
    int64_t out_bytes;
    int32_t* status;
};

// Every refusal of the probe's arguments, before any allocation or launch.
int zlib_check(const ZArgs& a) {
    const std::string w("mgp_zlib_inflate");
    if (a.n < 0 || a.src_bytes < 0 || a.out_bytes < 0) return set_err(MGP_E_INVALID, w + ": negative count");
    if (a.n > 0x7FFFFFFF) return set_err(MGP_E_INVALID, w + ": more than 2^31 - 1 streams in one call");
    if (a.n && (!a.coff || !a.clen || !a.isize || !a.out_off || !a.status)) return set_err(MGP_E_INVALID, w + ": null array");
    if ((a.src_bytes && !a.src) || (a.out_bytes && !a.out)) return set_err(MGP_E_INVALID, w + ": null buffer");
    uint64_t end = 0;  // the end of the output range before
    for (int64_t i = 0; i < a.n; ++i) {
        const std::string at = " (stream " + std::to_string(i) + ")";
        if (a.isize[i] >= 0x80000000u || a.clen[i] >= 0x80000000u)
            return set_err(MGP_E_INVALID, w + ": a stream or its output of 2^31 bytes or more" + at);
        if (a.coff[i] > (uint64_t)a.src_bytes || a.clen[i] > (uint64_t)a.src_bytes - a.coff[i])
            return set_err(MGP_E_INVALID, w + ": compressed range outside src" + at);
        if (a.out_off[i] > (uint64_t)a.out_bytes || a.isize[i] > (uint64_t)a.out_bytes - a.out_off[i])
            return set_err(MGP_E_INVALID, w + ": output range outside out" + at);
        if (a.out_off[i] < end) return set_err(MGP_E_INVALID, w + ": output ranges unsorted or overlapping" + at);
        end = a.out_off[i] + a.isize[i];
    }
    return MGP_OK;
}

// the probe's device side, with buffers, a stream of the call's own (freed by the caller's scope)
struct ZCall {
    DevBuf src, out, meta, status;
    hipStream_t s = nullptr;
    ~ZCall() {
        if (s) (void)hipStreamDestroy(s);
    }
};

int zlib_run(ZCall& z, const ZArgs& a) {
    const size_t n = (size_t)a.n;
    HIP_TRY(hipStreamCreateWithFlags(&z.s, hipStreamNonBlocking));
    MGP_TRY(z.src.ensure((size_t)a.src_bytes + 64));
    MGP_TRY(z.out.ensure((size_t)a.out_bytes + 64));
    MGP_TRY(z.meta.ensure(n * 24));
    MGP_TRY(z.status.ensure(n * 4));
    std::vector<uint8_t> m(n * 24);
    std::memcpy(m.data(), a.coff, n * 8);
    std::memcpy(m.data() + n * 8, a.out_off, n * 8);
    std::memcpy(m.data() + n * 16, a.clen, n * 4);
    std::memcpy(m.data() + n * 20, a.isize, n * 4);
    HIP_TRY(hipMemcpyAsync(z.meta.p, m.data(), n * 24, hipMemcpyHostToDevice, z.s));
    if (a.src_bytes) HIP_TRY(hipMemcpyAsync(z.src.p, a.src, (size_t)a.src_bytes, hipMemcpyHostToDevice, z.s));
    const uint8_t* dm = z.meta.as<uint8_t>();
    hipLaunchKernelGGL(inflate_chunks, dim3((uint32_t)n), dim3(64), 0, z.s, z.src.as<uint8_t>(), (const uint64_t*)dm,
                       (const uint32_t*)(dm + n * 16), (const uint32_t*)(dm + n * 20), (const uint64_t*)(dm + n * 8),
                       (const uint8_t*)nullptr, z.out.as<uint8_t>(), z.status.as<int32_t>(), (uint32_t)n);
    if (hipGetLastError() != hipSuccess) return set_err(MGP_E_HIP, "mgp_zlib_inflate: kernel launch failed");
    HIP_TRY(hipMemcpyAsync(a.status, z.status.p, n * 4, hipMemcpyDeviceToHost, z.s));
    HIP_TRY(hipStreamSynchronize(z.s));
    // the bytes of the streams that inflated (a refused one may have written a part of its
    // range on the device: it stays there)
    for (size_t i = 0; i < n; ++i)
        if (a.status[i] == ST_OK && a.isize[i])
            HIP_TRY(hipMemcpyAsync(a.out + a.out_off[i], z.out.as<uint8_t>() + a.out_off[i], a.isize[i],
                                   hipMemcpyDeviceToHost, z.s));
    HIP_TRY(hipStreamSynchronize(z.s));
    return MGP_OK;
}

}  // namespace

extern "C" {

int mgp_table_check(int32_t n_cells, int32_t mito_len, const mgp_table_chunks* job, int planes) {
    return table_check(planes ? "mgp_table_load_planes" : "mgp_table_load", n_cells, mito_len, job, planes != 0);
}

int mgp_table_load(mgp_ctx* ctx, mgp_table_chunks* job) { return table_load(ctx, job, false); }

int mgp_table_load_planes(mgp_ctx* ctx, mgp_table_chunks* job) { return table_load(ctx, job, true); }

int mgp_zlib_inflate(int device, const uint8_t* src, int64_t src_bytes, int64_t n_streams, const uint64_t* coff,
                     const uint32_t* clen, const uint32_t* isize, const uint64_t* out_off, uint8_t* out,
                     int64_t out_bytes, int32_t* status) {
    const ZArgs a{src, src_bytes, n_streams, coff, clen, isize, out_off, out, out_bytes, status};
    MGP_TRY(zlib_check(a));
    if (n_streams == 0) return MGP_OK;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
        return set_err(MGP_E_INVALID, "mgp_zlib_inflate: device " + std::to_string(device) + " not present");
    HIP_TRY(hipSetDevice(device));
    ZCall z;  // (its buffers and stream are freed on every return)
    return zlib_run(z, a);
}

}  // extern "C"
