// mgp_inflate.hip — BGZF blocks inflated on the device for the BAM ingest:
// the kernel, one wave per block over the decoder of mgp_inflate_core.h, and its C-ABI
// (include/mgpileup.h): mgp_bgzf_inflate with buffers of the call's own, and the
// mgp_inflater that the ingest keeps (device buffers, one stream, pinned staging) with
// mgp_inflater_run, the hook libmgphost calls per chunk (mgp_bam_set_inflater). CRC32
// stays on the host.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mgpileup.h"
#include "mgp_host.h"
#include "mgp_inflate_core.h"

namespace {

using namespace mgp_inflate;

// The wave of the kernel: a workgroup is one wave of 64 lanes, so the workgroup barrier
// is the wave's own (it orders the LDS and global accesses of its lanes).
struct DeviceWave {
    __device__ uint32_t lane() const { return threadIdx.x; }
    __device__ uint32_t width() const { return 64; }
    __device__ bool leader() const { return threadIdx.x == 0; }
    __device__ void sync() const { __syncthreads(); }
};

// Block b = blockIdx.x: src[coff[b], + clen[b]) into out[out_off[b], + isize[b]) through the
// LDS window; a refused block writes its status alone. The host checked every range against
// src and out (check_args) before the launch.
__global__ __launch_bounds__(64) void inflate_blocks(const uint8_t* __restrict__ src, const uint64_t* __restrict__ coff,
                                                     const uint32_t* __restrict__ clen,
                                                     const uint32_t* __restrict__ isize,
                                                     const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out,
                                                     int32_t* __restrict__ status, uint32_t n_blocks) {
    __shared__ Scratch sc;
    __shared__ alignas(16) uint8_t win[kMaxIsize];
    const uint32_t b = blockIdx.x;
    if (b >= n_blocks) return;
    const DeviceWave w;
    const uint32_t n = isize[b];
    const int32_t st = inflate(w, src + coff[b], clen[b], win, n, &sc);
    if (st == ST_OK) flush(w, win, n, out + out_off[b]);
    if (w.leader()) status[b] = st;
}

struct Args {
    const uint8_t* src;
    int64_t src_bytes, n_blocks;
    const uint64_t* coff;
    const uint32_t* clen;
    const uint32_t* isize;
    const uint64_t* out_off;
    uint8_t* out;
    int64_t out_bytes;
    int32_t* status;
};

// Every refusal of the arguments, before any allocation or launch.
int check_args(const char* who, const Args& a) {
    const std::string w(who);
    if (a.n_blocks < 0 || a.src_bytes < 0 || a.out_bytes < 0) return set_err(MGP_E_INVALID, w + ": negative count");
    if (a.n_blocks > 0x7FFFFFFF) return set_err(MGP_E_INVALID, w + ": more than 2^31 - 1 blocks in one call");
    if (a.n_blocks && (!a.coff || !a.clen || !a.isize || !a.out_off || !a.status))
        return set_err(MGP_E_INVALID, w + ": null array");
    if ((a.src_bytes && !a.src) || (a.out_bytes && !a.out)) return set_err(MGP_E_INVALID, w + ": null buffer");
    uint64_t end = 0;  // the end of the output range before
    for (int64_t i = 0; i < a.n_blocks; ++i) {
        const std::string at = " (block " + std::to_string(i) + ")";
        if (a.isize[i] > kMaxIsize) return set_err(MGP_E_INVALID, w + ": isize above 65536" + at);
        if (a.coff[i] > (uint64_t)a.src_bytes || a.clen[i] > (uint64_t)a.src_bytes - a.coff[i])
            return set_err(MGP_E_INVALID, w + ": compressed range outside src" + at);
        if (a.out_off[i] > (uint64_t)a.out_bytes || a.isize[i] > (uint64_t)a.out_bytes - a.out_off[i])
            return set_err(MGP_E_INVALID, w + ": output range outside out" + at);
        if (a.out_off[i] < end) return set_err(MGP_E_INVALID, w + ": output ranges unsorted or overlapping" + at);
        end = a.out_off[i] + a.isize[i];
    }
    return MGP_OK;
}

}  // namespace

// Device buffers, the stream and the pinned staging of the block tables, kept across calls.
struct mgp_inflater {
    int device = 0;
    int64_t max_src = 0, max_out = 0;
    hipStream_t s = nullptr;
    DevBuf src, out, meta, status;
    uint8_t* pin = nullptr;  // the block tables on their way up, the statuses on their way back
    size_t pin_cap = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // before H2D, before and after the kernel, after D2H
    double ms[3] = {0, 0, 0};                                  // summed over the calls (mgp_inflater_times)
    int64_t calls = 0, blocks = 0;
    ~mgp_inflater() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (pin) (void)hipHostFree(pin);
        if (s) (void)hipStreamDestroy(s);
    }
};

namespace {

// bytes of the tables of n blocks: coff, out_off (8 each), clen, isize (4 each); the
// statuses follow in the pinned buffer
size_t meta_bytes(int64_t n) { return (size_t)n * 24; }

int inflater_run(mgp_inflater* inf, const char* who, const Args& a) {
    MGP_TRY(check_args(who, a));
    if (a.src_bytes > inf->max_src || a.out_bytes > inf->max_out)
        return set_err(MGP_E_INVALID, std::string(who) + ": more bytes than the inflater was created for");
    const int64_t n = a.n_blocks;
    if (n == 0) return MGP_OK;
    HIP_TRY(hipSetDevice(inf->device));
    const size_t mb = meta_bytes(n), need = mb + (size_t)n * 4;
    if (need > inf->pin_cap) {
        if (inf->pin) (void)hipHostFree(inf->pin);
        inf->pin = nullptr;
        inf->pin_cap = 0;
        const size_t cap = need + need / 2;
        HIP_TRY(hipHostMalloc((void**)&inf->pin, cap, hipHostMallocDefault));
        inf->pin_cap = cap;
    }
    MGP_TRY(inf->meta.ensure(mb));
    MGP_TRY(inf->status.ensure((size_t)n * 4));
    uint8_t* p = inf->pin;
    std::memcpy(p, a.coff, (size_t)n * 8);
    std::memcpy(p + (size_t)n * 8, a.out_off, (size_t)n * 8);
    std::memcpy(p + (size_t)n * 16, a.clen, (size_t)n * 4);
    std::memcpy(p + (size_t)n * 20, a.isize, (size_t)n * 4);
    hipStream_t s = inf->s;
    HIP_TRY(hipEventRecord(inf->ev[0], s));
    HIP_TRY(hipMemcpyAsync(inf->meta.p, p, mb, hipMemcpyHostToDevice, s));
    if (a.src_bytes) HIP_TRY(hipMemcpyAsync(inf->src.p, a.src, (size_t)a.src_bytes, hipMemcpyHostToDevice, s));
    const uint8_t* dm = inf->meta.as<uint8_t>();
    HIP_TRY(hipEventRecord(inf->ev[1], s));
    hipLaunchKernelGGL(inflate_blocks, dim3((uint32_t)n), dim3(64), 0, s, inf->src.as<uint8_t>(),
                       (const uint64_t*)dm, (const uint32_t*)(dm + (size_t)n * 16),
                       (const uint32_t*)(dm + (size_t)n * 20), (const uint64_t*)(dm + (size_t)n * 8),
                       inf->out.as<uint8_t>(), inf->status.as<int32_t>(), (uint32_t)n);
    if (hipGetLastError() != hipSuccess) return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
    HIP_TRY(hipEventRecord(inf->ev[2], s));
    // the blocks' bytes back, one copy per run of abutting ranges (a chunk of the ingest is
    // one run), so nothing outside the blocks' ranges is written in out
    for (int64_t i = 0; i < n;) {
        const uint64_t lo = a.out_off[i];
        uint64_t hi = lo + a.isize[i];
        int64_t j = i + 1;
        while (j < n && a.out_off[j] == hi) hi += a.isize[j++];
        if (hi > lo)
            HIP_TRY(hipMemcpyAsync(a.out + lo, inf->out.as<uint8_t>() + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, s));
        i = j;
    }
    HIP_TRY(hipMemcpyAsync(p + mb, inf->status.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(inf->ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 3; ++k) {
        float t = 0;
        if (hipEventElapsedTime(&t, inf->ev[k], inf->ev[k + 1]) == hipSuccess) inf->ms[k] += t;
    }
    inf->calls += 1;
    inf->blocks += n;
    std::memcpy(a.status, p + mb, (size_t)n * 4);
    return MGP_OK;
}

int inflater_create(int device, int64_t max_src_bytes, int64_t max_out_bytes, mgp_inflater** out) {
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
        return set_err(MGP_E_INVALID, "mgp_inflater_create: device " + std::to_string(device) + " not present");
    HIP_TRY(hipSetDevice(device));
    mgp_inflater* inf = new mgp_inflater();
    inf->device = device;
    inf->max_src = max_src_bytes;
    inf->max_out = max_out_bytes;
    int rc = MGP_OK;
    hipError_t e = hipStreamCreateWithFlags(&inf->s, hipStreamNonBlocking);
    if (e != hipSuccess) rc = set_err(MGP_E_HIP, std::string("mgp_inflater_create: ") + hipGetErrorString(e));
    for (hipEvent_t& ev : inf->ev)
        if (rc == MGP_OK && (e = hipEventCreate(&ev)) != hipSuccess)
            rc = set_err(MGP_E_HIP, std::string("mgp_inflater_create: ") + hipGetErrorString(e));
    if (rc == MGP_OK) rc = inf->src.ensure((size_t)max_src_bytes + 64);
    if (rc == MGP_OK) rc = inf->out.ensure((size_t)max_out_bytes + 64);
    if (rc != MGP_OK) {
        delete inf;  // (nothing stays allocated)
        return rc;
    }
    *out = inf;
    return MGP_OK;
}

}  // namespace

extern "C" {

int mgp_inflater_create(int device, int64_t max_src_bytes, int64_t max_out_bytes, mgp_inflater** out) {
    if (!out || max_src_bytes < 0 || max_out_bytes < 0 || max_src_bytes > ((int64_t)1 << 40) ||
        max_out_bytes > ((int64_t)1 << 40))
        return set_err(MGP_E_INVALID, "mgp_inflater_create: bad arguments");
    *out = nullptr;
    return inflater_create(device, max_src_bytes, max_out_bytes, out);
}

void mgp_inflater_destroy(mgp_inflater* inf) {
    if (!inf) return;
    (void)hipSetDevice(inf->device);
    if (inf->s) (void)hipStreamSynchronize(inf->s);
    delete inf;
}

int mgp_inflater_run(void* inflater, const uint8_t* src, int64_t src_bytes, int64_t n_blocks, const uint64_t* coff,
                     const uint32_t* clen, const uint32_t* isize, const uint64_t* out_off, uint8_t* out,
                     int64_t out_bytes, int32_t* status) {
    if (!inflater) return set_err(MGP_E_INVALID, "mgp_inflater_run: null inflater");
    const Args a{src, src_bytes, n_blocks, coff, clen, isize, out_off, out, out_bytes, status};
    return inflater_run(static_cast<mgp_inflater*>(inflater), "mgp_inflater_run", a);
}

int mgp_bgzf_inflate(int device, const uint8_t* src, int64_t src_bytes, int64_t n_blocks, const uint64_t* coff,
                     const uint32_t* clen, const uint32_t* isize, const uint64_t* out_off, uint8_t* out,
                     int64_t out_bytes, int32_t* status) {
    const Args a{src, src_bytes, n_blocks, coff, clen, isize, out_off, out, out_bytes, status};
    MGP_TRY(check_args("mgp_bgzf_inflate", a));
    if (n_blocks == 0) return MGP_OK;
    mgp_inflater* inf = nullptr;
    MGP_TRY(inflater_create(device, src_bytes, out_bytes, &inf));
    const int rc = inflater_run(inf, "mgp_bgzf_inflate", a);
    mgp_inflater_destroy(inf);
    return rc;
}

int mgp_inflater_times(mgp_inflater* inf, double* ms3, int64_t* calls, int64_t* blocks) {
    if (!inf || !ms3) return set_err(MGP_E_INVALID, "mgp_inflater_times: null argument");
    for (int k = 0; k < 3; ++k) ms3[k] = inf->ms[k];
    if (calls) *calls = inf->calls;
    if (blocks) *blocks = inf->blocks;
    return MGP_OK;
}

// Pinned memory in the shape of the ingest hook's allocators (mgp_bam_inflater.alloc /
// .release, include/mgpileup_host.h): null when the allocation fails.
void* mgp_inflater_host_alloc(int64_t bytes) {
    void* p = nullptr;
    return mgp_host_alloc(bytes, &p) == MGP_OK ? p : nullptr;
}
void mgp_inflater_host_release(void* p) { (void)mgp_host_free(p); }

}  // extern "C"
