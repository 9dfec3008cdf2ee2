// Host link probe: H2D alone, D2H alone and both at once (pinned host memory,
// hipMemcpyAsync in 256 MiB pieces on one stream per direction), and H2D beside a
// kernel that writes to mapped pinned memory (as k_rows_to_host does); and a kernel that
// pulls mapped pinned host memory into device memory (instead of the copy engine), alone
// and beside the copy engine's D2H or the host-writing kernel.
// Every concurrent case prints each direction's own rate (events on its stream) beside the
// joint end. Then two questions about the streamed rows:
//   paced:  the host-writing kernel held to R GB/s by a schedule against wall_clock64(),
//           beside H2D: what rate does H2D keep?
//   shape:  the engine's store shape (8/2/1-byte lanes, 11 bytes per position in three
//           planes, rows at the odd pitch 16569, 13 segments of 1275 positions) against
//           the same bytes in 16-byte lanes on 64-byte-aligned addresses, alone and beside H2D.
//   hipcc --offload-arch=gfx950 -O2 scripts/probe_pcie.hip -o /tmp/probe_pcie && /tmp/probe_pcie [reps]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

__global__ void k_write_host(uint4* __restrict__ h, const uint4* __restrict__ d, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) h[i] = d[i];
}

__global__ void k_read_host(uint4* __restrict__ d, const uint4* __restrict__ h, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        d[i] = h[i];
}

// k_write_host on a schedule: slice s (one workgroup's 256 x 16 bytes) is not stored before
// t0 + s * ticks_q16 / 65536 on the device's wall clock; t0 is the first workgroup's start
// (*t0w is 0 at launch). nslice slices over a buffer of n uint4 (wrapping). ticks_q16 = 0
// runs free. A wait never outlasts max_ticks past t0.
__global__ void __launch_bounds__(256) k_write_host_paced(uint4* __restrict__ h, const uint4* __restrict__ d, size_t n,
                                                           size_t nslice, unsigned long long ticks_q16,
                                                           unsigned long long max_ticks,
                                                           unsigned long long* __restrict__ t0w) {
    __shared__ unsigned long long t0s;
    if (threadIdx.x == 0) {
        const unsigned long long now = wall_clock64();
        const unsigned long long old = atomicCAS(t0w, 0ull, now);
        t0s = old ? old : now;
    }
    __syncthreads();
    const unsigned long long t0 = t0s;
    for (size_t s = blockIdx.x; s < nslice; s += gridDim.x) {
        if (ticks_q16) {
            const unsigned long long due = std::min((unsigned long long)((s * ticks_q16) >> 16), max_ticks);
            while (wall_clock64() - t0 < due) __builtin_amdgcn_s_sleep(8);
        }
        const size_t i = (s * 256 + threadIdx.x) % n;
        h[i] = d[i];
    }
}

// the engine's k_rows_to_host8 on a window that fits bytes: one lane per position, 8 + 2 + 1
// bytes into three planes, rows at pitch L
__global__ void __launch_bounds__(256) k_rows_shape(int L, int nc, int p0, int p1, const uint2* __restrict__ dc,
                                                     const uint16_t* __restrict__ dt, const uint8_t* __restrict__ dd,
                                                     uint2* __restrict__ hc, uint16_t* __restrict__ ht,
                                                     uint8_t* __restrict__ hd) {
    const int p = p0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= p1) return;
    for (int c = blockIdx.y; c < nc; c += gridDim.y) {
        const size_t P = (size_t)c * L + p;
        hc[P] = dc[P];
        ht[P] = dt[P];
        hd[P] = dd[P];
    }
}

// the same bytes in 16-byte lanes: a cell's chunk of a plane is q uint4 at pitch pq uint4,
// from o (all multiples of 4 uint4: whole 64-byte lines)
__device__ __forceinline__ void plane16(const uint4* __restrict__ d, uint4* __restrict__ h, size_t pq, size_t o, int q,
                                        int nc) {
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (x >= q) return;
    for (int c = blockIdx.y; c < nc; c += gridDim.y) h[(size_t)c * pq + o + x] = d[(size_t)c * pq + o + x];
}
__global__ void __launch_bounds__(256) k_rows_lines(int Lp, int nc, int p0, int w, const uint4* __restrict__ dc,
                                                     const uint4* __restrict__ dt, const uint4* __restrict__ dd,
                                                     uint4* __restrict__ hc, uint4* __restrict__ ht, uint4* __restrict__ hd) {
    plane16(dc, hc, (size_t)Lp / 2, (size_t)p0 / 2, w / 2, nc);
    plane16(dt, ht, (size_t)Lp / 8, (size_t)p0 / 8, w / 8, nc);
    plane16(dd, hd, (size_t)Lp / 16, (size_t)p0 / 16, w / 16, nc);
}

struct Res { double a, b, joint; };  // seconds: stream a's work, stream b's work, host clock over both

int main(int argc, char** argv) {
    const int reps = argc > 1 ? std::max(1, atoi(argv[1])) : 3;
    const size_t N = 4ull << 30, P = 256ull << 20;
    void *h1, *h2, *d1, *d2;
    unsigned long long* t0w;
    CK(hipHostMalloc(&h1, N, hipHostMallocDefault));
    CK(hipHostMalloc(&h2, N, hipHostMallocDefault));
    CK(hipMalloc(&d1, N));
    CK(hipMalloc(&d2, N));
    CK(hipMalloc(&t0w, 8));
    memset(h1, 1, N);
    memset(h2, 2, N);
    CK(hipMemset(d2, 3, N));
    int khz = 0;
    CK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0));
    printf("wall clock %d kHz, %d repeats\n", khz, reps);
    hipStream_t a, b;
    CK(hipStreamCreateWithFlags(&a, hipStreamNonBlocking));
    CK(hipStreamCreateWithFlags(&b, hipStreamNonBlocking));
    hipEvent_t ea0, ea1, eb0, eb1;
    CK(hipEventCreate(&ea0)); CK(hipEventCreate(&ea1)); CK(hipEventCreate(&eb0)); CK(hipEventCreate(&eb1));
    // fa's work on stream a, fb's on stream b, both started together; each stream's own time
    auto both = [&](const std::function<void()>& fa, const std::function<void()>& fb) -> Res {
        CK(hipDeviceSynchronize());
        auto t0 = std::chrono::steady_clock::now();
        CK(hipEventRecord(ea0, a));
        CK(hipEventRecord(eb0, b));
        if (fa) fa();
        CK(hipEventRecord(ea1, a));
        if (fb) fb();
        CK(hipEventRecord(eb1, b));
        CK(hipDeviceSynchronize());
        Res r;
        r.joint = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        float ms;
        CK(hipEventElapsedTime(&ms, ea0, ea1)); r.a = ms * 1e-3;
        CK(hipEventElapsedTime(&ms, eb0, eb1)); r.b = ms * 1e-3;
        return r;
    };
    auto h2d = [&](int times) { return [&, times]() {
        for (int k = 0; k < times; ++k)
            for (size_t o = 0; o < N; o += P) CK(hipMemcpyAsync((char*)d1 + o, (char*)h1 + o, P, hipMemcpyHostToDevice, a));
    }; };
    auto d2h = [&]() { for (size_t o = 0; o < N; o += P) CK(hipMemcpyAsync((char*)h2 + o, (char*)d2 + o, P, hipMemcpyDeviceToHost, b)); };
    auto kwr = [&](int wg) { return [&, wg]() { k_write_host<<<wg, 256, 0, b>>>((uint4*)h2, (const uint4*)d2, N / 16); }; };
    auto pull = [&](int wg) { return [&, wg]() { k_read_host<<<wg, 256, 0, a>>>((uint4*)d1, (const uint4*)h1, N / 16); }; };
    const double G = 1e9;

    // ---- the rows' store shape: C4's 8-bit target, 10k cells x 16569 positions in 13 segments
    const int L = 16569, nc = 10000, nseg = 13, segw = 1275;  // 13 * 1275 = 16575 >= L
    const int Lp = 16640, segwp = 1280;                       // the aligned twin: 13 * 1280, whole lines
    const size_t oc = 0, ot = 1536ull << 20, od = 2048ull << 20;  // plane offsets in h2 / d2
    static_assert((size_t)10000 * 16640 * 8 <= (1536ull << 20), "counts plane");
    static_assert((1536ull << 20) + (size_t)10000 * 16640 * 2 <= (2048ull << 20), "tn5 plane");
    static_assert((2048ull << 20) + (size_t)10000 * 16640 <= (4ull << 30), "depth plane");
    const double shape_bytes = (double)nc * L * 11, lines_bytes = (double)nc * Lp * 11;
    auto rows_shape = [&](int rounds) { return [&, rounds]() {
        for (int r = 0; r < rounds; ++r)
            for (int s = 0; s < nseg; ++s) {
                const int p0 = s * segw, p1 = std::min(L, p0 + segw);
                const unsigned gx = (unsigned)((p1 - p0 + 255) / 256);
                k_rows_shape<<<dim3(gx, 256 / gx), 256, 0, b>>>(L, nc, p0, p1, (const uint2*)((char*)d2 + oc),
                    (const uint16_t*)((char*)d2 + ot), (const uint8_t*)((char*)d2 + od), (uint2*)((char*)h2 + oc),
                    (uint16_t*)((char*)h2 + ot), (uint8_t*)((char*)h2 + od));
            }
    }; };
    auto rows_lines = [&](int rounds) { return [&, rounds]() {
        for (int r = 0; r < rounds; ++r)
            for (int s = 0; s < nseg; ++s) {
                const unsigned gx = (unsigned)((segwp / 2 + 255) / 256);
                k_rows_lines<<<dim3(gx, 256 / gx), 256, 0, b>>>(Lp, nc, s * segwp, segwp, (const uint4*)((char*)d2 + oc),
                    (const uint4*)((char*)d2 + ot), (const uint4*)((char*)d2 + od), (uint4*)((char*)h2 + oc),
                    (uint4*)((char*)h2 + ot), (uint4*)((char*)h2 + od));
            }
    }; };
    // ---- the paced writer: R GB/s for about T seconds (free: 6 GiB), 128 workgroups
    auto paced = [&](double R) { return [&, R]() {
        const double T = 0.13;
        const size_t nslice = R > 0 ? (size_t)(R * G * T / 4096) : (6ull << 30) / 4096;
        const double ticks = R > 0 ? 4096.0 / (R * G) * khz * 1e3 : 0.0;
        CK(hipMemsetAsync(t0w, 0, 8, b));
        k_write_host_paced<<<128, 256, 0, b>>>((uint4*)h2, (const uint4*)d2, N / 16, nslice,
            (unsigned long long)(ticks * 65536.0), (unsigned long long)(2.0 * T * khz * 1e3), t0w);
    }; };
    auto paced_bytes = [&](double R) { return R > 0 ? (double)((size_t)(R * G * 0.13 / 4096)) * 4096 : (double)(6ull << 30); };

    for (int rep = 0; rep < reps; ++rep) {
        Res r;
        printf("---- repeat %d\n", rep);
        r = both(h2d(1), nullptr);  printf("H2D alone          %6.1f GB/s\n", N / r.a / G);
        r = both(nullptr, d2h);     printf("D2H alone          %6.1f GB/s\n", N / r.b / G);
        r = both(h2d(1), d2h);      printf("H2D + D2H          H2D %6.1f  D2H %6.1f GB/s (joint end %.3f s: %.1f GB/s each)\n", N / r.a / G, N / r.b / G, r.joint, N / r.joint / G);
        r = both(nullptr, kwr(256));  printf("kernel writes host %6.1f GB/s (256 WGs)\n", N / r.b / G);
        r = both(nullptr, kwr(2048)); printf("kernel writes host %6.1f GB/s (2048 WGs)\n", N / r.b / G);
        r = both(h2d(1), kwr(256));   printf("H2D + kernel wr    H2D %6.1f  wr %6.1f GB/s (joint end %.3f s: %.1f GB/s each)\n", N / r.a / G, N / r.b / G, r.joint, N / r.joint / G);
        for (int wg : {256, 1024, 4096}) {
            r = both(pull(wg), nullptr); printf("kernel pulls host  %6.1f GB/s (%d WGs)\n", N / r.a / G, wg);
        }
        r = both(pull(1024), d2h);      printf("pull + D2H         pull %6.1f  D2H %6.1f GB/s (joint end %.3f s)\n", N / r.a / G, N / r.b / G, r.joint);
        r = both(pull(1024), kwr(256)); printf("pull + kernel wr   pull %6.1f  wr %6.1f GB/s (joint end %.3f s)\n", N / r.a / G, N / r.b / G, r.joint);
        // (b) the writer outlasts the 4 GiB of H2D in every case: H2D's rate is its rate beside the writer
        for (double R : {0.0, 40.0, 30.0, 20.0, 15.0, 10.0, 5.0}) {
            r = both(nullptr, paced(R));
            const double alone = paced_bytes(R) / r.b / G;
            r = both(h2d(1), paced(R));
            printf("paced wr %4.0f GB/s  alone %6.1f  | beside H2D: H2D %6.1f  wr %6.1f GB/s (wr ran %.3f s, H2D %.3f s)\n", R, alone,
                   N / r.a / G, paced_bytes(R) / r.b / G, r.b, r.a);
        }
        // (c) three rounds of the 13 segments outlast 4 GiB of H2D (H2D's rate beside the writer);
        // 8 GiB of H2D outlast one round (the writer's rate beside H2D)
        r = both(nullptr, rows_shape(1)); printf("rows 8/2/1 B odd   alone %6.1f GB/s\n", shape_bytes / r.b / G);
        r = both(nullptr, rows_lines(1)); printf("rows 16 B aligned  alone %6.1f GB/s\n", lines_bytes / r.b / G);
        r = both(h2d(1), rows_shape(3));  printf("rows 8/2/1 B odd   beside H2D: H2D %6.1f GB/s (wr ran %.3f s, H2D %.3f s)\n", N / r.a / G, r.b, r.a);
        r = both(h2d(1), rows_lines(3));  printf("rows 16 B aligned  beside H2D: H2D %6.1f GB/s (wr ran %.3f s, H2D %.3f s)\n", N / r.a / G, r.b, r.a);
        r = both(h2d(2), rows_shape(1));  printf("rows 8/2/1 B odd   beside H2D: wr  %6.1f GB/s (wr ran %.3f s, H2D %.3f s)\n", shape_bytes / r.b / G, r.b, r.a);
        r = both(h2d(2), rows_lines(1));  printf("rows 16 B aligned  beside H2D: wr  %6.1f GB/s (wr ran %.3f s, H2D %.3f s)\n", lines_bytes / r.b / G, r.b, r.a);
        fflush(stdout);
    }
    return 0;
}
