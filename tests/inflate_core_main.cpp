// Stand-alone driver of mgp_inflate_core.h on the host (HostWave: width 1), built with
// -fsanitize=address,undefined by tests/test_inflate_core.py. Reads a corpus file
// (tests/inflate_corpus.py: write_corpus_file), inflates every case from a heap copy of
// exactly clen bytes into a heap window of exactly isize bytes (so the sanitizer sees any
// access one byte outside either), flushes the good ones into a guarded buffer at a
// rotating alignment, and compares status, bytes and guards. Prints one line per failing
// case and a summary; exit status 1 when any case fails.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "mgp_inflate_core.h"

using namespace mgp_inflate;

static bool read_u32(FILE* f, uint32_t* v) { return std::fread(v, 4, 1, f) == 1; }

int main(int argc, char** argv) {
    if (argc < 2) return std::fprintf(stderr, "usage: %s corpus.bin\n", argv[0]), 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    uint32_t n = 0;
    if (!read_u32(f, &n)) return 2;
    std::unique_ptr<Scratch> sc(new Scratch());
    const HostWave w;
    constexpr uint32_t kGuard = 64;
    uint32_t bad = 0, n_ok = 0;
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t want, isize, clen, has;
        if (!read_u32(f, &want) || !read_u32(f, &isize) || !read_u32(f, &clen) || !read_u32(f, &has)) return 2;
        // (malloc(0) may return null: one spare allocation size is avoided by new[])
        std::unique_ptr<uint8_t[]> src(new uint8_t[clen]);
        if (clen && std::fread(src.get(), 1, clen, f) != clen) return 2;
        std::vector<uint8_t> exp(has ? isize : 0);
        if (has && isize && std::fread(exp.data(), 1, isize, f) != isize) return 2;
        std::unique_ptr<uint8_t[]> win(new uint8_t[isize]);
        std::memset(win.get(), 0x5A, isize);
        std::memset(sc.get(), 0xEE, sizeof(Scratch));  // (nothing is read before it is written)
        const int32_t st = inflate(w, src.get(), clen, win.get(), isize, sc.get());
        const uint32_t shift = c & 3;
        std::vector<uint8_t> out(kGuard + shift + isize + kGuard, 0xA5);
        uint8_t* dst = out.data() + kGuard + shift;
        if (st == ST_OK) flush(w, win.get(), isize, dst);
        bool good = want == 255 ? st != ST_OK : st == (int32_t)want;
        if (good && st == ST_OK && has && isize && std::memcmp(dst, exp.data(), isize) != 0) good = false;
        for (uint32_t i = 0; i < kGuard + shift; ++i) good = good && out[i] == 0xA5;
        for (uint32_t i = 0; i < kGuard; ++i) good = good && out[kGuard + shift + isize + i] == 0xA5;
        if (st != ST_OK)
            for (uint32_t i = 0; i < isize; ++i) good = good && dst[i] == 0xA5;
        n_ok += st == ST_OK;
        if (!good) {
            ++bad;
            std::printf("FAIL case %u: status %d, expected %u (isize %u, clen %u)\n", c, st, want, isize, clen);
        }
    }
    std::fclose(f);
    std::printf("%u cases, %u inflated, %u failed\n", n, n_ok, bad);
    return bad ? 1 : 0;
}
