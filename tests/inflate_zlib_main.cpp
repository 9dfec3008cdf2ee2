// Stand-alone driver of inflate_zlib (mgp_inflate_core.h) on the host (HostWave: width 1),
// built with -fsanitize=address,undefined by tests/test_inflate_zlib.py. Reads a corpus file
// (tests/inflate_corpus.py: write_corpus_file; tests/zlib_corpus.py makes the cases), inflates
// every case from a heap copy of exactly clen bytes, through a heap ring of exactly kRing
// bytes, into a heap block of exactly shift + isize bytes at a rotating alignment (so the
// sanitizer sees any access one byte outside any of them), and compares status and bytes;
// a refused stream may have written a part of its output, never a byte before it. Prints
// one line per failing case and a summary; exit status 1 when any case fails.
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
    std::unique_ptr<uint8_t[]> ring(new uint8_t[kRing]);
    const HostWave w;
    uint32_t bad = 0, n_ok = 0;
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t want, isize, clen, has;
        if (!read_u32(f, &want) || !read_u32(f, &isize) || !read_u32(f, &clen) || !read_u32(f, &has)) return 2;
        std::unique_ptr<uint8_t[]> src(new uint8_t[clen]);
        if (clen && std::fread(src.get(), 1, clen, f) != clen) return 2;
        std::vector<uint8_t> exp(has ? isize : 0);
        if (has && isize && std::fread(exp.data(), 1, isize, f) != isize) return 2;
        std::memset(ring.get(), 0x5A, kRing);
        std::memset(sc.get(), 0xEE, sizeof(Scratch));  // (nothing is read before it is written)
        const uint32_t shift = c & 3;
        std::unique_ptr<uint8_t[]> out(new uint8_t[shift + isize]);
        std::memset(out.get(), 0xA5, shift + isize);
        uint8_t* dst = out.get() + shift;
        const int32_t st = inflate_zlib(w, src.get(), clen, ring.get(), dst, isize, sc.get());
        bool good = want == 255 ? st != ST_OK : st == (int32_t)want;
        if (good && st == ST_OK && has && isize && std::memcmp(dst, exp.data(), isize) != 0) good = false;
        for (uint32_t i = 0; i < shift; ++i) good = good && out[i] == 0xA5;
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
