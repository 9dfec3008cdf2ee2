// mgp_inflate_core.h — the raw-deflate (RFC 1951) decoder of the device inflate, one BGZF
// block per wave (mgp_inflate.hip), in a form that also compiles for the host: header
// parse, table build, symbol decode, the copies and every bounds decision are here, and
// the wave enters only through W (lane, width, leader, sync): the device's W is a
// 64-lane wave, the host's (HostWave below) is width 1. tests/inflate_core_main.cpp runs
// this very code under the sanitizers.
//
// How a wave works a block: every lane runs the whole decode with the same values (the
// bit reader, the tables' lookups and the branches are uniform), the stores of a
// uniform value are the leader's, and the parts with width are shared out by lane: the
// input window's refill, the tables' fill and the match copies. The output of the block
// is staged in `win` (isize bytes: LDS on the device) and flushed to the caller's bytes
// only once the stream has ended well, so a refused block writes nothing.
//
// Bounds, all explicit:
//   input   src[i] is read only in fill_window and the stored copy, both under i < clen
//   output  win[i] is written under i < isize (lit: op < isize; copies: op + len <= isize)
//           and read under i < op (match sources: dist <= op)
//   loops   the symbol loop ends on its budget of 8 * clen + 64 steps at the latest (each
//           step takes at least one bit or ends); the table builders run to 19, 288 (the
//           fixed code's 288, a dynamic code's <= 286) and 32 (30); the slow decode to 15
//           lengths; a copy to its length (<= 258, or a stored LEN <= 65535)
//   tables  every index is masked or compared against the table's size before use
// Strictness follows zlib's inflate: a code-length code must be complete; a literal/length
// or distance code may be incomplete only as one code of one bit; a distance code may be
// empty (a match then is an error); over-subscribed codes, HLIT > 286 and HDIST > 30 are
// errors. An unused code decoded from an incomplete set is an error.
//
// inflate_zlib (below inflate) is the streaming form for the HDF5 chunks (mgp_table.hip):
// a whole zlib stream (RFC 1950) of any size below 2^31, its output staged in a ring of
// kRing bytes and flushed to the caller's bytes half by half, Adler-32 checked. It shares
// the bit reader, the header parse, the table build and the symbol decode with inflate.
// Bounds, all explicit:
//   input   src[i] is read under i < clen: the two header bytes and the four of the trailer
//           after clen >= 6 / pos + 4 <= clen, the rest through fill_window and the stored
//           copy as above (over src + 2, clen - 2)
//   ring    every index is masked with & (kRing - 1); a step writes [op, op + n) with
//           n <= kHalf - (op - flushed) for a stored piece and n <= 258 for a match, and
//           op - flushed < kHalf holds before every step, so the bytes written, at most
//           kHalf + 257 past flushed, never reach the unflushed bytes one turn behind
//           (flushed + kRing) nor the match sources [op - kHalf, op): dist <= 32768 = kHalf
//           and dist <= op (the refusal), so a source byte was written by this stream
//   dst     written only by flush_ring, [flushed, flushed + n) with flushed + n <= op <= isize
//           (lit: op < isize; copies: len <= isize - op)
//   loops   the symbol loop on the same budget of 8 * clen + 64 steps; a stored block in
//           at most 3 pieces (LEN <= 65535 < 2 * kHalf); the Adler sums over a piece of
//           n <= kHalf bytes: per lane s1 <= 255 * n, s2 <= 255 * n * n < 2^38 in u64
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MGPI_HD __host__ __device__
#else
#define MGPI_HD
#endif

namespace mgp_inflate {

enum : int32_t { ST_OK = 0, ST_INVALID = 1, ST_SIZE = 2, ST_CHECK = 3 };  // (3: inflate_zlib's alone)

constexpr uint32_t kMaxIsize = 65536;
constexpr uint32_t kRing = 65536, kHalf = 32768;  // inflate_zlib's staging ring and its flush unit
constexpr uint32_t kAdlerMod = 65521;
constexpr uint32_t kMaxLanes = 64;  // the widest W (Scratch::red)
constexpr uint32_t kInWin = 4096;  // bytes of the compressed stream staged at a time
constexpr uint32_t kLitBits = 10, kDistBits = 8, kClBits = 7;
constexpr uint32_t kMaxLit = 288, kMaxDist = 32, kMaxCl = 19;

// A canonical Huffman code: the primary table (entry = symbol << 4 | length, 0 = not a
// code of <= bits bits) and, for the longer codes and the refusals, count[] / sorted[] read
// length by length.
struct Huff {
    uint16_t count[16];
    uint16_t first[16];  // first code of each length
    uint16_t offs[16];   // index in sorted of each length's first symbol
    uint16_t sorted[kMaxLit];
};

// The decoder's memory besides win: LDS on the device.
struct Scratch {
    alignas(16) uint8_t inwin[kInWin];
    uint16_t lit_tab[1u << kLitBits];
    uint16_t dist_tab[1u << kDistBits];
    uint16_t cl_tab[1u << kClBits];
    Huff lit, dist, cl;
    uint8_t lens[kMaxLit + kMaxDist];  // code lengths: literal/length then distance
    uint8_t cl_lens[kMaxCl + 1];
    uint32_t red[2 * kMaxLanes];  // inflate_zlib: the lanes' Adler-32 sums of a flushed piece
};

struct HostWave {
    MGPI_HD uint32_t lane() const { return 0; }
    MGPI_HD uint32_t width() const { return 1; }
    MGPI_HD bool leader() const { return true; }
    MGPI_HD void sync() const {}
};

// The bit reader over src[0, clen), through the window s->inwin = src[wbase, wbase + kInWin)
// (zero past clen). ip: the next byte to enter bitbuf; (ip - wbase) stays a multiple of 4.
struct Bits {
    const uint8_t* src;
    uint32_t clen;
    uint64_t bitbuf = 0;
    uint32_t bitcnt = 0;
    uint32_t ip = 0;
    uint32_t wbase = 0, wend = 0;  // window = [wbase, wend); empty at the start
};

template <class W>
MGPI_HD inline void fill_window(const W& w, Bits& b, Scratch* s) {
    w.sync();  // (the window's earlier readers are done)
    b.wbase = b.ip;
    b.wend = b.ip + kInWin;
    for (uint32_t i = w.lane(); i < kInWin; i += w.width()) {
        const uint32_t g = b.wbase + i;  // (ip <= clen <= 2^32 - 1 - kInWin is checked by the caller of inflate)
        s->inwin[i] = g < b.clen ? b.src[g] : (uint8_t)0;
    }
    w.sync();
}

// Brings bitcnt above 32 while input remains: at most two words.
template <class W>
MGPI_HD inline void refill(const W& w, Bits& b, Scratch* s) {
    for (int k = 0; k < 2; ++k) {
        if (b.bitcnt > 32 || b.ip >= b.clen) return;
        if (b.ip >= b.wend) fill_window(w, b, s);
        const uint32_t o = b.ip - b.wbase;  // < kInWin, multiple of 4
        const uint32_t word = (uint32_t)s->inwin[o] | (uint32_t)s->inwin[o + 1] << 8 | (uint32_t)s->inwin[o + 2] << 16 |
                              (uint32_t)s->inwin[o + 3] << 24;
        const uint32_t left = b.clen - b.ip;
        const uint32_t nb = left < 4 ? left : 4;
        b.bitbuf |= (uint64_t)word << b.bitcnt;  // (bytes past clen are zero in the window)
        b.bitcnt += 8 * nb;
        b.ip += nb;
    }
}

MGPI_HD inline uint32_t peek(const Bits& b, uint32_t n) { return (uint32_t)(b.bitbuf & ((1ull << n) - 1)); }
MGPI_HD inline void drop(Bits& b, uint32_t n) {
    b.bitbuf >>= n;
    b.bitcnt -= n;
}

MGPI_HD inline uint32_t bitrev(uint32_t v, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < 15; ++i) {
        if (i < n) r |= ((v >> i) & 1u) << (n - 1 - i);
    }
    return r;
}

// Builds h and tab (1 << bits entries) from lens[0, nsym), nsym <= cap <= kMaxLit, every
// length <= 15. is_codes: the code-length code (must be complete). Returns ST_OK or
// ST_INVALID, the same in every lane.
template <class W>
MGPI_HD inline int32_t build(const W& w, const uint8_t* lens, uint32_t nsym, uint32_t cap, bool is_codes, Huff* h,
                             uint16_t* tab, uint32_t bits) {
    if (nsym > cap) nsym = cap;
    const uint32_t tsize = 1u << bits;
    w.sync();  // (lens written, earlier tables' readers done)
    // count[l], one length per lane
    for (uint32_t l = w.lane(); l < 16; l += w.width()) {
        uint32_t c = 0;
        for (uint32_t i = 0; i < nsym; ++i) c += (lens[i] & 15u) == l;
        h->count[l] = (uint16_t)c;
    }
    for (uint32_t i = w.lane(); i < tsize; i += w.width()) tab[i] = 0;
    w.sync();
    uint32_t maxlen = 0;
    int32_t left = 1;
    bool over = false;
    for (uint32_t l = 1; l < 16; ++l) {
        const uint32_t c = h->count[l];
        if (c) maxlen = l;
        left <<= 1;
        left -= (int32_t)c;
        if (left < 0) {
            over = true;
            left = 0;  // (keeps the shifts small; the verdict is made)
        }
    }
    if (over) return ST_INVALID;
    if (maxlen == 0) return is_codes ? ST_INVALID : ST_OK;  // no code at all: every lookup refuses
    if (left > 0 && (is_codes || maxlen != 1)) return ST_INVALID;
    if (w.leader()) {
        uint32_t code = 0, off = 0;
        h->first[0] = 0;
        h->offs[0] = 0;
        for (uint32_t l = 1; l < 16; ++l) {
            code = (code + h->count[l - 1] * (l > 1)) << 1;
            h->first[l] = (uint16_t)code;
            h->offs[l] = (uint16_t)off;
            off += h->count[l];
        }
    }
    w.sync();
    // sorted[]: the symbols of each length in symbol order, one length per lane
    for (uint32_t l = 1 + w.lane(); l < 16; l += w.width()) {
        uint32_t k = h->offs[l];
        const uint32_t end = k + h->count[l];  // <= nsym <= kMaxLit
        for (uint32_t i = 0; i < nsym; ++i)
            if ((lens[i] & 15u) == l && k < end && k < kMaxLit) h->sorted[k++] = (uint16_t)i;
    }
    w.sync();
    // primary table: sorted index j has code first[l] + (j - offs[l])
    const uint32_t nused = nsym - h->count[0];
    for (uint32_t j = w.lane(); j < nused && j < kMaxLit; j += w.width()) {
        const uint32_t sym = h->sorted[j];
        const uint32_t l = sym < nsym ? (lens[sym] & 15u) : 0;
        if (l == 0 || l > bits) continue;
        const uint32_t code = (uint32_t)h->first[l] + (j - h->offs[l]);
        const uint16_t e = (uint16_t)(sym << 4 | l);
        for (uint32_t k = bitrev(code, l) & (tsize - 1); k < tsize; k += 1u << l) tab[k] = e;
    }
    w.sync();
    return ST_OK;
}

// One symbol: *sym and the code's length in *len (not yet dropped). ST_INVALID: no code of
// this set starts the bits. The caller compares *len with bitcnt.
MGPI_HD inline int32_t decode(const Bits& b, const Huff* h, const uint16_t* tab, uint32_t bits, uint32_t* sym,
                              uint32_t* len) {
    const uint32_t e = tab[peek(b, bits)];
    if (e & 15u) {
        *sym = e >> 4;
        *len = e & 15u;
        return ST_OK;
    }
    uint32_t code = 0, first = 0, index = 0;
    uint64_t v = b.bitbuf;
    for (uint32_t l = 1; l < 16; ++l) {
        code |= (uint32_t)(v & 1);
        v >>= 1;
        const uint32_t c = h->count[l];
        if (code < first + c) {  // (code >= first always)
            const uint32_t k = index + (code - first);
            if (k >= kMaxLit) return ST_INVALID;
            *sym = h->sorted[k];
            *len = l;
            return ST_OK;
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return ST_INVALID;
}

MGPI_HD inline uint32_t len_base(uint32_t s) {  // s = symbol - 257, 0..28
    return s < 8 ? 3 + s : s == 28 ? 258 : 3 + ((4 + (s & 3)) << ((s >> 2) - 1));
}
MGPI_HD inline uint32_t len_extra(uint32_t s) { return s < 8 || s == 28 ? 0 : (s >> 2) - 1; }
MGPI_HD inline uint32_t dist_base(uint32_t s) {  // 0..29
    return s < 4 ? 1 + s : 1 + ((2 + (s & 1)) << ((s >> 1) - 1));
}
MGPI_HD inline uint32_t dist_extra(uint32_t s) { return s < 4 ? 0 : (s >> 1) - 1; }

// The fixed code's lengths into s->lens (288 + 32).
template <class W>
MGPI_HD inline void fixed_lens(const W& w, Scratch* s) {
    w.sync();
    for (uint32_t i = w.lane(); i < kMaxLit + kMaxDist; i += w.width())
        s->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
}

// The dynamic block's header: HLIT, HDIST, HCLEN, the code-length code and the two sets of
// lengths into s->lens ([0, nlen) and [kMaxLit, kMaxLit + ndist)).
template <class W>
MGPI_HD inline int32_t dynamic_header(const W& w, Bits& b, Scratch* s, uint32_t* nlen_out, uint32_t* ndist_out) {
    // the order of the code-length code's lengths, 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15,
    // five bits each (a constant in registers: no table in memory)
    constexpr uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                                  6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    constexpr uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    refill(w, b, s);
    if (b.bitcnt < 14) return ST_SIZE;
    const uint32_t nlen = peek(b, 5) + 257;
    drop(b, 5);
    const uint32_t ndist = peek(b, 5) + 1;
    drop(b, 5);
    const uint32_t ncode = peek(b, 4) + 4;  // <= 19
    drop(b, 4);
    if (nlen > 286 || ndist > 30) return ST_INVALID;
    w.sync();
    for (uint32_t i = 0; i < kMaxCl; ++i) {
        uint32_t v = 0;
        if (i < ncode) {
            refill(w, b, s);
            if (b.bitcnt < 3) return ST_SIZE;
            v = peek(b, 3);
            drop(b, 3);
        }
        const uint32_t at = (uint32_t)((i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31u);
        if (w.leader() && at < kMaxCl) s->cl_lens[at] = (uint8_t)v;
    }
    int32_t rc = build(w, s->cl_lens, kMaxCl, kMaxCl, true, &s->cl, s->cl_tab, kClBits);
    if (rc != ST_OK) return rc;
    // the nlen + ndist lengths (<= 316 symbols, each one step of this loop or the end)
    const uint32_t total = nlen + ndist;
    uint32_t have = 0, prev = 0;
    for (uint32_t step = 0; step < kMaxLit + kMaxDist && have < total; ++step) {
        refill(w, b, s);
        uint32_t sym, len;
        if (decode(b, &s->cl, s->cl_tab, kClBits, &sym, &len) != ST_OK) return ST_INVALID;
        if (len > b.bitcnt) return ST_SIZE;
        drop(b, len);
        uint32_t rep = 1, val = sym;
        if (sym >= 16) {
            const uint32_t eb = sym == 16 ? 2 : sym == 17 ? 3 : 7;
            if (sym > 18) return ST_INVALID;
            if (b.bitcnt < eb) return ST_SIZE;
            if (sym == 16 && have == 0) return ST_INVALID;
            rep = (sym == 16 ? 3 : sym == 17 ? 3 : 11) + peek(b, eb);
            drop(b, eb);
            val = sym == 16 ? prev : 0;
            if (have + rep > total) return ST_INVALID;
        }
        // lengths [have, have + rep): rep <= 138, have + rep <= total <= 316
        if (w.leader())
            for (uint32_t k = 0; k < rep; ++k) {
                const uint32_t i = have + k;
                const uint32_t at = i < nlen ? i : kMaxLit + (i - nlen);
                if (at < kMaxLit + kMaxDist) s->lens[at] = (uint8_t)val;
            }
        have += rep;
        prev = val;
    }
    if (have != total) return ST_INVALID;
    w.sync();
    if (s->lens[256] == 0) return ST_INVALID;  // no end-of-block code
    *nlen_out = nlen;
    *ndist_out = ndist;
    return ST_OK;
}

// Inflates src[0, clen) into win[0, isize). Returns the block's status, the same in every
// lane; win holds the block's bytes when it is ST_OK. clen < 2^31.
template <class W>
MGPI_HD inline int32_t inflate(const W& w, const uint8_t* src, uint32_t clen, uint8_t* win, uint32_t isize, Scratch* s) {
    if (isize > kMaxIsize || clen >= 0x80000000u) return ST_INVALID;
    Bits b;
    b.src = src;
    b.clen = clen;
    uint32_t op = 0;
    uint64_t budget = 8ull * clen + 64;  // steps: block headers and symbols, each takes >= 1 bit
    bool final_seen = false;
    while (!final_seen) {
        if (budget-- == 0) return ST_INVALID;
        refill(w, b, s);
        if (b.bitcnt < 3) return ST_SIZE;
        final_seen = peek(b, 1) != 0;
        const uint32_t type = peek(b, 3) >> 1;
        drop(b, 3);
        if (type == 3) return ST_INVALID;
        if (type == 0) {
            drop(b, b.bitcnt & 7);
            refill(w, b, s);
            if (b.bitcnt < 32) return ST_SIZE;
            const uint32_t len = peek(b, 16);
            drop(b, 16);
            const uint32_t nlen = peek(b, 16);
            drop(b, 16);
            if ((len ^ 0xFFFFu) != nlen) return ST_INVALID;
            const uint32_t pos = b.ip - (b.bitcnt >> 3);  // the byte after NLEN (bitcnt is a multiple of 8)
            if (len > clen - pos) return ST_SIZE;         // (pos <= ip <= clen)
            if (len > isize - op) return ST_SIZE;         // (op <= isize)
            w.sync();
            for (uint32_t i = w.lane(); i < len; i += w.width()) win[op + i] = src[pos + i];
            w.sync();
            op += len;
            b.bitbuf = 0;
            b.bitcnt = 0;
            b.ip = pos + len;
            b.wbase = b.wend = b.ip;  // (the next refill stages the window from here)
            continue;
        }
        uint32_t nlen = kMaxLit, ndist = kMaxDist;
        if (type == 1) {
            fixed_lens(w, s);
        } else {
            const int32_t rc = dynamic_header(w, b, s, &nlen, &ndist);
            if (rc != ST_OK) return rc;
        }
        int32_t rc = build(w, s->lens, nlen, kMaxLit, false, &s->lit, s->lit_tab, kLitBits);
        if (rc != ST_OK) return rc;
        rc = build(w, s->lens + kMaxLit, ndist, kMaxDist, false, &s->dist, s->dist_tab, kDistBits);
        if (rc != ST_OK) return rc;
        // the symbols of this block
        bool end_of_block = false;
        while (!end_of_block) {
            if (budget-- == 0) return ST_INVALID;
            refill(w, b, s);
            uint32_t sym, len;
            if (decode(b, &s->lit, s->lit_tab, kLitBits, &sym, &len) != ST_OK) return ST_INVALID;
            if (len > b.bitcnt) return ST_SIZE;
            drop(b, len);
            if (sym < 256) {
                if (op >= isize) return ST_SIZE;
                if (w.leader()) win[op] = (uint8_t)sym;
                ++op;
                continue;
            }
            if (sym == 256) {
                end_of_block = true;
                continue;
            }
            if (sym >= 286) return ST_INVALID;
            const uint32_t ls = sym - 257;
            const uint32_t le = len_extra(ls);
            if (b.bitcnt < le) return ST_SIZE;
            const uint32_t mlen = len_base(ls) + peek(b, le);
            drop(b, le);
            refill(w, b, s);
            uint32_t dsym, dlen;
            if (decode(b, &s->dist, s->dist_tab, kDistBits, &dsym, &dlen) != ST_OK) return ST_INVALID;
            if (dlen > b.bitcnt) return ST_SIZE;
            drop(b, dlen);
            if (dsym >= 30) return ST_INVALID;
            const uint32_t de = dist_extra(dsym);
            if (b.bitcnt < de) return ST_SIZE;
            const uint32_t dist = dist_base(dsym) + peek(b, de);
            drop(b, de);
            if (dist > op) return ST_INVALID;         // before the start of the output
            if (mlen > isize - op) return ST_SIZE;    // more than isize bytes
            // every source byte lies in [op - dist, op), written before this step; the bytes
            // of an overlapping match (dist < mlen) repeat with period dist
            w.sync();
            const uint32_t from = op - dist;
            if (dist >= mlen) {
                for (uint32_t i = w.lane(); i < mlen; i += w.width()) win[op + i] = win[from + i];
            } else {
                for (uint32_t i = w.lane(); i < mlen; i += w.width()) win[op + i] = win[from + i % dist];
            }
            w.sync();
            op += mlen;
        }
    }
    w.sync();
    return op == isize ? ST_OK : ST_SIZE;
}

// win[0, n) to dst[0, n): bytes up to dst's first 4-byte boundary and after its last, whole
// words between, so no store touches a byte outside [dst, dst + n).
template <class W>
MGPI_HD inline void flush(const W& w, const uint8_t* win, uint32_t n, uint8_t* dst) {
    const uint32_t mis = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
    const uint32_t head = mis < n ? mis : n;
    const uint32_t words = (n - head) >> 2;
    const uint32_t tail0 = head + 4 * words;
    for (uint32_t i = w.lane(); i < head; i += w.width()) dst[i] = win[i];
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + head);  // 4-byte aligned when words > 0
    for (uint32_t k = w.lane(); k < words; k += w.width()) {
        const uint8_t* p = win + head + 4 * k;
        d32[k] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    }
    for (uint32_t i = tail0 + w.lane(); i < n; i += w.width()) dst[i] = win[i];
}

// The piece ring[(from & mask) ...) of n <= kHalf bytes, which does not wrap (from is a
// multiple of kHalf), to dst[from, from + n), and its bytes into the Adler-32 state
// (*a, *b), the same in every lane: lane l sums the bytes i = l, l + width, ... as
// s1 = sum d_i and s2 = sum (n - i) d_i, the sums are reduced mod 65521 and combined
// through s->red, and then a' = a + S1, b' = b + n * a + S2 (mod 65521).
template <class W>
MGPI_HD inline void flush_ring(const W& w, const uint8_t* ring, uint32_t from, uint32_t n, uint8_t* dst, Scratch* s,
                               uint32_t* a, uint32_t* b) {
    if (n == 0) return;
    w.sync();  // (the piece's bytes are written)
    const uint8_t* p = ring + (from & (kRing - 1));  // (from & (kRing - 1)) + n <= kRing
    flush(w, p, n, dst + from);
    uint64_t s1 = 0, s2 = 0;
    for (uint32_t i = w.lane(); i < n; i += w.width()) {
        const uint64_t d = p[i];
        s1 += d;
        s2 += (uint64_t)(n - i) * d;
    }
    const uint32_t l = w.lane() < kMaxLanes ? w.lane() : kMaxLanes - 1;
    s->red[2 * l] = (uint32_t)(s1 % kAdlerMod);
    s->red[2 * l + 1] = (uint32_t)(s2 % kAdlerMod);
    w.sync();
    uint64_t t1 = 0, t2 = 0;
    const uint32_t nl = w.width() < kMaxLanes ? w.width() : kMaxLanes;
    for (uint32_t k = 0; k < nl; ++k) {
        t1 += s->red[2 * k];
        t2 += s->red[2 * k + 1];
    }
    const uint64_t a0 = *a;
    *a = (uint32_t)((a0 + t1) % kAdlerMod);
    *b = (uint32_t)((*b + (uint64_t)n * a0 + t2) % kAdlerMod);
    w.sync();  // (red and the piece's ring bytes may be written again)
}

// Inflates the zlib stream src[0, clen) into dst[0, isize) through ring (kRing bytes).
// Returns the stream's status, the same in every lane: ST_OK, dst then holds the bytes;
// ST_INVALID (a bad header or deflate stream), ST_SIZE (more or fewer than isize bytes, or
// the input ends early), ST_CHECK (a well-formed stream whose Adler-32 differs, or bytes
// after the trailer). A refused stream may have written a part of dst.
template <class W>
MGPI_HD inline int32_t inflate_zlib(const W& w, const uint8_t* src, uint32_t clen, uint8_t* ring, uint8_t* dst,
                                    uint32_t isize, Scratch* s) {
    if (isize >= 0x80000000u || clen >= 0x80000000u) return ST_INVALID;
    if (clen < 2) return ST_SIZE;
    const uint32_t cmf = src[0], flg = src[1];
    if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || (flg & 0x20u) || ((cmf << 8) | flg) % 31 != 0) return ST_INVALID;
    if (clen < 6) return ST_SIZE;
    Bits b;
    b.src = src + 2;
    b.clen = clen - 2;
    uint32_t op = 0, flushed = 0;  // bytes written to the ring; bytes of them in dst (a multiple of kHalf)
    uint32_t ad_a = 1, ad_b = 0;
    uint64_t budget = 8ull * clen + 64;  // steps: block headers and symbols, each takes >= 1 bit
    bool final_seen = false;
    while (!final_seen) {
        if (budget-- == 0) return ST_INVALID;
        refill(w, b, s);
        if (b.bitcnt < 3) return ST_SIZE;
        final_seen = peek(b, 1) != 0;
        const uint32_t type = peek(b, 3) >> 1;
        drop(b, 3);
        if (type == 3) return ST_INVALID;
        if (type == 0) {
            drop(b, b.bitcnt & 7);
            refill(w, b, s);
            if (b.bitcnt < 32) return ST_SIZE;
            const uint32_t len = peek(b, 16);
            drop(b, 16);
            const uint32_t nlen = peek(b, 16);
            drop(b, 16);
            if ((len ^ 0xFFFFu) != nlen) return ST_INVALID;
            uint32_t pos = b.ip - (b.bitcnt >> 3);    // the byte after NLEN (bitcnt is a multiple of 8)
            if (len > b.clen - pos) return ST_SIZE;   // (pos <= ip <= clen)
            if (len > isize - op) return ST_SIZE;     // (op <= isize)
            for (uint32_t left = len; left;) {        // pieces that end at the half's end at the latest
                const uint32_t room = kHalf - (op - flushed), n = left < room ? left : room;
                w.sync();
                for (uint32_t i = w.lane(); i < n; i += w.width()) ring[(op + i) & (kRing - 1)] = b.src[pos + i];
                op += n;
                pos += n;
                left -= n;
                if (op - flushed == kHalf) {
                    flush_ring(w, ring, flushed, kHalf, dst, s, &ad_a, &ad_b);
                    flushed += kHalf;
                }
            }
            w.sync();
            b.bitbuf = 0;
            b.bitcnt = 0;
            b.ip = pos;
            b.wbase = b.wend = b.ip;  // (the next refill stages the window from here)
            continue;
        }
        uint32_t nlen = kMaxLit, ndist = kMaxDist;
        if (type == 1) {
            fixed_lens(w, s);
        } else {
            const int32_t rc = dynamic_header(w, b, s, &nlen, &ndist);
            if (rc != ST_OK) return rc;
        }
        int32_t rc = build(w, s->lens, nlen, kMaxLit, false, &s->lit, s->lit_tab, kLitBits);
        if (rc != ST_OK) return rc;
        rc = build(w, s->lens + kMaxLit, ndist, kMaxDist, false, &s->dist, s->dist_tab, kDistBits);
        if (rc != ST_OK) return rc;
        bool end_of_block = false;
        while (!end_of_block) {
            if (budget-- == 0) return ST_INVALID;
            refill(w, b, s);
            uint32_t sym, len;
            if (decode(b, &s->lit, s->lit_tab, kLitBits, &sym, &len) != ST_OK) return ST_INVALID;
            if (len > b.bitcnt) return ST_SIZE;
            drop(b, len);
            if (sym < 256) {
                if (op >= isize) return ST_SIZE;
                if (w.leader()) ring[op & (kRing - 1)] = (uint8_t)sym;
                ++op;
            } else if (sym == 256) {
                end_of_block = true;
                continue;
            } else {
                if (sym >= 286) return ST_INVALID;
                const uint32_t ls = sym - 257;
                const uint32_t le = len_extra(ls);
                if (b.bitcnt < le) return ST_SIZE;
                const uint32_t mlen = len_base(ls) + peek(b, le);
                drop(b, le);
                refill(w, b, s);
                uint32_t dsym, dlen;
                if (decode(b, &s->dist, s->dist_tab, kDistBits, &dsym, &dlen) != ST_OK) return ST_INVALID;
                if (dlen > b.bitcnt) return ST_SIZE;
                drop(b, dlen);
                if (dsym >= 30) return ST_INVALID;
                const uint32_t de = dist_extra(dsym);
                if (b.bitcnt < de) return ST_SIZE;
                const uint32_t dist = dist_base(dsym) + peek(b, de);  // <= 32768 = kHalf
                drop(b, de);
                if (dist > op) return ST_INVALID;       // before the start of the output
                if (mlen > isize - op) return ST_SIZE;  // more than isize bytes
                // every source byte lies in [op - dist, op), still in the ring (dist <= kHalf);
                // the bytes of an overlapping match (dist < mlen) repeat with period dist
                w.sync();
                const uint32_t from = op - dist;
                if (dist >= mlen) {
                    for (uint32_t i = w.lane(); i < mlen; i += w.width())
                        ring[(op + i) & (kRing - 1)] = ring[(from + i) & (kRing - 1)];
                } else {
                    for (uint32_t i = w.lane(); i < mlen; i += w.width())
                        ring[(op + i) & (kRing - 1)] = ring[(from + i % dist) & (kRing - 1)];
                }
                w.sync();
                op += mlen;
            }
            if (op - flushed >= kHalf) {  // (< kHalf + 258)
                flush_ring(w, ring, flushed, kHalf, dst, s, &ad_a, &ad_b);
                flushed += kHalf;
            }
        }
    }
    if (op != isize) return ST_SIZE;
    flush_ring(w, ring, flushed, op - flushed, dst, s, &ad_a, &ad_b);  // the tail, < kHalf bytes
    // the trailer: Adler-32, big-endian, at the byte after the last block's last bit
    const uint32_t pos = b.ip - (b.bitcnt >> 3);  // <= b.clen
    if (b.clen - pos < 4) return ST_SIZE;
    const uint8_t* t = b.src + pos;
    const uint32_t want = (uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | (uint32_t)t[3];
    if (want != (ad_b << 16 | ad_a)) return ST_CHECK;
    return b.clen - pos == 4 ? ST_OK : ST_CHECK;
}

}  // namespace mgp_inflate
