"""An instrumented inflate for the tests: RFC 1951 decoded in plain Python, with what each
block was made of.

probe_gzip(member) / probe_zlib(stream) / probe_deflate(raw) return a Probe: the decoded
bytes and, per block (Block), BTYPE and BFINAL, the dynamic header (HLIT, HDIST, HCLEN, the
three code-length arrays, the code-length symbols as sent), the tokens, the block's exact
bit size and, for a stored block, its LEN. They raise ProbeError on an over-subscribed code,
a symbol used without a code, LEN != ~NLEN, a distance that reaches before the start, and
on anything but the exact trailer after the final block (gzip: CRC-32 and ISIZE, zlib:
Adler-32; both headers are checked too). An incomplete code is recorded (kraft_*), not
refused: zlib itself sends a distance code of one symbol.

The helpers below the decoder compute what the device tests assert from those stats: Kraft
sums, the unrestricted Huffman depth and cost of a histogram (heapq), the optimal
length-limited cost (package-merge), the fixed code's and a stored block's sizes.
"""

from __future__ import annotations

import heapq
import zlib
from dataclasses import dataclass, field
from fractions import Fraction

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258)
LEN_XB = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577)
DIST_XB = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class ProbeError(ValueError):
    pass


@dataclass
class Block:
    btype: int
    bfinal: int
    bits: int = 0            # the block's exact size, header and EOB included
    start_bit: int = 0       # where it starts in the deflate stream
    n_bytes: int = 0         # bytes it decodes to
    stored_len: int | None = None
    # dynamic blocks
    hlit: int = 0
    hdist: int = 0
    hclen: int = 0
    cl_lengths: list = field(default_factory=list)    # [19] by symbol
    lit_lengths: list = field(default_factory=list)   # [hlit]
    dist_lengths: list = field(default_factory=list)  # [hdist]
    cl_syms: list = field(default_factory=list)       # the code-length symbols as sent
    header_bits: int = 0     # the 3 block bits, HLIT/HDIST/HCLEN, the code-length code and the lengths
    # tokens: a literal byte, or (length, distance)
    tokens: list = field(default_factory=list)
    lit_hist: list = field(default_factory=lambda: [0] * 288)   # literal/length symbols, EOB (1) included
    dist_hist: list = field(default_factory=lambda: [0] * 32)
    max_len: int = 0
    max_dist: int = 0

    @property
    def cl_hist(self) -> list:
        h = [0] * 19
        for s in self.cl_syms:
            h[s] += 1
        return h

    @property
    def kraft_lit(self) -> Fraction:
        return kraft(self.lit_lengths)

    @property
    def kraft_dist(self) -> Fraction:
        return kraft(self.dist_lengths)

    @property
    def kraft_cl(self) -> Fraction:
        return kraft(self.cl_lengths)


@dataclass
class Probe:
    data: bytes
    blocks: list
    deflate_bytes: int  # bytes of the deflate stream (the last one padded)

    @property
    def btypes(self) -> list:
        return [b.btype for b in self.blocks]


def kraft(lengths) -> Fraction:
    return sum((Fraction(1, 1 << l) for l in lengths if l), Fraction(0))


class _Bits:
    def __init__(self, buf: bytes):
        self.buf = buf
        self.pos = 0  # in bits

    def get(self, n: int) -> int:
        if n == 1 and self.pos < 8 * len(self.buf):
            p = self.pos
            self.pos = p + 1
            return (self.buf[p >> 3] >> (p & 7)) & 1
        if self.pos + n > 8 * len(self.buf):
            raise ProbeError("the stream ends inside a block")
        v = 0
        p = self.pos
        for k in range(n):
            v |= ((self.buf[(p + k) >> 3] >> ((p + k) & 7)) & 1) << k
        self.pos = p + n
        return v


def _decoder(lengths, what: str):
    """{(length, code): symbol} of a canonical code; raises if over-subscribed."""
    if kraft(lengths) > 1:
        raise ProbeError(f"over-subscribed {what} code")
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt = [0] * 17
    code = 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def _sym(br: _Bits, table, what: str) -> int:
    code = 0
    for l in range(1, 16):
        code = (code << 1) | br.get(1)
        s = table.get((l, code))
        if s is not None:
            return s
    raise ProbeError(f"a {what} symbol without a code")


def probe_deflate(raw: bytes) -> Probe:
    """A raw deflate stream at raw[0]; Probe.deflate_bytes tells where it ends."""
    br = _Bits(raw)
    out = bytearray()
    blocks = []
    while True:
        blk = Block(btype=0, bfinal=0, start_bit=br.pos)
        blk.bfinal = br.get(1)
        blk.btype = br.get(2)
        n0 = len(out)
        if blk.btype == 0:
            br.pos = (br.pos + 7) & ~7
            ln, nl = br.get(16), br.get(16)
            if ln != (~nl & 0xFFFF):
                raise ProbeError("stored block: LEN is not ~NLEN")
            a = br.pos >> 3
            if a + ln > len(raw):
                raise ProbeError("the stream ends inside a stored block")
            out += raw[a:a + ln]
            br.pos += 8 * ln
            blk.stored_len = ln
        elif blk.btype in (1, 2):
            if blk.btype == 1:
                lit_l, dist_l = FIXED_LIT, FIXED_DIST
                blk.header_bits = 3
            else:
                blk.hlit, blk.hdist, blk.hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
                if blk.hlit > 286 or blk.hdist > 30:
                    raise ProbeError("HLIT or HDIST past the format's symbols")
                cl = [0] * 19
                for i in range(blk.hclen):
                    cl[CL_ORDER[i]] = br.get(3)
                blk.cl_lengths = cl
                cl_t = _decoder(cl, "code-length")
                lens = []
                while len(lens) < blk.hlit + blk.hdist:
                    s = _sym(br, cl_t, "code-length")
                    blk.cl_syms.append(s)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise ProbeError("repeat with no previous length")
                        lens += [lens[-1]] * (3 + br.get(2))
                    elif s == 17:
                        lens += [0] * (3 + br.get(3))
                    else:
                        lens += [0] * (11 + br.get(7))
                if len(lens) != blk.hlit + blk.hdist:
                    raise ProbeError("a repeat runs past the code lengths")
                lit_l, dist_l = lens[:blk.hlit], lens[blk.hlit:]
                blk.lit_lengths, blk.dist_lengths = lit_l, dist_l
                blk.header_bits = br.pos - blk.start_bit
                if not lit_l[256]:
                    raise ProbeError("no code for the end of block")
            lit_t = _decoder(lit_l, "literal/length")
            dist_t = _decoder(dist_l, "distance")
            while True:
                s = _sym(br, lit_t, "literal/length")
                blk.lit_hist[s] += 1
                if s < 256:
                    out.append(s)
                    blk.tokens.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise ProbeError("length symbol 286 or 287")
                ln = LEN_BASE[s - 257] + br.get(LEN_XB[s - 257])
                d = _sym(br, dist_t, "distance")
                if d > 29:
                    raise ProbeError("distance symbol 30 or 31")
                blk.dist_hist[d] += 1
                dist = DIST_BASE[d] + br.get(DIST_XB[d])
                if dist > len(out):
                    raise ProbeError("a distance reaches before the start")
                if dist > 32768:
                    raise ProbeError("a distance past the window")
                for _ in range(ln):
                    out.append(out[-dist])
                blk.tokens.append((ln, dist))
                blk.max_len = max(blk.max_len, ln)
                blk.max_dist = max(blk.max_dist, dist)
        else:
            raise ProbeError("BTYPE 3")
        blk.bits = br.pos - blk.start_bit
        blk.n_bytes = len(out) - n0
        blocks.append(blk)
        if blk.bfinal:
            break
    return Probe(bytes(out), blocks, (br.pos + 7) >> 3)


def probe_gzip(member: bytes) -> Probe:
    """One gzip member (RFC 1952) and nothing after it."""
    member = bytes(member)
    if len(member) < 18 or member[:3] != b"\x1f\x8b\x08":
        raise ProbeError("not a gzip member")
    flg = member[3]
    at = 10
    if flg & 4:
        at += 2 + int.from_bytes(member[at:at + 2], "little")
    for bit in (8, 16):
        if flg & bit:
            at = member.index(b"\0", at) + 1
    if flg & 2:
        at += 2
    p = probe_deflate(member[at:])
    tail = member[at + p.deflate_bytes:]
    want = (zlib.crc32(p.data) & 0xFFFFFFFF).to_bytes(4, "little") + (len(p.data) & 0xFFFFFFFF).to_bytes(4, "little")
    if tail != want:
        raise ProbeError("the bytes after the final block are not CRC-32 and ISIZE of the data")
    return p


def probe_zlib(stream: bytes) -> Probe:
    """One zlib stream (RFC 1950) and nothing after it."""
    stream = bytes(stream)
    if len(stream) < 6 or (stream[0] & 15) != 8 or (stream[0] >> 4) > 7 or int.from_bytes(stream[:2], "big") % 31:
        raise ProbeError("not a zlib header")
    if stream[1] & 0x20:
        raise ProbeError("a preset dictionary")
    p = probe_deflate(stream[2:])
    if stream[2 + p.deflate_bytes:] != (zlib.adler32(p.data) & 0xFFFFFFFF).to_bytes(4, "big"):
        raise ProbeError("the bytes after the final block are not the Adler-32 of the data")
    return p


# ---- what the tests compute from a block ----
def len_symbol(ln: int) -> int:
    for c in range(28, -1, -1):
        if ln >= LEN_BASE[c]:
            return 257 + c
    raise ValueError(ln)


def dist_symbol(d: int) -> int:
    for c in range(29, -1, -1):
        if d >= DIST_BASE[c]:
            return c
    raise ValueError(d)


def extra_bits(blk: Block) -> int:
    """The extra bits of the block's length and distance symbols."""
    return (sum(n * LEN_XB[s - 257] for s, n in enumerate(blk.lit_hist) if s > 256 and n)
            + sum(n * DIST_XB[s] for s, n in enumerate(blk.dist_hist[:30]) if n))


def fixed_bits(blk: Block) -> int:
    """The block's tokens and EOB under the fixed codes (RFC 1951 3.2.6), without the 3 header bits."""
    return (sum(n * FIXED_LIT[s] for s, n in enumerate(blk.lit_hist)) + 5 * sum(blk.dist_hist) + extra_bits(blk))


def stored_bytes(n: int) -> int:
    return n + 5 * (n // 65535 + 1)


def huffman_depth_cost(hist) -> tuple[int, int]:
    """(depth, cost in bits) of an unrestricted Huffman code of the nonzero counts: the cost is
    the optimum, unique whatever the ties; the depth is the least among optimal trees (ties
    take the shallower subtree first). One symbol: (1, its count)."""
    f = [c for c in hist if c]
    if not f:
        return 0, 0
    if len(f) == 1:
        return 1, f[0]
    h = [(c, 0) for c in f]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a, da = heapq.heappop(h)
        b, db = heapq.heappop(h)
        cost += a + b
        heapq.heappush(h, (a + b, max(da, db) + 1))
    return h[0][1], cost


def package_merge_cost(hist, limit: int) -> int:
    """The cost of an optimal prefix code of the nonzero counts with no length above `limit`."""
    f = sorted(c for c in hist if c)
    n = len(f)
    if n == 0:
        return 0
    if n == 1:
        return f[0]
    if n > 1 << limit:
        raise ValueError("no such code")
    leaves = [(c, (i,)) for i, c in enumerate(f)]
    cur = list(leaves)
    for _ in range(limit - 1):
        pk = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + pk, key=lambda x: x[0])
    length = [0] * n
    for _, items in cur[:2 * n - 2]:
        for i in items:
            length[i] += 1
    assert kraft(length) == 1
    return sum(c * l for c, l in zip(f, length))


# ---- the invariants the device tests hold every block to ----
def _code_report(name: str, hist, lengths, limit: int, out: dict) -> None:
    """One code of a dynamic block against its own symbols' counts `hist`: every used symbol
    has a code, no length above `limit`, a symbol that occurs more often never has a longer
    code, and the coded bits equal the optimum (unrestricted Huffman, unique whatever the
    ties) when that tree fits the limit; when it does not, they are at least the optimum and
    the longest code is `limit` long (the ratio to package-merge's optimum is recorded)."""
    lengths = list(lengths) + [0] * (len(hist) - len(lengths))
    used = [(n, lengths[s]) for s, n in enumerate(hist) if n]
    assert all(l for _, l in used), f"{name}: a used symbol without a code"
    assert max(lengths) <= limit, f"{name}: a code of {max(lengths)} bits, limit {limit}"
    # by rising count: the shortest code among the rarer symbols so far is no shorter than
    # the longest code of any more frequent symbol
    by_count: dict = {}
    for s, l in enumerate(lengths):
        if l:
            by_count.setdefault(hist[s] if s < len(hist) else 0, []).append(l)
    shortest_rarer, rarer = None, None
    for n in sorted(by_count):
        if shortest_rarer is not None:
            assert max(by_count[n]) <= shortest_rarer, \
                f"{name}: count {n} has {max(by_count[n])} bits, count {rarer} only {shortest_rarer}"
        if shortest_rarer is None or min(by_count[n]) <= shortest_rarer:
            shortest_rarer, rarer = min(by_count[n]), n
    bits = sum(n * l for n, l in used)
    out[f"{name}_max_len"] = max(lengths)
    out[f"{name}_bits"] = bits
    if len(used) < 2:
        return
    depth, cost = huffman_depth_cost(hist)
    out[f"{name}_depth"] = depth
    if depth <= limit:
        assert bits == cost, f"{name}: {bits} coded bits, the optimum is {cost} (depth {depth} fits {limit})"
    else:
        assert bits >= cost and max(lengths) == limit, (name, bits, cost, max(lengths))
        best = package_merge_cost(hist, limit)
        assert bits >= best
        out[f"{name}_clipped_ratio"] = bits / best
        print(f"{name} code clipped: depth {depth} > {limit}, {bits} bits, package-merge {best}, "
              f"ratio {bits / best:.5f}, unrestricted {cost}")


def check_dynamic_block(blk: Block) -> dict:
    """The invariants of a dynamic block the device wrote (see _code_report); returns what
    was measured. The device always sends at least two distance and two code-length codes,
    so all three codes must be complete."""
    assert blk.btype == 2
    out: dict = {}
    assert blk.kraft_lit == 1 and blk.kraft_dist == 1 and blk.kraft_cl == 1, \
        (blk.kraft_lit, blk.kraft_dist, blk.kraft_cl)
    _code_report("lit", blk.lit_hist[:286], blk.lit_lengths, 15, out)
    _code_report("dist", blk.dist_hist[:30], blk.dist_lengths, 15, out)
    _code_report("cl", blk.cl_hist, blk.cl_lengths, 7, out)
    assert blk.hlit == 257 or blk.lit_lengths[blk.hlit - 1], "HLIT past the last used length symbol"
    assert blk.hdist == 1 or blk.dist_lengths[blk.hdist - 1], "HDIST past the last distance code"
    assert blk.hclen == 4 or blk.cl_lengths[CL_ORDER[blk.hclen - 1]], "HCLEN past the last code-length code"
    coded = out["lit_bits"] + out["dist_bits"] + extra_bits(blk)
    assert blk.bits == blk.header_bits + coded
    return out


def documented_huffman_lengths(freq, limit: int) -> list:
    """Code lengths by the procedure the encoder documents (and zlib's gen_bitlen follows):
    symbols ranked by (count, symbol), one Huffman tree from two queues (a leaf before an
    internal node of equal weight), leaves deeper than `limit` clipped to it, the Kraft sum
    repaired (the deepest shorter leaf one level down until it fits, then the deepest leaf whose
    move up fits, until it is 1), the lengths dealt out longest to rarest."""
    used = sorted((f, s) for s, f in enumerate(freq) if f)
    m = len(used)
    length = [0] * len(freq)
    if m == 0:
        return length
    if m == 1:
        length[used[0][1]] = 1
        return length
    w = [f for f, _ in used]
    par = {}
    li, ni = 0, m
    for _ in range(m - 1):
        pair = []
        for _ in range(2):
            if li < m and (ni >= len(w) or w[li] <= w[ni]):
                pair.append(li)
                li += 1
            else:
                pair.append(ni)
                ni += 1
        w.append(w[pair[0]] + w[pair[1]])
        par[pair[0]] = par[pair[1]] = len(w) - 1
    dep = {len(w) - 1: 0}
    cnt = [0] * (limit + 1)
    for x in range(len(w) - 2, -1, -1):
        dep[x] = dep[par[x]] + 1
        if x < m:
            cnt[min(dep[x], limit)] += 1
    full = 1 << limit
    k = sum(cnt[l] << (limit - l) for l in range(1, limit + 1))
    while k > full:
        b = limit - 1
        while cnt[b] == 0:
            b -= 1
        cnt[b] -= 1
        cnt[b + 1] += 1
        k -= 1 << (limit - b - 1)
    while k < full:
        b = limit
        while cnt[b] == 0 or (1 << (limit - b)) > full - k:
            b -= 1
        cnt[b] -= 1
        cnt[b - 1] += 1
        k += 1 << (limit - b)
    i = 0
    for l in range(limit, 0, -1):
        for _ in range(cnt[l]):
            length[used[i][1]] = l
            i += 1
    return length


def code_length_symbols(lengths) -> list:
    """The run-length form of a dynamic header's lengths, (symbol, extra) pairs: 18 for 11-138
    zeros, 17 for 3-10, a length then 16 for 3-6 repeats of it (runs of 4 and more)."""
    out = []
    i, n = 0, len(lengths)
    while i < n:
        v = lengths[i]
        r = 1
        while i + r < n and lengths[i + r] == v:
            r += 1
        if v == 0 and r >= 3:
            q = min(r, 138)
            out.append((18, q - 11) if q >= 11 else (17, q - 3))
            i += q
        elif v != 0 and r >= 4:
            q = min(r - 1, 6)
            out += [(v, 0), (16, q - 3)]
            i += 1 + q
        else:
            out.append((v, 0))
            i += 1
    return out


def documented_dynamic_bits(lit_hist, dist_hist, extra: int) -> dict:
    """The size of the dynamic block the documented procedure gives for these symbol counts
    (EOB included in lit_hist): what a block written fixed or stored was weighed against.
    Returns the lengths, the code-length histogram and header_bits / bits.

    This is a model of the encoder's own procedure (its tie-breaks and repair loops restated),
    not an independent reference: it is used only to know what the encoder weighed a fixed or
    stored block against. A change of tie-break in the encoder changes it too; what holds the
    encoder's codes to the format are check_dynamic_block's invariants, which use none of it."""
    lit = documented_huffman_lengths(list(lit_hist[:286]) + [0] * (286 - len(lit_hist[:286])), 15)
    dist = documented_huffman_lengths(list(dist_hist[:30]), 15)
    if sum(1 for l in dist if l) < 2:  # at least two distance codes: the used one (or 0) and 0 or 1
        a = max((s for s, l in enumerate(dist) if l), default=0)
        dist = [0] * 30
        dist[a] = 1
        dist[1 if a == 0 else 0] = 1
    hlit = max([257] + [s + 1 for s in range(257, 286) if lit[s]])
    hdist = max(s + 1 for s in range(30) if dist[s])
    syms = code_length_symbols(lit[:hlit] + dist[:hdist])
    cl_hist = [0] * 19
    for s, _ in syms:
        cl_hist[s] += 1
    cl = documented_huffman_lengths(cl_hist, 7)
    if sum(1 for l in cl if l) == 1:
        cl[1 if cl[0] else 0] = 1
    hclen = max([4] + [i + 1 for i in range(19) if cl[CL_ORDER[i]]])
    header = 17 + 3 * hclen + sum(cl[s] + {16: 2, 17: 3, 18: 7}.get(s, 0) for s, _ in syms)
    bits = (header + sum(n * lit[s] for s, n in enumerate(lit_hist[:286]))
            + sum(n * dist[s] for s, n in enumerate(dist_hist[:30])) + extra)
    return dict(lit=lit, dist=dist, cl=cl, cl_hist=cl_hist, hlit=hlit, hdist=hdist, hclen=hclen, header_bits=header,
                bits=bits)


def check_block_choice(blocks: list, literals: bytes | None = None) -> str:
    """The kind written is the smallest of the three the format offers for the encoder's own
    tokens (ties: dynamic, then fixed, then stored): dynamic = its header and coded bits,
    fixed = (3 + the tokens and EOB under the fixed codes + 7) // 8, stored = n + 5 (n // 65535
    + 1), in bytes. `blocks`: the stream's blocks, one coded block or a stored stream. A
    dynamic block's size is its own; for a fixed block it is documented_dynamic_bits of its
    tokens; stored blocks show no tokens, so the caller passes `literals` (the data) when its
    input can only parse to literals. Returns a line for the log."""
    kind = blocks[0].btype
    n = sum(b.n_bytes for b in blocks)
    if kind == 0:
        assert all(b.btype == 0 for b in blocks)
        assert literals is not None and len(literals) == n, "a stored stream whose tokens the test cannot know"
        lit_hist = [0] * 288
        for c in literals:
            lit_hist[c] += 1
        lit_hist[256] = 1
        dist_hist, extra = [0] * 32, 0
        fixed = (3 + sum(c * FIXED_LIT[s] for s, c in enumerate(lit_hist)) + 7) // 8
        written = sum(5 + b.stored_len for b in blocks)
    else:
        assert len(blocks) == 1
        b = blocks[0]
        lit_hist, dist_hist, extra = b.lit_hist, b.dist_hist, extra_bits(b)
        fixed = (3 + fixed_bits(b) + 7) // 8
        written = (b.bits + 7) // 8
    stored = stored_bytes(n)
    if kind == 2:
        dynamic = written
    else:
        dynamic = (documented_dynamic_bits(lit_hist, dist_hist, extra)["bits"] + 7) // 8
    want = 2 if dynamic <= fixed and dynamic <= stored else 1 if fixed <= stored else 0
    assert written == {2: dynamic, 1: fixed, 0: stored}[kind], (kind, written, dynamic, fixed, stored)
    assert kind == want, f"BTYPE {kind} written; dynamic {dynamic}, fixed {fixed}, stored {stored} bytes"
    return f"BTYPE {kind}: dynamic {dynamic} fixed {fixed} stored {stored} bytes of {n}"
