"""The raw-deflate streams the inflate tests share (test_inflate_core.py on the CPU,
test_gpu_inflate.py on the device): Python's zlib (wbits=-15) makes the valid ones and
their expected bytes, a small LSB-first bit writer the hand-made ones, and the native
BAM writer libdeflate's. Every case is (name, stream, isize, status, expected bytes or
None); status as mgp_bgzf_inflate reports it: 0 ok, 1 invalid stream, 2 wrong size or
input ended early."""

from __future__ import annotations

import functools
import random
import struct
import zlib
from pathlib import Path

import numpy as np

OK, INVALID, SIZE = 0, 1, 2
ANY_ERROR = 255  # (the mutations: any non-zero status)


class BitWriter:
    """Deflate's bit order: data elements LSB first, Huffman codes MSB first."""

    def __init__(self):
        self.acc = 0
        self.n = 0

    def bits(self, value: int, count: int):
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        return self

    def code(self, code: int, length: int):
        for i in range(length - 1, -1, -1):
            self.bits((code >> i) & 1, 1)
        return self

    def align(self):
        self.n = (self.n + 7) & ~7
        return self

    def bytes_(self, data: bytes):
        assert self.n % 8 == 0
        for x in data:
            self.bits(x, 8)
        return self

    def done(self) -> bytes:
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def fixed_lit(w: BitWriter, sym: int):
    """One literal/length symbol of the fixed code (RFC 1951 3.2.6)."""
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xC0 + sym - 280, 8)


def raw(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(data) + co.flush()


def zlib_verdict(stream: bytes, limit: int = 1 << 17):
    """(bytes, reached the end of the stream) as zlib decodes it; (None, False) on zlib.error."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream, limit)
    except zlib.error:
        return None, False
    return out, bool(d.eof)


def _periodic(period: int, n: int = 20000) -> bytes:
    rng = random.Random(period)
    unit = bytes(rng.randrange(256) for _ in range(period))
    return (unit * (n // period + 1))[:n]


def _far_match() -> tuple[bytes, bytes]:
    """Fixed block: 32,768 literals, then length 258 (symbol 285) at distance 32,768 (code
    29, its 13 extra bits all ones)."""
    rng = random.Random(29)
    lit = bytes(rng.randrange(256) for _ in range(32768))
    w = BitWriter().bits(1, 1).bits(1, 2)
    for x in lit:
        fixed_lit(w, x)
    fixed_lit(w, 285)
    w.code(29, 5).bits(0x1FFF, 13)
    fixed_lit(w, 256)
    return w.done(), lit + lit[:258]


def bgzf_blocks(path) -> list[tuple[bytes, int, int]]:
    """(raw deflate stream, isize, crc) of every BGZF block of a file."""
    data = Path(path).read_bytes()
    out, p = [], 0
    while p < len(data):
        xlen = struct.unpack_from("<H", data, p + 10)[0]
        bsize = struct.unpack_from("<H", data, p + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", data, p + bsize - 8)
        out.append((data[p + 12 + xlen:p + bsize - 8], isize, crc))
        p += bsize
    return out


def write_test_bam(path, level: int, n_reads: int = 3000, n_cells: int = 16, seed: int = 5):
    """The 3,000-read BAM of the tests, from the native writer (libdeflate's streams)."""
    from mgatk2_amd.bam import write_bam
    from mgatk2_amd.synth import barcode_names, synth_reads

    names = barcode_names(n_cells, seed)
    write_bam(path, synth_reads(seed, n_reads, n_cells), names, level=level, n_threads=2)
    return names


@functools.lru_cache(maxsize=None)
def valid_cases() -> tuple:
    rng = random.Random(1951)
    acgt = bytes(rng.choice(b"ACGT") for _ in range(65280))
    skew = bytes(rng.choice(b"aaaaaaaabbbbccd") for _ in range(3000))
    noise = bytes(rng.randrange(256) for _ in range(30000))
    cases = [("eof", bytes.fromhex("0300")), ("one", raw(b"x"))]
    cases.append(("stored", raw(bytes(rng.randrange(256) for _ in range(65280)), 0)))
    cases.append(("fixed50", raw(bytes(rng.randrange(97, 101) for _ in range(50)), 6, zlib.Z_FIXED)))
    cases.append(("fixed256", raw(bytes(range(256)), 6, zlib.Z_FIXED)))
    cases.append(("huffman_only", raw(skew, 6, zlib.Z_HUFFMAN_ONLY)))
    cases.append(("rle", raw(b"a" * 65536, 6, zlib.Z_RLE)))
    for lv in (1, 6, 9):
        cases.append((f"acgt{lv}", raw(acgt, lv)))
    cases.append(("noise", raw(noise)))
    for p in (1, 2, 3, 63, 64, 65, 257):
        cases.append((f"period{p}", raw(_periodic(p))))
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    cases.append(("full_flush", co.compress(acgt[:5000]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(skew) +
                  co.flush(zlib.Z_FULL_FLUSH) + co.flush()))
    out = []
    for name, s in cases:
        exp, eof = zlib_verdict(s)
        assert exp is not None and eof and len(exp) <= 65536, name
        out.append((name, s, len(exp), OK, exp))
    s, exp = _far_match()
    got, eof = zlib_verdict(s)
    assert got == exp and eof
    out.append(("far_match", s, len(exp), OK, exp))
    return tuple(out)


def bam_cases(tmp_dir) -> list:
    """The blocks of the 3,000-read BAM at levels 1, 6 and 9."""
    out = []
    for lv in (1, 6, 9):
        path = Path(tmp_dir) / f"corpus{lv}.bam"
        write_test_bam(path, lv)
        for i, (s, isize, crc) in enumerate(bgzf_blocks(path)):
            exp, eof = zlib_verdict(s)
            assert exp is not None and eof and len(exp) == isize and zlib.crc32(exp) == crc
            out.append((f"bam{lv}_{i}", s, isize, OK, exp))
    return out


@functools.lru_cache(maxsize=None)
def invalid_cases() -> tuple:
    out = []
    out.append(("type3", BitWriter().bits(1, 1).bits(3, 2).bits(0, 5).done() + b"\0" * 4, 10, INVALID))
    out.append(("len_nlen", b"\x01\x05\x00\xfb\xff" + b"hello", 5, INVALID))
    out.append(("len_past_input", b"\x01\x05\x00\xfa\xff" + b"hel", 5, SIZE))
    w = BitWriter().bits(1, 1).bits(1, 2)
    fixed_lit(w, ord("a"))
    fixed_lit(w, 257)  # length 3
    w.code(1, 5)  # distance 2: one byte before the start
    fixed_lit(w, 256)
    out.append(("before_start", w.done(), 4, INVALID))
    w = BitWriter().bits(1, 1).bits(1, 2)
    for _ in range(4):
        fixed_lit(w, ord("a"))
    fixed_lit(w, 257)
    w.code(30, 5)
    fixed_lit(w, 256)
    out.append(("dist30", w.done(), 7, INVALID))
    w = BitWriter().bits(1, 1).bits(1, 2)
    fixed_lit(w, ord("a"))
    fixed_lit(w, 286)
    w.code(0, 5)
    fixed_lit(w, 256)
    out.append(("lit286", w.done(), 4, INVALID))
    w = BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(15, 4)
    for _ in range(19):
        w.bits(1, 3)  # nineteen codes of one bit
    w.bits(0, 32)
    out.append(("oversubscribed", w.done(), 10, INVALID))
    for name, s, _, _ in out[:2] + out[3:]:
        assert zlib_verdict(s)[0] is None, name
    rng = random.Random(100)
    base = raw(bytes(rng.choice(b"ACGTN#FF:,") for _ in range(3000)), 6)
    assert len(base) > 200
    got, eof = zlib_verdict(base[:100])
    assert got is not None and not eof
    out.append(("cut100", base[:100], 3000, SIZE))
    out.append(("isize_less", base, 2999, SIZE))
    out.append(("isize_more", base, 3001, SIZE))
    return tuple((n, s, i, st, None) for n, s, i, st in out)


def mutations(n: int = 20000, seed: int = 7) -> list:
    """Single-byte and single-bit mutations of the valid streams with zlib's verdict: status
    0 (and the bytes) exactly when zlib decodes to exactly isize bytes and reaches the end
    of the stream. A case is drawn with weight 1 / (64 + its length), so the short streams,
    where a mutation more often lands in a header or a table, are mutated as often as the long."""
    rng = random.Random(seed)
    cases = [c for c in valid_cases() if len(c[1]) > 2]
    weights = [1.0 / (64 + len(c[1])) for c in cases]
    out = []
    for k in range(n):
        name, s, isize, _, _ = rng.choices(cases, weights)[0]
        b = bytearray(s)
        at = rng.randrange(len(b))
        if k & 1:
            b[at] ^= 1 << rng.randrange(8)
        else:
            b[at] = (b[at] + 1 + rng.randrange(255)) & 255
        m = bytes(b)
        got, eof = zlib_verdict(m)
        ok = got is not None and eof and len(got) == isize
        out.append((f"mut{k}_{name}@{at}", m, isize, OK if ok else ANY_ERROR, got if ok else None))
    return out


def write_corpus_file(path, cases) -> None:
    """The corpus as inflate_core_main reads it: u32 count, then per case u32 status, isize,
    clen, has_expected, the stream and (has_expected) the expected bytes."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _, s, isize, status, exp in cases:
            f.write(struct.pack("<IIII", status, isize, len(s), 1 if exp is not None else 0))
            f.write(s)
            if exp is not None:
                assert len(exp) == isize
                f.write(exp)


@functools.lru_cache(maxsize=None)
def odd_cases() -> tuple:
    """Valid streams of odd sizes (the others' bytes cut to an odd length and deflated again),
    so that blocks laid end to end abut at unaligned offsets."""
    out = []
    for k, (name, _, isize, _, exp) in enumerate(valid_cases()):
        if isize < 8 or k % 3:
            continue
        cut = exp[:(isize - 1 - 2 * (k % 5)) | 1]
        out.append((f"odd_{name}", raw(cut, 1 + k % 9), len(cut), OK, cut))
    return tuple(out)


def pack_blocks(cases):
    """src, coff, clen, isize, out_off (numpy) of the cases laid end to end; the outputs abut."""
    src = bytearray()
    coff, clen, isize, ooff = [], [], [], []
    o = 0
    for _, s, n, _, _ in cases:
        coff.append(len(src))
        clen.append(len(s))
        src += s
        isize.append(n)
        ooff.append(o)
        o += n
    return (np.frombuffer(bytes(src), np.uint8), np.array(coff, np.uint64), np.array(clen, np.uint32),
            np.array(isize, np.uint32), np.array(ooff, np.uint64), o)
