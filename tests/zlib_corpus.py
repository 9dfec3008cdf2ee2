"""The zlib streams (RFC 1950) the streaming-inflate tests share (test_inflate_zlib.py on the
CPU, test_gpu_table.py on the device), in the case shape of inflate_corpus.py: (name, stream,
isize, status, expected bytes or None); status as mgp_zlib_inflate reports it: 0 ok, 1 invalid
stream, 2 wrong size or input ended early, 3 Adler-32 differs or bytes follow the trailer."""

from __future__ import annotations

import functools
import random
import struct
import zlib

import numpy as np

from inflate_corpus import ANY_ERROR, INVALID, OK, SIZE, BitWriter, fixed_lit

CHECK = 3
SIZES = (0, 1, 32767, 32768, 32769, 65535, 65536, 65537, 200000, 262144)
LEVELS = (0, 1, 4, 9)


def zlib_verdict(stream: bytes, isize: int):
    """(ok, bytes): zlib.decompressobj() yields exactly isize bytes, reaches the end of the
    stream and leaves nothing unused."""
    d = zlib.decompressobj()
    try:
        out = d.decompress(stream, isize + 1)
    except zlib.error:
        return False, None
    ok = len(out) == isize and d.eof and not d.unused_data and not d.unconsumed_tail
    return ok, out if ok else None


def content(kind: str, n: int, seed: int = 0) -> bytes:
    """zero: matches of 258 at distance 1; counts: sparse u16 values as a count plane holds
    them; noise: random bytes (deflate stores them: blocks longer than a ring half)."""
    rng = np.random.default_rng(1950 + seed)
    if kind == "zero":
        return bytes(n)
    if kind == "noise":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    m = (n + 1) // 2
    v = np.where(rng.random(m) < 0.1, rng.poisson(4.0, m), 0).astype(np.uint16)
    v[rng.random(m) < 0.002] = 65535
    return v.tobytes()[:n]


def deflate(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, wbits: int = 15) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return co.compress(data) + co.flush()


def _stored(data: bytes) -> bytes:
    """A non-final stored block that starts on a byte boundary."""
    assert len(data) <= 65535
    return b"\x00" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data


def _far_block(final: bool, then_stored: bool) -> bytes:
    """A fixed block of one match, length 258 (symbol 285) at distance 32,768 (code 29, its
    13 extra bits all ones), and, unless final, the 3 header bits of a stored block after it."""
    w = BitWriter().bits(1 if final else 0, 1).bits(1, 2)
    fixed_lit(w, 285)
    w.code(29, 5).bits(0x1FFF, 13)
    fixed_lit(w, 256)
    if then_stored:
        w.bits(0, 3)
    return w.done()


def far_match_wrap() -> tuple[bytes, bytes]:
    """Stored noise up to 100 bytes before 65,536, a match of 258 at distance 32,768 (its
    copy straddles the ring's wrap), stored noise up to 100 bytes before 131,072 and the same
    match again, in the final block."""
    rng = random.Random(32768)
    out = bytearray()
    s = bytearray(b"\x78\x01")
    own_header = True  # the stored header's 3 bits: a byte of their own, or the far block's last bits
    for target, final in ((65536 - 100, False), (131072 - 100, True)):
        while len(out) < target:
            piece = rng.randbytes(min(40000, target - len(out)))
            s += _stored(piece) if own_header else _stored(piece)[1:]
            out += piece
            own_header = True
        s += _far_block(final, not final)
        own_header = False
        out += bytes(out[len(out) - 32768 + i] for i in range(258))
    exp = bytes(out)
    s += struct.pack(">I", zlib.adler32(exp))
    return bytes(s), exp


@functools.lru_cache(maxsize=None)
def valid_cases() -> tuple:
    cases = []
    for kind in ("zero", "counts"):
        for n in SIZES:
            for lv in LEVELS:
                cases.append((f"{kind}{n}_l{lv}", deflate(content(kind, n, lv), lv)))
    for n in SIZES:
        for lv in (0, 9):
            cases.append((f"noise{n}_l{lv}", deflate(content("noise", n, lv), lv)))
    for name, st in (("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("huffman_only", zlib.Z_HUFFMAN_ONLY)):
        for n in (1, 32769, 200000):
            cases.append((f"{name}{n}", deflate(content("counts", n, 7), 6, st)))
    for wb in range(9, 16):
        cases.append((f"wbits{wb}", deflate(content("counts", 70000, wb), 6, wbits=wb)))
    out = []
    for name, s in cases:
        exp = zlib.decompress(s)
        assert zlib_verdict(s, len(exp))[0], name
        out.append((name, s, len(exp), OK, exp))
    s, exp = far_match_wrap()
    assert zlib.decompress(s) == exp and len(exp) == 131072 - 100 + 258 and zlib_verdict(s, len(exp))[0]
    out.append(("far_match_wrap", s, len(exp), OK, exp))
    return tuple(out)


def _header(cmf: int, flg_high: int) -> bytes:
    """CMF and the FLG with these high three bits whose FCHECK is valid."""
    flg = flg_high & 0xE0
    flg += (31 - (cmf * 256 + flg) % 31) % 31
    return bytes([cmf, flg])


@functools.lru_cache(maxsize=None)
def invalid_cases() -> tuple:
    data = content("counts", 3000, 3)
    base = deflate(data, 6)
    body = base[2:]
    out = [
        ("bad_cm", _header(0x79, 0x80) + body, 3000, INVALID),
        ("cinfo8", _header(0x88, 0x80) + body, 3000, INVALID),
        ("fdict", _header(0x78, 0xA0) + body, 3000, INVALID),
        ("bad_fcheck", bytes([base[0], base[1] ^ 1]) + body, 3000, INVALID),
        ("trailer_cut1", base[:-1], 3000, SIZE),
        ("trailer_cut4", base[:-4], 3000, SIZE),
        ("adler", base[:-1] + bytes([base[-1] ^ 0x40]), 3000, CHECK),
        ("trailing_byte", base + b"\0", 3000, CHECK),
        ("isize_less", base, 2999, SIZE),
        ("isize_more", base, 3001, SIZE),
    ]
    w = BitWriter().bits(1, 1).bits(1, 2)
    fixed_lit(w, ord("a"))
    fixed_lit(w, 257)  # length 3
    w.code(1, 5)  # distance 2: one byte before the start
    fixed_lit(w, 256)
    out.append(("before_start", b"\x78\x01" + w.done() + struct.pack(">I", zlib.adler32(b"aaaa")), 4, INVALID))
    for name, s, isize, _ in out:
        assert not zlib_verdict(s, isize)[0], name
    return tuple((n, s, i, st, None) for n, s, i, st in out)


@functools.lru_cache(maxsize=None)
def padded_cases() -> tuple:
    """Valid streams rich in bits no decoder reads (the padding before a stored block's LEN):
    a few counts in stored blocks of a few bytes each with a sync flush's empty stored block
    after every one, so that a fair share of the single-bit mutations leaves the stream valid."""
    out = []
    for k, step in enumerate((1, 2, 3, 5)):
        data = content("counts", 12 + 4 * k, 40 + k)
        co = zlib.compressobj(0)
        s = b""
        for i in range(0, len(data), step):
            s += co.compress(data[i:i + step]) + co.flush(zlib.Z_SYNC_FLUSH)
        s += co.flush()
        assert zlib.decompress(s) == data
        out.append((f"padded{step}", s, len(data), OK, data))
    return tuple(out)


def mutations(n: int = 20000, seed: int = 11) -> list:
    """Single-byte and single-bit mutations of the valid streams with zlib's verdict: status 0
    (and the bytes) exactly when zlib.decompressobj() yields exactly isize bytes with eof and
    nothing unused. Two draws in three mutate a stream of padded_cases(), the third any valid
    stream of up to 4,096 bytes with weight 1 / (64 + its length); three mutations in four
    flip one bit, the fourth replaces one byte."""
    rng = random.Random(seed)
    small = [c for c in valid_cases() if len(c[1]) <= 4096]
    weights = [1.0 / (64 + len(c[1])) for c in small]
    padded = padded_cases()
    out = []
    for k in range(n):
        name, s, isize, _, _ = rng.choice(padded) if k % 3 else rng.choices(small, weights)[0]
        b = bytearray(s)
        at = rng.randrange(len(b))
        if k & 3:
            b[at] ^= 1 << rng.randrange(8)
        else:
            b[at] = (b[at] + 1 + rng.randrange(255)) & 255
        m = bytes(b)
        ok, got = zlib_verdict(m, isize)
        out.append((f"mut{k}_{name}@{at}", m, isize, OK if ok else ANY_ERROR, got))
    return out
