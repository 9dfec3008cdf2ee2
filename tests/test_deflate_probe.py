"""The instrumented inflate of the tests (deflate_probe.py) pinned to zlib: it decodes what
zlib decodes, names the block kinds zlib is known to write, and refuses corrupted streams.
The device deflate's tests (test_gpu_deflate_edges.py) stand on it."""

from __future__ import annotations

import zlib
from fractions import Fraction

import numpy as np
import pytest

import deflate_probe as dp


def _count_text() -> bytes:
    rng = np.random.default_rng(11)
    return "".join(f"{p + 1},ACGTACGTACGTACGT-1,{int(rng.integers(1, 400))},{int(rng.integers(0, 30))}\n"
                   for p in range(3000)).encode()


DATA = {
    "empty": b"",
    "one_byte": b"\x9c",
    "random_70000": np.random.default_rng(5).integers(0, 256, 70_000, dtype=np.uint8).tobytes(),
    "zeros_300000": bytes(300_000),
    "count_text": _count_text(),
}


def _compress(data: bytes, wbits: int, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return c.compress(data) + c.flush()


def _probe(stream: bytes, wbits: int) -> dp.Probe:
    return dp.probe_gzip(stream) if wbits == 31 else dp.probe_zlib(stream)


@pytest.mark.parametrize("wbits", [31, 15])
@pytest.mark.parametrize("name", list(DATA))
@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_probe_decodes_what_zlib_decodes(name, level, wbits):
    data = DATA[name]
    stream = _compress(data, wbits, level)
    p = _probe(stream, wbits)
    assert p.data == zlib.decompress(stream, wbits) == data
    assert [b.bfinal for b in p.blocks] == [0] * (len(p.blocks) - 1) + [1]
    assert sum(b.n_bytes for b in p.blocks) == len(data)
    # the blocks tile the deflate stream: each starts where the one before ended
    at = 0
    for b in p.blocks:
        assert b.start_bit == at
        at += b.bits
    assert (at + 7) // 8 == p.deflate_bytes == len(stream) - (18 if wbits == 31 else 6)
    if level == 0:
        assert set(p.btypes) == {0}
        lens = [b.stored_len for b in p.blocks]
        assert sum(lens) == len(data) and all(0 <= x <= 65535 for x in lens)
        if name == "random_70000":
            assert len(lens) >= 2  # (several stored blocks)
    elif name == "random_70000":
        assert set(p.btypes) == {0}  # (incompressible: zlib stores it at every level)
    elif name in ("empty", "one_byte"):
        assert p.btypes == [1]
    else:
        assert set(p.btypes) == {2}
    for b in p.blocks:
        if b.btype == 0:
            continue
        assert b.lit_hist[256] == 1
        assert sum(b.lit_hist[:256]) + sum(ln for ln, _ in (t for t in b.tokens if isinstance(t, tuple))) == b.n_bytes
    if name == "zeros_300000" and level:
        b = p.blocks[0]
        assert b.max_len == 258 and b.kraft_lit == 1
        if level > 1:  # (level 1's fast matcher may take a run from further back)
            assert b.max_dist == 1 and sum(1 for x in b.dist_hist if x) == 1
        assert b.kraft_dist <= 1


@pytest.mark.parametrize("wbits", [31, 15])
@pytest.mark.parametrize("name", ["one_byte", "zeros_300000", "count_text"])
def test_probe_names_fixed_and_huffman_only_blocks(name, wbits):
    data = DATA[name]
    fx = _probe(_compress(data, wbits, 6, zlib.Z_FIXED), wbits)
    assert fx.data == data and set(fx.btypes) == {1}
    for b in fx.blocks:
        assert b.bits == 3 + dp.fixed_bits(b)
    ho = _probe(_compress(data, wbits, 6, zlib.Z_HUFFMAN_ONLY), wbits)
    assert ho.data == data
    assert all(b.max_len == 0 and sum(b.dist_hist) == 0 for b in ho.blocks)
    if name != "one_byte":
        assert set(ho.btypes) == {2}


def test_probe_dynamic_header_stats_add_up():
    """The header fields of zlib's dynamic blocks: the code-length symbols expand to HLIT + HDIST
    lengths, the block's bits are its header, its coded symbols and their extra bits, and
    zlib's codes are optimal where their depth allows it (the helpers' own check)."""
    p = dp.probe_zlib(zlib.compress(DATA["count_text"], 9))
    assert set(p.btypes) == {2}
    for b in p.blocks:
        assert 257 <= b.hlit <= 286 and 1 <= b.hdist <= 30 and 4 <= b.hclen <= 19
        assert len(b.lit_lengths) == b.hlit and len(b.dist_lengths) == b.hdist and len(b.cl_lengths) == 19
        h = b.cl_hist
        assert sum(h) == len(b.cl_syms) and all(h[s] == 0 or b.cl_lengths[s] for s in range(19))
        assert b.lit_lengths[b.hlit - 1] or b.hlit == 257
        coded = (sum(n * b.lit_lengths[s] for s, n in enumerate(b.lit_hist[:b.hlit]))
                 + sum(n * b.dist_lengths[s] for s, n in enumerate(b.dist_hist[:b.hdist])))
        assert b.bits == b.header_bits + coded + dp.extra_bits(b)
        depth, cost = dp.huffman_depth_cost(b.lit_hist)
        assert depth <= 15 and sum(n * b.lit_lengths[s] for s, n in enumerate(b.lit_hist[:b.hlit])) == cost
        assert b.kraft_lit == 1 and b.kraft_cl == 1


def test_huffman_helpers():
    fib = [1, 1, 2, 3, 5, 8, 13, 21]
    assert dp.huffman_depth_cost(fib) == (7, sum(c * l for c, l in zip(fib, [7, 7, 6, 5, 4, 3, 2, 1])))
    assert dp.huffman_depth_cost([4, 0, 4, 4, 4]) == (2, 32)
    assert dp.huffman_depth_cost([0, 9]) == (1, 9)
    assert dp.package_merge_cost(fib, 7) == dp.huffman_depth_cost(fib)[1]
    # limit 4 for 8 symbols: brute force over the sorted length vectors
    best = None
    import itertools
    for ls in itertools.product(range(1, 5), repeat=8):
        if list(ls) == sorted(ls, reverse=True) and dp.kraft(ls) <= 1:
            c = sum(a * b for a, b in zip(fib, ls))
            best = c if best is None else min(best, c)
    assert dp.package_merge_cost(fib, 4) == best > dp.huffman_depth_cost(fib)[1]
    assert dp.package_merge_cost(fib, 3) == 3 * sum(fib)
    assert [dp.len_symbol(x) for x in (3, 10, 11, 12, 257, 258)] == [257, 264, 265, 265, 284, 285]
    assert [dp.dist_symbol(x) for x in (1, 4, 5, 6, 7, 16384, 16385, 24577, 32768)] == [0, 3, 4, 4, 5, 27, 28, 29, 29]
    assert dp.stored_bytes(0) == 5 and dp.stored_bytes(65534) == 65539 and dp.stored_bytes(65535) == 65545


def _flip(b: bytes, at: int, mask: int = 0xFF) -> bytes:
    a = bytearray(b)
    a[at] ^= mask
    return bytes(a)


def test_probe_refuses_corrupted_streams():
    data = DATA["random_70000"]
    gz = _compress(data, 31, 0)
    zz = _compress(data, 15, 0)
    assert dp.probe_gzip(gz).data == data and dp.probe_zlib(zz).data == data
    with pytest.raises(dp.ProbeError, match="LEN"):
        dp.probe_gzip(_flip(gz, 10 + 3, 0x01))  # NLEN of the first stored block
    with pytest.raises(dp.ProbeError, match="LEN"):
        dp.probe_zlib(_flip(zz, 2 + 4, 0x80))
    for cut in (1, 4, 8):
        with pytest.raises(dp.ProbeError):
            dp.probe_gzip(gz[:-cut])  # a truncated trailer
    with pytest.raises(dp.ProbeError):
        dp.probe_zlib(zz[:-1])
    with pytest.raises(dp.ProbeError, match="CRC-32"):
        dp.probe_gzip(_flip(gz, len(gz) - 8, 0x10))  # a wrong CRC
    with pytest.raises(dp.ProbeError, match="CRC-32"):
        dp.probe_gzip(_flip(gz, len(gz) - 1, 0x01))  # a wrong ISIZE
    with pytest.raises(dp.ProbeError, match="Adler-32"):
        dp.probe_zlib(_flip(zz, len(zz) - 2))
    with pytest.raises(dp.ProbeError):
        dp.probe_gzip(gz + b"\0")  # bytes after the trailer
    with pytest.raises(dp.ProbeError):
        dp.probe_zlib(zz + b"\0")
    with pytest.raises(dp.ProbeError):
        dp.probe_zlib(_flip(zz, 0, 0x01))  # the zlib header's check bits


def _bits_to_bytes(bits: str) -> bytes:
    bits += "0" * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8][::-1], 2) for i in range(0, len(bits), 8))


def test_probe_refuses_bad_codes_and_distances():
    # fixed block: a match of length 3 at distance 1 with nothing before it
    # (BFINAL 1, BTYPE 01 LSB first = "1" "10"; symbol 257 = 0000001; distance 0 = 00000)
    with pytest.raises(dp.ProbeError, match="before the start"):
        dp.probe_deflate(_bits_to_bytes("1" + "10" + "0000001" + "00000" + "0000000"))
    # a literal, then the same match: fine ('a' = 0x61 -> 8-bit code 0x30 + 0x61 = 10010001)
    ok = dp.probe_deflate(_bits_to_bytes("1" + "10" + "10010001" + "0000001" + "00000" + "0000000"))
    assert ok.data == b"aaaa" and ok.blocks[0].tokens == [0x61, (3, 1)]
    # dynamic block whose code-length code is over-subscribed: three symbols of length 1
    hdr = "1" + "01" + "00000" + "00000" + "0000"  # HLIT 257, HDIST 1, HCLEN 4: symbols 16, 17, 18, 0
    with pytest.raises(dp.ProbeError, match="over-subscribed"):
        dp.probe_deflate(_bits_to_bytes(hdr + "100" + "100" + "100" + "000" + "0" * 64))
    # dynamic block whose code-length code is incomplete (18 alone, length 1) and whose unused
    # code is then sent: a symbol without a code
    with pytest.raises(dp.ProbeError, match="without a code"):
        dp.probe_deflate(_bits_to_bytes(hdr + "000" + "000" + "100" + "000" + "1" * 64))
    # incomplete codes are recorded, not refused: code-length code {18: 1 bit, 1: 2 bits}, 256
    # zero lengths (138 + 118), then length 1 for the end of block and for distance 0
    cl = ["000"] * 18
    cl[2], cl[17] = "100", "010"
    inc = dp.probe_deflate(_bits_to_bytes("1" + "01" + "00000" + "00000" + "0111" + "".join(cl)
                                          + "0" + "1111111" + "0" + "1101011" + "10" + "10" + "0"))
    b = inc.blocks[0]
    assert inc.data == b"" and (b.hlit, b.hdist, b.hclen) == (257, 1, 18) and b.cl_syms == [18, 18, 1, 1]
    assert (b.kraft_cl, b.kraft_lit, b.kraft_dist) == (Fraction(3, 4), Fraction(1, 2), Fraction(1, 2))
    assert b.bits == 17 + 54 + 8 + 8 + 2 + 2 + 1 and b.cl_hist[18] == 2 and b.cl_hist[16] == b.cl_hist[17] == 0
    with pytest.raises(dp.ProbeError, match="BTYPE 3"):
        dp.probe_deflate(_bits_to_bytes("1" + "11" + "0" * 16))


# ---- the invariants and the model the device tests rest on ----
def _block(lit: dict, dist: dict, lit_len: dict, dist_len: dict) -> dp.Block:
    """A hand-built dynamic block: symbol counts and code lengths, its header as the run-length
    code of those lengths under an optimal code-length code."""
    b = dp.Block(btype=2, bfinal=1)
    for s, n in lit.items():
        b.lit_hist[s] = n
    for s, n in dist.items():
        b.dist_hist[s] = n
    b.hlit = max([257] + [s + 1 for s in lit_len if s > 256])
    b.hdist = max(s + 1 for s in dist_len)
    b.lit_lengths = [lit_len.get(s, 0) for s in range(b.hlit)]
    b.dist_lengths = [dist_len.get(s, 0) for s in range(b.hdist)]
    syms = dp.code_length_symbols(b.lit_lengths + b.dist_lengths)
    b.cl_syms = [s for s, _ in syms]
    b.cl_lengths = dp.documented_huffman_lengths(b.cl_hist, 7)
    b.hclen = max([4] + [i + 1 for i in range(19) if b.cl_lengths[dp.CL_ORDER[i]]])
    b.header_bits = 17 + 3 * b.hclen + sum(b.cl_lengths[s] + {16: 2, 17: 3, 18: 7}.get(s, 0) for s, _ in syms)
    coded = sum(n * b.lit_lengths[s] for s, n in lit.items()) + sum(n * b.dist_lengths[s] for s, n in dist.items())
    b.bits = b.header_bits + coded + dp.extra_bits(b)
    return b


GOOD = dict(lit={65: 8, 66: 4, 67: 2, 68: 1, 256: 1, 260: 3}, dist={0: 2, 5: 1},
            lit_len={65: 1, 66: 3, 260: 3, 67: 3, 68: 4, 256: 4}, dist_len={0: 1, 5: 1})


def test_check_dynamic_block_accepts_a_good_block_and_refuses_bad_ones():
    st = dp.check_dynamic_block(_block(**GOOD))
    assert st["lit_depth"] == 4 and st["lit_max_len"] == 4 and st["dist_max_len"] == 1

    def bad(match, **change):
        kw = {k: dict(v) for k, v in GOOD.items()}
        for k, v in change.items():
            kw[k].update(v)
        with pytest.raises(AssertionError, match=match):
            dp.check_dynamic_block(_block(**kw))

    bad("Fraction", lit_len={65: 2})                      # incomplete literal/length code
    bad("Fraction", dist_len={5: 2})                      # incomplete distance code
    bad("has 3 bits", lit_len={65: 3, 66: 1})             # the frequent symbol's code swapped with a rarer one's
    bad("the optimum is", lit_len={65: 2, 66: 2, 260: 2, 67: 3, 68: 4, 256: 4})  # complete, monotone, not optimal
    bad("without a code", lit={70: 1})                    # a used symbol with length 0
    b = _block(**GOOD)
    b.hlit += 1
    b.lit_lengths.append(0)
    with pytest.raises(AssertionError, match="HLIT"):
        dp.check_dynamic_block(b)
    b = _block(**GOOD)
    b.bits += 1
    with pytest.raises(AssertionError):
        dp.check_dynamic_block(b)


def test_code_report_refuses_swapped_lengths_clipped_and_unclipped():
    """A length assignment dealt to the wrong symbols, where the cost checks cannot see it: a
    clipped code (only bits >= optimum holds there) and an unclipped one."""
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34]
    assert dp.huffman_depth_cost(fib)[0] == 8
    good = dp.documented_huffman_lengths(fib, 4)
    assert max(good) == 4 and dp.kraft(good) == 1
    dp._code_report("x", fib, good, 4, {})
    with pytest.raises(AssertionError, match="has 4 bits"):
        dp._code_report("x", fib, [1, 4, 4, 4, 4, 4, 4, 4, 4], 4, {})  # the rarest has the 1-bit code
    swapped = list(good)
    swapped[0], swapped[8] = swapped[8], swapped[0]
    assert swapped != good
    with pytest.raises(AssertionError, match="bits, count"):
        dp._code_report("x", fib, swapped, 4, {})
    with pytest.raises(AssertionError, match="bits, count"):
        dp._code_report("x", fib, good[::-1], 4, {})  # dealt shortest to rarest
    # unclipped: counts 1, 1, 2, 2 with lengths 3, 1, 2, 3
    with pytest.raises(AssertionError, match="bits, count"):
        dp._code_report("x", [1, 1, 2, 2], [3, 1, 2, 3], 15, {})
    dp._code_report("x", [1, 1, 2, 2], [2, 2, 2, 2], 15, {})
    with pytest.raises(AssertionError, match="limit 4"):
        dp._code_report("x", fib, dp.documented_huffman_lengths(fib, 15), 4, {})


def test_documented_lengths_and_header_model():
    """The model of the encoder's procedure: complete codes within the limit, optimal when nothing
    is clipped, never better than package-merge; the run-length code of the lengths; and on
    zlib's own dynamic blocks (whose gen_bitlen is the same procedure) the model's block size
    is zlib's."""
    rng = np.random.default_rng(3)
    for trial in range(60):
        n = int(rng.integers(2, 40))
        f = [int(x) for x in rng.integers(0, 5, n) * rng.integers(1, 2000, n)]
        if trial % 3 == 0:
            f = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89][:max(2, n % 12)]
        used = [x for x in f if x]
        if len(used) < 2:
            continue
        for limit in (7, 15):
            l = dp.documented_huffman_lengths(f, limit)
            assert dp.kraft(l) == 1 and max(l) <= limit and all(bool(a) == bool(b) for a, b in zip(f, l))
            depth, cost = dp.huffman_depth_cost(f)
            bits = sum(a * b for a, b in zip(f, l))
            assert bits == cost if depth <= limit else bits >= dp.package_merge_cost(f, limit) > cost
            dp._code_report("x", f, l, limit, {})
    assert dp.documented_huffman_lengths([0, 7, 0], 15) == [0, 1, 0]
    assert dp.code_length_symbols([0] * 139 + [5] * 8 + [0, 0] + [3] * 3 + [0] * 3 + [2] * 4) == \
        [(18, 127), (0, 0), (5, 0), (16, 3), (5, 0), (0, 0), (0, 0), (3, 0), (3, 0), (3, 0), (17, 0), (2, 0), (16, 0)]
    for data, level in ((DATA["count_text"], 9), (DATA["zeros_300000"], 6)):
        for b in dp.probe_zlib(zlib.compress(data, level)).blocks:
            m = dp.documented_dynamic_bits(b.lit_hist, b.dist_hist, dp.extra_bits(b))
            assert (m["bits"], m["header_bits"], m["hlit"], m["hdist"], m["hclen"]) == \
                (b.bits, b.header_bits, b.hlit, b.hdist, b.hclen)
            assert sorted(m["lit"][:b.hlit]) == sorted(b.lit_lengths)  # (zlib breaks ties among equal counts its own way)
            dp.check_dynamic_block(b)


def test_check_block_choice():
    """Fixed output that is the smallest kind passes; zlib's Z_FIXED output of compressible text
    does not (a dynamic block is smaller); stored streams need their literals and are weighed."""
    assert "BTYPE 1" in dp.check_block_choice(dp.probe_zlib(_compress(b"\x9c", 15, 6, zlib.Z_FIXED)).blocks)
    assert "BTYPE 1" in dp.check_block_choice(dp.probe_zlib(_compress(b"ab,1\n", 15, 9)).blocks)
    with pytest.raises(AssertionError, match="BTYPE 1 written"):
        dp.check_block_choice(dp.probe_zlib(_compress(DATA["count_text"][:20000], 15, 6, zlib.Z_FIXED)).blocks[:1])
    p = dp.probe_zlib(zlib.compress(DATA["count_text"][:20000], 9))
    assert len(p.blocks) == 1 and "BTYPE 2" in dp.check_block_choice(p.blocks)
    rnd = DATA["random_70000"]
    st = dp.probe_zlib(_compress(rnd, 15, 0))
    with pytest.raises(AssertionError, match="cannot know"):
        dp.check_block_choice(st.blocks)
    lens = [b.stored_len for b in st.blocks]
    if lens == [65535, 70000 - 65535]:  # (the format's fewest blocks: what stored_bytes counts)
        assert "BTYPE 0" in dp.check_block_choice(st.blocks, rnd)
    # compressible bytes written stored: refused
    zeros = dp.probe_zlib(_compress(bytes(1000), 15, 0))
    with pytest.raises(AssertionError, match="BTYPE 0 written"):
        dp.check_block_choice(zeros.blocks, bytes(1000))
    # a stream with an extra empty stored block is not the size the format needs
    one = dp.probe_deflate(b"\x00\x02\x00\xfd\xff\xf0\xf1" + b"\x01\x00\x00\xff\xff")
    assert one.data == b"\xf0\xf1" and [b.stored_len for b in one.blocks] == [2, 0]
    with pytest.raises(AssertionError):
        dp.check_block_choice(one.blocks, one.data)
