"""GPU: the device deflate (mgatk2_amd/csrc/mgp_txtgz.hip: huff_lengths, deflate_block,
k_h5_code, k_txt_code) at the format's edges, through mgp_h5_tiles_rows and mgp_txt_gz_rows.

Every stream is decoded by the tests' own inflate (deflate_probe.py, pinned to zlib by
test_deflate_probe.py) and compared with bytes built here from numpy or plain Python; then
the case asserts, from the probe's statistics, that it reached the branch it is there for,
and every block is held to the invariants of deflate_probe.check_dynamic_block (complete
codes, length limits, monotone lengths, the optimal cost when nothing was clipped) and
check_block_choice (the smallest of dynamic, fixed and stored was written).

Measured on an MI355X (the figures the cases print):
* literal/length code clipped at 15: 4,180 bytes over 16 values (unrestricted depth 16): 10,927
  coded bits, package-merge 10,927 (ratio 1.00000), unrestricted 10,926; 17,710 bytes over 19
  values (depth 19): 46,375 bits, package-merge 46,349 (ratio 1.00056), unrestricted 46,345; both
  blocks dynamic, longest code 15;
* code-length code clipped at 7: 2,048 bytes whose 79 literal lengths and zero runs give the
  code-length histogram 1:2 4:3 5:13 6:21 7:1 9:34 11:8 17:5 18:1, unrestricted depth 8: 221 bits,
  package-merge 221, unrestricted 220, longest code 7;
* stored: LENs (65535, 65535, 0), (65535, 65535, 514) and (40), BFINAL on the last block only;
* chunks of 2, 14 and 30 bytes: fixed blocks (those with bytes from 144 did not inflate to their
  input before deflate_block's fixed code was mended);
* runs in 288-byte segments: match lengths [258], [258], [258], [258, 257], [258, 258] for R = 259,
  260, 261, 516, 517; in (16, 16) chunks R = 259 gives [258] and R = 511 [258, 252] (with the
  16-byte segments such chunks had before, R = 511 gave 30, 16, 16, ...);
* txt: BTYPE 1 for one-line members, 0 for the 4,096-byte barcode of all byte values, 2 for 400
  lines; the far match is (31 bytes, distance 16,416), distance symbol 28 used once; 16,569 lines
  under the empty barcode: 138,015 bytes, longest match 8, largest distance 144.
"""

from __future__ import annotations

import ctypes as C
import gzip

import numpy as np
import pytest

import deflate_probe as dp

pytestmark = pytest.mark.gpu

FILES = ("coverage", "A", "C", "G", "T")


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def check_stream(p: dp.Probe, literal_parse: bool = False) -> list:
    """The per-block invariants of one stream; returns what was measured per dynamic block.
    literal_parse: the input can only parse to literals (what a stored stream, which shows no
    tokens, was weighed as)."""
    stats = []
    for b in p.blocks:
        if b.btype == 2:
            stats.append(dp.check_dynamic_block(b))
    assert [b.bfinal for b in p.blocks] == [0] * (len(p.blocks) - 1) + [1]
    dp.check_block_choice(p.blocks, p.data if literal_parse else None)
    return stats


def no_equal_neighbours(b: bytes) -> bool:
    a = np.frombuffer(b, np.uint8)
    return bool(np.all(a[1:] != a[:-1]))


def arrange(hist: dict) -> bytes:
    """The bytes of `hist` (value -> count) in an order with no two equal neighbours: the
    values by falling count into the even places, then the odd ones."""
    seq = [v for v, n in sorted(hist.items(), key=lambda x: (-x[1], x[0])) for _ in range(n)]
    out = [0] * len(seq)
    out[0::2] = seq[:(len(seq) + 1) // 2]
    out[1::2] = seq[(len(seq) + 1) // 2:]
    b = bytes(out)
    assert no_equal_neighbours(b)
    return b


def zigzag(n: int, lo: int = 1, span: int = 100, avoid: int = -1) -> bytes:
    """n bytes with no equal neighbours (and none equal to `avoid`): a pattern that never repeats
    a byte within three places."""
    vals = [v for v in range(lo, lo + span) if v != avoid]
    return bytes(vals[(7 * i) % len(vals)] for i in range(n))


def plane_of_bytes(raw: bytes, crow: int, ccol: int) -> np.ndarray:
    assert len(raw) == 2 * crow * ccol
    return np.frombuffer(raw, "<u2").reshape(crow, ccol).astype(np.uint32)


def expected_chunks(plane16: np.ndarray, chunks) -> list:
    """The padded (crow, ccol) chunks of a u16 plane [L][n_cols], row-major over the grid."""
    crow, ccol = chunks
    L, nco = plane16.shape
    out = []
    for r0 in range(0, L, crow):
        for c0 in range(0, nco, ccol):
            ch = np.zeros((crow, ccol), "<u2")
            blk = plane16[r0:r0 + crow, c0:c0 + ccol]
            ch[:blk.shape[0], :blk.shape[1]] = blk
            out.append(ch.tobytes())
    return out


def coverage_tiles(engine, plane: np.ndarray, chunks, sums=None) -> dict:
    """mgp_h5_tiles_rows with `plane` ([L][n_cols], u32) as the coverage plane (column j is row
    j's depth), every other plane zero."""
    L, nco = plane.shape
    depth = np.ascontiguousarray(plane.T, np.uint32)
    counts = np.zeros((nco, L, 8), np.uint32)
    tn5 = np.zeros((nco, L, 2), np.uint32)
    return engine.h5_tiles_rows(counts, tn5, depth, np.arange(nco), chunks, sums=sums)


def check_coverage_tiles(engine, tiles: dict, plane: np.ndarray, chunks) -> list:
    """Every chunk of every plane decoded and compared: the coverage plane with min(plane,
    65535), the other ten with zeros; all blocks held to the invariants. Returns the coverage
    chunks' probes."""
    exp = expected_chunks(np.minimum(plane, 65535).astype("<u2"), chunks)
    zero = bytes(2 * chunks[0] * chunks[1])
    probes = []
    for name in engine.H5_PLANES:
        got = tiles[name]
        assert len(got) == len(exp), name
        for i, g in enumerate(got):
            p = dp.probe_zlib(g.tobytes())
            want = exp[i] if name == "coverage" else zero
            assert p.data == want, f"{name} chunk {i}"
            check_stream(p, literal_parse=no_equal_neighbours(want))
            if name == "coverage":
                probes.append(p)
            else:
                assert p.blocks[0].max_dist <= 1 and p.blocks[0].max_len <= 258
    return probes


def fib_chain(k: int) -> list:
    a = [1, 2]
    while len(a) < k:
        a.append(a[-1] + a[-2])
    return a[:k]


# ---------------------------------------------------------------------------
# cases through mgp_h5_tiles_rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,shape", [(16, (209, 10)), (19, (1771, 5))])
def test_h5_literal_length_code_clipped_at_15(engine_lib, k, shape):
    """k byte values with counts 1, 2, 3, 5, ... (one more on the largest, for an even size) and
    no two equal neighbours: with EOB's 1 the unrestricted Huffman tree is a chain k deep, so
    huff_lengths clips at 15 and repairs the Kraft sum (k = 19: many steps of the first loop)."""
    counts = fib_chain(k)
    counts[-1] += 1
    hist = {37 + 11 * i: n for i, n in enumerate(counts)}  # values on both sides of 144
    raw = arrange(hist)
    assert len(raw) == 2 * shape[0] * shape[1]
    lit = [0] * 286
    for v, n in hist.items():
        lit[v] = n
    lit[256] = 1
    depth, cost = dp.huffman_depth_cost(lit)
    assert depth == k > 15  # (the input alone decides this)
    plane = plane_of_bytes(raw, *shape)
    tiles = coverage_tiles(engine_lib, plane, shape)
    (p,) = check_coverage_tiles(engine_lib, tiles, plane, shape)
    (b,) = p.blocks
    assert b.btype == 2 and b.max_len == 0 and b.lit_hist[:286] == lit
    st = dp.check_dynamic_block(b)
    assert st["lit_depth"] == k and st["lit_max_len"] == 15 and "lit_clipped_ratio" in st
    print(f"fib {k}: {len(raw)} bytes, BTYPE {p.btypes}, lit depth {depth} -> max length {st['lit_max_len']}, "
          f"coded {st['lit_bits']} bits, unrestricted {cost}, ratio to package-merge {st['lit_clipped_ratio']:.5f}, "
          f"cl depth {st.get('cl_depth')} max {st['cl_max_len']}")


def cl_clip_bytes() -> tuple[bytes, list]:
    """2,048 bytes whose literal code lengths are known (dyadic counts: a value of length l occurs
    2^(11 - l) times, EOB once, one more of the most frequent value for an even size) and laid
    out over the byte values so that the header's run-length code has the symbol counts
    1 (18: the 138 unused values at the end), 1 (length 7), 2 (the two distance codes of length
    1), 3 (4), 5 (17: five gaps of 3 to 10 unused values), 8 (11), 13 (5), 21 (6), 34 (9): a
    Fibonacci chain of nine code-length symbols, depth 8 > 7. Found by a search over the
    assignments of those counts to lengths whose Kraft sum is 1; equal lengths never sit on
    four neighbouring values, so no repeat symbol (16) merges them."""
    n_of_len = {4: 3, 5: 13, 6: 21, 7: 1, 9: 34, 11: 8}  # 11: 7 values and EOB
    rem = dict(n_of_len)
    rem[11] -= 1
    seq = []
    while any(rem.values()):
        c = [l for l in rem if rem[l] and (not seq or l != seq[-1])] or [l for l in rem if rem[l]]
        l = max(c, key=lambda x: (rem[x], x))
        seq.append(l)
        rem[l] -= 1
    zeros = 256 - len(seq) - 138
    gaps = [zeros // 5 + (1 if i < zeros % 5 else 0) for i in range(5)]
    hist, lengths, v = {}, [0] * 256, 0
    for i, l in enumerate(seq):
        hist[v] = 1 << (11 - l)
        lengths[v] = l
        v += 1 + (gaps[i] if i < 5 else 0)
    assert v + 138 == 256 and all(3 <= g <= 10 for g in gaps)
    top = max(hist, key=lambda s: (hist[s], -s))
    hist[top] += 1
    return arrange(hist), lengths


def test_h5_code_length_code_clipped_at_7(engine_lib):
    raw, lengths = cl_clip_bytes()
    shape = (64, 16)
    assert len(raw) == 2048 == 2 * shape[0] * shape[1]
    plane = plane_of_bytes(raw, *shape)
    tiles = coverage_tiles(engine_lib, plane, shape)
    (p,) = check_coverage_tiles(engine_lib, tiles, plane, shape)
    (b,) = p.blocks
    assert b.btype == 2 and b.max_len == 0
    assert b.lit_lengths[:256] == lengths and b.lit_lengths[256] == 11  # the dyadic counts' own lengths
    depth, cost = dp.huffman_depth_cost(b.cl_hist)
    st = dp.check_dynamic_block(b)
    print(f"cl clip: code-length histogram {b.cl_hist} (16/17/18 used {b.cl_hist[16:]}), depth {depth}, "
          f"lengths {b.cl_lengths}, coded {st['cl_bits']} bits, unrestricted {cost}, "
          f"ratio to package-merge {st.get('cl_clipped_ratio')}")
    assert depth > 7 and st["cl_max_len"] == 7 and "cl_clipped_ratio" in st


def random_no_neighbours(rng, n: int, lo: int = 0) -> bytes:
    a = rng.integers(lo, 256, n).astype(np.int64)
    while True:
        eq = np.flatnonzero(a[1:] == a[:-1]) + 1
        if eq.size == 0:
            return a.astype(np.uint8).tobytes()
        a[eq] = rng.integers(lo, 256, eq.size)


@pytest.mark.parametrize("shape,lens", [((255, 257), (65535, 65535, 0)), ((256, 257), (65535, 65535, 514)),
                                        ((4, 5), (40,))])
def test_h5_stored_blocks(engine_lib, shape, lens):
    """Random bytes (redrawn where two neighbours were equal, so the run parse can only give
    literals): stored, in blocks of 65,535 bytes; 131,070 bytes end on an empty final block. The
    (4, 5) chunk holds bytes >= 144, 9 bits each under the fixed code."""
    rng = np.random.default_rng(shape[0])
    raw = random_no_neighbours(rng, 2 * shape[0] * shape[1], lo=144 if shape == (4, 5) else 0)
    plane = plane_of_bytes(raw, *shape)
    tiles = coverage_tiles(engine_lib, plane, shape)
    (p,) = check_coverage_tiles(engine_lib, tiles, plane, shape)
    print(f"stored {shape}: BTYPE {p.btypes}, LEN {[b.stored_len for b in p.blocks]}, BFINAL {[b.bfinal for b in p.blocks]}")
    assert p.btypes == [0] * len(lens)
    assert tuple(b.stored_len for b in p.blocks) == lens
    assert [b.bfinal for b in p.blocks] == [0] * (len(lens) - 1) + [1]
    assert len(tiles["coverage"][0]) == 2 + len(raw) + 5 * len(lens) + 4


RUNS = (2, 3, 15, 16, 17, 31, 32, 33, 258, 259, 260, 261, 511)
OFFSETS = (0, 1, 15, 16)


def run_chunk(R: int, off: int, n: int = 512, span: int = 100) -> tuple[bytes, int]:
    """n bytes: a no-neighbours pattern, and at `off` one differing byte followed by a run of R
    bytes 0xEE (cut at the chunk's end: R = 511 fits at offset 0 only). Returns the run's length."""
    a = bytearray(zigzag(n, 1, span))
    r = min(R, n - off - 1)
    a[off] = 0xDD
    a[off + 1:off + 1 + r] = b"\xee" * r
    return bytes(a), r


def run_tiles(engine, shape, offsets, runs, span: int = 100):
    """One plane of len(runs) x len(offsets) column chunks, one crafted chunk each."""
    crow, ccol = shape
    chunks = [run_chunk(R, off, 2 * crow * ccol, span) for R in runs for off in offsets]
    plane = np.concatenate([plane_of_bytes(c, crow, ccol) for c, _ in chunks], axis=1)
    tiles = coverage_tiles(engine, plane, shape)
    return chunks, check_coverage_tiles(engine, tiles, plane, shape)


MIN_SEG = 272  # a thread's segment is never shorter (kH5MinSeg, mgp_txtgz.h)


def expected_run_matches(r: int) -> list:
    """The match lengths of a run of r equal bytes that is one thread's: its first byte is a
    literal, every 258 pending bytes become a match, what is left a match or one or two literals."""
    rem = (r - 1) % 258
    return [258] * ((r - 1) // 258) + ([rem] if rem >= 3 else [])


def check_runs(chunks, probes, runs, offsets, seg: int, show=()):
    """Every crafted chunk decodes to its bytes with distance 1 only and no length past 258, and
    a run that is one thread's (it ends before the second segment after its start) is coded as
    expected_run_matches says, so length 258 occurs where the run holds 259 bytes and more."""
    k = 0
    for R in runs:
        for off in offsets:
            (raw, r), p = chunks[k], probes[k]
            k += 1
            assert p.data == raw
            (b,) = p.blocks
            matches = [t for t in b.tokens if isinstance(t, tuple)]
            lens = [ln for ln, _ in matches]
            assert all(d == 1 for _, d in matches), (R, off)
            assert all(3 <= ln <= 258 for ln in lens), (R, off)
            assert sum(lens) <= max(0, r - 1)
            start = off + 1
            if start + r < (start // seg + 2) * seg:
                assert lens == expected_run_matches(r), (R, off, lens)
            if r >= 259:
                assert b.max_len == 258, (R, off, lens)
            if (R, off) in show:
                print(f"run {R} at {off}: BTYPE {b.btype}, match lengths {lens}")


def test_h5_runs_in_16x16_chunks(engine_lib):
    """(16, 16) chunks, 512 bytes: runs of 2 to 511 bytes at the offsets 0, 1, 15 and 16. Length
    258 occurs where R >= 259. (Segments were ceil(bytes / 256) rounded up to 16 bytes, 16 here,
    and a run is one thread's only as far as the next segment's head: the longest match of R = 259
    and of R = 511 was 30 or 31, the matches 30, 16, 16, ... Segments are now 272 bytes at least.)"""
    chunks, probes = run_tiles(engine_lib, (16, 16), OFFSETS, RUNS)
    for (raw, r), R_off in zip(chunks, [(R, off) for R in RUNS for off in OFFSETS]):
        assert r == min(R_off[0], 511 - R_off[1])
    check_runs(chunks, probes, RUNS, OFFSETS, MIN_SEG, show=[(31, 15), (258, 0), (259, 16), (261, 1), (511, 0), (511, 16)])


def test_h5_runs_across_a_short_chunk_s_segment_start(engine_lib):
    """(16, 16) chunks again: runs that end before, on and after the second thread's start (byte
    272), begin on it, and begin right after it."""
    runs, offsets = (2, 3, 4, 16, 33, 200), (240, 254, 267, 268, 269, 270, 271, 272)
    chunks, probes = run_tiles(engine_lib, (16, 16), offsets, runs)
    check_runs(chunks, probes, runs, offsets, MIN_SEG, show=[(33, 254), (200, 271)])


def test_h5_runs_of_258_and_more_in_long_segments(engine_lib):
    """(500, 70) chunks: 70,000 bytes in 288-byte segments, so one thread can hold a run of 258
    and more. Runs of 258, 259, 260, 261, 516 and 517 equal bytes after a differing one (the
    first is a literal, R - 1 are pending), one byte into a segment, across the next segment's
    start and deep in the chunk: 258 pending bytes become one match of 258, what is left goes on
    as a run of its own (a match, or one or two literals)."""
    runs, offsets, seg = (258, 259, 260, 261, 516, 517), (1, 288 - 40, 10 * 288 + 17), 288
    chunks, probes = run_tiles(engine_lib, (500, 70), offsets, runs, span=2)
    assert all(r == R for (_, r), R in zip(chunks, [R for R in runs for _ in offsets]))
    check_runs(chunks, probes, runs, offsets, seg, show=[(R, 1) for R in runs])


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (3, 5)])
@pytest.mark.parametrize("kind", ["low", "high", "zero"])
def test_h5_chunks_shorter_than_one_load(engine_lib, shape, kind):
    """Chunks of 2, 14 and 30 bytes (most threads own nothing): bytes below 144 (8 bits under
    the fixed code), bytes from 144 (9 bits) and zeros."""
    n = 2 * shape[0] * shape[1]
    raw = {"low": zigzag(n, 1, 100), "high": zigzag(n, 150, 100), "zero": bytes(n)}[kind]
    plane = plane_of_bytes(raw, *shape)
    tiles = coverage_tiles(engine_lib, plane, shape)
    (p,) = check_coverage_tiles(engine_lib, tiles, plane, shape)
    print(f"{shape} {kind}: BTYPE {p.btypes}, {len(tiles['coverage'][0])} bytes for {n}")
    if shape == (1, 1) or kind == "zero":
        assert p.btypes == [1]  # (a few tokens: no room for a dynamic header, shorter than stored)


def test_h5_alternating_bytes_and_saturation(engine_lib):
    """A (1000, 100) chunk of one value 0x0201: every byte differs from its neighbour, nothing is
    a run, two literals of one bit each. And the all-0xFFFF chunk from rows of 70,000 and
    4,294,967,295: one run."""
    shape = (1000, 100)
    plane = np.full(shape, 0x0201, np.uint32)
    sums = {}
    tiles = coverage_tiles(engine_lib, plane, shape, sums=sums)
    (p,) = check_coverage_tiles(engine_lib, tiles, plane, shape)
    (b,) = p.blocks
    assert b.btype == 2 and b.max_len == 0 and b.lit_hist[1] == b.lit_hist[2] == 100_000
    np.testing.assert_array_equal(sums["coverage"], np.full(1000, 100 * 0x0201))
    sat = np.full(shape, 70_000, np.uint32)
    sat[::2, ::3] = 4_294_967_295
    sums = {}
    tiles = coverage_tiles(engine_lib, sat, shape, sums=sums)
    (p,) = check_coverage_tiles(engine_lib, tiles, sat, shape)
    (b,) = p.blocks
    assert p.data == b"\xff" * 200_000 and b.btype == 2 and b.max_len == 258 and b.max_dist == 1
    np.testing.assert_array_equal(sums["coverage"], np.full(1000, 100 * 65535))
    print(f"0x0201 chunk: {len(tiles['coverage'][0])} bytes; saturated chunk: BTYPE {p.btypes}, "
          f"{sum(1 for t in b.tokens if isinstance(t, tuple))} matches")


def test_h5_rows_equal_the_run_path(engine_lib):
    """The streams of mgp_h5_tiles_rows on a run's fetched u32 result are the run path's own,
    byte for byte, sums included."""
    from mgatk2_amd.engine import EngineConfig
    from mgatk2_amd.synth import synth_reads

    nc = 20
    soa = synth_reads(777, 40_000, nc)
    cfg = EngineConfig(n_cells=nc, min_baseq=20, min_mapq=30, dedup_mode="alignment_and_fragment_length", min_reads=1)
    coc = np.concatenate([np.arange(nc)[::-1], [-1, 3, 3]])
    with engine_lib.Engine(cfg) as eng:
        eng.push(soa)
        eng.run()
        res = eng.fetch()
        run = {}
        for chunks in ((1000, 100), (700, 30)):
            s = {}
            run[chunks] = (eng.h5_tiles(coc, chunks, sums=s), s)
    for chunks, (tiles, s) in run.items():
        s2 = {}
        rows = engine_lib.h5_tiles_rows(res.counts, res.tn5, res.depth, coc, chunks, sums=s2)
        for name in engine_lib.H5_PLANES:
            assert len(rows[name]) == len(tiles[name])
            for i, (a, b) in enumerate(zip(rows[name], tiles[name])):
                assert a.tobytes() == b.tobytes(), (chunks, name, i)
        for k in ("coverage", "tn5_fwd", "tn5_rev"):
            np.testing.assert_array_equal(s2[k], s[k])
        sub = engine_lib.h5_tiles_rows(res.counts, res.tn5, res.depth, coc, (700, 5), col_chunks=(1, 3))
        full = engine_lib.h5_tiles_rows(res.counts, res.tn5, res.depth, coc, (700, 5))
    ncc = -(-coc.size // 5)
    for name in engine_lib.H5_PLANES:
        want = [full[name][r * ncc + c] for r in range(-(-16569 // 700)) for c in (1, 2)]
        assert [x.tobytes() for x in sub[name]] == [x.tobytes() for x in want]


def test_h5_rows_capacity_and_refusals(engine_lib):
    eng = engine_lib
    lib = eng.load_library()
    L, n = 40, 6
    rng = np.random.default_rng(1)
    depth = rng.integers(0, 50, (n, L)).astype(np.uint32)
    counts = np.zeros((n, L, 8), np.uint32)
    tn5 = np.zeros((n, L, 2), np.uint32)
    coc = np.arange(n, dtype=np.int32)

    def call(coc, crow, ccol, cap, dst):
        cb = np.zeros(11 * -(-L // crow) * -(-coc.size // ccol), np.int64)
        job = eng.mgp_h5_tiles(coc.size, coc.ctypes.data, crow, ccol, 0, -(-coc.size // ccol), cb.ctypes.data, None)
        tot = C.c_int64(-1)
        rc = lib.mgp_h5_tiles_rows(0, counts.ctypes.data, tn5.ctypes.data, depth.ctypes.data, n, L, C.byref(job),
                                   dst.ctypes.data, cap, C.byref(tot))
        return rc, tot.value, (lib.mgp_last_error() or b"").decode()

    dst = np.full(1 << 16, 0xA5, np.uint8)
    rc, total, _ = call(coc, 16, 4, dst.size, dst)
    assert rc == eng.MGP_OK and 0 < total < dst.size and np.all(dst[total:] == 0xA5)
    ok = dst[:total].copy()
    dst[:] = 0xA5
    rc, tot2, msg = call(coc, 16, 4, total - 1, dst)
    assert rc == eng.MGP_E_INVALID and tot2 == total and msg == "mgp_h5_tiles_rows: destination too small"
    assert np.all(dst == 0xA5)  # nothing written
    rc, tot2, _ = call(coc, 16, 4, total, dst)
    assert rc == eng.MGP_OK and tot2 == total and np.array_equal(dst[:total], ok) and np.all(dst[total:] == 0xA5)
    for bad in (n, -2):
        c2 = coc.copy()
        c2[3] = bad
        rc, _, msg = call(c2, 16, 4, dst.size, dst)
        assert rc == eng.MGP_E_INVALID and msg == "mgp_h5_tiles: cell of a column out of range"
    rc, _, msg = call(coc, 2049, 2048, dst.size, dst)  # chunk_rows * chunk_cols > 2^22
    assert rc == eng.MGP_E_INVALID and msg == "mgp_h5_tiles: bad arguments"
    with pytest.raises(eng.InvalidInputError, match="cell of a column out of range"):
        eng.h5_tiles_rows(counts, tn5, depth, [0, n], (16, 4))
    with pytest.raises(eng.InvalidInputError, match="mgp_h5_tiles: bad arguments"):
        eng.h5_tiles_rows(counts, tn5, depth, coc, (2049, 2048))


# ---------------------------------------------------------------------------
# cases through mgp_txt_gz_rows
# ---------------------------------------------------------------------------
def as_bytes(name) -> bytes:
    return bytes(name) if isinstance(name, (bytes, bytearray)) else name.encode()


def expected_text(counts, depth, cell: int, name, f: int) -> tuple[bytes, int]:
    """File f's lines of one cell, f"{p+1},{bc},{d}\\n" / f"{p+1},{bc},{fwd},{rev}\\n", and their number."""
    bc = as_bytes(name)
    out = []
    for p in np.flatnonzero(depth[cell]).tolist():
        if f == 0:
            out.append(b"%d,%s,%d\n" % (p + 1, bc, int(depth[cell, p])))
        else:
            a, b = int(counts[cell, p, 2 * f - 2]), int(counts[cell, p, 2 * f - 1])
            if a or b:
                out.append(b"%d,%s,%d,%d\n" % (p + 1, bc, a, b))
    return b"".join(out), len(out)


def check_txt(engine, counts, depth, cells, names, tmp_path=None) -> dict:
    """mgp_txt_gz_rows on the rows; every member decoded by the probe and compared with
    expected_text, every block held to the invariants. With tmp_path (str names only) the host
    formatter's files must hold the same text. Returns {(f, k): Probe}."""
    mem = engine.txt_gz_rows(counts, depth, cells, names)
    blob = mem.blob.tobytes()
    at = 0
    probes, text = {}, {f: [] for f in range(5)}
    for f in range(5):
        for k, (c, name) in enumerate(zip(cells, names)):
            want, n_lines = expected_text(counts, depth, c, name, f)
            nb = int(mem.member_bytes[f, k])
            assert int(mem.text_bytes[f, k]) == len(want)
            if not want:
                assert nb == 0
                continue
            p = dp.probe_gzip(blob[at:at + nb])
            at += nb
            assert p.data == want, (FILES[f], k)
            check_stream(p, literal_parse=n_lines == 1)  # (no earlier line to match: literals)
            probes[(f, k)] = p
            text[f].append(want)
    assert at == len(blob)
    if tmp_path is not None:
        from mgatk2_amd.bam import txt_write_cells

        txt_write_cells(tmp_path / "host", counts, depth, cells, list(names), level=1, append=False)
        for f in range(5):
            assert gzip.decompress((tmp_path / f"host.{FILES[f]}.txt.gz").read_bytes()) == b"".join(text[f])
    return probes


def test_txt_each_block_kind(engine_lib, tmp_path):
    """Fixed: one-line members with a short barcode (also one of bytes >= 144, the fixed code's
    9-bit literals). Stored: a one-line member whose 4,096-byte barcode holds all 256 byte values
    at random. Dynamic: a member of a few hundred lines. A one-line member has no earlier line to
    match, so its parse is literals."""
    rng = np.random.default_rng(256)
    L, n = 600, 4
    counts = np.zeros((n, L, 8), np.uint32)
    depth = np.zeros((n, L), np.uint32)
    depth[0, 77] = 3
    counts[0, 77, 4] = 3
    depth[1, 599] = 12
    counts[1, 599, 7] = 12
    depth[2, 0] = 5
    counts[2, 0, 0] = 5
    depth[3, 100:500] = rng.integers(1, 40, 400)
    counts[3, 100:500, 2] = depth[3, 100:500]
    wild = rng.integers(0, 256, 4096).astype(np.uint8)
    wild[rng.permutation(4096)[:256]] = np.arange(256)
    names = ["AC-1", bytes([0xFF, 0xFE, 0x90, 0xC8, 0xFF]), wild.tobytes(), "ACGTACGTACGTACGT-1"]
    assert set(names[2]) == set(range(256))
    probes = check_txt(engine_lib, counts, depth, [0, 1, 2, 3], names)
    kinds = {k: p.btypes for k, p in probes.items()}
    print("block kinds by (file, cell):", kinds)
    assert kinds[(0, 0)] == [1] and kinds[(3, 0)] == [1]
    assert kinds[(0, 1)] == [1] and kinds[(4, 1)] == [1]
    assert kinds[(0, 2)] == [0] and kinds[(1, 2)] == [0]
    assert [b.stored_len for b in probes[(0, 2)].blocks] == [len(b"1,") + 4096 + len(b",5\n")]
    assert kinds[(0, 3)] == [2] and kinds[(2, 3)] == [2]
    # the str-named cells against the host formatter too
    check_txt(engine_lib, counts, depth, [3, 0], [names[3], names[0]], tmp_path)


BIG = (99_999_999, 100_000_000, 100_000_001, 999_999_999, 1_000_000_000, 4_294_967_295)


def test_txt_ten_digit_numbers(engine_lib, tmp_path):
    """Counts and depths of 8, 9 and 10 digits (TextOut::num's split at 10^8) in every field, next
    to one-digit values, under barcodes of 0, 1, 7, 8, 9, 15, 16 and 17 bytes (the staging block's
    alignments)."""
    rng = np.random.default_rng(10)
    names = ["ACGTACGTACGTACGTA"[:k] for k in (0, 1, 7, 8, 9, 15, 16, 17)]
    n, L = len(names), 300
    pick = np.array(BIG + (1, 2, 5, 9, 0, 7), np.uint32)
    counts = pick[rng.integers(0, pick.size, (n, L, 8))]
    depth = pick[rng.integers(0, pick.size, (n, L))]
    depth[:, ::17] = 0
    for c in range(n):  # every big value in every field of every cell, next to one-digit lines
        for j, v in enumerate(BIG):
            assert (depth[c] == v).any()
            for q in range(8):
                assert ((counts[c, :, q] == v) & (depth[c] > 0)).any(), (c, q, v)
    probes = check_txt(engine_lib, counts, depth, list(range(n)), names, tmp_path)
    for k in range(n):
        for v in BIG:
            assert b",%d\n" % v in probes[(0, k)].data
            assert b",%d," % v in probes[(1, k)].data and b",%d\n" % v in probes[(4, k)].data
    print("ten-digit members:", sorted({tuple(p.btypes) for p in probes.values()}))


@pytest.mark.parametrize("L", [1, 255, 256, 257, 16569])
def test_txt_empty_barcode_with_lines(engine_lib, tmp_path, L):
    """The empty barcode on every position: "p,,d" (the second comma right after the first), the
    shortest lines there are; 16,569 of them pass the match finder's 1,024-line windows."""
    rng = np.random.default_rng(L)
    depth = rng.integers(1, 10, (2, L)).astype(np.uint32)
    counts = np.zeros((2, L, 8), np.uint32)
    counts[:, :, 0] = depth
    counts[1, :, 0] = 0
    counts[1, ::2, 7] = 3
    probes = check_txt(engine_lib, counts, depth, [1, 0], ["", ""], tmp_path)
    p = probes[(0, 0)]
    assert p.data.count(b"\n") == L and p.data.count(b",,") == L
    assert (4, 1) not in probes and p.data.startswith(b"1,,")
    if L == 16569:
        assert p.btypes == [2] and p.blocks[0].max_len >= 3
        print(f"empty barcode, {L} lines: {len(p.data)} bytes, longest match {p.blocks[0].max_len}, "
              f"largest distance {p.blocks[0].max_dist}")


def test_txt_far_matches(engine_lib, tmp_path):
    """Distance codes 28 and 29 (13 extra bits: a match more than 16,384 bytes back). Nine lines
    at positions 100..108 under a 4,089-byte barcode; lines 0..4 carry nine-digit depths (4,104
    bytes each), lines 0 and 4 the same one and lines 1..3 rotations of it that differ from it
    in every digit. The match finder's first window holds the lines 0..4 (24 KB), so line 4 sees
    line 0 at 4 x 4,104 = 16,416 bytes, and only there do its digits match. (With one-digit depths
    a line is 4,096 bytes and four lines back is 16,384, still code 27: the nine digits both make
    the match worth its 13 extra bits and push it past 16,384.)"""
    rng = np.random.default_rng(28)
    name = "".join(rng.choice(list("ACGT"), 4089))
    L = 300
    depth = np.zeros((1, L), np.uint32)
    d0 = "123456789"
    rot = [int(d0[k:] + d0[:k]) for k in (1, 2, 3)]
    depth[0, 99:108] = [int(d0), *rot, int(d0), 7, 1, 9, 4]
    for r in rot:
        assert all(a != b for a, b in zip(str(r), d0))
    counts = np.zeros((1, L, 8), np.uint32)
    probes = check_txt(engine_lib, counts, depth, [0], [name], tmp_path)
    (p,) = probes.values()
    (b,) = p.blocks
    far = [(ln, d) for ln, d in (t for t in b.tokens if isinstance(t, tuple)) if d > 16384]
    print(f"far matches: BTYPE {b.btype}, largest distance {b.max_dist}, distance symbols 28/29 used "
          f"{b.dist_hist[28]}/{b.dist_hist[29]}, far tokens {far}")
    assert b.btype == 2 and 16384 < b.max_dist <= 32768
    assert b.dist_hist[28] >= 1 and any(ln >= 9 for ln, _ in far) and all(d == 16416 for _, d in far)


def test_txt_refusals(engine_lib):
    eng = engine_lib
    depth = np.ones((2, 10), np.uint32)
    counts = np.ones((2, 10, 8), np.uint32)
    with pytest.raises(eng.InvalidInputError, match=r"mgp_txt_gz: barcode names of 0\.\.4096 bytes"):
        eng.txt_gz_rows(counts, depth, [0], ["A" * 4097])
    with pytest.raises(eng.InvalidInputError, match=r"mgp_txt_gz: barcode names of 0\.\.4096 bytes"):
        eng.txt_gz_rows(counts, depth, [0], [bytes(4097)])
    for bad in (2, -1):
        with pytest.raises(eng.InvalidInputError, match="mgp_txt_gz: cell out of range"):
            eng.txt_gz_rows(counts, depth, [0, bad], ["A", "C"])
    assert eng.txt_gz_rows(counts, depth, [1], [bytes(4096)]).member_bytes[0, 0] > 0
