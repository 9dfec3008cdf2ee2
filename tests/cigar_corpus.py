"""Seeded random reads aimed at the pileup's CIGAR paths (k_pileup, mgp_engine.hip),
their classification, and the pieces the CPU and GPU tests of them share.

A wave piles 64 reads of one cell and one window, so each stratum below goes to a cell
of its own (corpus A): a cell's waves are then made of one kind of read, which is what
steers the wave-uniform branches of pile_bases / pile_bases_packed / pile_bases_p32.
Most reads start near a window edge, so the window clamp of either block, the halo and
the Tn5 cut of a reverse read (start + l_seq - 1) fall on both sides of it.

Strata (STRATA; `classify(read).stratum` restates the rule, with no engine import):
  plain      one M of 50 bases, qualities <= 62
  one_block  one aligned block after the extension merge (M/=/X with S, H, I, P around
             it; M I M and M P M, which extend: pileup.py Q1), <= 4 ops, l_seq 1-50
  two_near   two blocks (split by D, N, S, or I/P beside a D), <= 4 ops, D/N <= 12
  two_far    two blocks with a D/N of 13..4095
  full_fast  register path of the full layout only: <= 4 ops, <= 2 blocks, but l_seq
             51-64, a quality of 63-255, or more than two aligned ops
  slow       l_seq 65-150 (`long`), 5-7 ops with <= 2 blocks (`many_ops`), >= 3 blocks
             (`blocks3`), or a D/N >= 4096 (`gap4096`: it fits no packed layout; with
             <= 4 ops the kernel still piles it from registers, `path` says so)
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MITO_LEN = 16569
WIN_TARGET = 1280  # MGP_WIN of mgp_engine.hip
STRATA = ("plain", "one_block", "two_near", "two_far", "full_fast", "slow")
PACKED_STRATA = STRATA[:4]
SLOW_KINDS = ("long", "many_ops", "blocks3", "gap4096")
# (min_baseq, min_distance_from_end); min_dist -1 acts as 0, 30 has no 32-byte layout
PAIRS = ((20, 5), (0, 0), (30, 2), (-128, 0), (127, 15), (0, 15), (0, -1), (10, 30))
PAIRS32 = tuple(p for p in PAIRS if p[1] <= 15)
MIN_MAPQ = 20
EDGE_OFFSETS = {"plain": (-60, 12), "one_block": (-60, 12), "two_near": (-60, 12), "two_far": (-160, 12),
                "full_fast": (-160, 12), "slow": (-160, 12)}

M, I, D, N, S, H, P, EQ, X = 0, 1, 2, 3, 4, 5, 6, 7, 8
ALIGNED = (M, EQ, X)
QUERY_OPS = (M, I, S, EQ, X)
CIGAR_CHARS = "MIDNSHP=X"


def window_geometry(mito_len: int = MITO_LEN) -> tuple[int, int]:
    """(windows, width) as configure_geometry (mgp_engine.hip) derives them."""
    nwin = (mito_len + WIN_TARGET - 1) // WIN_TARGET
    w = (mito_len + nwin - 1) // nwin
    w = (w + 7) // 8 * 8
    return (mito_len + w - 1) // w, w


def cigar_string(cig) -> str:
    return "".join(f"{ln}{CIGAR_CHARS[op]}" for op, ln in cig)


# ---------------------------------------------------------------------------
# classification
# ---------------------------------------------------------------------------
def aligned_blocks(cig) -> list[tuple[int, int, int]]:
    """(query start, query end, reference start) of the aligned blocks as the reference
    walks the CIGAR (pileup.py:55-95: I, H, P move nothing), an aligned op that starts
    where the last block ended in both query and reference extending it (the comment
    above pile_line)."""
    out: list[list[int]] = []
    q = ref = 0
    for op, ln in cig:
        if op in ALIGNED:
            if out and out[-1][1] == q and out[-1][2] - out[-1][0] == ref - q:
                out[-1][1] = q + ln
            else:
                out.append([q, q + ln, ref])
            q += ln
            ref += ln
        elif op in (D, N):
            ref += ln
        elif op == S:
            q += ln
    return [tuple(b) for b in out]


@dataclass(frozen=True)
class ReadClass:
    stratum: str
    kind: str          # the slow stratum's kind, "" elsewhere
    path: str          # "regs" (pile_bases*) or "slow" (pile_slow) for a full-layout record
    n_blocks: int
    n_aligned_ops: int
    fits64: bool       # the 64-byte layout takes it (mgp_pack_record)
    fits32: bool       # the 32-byte layout takes it at some pair (mgp_pack32_record)

    def __str__(self):
        return f"{self.stratum}{'/' + self.kind if self.kind else ''}:{self.path}:{self.n_blocks}blk"


def classify(read: dict) -> ReadClass:
    cig = read["cigartuples"]
    lseq = len(read["query_sequence"])
    start = read["reference_start"]
    blocks = aligned_blocks(cig)
    nb, ncig = len(blocks), len(cig)
    n_al = sum(1 for op, _ in cig if op in ALIGNED)
    gap = max([ln for op, ln in cig if op in (D, N)], default=0)
    regs = lseq <= 64 and ncig <= 4 and nb <= 2 and -(1 << 28) <= start < (1 << 28)
    layout_ok = 1 <= lseq <= 50 and ncig <= 4 and n_al <= 2 and all(ln < 4096 for _, ln in cig)
    fits64 = layout_ok and max(read["query_qualities"]) <= 62 and -(1 << 28) <= start < (1 << 28)
    fits32 = layout_ok and 0 <= start < 65536
    kind = ""
    if lseq > 64:
        stratum, kind = "slow", "long"
    elif nb >= 3:
        stratum, kind = "slow", "blocks3"
    elif ncig > 4:
        stratum, kind = "slow", "many_ops"
    elif gap >= 4096:
        stratum, kind = "slow", "gap4096"
    elif not fits64:
        stratum = "full_fast"
    elif nb == 2:
        stratum = "two_far" if gap > 12 else "two_near"
    elif cig == [(M, 50)]:
        stratum = "plain"
    else:
        stratum = "one_block"
    return ReadClass(stratum, kind, "regs" if regs else "slow", nb, n_al, fits64, fits32)


def block_windows(read: dict, w: int) -> list[tuple[int, int]]:
    """(window of the first base, window of the last base) of every block."""
    s = read["reference_start"]
    return [((s + r) // w, (s + r + qe - qs - 1) // w) for qs, qe, r in aligned_blocks(read["cigartuples"])]


def cut_position(read: dict) -> int:
    return read["reference_start"] + (len(read["query_sequence"]) - 1 if read["flag"] & 0x10 else 0)


def last_aligned_position(read: dict) -> int:
    b = aligned_blocks(read["cigartuples"])
    return read["reference_start"] + max(r + qe - qs - 1 for qs, qe, r in b) if b else -1


# ---------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------
def _split(rng, total: int, parts: int) -> list[int]:
    """`parts` positive integers summing to `total`."""
    cuts = np.sort(rng.choice(np.arange(1, total), parts - 1, replace=False)) if parts > 1 else np.zeros(0, int)
    edges = [0, *[int(c) for c in cuts], total]
    return [edges[k + 1] - edges[k] for k in range(parts)]


def _fill(rng, ops: list[int], lseq: int, gap_hi: int = 12, gap_lo: int = 1) -> list[tuple[int, int]]:
    """Lengths for a template of ops: the query-consuming ones sum to lseq."""
    nq = sum(1 for op in ops if op in QUERY_OPS)
    ql = iter(_split(rng, lseq, nq))
    return [(op, next(ql)) if op in QUERY_OPS else
            (op, int(rng.integers(gap_lo, gap_hi + 1)) if op in (D, N) else int(rng.integers(1, 20))) for op in ops]


def _al(rng) -> int:
    return int(rng.choice([M, M, M, M, EQ, X]))


_ONE_BLOCK = ["A", "SA", "AS", "SAS", "HA", "AH", "HSA", "ASH", "HSAS", "IA", "AI", "SAI", "IAS", "PA", "AP", "SAP",
              "AIA", "AIA", "AIA", "SAIA", "AIAS", "APA", "HAIA"]
_TWO = ["ADA", "ANA", "ASA", "AIDA", "ADIA", "APDA", "ANPA", "SADA", "ANAS", "HADA", "ADAH", "ASAS", "SASA", "ADAI",
        "IANA"]
_TWO_GAP = [t for t in _TWO if "D" in t or "N" in t]
_FULL_FAST = _ONE_BLOCK + _TWO + ["AAA", "AAIA", "ADAA"]
_MANY_OPS = ["HSAIASH", "SADAS", "HSANAS", "SAIAS", "HSASH", "AIAIA", "SAPADAS", "HSADASH", "AIDAS"]
_BLOCKS3 = ["ADADA", "ANASA", "ASADA", "ADANADA", "SADANA", "ADASAH", "ASASA"]
_OPS = {"A": None, "S": S, "H": H, "I": I, "P": P, "D": D, "N": N}


def _template(rng, t: str) -> list[int]:
    return [_al(rng) if ch == "A" else _OPS[ch] for ch in t]


def _cigar(rng, stratum: str) -> tuple[list[tuple[int, int]], int, str]:
    """(cigar, l_seq, quality kind) of one read of a stratum."""
    pick = lambda ts: _template(rng, ts[int(rng.integers(len(ts)))])  # noqa: E731
    if stratum == "plain":
        return [(M, 50)], 50, "low"
    if stratum == "one_block":
        ops = pick(_ONE_BLOCK)
        lseq = int(rng.integers(max(1, sum(op in QUERY_OPS for op in ops)), 51))
        return _fill(rng, ops, lseq), lseq, "low"
    if stratum in ("two_near", "two_far"):
        far = stratum == "two_far"
        ops = pick(_TWO_GAP if far else _TWO)
        lseq = int(rng.integers(max(2, sum(op in QUERY_OPS for op in ops)), 51))
        if not far:
            return _fill(rng, ops, lseq), lseq, "low"
        hi = 3000 if rng.random() < 0.06 else 150
        return _fill(rng, ops, lseq, gap_hi=hi, gap_lo=13), lseq, "low"
    if stratum == "full_fast":
        ops = pick(_FULL_FAST)
        if rng.random() < 0.5:
            lseq, qk = int(rng.integers(51, 65)), "low"
        else:
            lseq, qk = int(rng.integers(max(3, sum(op in QUERY_OPS for op in ops)), 65)), "high"
        return _fill(rng, ops, lseq, gap_hi=12 if rng.random() < 0.8 else 400), lseq, qk
    kind = SLOW_KINDS[int(rng.integers(4))]
    qk = "any"
    if kind == "long":
        ops = pick(_ONE_BLOCK + _TWO + _MANY_OPS + _BLOCKS3)
        lseq = int(rng.integers(65, 151))
        return _fill(rng, ops, lseq, gap_hi=12 if rng.random() < 0.8 else 2000), lseq, qk
    if kind == "many_ops":
        ops = pick(_MANY_OPS)
    elif kind == "blocks3":
        ops = pick(_BLOCKS3)
    else:
        ops = pick(["ANA", "ADA", "SANA", "ANAS"])
    lseq = int(rng.integers(max(3, sum(op in QUERY_OPS for op in ops)), 65 if rng.random() < 0.3 else 51))
    if kind == "gap4096":
        return _fill(rng, ops, lseq, gap_hi=9000, gap_lo=4096), lseq, qk
    return _fill(rng, ops, lseq, gap_hi=12 if rng.random() < 0.8 else 1500), lseq, qk


def _late_cut(rng, stratum: str) -> tuple[list[tuple[int, int]], int, int]:
    """A reverse read whose aligned bases end before a window edge and whose Tn5 cut
    (start + l_seq - 1) lies past it: >= 20 soft-clipped or inserted bases after at
    most 20 aligned ones. Returns (cigar, l_seq, bases from the start to the edge)."""
    lseq = int(rng.integers(25, 51)) if stratum == "one_block" else int(rng.integers(65, 151))
    a = int(rng.integers(1, min(20, lseq - 20) + 1))
    r = int(rng.integers(a, 21))
    tail = S if rng.random() < 0.6 else I
    return [(_al(rng), a), (tail, lseq - a)], lseq, r


def _qualities(rng, lseq: int, kind: str) -> list[int]:
    if kind == "low":
        top = 63
    elif kind == "high":
        top = 256
    else:
        top = 256 if rng.random() < 0.3 else 63
    q = rng.integers(0, top, lseq)
    if kind == "high" and q.max() <= 62:
        q[int(rng.integers(lseq))] = int(rng.integers(63, 256))
    return [int(x) for x in q]


def _start(rng, stratum: str, mito_len: int, w: int, max_start: int) -> int:
    nwin = (mito_len + w - 1) // w
    u = rng.random()
    if u < 0.6 and nwin > 1:
        lo, hi = EDGE_OFFSETS[stratum]
        s = int(rng.integers(1, nwin)) * w + int(rng.integers(lo, hi + 1))
    elif u < 0.7:
        s = int(rng.integers(0, 20))
    elif u < 0.85:
        s = int(rng.integers(mito_len - 160, mito_len + 6))
    else:
        s = int(rng.integers(0, mito_len))
    return min(max(s, 0), max_start)


def stratum_reads(rng, stratum: str, n: int, mito_len: int = MITO_LEN, bc: int = 0, clean: bool = False,
                  start_range: tuple[int, int] | None = None) -> list[dict]:
    """n reads of one stratum (unsorted). clean: paired flags only and starts below
    mito_len (corpus P). start_range: every start uniform in [lo, hi] instead."""
    _, w = window_geometry(mito_len)
    nwin = (mito_len + w - 1) // w
    max_start = mito_len - 1 if clean else mito_len + 5
    out = []
    for _ in range(n):
        flag = int(rng.choice([0x1, 0x11] if clean else [0x0, 0x1, 0x10, 0x11]))
        start = None
        if stratum in ("one_block", "slow") and nwin > 1 and start_range is None and rng.random() < 0.16:
            cig, lseq, r = _late_cut(rng, stratum)
            qk = "low" if stratum == "one_block" else "any"
            flag |= 0x10
            start = int(rng.integers(1, nwin)) * w - r
        else:
            cig, lseq, qk = _cigar(rng, stratum)
            if stratum == "one_block" and cig == [(M, 50)]:
                cig = [(EQ, 50)]  # one M of 50 is the plain stratum
        if start_range is not None:
            start = int(rng.integers(start_range[0], start_range[1] + 1))
        elif start is None:
            start = _start(rng, stratum, mito_len, w, max_start)
            if stratum == "two_near" and nwin > 1 and rng.random() < 0.15:
                # the edge inside the gap between the blocks (or right at the block boundary)
                b = aligned_blocks(cig)
                start = int(rng.integers(1, nwin)) * w - int(rng.integers(b[0][2] + b[0][1] - b[0][0], b[1][2] + 1))
        seq = "".join(rng.choice(list("ACGTACGTACGTACGTNRY"), lseq))
        if not clean:
            u = rng.random()
            flag |= 0x4 if u < 0.01 else 0x100 if u < 0.02 else 0x800 if u < 0.03 else 0
        out.append(dict(reference_start=max(start, 0), cigartuples=cig, query_sequence=seq,
                        query_qualities=_qualities(rng, lseq, qk), flag=flag,
                        mapping_quality=int(rng.choice([60, 60, 60, 60, 60, 60, 20, 20, 0])),
                        template_length=int(rng.choice([-1, 1])) * int(rng.integers(100, 104)),
                        bc=-1 if rng.random() < 0.03 else bc, stratum=stratum))
    return out


def _sorted(reads: list[dict]) -> list[dict]:
    return sorted(reads, key=lambda r: r["reference_start"])


def corpus_a(per_stratum: int = 3500, seed: int = 20251) -> list[dict]:
    """The six strata in six cells (cell k = STRATA[k]), sorted by start."""
    rng = np.random.default_rng(seed)
    return _sorted([r for k, s in enumerate(STRATA) for r in stratum_reads(rng, s, per_stratum, bc=k)])


def corpus_b_cells(n: int, seed: int = 20252) -> np.ndarray:
    """Corpus B is corpus A's reads (and so its records) shuffled into two cells: the
    cell of read i; -1 where corpus A has none."""
    return np.random.default_rng(seed).integers(0, 2, n).astype(np.int32)


def corpus_p(per_stratum: int = 3500, seed: int = 20253) -> list[dict]:
    """The four strata that pack, in four cells; paired flags and starts < mito_len."""
    rng = np.random.default_rng(seed)
    return _sorted([r for k, s in enumerate(PACKED_STRATA) for r in stratum_reads(rng, s, per_stratum, bc=k,
                                                                                  clean=True)])


ONE_WINDOW_LEN = 1000
ONE_WINDOW_STRATA = ("one_block", "two_near", "slow")


def corpus_one_window(per_stratum: int = 1200, seed: int = 20254) -> list[dict]:
    """mito_len 1000 is a single window: reads starting in [880, 1005], three cells."""
    rng = np.random.default_rng(seed)
    return _sorted([r for k, s in enumerate(ONE_WINDOW_STRATA)
                    for r in stratum_reads(rng, s, per_stratum, mito_len=ONE_WINDOW_LEN, bc=k,
                                           start_range=(880, 1005))])


# ---------------------------------------------------------------------------
# packing: pack_reads' records, built with the vectorised layout functions
# ---------------------------------------------------------------------------
def pack_corpus(reads: list[dict], layout: str, pair: tuple[int, int] | None = None, full=None):
    """pack_reads(reads, pack=False) for layout "full", pack_reads(reads) for "p64",
    pack_reads(reads, pack32=q, pack32_dist=d) for "p32" with pair (q, d): the same
    flags, offsets and payload bytes (test_cigar_corpus checks that), from one call of
    the layout functions per corpus instead of one per read. full: the corpus packed as
    "full" already."""
    from mgatk2_amd.synth import (_NT16_IDX, FLAG_PACK32, FLAG_PACKED, PACK32_BYTES, PACK_BYTES, ReadSoA, pack32_bytes,
                                  pack32_mask, pack_bytes, pack_reads, packable_mask)

    if full is None:
        full = pack_reads(reads, pack=False)
    if layout == "full":
        return full
    n = len(reads)
    lseq = np.array([len(r["query_sequence"]) for r in reads], np.int64)
    ncig = np.array([len(r["cigartuples"]) for r in reads], np.int64)
    cig = np.zeros((n, 8), np.int64)
    qual = np.zeros((n, 50), np.int64)
    code = np.zeros((n, 50), np.int64)
    for i, r in enumerate(reads):
        cig[i, : ncig[i]] = [(ln << 4) | op for op, ln in r["cigartuples"]]
        k = min(int(lseq[i]), 50)
        qual[i, :k] = r["query_qualities"][:k]
        code[i, :k] = [_NT16_IDX[ch] for ch in r["query_sequence"][:k]]
    rev = (full.flag & 0x10) != 0
    fit64 = packable_mask(full.start, full.flag, lseq, ncig, cig, qual)
    fit32 = np.zeros(n, bool)
    if layout == "p32":
        fit32 = pack32_mask(full.start, full.flag, lseq, ncig, cig, pair[0], pair[1])
        fit64 &= ~fit32
    fsize = np.diff(np.append(full.rec_off.astype(np.int64), full.payload.shape[0]))
    size = np.where(fit32, PACK32_BYTES, np.where(fit64, PACK_BYTES, fsize))
    off = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)
    payload = np.zeros(int(size.sum()), np.uint8)
    for fit, nbytes, recs in ((fit32, PACK32_BYTES, None), (fit64, PACK_BYTES, None)):
        idx = np.flatnonzero(fit)
        if not idx.size:
            continue
        if nbytes == PACK32_BYTES:
            recs = pack32_bytes(full.start[idx], lseq[idx], rev[idx], ncig[idx], cig[idx], qual[idx], code[idx],
                                pair[0], pair[1])
        else:
            recs = pack_bytes(full.start[idx], lseq[idx], rev[idx], ncig[idx], cig[idx], qual[idx], code[idx])
        payload[off[idx, None] + np.arange(nbytes)[None, :]] = recs
    fo = full.rec_off.astype(np.int64)
    for i in np.flatnonzero(~fit32 & ~fit64):
        payload[off[i] : off[i] + fsize[i]] = full.payload[fo[i] : fo[i] + fsize[i]]
    flag = (full.flag | np.where(fit32, FLAG_PACK32, np.where(fit64, FLAG_PACKED, 0))).astype(np.uint16)
    return ReadSoA(full.start.copy(), full.bc.copy(), full.tlen.copy(), flag, full.mapq.copy(), full.span.copy(),
                   off.astype(np.uint64), payload)


def with_cells(soa, bc: np.ndarray):
    """The same records under other cells (a read without a cell keeps none)."""
    from mgatk2_amd.synth import ReadSoA

    return ReadSoA(soa.start, np.where(soa.bc < 0, soa.bc, bc).astype(np.int32), soa.tlen, soa.flag, soa.mapq,
                   soa.span, soa.rec_off, soa.payload)


def layout_name(flag: int) -> str:
    return "p32" if flag & 0x4000 else "p64" if flag & 0x2000 else "full"


# ---------------------------------------------------------------------------
# comparison with a useful failure message
# ---------------------------------------------------------------------------
ARRAYS = ("counts", "tn5", "depth", "n_reads", "any_paired", "passed", "covered", "depth_sum", "depth_max",
          "median_lo", "median_hi", "ref_tally")
STATS = ("total_reads", "filtered_reads", "n_barcodes", "duplicate_reads_with_length",
         "duplicate_reads_position_only", "cells_passed")
_COLS = {"counts": ("A+", "A-", "C+", "C-", "G+", "G-", "T+", "T-"), "tn5": ("cut+", "cut-"), "depth": ("depth",)}


def describe_mismatch(got, exp, soa, reads, cells=None) -> str | None:
    """None when `got` equals `exp` on every array and statistic the GPU tests compare;
    else the first differing (cell, position, column) and the reads of that cell whose
    reference span or Tn5 cut covers the position. reads: the dicts behind soa, in its
    order. cells: names of the cells (corpus A: the strata)."""
    for k in ("counts", "tn5", "depth"):
        x, y = getattr(got, k), getattr(exp, k)
        if np.array_equal(x, y):
            continue
        x3, y3 = x.reshape(x.shape[0], x.shape[1], -1), y.reshape(y.shape[0], y.shape[1], -1)
        c, p, col = (int(v) for v in np.argwhere(x3 != y3)[0])
        name = f" ({cells[c]})" if cells and c < len(cells) else ""
        lines = [f"{k}: first difference at cell {c}{name}, position {p}, column {_COLS[k][col]}: "
                 f"engine {int(x3[c, p, col])}, oracle {int(y3[c, p, col])}; "
                 f"{int((x3 != y3).sum())} entries differ. Reads of the cell over the position:"]
        assert len(reads) == soa.n and all(r["reference_start"] == s for r, s in zip(reads, soa.start.tolist()))
        for i, r in enumerate(reads):
            if int(soa.bc[i]) != c:
                continue
            s = r["reference_start"]
            if s <= p < s + max(int(soa.span[i]), 1) or cut_position(r) == p:
                lines.append(f"  read {i}: {cigar_string(r['cigartuples'])} start {s} l_seq {len(r['query_sequence'])} "
                             f"flag {int(soa.flag[i]) & 0xFFF:#x} mapq {r['mapping_quality']} "
                             f"layout {layout_name(int(soa.flag[i]))} {classify(r)}")
                if len(lines) > 40:
                    lines.append("  ...")
                    break
        return "\n".join(lines)
    for k in ARRAYS:
        if not np.array_equal(getattr(got, k), getattr(exp, k)):
            bad = np.argwhere(np.asarray(getattr(got, k) != getattr(exp, k)))[0].tolist()
            return f"{k} differs first at {bad}"
    if not np.array_equal(got.cell_order(), exp.cell_order()):
        return "cell order differs"
    for k in STATS:
        if got.stats[k] != exp.stats[k]:
            return f"stats[{k}]: engine {got.stats[k]}, oracle {exp.stats[k]}"
    return None
