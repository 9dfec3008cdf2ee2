"""The CIGAR-path corpus (tests/cigar_corpus.py) on CPU: every read classifies as the
stratum it was made for, the strata hold the shapes they aim at, the oracle gives the
same result for the full, 64-byte and 32-byte records of the same reads at every
threshold pair, and the oracle's counts equal a few lines of Python written from
pileup.py:55-95. The GPU side is tests/test_gpu_cigar_paths.py."""

from __future__ import annotations

import functools
from collections import Counter

import numpy as np
import pytest

import cigar_corpus as cc


@functools.lru_cache(maxsize=None)
def _corpus(name):
    return {"A": cc.corpus_a, "P": cc.corpus_p, "W": cc.corpus_one_window}[name]()


@functools.lru_cache(maxsize=None)
def _packed(name, layout, pair=None):
    full = None if layout == "full" else _packed(name, "full")
    return cc.pack_corpus(_corpus(name), layout, pair, full=full)


def _cfg(pair, n_cells, dedup="none", mito_len=cc.MITO_LEN):
    from mgatk2_amd.engine import EngineConfig

    return EngineConfig(n_cells=n_cells, min_baseq=pair[0], min_mapq=cc.MIN_MAPQ, min_distance_from_end=pair[1],
                        dedup_mode=dedup, min_reads=1, mito_len=mito_len)


def test_window_geometry():
    assert cc.window_geometry() == (13, 1280)
    assert cc.window_geometry(cc.ONE_WINDOW_LEN) == (1, 1000)


@pytest.mark.parametrize("name", ["A", "P", "W"])
def test_every_read_classifies_as_its_stratum(name):
    reads = _corpus(name)
    made = Counter(r["stratum"] for r in reads)
    ok = Counter(r["stratum"] for r in reads if cc.classify(r).stratum == r["stratum"])
    assert ok == made, {s: (ok[s], made[s]) for s in made}
    assert set(made) == set({"A": cc.STRATA, "P": cc.PACKED_STRATA, "W": cc.ONE_WINDOW_STRATA}[name])
    assert all(r["reference_start"] >= 0 for r in reads)
    assert all(reads[i]["reference_start"] <= reads[i + 1]["reference_start"] for i in range(len(reads) - 1))
    for r in reads:  # as pysam guarantees
        assert sum(ln for op, ln in r["cigartuples"] if op in cc.QUERY_OPS) == len(r["query_sequence"])
        assert len(r["query_qualities"]) == len(r["query_sequence"])
    # the register path of the full layout and pile_slow are both present where full records are
    if name != "P":
        assert {cc.classify(r).path for r in reads if r["stratum"] == "slow"} == {"regs", "slow"}


def test_strata_hold_the_shapes_they_aim_at():
    reads = _corpus("A")
    _, w = cc.window_geometry()
    by = {s: [r for r in reads if r["stratum"] == s] for s in cc.STRATA}
    assert all(len(v) == 3500 for v in by.values())
    split = [r for r in by["two_near"] if (lambda b: b[0][1] != b[1][0])(cc.block_windows(r, w))]
    assert len(split) >= 200, len(split)
    mim = [r for r in by["one_block"]
           if any(a[0] in cc.ALIGNED and b[0] == cc.I and c[0] in cc.ALIGNED
                  for a, b, c in zip(r["cigartuples"], r["cigartuples"][1:], r["cigartuples"][2:]))]
    assert len(mim) >= 200 and all(cc.classify(r).n_blocks == 1 for r in mim), len(mim)
    kinds = Counter(cc.classify(r).kind for r in by["slow"])
    assert set(kinds) == set(cc.SLOW_KINDS) and min(kinds.values()) >= 300, kinds
    late = [r for r in reads if r["flag"] & 0x10 and cc.cut_position(r) // w > cc.last_aligned_position(r) // w >= 0]
    assert len(late) >= 100, len(late)
    assert {r["stratum"] for r in late} >= {"one_block", "slow"}
    # lengths on both sides of the limits, the sprinkles, every op
    assert {len(r["query_sequence"]) for r in by["full_fast"]} >= {51, 64}
    assert any(max(r["query_qualities"]) >= 128 for r in by["full_fast"])
    assert {len(r["query_sequence"]) for r in by["one_block"]} >= {1, 2, 9, 10, 50}
    assert any(ln > 1280 for r in by["two_far"] for op, ln in r["cigartuples"] if op in (cc.D, cc.N))
    assert all(ln < 4096 for r in by["two_far"] for op, ln in r["cigartuples"])
    assert {op for r in reads for op, _ in r["cigartuples"]} == set(range(9))
    assert {r["flag"] & 0x11 for r in reads} == {0x0, 0x1, 0x10, 0x11}
    assert all(any(r["flag"] & f for r in reads) for f in (0x4, 0x100, 0x800))
    assert any(r["bc"] < 0 for r in reads) and {r["mapping_quality"] for r in reads} == {0, 20, 60}
    assert any(r["reference_start"] >= cc.MITO_LEN for r in reads) and any(r["reference_start"] == 0 for r in reads)


def test_corpus_p_packs_entirely():
    from mgatk2_amd.synth import FLAG_PACK32, FLAG_PACKED

    reads = _corpus("P")
    assert {r["flag"] for r in reads} == {0x1, 0x11} and max(r["reference_start"] for r in reads) < cc.MITO_LEN
    assert (_packed("P", "p64").flag & FLAG_PACKED).all()
    for pair in cc.PAIRS32:
        assert (_packed("P", "p32", pair).flag & FLAG_PACK32).all(), pair


def test_pack_corpus_gives_pack_reads_records():
    """The corpus packer against pack_reads, byte for byte, on every tenth read of
    corpus A in each layout and at each pair."""
    from mgatk2_amd.synth import pack_reads

    sub = _corpus("A")[::10]
    cases = [("full", None, dict(pack=False)), ("p64", None, {})]
    cases += [("p32", p, dict(pack32=p[0], pack32_dist=p[1])) for p in cc.PAIRS]
    for layout, pair, kw in cases:
        want, got = pack_reads(sub, **kw), cc.pack_corpus(sub, layout, pair)
        for k in ("start", "bc", "tlen", "flag", "mapq", "span", "rec_off", "payload"):
            np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=f"{layout} {pair} {k}")


@pytest.mark.parametrize("pair", cc.PAIRS, ids=lambda p: f"q{p[0]}_d{p[1]}")
def test_oracle_agrees_across_layouts(oracle_lib, pair):
    """Full, 64-byte and 32-byte records of corpora A and B mean the same thing."""
    from mgatk2_amd.synth import FLAG_PACK32, FLAG_PACKED

    reads = _corpus("A")
    layouts = [("p64", None)] + ([("p32", pair)] if pair[1] <= 15 else [])
    cells_b = cc.corpus_b_cells(len(reads))
    for corpus, nc, dedups in (("A", 6, ("none", "alignment_start")), ("B", 2, ("none",))):
        for dedup in dedups:
            cfg = _cfg(pair, nc, dedup)
            base = _packed("A", "full")
            base = base if corpus == "A" else cc.with_cells(base, cells_b)
            exp, _ = oracle_lib.oracle_run(cfg, base)
            assert exp.counts.any() and exp.passed.any()
            for layout, p in layouts:
                soa = _packed("A", layout, p)
                assert (soa.flag & (FLAG_PACK32 if layout == "p32" else FLAG_PACKED)).sum() > 12_000
                soa = soa if corpus == "A" else cc.with_cells(soa, cells_b)
                got, _ = oracle_lib.oracle_run(cfg, soa)
                msg = cc.describe_mismatch(got, exp, soa, reads, cc.STRATA if corpus == "A" else None)
                assert msg is None, f"corpus {corpus} {layout} {pair} {dedup}: {msg}"
                np.testing.assert_array_equal(got.first_read, exp.first_read)


def _python_pileup(reads, n_cells, mito_len, min_baseq, min_dist):
    """pileup.py:32-95 for reads that pass the reader's filters."""
    counts = np.zeros((n_cells, mito_len, 8), np.uint32)
    for r in reads:
        if r["flag"] & 0x904 or r["bc"] < 0 or r["mapping_quality"] < cc.MIN_MAPQ:
            continue
        seq, n = r["query_sequence"], len(r["query_sequence"])
        qual = np.array(r["query_qualities"], np.uint8).astype(np.int8)
        lo, hi = (min_dist, n - min_dist) if min_dist > 0 else (0, n)
        ref, q = r["reference_start"], 0
        for op, ln in r["cigartuples"]:
            if op in (0, 7, 8):
                for p in range(max(0, ref), min(ref + ln, mito_len)):
                    k = q + p - ref
                    if lo <= k < hi and qual[k] >= min_baseq and seq[k] in "ACGT":
                        counts[r["bc"], p, 2 * "ACGT".index(seq[k]) + (1 if r["flag"] & 0x10 else 0)] += 1
                q, ref = q + ln, ref + ln
            elif op in (2, 3):
                ref += ln
            elif op == 4:
                q += ln
    return counts


@pytest.mark.parametrize("name", ["A", "W"])
def test_oracle_equals_python_pileup_on_a_sample(oracle_lib, name):
    from mgatk2_amd.synth import pack_reads

    reads = _corpus(name)
    sub = reads[:: len(reads) // 500]
    assert len(set(r["stratum"] for r in sub)) == len(set(r["stratum"] for r in reads))
    mito_len = cc.MITO_LEN if name == "A" else cc.ONE_WINDOW_LEN
    soa = pack_reads(sub, pack=False)
    for pair in cc.PAIRS:
        got, _ = oracle_lib.oracle_run(_cfg(pair, 6, mito_len=mito_len), soa)
        np.testing.assert_array_equal(got.counts, _python_pileup(sub, 6, mito_len, *pair), err_msg=str(pair))
    assert got.counts.any()
