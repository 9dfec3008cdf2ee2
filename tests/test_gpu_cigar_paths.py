"""GPU: the pileup's CIGAR paths (pile_line, pile_bases<false>, pile_bases_packed,
pile_bases_p32, pile_slow, tn5_cut in the three forms of k_pileup) on the random
corpus of tests/cigar_corpus.py: reads of every CIGAR shape at the window edges, in
the full, 64-byte and 32-byte layouts. Every result is bit-equal to the oracle on the
same ReadSoA; tests/test_cigar_corpus.py shows on CPU that the oracle gives the three
layouts the same result. A failure names the first differing (cell, position, column)
and the reads over it."""

from __future__ import annotations

import functools
from dataclasses import replace

import numpy as np
import pytest

import cigar_corpus as cc

pytestmark = pytest.mark.gpu


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


def _run(engine_lib, cfg, soa):
    with engine_lib.Engine(cfg) as eng:
        eng.push(soa)
        eng.run()
        return eng.fetch()


def _check(engine_lib, oracle_lib, cfg, soa, reads, what, cells=None, got=None):
    got = _run(engine_lib, cfg, soa) if got is None else got
    exp, _ = oracle_lib.oracle_run(cfg, soa)
    assert exp.counts.any(), what
    msg = cc.describe_mismatch(got, exp, soa, reads, cells)
    assert msg is None, f"{what}: {msg}"
    return got


def _layout_shares(soa):
    from mgatk2_amd.synth import FLAG_PACK32, FLAG_PACKED

    p32 = int(((soa.flag & FLAG_PACK32) != 0).sum())
    p64 = int(((soa.flag & FLAG_PACKED) != 0).sum())
    return p32, p64, soa.n - p32 - p64


_ids = lambda p: f"q{p[0]}_d{p[1]}"  # noqa: E731
_A_CASES = [pytest.param(lay, p, id=f"{lay}-{_ids(p)}") for lay in ("full", "p64", "p32")
            for p in (cc.PAIRS32 if lay == "p32" else cc.PAIRS)]


def test_window_geometry_is_the_engines(engine_lib):
    for mito_len in (cc.MITO_LEN, cc.ONE_WINDOW_LEN):
        with engine_lib.Engine(_cfg((20, 5), 1, mito_len=mito_len)) as eng:
            assert eng.windows() == cc.window_geometry(mito_len)


@pytest.mark.parametrize("layout, pair", _A_CASES)
def test_corpus_a_strata_by_cell(engine_lib, oracle_lib, layout, pair):
    """One stratum per cell: a difference names the stratum, so the path."""
    reads = _corpus("A")
    soa = _packed("A", layout, pair if layout == "p32" else None)
    p32, p64, full = _layout_shares(soa)
    print(f"corpus A as {layout}: {p32} 32-byte, {p64} 64-byte, {full} full records")
    assert (p32 if layout == "p32" else p64 if layout == "p64" else full) > 12_000
    dedups = ("none", "alignment_start", "alignment_and_fragment_length") if pair in ((20, 5), (0, 0)) else ("none",)
    for dedup in dedups:
        got = _check(engine_lib, oracle_lib, _cfg(pair, 6, dedup), soa, reads, f"A {layout} {pair} {dedup}", cc.STRATA)
        if dedup != "none":
            assert got.stats["duplicate_reads_with_length"] > 100


@pytest.mark.parametrize("pair", [(20, 5), (0, 0), (0, 15)], ids=_ids)
def test_corpus_b_mixed_layouts_in_a_wave(engine_lib, oracle_lib, pair):
    """All strata in two cells, read i in layout i mod 3: waves mix register and
    slow lanes and the three layouts (kLayAny)."""
    from mgatk2_amd.shard import shard_soa
    from mgatk2_amd.synth import FLAG_PACK32, FLAG_PACKED, ReadSoA, concat_soa

    reads = _corpus("A")
    n = len(reads)
    cells = cc.corpus_b_cells(n)
    parts = [cc.with_cells(_packed("A", lay, p), cells) for lay, p in (("p32", pair), ("p64", None), ("full", None))]
    cat = concat_soa(parts)
    idx = np.arange(n) + n * (np.arange(n) % 3)
    mixed = ReadSoA(cat.start[idx], cat.bc[idx], cat.tlen[idx], cat.flag[idx], cat.mapq[idx], cat.span[idx],
                    cat.rec_off[idx], cat.payload)
    mixed, _ = shard_soa(mixed, 0, 2, paired=True, keep_all=True)
    p32, p64, full = _layout_shares(mixed)
    print(f"corpus B mixed: {p32} 32-byte, {p64} 64-byte, {full} full records")
    assert p32 > 3000 and p64 > 3000 and full > 7000
    assert (mixed.flag & FLAG_PACK32).any() and (mixed.flag & FLAG_PACKED).any()
    assert ((mixed.flag & (FLAG_PACK32 | FLAG_PACKED)) == 0).any()
    for dedup in ("none", "alignment_and_fragment_length"):
        _check(engine_lib, oracle_lib, _cfg(pair, 2, dedup), mixed, reads, f"B mixed {pair} {dedup}")


@pytest.mark.parametrize("pair", [(20, 5), (0, 0), (0, 15)], ids=_ids)
@pytest.mark.parametrize("placement", ["p64_dense", "p64_paired", "p32_dense", "p32_quad"])
def test_corpus_p_all_packed_kernels(engine_lib, oracle_lib, monkeypatch, placement, pair):
    """Every record packed: k_pileup<kLayP64> / <kLayP32>, with the compact and the
    wide grouping element."""
    from mgatk2_amd.synth import FLAG_PACK32, FLAG_PACKED, relocate

    reads = _corpus("P")
    layout = placement[:3]
    soa = _packed("P", layout, pair if layout == "p32" else None)
    if placement in ("p64_paired", "p32_quad"):
        soa = relocate(soa, paired=True, n_cells=4)
    assert (soa.flag & (FLAG_PACK32 if layout == "p32" else FLAG_PACKED)).all()  # no full-layout record
    dedup = "alignment_and_fragment_length" if pair == (20, 5) else "none"
    for wide in ("0", "1"):
        monkeypatch.setenv("MGP_GROUP_WIDE", wide)
        _check(engine_lib, oracle_lib, _cfg(pair, 4, dedup), soa, reads, f"P {placement} {pair} wide={wide}",
               cc.PACKED_STRATA)


@pytest.mark.parametrize("layout", ["p32", "full"])
def test_corpus_a_streamed(engine_lib, oracle_lib, layout):
    """Batches of 3,000 reads on a streaming context: two_far's long N/D reads reach
    over the segment ends."""
    pair = (20, 5)
    reads = _corpus("A")
    soa = _packed("A", layout, pair if layout == "p32" else None)
    cfg = _cfg(pair, 6, "alignment_and_fragment_length")
    scfg = replace(cfg, stream=True, reserve_reads=soa.n, reserve_payload=int(soa.payload.shape[0]) + 65536)
    with engine_lib.Engine(scfg) as eng:
        for a in range(0, soa.n, 3000):
            eng.push(soa.slice(a, min(soa.n, a + 3000)))
        segs, _ = eng.stream_info()
        eng.run()
        got = eng.fetch()
    assert segs > 0
    _check(engine_lib, oracle_lib, cfg, soa, reads, f"A streamed {layout}", cc.STRATA, got=got)


@pytest.mark.parametrize("layout", ["full", "p64", "p32"])
def test_one_window_genome(engine_lib, oracle_lib, layout):
    """mito_len 1000 is one window of 1000 positions: every clamp of a read starting
    in [880, 1005] is the end-of-genome clamp."""
    pair = (0, 0)
    reads = _corpus("W")
    soa = _packed("W", layout, pair if layout == "p32" else None)
    cfg = _cfg(pair, 3, mito_len=cc.ONE_WINDOW_LEN)
    _check(engine_lib, oracle_lib, cfg, soa, reads, f"one window {layout}", cc.ONE_WINDOW_STRATA)


def test_second_run_gives_the_same_arrays(engine_lib):
    soa = _packed("A", "p32", (20, 5))
    with engine_lib.Engine(_cfg((20, 5), 6, "alignment_start")) as eng:
        eng.push(soa)
        eng.run()
        a = eng.fetch()
        eng.run()
        b = eng.fetch()
    assert a.counts.any()
    for k in cc.ARRAYS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
    assert a.stats == b.stats
