"""The cell sweeps (sweep() of mgp_sweep.h: k_moments, k_dev2, k_pos_stats) and k_gather at the
slab sizes a production run gives them, and at windows that straddle a sweep block.

A slab goes round sweep()'s 128-cell staging loop a second time only when it holds more than 128
cells; the other GPU tests' slabs hold 20 to 64. Here the populations are 530 to 2083 entries long,
drawn from a handful of distinct rows, so the reference is exact and cheap: the sum over the distinct
rows of multiplicity x that row's own contribution, each taken from the existing full-array oracles
(test_variants.oracle_moments / oracle_dev2, test_coverage.oracle_position_ints) run on the row as a
population of one. The helper is checked on the CPU against those oracles run on the whole
population (test_weighted_oracle_equals_the_full_arrays).

Integers: bit-equal. s_af: atol = n * tol(n), as test_gpu_variants.check_moments. dev2 / (n - 1):
rtol = atol = tol(n), the variance's bound (test_variants.tol, with its derivation). The matrix:
bit-equal. Two calls on the same rows: identical bytes.

Every GPU test asserts through sweep_slab() / slab_chunks(), a mirror of the library's slab
arithmetic, that its population gives the slabs, chunks and tails it was written for.

Two builds with a deliberate error in sweep() were run against this module (neither is kept):
later chunks re-staging the first chunk's indices fails both caller-row cases and the long
straddled populations; the second flag column ignored (myw = 0) fails only where the drained
window is the upper one of a block (`straddle_upper`), because the u32 rows are exact everywhere.
The other sweep tests pass on both builds.
"""

from __future__ import annotations

import math

import numpy as np
import pytest

from test_coverage import POS_INTS, _exact, check_ints, oracle_position_ints
from test_coverage import crafted_rows as coverage_crafted_rows
from test_coverage import population as coverage_population
from test_variants import INT_FIELDS, oracle_allele_freq, oracle_dev2, oracle_moments, tol
from test_variants import crafted_rows as variant_crafted_rows
from test_variants import population as variant_population

gpu = pytest.mark.gpu

# mgp_sweep.h: kBlock, kChunk, kUnroll; mgp_variants.hip / mgp_qc.hip: kTargetGroups, 32 cells at least
BLOCK, CHUNK, UNROLL, GROUPS, LEAST = 256, 128, 4, 1024, 32
MAX_L = 1 << 16  # qc::kMaxL
STRADDLE_L = 16299  # mouse chrM: windows of 1256 positions, no multiple of BLOCK


# ---- the slab arithmetic, for preconditions only ------------------------------------------
def sweep_slab(n: int, L: int) -> int:
    """Cells per slab of a sweep over n cells and L positions. Mirrors slab_cells(n, L) of
    mgp_variants.hip and slab_cells(n, gx, kTargetGroups, 32) of mgp_qc.hip."""
    n = max(n, 1)
    gx = -(-L // BLOCK)
    want = max(1, GROUPS // gx)
    ns = max(1, min(want, -(-n // LEAST)))
    return -(-n // ns)


def slab_chunks(n: int, L: int) -> list:
    """[(first list position, [cells of each staged chunk])] of every slab."""
    slab = sweep_slab(n, L)
    out = []
    for k0 in range(0, n, slab):
        m = min(slab, n - k0)
        out.append((k0, [min(CHUNK, m - c) for c in range(0, m, CHUNK)]))
    return out


def second_chunk_positions(layout) -> np.ndarray:
    """The list positions every slab's second staged chunk holds."""
    return np.concatenate([np.arange(k0 + CHUNK, k0 + CHUNK + ch[1]) for k0, ch in layout if len(ch) > 1])


def last_tail_positions(layout) -> np.ndarray:
    k0, ch = layout[-1]
    return np.arange(k0 + sum(ch[:-1]), k0 + sum(ch))


# ---- the weighted oracle --------------------------------------------------------------------
def _zero_row_added(a):
    a = np.asarray(a)
    return np.concatenate([a, np.zeros((1,) + a.shape[1:], a.dtype)])


def _distinct(cells, n_rows):
    """(distinct rows, their multiplicities, the list with -1 as row n_rows: the row of zeros)."""
    ids = np.asarray(cells, np.int64)
    ids = np.where(ids < 0, n_rows, ids)
    rows, mult = np.unique(ids, return_counts=True)
    return rows.tolist(), mult.tolist(), ids


def _fsum(terms):
    """math.fsum over the list's arrays, element by element."""
    flat = np.stack(terms).reshape(len(terms), -1).T.tolist()
    return np.array([math.fsum(col) for col in flat]).reshape(terms[0].shape)


def weighted_moments(counts, depth, cells, thr=0):
    """oracle_moments of the population `cells`, from the distinct rows alone."""
    c, d = _zero_row_added(counts), _zero_row_added(depth)
    rows, mult, _ = _distinct(cells, len(counts))
    out, terms = {}, []
    for r, m in zip(rows, mult):
        one = oracle_moments(c[r:r + 1], d[r:r + 1], thr)
        for k in INT_FIELDS:
            out[k] = out.get(k, np.uint64(0)) + np.uint64(m) * one[k]
        terms.append(float(m) * one["s_af"])
    out["s_af"] = _fsum(terms)
    return out


def weighted_dev2(counts, depth, cells, mu, thr=0):
    c, d = _zero_row_added(counts), _zero_row_added(depth)
    rows, mult, _ = _distinct(cells, len(counts))
    return _fsum([float(m) * oracle_dev2(c[r:r + 1], d[r:r + 1], mu, thr) for r, m in zip(rows, mult)])


def weighted_position(counts, tn5, depth, cells):
    """oracle_position_ints' POS_INTS of the population, in Python integers."""
    c, t, d = _zero_row_added(counts), _zero_row_added(tn5), _zero_row_added(depth)
    rows, mult, _ = _distinct(cells, len(counts))
    out = {}
    for r, m in zip(rows, mult):
        one = oracle_position_ints(c[r:r + 1], t[r:r + 1], d[r:r + 1])
        for k in POS_INTS:
            v = _exact(one[k])
            out[k] = (np.maximum(out[k], v) if k in out else v) if k == "max_depth" else out.get(k, 0) + int(m) * v
    return out


def weighted_allele_freq(counts, depth, cells, pairs, min_coverage=1):
    c, d = _zero_row_added(counts), _zero_row_added(depth)
    _, _, ids = _distinct(cells, len(counts))
    return oracle_allele_freq(c, d, pairs, min_coverage)[:, ids]


# ---- rows and populations ---------------------------------------------------------------------
VARIANT_PICK = (0, 5, 11, 20, 23, 31, 3, 26)  # of test_variants.crafted_rows: one row of each of its cases
TILE = 300 + 333


def slab_rows(L: int, seed: int = 3):
    """Eight u32 rows (counts [8, L, 8], tn5 [8, L, 2], depth [8, L]): the columns of
    test_variants.crafted_rows (300 positions; counts above 65,535 at column 9) beside those of
    test_coverage.crafted_rows (333 positions; a depth of 2^24 - 1 at its column 5), tiled along
    L. The first tile is theirs unchanged; the later ones get a small count that differs from tile
    to tile and row to row, so no two position blocks hold the same numbers."""
    vc, _ = variant_crafted_rows()
    vc = vc[list(VARIANT_PICK)]
    cc, ct, _ = coverage_crafted_rows(8, 333)
    rng = np.random.default_rng(seed)
    vt = (rng.random((8, 300, 2)) * 4 * (rng.random((8, 300, 1)) < 0.3)).astype(np.uint32)
    reps = -(-L // TILE)
    counts = np.tile(np.concatenate([vc, cc], axis=1), (1, reps, 1))[:, :L].copy()
    tn5 = np.tile(np.concatenate([vt, ct], axis=1), (1, reps, 1))[:, :L].copy()
    tile = np.arange(L) // TILE
    small = counts.astype(np.int64).sum(axis=2) < 1 << 20
    bump = (tile[None, :] + np.arange(8)[:, None]) % 4 * (tile[None, :] > 0) * small
    counts[:, :, 6] += bump.astype(np.uint32)
    tn5[:, :, 1] += (bump % 3).astype(np.uint32)
    depth = counts.astype(np.int64).sum(axis=2)
    assert counts.max() < 1 << 24 and (counts > 65_535).any()
    assert depth.max() == (1 << 24) - 1 or L < 300 + 6
    return counts, tn5, depth.astype(np.uint32)


def placed_population(n: int, L: int, general, second_row: int, tail_row: int, seed: int) -> np.ndarray:
    """A list of n entries over the rows `general` and -1, with unequal multiplicities, in
    which `second_row` occurs only inside second staged chunks (at a chunk's first and last
    cell among them, never in the last tail) and `tail_row` only in the last slab's tail."""
    layout = slab_chunks(n, L)
    rng = np.random.default_rng(seed)
    w = np.arange(len(general) + 1, 0, -1, dtype=np.float64)  # (-1 the rarest)
    cells = rng.choice(np.array(list(general) + [-1]), size=n, p=w / w.sum())
    tail = last_tail_positions(layout)
    inner = np.setdiff1d(second_chunk_positions(layout), tail)
    first = inner[inner < layout[1][0]]  # the first slab's second chunk
    cells[np.concatenate([first[[0, -1]], rng.choice(np.setdiff1d(inner, first), 3, replace=False)])] = second_row
    cells[tail[-1]] = tail_row
    if tail.size >= 3:
        cells[tail[0]], cells[tail[1]] = tail_row, -1
    return cells.astype(np.int32)


def check_placement(cells, layout, second_row, tail_row):
    """The preconditions of a placed population: a wrong, skipped or replayed later chunk
    changes the sums."""
    tail = last_tail_positions(layout)
    at_second, at_tail = np.flatnonzero(cells == second_row), np.flatnonzero(cells == tail_row)
    assert at_second.size >= 2 and np.isin(at_second, np.setdiff1d(second_chunk_positions(layout), tail)).all()
    assert at_tail.size >= 1 and np.isin(at_tail, tail).all()
    mult = np.unique(cells, return_counts=True)[1]
    assert len(set(mult.tolist())) >= 4 and int((cells == -1).sum()) >= 3


def same_bytes(a, b):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- 1. the oracle and the mirror, on the CPU ------------------------------------------------
def test_weighted_oracle_equals_the_full_arrays():
    """A population of 41 over eight short rows: the weighted helper against the existing
    oracles run on the whole population's arrays. The slab mirror against the library's slab
    sizes for the shapes of the other tests and of the measured workload."""
    from mgatk2_amd.analysis.variants import mean_af

    counts, tn5, depth = slab_rows(700)
    rng = np.random.default_rng(17)
    cells = np.concatenate([rng.choice(8, size=37, p=np.arange(8, 0, -1) / 36.0), [-1, -1, -1, 7]])
    rng.shuffle(cells)
    n = cells.size
    assert len(set(np.unique(cells, return_counts=True)[1].tolist())) >= 4 and set(cells.tolist()) == set(range(-1, 8))
    pc, pd = variant_population(counts, depth, cells)
    for thr in (0, 10):
        full, got = oracle_moments(pc, pd, thr), weighted_moments(counts, depth, cells, thr)
        for k in INT_FIELDS:
            assert got[k].dtype == np.uint64
            np.testing.assert_array_equal(got[k], full[k], err_msg=f"thr {thr} {k}")
        assert (full["n_low"] > 0).any() == (thr > 0)
        np.testing.assert_allclose(got["s_af"], full["s_af"], rtol=0, atol=n * tol(n))
        mu = mean_af(full, n)
        np.testing.assert_allclose(weighted_dev2(counts, depth, cells, mu, thr) / (n - 1),
                                   oracle_dev2(pc, pd, mu, thr) / (n - 1), rtol=tol(n), atol=tol(n))
    got = weighted_position(counts, tn5, depth, cells)
    full = oracle_position_ints(*coverage_population(counts, tn5, depth, cells))
    for k in POS_INTS:
        assert _exact(got[k]).tolist() == _exact(full[k]).tolist(), k
    pairs = [(9, b) for b in range(4)] + [(0, 1), (305, 2), (699, 3)]
    for min_cov in (1, 12):
        np.testing.assert_array_equal(weighted_allele_freq(counts, depth, cells, pairs, min_cov),
                                      oracle_allele_freq(pc, pd, pairs, min_cov))
    # the mirror: the slab sizes of the suite's other shapes and of the measured workload
    shapes = ((150, 333), (40, 300), (130, 16569), (65536, 70), (65536, 8), (10_000, 16569))
    assert [sweep_slab(*s) for s in shapes] == [30, 20, 26, 64, 64, 667]
    assert slab_chunks(10_000, 16569)[0] == (0, [128] * 5 + [27]) and len(slab_chunks(10_000, 16569)) == 15


# ---- 2. caller rows over several chunks -------------------------------------------------------
@pytest.fixture(scope="module")
def long_rows():
    return slab_rows(MAX_L)


LAYOUTS = {
    530: [(0, [128, 5]), (133, [128, 5]), (266, [128, 5]), (399, [128, 3])],  # a tail shorter than the unroll
    1028: [(k0, [128, 128, 1]) for k0 in (0, 257, 514, 771)],  # a third chunk of one cell
}


def long_population(n):
    """The list of n over rows 0..5 and -1, row 6 in second chunks only, row 7 in the last
    tail only, with its preconditions asserted."""
    layout = slab_chunks(n, MAX_L)
    assert sweep_slab(n, MAX_L) > CHUNK and layout == LAYOUTS[n]
    tails = [ch[-1] for _, ch in layout]  # none ends on a full group of kUnroll rows, one is shorter than a group
    assert all(t % UNROLL for t in tails) and min(tails) < UNROLL
    cells = placed_population(n, MAX_L, range(6), 6, 7, seed=n)
    check_placement(cells, layout, 6, 7)
    return cells


@gpu
@pytest.mark.parametrize("n", [530, 1028])
def test_caller_rows_over_several_chunks(engine_lib, long_rows, n):
    """L = 65,536 (four slabs). n = 530: slabs of 133, 133, 133, 131 cells, staged as 128 + 5 and
    128 + 3. n = 1028: four slabs of 257, staged as 128 + 128 + 1. One row lies only in second
    chunks (at their first and last cell too), one only in the last tail."""
    from mgatk2_amd.analysis.variants import mean_af

    eng = engine_lib
    counts, tn5, depth = long_rows
    cells = long_population(n)
    for thr in (0, 10):
        mom = eng.variant_moments_rows(counts, depth, cells, thr)
        want = weighted_moments(counts, depth, cells, thr)
        for k in INT_FIELDS:
            assert mom[k].dtype == np.uint64
            np.testing.assert_array_equal(mom[k], want[k], err_msg=f"n {n} thr {thr} {k}")
        np.testing.assert_allclose(mom["s_af"], want["s_af"], rtol=0, atol=n * tol(n), err_msg=f"n {n} thr {thr} s_af")
        assert (mom["n_low"] > 0).any() == (thr > 0) and int(mom["sff"].max()) > 2 ** 40
        mu = mean_af(mom, n)
        dev2 = eng.variant_dev2_rows(counts, depth, mu, cells, thr)
        np.testing.assert_allclose(dev2 / (n - 1), weighted_dev2(counts, depth, cells, mu, thr) / (n - 1),
                                   rtol=tol(n), atol=tol(n), err_msg=f"n {n} thr {thr} dev2")
        if thr == 0:
            same_bytes(mom, eng.variant_moments_rows(counts, depth, cells, thr))
            assert dev2.tobytes() == eng.variant_dev2_rows(counts, depth, mu, cells, thr).tobytes()
    pos = eng.position_coverage_rows(counts, tn5, depth, cells)
    check_ints(pos, weighted_position(counts, tn5, depth, cells), POS_INTS, f"n {n} position")
    assert int(pos["max_depth"].max()) == (1 << 24) - 1
    assert int(pos["s_tn5_fwd"].max()) > 0 and int(pos["s_tn5_rev"].max()) > 0
    assert 0 < int(pos["n_tn5"].max()) <= n
    same_bytes(pos, eng.position_coverage_rows(counts, tn5, depth, cells))


@gpu
def test_gather_over_three_cell_blocks(engine_lib, long_rows):
    """k_gather with grid.x = 3 (the n = 530 list), pairs at the first, middle and last
    positions and at the columns with counts above 65,535 and the depth of 2^24 - 1."""
    counts, _, depth = long_rows
    cells = long_population(530)
    assert -(-cells.size // BLOCK) == 3
    pairs = [(p, b) for p in (0, 9, 300 + 5, MAX_L // 2, MAX_L - 1) for b in range(4)]
    for min_cov in (1, 12):
        af = engine_lib.allele_freq_rows(counts, depth, pairs, cells, min_cov)
        assert af.dtype == np.float64 and af.shape == (len(pairs), 530)
        np.testing.assert_array_equal(af, weighted_allele_freq(counts, depth, cells, pairs, min_cov))
    assert (af > 0).any(axis=1).sum() >= 5 and (af[:, cells == 7] > 0).any() and (af[:, cells == -1] == 0).all()


# ---- 3. the gather's launch loop ----------------------------------------------------------------
@gpu
def test_gather_launch_loop(engine_lib):
    """65,535 + 3 pairs over 3 rows x 8 positions: variants::gather launches twice (grid.y's
    limit). The three pairs of the second launch are not the first launch's first three."""
    rng = np.random.default_rng(23)
    counts = rng.integers(0, 50, size=(3, 8, 8)).astype(np.uint32)
    counts[1, 2] = 0  # a depth of zero
    counts[2, 5, 3] = 70_000
    depth = counts.astype(np.int64).sum(axis=2).astype(np.uint32)
    distinct = [(p, b) for p in range(8) for b in range(4)]
    idx = rng.integers(0, len(distinct), size=65_535 + 3)
    idx[:3], idx[-3:] = (0, 1, 2), (29, 21, 10)
    table = oracle_allele_freq(counts, depth, distinct)  # [32, 3]
    assert idx.size > 65_535 and not (table[idx[:3]] == table[idx[-3:]]).any()
    af = engine_lib.allele_freq_rows(counts, depth, [distinct[i] for i in idx.tolist()])
    assert af.shape == (idx.size, 3)
    np.testing.assert_array_equal(af, table[idx])


# ---- 4. engine rows whose windows straddle the sweep's blocks -----------------------------------
def straddle_context(engine_lib, first):
    """The context of the wide-window tests (one cell 180k deep over 110 positions from
    `first`) at mito_len = 16,299, with ordinary reads over the genome for all five cells, the
    deep one included. Left open for the module's tests."""
    from mgatk2_amd.engine import EngineConfig
    from mgatk2_amd.file_io.writers import ref_alleles
    from mgatk2_amd.synth import ReadSoA, concat_soa, synth_reads

    L = STRADDLE_L
    deep = synth_reads(91, 400_000, 1, mito_len=L)
    deep.start[:] = (first + np.sort(deep.start % 60)).astype(np.int32)
    deep.payload.reshape(-1, 64)[:, 0:4] = deep.start.view(np.uint8).reshape(-1, 4)
    rest = synth_reads(92, 40_000, 5, mito_len=L)
    both = concat_soa([deep, rest])
    order = np.argsort(both.start, kind="stable")  # coordinate order; the records stay where they are
    soa = ReadSoA(*[np.ascontiguousarray(getattr(both, k)[order]) for k in ("start", "bc", "tlen", "flag", "mapq",
                                                                            "span", "rec_off")], both.payload)
    cfg = EngineConfig(n_cells=5, min_baseq=0, min_mapq=0, dedup_mode="none", min_reads=0, mito_len=L)
    with engine_lib.Engine(cfg) as eng:
        eng.push(soa)
        eng.run()
        res = eng.fetch()
        yield dict(eng=eng, res=res, rows16=eng.fetch_rows16(), ref=ref_alleles(res.ref_tally),
                   deep_window=first // 1256)


@pytest.fixture(scope="module")
def straddle(engine_lib):
    """The deep reads over positions [0, 110): window 0 of cell 0 is drained, window 1 is not."""
    yield from straddle_context(engine_lib, 0)


@pytest.fixture(scope="module")
def straddle_upper(engine_lib):
    """The deep reads over positions [1256, 1366): window 1 of cell 0 is drained, window 0 is
    not, and the depths above 65,535 begin inside the sweep block [1024, 1280). The u32 rows are
    exact in every window, so a sweep that took window 0's flag for these positions would pass
    on `straddle` (it reads the exact rows where the 16-bit ones would do); here it reads the
    saturated 16-bit rows."""
    yield from straddle_context(engine_lib, 1256)


def check_straddle(s):
    """Of cell 0's windows 0 and 1 one is drained and the other is not, their boundary lies
    inside the sweep block [1024, 1280), and cell 0 has depth on both sides of it."""
    res, r16 = s["res"], s["rows16"]
    W = r16.window_width
    assert W == 1256 and W % BLOCK != 0 and 1024 // W == 0 and 1279 // W == 1
    if s["deep_window"] == 0:
        assert r16.wide[0, 0] and not r16.wide[0, 1]
    else:
        assert r16.wide[0, 1] and not r16.wide[0, 0] and res.depth[0, W:1280].max() > 65_535
    assert res.depth[0, 1024:W].any() and res.depth[0, W:1280].any()
    assert res.depth.max() > 65_535 and res.depth.shape == (5, STRADDLE_L)


@gpu
def test_straddled_window_small_populations(straddle):
    """The plain population and a short listed one, against the full-array oracles as
    test_wide_window_uses_the_exact_rows of test_gpu_variants and test_gpu_coverage: one chunk,
    so what is new is the second staged flag column (myw == 1)."""
    from test_gpu_coverage import check_against_oracle, device_all
    from test_gpu_variants import check_moments, device_table
    from test_variants import check_table, oracle_table

    check_straddle(straddle)
    eng, res, ref = straddle["eng"], straddle["res"], straddle["ref"]
    calls = (lambda c, t: eng.variant_moments(c, t), lambda mu, c, t: eng.variant_dev2(mu, c, t))
    for name, cells in (("all", None), ("listed", np.array([4, 0, -1, 2, 1, 3, 0], np.int32))):
        pc, pd = variant_population(res.counts, res.depth, cells)
        n = pc.shape[0]
        mom, dev2, table = device_table(calls, res.counts, res.depth, ref, n, 0, (0, -1.0, 0.0), cells)
        check_moments(mom, pc, pd, 0, f"straddle {name}")
        assert int(mom["s_cov"].max()) > 65_535 + 4 * 1000
        want, _ = oracle_table(pc, pd, ref, 0, 0, -1.0, 0.0)
        assert any(p < 110 for p, _ in want) and any(1256 <= p < 1280 for p, _ in want)
        check_table(table, want, n, f"straddle {name}")
        np.testing.assert_array_equal(eng.allele_freq(table.pairs(), cells), oracle_allele_freq(pc, pd, table.pairs()))
        pc, pt, pd = coverage_population(res.counts, res.tn5, res.depth, cells)
        got = device_all(eng, cells, n)
        check_against_oracle(*got[:4], pc, pt, pd, f"straddle {name}")
        assert int(got[1]["max_depth"].max()) > 65_535 and int(got[0]["max_depth"].max()) > 65_535


@gpu
def test_straddled_window_drained_above_the_boundary(straddle_upper):
    """The plain population of the context whose drained window is the upper one of the block:
    one chunk, so a failure here is the flag column alone."""
    from test_gpu_variants import check_moments

    check_straddle(straddle_upper)
    eng, res = straddle_upper["eng"], straddle_upper["res"]
    mom = eng.variant_moments(None, 0)
    check_moments(mom, res.counts, res.depth, 0, "drained above")
    assert int(mom["s_cov"][1256:1280].max()) > 65_535 + 4 * 1000
    pos = eng.position_coverage(None)
    check_ints(pos, oracle_position_ints(res.counts, res.tn5, res.depth), POS_INTS, "drained above")
    assert int(pos["max_depth"][1256:1280].max()) > 65_535
    pairs = [(p, b) for p in (1255, 1256, 1270, 1279, 1280) for b in range(4)]
    np.testing.assert_array_equal(eng.allele_freq(pairs), oracle_allele_freq(res.counts, res.depth, pairs))


@gpu
@pytest.mark.parametrize("context", ["straddle", "straddle_upper"])
def test_straddled_window_over_several_chunks(request, context):
    """A listed population of 2083 over the five cells and -1: 15 slabs of 131 (128 + 3) and
    one of 118. The deep cell lies only in second chunks, which here are the tails. The 16-bit
    rows, the drained window, the straddled block and the re-staging together, against the
    weighted oracle on fetch()'s exact rows; with the drained window below and above the
    boundary inside the block."""
    from mgatk2_amd.analysis.variants import mean_af

    straddle = request.getfixturevalue(context)
    check_straddle(straddle)
    eng, res = straddle["eng"], straddle["res"]
    n, L = 2083, STRADDLE_L
    layout = slab_chunks(n, L)
    assert sweep_slab(n, L) == 131 and layout == [(131 * s, [128, 3]) for s in range(15)] + [(1965, [118])]
    rng = np.random.default_rng(41)
    cells = rng.choice(np.array([1, 2, 3, 4, -1]), size=n, p=np.array([16, 9, 6, 4, 1]) / 36.0)
    at = np.array([131 * 2 + 128, 131 * 7 + 130, 131 * 11 + 129, 131 * 14 + 128, 131 * 14 + 130])
    cells[at] = 0
    cells = cells.astype(np.int32)
    assert np.isin(np.flatnonzero(cells == 0), second_chunk_positions(layout)).all() and (cells == 0).sum() == at.size
    assert len(set(np.unique(cells, return_counts=True)[1].tolist())) == 6 and int((cells == -1).sum()) >= 3
    counts, tn5, depth = res.counts, res.tn5, res.depth
    for thr in (0, 10):
        mom = eng.variant_moments(cells, thr)
        want = weighted_moments(counts, depth, cells, thr)
        for k in INT_FIELDS:
            assert mom[k].dtype == np.uint64
            np.testing.assert_array_equal(mom[k], want[k], err_msg=f"thr {thr} {k}")
        np.testing.assert_allclose(mom["s_af"], want["s_af"], rtol=0, atol=n * tol(n), err_msg=f"thr {thr} s_af")
        mu = mean_af(mom, n)
        dev2 = eng.variant_dev2(mu, cells, thr)
        np.testing.assert_allclose(dev2 / (n - 1), weighted_dev2(counts, depth, cells, mu, thr) / (n - 1),
                                   rtol=tol(n), atol=tol(n), err_msg=f"thr {thr} dev2")
        if thr == 0:
            same_bytes(mom, eng.variant_moments(cells, thr))
            assert dev2.tobytes() == eng.variant_dev2(mu, cells, thr).tobytes()
    pos = eng.position_coverage(cells)
    check_ints(pos, weighted_position(counts, tn5, depth, cells), POS_INTS, "straddle position")
    assert int(pos["max_depth"].max()) > 65_535
    same_bytes(pos, eng.position_coverage(cells))
    pairs = [(p, b) for p in (0, 50, 1100, 1255, 1256, 1270, 1279, 1280, L - 1) for b in range(4)]
    af = eng.allele_freq(pairs, cells)
    np.testing.assert_array_equal(af, weighted_allele_freq(counts, depth, cells, pairs))
    assert (af[:, cells == 0] > 0).any() and af.shape == (len(pairs), n)
