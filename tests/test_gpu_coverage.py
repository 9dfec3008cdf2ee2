"""Coverage QC on the device (mgp_qc.hip) against the numpy oracle of tests/test_coverage.py,
which works from per-cell arrays (np.mean, np.median, np.std(ddof=1), comparisons and sums).

Every integer the device returns, every median, the kept mask, the recomputed alleles and the
strings: bit-equal. The floating-point columns are compared with numpy's own rounded means
and sds: rtol = test_variants.tol(m), atol = tol(m) x the case's largest depth, m = the terms
numpy summed (the oracle's rounding; the device side is exact). Two calls on the same rows:
identical bytes.
"""

from __future__ import annotations

import numpy as np
import pytest

from test_coverage import (CELL_INTS, POS_INTS, check_ints, check_table, crafted_rows, oracle_cell_ints,
                           oracle_cell_table, oracle_position_ints, oracle_position_tables, population)
from test_gpu_variants import CTX_SEED, RUN, _files, _pipeline, _same_file
from test_variants import oracle_allele_freq, oracle_table, tol

pytestmark = pytest.mark.gpu


class RowSource:
    """The four passes over caller rows, with Engine's method names (what run_coverage calls)."""

    def __init__(self, eng, counts, tn5, depth):
        self.eng, self.counts, self.tn5, self.depth = eng, counts, tn5, depth

    def cell_coverage(self, cells=None):
        return self.eng.cell_coverage_rows(self.depth, cells)

    def position_coverage(self, cells=None):
        return self.eng.position_coverage_rows(self.counts, self.tn5, self.depth, cells)

    def position_depth_hist(self, shift, prefix=None, cells=None):
        return self.eng.position_depth_hist_rows(self.depth, shift, prefix, cells)

    def position_depth_next(self, v, cells=None):
        return self.eng.position_depth_next_rows(self.depth, v, cells)


def device_all(src, cells, n):
    """(cell ints, position ints, mid_lo, mid_hi, hist / next calls made) of one source."""
    from mgatk2_amd.analysis.coverage import position_medians

    calls = {"hist": 0, "next": 0}

    def hist_fn(shift, prefix):
        calls["hist"] += 1
        return src.position_depth_hist(shift, prefix, cells)["hist"]

    def next_fn(v):
        calls["next"] += 1
        got = src.position_depth_next(v, cells)
        return got["n_le"], got["next"]

    cell = src.cell_coverage(cells)
    pos = src.position_coverage(cells)
    lo, hi = position_medians(hist_fn, next_fn, pos["max_depth"], n)
    return cell, pos, lo, hi, calls


def check_against_oracle(cell, pos, lo, hi, pc, pt, pd, what):
    """The device's integers bit-equal to the oracle's, then the four tables."""
    from mgatk2_amd.analysis import coverage as cov

    n, L = pd.shape
    top = int(pd.max()) if pd.size else 0
    check_ints(cell, oracle_cell_ints(pd), CELL_INTS, what + " cell")
    want = oracle_position_ints(pc, pt, pd)
    check_ints(pos, want, POS_INTS, what + " position")
    np.testing.assert_array_equal(lo, want["mid_lo"], err_msg=what)
    np.testing.assert_array_equal(hi, want["mid_hi"], err_msg=what)
    check_table(cov.cell_coverage_stats(cell, L), oracle_cell_table(pd), L, top, what + " cell table")
    tabs = oracle_position_tables(pc, pt, pd)
    check_table(cov.position_coverage_stats(pos, lo, hi, n), tabs[0], n, top, what + " position table")
    check_table(cov.strand_coverage_stats(pos, n), tabs[1], 4 * n, top, what + " strand table")
    check_table(cov.transposition_stats(pos, n), tabs[2], n, top, what + " tn5 table")


# ---- 1. crafted rows through the *_rows forms --------------------------------------------
@pytest.fixture(scope="module")
def crafted():
    counts, tn5, depth = crafted_rows()  # 150 rows x 333 positions
    rng = np.random.default_rng(5)
    holes = np.concatenate([rng.permutation(150)[:40], [-1, -1, -1, 17, 17]])  # zero rows and a duplicate
    rng.shuffle(holes)
    pops = {"all": None, "subset": rng.permutation(150)[:77], "holes": holes, "one": np.array([149]),
            "two": np.array([3, 140]), "empty": np.zeros(0, np.int64)}
    return counts, tn5, depth, pops


@pytest.mark.parametrize("pop", ["all", "subset", "holes", "one", "two", "empty"])
def test_crafted_rows(engine_lib, crafted, pop):
    """150 rows give five cell slabs of 30, each a single staging chunk (slabs of more than 128
    cells, which stage twice: tests/test_gpu_sweep_slabs.py); 333 positions are
    one full and one ragged 256-position block and a ragged 64-position block. Columns: all
    zero, constant, differing middles, depths in each byte range up to 2^24 - 1, Tn5 cuts at a
    depth-0 position, ties across the middle."""
    counts, tn5, depth, pops = crafted
    cells = pops[pop]
    pc, pt, pd = population(counts, tn5, depth, cells)
    n = pd.shape[0]
    src = RowSource(engine_lib, counts, tn5, depth)
    cell, pos, lo, hi, calls = device_all(src, cells, n)
    check_against_oracle(cell, pos, lo, hi, pc, pt, pd, pop)
    if n:
        assert calls["hist"] == 3  # depths reach 2^24 - 1 (column 5): three bytes
        rows = n if cells is None else int((np.asarray(cells) >= 0).sum())  # (the -1 rows have no cut)
        assert int(pos["n_tn5"][6]) == rows and int(pos["s_depth"][6]) == 0
    else:
        assert calls == {"hist": 0, "next": 0}
    if pop == "all":
        assert int(lo[2]) != int(hi[2]) and int(lo[7]) == int(hi[7]) and int(pos["max_depth"][5]) == (1 << 24) - 1
        assert calls["next"] == 1
    again = device_all(src, cells, n)
    for a, b in zip((cell, pos), again[:2]):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    assert lo.tobytes() == again[2].tobytes() and hi.tobytes() == again[3].tobytes()
    if n:  # the primitives' own bytes
        pre = (lo >> np.uint32(8)).astype(np.uint32)
        assert src.position_depth_hist(0, pre, cells)["hist"].tobytes() == \
            src.position_depth_hist(0, pre, cells)["hist"].tobytes()
        a, b = src.position_depth_next(lo, cells), src.position_depth_next(lo, cells)
        assert a["n_le"].tobytes() == b["n_le"].tobytes() and a["next"].tobytes() == b["next"].tobytes()


def test_hist_and_next_against_numpy(engine_lib, crafted):
    """The two primitives alone, every shift, against the numpy stand-ins of the host tests."""
    from test_coverage import numpy_primitives

    counts, tn5, depth, pops = crafted
    cells = pops["holes"]
    _, _, pd = population(counts, tn5, depth, cells)
    hist_fn, next_fn, _ = numpy_primitives([pd])
    rng = np.random.default_rng(8)
    for shift in (24, 16, 8, 0):
        pick = pd[rng.integers(0, pd.shape[0], pd.shape[1]), np.arange(pd.shape[1])].astype(np.uint64)
        prefix = (pick >> np.uint64(shift + 8)).astype(np.uint32)  # a prefix some cell of the column has
        got = engine_lib.position_depth_hist_rows(depth, shift, prefix, cells)["hist"]
        assert got.dtype == np.uint32
        np.testing.assert_array_equal(got, hist_fn(shift, prefix), err_msg=f"shift {shift}")
        assert shift == 24 or got.sum() > 0
    for v in (np.zeros(333, np.uint32), pd[0], np.full(333, 0xFFFFFFFF, np.uint32)):
        got = engine_lib.position_depth_next_rows(depth, v, cells)
        n_le, nxt = next_fn(np.asarray(v, np.uint32))
        np.testing.assert_array_equal(got["n_le"], n_le)
        np.testing.assert_array_equal(got["next"], nxt)


# ---- 2. the bounds -----------------------------------------------------------------------
def test_bounds(engine_lib):
    """2^16 cells of depth 2^24 - 1 are exact; 2^16 + 1 cells, or a depth or count of 2^24 in
    the sum passes, is MGP_E_INVALID; the histogram and `next` passes take a depth of 2^24."""
    from mgatk2_amd.exceptions import InvalidInputError

    eng = engine_lib
    top = (1 << 24) - 1
    counts = np.zeros((2, 70, 8), np.uint32)
    counts[0, 3, 2] = top
    counts[1, 3, 0:2] = (5, 7)
    depth = counts.astype(np.int64).sum(axis=2).astype(np.uint32)
    tn5 = np.zeros((2, 70, 2), np.uint32)
    tn5[0, 3] = (0xFFFFFFFF, 1)
    cells = np.zeros(1 << 16, np.int32)
    pos = eng.position_coverage_rows(counts, tn5, depth, cells)
    assert int(pos["s_depth2"][3]) == (1 << 16) * top * top and int(pos["s_depth"][3]) == (1 << 16) * top
    assert int(pos["s_tn5_fwd"][3]) == (1 << 16) * 0xFFFFFFFF and int(pos["n_tn5"][3]) == 1 << 16
    assert int(pos["tally"][3, 1]) == (1 << 16) * top == int(pos["s_fwd"][3]) and int(pos["max_depth"][3]) == top
    cell = eng.cell_coverage_rows(depth, cells)
    assert cell["s_depth2"].tolist() == [top * top] * (1 << 16) and cell["mid_hi"].max() == 0
    hist = eng.position_depth_hist_rows(depth, 16, np.zeros(70, np.uint32), cells)["hist"]
    assert int(hist[3, 255]) == 1 << 16 and int(hist[0, 0]) == 1 << 16
    many = np.zeros((1 << 16) + 1, np.int32)
    for call in (lambda: eng.position_coverage_rows(counts, tn5, depth, many), lambda: eng.cell_coverage_rows(depth, many),
                 lambda: eng.position_depth_hist_rows(depth, 0, None, many),
                 lambda: eng.position_depth_next_rows(depth, depth[0], many)):
        with pytest.raises(InvalidInputError, match="65536 cells"):
            call()
    over = counts.copy()
    over[0, 3, 2] = 1 << 24
    odepth = over.astype(np.int64).sum(axis=2).astype(np.uint32)
    with pytest.raises(InvalidInputError, match="2\\^24"):
        eng.position_coverage_rows(over, tn5, odepth)
    with pytest.raises(InvalidInputError, match="2\\^24"):
        eng.cell_coverage_rows(odepth)
    with pytest.raises(InvalidInputError, match="2\\^24"):  # a count alone (the depth below the bound)
        eng.position_coverage_rows(over, tn5, depth)
    assert eng.cell_coverage_rows(odepth, [1, 1])["s_depth"].tolist() == [12, 12]  # the other row is fine
    hist = eng.position_depth_hist_rows(odepth, 24)["hist"]
    assert int(hist[3, 1]) == 1 and int(hist[3, 0]) == 1 and int(hist[:, 0].sum()) == 2 * 70 - 1
    nxt = eng.position_depth_next_rows(odepth, np.full(70, 12, np.uint32))
    assert int(nxt["next"][3]) == 1 << 24 and int(nxt["n_le"][3]) == 1 and int(nxt["next"][0]) == 0xFFFFFFFF
    with pytest.raises(InvalidInputError, match="out of range"):
        eng.cell_coverage_rows(depth, [0, 2])
    with pytest.raises(InvalidInputError, match="shift"):
        eng.position_depth_hist_rows(depth, 4, np.zeros(70, np.uint32))


# ---- 3. the rows a run leaves in HBM ------------------------------------------------------
@pytest.fixture(scope="module")
def ctx_run(engine_lib):
    """One `run`-parameter context over synth_reads(CTX_SEED, 400_000, 130), as
    test_gpu_variants' ctx_run: the fetched u32 arrays and the device's coverage integers with
    the cells that did not pass as all-zero rows (the pipeline's default population)."""
    from mgatk2_amd.analysis.coverage import run_coverage
    from mgatk2_amd.engine import EngineConfig
    from mgatk2_amd.synth import synth_reads

    nc = 130
    soa = synth_reads(CTX_SEED, 400_000, nc)
    cfg = EngineConfig(n_cells=nc, **RUN)
    with engine_lib.Engine(cfg) as eng:
        eng.push(soa)
        eng.run()
        res = eng.fetch()
        pop = np.where(res.passed.astype(bool), np.arange(nc), -1)
        pop[5] = -1  # (and one listed as a zero row whatever it holds)
        got = device_all(eng, pop.astype(np.int32), nc)
        again = device_all(eng, pop.astype(np.int32), nc)
        full = run_coverage(eng)
        cut = run_coverage(eng, cells=pop, min_mean_coverage=float(np.median(res.depth.mean(axis=1))),
                           recompute_reference=True)
    return dict(soa=soa, cfg=cfg, res=res, pop=pop, got=got, again=again, nc=nc, full=full, cut=cut)


def test_context_rows(ctx_run):
    c = ctx_run
    res = c["res"]
    pc, pt, pd = population(res.counts, res.tn5, res.depth, c["pop"])
    assert (pd.sum(axis=1) == 0).any() and pd.max() > 10 and pt.sum() > 0
    check_against_oracle(*c["got"][:4], pc, pt, pd, "context")
    for a, b in zip(c["got"][:2], c["again"][:2]):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    assert c["got"][2].tobytes() == c["again"][2].tobytes() and c["got"][3].tobytes() == c["again"][3].tobytes()


def test_run_coverage_filters_and_recomputes(ctx_run):
    """run_coverage over the context: every cell at thresholds 0; at the median of the cells'
    mean depth (inclusive) the upper half is kept, the position tables and the recomputed
    reference are the kept cells'."""
    from mgatk2_amd.file_io.writers import ref_alleles

    c = ctx_run
    res, nc = c["res"], c["nc"]
    full = c["full"]
    assert full.kept.all() and full.cells.tolist() == list(range(nc)) and full.ref_alleles is None
    tabs = oracle_position_tables(res.counts, res.tn5, res.depth)
    top = int(res.depth.max())
    check_table(full.position, tabs[0], nc, top, "all cells")
    check_table(full.cell, oracle_cell_table(res.depth), res.depth.shape[1], top, "all cells")
    cut = c["cut"]
    pc, pt, pd = population(res.counts, res.tn5, res.depth, c["pop"])
    want_kept = pd.astype(np.float64).mean(axis=1) >= float(np.median(res.depth.mean(axis=1)))
    np.testing.assert_array_equal(cut.kept, want_kept)
    assert 0 < cut.kept.sum() < nc
    kc, kt, kd = pc[cut.kept], pt[cut.kept], pd[cut.kept]
    tabs = oracle_position_tables(kc, kt, kd)
    m = int(cut.kept.sum())
    check_table(cut.position, tabs[0], m, top, "kept")
    check_table(cut.strand, tabs[1], 4 * m, top, "kept")
    check_table(cut.transposition, tabs[2], m, top, "kept")
    tally = (kc[:, :, 0::2].astype(np.int64) + kc[:, :, 1::2]).sum(axis=0)
    np.testing.assert_array_equal(cut.tally, tally)
    assert cut.ref_alleles == ref_alleles(tally)


# ---- 4. a drained ("wide") window ---------------------------------------------------------
def test_wide_window_uses_the_exact_rows(engine_lib):
    """One cell 180k deep over positions [0, 110) (the construction of test_gpu_variants' wide
    test) beside four ordinary cells: the max, the medians, the sums of squares and the Tn5
    sums are made of the exact u32 values of its drained window, not of the 16-bit rows."""
    from mgatk2_amd.engine import EngineConfig
    from mgatk2_amd.synth import ReadSoA, concat_soa, synth_reads

    deep = synth_reads(91, 400_000, 1)
    deep.start[:] = np.sort(deep.start % 60).astype(np.int32)
    deep.payload.reshape(-1, 64)[:, 0:4] = deep.start.view(np.uint8).reshape(-1, 4)
    rest = synth_reads(92, 40_000, 4)
    rest.bc[rest.bc >= 0] += 1
    both = concat_soa([deep, rest])
    order = np.argsort(both.start, kind="stable")
    soa = ReadSoA(*[np.ascontiguousarray(getattr(both, k)[order]) for k in ("start", "bc", "tlen", "flag", "mapq",
                                                                            "span", "rec_off")], both.payload)
    cfg = EngineConfig(n_cells=5, min_baseq=0, min_mapq=0, dedup_mode="none", min_reads=0)
    pops = {"all": None, "listed": np.array([4, 0, -1, 2, 1, 3, 0], np.int32), "deep alone": np.array([0], np.int32),
            "deep twice": np.array([0, 0, 1], np.int32)}
    out = {}
    with engine_lib.Engine(cfg) as eng:
        eng.push(soa)
        eng.run()
        res = eng.fetch()
        assert eng.fetch_rows16().wide.any()
        for name, cells in pops.items():
            pc, pt, pd = population(res.counts, res.tn5, res.depth, cells)
            out[name] = (pc, pt, pd, device_all(eng, cells, pd.shape[0]))
    assert res.depth.max() > 65535
    for name, (pc, pt, pd, got) in out.items():
        check_against_oracle(*got[:4], pc, pt, pd, f"wide {name}")
        assert int(got[1]["max_depth"].max()) > 65535 and int(got[0]["max_depth"].max()) > 65535
    assert int(out["deep alone"][3][2].max()) > 65535  # a median above the 16-bit rows' ceiling
    assert int(out["deep twice"][3][2].max()) > 65535 and out["deep twice"][3][4]["hist"] == 3


# ---- 5. one population over two contexts --------------------------------------------------
def test_parts_merge_to_the_single_context_result(engine_lib, ctx_run):
    """The same reads in two contexts on device 0, split by cell (set_cell_range), through
    run_coverage: every table equal to the single context's, the device integers byte-equal."""
    from mgatk2_amd.analysis.coverage import _position_pass, run_coverage
    from mgatk2_amd.engine import EngineConfig

    c = ctx_run
    nc, soa, cut = c["nc"], c["soa"], 47
    engines = []
    try:
        for lo, hi in ((0, cut), (cut, nc)):
            eng = engine_lib.Engine(EngineConfig(**{**c["cfg"].__dict__, "n_cells": hi - lo}))
            engines.append((eng, lo, hi))
            eng.set_cell_range(lo, hi)
            eng.push(soa)
            eng.run()
        pos, lo_, hi_ = _position_pass(engines, c["pop"].astype(np.int64), c["res"].depth.shape[1])
        full = run_coverage(engines)
        part = run_coverage(engines, cells=c["pop"], min_mean_coverage=float(np.median(c["res"].depth.mean(axis=1))),
                            recompute_reference=True)
    finally:
        for eng, _, _ in engines:
            eng.close()
    for k in POS_INTS:
        assert pos[k].tobytes() == c["got"][1][k].tobytes(), k
    assert lo_.tobytes() == c["got"][2].tobytes() and hi_.tobytes() == c["got"][3].tobytes()
    for got, one in ((full, c["full"]), (part, c["cut"])):
        np.testing.assert_array_equal(got.kept, one.kept)
        np.testing.assert_array_equal(got.tally, one.tally)
        assert got.ref_alleles == one.ref_alleles
        for a, b in ((got.cell, one.cell), (got.position, one.position), (got.strand, one.strand),
                     (got.transposition, one.transposition)):
            assert list(a) == list(b)
            for k in a:  # made of the same integers: the same bytes
                assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


# ---- 6. the pipeline, from the user's side -------------------------------------------------
def _h5_rows(h5out):
    """The u32 rows an hdf5 run stores: counts [n, L, 8], tn5 [n, L, 2], depth [n, L], the
    barcodes and the run's reference alleles."""
    from mgatk2_amd import h5lite

    names = [f"{b}_{s}" for b in "ACGT" for s in ("fwd", "rev")]
    with h5lite.File(h5out / "output" / "counts.h5", "r") as f:
        counts = np.stack([f[k][...] for k in names], axis=-1).transpose(1, 0, 2).astype(np.uint32)
        tn5 = np.stack([f[k][...] for k in ("tn5_cuts_fwd", "tn5_cuts_rev")], axis=-1).transpose(1, 0, 2).astype(np.uint32)
        barcodes = [x.decode() for x in f["barcode"][...].tolist()]
    with h5lite.File(h5out / "output" / "metadata.h5", "r") as f:
        depth = f["coverage"][...].T.astype(np.uint32)
        ref = [x.decode() for x in f["reference"][...].tolist()]
    assert counts.max() < 65535 and depth.max() < 65535  # nothing saturates at this size
    return counts, tn5, depth, barcodes, ref


def _check_files(cdir, barcodes, kept, counts, tn5, depth):
    """coverage/'s four tables against the oracle: the cell table over every column of
    counts.h5, the position tables over the kept ones."""
    from mgatk2_amd.analysis import coverage as cov

    n, L = depth.shape
    top = int(depth.max())
    got = cov.read_table(cdir / "cell_coverage_stats.tsv")
    assert got.pop("barcode") == barcodes and got.pop("kept") == ["TRUE" if k else "FALSE" for k in kept]
    check_table({k: np.asarray(v) for k, v in got.items()}, oracle_cell_table(depth), L, top, "cell file")
    tabs = oracle_position_tables(counts[kept], tn5[kept], depth[kept])
    m = int(kept.sum())
    for name, want, terms in (("position_coverage_stats.tsv", tabs[0], m), ("strand_coverage_stats.tsv", tabs[1], 4 * m),
                              ("transposition_stats.tsv", tabs[2], m)):
        got = cov.read_table(cdir / name)
        check_table({k: np.asarray(v) for k, v in got.items()}, want, terms, top, name)


@pytest.mark.parametrize("fmt", ["hdf5", "txt"])
def test_pipeline_coverage(fmt, tmp_path, engine_lib, monkeypatch):
    """run_pipeline on the synth_run_h5 golden reads. With coverage_stats the four files equal
    the oracle on the run's own counts.h5 / metadata.h5 (the hdf5 run's) and every other output
    file is what a run without the flag writes. Then the vignette's sequence in one run: the
    filter thresholds are chosen here on the CPU oracle, from the plain run's counts.h5: the
    median of the cells' mean depth and the lower quartile of their breadth (both inclusive),
    which keeps about half of the cells whatever the seed; the assertions below check that at
    least one cell is dropped and at least one variant row remains. variant_stats.tsv then
    equals test_variants.oracle_table on the kept cells' columns with the reference of the kept
    cells' tallies, and the heteroplasmy matrix has exactly the kept barcodes."""
    import gzip

    from mgatk2_amd import h5lite
    from mgatk2_amd.analysis.coverage import read_table
    from mgatk2_amd.analysis.variants import read_variant_stats
    from mgatk2_amd.file_io.writers import ref_alleles

    g, plain = _pipeline(tmp_path, "plain", fmt, monkeypatch)
    h5out = plain if fmt == "hdf5" else _pipeline(tmp_path, "h5", "hdf5", monkeypatch)[1]
    counts, tn5, depth, barcodes, run_ref = _h5_rows(h5out)
    n = len(g.whitelist)
    assert barcodes == g.whitelist and depth.shape == (n, 16569)
    _, out = _pipeline(tmp_path, "cov", fmt, monkeypatch, coverage_stats=True)
    tables = ["coverage/cell_coverage_stats.tsv", "coverage/position_coverage_stats.tsv",
              "coverage/strand_coverage_stats.tsv", "coverage/transposition_stats.tsv"]
    assert [f for f in _files(out) if f.startswith("coverage")] == tables
    assert [f for f in _files(out) if not f.startswith("coverage")] == _files(plain)
    for rel in _files(plain):
        _same_file(out, plain, rel)
    _check_files(out / "coverage", barcodes, np.ones(n, bool), counts, tn5, depth)
    # the thresholds, on the oracle
    cell = oracle_cell_table(depth)
    a, b = float(np.median(cell["mean_coverage"])), float(np.quantile(cell["coverage_breadth"], 0.25))
    kept = (cell["mean_coverage"] >= a) & (cell["coverage_breadth"] >= b)
    assert 0 < kept.sum() < n
    kc, kd = counts[kept], depth[kept]
    ref = ref_alleles((kc[:, :, 0::2].astype(np.int64) + kc[:, :, 1::2]).sum(axis=0))
    want, _ = oracle_table(kc, kd, ref, 0, 0, -1.0, 0.0)
    assert len(want) > 0
    kw = dict(coverage_stats=True, cell_min_mean_coverage=a, cell_min_coverage_breadth=b, recompute_reference=True,
              call_variants=True, variant_min_cells=0, variant_min_strand_cor=-1.0, variant_min_vmr=0.0)
    _, out = _pipeline(tmp_path, "vignette", fmt, monkeypatch, **kw)
    matrix = "variants/allele_freq.h5" if fmt == "hdf5" else "variants/output.allele_freq.txt.gz"
    assert [f for f in _files(out) if f.startswith(("coverage", "variants"))] == \
        sorted(tables + ["coverage/reference_alleles.tsv", matrix, "variants/variant_stats.tsv"])
    for rel in _files(plain):
        _same_file(out, plain, rel)
    _check_files(out / "coverage", barcodes, kept, counts, tn5, depth)
    refs = read_table(out / "coverage" / "reference_alleles.tsv")
    assert refs["position"] == list(range(1, 16570)) and refs["reference"] == run_ref and refs["recomputed"] == ref
    got = read_variant_stats(out / "variants" / "variant_stats.tsv")
    keys = [(p - 1, "ACGT".index(nt[-1])) for p, nt in zip(got["position"], got["nucleotide"])]
    assert sorted(keys) == sorted(want)
    m = int(kept.sum())
    t = tol(m)
    for i, k in enumerate(keys):
        w = want[k]
        assert got["mean"][i] == w["mean"] and got["n_cells_detected"][i] == w["n_det"]
        assert got["n_cells_conf_detected"][i] == w["n_conf"]
        assert got["variant"][i] == f"{k[0] + 1}{ref[k[0]]}>{'ACGT'[k[1]]}"
        np.testing.assert_allclose(got["vmr"][i] * w["mean"], w["variance"], rtol=2 * t, atol=t)
        np.testing.assert_allclose(got["strand_correlation"][i], w["cor"], rtol=t, atol=t)
    af = oracle_allele_freq(kc, kd, keys)
    names = [bc for bc, k in zip(barcodes, kept) if k]
    if fmt == "hdf5":
        with h5lite.File(out / matrix, "r") as f:
            np.testing.assert_array_equal(f["allele_freq"][...], af)
            assert [x.decode() for x in f["barcode"][...].tolist()] == names
    else:
        lines = gzip.decompress((out / matrix).read_bytes()).decode().splitlines()
        assert lines == [f"{got['variant'][v]},{names[j]},{float(af[v, j])!r}" for v in range(len(keys))
                         for j in range(m) if af[v, j] > 0]
    # the filter without the tables, and the reference alone
    _, only = _pipeline(tmp_path, "filter", fmt, monkeypatch, **{**kw, "coverage_stats": False, "recompute_reference": False})
    assert [f for f in _files(only) if f.startswith("coverage")] == []
    assert sorted(read_variant_stats(only / "variants" / "variant_stats.tsv")["variant"]) == \
        sorted(f"{p + 1}{run_ref[p]}>{'ACGT'[q]}" for p, q in oracle_table(kc, kd, run_ref, 0, 0, -1.0, 0.0)[0])
    _, alone = _pipeline(tmp_path, "ref", fmt, monkeypatch, recompute_reference=True)
    assert [f for f in _files(alone) if f.startswith(("coverage", "variants"))] == ["coverage/reference_alleles.tsv"]


@pytest.mark.parametrize("stream", ["1", "0"])
def test_pipeline_coverage_sharded(stream, tmp_path, engine_lib, monkeypatch):
    """The cells over three contexts (one GPU), streamed and resident: the parts' integers
    merged on the host give the single context's coverage files byte for byte, and the same
    variants over the same kept cells."""
    import gzip

    from mgatk2_amd.analysis.coverage import read_table
    from mgatk2_amd.analysis.variants import read_variant_stats

    monkeypatch.setenv("MGP_STREAM_BATCH", "1500")
    _, probe = _pipeline(tmp_path, "probe", "txt", monkeypatch, coverage_stats=True)
    mean = read_table(probe / "coverage" / "cell_coverage_stats.tsv")["mean_coverage"]
    kw = dict(coverage_stats=True, cell_min_mean_coverage=float(np.median(mean)), recompute_reference=True,
              call_variants=True, variant_min_cells=0, variant_min_strand_cor=-1.0, variant_min_vmr=0.0)
    _, one = _pipeline(tmp_path, "one", "txt", monkeypatch, **kw)
    _, many = _pipeline(tmp_path, "many", "txt", monkeypatch, stream=stream, devices=[0, 0, 0], **kw)
    cov = [f for f in _files(one) if f.startswith("coverage")]
    assert len(cov) == 5 and cov == [f for f in _files(many) if f.startswith("coverage")]
    for rel in cov:
        assert (one / rel).read_bytes() == (many / rel).read_bytes(), rel
    kept = read_table(one / "coverage" / "cell_coverage_stats.tsv")["kept"]
    assert 0 < kept.count("TRUE") < len(kept)
    a = read_variant_stats(one / "variants" / "variant_stats.tsv")
    b = read_variant_stats(many / "variants" / "variant_stats.tsv")
    assert len(a["variant"]) > 0 and sorted(a["variant"]) == sorted(b["variant"])
    lines = [sorted(gzip.decompress((d / "variants" / "output.allele_freq.txt.gz").read_bytes()).decode().splitlines())
             for d in (one, many)]
    assert lines[0] == lines[1] and len(lines[0]) > 0
