"""Variant statistics and heteroplasmy on the device (mgp_variants.hip) against the numpy
oracle of tests/test_variants.py, which works from per-cell arrays (np.corrcoef, np.var).

Integer moments, n_cells_detected, n_cells_conf_detected, mean and the heteroplasmy matrix:
bit-equal. Variance and strand correlation: atol = rtol = 16 n 2^-53 (test_variants.tol, with
its derivation). vmr = variance / mean exactly. Two calls on the same rows: identical bytes.
"""

from __future__ import annotations

import gzip
import re

import numpy as np
import pytest

from golden_io import Golden
from test_variants import (INT_FIELDS, check_table, crafted_rows, oracle_allele_freq, oracle_dev2, oracle_moments,
                           oracle_table, population, ref_of, tol)

pytestmark = pytest.mark.gpu

RUN = dict(min_baseq=20, min_mapq=30, dedup_mode="alignment_and_fragment_length", min_reads=1)
# synth_reads(5, 400_000, 130): 20251019, the seed of the neighbouring tests, gives no variant
# with a confidently detecting cell at this depth (~5x); seeds 1..12 were tried on the CPU
# oracle, and 5 gives the most (7 variants with n_cells_conf_detected = 1)
CTX_SEED = 5


def check_moments(got, counts, depth, thr, what=""):
    """Pass 1's integer fields bit-equal to the oracle's; the fp64 sum of at most n terms in
    [0, 1] within n times the tolerance of one term."""
    want = oracle_moments(counts, depth, thr)
    n = counts.shape[0]
    for k in INT_FIELDS:
        assert got[k].dtype == np.uint64
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
    np.testing.assert_allclose(got["s_af"], want["s_af"], rtol=0, atol=max(1, n) * tol(n), err_msg=f"{what} s_af")


def device_table(calls, counts, depth, ref, n, thr, filters, cells=None):
    """moments -> mean -> dev2 -> table through `calls` = (moments, dev2) of a row source."""
    from mgatk2_amd.analysis.variants import mean_af, variant_table

    mom = calls[0](cells, thr)
    dev2 = calls[1](mean_af(mom, n), cells, thr)
    return mom, dev2, variant_table(mom, dev2, ref, n, *filters)


# ---- 1. crafted rows through the *_rows forms --------------------------------------------
@pytest.fixture(scope="module")
def crafted():
    counts, depth = crafted_rows()
    rng = np.random.default_rng(99)
    subset = rng.permutation(40)[:23]  # a shuffled proper subset
    holes = np.concatenate([rng.permutation(40)[:17], [-1, -1, -1]])  # and one with all-zero rows
    rng.shuffle(holes)
    return counts, depth, {"all": None, "subset": subset, "holes": holes}


@pytest.mark.parametrize("pop", ["all", "subset", "holes"])
@pytest.mark.parametrize("thr", [0, 1, 10])
def test_crafted_rows(engine_lib, crafted, thr, pop):
    """One variant in one cell only (m = 1), constant f (vf = 0), perfectly correlated and
    anti-correlated strands, cov = 0 cells, an all-zero position (ref "N"), a covered "N"
    position, counts above 65,535, f >= 2 with r = 1, stabilisation thresholds 0, 1, 10, and
    shuffled proper subsets of the rows as the population (one with all-zero rows)."""
    eng = engine_lib
    counts, depth, pops = crafted
    cells = pops[pop]
    pc, pd = population(counts, depth, cells)
    n = pc.shape[0]
    ref = ref_of(pc)
    ref[22] = "N"
    calls = (lambda c, t: eng.variant_moments_rows(counts, depth, c, t),
             lambda mu, c, t: eng.variant_dev2_rows(counts, depth, mu, c, t))
    filters = (0, -1.0, 0.0)
    mom, dev2, table = device_table(calls, counts, depth, ref, n, thr, filters, cells)
    check_moments(mom, pc, pd, thr, f"thr {thr} {pop}")
    assert (mom["sff"].max() > 2 ** 40 or pop != "all") and (mom["n_low"] > 0).any() == (thr > 0)
    want, _ = oracle_table(pc, pd, ref, thr, *filters)
    assert len(want) > 100
    check_table(table, want, n, f"thr {thr} {pop}")
    # R's defaults and mgatk-like thresholds: the drop rules on the device's numbers
    from mgatk2_amd.analysis.variants import variant_table

    for f in ((0, 0, 0), (1, 0.3, 0.005)):
        w, _ = oracle_table(pc, pd, ref, thr, *f)
        check_table(variant_table(mom, dev2, ref, n, *f), w, n, f"thr {thr} {pop} filters {f}")
    # the matrix, bit-equal, and a second call's bytes
    pairs = table.pairs()[:50] + [(20, 0), (9, int(np.argmax(mom["s_total"][9])))]
    for min_cov in (1, 12):
        af = eng.allele_freq_rows(counts, depth, pairs, cells, min_cov)
        assert af.dtype == np.float64 and af.shape == (len(pairs), n)
        np.testing.assert_array_equal(af, oracle_allele_freq(pc, pd, pairs, min_cov))
    again = calls[0](cells, thr)
    for k in mom:
        assert mom[k].tobytes() == again[k].tobytes(), k
    assert calls[1](np.ascontiguousarray(dev2 * 0 + 0.25), cells, thr).tobytes() == \
        calls[1](np.full_like(dev2, 0.25), cells, thr).tobytes()


def test_overflow_bound(engine_lib):
    """The documented bound: at most 2^16 cells per call, every fwd / rev count below 2^24.
    At the bound the u64 moments are exact; one past it, either way, is MGP_E_INVALID."""
    from mgatk2_amd.exceptions import InvalidInputError

    eng = engine_lib
    top = (1 << 24) - 1
    counts = np.zeros((2, 8, 8), np.uint32)
    counts[0, 3, 2:4] = top  # C fwd and rev at position 3
    counts[1, 3, 0:2] = (5, 7)
    depth = counts.astype(np.int64).sum(axis=2).astype(np.uint32)
    cells = np.zeros(1 << 16, np.int32)
    mom = eng.variant_moments_rows(counts, depth, cells)
    assert int(mom["sff"][3, 1]) == (1 << 16) * top * top == int(mom["srr"][3, 1]) == int(mom["sfr"][3, 1])
    assert int(mom["sf"][3, 1]) == (1 << 16) * top and int(mom["m"][3, 1]) == 1 << 16
    assert int(mom["s_cov"][3]) == (1 << 16) * 2 * top and mom["s_af"][3, 1] == float(1 << 16)
    with pytest.raises(InvalidInputError, match="65536 cells"):
        eng.variant_moments_rows(counts, depth, np.zeros((1 << 16) + 1, np.int32))
    with pytest.raises(InvalidInputError, match="65536 cells"):
        eng.variant_dev2_rows(counts, depth, np.zeros((8, 4)), np.zeros((1 << 16) + 1, np.int32))
    over = counts.copy()
    over[0, 3, 3] = 1 << 24
    with pytest.raises(InvalidInputError, match="2\\^24"):
        eng.variant_moments_rows(over, over.astype(np.int64).sum(axis=2).astype(np.uint32))
    check_moments(eng.variant_moments_rows(over, depth, [1, 1]), *population(over, depth, [1, 1]), 0)
    with pytest.raises(InvalidInputError, match="out of range"):
        eng.variant_moments_rows(counts, depth, [0, 2])
    with pytest.raises(InvalidInputError, match="out of range"):
        eng.allele_freq_rows(counts, depth, [(8, 0)])
    with pytest.raises(InvalidInputError, match="out of range"):
        eng.allele_freq_rows(counts, depth, [(0, 4)])


# ---- 2. the rows a run leaves in HBM ------------------------------------------------------
@pytest.fixture(scope="module")
def ctx_run(engine_lib):
    """One `run`-parameter context over synth_reads(CTX_SEED, 400_000, 130): the fetched u32
    arrays, and the device's moments, dev2, table and matrix of the resident rows."""
    from mgatk2_amd.analysis.variants import mean_af, variant_table
    from mgatk2_amd.engine import EngineConfig
    from mgatk2_amd.file_io.writers import ref_alleles
    from mgatk2_amd.synth import synth_reads

    nc = 130
    soa = synth_reads(CTX_SEED, 400_000, nc)
    cfg = EngineConfig(n_cells=nc, **RUN)
    with engine_lib.Engine(cfg) as eng:
        eng.push(soa)
        eng.run()
        res = eng.fetch()
        ref = ref_alleles(res.ref_tally)
        mom = eng.variant_moments()
        dev2 = eng.variant_dev2(mean_af(mom, nc))
        table = variant_table(mom, dev2, ref, nc, 0, -1.0, 0.0)
        af = eng.allele_freq(table.pairs())
        again = (eng.variant_moments(), eng.variant_dev2(mean_af(mom, nc)), eng.allele_freq(table.pairs()))
        stab = eng.variant_moments(None, 10)
        stab_dev2 = eng.variant_dev2(mean_af(stab, nc), None, 10)
    return dict(soa=soa, cfg=cfg, res=res, ref=ref, mom=mom, dev2=dev2, table=table, af=af, again=again, stab=stab,
                stab_dev2=stab_dev2, nc=nc)


def test_context_rows(ctx_run):
    from mgatk2_amd.analysis.variants import variant_table

    c = ctx_run
    res, nc = c["res"], c["nc"]
    check_moments(c["mom"], res.counts, res.depth, 0, "context")
    want, _ = oracle_table(res.counts, res.depth, c["ref"], 0, 0, -1.0, 0.0)
    check_table(c["table"], want, nc, "context")
    assert int(c["table"].n_cells_conf_detected.max()) >= 1  # not vacuous: a confidently detected variant
    np.testing.assert_array_equal(c["af"], oracle_allele_freq(res.counts, res.depth, c["table"].pairs()))
    for a, b in zip((c["mom"], c["dev2"], c["af"]), c["again"]):  # identical bytes on a second call
        for x, y in zip(a.values() if isinstance(a, dict) else [a], b.values() if isinstance(b, dict) else [b]):
            assert x.tobytes() == y.tobytes()
    # variance stabilisation at the default threshold
    check_moments(c["stab"], res.counts, res.depth, 10, "context thr 10")
    want, _ = oracle_table(res.counts, res.depth, c["ref"], 10, 1, -1.0, 0.0)
    assert len(want) > 0
    check_table(variant_table(c["stab"], c["stab_dev2"], c["ref"], nc, 1, -1.0, 0.0), want, nc, "context thr 10")


# ---- 3. a drained ("wide") window ---------------------------------------------------------
def test_wide_window_uses_the_exact_rows(engine_lib):
    """One cell 180k deep over positions [0, 110) (the construction of test_gpu_h5tiles'
    wide-window test) beside four ordinary cells: the moments and the matrix are made of the
    exact u32 values of its drained window, not of the 16-bit rows' 65,535."""
    from mgatk2_amd.engine import EngineConfig
    from mgatk2_amd.file_io.writers import ref_alleles
    from mgatk2_amd.synth import ReadSoA, concat_soa, synth_reads

    deep = synth_reads(91, 400_000, 1)
    deep.start[:] = np.sort(deep.start % 60).astype(np.int32)
    deep.payload.reshape(-1, 64)[:, 0:4] = deep.start.view(np.uint8).reshape(-1, 4)
    rest = synth_reads(92, 40_000, 4)
    rest.bc[rest.bc >= 0] += 1
    both = concat_soa([deep, rest])
    order = np.argsort(both.start, kind="stable")  # coordinate order; the records stay where they are
    soa = ReadSoA(*[np.ascontiguousarray(getattr(both, k)[order]) for k in ("start", "bc", "tlen", "flag", "mapq",
                                                                            "span", "rec_off")], both.payload)
    cfg = EngineConfig(n_cells=5, min_baseq=0, min_mapq=0, dedup_mode="none", min_reads=0)
    pop = np.array([4, 0, -1, 2, 1, 3], np.int32)
    with engine_lib.Engine(cfg) as eng:
        eng.push(soa)
        eng.run()
        res = eng.fetch()
        assert eng.fetch_rows16().wide.any()
        ref = ref_alleles(res.ref_tally)
        calls = (lambda c, t: eng.variant_moments(c, t), lambda mu, c, t: eng.variant_dev2(mu, c, t))
        out = {}
        for name, cells in (("all", None), ("listed", pop)):
            pc, pd = population(res.counts, res.depth, cells)
            mom, dev2, table = device_table(calls, res.counts, res.depth, ref, pc.shape[0], 0, (0, -1.0, 0.0), cells)
            out[name] = (pc, pd, mom, table, eng.allele_freq(table.pairs(), cells))
    assert res.depth.max() > 65535
    for name, (pc, pd, mom, table, af) in out.items():
        check_moments(mom, pc, pd, 0, f"wide {name}")
        assert int(mom["s_cov"].max()) > 65535 + 4 * 1000  # more than a saturated cell and the others
        want, _ = oracle_table(pc, pd, ref, 0, 0, -1.0, 0.0)
        assert any(p < 110 for p, _ in want)
        check_table(table, want, pc.shape[0], f"wide {name}")
        np.testing.assert_array_equal(af, oracle_allele_freq(pc, pd, table.pairs()))


# ---- 4. one population over two contexts --------------------------------------------------
def test_parts_merge_to_the_single_context_result(engine_lib, ctx_run):
    """The same reads in two contexts on device 0, split by cell (set_cell_range), through
    run_variants: integer columns and the matrix bit-equal to the single context's, the
    floating-point columns within the tolerance."""
    from mgatk2_amd.analysis.variants import identify_variants, run_variants
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
        vr = run_variants(engines, c["ref"], min_strand_cor=-1.0)
        own_ref = identify_variants(engines, min_strand_cor=-1.0)  # the reference alleles from the parts' tallies
        one = identify_variants(engines[0][0], c["ref"], min_strand_cor=-1.0)  # a single Engine as the source
    finally:
        for eng, _, _ in engines:
            eng.close()
    for k in INT_FIELDS:
        np.testing.assert_array_equal(vr.moments[k], c["mom"][k], err_msg=k)
    t = tol(nc)
    np.testing.assert_allclose(vr.dev2, c["dev2"], rtol=t, atol=(nc - 1) * t)  # (the variance is dev2 / (n - 1))
    # (rows whose vmr differ by less than the rounding may change places: compared by variant)
    single = c["table"]
    assert sorted(vr.table.pairs()) == sorted(single.pairs()) == sorted(own_ref.pairs()) and vr.n == nc
    at = {k: i for i, k in enumerate(single.pairs())}
    perm = np.array([at[k] for k in vr.table.pairs()], np.int64)
    for k in ("position", "base", "mean", "n_cells_detected", "n_cells_conf_detected", "strand_correlation"):
        np.testing.assert_array_equal(getattr(vr.table, k), getattr(single, k)[perm], err_msg=k)
    np.testing.assert_allclose(vr.table.variance, single.variance[perm], rtol=t, atol=t)
    np.testing.assert_array_equal(vr.table.vmr, vr.table.variance / vr.table.mean)
    assert np.all(np.diff(vr.table.vmr) <= 0)
    np.testing.assert_array_equal(vr.allele_freq, c["af"][perm])
    want, _ = oracle_table(c["res"].counts[:cut], c["res"].depth[:cut], c["ref"], 0, 0, -1.0, 0.0)
    check_table(one, want, cut, "first part alone")


# ---- 5. the pipeline, from the user's side -------------------------------------------------
def _pipeline(tmp_path, name, fmt, monkeypatch, stream="1", **kw):
    from mgatk2_amd.bam import soa_to_bam
    from mgatk2_amd.pipeline import run_pipeline

    monkeypatch.setenv("MGP_STREAM", stream)
    g = Golden("synth_run_h5")
    p = g.params
    d = tmp_path / name
    d.mkdir()
    soa_to_bam(d / "x.bam", g.soa, g.whitelist)
    (d / "barcodes.tsv").write_text("".join(b + "\n" for b in g.whitelist))
    run_pipeline(str(d / "x.bam"), str(d / "barcodes.tsv"), str(d / "out"), min_baseq=p["min_baseq"],
                 min_mapq=p["min_mapq"], min_reads_per_cell=p["min_reads_per_cell"],
                 max_strand_bias=p["max_strand_bias"], skip_deduplication=p["skip_deduplication"],
                 use_fragment_length_dedup=p["use_fragment_length_dedup"], output_format=fmt, **kw)
    return g, d / "out"


def _files(out):
    return sorted(str(p.relative_to(out)) for p in out.rglob("*") if p.is_file())


def _h5_tree(path):
    from mgatk2_amd import h5lite

    def walk(g, pre=""):
        for k in g.keys():
            x = g[k]
            if hasattr(x, "keys"):
                yield from walk(x, pre + k + "/")
            else:
                a = x[...]
                yield pre + k, a.dtype.str, a.shape, a.tobytes()

    with h5lite.File(path, "r") as f:
        return list(walk(f))


def _same_file(a, b, rel):
    """Byte-identical, but for what carries the wall clock or the run's directory: the
    summary's run_date / paths, the report's date, HDF5's object times (there: every
    dataset's type, shape and bytes)."""
    if rel.endswith(".h5"):
        assert _h5_tree(a / rel) == _h5_tree(b / rel), rel
        return
    x, y = (a / rel).read_bytes(), (b / rel).read_bytes()
    if rel.endswith("summary.txt") or rel.endswith(".html"):
        def norm(t, root):
            t = t.decode().replace(str(root.parent), "RUN")
            t = re.sub(r"run_date: .*", "run_date:", t)
            return re.sub(r"<strong>Date:</strong> [^<]*", "Date", t)
        assert norm(x, a) == norm(y, b), rel
        return
    assert x == y, rel


@pytest.mark.parametrize("fmt", ["hdf5", "txt"])
def test_pipeline_variants(fmt, tmp_path, engine_lib, monkeypatch):
    """run_pipeline(call_variants=True) on the synth_run_h5 golden reads, thresholds lowered
    to R's defaults with min_strand_cor = -1 so the table is not empty at that depth: the tsv and the matrix equal
    the oracle applied to the counts of the run's own counts.h5 / metadata.h5 (the hdf5 run's;
    nothing saturates at this size), every other output file is what a run without the flag
    writes, the streamed and the resident path write the same files, and a run without the
    flag makes no variants/ directory."""
    from mgatk2_amd import h5lite
    from mgatk2_amd.analysis.variants import read_variant_stats

    kw = dict(call_variants=True, variant_min_cells=0, variant_min_strand_cor=-1.0, variant_min_vmr=0.0)
    g, out = _pipeline(tmp_path, "streamed", fmt, monkeypatch, **kw)
    _, resident = _pipeline(tmp_path, "resident", fmt, monkeypatch, stream="0", **kw)
    _, plain = _pipeline(tmp_path, "plain", fmt, monkeypatch)
    assert not (plain / "variants").exists()
    matrix = "variants/allele_freq.h5" if fmt == "hdf5" else "variants/output.allele_freq.txt.gz"
    assert [f for f in _files(out) if f.startswith("variants")] == sorted([matrix, "variants/variant_stats.tsv"])
    assert [f for f in _files(out) if not f.startswith("variants")] == _files(plain)
    for rel in _files(plain):
        _same_file(out, plain, rel)
    assert _files(resident) == _files(out)
    for rel in _files(out):
        _same_file(out, resident, rel)
    # the oracle on the counts an hdf5 run of the same reads stores
    h5out = out if fmt == "hdf5" else _pipeline(tmp_path, "h5", "hdf5", monkeypatch)[1]
    names = [f"{b}_{s}" for b in "ACGT" for s in ("fwd", "rev")]
    with h5lite.File(h5out / "output" / "counts.h5", "r") as f:
        counts = np.stack([f[k][...] for k in names], axis=-1).transpose(1, 0, 2).astype(np.uint32)
        barcodes = [x.decode() for x in f["barcode"][...].tolist()]
    with h5lite.File(h5out / "output" / "metadata.h5", "r") as f:
        depth = f["coverage"][...].T.astype(np.uint32)
        ref = [x.decode() for x in f["reference"][...].tolist()]
    n = len(g.whitelist)
    assert counts.shape == (n, 16569, 8) and depth.shape == (n, 16569) and counts.max() < 65535 and barcodes == g.whitelist
    want, _ = oracle_table(counts, depth, ref, 0, 0, -1.0, 0.0)
    assert len(want) > 0
    got = read_variant_stats(out / "variants" / "variant_stats.tsv")
    keys = [(p - 1, "ACGT".index(nt[-1])) for p, nt in zip(got["position"], got["nucleotide"])]
    assert sorted(keys) == sorted(want)
    t = tol(n)
    for i, k in enumerate(keys):
        w = want[k]
        assert got["mean"][i] == w["mean"] and got["n_cells_detected"][i] == w["n_det"]
        assert got["n_cells_conf_detected"][i] == w["n_conf"]
        assert got["variant"][i] == f"{k[0] + 1}{ref[k[0]]}>{'ACGT'[k[1]]}" and got["nucleotide"][i] == got["variant"][i][-3:]
        # vmr = variance / mean: the variance's tolerance over the exact mean
        np.testing.assert_allclose(got["vmr"][i] * w["mean"], w["variance"], rtol=2 * t, atol=t)
        np.testing.assert_allclose(got["strand_correlation"][i], w["cor"], rtol=t, atol=t)
    order = [(-v, p, "ACGT".index(nt[-1])) for v, p, nt in zip(got["vmr"], got["position"], got["nucleotide"])]
    assert order == sorted(order)
    af = oracle_allele_freq(counts, depth, keys)
    if fmt == "hdf5":
        with h5lite.File(out / matrix, "r") as f:
            np.testing.assert_array_equal(f["allele_freq"][...], af)
            assert [x.decode() for x in f["variant"][...].tolist()] == [v.replace(">", "-") for v in got["variant"]]
            assert [x.decode() for x in f["barcode"][...].tolist()] == g.whitelist
    else:
        lines = gzip.decompress((out / matrix).read_bytes()).decode().splitlines()
        assert lines == [f"{got['variant'][v]},{g.whitelist[j]},{float(af[v, j])!r}" for v in range(len(keys))
                         for j in range(n) if af[v, j] > 0]


@pytest.mark.parametrize("stream", ["1", "0"])
def test_pipeline_variants_sharded(stream, tmp_path, engine_lib, monkeypatch):
    """The cells over three contexts (one GPU), streamed and resident: each part's pass 1,
    the host merge, pass 2 and each part's columns of the matrix give the single context's
    files: the same variants, exact columns and matrix values equal, vmr within the tolerance."""
    from mgatk2_amd.analysis.variants import read_variant_stats

    monkeypatch.setenv("MGP_STREAM_BATCH", "1500")
    kw = dict(call_variants=True, variant_min_cells=0, variant_min_strand_cor=-1.0, variant_min_vmr=0.0)
    g, one = _pipeline(tmp_path, "one", "txt", monkeypatch, **kw)
    _, many = _pipeline(tmp_path, "many", "txt", monkeypatch, stream=stream, devices=[0, 0, 0], **kw)
    a = read_variant_stats(one / "variants" / "variant_stats.tsv")
    b = read_variant_stats(many / "variants" / "variant_stats.tsv")
    assert len(a["variant"]) > 0 and sorted(a["variant"]) == sorted(b["variant"])
    at = {v: i for i, v in enumerate(a["variant"])}
    n, t = len(g.whitelist), tol(len(g.whitelist))
    for j, v in enumerate(b["variant"]):
        i = at[v]
        for k in ("position", "nucleotide", "mean", "n_cells_detected", "n_cells_conf_detected", "strand_correlation"):
            assert a[k][i] == b[k][j], (v, k)
        np.testing.assert_allclose(b["vmr"][j] * b["mean"][j], a["vmr"][i] * a["mean"][i], rtol=2 * t, atol=t)
    assert b["vmr"] == sorted(b["vmr"], reverse=True) and n >= 2
    lines = [sorted(gzip.decompress((d / "variants" / "output.allele_freq.txt.gz").read_bytes()).decode().splitlines())
             for d in (one, many)]
    assert lines[0] == lines[1] and len(lines[0]) > 0
