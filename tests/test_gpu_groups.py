"""The grouped sweep on the device (mgp_groups.hip) against the numpy oracle of tests/test_groups.py, bit for
bit: crafted rows through the detached form at item sizes around the sweep's unroll and chunk, the bounds,
the rows a run leaves in HBM, a drained window, two contexts split by cell, and the pipeline's groups/
files from the user's side."""

from __future__ import annotations

import numpy as np
import pytest

from golden_io import Golden
from test_groups import FIELDS, oracle_group_moments, oracle_totals, same
from test_gpu_variants import CTX_SEED, RUN, _files, _pipeline, _same_file
from test_variants import crafted_rows, population

pytestmark = pytest.mark.gpu


# ---- 1. crafted rows through the detached form -----------------------------------------------------
@pytest.fixture(scope="module")
def crafted():
    """crafted_rows(40, 300): two position blocks, the second partial, counts above 65,535. A population of
    700 entries (the 40 rows repeated and shuffled, three -1 rows inside groups) in groups of 1, 2, 3, 5,
    129, 257 and 300 cells (around the sweep's unroll of 4 and chunk of 128), one empty group (number 3) and
    three unlabelled entries, the labels interleaved. The oracle is computed once."""
    counts, depth = crafted_rows(40, 300)
    rng = np.random.default_rng(17)
    sizes = {0: 1, 1: 2, 2: 3, 3: 0, 4: 5, 5: 129, 6: 257, 7: 300, -1: 3}
    group = np.concatenate([np.full(m, g, np.int32) for g, m in sizes.items()])
    assert group.size == 700
    rng.shuffle(group)
    cells = rng.integers(0, 40, 700).astype(np.int32)
    for g in (2, 5, 7):  # all-zero rows inside groups
        cells[np.flatnonzero(group == g)[1]] = -1
    return dict(counts=counts, depth=depth, cells=cells, group=group, n_groups=8,
                want=oracle_group_moments(counts, depth, cells, group, 8))


@pytest.mark.parametrize("max_item_cells", [0, 1, 4, 129])
def test_crafted_rows(engine_lib, crafted, max_item_cells):
    c = crafted
    got = engine_lib.group_moments_rows(c["counts"], c["depth"], c["group"], c["n_groups"], c["cells"], max_item_cells)
    same(got, c["want"], f"item cells {max_item_cells}")
    assert int(got["fwd"].max()) > 65535 and not got["cov"][3].any()
    again = engine_lib.group_moments_rows(c["counts"], c["depth"], c["group"], c["n_groups"], c["cells"], max_item_cells)
    for k in FIELDS:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_groups_add_up_to_the_variant_moments(engine_lib, crafted):
    c = crafted
    got = engine_lib.group_moments_rows(c["counts"], c["depth"], c["group"], c["n_groups"], c["cells"])
    mom = engine_lib.variant_moments_rows(c["counts"], c["depth"], c["cells"][c["group"] >= 0])
    np.testing.assert_array_equal((got["fwd"] + got["rev"]).sum(0), mom["s_total"])
    np.testing.assert_array_equal(got["n_det"].sum(0, dtype=np.uint64), mom["n_det"])
    np.testing.assert_array_equal(got["n_conf"].sum(0, dtype=np.uint64), mom["n_conf"])
    np.testing.assert_array_equal(got["cov"].sum(0), mom["s_cov"])


# ---- 2. the bounds ---------------------------------------------------------------------------------
def test_bounds(engine_lib):
    """At most 2^16 cells per call and every count below 2^24: exact at the bound, refused past it."""
    from mgatk2_amd.exceptions import InvalidInputError

    eng = engine_lib
    top = (1 << 24) - 1
    counts = np.zeros((2, 8, 8), np.uint32)
    counts[0, 3, 2:4] = top
    counts[1, 3, 0:2] = (5, 7)
    depth = counts.astype(np.int64).sum(axis=2).astype(np.uint32)
    n = 1 << 16
    got = eng.group_moments_rows(counts, depth, np.ones(n, np.int32), 2, np.zeros(n, np.int32))
    assert int(got["fwd"][1, 3, 1]) == n * top == int(got["rev"][1, 3, 1]) and int(got["cov"][1, 3]) == 2 * n * top
    assert int(got["n_det"][1, 3, 1]) == n == int(got["n_conf"][1, 3, 1]) and not got["fwd"][0].any()
    with pytest.raises(InvalidInputError, match="65536 cells"):
        eng.group_moments_rows(counts, depth, np.zeros(n + 1, np.int32), 2, np.zeros(n + 1, np.int32))
    over = counts.copy()
    over[0, 3, 3] = 1 << 24
    with pytest.raises(InvalidInputError, match="2\\^24"):
        eng.group_moments_rows(over, over.astype(np.int64).sum(axis=2).astype(np.uint32), [0, 1], 2)
    same(eng.group_moments_rows(over, depth, [-1, 0], 2), oracle_group_moments(over, depth, None, [-1, 0], 2),
         "the large count in no group")  # (an unlabelled cell is never read)
    with pytest.raises(InvalidInputError, match="out of range"):
        eng.group_moments_rows(counts, depth, [0, 2], 2)
    with pytest.raises(InvalidInputError, match="out of range"):
        eng.group_moments_rows(counts, depth, [0, 1], 2, [0, 2])
    with pytest.raises(InvalidInputError, match="n_groups"):
        eng.group_moments_rows(counts, depth, [-1, -1], 0)


def test_more_than_256_groups(engine_lib):
    rng = np.random.default_rng(23)
    counts = rng.integers(0, 50, (64, 8, 8)).astype(np.uint32)
    depth = counts.sum(axis=2).astype(np.uint32)
    cells = rng.integers(-1, 64, 1000).astype(np.int32)
    group = rng.integers(-1, 300, 1000).astype(np.int32)
    same(engine_lib.group_moments_rows(counts, depth, group, 300, cells),
         oracle_group_moments(counts, depth, cells, group, 300), "300 groups")


# ---- 3. the rows a run leaves in HBM ---------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(engine_lib):
    """The context of test_gpu_variants.ctx_run, left open: its fetched u32 arrays and the engine."""
    from mgatk2_amd.engine import EngineConfig
    from mgatk2_amd.synth import synth_reads

    nc = 130
    soa = synth_reads(CTX_SEED, 400_000, nc)
    cfg = EngineConfig(n_cells=nc, **RUN)
    rng = np.random.default_rng(29)
    cells = np.concatenate([rng.permutation(nc), [-1, -1, 12]]).astype(np.int32)
    rng.shuffle(cells)
    group = rng.integers(-1, 7, cells.size).astype(np.int32)
    with engine_lib.Engine(cfg) as eng:
        eng.push(soa)
        eng.run()
        res = eng.fetch()
        yield dict(eng=eng, res=res, soa=soa, cfg=cfg, nc=nc, cells=cells, group=group,
                   want=oracle_group_moments(res.counts, res.depth, cells, group, 7))


def test_context_rows(ctx):
    got = ctx["eng"].group_moments(ctx["group"], 7, ctx["cells"])
    same(got, ctx["want"], "context")
    assert int(got["n_conf"].max()) >= 1 and (ctx["group"] < 0).any() and (ctx["cells"] < 0).any()
    everyone = ctx["eng"].group_moments(np.arange(ctx["nc"]) % 3, 3)  # no cell list: every cell of the context
    same(everyone, oracle_group_moments(ctx["res"].counts, ctx["res"].depth, None, np.arange(ctx["nc"]) % 3, 3), "all")


# ---- 4. a drained window -----------------------------------------------------------------------------
def test_wide_window_uses_the_exact_rows(engine_lib):
    """The five cells of test_gpu_variants' wide-window test (cell 0 is 180k deep over positions [0, 110)):
    the deep cell and one other in one group, the rest in another. The sums are made of the exact u32 rows
    of the drained window, not of the 16-bit rows' 65,535."""
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
    group = np.array([0, 1, 1, 0, 1], np.int32)
    with engine_lib.Engine(cfg) as eng:
        eng.push(soa)
        eng.run()
        res = eng.fetch()
        assert eng.fetch_rows16().wide.any()
        got = eng.group_moments(group, 2)
    assert res.depth.max() > 65535
    same(got, oracle_group_moments(res.counts, res.depth, None, group, 2), "wide")
    assert int(got["cov"][0].max()) > 65535 + 4 * 1000


# ---- 5. two contexts split by cell -------------------------------------------------------------------
def test_parts_merge_to_the_single_context_result(engine_lib, ctx):
    from mgatk2_amd.analysis.groups import run_groups
    from mgatk2_amd.engine import EngineConfig

    nc, soa, cut = ctx["nc"], ctx["soa"], 47
    cells, group = ctx["cells"].astype(np.int64), ctx["group"]
    engines = []
    try:
        for lo, hi in ((0, cut), (cut, nc)):
            eng = engine_lib.Engine(EngineConfig(**{**ctx["cfg"].__dict__, "n_cells": hi - lo}))
            engines.append((eng, lo, hi))
            eng.set_cell_range(lo, hi)
            eng.push(soa)
            eng.run()
        two = run_groups(engines, group, 7, cells)
    finally:
        for eng, _, _ in engines:
            eng.close()
    one = run_groups(ctx["eng"], group, 7, cells)
    same(one[0], ctx["want"], "one context")
    for a, b in zip(one, two):
        for k in FIELDS:
            assert a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape, k
    np.testing.assert_array_equal(one[1]["cov"], oracle_totals(ctx["res"].counts, ctx["res"].depth, cells)["cov"])


# ---- 6. the pipeline, from the user's side -------------------------------------------------------------
VARIANTS = dict(call_variants=True, variant_min_cells=0, variant_min_strand_cor=-1.0, variant_min_vmr=0.0)
THRESHOLDS = dict(group_min_cells=0, group_min_af=0.0)
GROUP_NAMES = ["1", "2", "10"]


def _label_of(i: int) -> int:
    """The group number of whitelist entry i (-1: not in the groups file): three groups of unequal size."""
    return -1 if i % 7 == 3 else (0 if i % 5 < 3 else 1 if i % 5 == 3 else 2)


def _groups_file(tmp_path, whitelist):
    path = tmp_path / "cell_groups.tsv"
    if not path.exists():
        lines = [f"{b}\t{GROUP_NAMES[_label_of(i)]}\n" for i, b in enumerate(whitelist) if _label_of(i) >= 0]
        path.write_text("barcode\tgroup\n" + "".join(lines) + "NOT-A-CELL\t2\n")
    return str(path)


def _run_counts(h5out):
    """(counts [n, L, 8], depth [n, L], ref, barcodes) of an hdf5 run's own count files."""
    from mgatk2_amd import h5lite

    names = [f"{b}_{s}" for b in "ACGT" for s in ("fwd", "rev")]
    with h5lite.File(h5out / "output" / "counts.h5", "r") as f:
        counts = np.stack([f[k][...] for k in names], axis=-1).transpose(1, 0, 2).astype(np.uint32)
        barcodes = [x.decode() for x in f["barcode"][...].tolist()]
    with h5lite.File(h5out / "output" / "metadata.h5", "r") as f:
        depth = f["coverage"][...].T.astype(np.uint32)
        ref = [x.decode() for x in f["reference"][...].tolist()]
    assert counts.max() < 65535
    return counts, depth, ref, barcodes


def _check_group_files(gdir, counts, depth, ref, labels, called_pairs=None, cells=None):
    """groups/ against the oracle on the count files' rows; labels: of each row (of each entry of `cells`)."""
    from mgatk2_amd import h5lite
    from mgatk2_amd.analysis.groups import MARKER_COLUMNS, read_tsv

    labels = np.asarray(labels)
    G, L = len(GROUP_NAMES), depth.shape[1]
    want = oracle_group_moments(counts, depth, cells, labels, G)
    g = read_tsv(gdir / "groups.tsv", {"n_cells": int, "n_cells_with_rows": int, "total_depth": int, "mean_depth": float})
    sizes = [int((labels == k).sum()) for k in (0, 1, 2, -1)]
    assert g["group"] == GROUP_NAMES + ["(none)"] and g["n_cells"] == sizes and min(sizes[:3]) > 0
    pc, pd = population(counts, depth, cells)
    assert g["total_depth"] == [int(pd[labels == k].sum()) for k in (0, 1, 2, -1)]
    assert g["mean_depth"] == [float(d) / float(n * L) if n else 0.0 for d, n in zip(g["total_depth"], sizes)]
    assert all(w <= n for w, n in zip(g["n_cells_with_rows"], sizes)) and min(g["n_cells_with_rows"][:3]) > 0
    with h5lite.File(gdir / "group_counts.h5", "r") as f:
        for b in range(4):
            for s in ("fwd", "rev"):
                np.testing.assert_array_equal(f[f"{'ACGT'[b]}_{s}"][...], want[s][:, :, b].T, err_msg=f"{b} {s}")
        np.testing.assert_array_equal(f["coverage"][...], want["cov"].T)
        assert f["coverage"][...].dtype == np.uint64 and f["n_cells"][...].tolist() == sizes[:3]
        assert [x.decode() for x in f["group"][...].tolist()] == GROUP_NAMES
        assert [x.decode() for x in f["reference"][...].tolist()] == ref
    m = read_tsv(gdir / "group_variants.tsv", {k: int for k in MARKER_COLUMNS[4:10] + ("position", "called")} |
                 {"heteroplasmy": float, "heteroplasmy_rest": float})
    assert tuple(m) == MARKER_COLUMNS and len(m["group"]) > 0  # not vacuous at group_min_cells = 0
    keys = [(GROUP_NAMES.index(gn), p - 1, "ACGT".index(nt[-1])) for gn, p, nt in zip(m["group"], m["position"], m["nucleotide"])]
    # (the brute-force loop of test_groups is for small rows: the same rule from the oracle's sums here)
    tot = oracle_totals(counts, depth, cells)
    alt_all = (tot["fwd"] + tot["rev"]).astype(np.int64)
    expect = {}
    for k in range(G):
        alt = (want["fwd"][k] + want["rev"][k]).astype(np.int64)
        cov = want["cov"][k].astype(np.int64)[:, None]
        cov_rest = tot["cov"].astype(np.int64)[:, None] - cov
        af_in = np.divide(alt.astype(np.float64), cov, out=np.zeros(alt.shape), where=cov > 0)
        af_rest = np.divide((alt_all - alt).astype(np.float64), cov_rest, out=np.zeros(alt.shape), where=cov_rest > 0)
        for p, b in np.argwhere(af_in > af_rest).tolist():
            if ref[p] != "ACGT"[b]:
                expect[(k, p, b)] = (float(af_in[p, b]), float(af_rest[p, b]))
    assert sorted(keys) == sorted(expect)
    for i, (k, p, b) in enumerate(keys):
        assert (m["heteroplasmy"][i], m["heteroplasmy_rest"][i]) == expect[(k, p, b)]
        assert (m["alt_fwd"][i], m["alt_rev"][i], m["depth"][i]) == (int(want["fwd"][k, p, b]), int(want["rev"][k, p, b]),
                                                                   int(want["cov"][k, p]))
        assert (m["n_cells_detected"][i], m["n_cells_conf_detected"][i], m["n_cells"][i]) == \
            (int(want["n_det"][k, p, b]), int(want["n_conf"][k, p, b]), sizes[k])
        assert m["variant"][i] == f"{p + 1}{ref[p]}>{'ACGT'[b]}"
        if called_pairs is not None:
            assert m["called"][i] == int((p, b) in called_pairs)
    order = [(k, -(a - r), p, b) for (k, p, b), a, r in zip(keys, m["heteroplasmy"], m["heteroplasmy_rest"])]
    assert order == sorted(order)
    return want, m


@pytest.mark.parametrize("fmt", ["hdf5", "txt"])
def test_pipeline_groups(fmt, tmp_path, engine_lib, monkeypatch):
    """run_pipeline(groups=FILE) on the synth_run_h5 golden reads, the groups file over the whitelist with one
    unknown barcode and every seventh cell unlabelled, group_min_cells = 0 and group_min_af = 0 (at this depth
    the marker table is then not empty; asserted): groups/ equals the oracle applied to the counts of the
    run's own counts.h5 / metadata.h5, every other output file is what a run without the option writes, the
    streamed and the resident path write the same groups/ files, and a run without the option makes none."""
    from mgatk2_amd.analysis.groups import read_tsv
    from mgatk2_amd.analysis.variants import read_variant_stats

    g = Golden("synth_run_h5")
    kw = dict(groups=_groups_file(tmp_path, g.whitelist), **THRESHOLDS)
    _, out = _pipeline(tmp_path, "streamed", fmt, monkeypatch, **kw)
    _, resident = _pipeline(tmp_path, "resident", fmt, monkeypatch, stream="0", **kw)
    _, plain = _pipeline(tmp_path, "plain", fmt, monkeypatch)
    _, both = _pipeline(tmp_path, "both", fmt, monkeypatch, **kw, **VARIANTS)
    assert not (plain / "groups").exists()
    made = ["groups/group_counts.h5", "groups/group_variants.tsv", "groups/groups.tsv"]
    assert [f for f in _files(out) if f.startswith("groups")] == made
    assert [f for f in _files(out) if not f.startswith("groups")] == _files(plain)
    for rel in _files(plain):
        _same_file(out, plain, rel)
    assert _files(resident) == _files(out)
    for rel in made:
        _same_file(out, resident, rel)
    assert [f for f in _files(both) if f.startswith("groups")] == sorted(made + ["groups/group_allele_freq.tsv"])
    h5out = out if fmt == "hdf5" else _pipeline(tmp_path, "h5", "hdf5", monkeypatch)[1]
    counts, depth, ref, barcodes = _run_counts(h5out)
    assert barcodes == g.whitelist
    labels = np.array([_label_of(i) for i in range(len(barcodes))])
    assert (labels < 0).any()  # cells in no group: the (none) line
    _check_group_files(out / "groups", counts, depth, ref, labels)
    stats = read_variant_stats(both / "variants" / "variant_stats.tsv")
    pairs = [(p - 1, "ACGT".index(nt[-1])) for p, nt in zip(stats["position"], stats["nucleotide"])]
    want, m = _check_group_files(both / "groups", counts, depth, ref, labels, set(pairs))
    assert len(pairs) > 0 and 0 < sum(m["called"])
    for rel in made[:1] + made[2:]:
        _same_file(out, both, rel)
    af = read_tsv(both / "groups" / "group_allele_freq.tsv", {k: float for k in GROUP_NAMES})
    assert list(af) == ["variant"] + GROUP_NAMES and af["variant"] == stats["variant"]
    for j, name in enumerate(GROUP_NAMES):
        assert af[name] == [float(int(want["fwd"][j, p, b]) + int(want["rev"][j, p, b])) / float(want["cov"][j, p])
                            if want["cov"][j, p] else 0.0 for p, b in pairs]


def test_pipeline_groups_sharded(tmp_path, engine_lib, monkeypatch):
    """The cells over two routed contexts (one GPU): the same groups/ files as the single context's, byte for
    byte. group_allele_freq.tsv follows the order of each run's own variant_stats.tsv, which is by vmr, a
    rounding that depends on how the cells were split (test_pipeline_variants_sharded): its lines are the same."""
    from mgatk2_amd.analysis.variants import read_variant_stats

    g = Golden("synth_run_h5")
    monkeypatch.setenv("MGP_STREAM_BATCH", "1500")
    kw = dict(groups=_groups_file(tmp_path, g.whitelist), **THRESHOLDS, **VARIANTS)
    _, one = _pipeline(tmp_path, "one", "txt", monkeypatch, **kw)
    _, many = _pipeline(tmp_path, "many", "txt", monkeypatch, devices=[0, 0], **kw)
    made = [f for f in _files(one) if f.startswith("groups")]
    assert len(made) == 4 and [f for f in _files(many) if f.startswith("groups")] == made
    for rel in made:
        if rel != "groups/group_allele_freq.tsv":
            _same_file(one, many, rel)
    lines = [(d / "groups" / "group_allele_freq.tsv").read_text().splitlines() for d in (one, many)]
    assert lines[0][0] == lines[1][0] and sorted(lines[0]) == sorted(lines[1]) and len(lines[0]) > 1
    for d, got in zip((one, many), lines):
        assert [x.split("\t")[0] for x in got[1:]] == read_variant_stats(d / "variants" / "variant_stats.tsv")["variant"]


def test_analyze_groups_equals_the_run(tmp_path, engine_lib, monkeypatch):
    """analyze -i out --groups FILE writes the run's own groups/ files, with the device inflate and with
    --host-inflate; with --barcodes too it equals the oracle over that subset, labelled by the file's columns."""
    from click.testing import CliRunner

    from mgatk2_amd import cli
    from mgatk2_amd.pipeline import analyze_outputs

    g = Golden("synth_run_h5")
    gf = _groups_file(tmp_path, g.whitelist)
    kw = dict(groups=gf, **THRESHOLDS, **VARIANTS)
    _, run = _pipeline(tmp_path, "run", "hdf5", monkeypatch, **kw)
    made = [f for f in _files(run) if f.startswith("groups")]
    assert len(made) == 4
    analyze_outputs(run, tmp_path / "dev", **kw)
    analyze_outputs(run, tmp_path / "host", host_inflate=True, **kw)
    r = CliRunner().invoke(cli.cli, ["analyze", "-i", str(run), "-o", str(tmp_path / "cmd"), "--groups", gf,
                                     "--group-min-cells", "0", "--group-min-af", "0", "--variants", "--variant-min-cells",
                                     "0", "--variant-min-strand-cor", "-1", "--variant-min-vmr", "0"])
    assert r.exit_code == 0, r.output
    for out in (tmp_path / "dev", tmp_path / "host", tmp_path / "cmd"):
        assert [f for f in _files(out) if f.startswith("groups")] == made
        for rel in made:
            _same_file(run, out, rel)
    counts, depth, ref, barcodes = _run_counts(run)
    pick = [i for i in range(len(barcodes)) if i % 3 != 1]
    analyze_outputs(run, tmp_path / "sub", barcodes=[barcodes[i] for i in reversed(pick)], groups=gf, **THRESHOLDS)
    labels = np.array([_label_of(i) for i in pick])
    # (the subset's reference alleles are the file's)
    _check_group_files(tmp_path / "sub" / "groups", counts, depth, ref, labels, cells=np.array(pick))


def test_pipeline_groups_with_the_coverage_filter(tmp_path, engine_lib, monkeypatch):
    """With the cell filter on, the groups cover the kept cells only."""
    from mgatk2_amd.analysis.groups import read_tsv

    g = Golden("synth_run_h5")
    kw = dict(groups=_groups_file(tmp_path, g.whitelist), **THRESHOLDS)
    _, out = _pipeline(tmp_path, "all", "hdf5", monkeypatch, **kw)
    counts, depth, ref, barcodes = _run_counts(out)
    mean = depth.astype(np.float64).mean(axis=1)
    thr = float(np.median(mean[mean > 0]))
    kept = np.flatnonzero(mean >= thr)
    _, filt = _pipeline(tmp_path, "kept", "hdf5", monkeypatch, cell_min_mean_coverage=thr, **kw)
    labels = np.array([_label_of(i) for i in kept])
    assert 0 < kept.size < len(barcodes)
    _check_group_files(filt / "groups", counts, depth, ref, labels, cells=kept)
    sizes = read_tsv(filt / "groups" / "groups.tsv", {"n_cells": int})["n_cells"]
    assert sum(sizes) == kept.size
