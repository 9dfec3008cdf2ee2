"""A finished run's count files loaded on the device (mgp_table.hip): the streaming zlib
inflate against zlib (the corpus of zlib_corpus.py, which test_inflate_zlib.py runs on the host
under the sanitizers first), the tiles' transposition into cell rows against numpy, the round
trip with the run's own HDF5 writer, and the analyses of a loaded table against the run's:
byte for byte, since nothing saturates at these depths."""

from __future__ import annotations

import zlib

import numpy as np
import pytest

import inflate_corpus as ic
import zlib_corpus as zc

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 0xA5
PLANES = 11


# ---- 1. mgp_zlib_inflate --------------------------------------------------------------------
def laid_out(cases):
    src, coff, clen, isize, ooff, total = ic.pack_blocks(cases)
    out = np.full(GUARD + total + GUARD, SENTINEL, np.uint8)
    return src, coff, clen, isize, ooff + np.uint64(GUARD), out, total


def check_streams(cases, status, out, ooff, total):
    assert bytes(out[:GUARD]) == bytes([SENTINEL]) * GUARD, "front guard written"
    assert bytes(out[GUARD + total:]) == bytes([SENTINEL]) * GUARD, "back guard written"
    for i, (name, _, n, want, exp) in enumerate(cases):
        assert status[i] == want, (i, name, int(status[i]))
        got = bytes(out[int(ooff[i]):int(ooff[i]) + n])
        # (a refused stream's bytes stay on the device: its range of out is untouched)
        assert got == (exp if want == ic.OK else bytes([SENTINEL]) * n), (i, name)


def test_zlib_valid_corpus_bit_equal(engine_lib):
    """Every valid stream of the corpus in one call, the outputs abutting at unaligned offsets:
    status 0, zlib's bytes, guards intact."""
    cases = list(zc.valid_cases()) + list(zc.padded_cases())
    src, coff, clen, isize, ooff, out, total = laid_out(cases)
    assert len({int(o) & 3 for o in ooff}) == 4 and total > 8_000_000
    status = engine_lib.inflate_zlib(src, coff, clen, isize, ooff, out)
    check_streams(cases, status, out, ooff, total)


def test_zlib_refusals_between_valid_neighbours(engine_lib):
    """The refusal corpus interleaved with valid streams in one call: each status as on the
    host, the neighbours bit-equal, the refused ranges of out untouched."""
    good = [c for c in zc.valid_cases() if c[2] in (1, 32769, 65537)]
    cases = []
    for i, b in enumerate(zc.invalid_cases()):
        cases += [good[(2 * i) % len(good)], b, good[(2 * i + 1) % len(good)]]
    src, coff, clen, isize, ooff, out, total = laid_out(cases)
    status = engine_lib.inflate_zlib(src, coff, clen, isize, ooff, out)
    assert sorted(set(status.tolist())) == [0, 1, 2, 3]
    check_streams(cases, status, out, ooff, total)


# ---- 2. tiles_to_rows / mgp_table_load -------------------------------------------------------
SHAPES = {  # name: (mito_len, n cells, chunk shape)
    "padded_both": (2500, 130, (1000, 100)),  # 3 x 2 chunks, padded edges in both axes
    "odd": (2500, 95, (700, 30)),
    "one_column": (2500, 3, (64, 1)),
    "larger_than_matrix": (2500, 130, (3000, 200)),
}


def random_planes(L, n, seed):
    """u16 [11][L][n]: sparse counts with 0, 255, 256, 65534 and 65535 among them."""
    rng = np.random.default_rng(seed)
    p = np.where(rng.random((PLANES, L, n)) < 0.2, rng.integers(0, 300, (PLANES, L, n)), 0).astype(np.uint16)
    edge = np.array([0, 255, 256, 65534, 65535], np.uint16)
    at = rng.random((PLANES, L, n)) < 0.01
    p[at] = edge[rng.integers(0, 5, int(at.sum()))]
    p[:, 0, 0], p[:, L - 1, n - 1] = 65535, 65534
    return p


def tiles_of(planes, chunks, lo, hi):
    """u16 [11][row chunks][hi - lo][chunk rows][chunk cols] of the column chunks [lo, hi), zero padded."""
    crow, ccol = chunks
    _, L, n = planes.shape
    nrc = -(-L // crow)
    pad = np.zeros((PLANES, nrc * crow, (hi - lo) * ccol), np.uint16)
    c1 = min(n, hi * ccol)
    pad[:, :L, :c1 - lo * ccol] = planes[:, :, lo * ccol:c1]
    return np.ascontiguousarray(pad.reshape(PLANES, nrc, crow, hi - lo, ccol).transpose(0, 1, 3, 2, 4))


def deflated(tiles, level):
    """(src, chunk_bytes, raw) of the tiles as zlib streams, in the tiles' order."""
    blobs = [zlib.compress(t.tobytes(), level) for t in tiles.reshape(-1, tiles.shape[-2], tiles.shape[-1])]
    return (np.frombuffer(b"".join(blobs), np.uint8), np.array([len(b) for b in blobs], np.int64),
            np.zeros(len(blobs), np.uint8))


def table_planes(eng, n, chunks):
    """The table's rows read back through its own HDF5 writer: u16 [11][L][n]."""
    from mgatk2_amd.engine import H5_PLANES

    crow, ccol = chunks
    L = eng.cfg.mito_len
    nrc, ncc = -(-L // crow), -(-n // ccol)
    got = eng.h5_tiles(np.arange(n, dtype=np.int32), chunks=chunks)
    out = np.zeros((PLANES, nrc * crow, ncc * ccol), np.uint16)
    for k, p in enumerate(H5_PLANES):
        for i, blob in enumerate(got[p]):
            rc, cc = divmod(i, ncc)
            t = np.frombuffer(zlib.decompress(bytes(blob)), np.uint16).reshape(crow, ccol)
            out[k, rc * crow:(rc + 1) * crow, cc * ccol:(cc + 1) * ccol] = t
    assert not out[:, L:].any() and not out[:, :, n:].any()
    return out[:, :L, :n]


@pytest.fixture(scope="module")
def shapes():
    return {k: random_planes(L, n, 7 + i) for i, (k, (L, n, _)) in enumerate(SHAPES.items())}


@pytest.mark.parametrize("level", [0, 4, 9])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_table_load_equals_the_planes(engine_lib, shapes, shape, level):
    """Compressed chunks loaded in one call, and in several calls over column ranges: the
    table's rows equal the planes, n_saturated is numpy's count, and load_planes of the same
    tiles gives the same rows."""
    L, n, chunks = SHAPES[shape]
    planes = shapes[shape]
    ncc = -(-n // chunks[1])
    want_sat = int((planes == 65535).sum())
    splits = {"one": [(0, ncc)], "several": [(c, c + 1) for c in range(ncc)][::-1]}  # (any order of the ranges)
    for how, ranges in splits.items():
        if how == "several" and (ncc == 1 or level != 4):
            continue
        with engine_lib.Engine.open_table(n, L) as eng:
            sat = 0
            for lo, hi in ranges:
                out = eng.load(n, chunks, (lo, hi), lo * chunks[1], *deflated(tiles_of(planes, chunks, lo, hi), level))
                sat += out["n_saturated"]
                assert out["inflate_ms"] > 0 and out["transpose_ms"] > 0
            eng.ready()
            np.testing.assert_array_equal(table_planes(eng, n, chunks), planes, err_msg=f"{shape} {how}")
            assert sat == want_sat > 0
    if level == 4:
        with engine_lib.Engine.open_table(n, L) as eng:
            out = eng.load_planes(n, chunks, (0, ncc), 0, tiles_of(planes, chunks, 0, ncc))
            assert out["n_saturated"] == want_sat and out["inflate_ms"] == 0
            eng.ready()
            np.testing.assert_array_equal(table_planes(eng, n, chunks), planes, err_msg=f"{shape} planes")


def test_table_raw_and_absent_chunks(engine_lib, shapes):
    """A chunk stored as it is (filter mask) is copied, an unallocated one is zeros."""
    from mgatk2_amd.engine import CHUNK_ABSENT, CHUNK_RAW

    L, n, chunks = SHAPES["odd"]
    planes = shapes["odd"].copy()
    ncc, nrc = -(-n // chunks[1]), -(-L // chunks[0])
    planes[3, chunks[0]:2 * chunks[0], chunks[1]:2 * chunks[1]] = 0  # plane 3, row chunk 1, column chunk 1: absent
    tiles = tiles_of(planes, chunks, 0, ncc)
    flat = tiles.reshape(-1, *chunks)
    blobs = [zlib.compress(t.tobytes(), 4) for t in flat]
    raw = np.zeros(len(blobs), np.uint8)
    k_abs, k_raw = (3 * nrc + 1) * ncc + 1, (10 * nrc + 2) * ncc + 3
    blobs[k_abs], raw[k_abs] = b"", CHUNK_ABSENT
    blobs[k_raw], raw[k_raw] = flat[k_raw].tobytes(), CHUNK_RAW
    with engine_lib.Engine.open_table(n, L) as eng:
        eng.load(n, chunks, (0, ncc), 0, np.frombuffer(b"".join(blobs), np.uint8),
                 np.array([len(b) for b in blobs], np.int64), raw)
        eng.ready()
        np.testing.assert_array_equal(table_planes(eng, n, chunks), planes)


def test_table_corrupted_chunk_is_an_error(engine_lib, shapes):
    """One corrupted chunk in the second of two batches: an error naming the chunk and its
    status; that batch's rows stay zero, the first batch's are kept."""
    from mgatk2_amd.exceptions import InvalidInputError, ProcessingError

    L, n, chunks = SHAPES["padded_both"]
    planes = shapes["padded_both"]
    nrc = -(-L // chunks[0])
    with engine_lib.Engine.open_table(n, L) as eng:
        with pytest.raises(ProcessingError, match="not loaded"):
            eng.cell_coverage()
        eng.load(n, chunks, (0, 1), 0, *deflated(tiles_of(planes, chunks, 0, 1), 4))
        src, cb, raw = deflated(tiles_of(planes, chunks, 1, 2), 4)
        k = 5 * nrc + 2  # plane 5, row chunk 2 (one column chunk in the batch)
        bad = src.copy()
        bad[int(cb[:k].sum()) + int(cb[k]) - 1] ^= 0x10  # its Adler-32
        with pytest.raises(InvalidInputError, match=r"plane 5, row chunk 2, column chunk 1\) did not inflate: status 3"):
            eng.load(n, chunks, (1, 2), chunks[1], bad, cb, raw)
        eng.ready()
        with pytest.raises(ProcessingError, match="ready"):
            eng.load(n, chunks, (1, 2), chunks[1], src, cb, raw)
        got = table_planes(eng, n, chunks)
        np.testing.assert_array_equal(got[:, :, :chunks[1]], planes[:, :, :chunks[1]])
        assert not got[:, :, chunks[1]:].any()
        for call in (eng.run, eng.sync, eng.reset, lambda: eng.fetch_rows16()):
            with pytest.raises(ProcessingError, match="loaded table"):
                call()


# ---- 3. a synth run, its own chunks, and the analyses ---------------------------------------
N_CELLS, CHUNKS = 150, (1000, 100)


@pytest.fixture(scope="module")
def synth_run(engine_lib, tmp_path_factory):
    """A run of 150 cells kept open, its chunks from Engine.h5_tiles, and an output directory
    written from them (counts.h5 / metadata.h5 with barcode and reference)."""
    from mgatk2_amd import h5lite
    from mgatk2_amd.engine import H5_PLANES, EngineConfig
    from mgatk2_amd.file_io.writers import ref_alleles
    from mgatk2_amd.synth import barcode_names, synth_reads

    soa = synth_reads(5, 300_000, N_CELLS)
    cfg = EngineConfig(n_cells=N_CELLS, min_baseq=20, min_mapq=30, dedup_mode="alignment_and_fragment_length")
    eng = engine_lib.Engine(cfg)
    eng.push(soa)
    res = eng.finish()
    assert int(res.depth.max()) < 65535  # nothing saturates
    tiles = eng.h5_tiles(np.arange(N_CELLS, dtype=np.int32), chunks=CHUNKS)
    names = barcode_names(N_CELLS, 5)
    refs = ref_alleles(res.ref_tally)
    L = cfg.mito_len
    d = tmp_path_factory.mktemp("table_run")
    (d / "output").mkdir()
    with h5lite.File(d / "output" / "counts.h5", "w", libver="latest") as f:
        f.create_dataset("barcode", data=np.array(names, dtype="S"))
        for p in H5_PLANES[:10]:
            f.create_dataset_from_chunks(p, (L, N_CELLS), np.uint16, CHUNKS, 4, tiles[p])
    with h5lite.File(d / "output" / "metadata.h5", "w", libver="latest") as f:
        f.create_dataset_from_chunks("coverage", (L, N_CELLS), np.uint16, CHUNKS, 4, tiles["coverage"])
        f.create_dataset("reference", data=np.array(refs, dtype="S1"))
    yield {"eng": eng, "res": res, "tiles": tiles, "names": names, "refs": refs, "dir": d, "L": L}
    eng.close()


def equal_dicts(a: dict, b: dict, what: str):
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k)


def equal_analyses(run_src, table_src, refs, cells=None, table_cells=None):
    """run_coverage and run_variants of the two sources, byte for byte."""
    from mgatk2_amd.analysis.coverage import run_coverage
    from mgatk2_amd.analysis.variants import run_variants

    a = run_coverage(run_src, cells=cells, min_mean_coverage=1.0, recompute_reference=True)
    b = run_coverage(table_src, cells=table_cells, min_mean_coverage=1.0, recompute_reference=True)
    for k in ("cell", "position", "strand", "transposition"):
        equal_dicts(getattr(a, k), getattr(b, k), k)
    assert a.kept.tolist() == b.kept.tolist() and a.tally.tobytes() == b.tally.tobytes()
    assert a.ref_alleles == b.ref_alleles and 0 < int(a.kept.sum())
    kw = dict(min_cells=0, min_strand_cor=-1.0, min_vmr=0.0)
    va, vb = run_variants(run_src, refs, cells=cells, **kw), run_variants(table_src, refs, cells=table_cells, **kw)
    equal_dicts(va.moments, vb.moments, "moments")
    assert va.dev2.tobytes() == vb.dev2.tobytes()
    assert len(va.table) > 0 and vars(va.table).keys() == vars(vb.table).keys()
    for k, x in vars(va.table).items():
        y = getattr(vb.table, k)
        assert (x.tobytes() == y.tobytes()) if isinstance(x, np.ndarray) else (x == y), k
    assert va.allele_freq.shape[0] > 0 and va.allele_freq.tobytes() == vb.allele_freq.tobytes()
    return va


def test_round_trip_with_the_runs_writer(engine_lib, synth_run):
    """The run's chunks loaded into a table; the table's own h5_tiles give chunks that inflate to
    the same planes; and the run's coverage and variant results equal the table's byte for byte."""
    from mgatk2_amd.engine import H5_PLANES

    s = synth_run
    ncc, nrc = -(-N_CELLS // CHUNKS[1]), -(-s["L"] // CHUNKS[0])
    blobs = [s["tiles"][p][rc * ncc + cc] for p in H5_PLANES for rc in range(nrc) for cc in range(ncc)]
    src = np.concatenate(blobs)
    with engine_lib.Engine.open_table(N_CELLS, s["L"]) as tab:
        out = tab.load(N_CELLS, CHUNKS, (0, ncc), 0, src, np.array([b.size for b in blobs], np.int64),
                       np.zeros(len(blobs), np.uint8))
        assert out["n_saturated"] == 0
        tab.ready()
        again = tab.h5_tiles(np.arange(N_CELLS, dtype=np.int32), chunks=CHUNKS)
        for p in H5_PLANES:
            for a, b in zip(s["tiles"][p], again[p]):
                assert zlib.decompress(bytes(a)) == zlib.decompress(bytes(b)), p
        equal_analyses(s["eng"], tab, s["refs"])


def test_load_counts_and_a_subset(engine_lib, synth_run):
    """load_counts on the written directory (device and host inflate): barcodes, reference and
    analyses equal the run's, also over a subset population in file order."""
    from mgatk2_amd.table import load_counts

    s = synth_run
    rng = np.random.default_rng(3)
    subset = np.sort(rng.permutation(N_CELLS)[:60]).astype(np.int64)
    for host in (False, True):
        with load_counts(s["dir"], host_inflate=host, col_chunks_per_call=1) as t:
            assert t.barcodes == s["names"] and t.ref_alleles == s["refs"] and t.n_saturated == 0
            assert t.device_inflate == (not host) and t.seconds["transpose"] > 0
            assert (t.seconds["inflate"] > 0) == (not host)
            equal_analyses(s["eng"], t.engine, s["refs"])
            equal_analyses(s["eng"], t.engine, s["refs"], subset, subset)


def test_analyze_outputs_subset_equals_the_run(engine_lib, synth_run, tmp_path):
    """analyze_outputs with a barcode list (given out of file order, with one unknown name):
    the population is those columns in file order, and the table and matrix equal the run's
    over the same cells."""
    from mgatk2_amd.analysis.variants import run_variants
    from mgatk2_amd.pipeline import analyze_outputs

    s = synth_run
    pick = [7, 3, 140, 99, 12, 64, 65, 1, 30, 31, 32, 120, 121, 5, 77]
    out = analyze_outputs(s["dir"], tmp_path / "sub", barcodes=[s["names"][i] for i in pick] + ["NOT-A-CELL"],
                          call_variants=True, variant_min_cells=0, variant_min_strand_cor=-1.0, variant_min_vmr=0.0)
    assert out["cells"] == len(pick) and out["columns"] == N_CELLS
    want = run_variants(s["eng"], s["refs"], cells=np.sort(np.array(pick, np.int64)), min_cells=0, min_strand_cor=-1.0,
                        min_vmr=0.0)
    res = out["result"]
    assert len(want.table) > 0 and res.variants.variant == want.table.variant
    assert res.variants.vmr.tobytes() == want.table.vmr.tobytes()
    assert res.allele_freq.tobytes() == want.allele_freq.tobytes()
    assert (tmp_path / "sub" / "variants" / "variant_stats.tsv").exists()
    assert not (tmp_path / "sub" / "output").exists()  # the count files are never rewritten


# ---- 4. analyze on a pipeline's output directory ---------------------------------------------
ANALYSES = dict(call_variants=True, variant_min_cells=0, variant_min_strand_cor=-1.0, variant_min_vmr=0.0,
                coverage_stats=True, cluster=True, clones=3, neighbors=5, clonotypes=True)


def test_analyze_equals_the_runs_files(engine_lib, tmp_path, monkeypatch):
    """run --format hdf5 with every analysis on, then analyze on its output directory: coverage/
    and variants/ are the run's files, byte for byte (allele_freq.h5: every dataset's bytes),
    from the device inflate, from --host-inflate, and from the command line."""
    from click.testing import CliRunner

    from mgatk2_amd import cli
    from mgatk2_amd.pipeline import analyze_outputs
    from test_gpu_variants import _files, _pipeline, _same_file

    _, run = _pipeline(tmp_path, "run", "hdf5", monkeypatch, **ANALYSES)
    made = [f for f in _files(run) if f.startswith(("coverage/", "variants/"))]
    assert {"variants/cell_clonotypes.tsv", "variants/cell_snn.mtx", "variants/cell_hclust.tsv",
            "coverage/cell_coverage_stats.tsv", "variants/allele_freq.h5"} <= set(made)
    dev, host, cmd = tmp_path / "dev", tmp_path / "host", tmp_path / "cmd"
    analyze_outputs(run, dev, **ANALYSES)
    analyze_outputs(run, host, host_inflate=True, **ANALYSES)
    r = CliRunner().invoke(cli.cli, ["analyze", "-i", str(run), "-o", str(cmd), "--variants", "--variant-min-cells", "0",
                                     "--variant-min-strand-cor", "-1", "--variant-min-vmr", "0", "--coverage-stats",
                                     "--cluster", "--clones", "3", "--neighbors", "5", "--clonotypes"])
    assert r.exit_code == 0, r.output
    for out in (dev, host, cmd):
        assert _files(out) == made
        for rel in made:
            _same_file(out, run, rel)
