"""Loading a finished run's count files, without a device: h5lite's chunk access, the argument
checks of the table's C-ABI, the new symbols, and the plumbing of `analyze` (its options, and
what analyze_outputs hands to the analyses over a numpy stand-in of the table)."""

from __future__ import annotations

import ctypes as C
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

PLANES = 11


# ---- h5lite: filters, chunk_info, read_chunk -------------------------------------------------
def reassembled(ds) -> np.ndarray:
    """The dataset from read_chunk + zlib of every chunk (unallocated: zeros; mask bit 0: stored)."""
    (L, n), (crow, ccol) = ds.shape, ds.chunks
    nrc, ncc = -(-L // crow), -(-n // ccol)
    out = np.zeros((nrc * crow, ncc * ccol), ds.dtype)
    for rc in range(nrc):
        for cc in range(ncc):
            info = ds.chunk_info((rc, cc))
            if info is None:
                continue
            buf = np.empty(info[0], np.uint8)
            mask = ds.read_chunk((rc, cc), buf)
            assert mask == info[1]
            raw = bytes(buf) if mask & 1 else zlib.decompress(bytes(buf))
            out[rc * crow:(rc + 1) * crow, cc * ccol:(cc + 1) * ccol] = np.frombuffer(raw, ds.dtype).reshape(crow, ccol)
    return out[:L, :n]


def test_h5lite_chunks(tmp_path):
    """read_chunk + zlib.decompress of every chunk, reassembled, equals Dataset.read() for a file
    written by create_dataset(compression="gzip") and one by create_dataset_from_chunks; filters,
    unallocated chunks and filter masks are reported."""
    from mgatk2_amd import h5lite
    from mgatk2_amd.bam import deflate_tiles

    rng = np.random.default_rng(4)
    a = np.where(rng.random((2500, 130)) < 0.1, rng.integers(0, 70000, (2500, 130)), 0).clip(0, 65535).astype(np.uint16)
    chunks = (1000, 100)
    tiles = list(deflate_tiles(a, chunks, level=4))
    lib = h5lite._h5()
    with h5lite.File(tmp_path / "a.h5", "w", libver="latest") as f:
        f.create_dataset("gz", data=a, chunks=chunks, compression="gzip", compression_opts=4)
        f.create_dataset_from_chunks("tiles", a.shape, np.uint16, chunks, 4, tiles)
        f.create_dataset("plain", data=a)
        f.create_dataset("chunked", data=a, chunks=chunks)
        # a dataset with two chunks written of six, one of them stored as it is (mask bit 0)
        sparse = f.create_dataset_from_chunks("sparse", a.shape, np.uint16, chunks, 4, [tiles[0]])
        raw = np.ascontiguousarray(np.zeros(chunks, np.uint16) + 7)
        off = (h5lite.hsize_t * 2)(2000, 100)
        assert lib.H5Dwrite_chunk(sparse._id, h5lite.H5P_DEFAULT, 1, off, raw.nbytes, raw.ctypes.data) >= 0
    with h5lite.File(tmp_path / "a.h5", "r") as f:
        for name in ("gz", "tiles"):
            ds = f[name]
            assert ds.filters == (h5lite.H5Z_FILTER_DEFLATE,) and ds.chunks == chunks
            assert all(ds.chunk_info((rc, cc))[1] == 0 for rc in range(3) for cc in range(2))
            np.testing.assert_array_equal(reassembled(ds), ds.read())
            np.testing.assert_array_equal(ds.read(), a)
        assert f["plain"].filters == () and f["plain"].chunks is None
        assert f["chunked"].filters == () and f["chunked"].chunks == chunks
        with pytest.raises(ValueError):
            f["plain"].chunk_info((0, 0))
        sp = f["sparse"]
        assert sp.chunk_info((0, 0)) == (len(tiles[0]), 0) and sp.chunk_info((2, 1)) == (raw.nbytes, 1)
        assert [sp.chunk_info(c) for c in ((0, 1), (1, 0), (1, 1), (2, 0))] == [None] * 4
        with pytest.raises(KeyError):
            sp.read_chunk((1, 1), np.empty(16, np.uint8))
        with pytest.raises(IndexError):
            sp.chunk_info((3, 0))
        with pytest.raises(ValueError):
            sp.read_chunk((0, 0), np.empty(4, np.uint8))  # too small
        np.testing.assert_array_equal(reassembled(sp), sp.read())
        assert sp.read()[2400, 129] == 7 and not sp.read()[1000:2000].any()


# ---- the C-ABI without a device --------------------------------------------------------------
NEW_SYMBOLS = ("mgp_zlib_inflate", "mgp_open_table", "mgp_table_load", "mgp_table_load_planes", "mgp_table_check",
               "mgp_table_ready")


def test_new_symbols_are_exported():
    from mgatk2_amd import engine

    lib = engine.load_library()
    for s in NEW_SYMBOLS:
        assert s in engine.ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.mgp_abi_version() == engine.ABI_VERSION == 7
    assert not [s for s in NEW_SYMBOLS if s.endswith("_rows")]
    for name in ("open_table", "load", "load_planes", "ready"):
        assert hasattr(engine.Engine, name)
    assert hasattr(engine, "inflate_zlib")


def test_struct_layout_matches_the_header(tmp_path):
    import subprocess
    from pathlib import Path

    from mgatk2_amd import engine

    root = Path(__file__).resolve().parent.parent
    cls = engine.mgp_table_chunks
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{root}/include/mgpileup.h"', "int main(){",
             'printf("%zu\\n", sizeof(mgp_table_chunks));']
    lines += [f'printf("%zu\\n", offsetof(mgp_table_chunks, {f}));' for f, _ in cls._fields_]
    (tmp_path / "l.c").write_text("\n".join(lines + ["return 0;}"]))
    subprocess.run(["gcc", str(tmp_path / "l.c"), "-o", str(tmp_path / "l")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "l")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]


def test_arguments_refused_without_a_device():
    """Every argument check of mgp_open_table, mgp_table_load, mgp_table_load_planes (through
    mgp_table_check, which makes the loads' checks without a context) and mgp_zlib_inflate is
    made before any allocation or launch: MGP_E_INVALID with its own message."""
    from mgatk2_amd import engine
    from mgatk2_amd.exceptions import InvalidInputError

    lib = engine.load_library()

    def refused(rc, message):
        assert rc == engine.MGP_E_INVALID, (rc, message)
        assert message in lib.mgp_last_error().decode(), (lib.mgp_last_error(), message)

    h = C.c_void_p()
    refused(lib.mgp_open_table(0, 4, 100, None), "mgp_open_table: null out")
    refused(lib.mgp_open_table(0, 4, 0, C.byref(h)), "mgp_open_table: mito_len out of range")
    refused(lib.mgp_open_table(0, 4, (1 << 24) + 1, C.byref(h)), "mgp_open_table: mito_len out of range")
    refused(lib.mgp_open_table(0, -1, 100, C.byref(h)), "mgp_open_table: n_cells < 0")
    refused(lib.mgp_table_load(None, None), "mgp_table_load: null ctx")
    refused(lib.mgp_table_load_planes(None, None), "mgp_table_load_planes: null ctx")
    refused(lib.mgp_table_ready(None), "mgp_table_ready: null ctx")

    # a batch of the 2500 x 130 table in chunks of (1000, 100): column chunk 1 -> 11 * 3 chunks
    n_cells, L, nch = 130, 2500, PLANES * 3
    sizes = np.full(nch, 10, np.int64)
    raw = np.zeros(nch, np.uint8)
    src = np.zeros(nch * 10, np.uint8)

    def job(**kw):
        d = dict(n_cols=130, chunk_rows=1000, chunk_cols=100, col_chunk_lo=1, col_chunk_hi=2, first_cell=100,
                 src=src, src_bytes=None, chunk_bytes=sizes, raw=raw)
        d.update(kw)
        keep = [d["src"], d["chunk_bytes"], d["raw"]]
        sb = d["src_bytes"] if d["src_bytes"] is not None else (0 if d["src"] is None else d["src"].size)
        j = engine.mgp_table_chunks(d["n_cols"], d["chunk_rows"], d["chunk_cols"], d["col_chunk_lo"], d["col_chunk_hi"],
                                    d["first_cell"], 0, engine._ptr(d["src"]), sb, engine._ptr(d["chunk_bytes"]),
                                    engine._ptr(d["raw"]), 0)
        return j, keep

    def check(message, planes=0, n=n_cells, mito=L, **kw):
        j, keep = job(**kw)
        rc = lib.mgp_table_check(n, mito, C.byref(j), planes)
        if message is None:
            assert rc == 0, lib.mgp_last_error()
        else:
            refused(rc, message)
        del keep

    check(None)
    refused(lib.mgp_table_check(n_cells, L, None, 0), "mgp_table_load: null job")
    refused(lib.mgp_table_check(n_cells, L, None, 1), "mgp_table_load_planes: null job")
    check("table shape out of range", mito=0)
    check("table shape out of range", n=-1)
    check("n_cols out of range", n_cols=-1)
    check("chunk shape not positive", chunk_rows=0)
    check("chunk shape not positive", chunk_cols=-3)
    check("a chunk of 2^31 bytes or more", chunk_rows=1 << 15, chunk_cols=1 << 15)
    check("column chunks out of range", col_chunk_lo=-1)
    check("column chunks out of range", col_chunk_lo=2, col_chunk_hi=1)
    check("column chunks out of range", col_chunk_hi=3)
    check("too many chunks for one call", chunk_rows=1, chunk_cols=1, col_chunk_lo=0, col_chunk_hi=130, mito=1 << 20)
    check("too many column chunks for one call", n_cols=70000, chunk_rows=2500, chunk_cols=1, col_chunk_lo=0,
          col_chunk_hi=70000, n=70000)
    check("columns outside the table's cells", first_cell=-1)
    check("columns outside the table's cells", first_cell=101)
    check("columns outside the table's cells", n=129)
    check("null or negative src", src=None, src_bytes=5)
    check("null or negative src", src_bytes=-1)
    check("null chunk_bytes or raw", chunk_bytes=None)
    check("null chunk_bytes or raw", raw=None)
    bad = raw.copy()
    bad[4] = 3
    check("unknown raw flag (chunk 4)", raw=bad)
    neg = sizes.copy()
    neg[7] = -1
    check("chunk size out of range (chunk 7)", chunk_bytes=neg)
    big = sizes.copy()
    big[7] = 1 << 31
    check("chunk size out of range (chunk 7)", chunk_bytes=big)
    absent = raw.copy()
    absent[2] = engine.CHUNK_ABSENT
    check("an absent chunk with bytes (chunk 2)", raw=absent)
    check("chunk sizes do not add up to src_bytes", src_bytes=src.size - 1)
    tiles = np.zeros(nch * 1000 * 100, np.uint16).view(np.uint8)
    check(None, planes=1, src=tiles, chunk_bytes=None, raw=None)
    check("src_bytes is not the batch's tiles", planes=1, src=tiles, src_bytes=tiles.size - 2)
    check(None, col_chunk_lo=1, col_chunk_hi=1, src=None, chunk_bytes=None, raw=None)  # no chunks: nothing needed

    s = zlib.compress(b"x")
    src2 = np.frombuffer(s + s, np.uint8)
    out = np.zeros(16, np.uint8)

    def call(coff, clen, isize, ooff, o=out):
        return engine.inflate_zlib(src2, coff, clen, isize, ooff, o)

    with pytest.raises(InvalidInputError, match="overlapping"):
        call([0, len(s)], [len(s)] * 2, [4, 4], [0, 3])
    with pytest.raises(InvalidInputError, match="2\\^31 bytes or more"):
        call([0], [len(s)], [1 << 31], [0])
    with pytest.raises(InvalidInputError, match="outside src"):
        call([len(s)], [len(s) + 1], [1], [0])
    with pytest.raises(InvalidInputError, match="outside out"):
        call([0], [len(s)], [17], [0])
    one = np.zeros(1, np.uint64)
    p = one.ctypes.data
    refused(lib.mgp_zlib_inflate(0, None, 4, 1, p, p, p, p, out.ctypes.data, 16, p), "mgp_zlib_inflate: null buffer")
    refused(lib.mgp_zlib_inflate(0, src2.ctypes.data, 4, 1, None, None, None, None, out.ctypes.data, 16, None),
            "mgp_zlib_inflate: null array")
    refused(lib.mgp_zlib_inflate(0, src2.ctypes.data, 4, -1, None, None, None, None, out.ctypes.data, 16, None),
            "mgp_zlib_inflate: negative count")
    assert lib.mgp_zlib_inflate(0, None, 0, 0, None, None, None, None, None, 0, None) == 0  # no streams: nothing launched


# ---- the command and analyze_outputs ---------------------------------------------------------
def test_analyze_help_and_requires():
    """`analyze --help` lists every analysis option of `run` (and not the BAM's), and an option
    without what it needs is refused with run's message."""
    from click.testing import CliRunner

    from mgatk2_amd import cli
    from mgatk2_amd.options import FLAGS, REQUIRES

    run_help = CliRunner().invoke(cli.cli, ["run", "--help"]).output
    r = CliRunner().invoke(cli.cli, ["analyze", "--help"])
    assert r.exit_code == 0
    run_flags = [p.opts[0] for p in cli.run.params]
    shared = [f for f in run_flags[run_flags.index("--variants"):] if f != "--device-inflate"]  # (after run's own)
    assert [p.opts[0] for p in cli.analyze.params][-len(shared):] == shared and len(shared) == 17
    assert set(FLAGS.values()) <= set(shared) and "--coverage-stats" in shared and "--variant-min-vmr" in shared
    for flag in shared + ["--input", "--output", "--barcodes", "--host-inflate", "--device"]:
        assert flag in r.output, flag
        assert flag in run_help or flag == "--host-inflate", flag
    assert "--device-inflate" in run_help and "--device-inflate" not in r.output and "--genome" not in r.output
    values = {"clones": ["--clones", "2"], "neighbors": ["--neighbors", "5"], "snn_prune": ["--snn-prune", "0.1"],
              "clonotype_resolution": ["--clonotype-resolution", "1.5"]}
    for option, needs in REQUIRES:
        args = values.get(option, [FLAGS[option]])
        a = CliRunner().invoke(cli.cli, ["analyze", "-i", ".", *args])
        b = CliRunner().invoke(cli.cli, ["run", "-i", ".", *args])
        msg = f"{FLAGS[option]} requires {FLAGS[needs]}"
        assert a.exit_code == 2 and msg in a.output and msg in b.output, (option, a.output)


class FakeTable:
    """A numpy stand-in of Engine.open_table: load inflates with zlib, load_planes takes the
    tiles, both into u16 planes [11][L][n]."""

    opened: list = []

    def __init__(self, n_cells, mito_len, device=0):
        self.cfg = SimpleNamespace(n_cells=n_cells, mito_len=mito_len)
        self.planes = np.zeros((PLANES, mito_len, n_cells), np.uint16)
        self.calls, self.is_ready, self.closed, self.device = [], False, False, device
        FakeTable.opened.append(self)

    def _put(self, tiles, chunks, col_chunks, first_cell):
        crow, ccol = chunks
        L, n = self.planes.shape[1:]
        lo, hi = col_chunks
        nrc = -(-L // crow)
        full = tiles.reshape(PLANES, nrc, hi - lo, crow, ccol).transpose(0, 1, 3, 2, 4).reshape(PLANES, nrc * crow, -1)
        w = min(n - first_cell, (hi - lo) * ccol)
        self.planes[:, :, first_cell:first_cell + w] = full[:, :L, :w]
        return {"n_saturated": int((full[:, :L, :w] == 65535).sum()), "h2d_ms": 1.0, "inflate_ms": 2.0, "transpose_ms": 3.0}

    def load(self, n_cols, chunks, col_chunks, first_cell, src, chunk_bytes, raw):
        assert not self.is_ready and first_cell == col_chunks[0] * chunks[1] and n_cols == self.planes.shape[2]
        self.calls.append(("load", tuple(col_chunks)))
        offs = np.concatenate([[0], np.cumsum(chunk_bytes)])
        tiles = []
        for k, kind in enumerate(raw.tolist()):
            blob = bytes(src[offs[k]:offs[k + 1]])
            data = bytes(chunks[0] * chunks[1] * 2) if kind == 2 else blob if kind == 1 else zlib.decompress(blob)
            tiles.append(np.frombuffer(data, np.uint16))
        return self._put(np.concatenate(tiles), chunks, col_chunks, first_cell)

    def load_planes(self, n_cols, chunks, col_chunks, first_cell, tiles):
        assert not self.is_ready
        self.calls.append(("planes", tuple(col_chunks)))
        return self._put(np.ascontiguousarray(tiles).reshape(-1), chunks, col_chunks, first_cell)

    def ready(self):
        self.is_ready = True

    def close(self):
        self.closed = True


@pytest.fixture()
def count_dir(tmp_path):
    """An output directory of 130 cells x 2500 positions: chunked gzip datasets, one chunk of
    one plane unallocated, barcodes, reference and a barcode_metadata column."""
    from mgatk2_amd import h5lite
    from mgatk2_amd.bam import deflate_tiles
    from mgatk2_amd.engine import H5_PLANES

    rng = np.random.default_rng(8)
    L, n, chunks = 2500, 130, (1000, 100)
    planes = np.where(rng.random((PLANES, L, n)) < 0.1, rng.integers(1, 40, (PLANES, L, n)), 0).astype(np.uint16)
    planes[2, 77, 5] = 65535
    planes[4, :1000, :100] = 0
    names = [f"CELL{i:04d}-1" for i in range(n)]
    refs = [("ACGTN"[i % 5]) for i in range(L)]
    out = tmp_path / "run" / "output"
    out.mkdir(parents=True)
    with h5lite.File(out / "counts.h5", "w", libver="latest") as f:
        f.create_dataset("barcode", data=np.array(names, dtype="S"))
        for k, p in enumerate(H5_PLANES[:10]):
            tiles = list(deflate_tiles(planes[k], chunks, level=4))
            if k == 4:  # its first chunk is never written
                ds = f.create_dataset_from_chunks(p, (L, n), np.uint16, chunks, 4, [])
                off = (h5lite.hsize_t * 2)()
                for i, blob in enumerate(tiles[1:], 1):
                    off[0], off[1] = (i // 2) * 1000, (i % 2) * 100
                    assert h5lite._h5().H5Dwrite_chunk(ds._id, 0, 0, off, len(blob), blob) >= 0
            else:
                f.create_dataset_from_chunks(p, (L, n), np.uint16, chunks, 4, tiles)
    with h5lite.File(out / "metadata.h5", "w", libver="latest") as f:
        f.create_dataset("coverage", data=planes[10], chunks=chunks, compression="gzip", compression_opts=4)
        f.create_dataset("reference", data=np.array(refs, dtype="S1"))
        f.create_group("barcode_metadata").create_dataset("passed_filters", data=np.arange(n))
    return SimpleNamespace(dir=tmp_path / "run", planes=planes, names=names, refs=refs, chunks=chunks)


@pytest.mark.parametrize("host", [False, True])
def test_load_counts_feeds_the_table(count_dir, monkeypatch, caplog, host):
    """load_counts reads barcode, reference and barcode_metadata, feeds the table batch by batch
    (raw chunks, an unallocated chunk as zeros; host_inflate: libhdf5's planes), marks it ready
    and warns about values of 65,535; the flat directory works too."""
    from mgatk2_amd import engine, table

    FakeTable.opened = []
    monkeypatch.setattr(engine.Engine, "open_table", classmethod(lambda cls, n, L, device=0: FakeTable(n, L, device)))
    with caplog.at_level("WARNING", logger="mgatk2_amd.table"):
        t = table.load_counts(count_dir.dir, device=3, host_inflate=host, col_chunks_per_call=1)
    fake = FakeTable.opened[0]
    assert t.engine is fake and fake.is_ready and not fake.closed and fake.device == 3
    assert fake.calls == [("planes" if host else "load", (0, 1)), ("planes" if host else "load", (1, 2))]
    np.testing.assert_array_equal(fake.planes, count_dir.planes)
    assert t.barcodes == count_dir.names and t.ref_alleles == count_dir.refs and t.n_saturated == 1
    assert t.barcode_metadata["passed_filters"].tolist() == list(range(130)) and t.device_inflate == (not host)
    assert t.seconds["h2d"] == pytest.approx(0.002) and t.seconds["transpose"] == pytest.approx(0.006)
    assert "1 loaded values are 65,535" in caplog.text
    t.close()
    assert fake.closed
    flat = table.load_counts(count_dir.dir / "output", host_inflate=host)  # the folder that holds the two files
    np.testing.assert_array_equal(FakeTable.opened[1].planes, count_dir.planes)
    assert FakeTable.opened[1].calls == [("planes" if host else "load", (0, 2))] and flat.n_cells == 130


def test_load_counts_refuses_what_it_cannot_read(count_dir, tmp_path, monkeypatch):
    from mgatk2_amd import engine, h5lite, table
    from mgatk2_amd.exceptions import InvalidInputError

    monkeypatch.setattr(engine.Engine, "open_table", classmethod(lambda cls, n, L, device=0: FakeTable(n, L, device)))
    with pytest.raises(InvalidInputError, match="Counts file not found"):
        table.load_counts(tmp_path / "nothing")
    (count_dir.dir / "output" / "metadata.h5").rename(tmp_path / "m.h5")
    with pytest.raises(InvalidInputError, match="Metadata file not found"):
        table.load_counts(count_dir.dir)
    with h5lite.File(count_dir.dir / "output" / "metadata.h5", "w") as f:
        f.create_dataset("coverage", data=np.zeros((2500, 129), np.uint16))
        f.create_dataset("reference", data=np.array(count_dir.refs, dtype="S1"))
    with pytest.raises(InvalidInputError, match="coverage: shape"):
        table.load_counts(count_dir.dir)
    with h5lite.File(count_dir.dir / "output" / "metadata.h5", "w") as f:
        f.create_dataset("coverage", data=np.zeros((2500, 130), np.uint32))
        f.create_dataset("reference", data=np.array(count_dir.refs, dtype="S1"))
    with pytest.raises(InvalidInputError, match="coverage: values are"):
        table.load_counts(count_dir.dir)
    # a contiguous dataset: every plane goes through libhdf5
    with h5lite.File(count_dir.dir / "output" / "metadata.h5", "w") as f:
        f.create_dataset("coverage", data=count_dir.planes[10])
        f.create_dataset("reference", data=np.array(count_dir.refs, dtype="S1"))
    FakeTable.opened = []
    t = table.load_counts(count_dir.dir)
    assert not t.device_inflate and {c[0] for c in FakeTable.opened[0].calls} == {"planes"}
    np.testing.assert_array_equal(FakeTable.opened[0].planes, count_dir.planes)


def test_analyze_outputs_plumbing(count_dir, tmp_path, monkeypatch):
    """analyze_outputs hands the analyses the table as one part, the file's reference, the subset
    population in file order and the options, and writes into output_dir alone."""
    from mgatk2_amd import engine, pipeline
    from mgatk2_amd.analysis import coverage, variants
    from mgatk2_amd.exceptions import InvalidInputError

    FakeTable.opened = []
    monkeypatch.setattr(engine.Engine, "open_table", classmethod(lambda cls, n, L, device=0: FakeTable(n, L, device)))
    seen = {}

    def fake_coverage(parts, cells=None, **opt):
        seen["coverage"] = (list(parts), None if cells is None else cells.copy(), opt)
        n = len(cells)
        kept = np.arange(n) % 2 == 0
        return SimpleNamespace(cells=cells, kept=kept, kept_cells=cells[kept], ref_alleles=None, cell={}, position={},
                               strand={}, transposition={}, tally=None, seconds={})

    def fake_variants(parts, ref, cells=None, **opt):
        assert not list(parts)[0][0].closed and list(parts)[0][0].is_ready
        seen["variants"] = (list(parts), list(ref), cells.copy(), opt)
        z, zi = np.zeros(0), np.zeros(0, np.int64)
        tab = variants.VariantTable(zi, zi, [], z, z, z, zi, zi, z)
        return SimpleNamespace(table=tab, allele_freq=np.zeros((0, len(cells))), seconds={})

    monkeypatch.setattr(coverage, "run_coverage", fake_coverage)
    monkeypatch.setattr(variants, "run_variants", fake_variants)
    names = count_dir.names
    bfile = tmp_path / "subset.tsv"
    bfile.write_text("\n".join([names[40], names[3], "NOT-THERE-1", names[129], names[41]]) + "\n")
    out = pipeline.analyze_outputs(count_dir.dir, tmp_path / "o", barcodes=str(bfile), device=2, call_variants=True,
                                   variant_min_vmr=0.5, variant_min_cells=2, cell_min_mean_coverage=1.5, neighbors=4)
    fake = FakeTable.opened[0]
    assert fake.closed and fake.device == 2 and out["cells"] == 4 and out["columns"] == 130
    parts, cells, opt = seen["coverage"]
    assert parts == [(fake, 0, 130)] and cells.tolist() == [3, 40, 41, 129]
    assert opt == dict(min_mean_coverage=1.5, min_coverage_breadth=0.0, recompute_reference=False)
    parts, ref, cells, opt = seen["variants"]
    assert parts == [(fake, 0, 130)] and ref == count_dir.refs and cells.tolist() == [3, 41]  # the kept of the subset
    assert opt == dict(min_cells=2, min_strand_cor=0.65, min_vmr=0.5, stabilize_variance=False,
                       low_coverage_threshold=10, min_coverage=1)
    assert (tmp_path / "o" / "variants" / "variant_stats.tsv").exists()
    assert sorted(p.name for p in (count_dir.dir).iterdir()) == ["output"]
    # no barcodes: every column, and the input directory receives the outputs
    pipeline.analyze_outputs(count_dir.dir, call_variants=True)
    assert seen["variants"][2].tolist() == list(range(130)) and (count_dir.dir / "variants").is_dir()
    with pytest.raises(InvalidInputError, match="No matching barcodes found"):
        pipeline.analyze_outputs(count_dir.dir, barcodes=["A", "B"], call_variants=True)
    with pytest.raises(InvalidInputError, match="--cluster requires --variants"):
        pipeline.analyze_outputs(count_dir.dir, cluster=True)
    assert all(t.closed for t in FakeTable.opened)
