"""The device inflate on the device (mgp_inflate.hip): the corpus of inflate_corpus.py in
calls of 1 to ~1,100 blocks at abutting unaligned offsets, the invalid streams between
valid neighbours, the persistent Inflater, the BAM ingest through the hook and the
pipeline's outputs with and without --device-inflate. The CPU program of
test_inflate_core.py runs the same decoder under the sanitizers first."""

import shutil
import struct
from pathlib import Path

import numpy as np
import pytest

import inflate_corpus as ic

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xA5
COLS = ("start", "bc", "tlen", "flag", "mapq", "span", "rec_off", "payload")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The valid streams: zlib's, the odd-sized ones, the far match, libdeflate's BAM blocks."""
    d = tmp_path_factory.mktemp("gpu_inflate_corpus")
    return list(ic.valid_cases()) + list(ic.odd_cases()) + ic.bam_cases(d)


def cycled(cases, n):
    """n blocks: the cases in turn, a 1-byte block after every third so offsets turn odd."""
    one = ic.valid_cases()[1]
    out, k = [], 0
    while len(out) < n:
        out.append(cases[k % len(cases)])
        k += 1
        if k % 3 == 0 and len(out) < n:
            out.append(one)
    return out


def laid_out(cases):
    """The call's arrays with the outputs abutting behind GUARD sentinel bytes, and out."""
    src, coff, clen, isize, ooff, total = ic.pack_blocks(cases)
    out = np.full(GUARD + total + GUARD, SENTINEL, np.uint8)
    return src, coff, clen, isize, ooff + np.uint64(GUARD), out, total


def check_blocks(cases, status, out, ooff, total):
    assert bytes(out[:GUARD]) == bytes([SENTINEL]) * GUARD, "front guard written"
    assert bytes(out[GUARD + total:]) == bytes([SENTINEL]) * GUARD, "back guard written"
    for i, (name, _, n, want, exp) in enumerate(cases):
        assert status[i] == want, (i, name, int(status[i]))
        got = bytes(out[int(ooff[i]):int(ooff[i]) + n])
        if want == ic.OK:  # (a refused block's own range is unspecified; everything around it is checked)
            assert got == exp, (i, name)


@pytest.mark.parametrize("n_blocks", [1, 2, 65, 1100])
def test_valid_corpus_bit_equal(engine_lib, corpus, n_blocks):
    """The valid corpus in one call of 1, 2, 65 and ~1,100 blocks, cycled, ranges abutting at
    unaligned offsets: zlib's bytes, guards intact, a second call the same bytes."""
    cases = cycled(corpus[1:], n_blocks) if n_blocks > 2 else corpus[7:7 + n_blocks]  # (1, 2: odd_* / acgt)
    if n_blocks == 2:
        cases = [ic.odd_cases()[1], corpus[8]]
    src, coff, clen, isize, ooff, out, total = laid_out(cases)
    assert n_blocks < 3 or len({int(o) & 3 for o in ooff}) == 4  # every alignment occurs
    status = engine_lib.inflate_bgzf(src, coff, clen, isize, ooff, out)
    check_blocks(cases, status, out, ooff, total)
    again = np.full_like(out, SENTINEL)
    status2 = engine_lib.inflate_bgzf(src, coff, clen, isize, ooff, again)
    assert np.array_equal(status, status2) and np.array_equal(out, again)


def test_invalid_streams_between_valid_neighbours(engine_lib, corpus):
    """The invalid corpus interleaved 1:3 with valid blocks in one call: each status as on the
    CPU, the neighbours bit-equal, nothing written outside the refused blocks' own ranges."""
    bad = list(ic.invalid_cases())
    good = cycled(corpus[1:], 3 * len(bad))
    cases = []
    for i, b in enumerate(bad):
        cases += good[3 * i:3 * i + 3] + [b]
    src, coff, clen, isize, ooff, out, total = laid_out(cases)
    status = engine_lib.inflate_bgzf(src, coff, clen, isize, ooff, out)
    assert sorted(set(status.tolist())) == [0, 1, 2]
    check_blocks(cases, status, out, ooff, total)


def test_inflater_reused_and_its_bounds(engine_lib, corpus):
    """One Inflater over three calls of different sizes, one of exactly max_src_bytes; one
    byte more is refused (MGP_E_INVALID)."""
    from mgatk2_amd.exceptions import InvalidInputError

    calls = [cycled(corpus[1:], 40), corpus[3:5], cycled(corpus[5:], 7)]
    laid = [laid_out(c) for c in calls]
    max_src = int(laid[0][0].shape[0])
    assert all(int(l[0].shape[0]) <= max_src for l in laid)
    max_out = max(int(l[5].shape[0]) for l in laid)
    with engine_lib.Inflater(0, max_src, max_out) as inf:
        for cases, (src, coff, clen, isize, ooff, out, total) in zip(calls, laid):
            status = inf.run(src, coff, clen, isize, ooff, out)
            check_blocks(cases, status, out, ooff, total)
        src, coff, clen, isize, ooff, out, total = laid[0]
        more = np.concatenate([src, np.zeros(1, np.uint8)])
        with pytest.raises(InvalidInputError, match="created for"):
            inf.run(more, coff, clen, isize, ooff, out)
        status = inf.run(src, coff, clen, isize, ooff, out)  # (still usable)
        assert not status.any()


def read_all(bam, names):
    soa = bam.read_soa("chrM", names)
    return {k: np.array(getattr(soa, k)) for k in COLS}


def stream_all(bam, names, batch=700):
    from mgatk2_amd.bam import StreamSlot

    parts = []
    slot = StreamSlot(batch, batch * 64 + 256 * (len(names) + 1) + (1 << 20))
    with bam.stream("chrM", names) as st:
        while st.next_into(slot):
            v = slot.soa()
            parts.append({k: getattr(v, k).copy() for k in COLS})
    return parts


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_bam_ingest_equals_the_host_path(engine_lib, tmp_path, level):
    """read_soa and stream of the 3,000-read BAM with set_device_inflate(0) equal the host
    path array for array (the first chunk is 64 KiB of blocks, so a chunk boundary falls inside
    a record), with pinned and with plain chunk buffers; None restores the host path."""
    from mgatk2_amd.bam import BamFile

    path = tmp_path / "r.bam"
    names = ic.write_test_bam(path, level)
    with BamFile(path) as bam:
        want, want_parts = read_all(bam, names), stream_all(bam, names)
    assert want["start"].shape[0] == 3000
    for pinned in (True, False):
        with BamFile(path, n_threads=3) as bam:
            bam.set_device_inflate(0, pinned=pinned)
            got, parts = read_all(bam, names), stream_all(bam, names)
            for k in COLS:
                np.testing.assert_array_equal(got[k], want[k], err_msg=k)
            assert len(parts) == len(want_parts)
            for a, b in zip(parts, want_parts):
                for k in COLS:
                    np.testing.assert_array_equal(a[k], b[k], err_msg=k)
            bam.set_device_inflate(None)
            back = read_all(bam, names)
            for k in COLS:
                np.testing.assert_array_equal(back[k], want[k], err_msg=k)


def test_bam_ingest_many_chunks_and_a_flipped_crc(engine_lib, tmp_path):
    """A BAM of several chunks (records carried across chunk ends) equals the host path; with
    one trailer CRC flipped both paths raise the same error."""
    from mgatk2_amd.bam import BamFile
    from mgatk2_amd.exceptions import BAMReadError

    path = tmp_path / "m.bam"
    names = ic.write_test_bam(path, 1, n_reads=60_000, n_cells=40, seed=11)
    assert path.stat().st_size > (64 << 10) * 5  # chunks of 64 KiB, 256 KiB, 1 MiB ...
    with BamFile(path) as bam:
        want = read_all(bam, names)
    with BamFile(path) as bam:
        bam.set_device_inflate(0)
        got = read_all(bam, names)
    for k in COLS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    data = bytearray(path.read_bytes())
    p, k = 0, 0
    while k < 4:  # the trailer of the fifth block
        p += struct.unpack_from("<H", data, p + 16)[0] + 1
        k += 1
    bsize = struct.unpack_from("<H", data, p + 16)[0] + 1
    data[p + bsize - 8] ^= 1
    bad = tmp_path / "bad.bam"
    bad.write_bytes(bytes(data))
    shutil.copy(str(path) + ".bai", str(bad) + ".bai")
    errs = []
    for dev in (None, 0):
        with BamFile(bad) as bam:
            bam.set_device_inflate(dev)
            with pytest.raises(BAMReadError) as e:
                bam.read_soa("chrM", names)
            errs.append(str(e.value))
    assert "BGZF inflate/CRC error" in errs[0] and errs[0] == errs[1]


def h5_content(path) -> list:
    """Every dataset of an HDF5 file (name, dtype, shape, bytes) and every attribute."""
    from mgatk2_amd import h5lite

    out = []

    def visit(g, prefix):
        out.append((prefix, "attrs", sorted((k, repr(v)) for k, v in g.attrs.items())))
        for k in sorted(g.keys()):
            x = g[k]
            if isinstance(x, h5lite.Group):
                visit(x, f"{prefix}{k}/")
            else:
                a = x.read()
                out.append((f"{prefix}{k}", str(a.dtype), a.shape, a.tobytes(),
                            sorted((n, repr(v)) for n, v in x.attrs.items())))

    with h5lite.File(path, "r") as f:
        visit(f, "/")
    return out


def tree(d: Path) -> dict:
    """Every file of an output directory; the two that record the run itself (qc/summary.txt,
    the report) without their lines of the run's date and output directory."""
    out = {}
    for p in sorted(d.rglob("*")):
        if not p.is_file() or p.name == "output.log":
            continue
        if p.suffix == ".h5":  # (libhdf5 stamps its object headers with the second of the write)
            out[str(p.relative_to(d))] = h5_content(p)
            continue
        data = p.read_bytes()
        if p.name in ("summary.txt", "mgatk2_report.html"):
            data = b"\n".join(ln for ln in data.split(b"\n")
                              if not any(w in ln.lower() for w in (b"date", b"output")))
        out[str(p.relative_to(d))] = data
    return out


@pytest.mark.parametrize("fmt,devices", [("txt", None), ("hdf5", None), ("txt", [0, 0]), ("hdf5", [0, 0])])
def test_pipeline_outputs_identical(engine_lib, tmp_path, fmt, devices):
    """The pipeline on a 4-cell synthetic BAM, txt and HDF5, one context and sharded over two
    (--devices), with --variants --neighbors 3: every output file with device_inflate is
    byte-identical to the run without it (an HDF5 file: every dataset and attribute)."""
    from mgatk2_amd import pipeline
    from mgatk2_amd.bam import write_bam
    from mgatk2_amd.synth import barcode_names, synth_reads

    names = barcode_names(4, 3)
    bam = tmp_path / "p.bam"
    write_bam(bam, synth_reads(3, 20_000, 4), names, level=6, n_threads=2)
    bfile = tmp_path / "barcodes.tsv"
    bfile.write_text("".join(b + "\n" for b in names))
    outs = {}
    for flag in (False, True):
        out = tmp_path / ("device" if flag else "host") / "out"
        pipeline.run_pipeline(str(bam), str(bfile), str(out), output_format=fmt, devices=devices,
                              call_variants=True, variant_min_cells=0, variant_min_strand_cor=-1.0,
                              variant_min_vmr=0.0, neighbors=3, device_inflate=flag, report_title="t",
                              working_directory=str(tmp_path))
        outs[flag] = tree(out)
    assert outs[False] and set(outs[False]) == set(outs[True])
    for rel in outs[False]:
        assert outs[False][rel] == outs[True][rel], rel
