"""A finished run's count files loaded onto the device (read_mgatk_hdf5 of R/mgatk2_functions.R:1-96).

``load_counts(output_dir)`` opens ``output/counts.h5`` and ``output/metadata.h5`` (or the two
files in ``output_dir`` itself), checks the 11 count datasets and loads them into a table
context (:meth:`Engine.open_table`): the chunks' stored bytes are read with ``H5Dread_chunk``
on a reader thread, one batch of column chunks ahead of the device, which inflates them and
transposes their tiles into the cell rows every analysis reads (mgp_table_load). The values
are the stored ones, min(v, 65535), as R reads them.
"""

from __future__ import annotations

import logging
import threading
import time
from dataclasses import dataclass, field
from pathlib import Path
from queue import Queue

import numpy as np

from . import h5lite
from .engine import CHUNK_ABSENT, CHUNK_RAW, CHUNK_ZLIB, H5_PLANES, Engine
from .exceptions import InvalidInputError

logger = logging.getLogger(__name__)

COL_CHUNKS_PER_CALL = 32  # column chunks of one mgp_table_load call


@dataclass
class LoadedCounts:
    """The table and what the files say about it; close() frees the device context."""

    engine: Engine
    barcodes: list[str]
    ref_alleles: list[str]
    barcode_metadata: dict | None
    n_saturated: int
    seconds: dict = field(default_factory=dict)  # read, h2d, inflate, transpose (and total)
    device_inflate: bool = True  # False: the planes were read by libhdf5 (host_inflate, or a pipeline not deflate alone)

    @property
    def n_cells(self) -> int:
        return len(self.barcodes)

    def close(self):
        self.engine.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def count_files(output_dir) -> tuple[Path, Path]:
    """counts.h5 and metadata.h5 of a run's output directory (its output/ folder, as
    read_mgatk_hdf5 takes it, or the folder that holds the two files)."""
    d = Path(output_dir)
    for base in (d / "output", d):
        if (base / "counts.h5").exists() or (base / "metadata.h5").exists():
            break
    else:
        base = d / "output"
    counts, meta = base / "counts.h5", base / "metadata.h5"
    if not counts.exists():
        raise InvalidInputError(f"Counts file not found: {counts}")
    if not meta.exists():
        raise InvalidInputError(f"Metadata file not found: {meta}")
    return counts, meta


def _strings(a) -> list[str]:
    return [x.decode() if isinstance(x, bytes) else str(x) for x in np.asarray(a).reshape(-1).tolist()]


def _check_datasets(ds: list) -> tuple[int, int]:
    """The 11 datasets have one shape (mito_len, n), u16 values and one chunk shape."""
    shape = ds[0].shape
    if len(shape) != 2:
        raise InvalidInputError(f"{H5_PLANES[0]}: a count dataset is [positions][cells], not {shape}")
    for name, d in zip(H5_PLANES, ds):
        if d.shape != shape:
            raise InvalidInputError(f"{name}: shape {d.shape} differs from {H5_PLANES[0]}'s {shape}")
        if np.dtype(d.dtype) != np.dtype("<u2"):
            raise InvalidInputError(f"{name}: values are {d.dtype}, not 16-bit unsigned")
    return int(shape[0]), int(shape[1])


def _device_loadable(ds: list) -> bool:
    """Every dataset is chunked alike with deflate as its whole pipeline."""
    ch = ds[0].chunks
    return ch is not None and all(d.chunks == ch and d.filters == (h5lite.H5Z_FILTER_DEFLATE,) for d in ds)


def _read_batch(ds: list, nrc: int, lo: int, hi: int):
    """The stored bytes of the column chunks [lo, hi) of every dataset, concatenated plane-major,
    then row chunk, then column chunk, with their sizes and kinds."""
    n = len(ds) * nrc * (hi - lo)
    sizes, kinds = np.zeros(n, np.int64), np.zeros(n, np.uint8)
    infos, k = [], 0
    for d in ds:
        for rc in range(nrc):
            for cc in range(lo, hi):
                info = d.chunk_info((rc, cc))
                infos.append(info)
                if info is None:
                    kinds[k] = CHUNK_ABSENT
                else:
                    sizes[k] = info[0]
                    kinds[k] = CHUNK_RAW if info[1] & 1 else CHUNK_ZLIB  # (bit 0: the pipeline's one filter skipped)
                k += 1
    offs = np.concatenate([[0], np.cumsum(sizes)])
    buf = np.empty(max(1, int(offs[-1])), np.uint8)
    k = 0
    for d in ds:
        for rc in range(nrc):
            for cc in range(lo, hi):
                if infos[k] is not None:
                    d.read_chunk((rc, cc), buf[offs[k]:offs[k + 1]])
                k += 1
    return buf[:int(offs[-1])], sizes, kinds


def _tiles_of(planes: list[np.ndarray], chunks: tuple[int, int], lo: int, hi: int) -> np.ndarray:
    """The column chunks [lo, hi) of the planes ([L][n] u16) as mgp_table_load_planes takes them:
    u16 [11][row chunks][hi - lo][chunk rows][chunk columns], edges padded with 0."""
    crow, ccol = chunks
    L, n = planes[0].shape
    nrc = -(-L // crow)
    c0, c1 = lo * ccol, min(n, hi * ccol)
    out = np.zeros((len(planes), nrc * crow, (hi - lo) * ccol), np.uint16)
    for k, p in enumerate(planes):
        out[k, :L, :c1 - c0] = p[:, c0:c1]
    return np.ascontiguousarray(out.reshape(len(planes), nrc, crow, hi - lo, ccol).transpose(0, 1, 3, 2, 4))


def load_counts(output_dir, device: int = 0, host_inflate: bool = False,
                col_chunks_per_call: int = COL_CHUNKS_PER_CALL) -> LoadedCounts:
    """The count files of `output_dir` as a table on `device`. Unallocated chunks are zeros
    and chunks whose filter mask says deflate was skipped are taken as stored. When a dataset
    is contiguous or its filter pipeline is not deflate alone (shuffle, szip), or with
    host_inflate, libhdf5 reads the planes (Dataset.read) and the device only transposes them
    (mgp_table_load_planes). Warns when values of 65,535 were loaded: they may be saturated
    counts, as they are for R."""
    counts_path, meta_path = count_files(output_dir)
    t_start = time.perf_counter()
    seconds = {"read": 0.0, "h2d": 0.0, "inflate": 0.0, "transpose": 0.0}
    with h5lite.File(counts_path, "r") as cf, h5lite.File(meta_path, "r") as mf:
        for name in H5_PLANES[:10] + ("barcode",):
            if name not in cf:
                raise InvalidInputError(f"{counts_path}: no dataset {name}")
        for name in ("coverage", "reference"):
            if name not in mf:
                raise InvalidInputError(f"{meta_path}: no dataset {name}")
        ds = [cf[p] for p in H5_PLANES[:10]] + [mf["coverage"]]
        L, n = _check_datasets(ds)
        barcodes = _strings(cf["barcode"].read())
        refs = _strings(mf["reference"].read())
        if len(barcodes) != n:
            raise InvalidInputError(f"{counts_path}: {len(barcodes)} barcodes for {n} columns")
        if len(refs) != L:
            raise InvalidInputError(f"{meta_path}: {len(refs)} reference alleles for {L} positions")
        bm = None
        if "barcode_metadata" in mf:
            g = mf["barcode_metadata"]
            bm = {k: g[k].read() for k in g.keys()}
        on_device = not host_inflate and n > 0 and _device_loadable(ds)
        chunks = ds[0].chunks if ds[0].chunks is not None and all(d.chunks == ds[0].chunks for d in ds) \
            else (min(1000, L), max(1, min(100, n)))
        crow, ccol = int(chunks[0]), int(chunks[1])
        nrc, ncc = -(-L // crow), -(-n // ccol)
        step = max(1, int(col_chunks_per_call))
        batches = [(lo, min(ncc, lo + step)) for lo in range(0, ncc, step)]
        eng = Engine.open_table(n, L, device)
        n_sat = 0
        try:
            planes = None
            if not on_device and n:
                t0 = time.perf_counter()
                planes = [d.read() for d in ds]
                seconds["read"] += time.perf_counter() - t0

            def produce(lo, hi):
                t0 = time.perf_counter()
                item = _read_batch(ds, nrc, lo, hi) if on_device else _tiles_of(planes, (crow, ccol), lo, hi)
                seconds["read"] += time.perf_counter() - t0
                return item

            # the reader thread is one batch ahead of the device (it alone calls libhdf5 meanwhile)
            q: Queue = Queue(maxsize=1)

            def reader():
                try:
                    for lo, hi in batches:
                        q.put((lo, hi, produce(lo, hi)))
                except BaseException as e:  # noqa: BLE001 - handed to the consumer
                    q.put(e)

            th = threading.Thread(target=reader, name="mgp-h5-chunks", daemon=True)
            th.start()
            try:
                for _ in batches:
                    item = q.get()
                    if isinstance(item, BaseException):
                        raise item
                    lo, hi, data = item
                    if on_device:
                        out = eng.load(n, (crow, ccol), (lo, hi), lo * ccol, *data)
                    else:
                        out = eng.load_planes(n, (crow, ccol), (lo, hi), lo * ccol, data)
                    n_sat += out["n_saturated"]
                    for k in ("h2d", "inflate", "transpose"):
                        seconds[k] += out[k + "_ms"] * 1e-3
            finally:
                while th.is_alive():  # (an error above: let the reader's pending put through)
                    if not q.empty():
                        q.get()
                    th.join(0.01)
            eng.ready()
        except BaseException:
            eng.close()
            raise
    seconds["total"] = time.perf_counter() - t_start
    if n_sat:
        logger.warning("%d loaded values are 65,535: counts.h5 stores min(count, 65535), so they may be saturated "
                       "counts (as they are for R)", n_sat)
    return LoadedCounts(eng, barcodes, refs, bm, int(n_sat), seconds, on_device)
