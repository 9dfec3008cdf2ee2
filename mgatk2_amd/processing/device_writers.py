"""The count files made on the devices at the end of a run, from the rows still in HBM: the txt
files' gzip members (mgp_txt_gz) and the HDF5 datasets' deflated chunks (mgp_h5_tiles). Both
work over the run's :class:`~mgatk2_amd.shard.DeviceParts`, each device making what its own
cells make up, and leave what they made on the run's result for the writers of file_io."""

from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ..engine import H5_PLANES, TXT_FILES, EngineResult
from ..shard import DeviceParts

# cells per mgp_txt_gz call (its device scratch is ~7 GB per 1000 C4 cells)
TXT_CHUNK_CELLS = 2048


def cells_written(res: EngineResult) -> np.ndarray:
    """The passing cells in first-seen order (processors.py:75's write order)."""
    order = res.cell_order()
    return order[res.passed[order].astype(bool)]


def _chunks(cells: np.ndarray):
    return (cells[a:a + TXT_CHUNK_CELLS] for a in range(0, cells.size, TXT_CHUNK_CELLS))


def write_txt(res: EngineResult, parts: DeviceParts, prefix: str, names: list[str]) -> None:
    """The written cells through mgp_txt_gz on their devices, appended to
    `prefix`.{coverage,A,C,G,T}.txt.gz; sets res.txt_gz_cells. With several devices each
    writes its own cells (in the global order, TXT_CHUNK_CELLS per call, the devices
    concurrently) and the members are interleaved back into the global order."""
    written = cells_written(res)

    def members(d, cells):
        return parts[d][0].txt_gz(parts.local(d, cells), [names[c] for c in cells.tolist()])

    files = [open(f"{prefix}.{f}.txt.gz", "ab") for f in TXT_FILES]
    try:
        if len(parts) == 1:
            def put(mem):
                for f in range(5):
                    files[f].write(memoryview(mem.file_part(f)))

            # a chunk's members go to the files while the device makes the next chunk's
            with ThreadPoolExecutor(1) as wr:
                pending = None
                for chunk in _chunks(written):
                    mem = members(0, chunk)
                    if pending is not None:
                        pending.result()
                    pending = wr.submit(put, mem)
                if pending is not None:
                    pending.result()
        else:
            dev = parts.owner(written)
            mems = parts.map(lambda d: [members(d, ch) for ch in _chunks(written[dev == d])])
            rank = np.zeros(written.size, np.int64)  # a cell's index among its part's cells
            for d in range(len(parts)):
                rank[dev == d] = np.arange(int((dev == d).sum()))
            call, k_in = np.divmod(rank, TXT_CHUNK_CELLS)
            order = list(zip(dev.tolist(), call.tolist(), k_in.tolist()))
            for f in range(5):
                views = [[memoryview(m.file_part(f)) for m in ms] for ms in mems]
                offs = [[np.concatenate([[0], np.cumsum(m.member_bytes[f])]).tolist() for m in ms] for ms in mems]
                files[f].writelines(views[d][j][offs[d][j][k]:offs[d][j][k + 1]]
                                    for d, j, k in order if offs[d][j][k + 1] > offs[d][j][k])
    finally:
        for fh in files:
            fh.close()
    res.txt_gz_cells = written


def write_h5(res: EngineResult, parts: DeviceParts, names: list[str], L: int) -> None:
    """The written cells' columns (hdf5_columns over `names`, the writer's barcodes), their
    chunks deflated on the devices; sets res.h5_tiles. A column chunk whose cells lie on one
    device is made there; one that spans two devices' cells (at most one per boundary) is
    deflated on the host from the fetched rows."""
    from ..bam import h5_plane_tiles
    from ..file_io.writers import hdf5_cell_of_col, hdf5_columns

    sel, cols = hdf5_columns(names, names, cells_written(res))
    if not (len(names) and sel.size):
        return
    n = len(names)
    coc = hdf5_cell_of_col(n, sel, cols)
    chunks = (min(1000, L), min(100, n))
    crow, ccol = chunks
    nrc, ncc = -(-L // crow), -(-n // ccol)
    maker = np.zeros(ncc, np.int64)  # the part making each column chunk, -1: the host
    for cc in range(ncc):
        v = coc[cc * ccol:(cc + 1) * ccol]
        v = v[v >= 0]
        if v.size:
            d = parts.owner(v)
            maker[cc] = d[0] if np.all(d == d[0]) else -1
    tiles = {p: [None] * (nrc * ncc) for p in H5_PLANES}
    total = np.zeros((3, L), np.int64)

    def runs(d):  # (c0, c1) runs of consecutive column chunks of part d
        idx = np.flatnonzero(maker == d)
        if not idx.size:
            return []
        cut = np.flatnonzero(np.diff(idx) > 1) + 1
        return [(int(g[0]), int(g[-1]) + 1) for g in np.split(idx, cut)]

    def one(d):
        local = parts.local(d, coc)
        out = []
        for c0, c1 in runs(d):
            sums = {}
            out.append((c0, c1, parts[d][0].h5_tiles(local, chunks, sums=sums, col_chunks=(c0, c1)), sums))
        return out

    for got in parts.map(one):
        for c0, c1, tl, sums in got:
            w = c1 - c0
            for p in H5_PLANES:
                src = tl[p]
                for rc in range(nrc):
                    tiles[p][rc * ncc + c0:rc * ncc + c1] = src[rc * w:(rc + 1) * w]
            total += np.stack([sums["coverage"], sums["tn5_fwd"], sums["tn5_rev"]])
    for cc in np.flatnonzero(maker < 0).tolist():  # chunks across a device boundary
        sub = coc[cc * ccol:(cc + 1) * ccol]
        made_h = (h5_plane_tiles(res.counts, sub, list(range(8)), chunks, level=4)
                  + h5_plane_tiles(res.tn5, sub, [0, 1], chunks, level=4)
                  + h5_plane_tiles(res.depth, sub, [0], chunks, level=4))
        for p, lst in zip(H5_PLANES, made_h):
            for rc in range(nrc):
                tiles[p][rc * ncc + cc] = lst[rc]
        ok = sub[sub >= 0]
        total[0] += np.minimum(res.depth[ok], 65535).astype(np.int64).sum(axis=0)
        total[1] += np.minimum(res.tn5[ok, :, 0], 65535).astype(np.int64).sum(axis=0)
        total[2] += np.minimum(res.tn5[ok, :, 1], 65535).astype(np.int64).sum(axis=0)
    res.h5_tiles = (coc, chunks, tiles, {"coverage": total[0], "tn5_fwd": total[1], "tn5_rev": total[2]})
