"""The host plumbing around a run's devices, with bare objects for engines: shard.DeviceParts
(global cell indices onto (engine, lo, hi) ranges), the streamed paths' rows-target helper,
the seconds CellProcessor._after_run reports and EngineResult's declared run fields. CPU only."""

from __future__ import annotations

import threading

import numpy as np
import pytest

from mgatk2_amd.engine import EngineResult, Rows16
from mgatk2_amd.exceptions import InvalidInputError
from mgatk2_amd.shard import DeviceParts

BOUNDS = [0, 3, 3, 7]  # three parts, the middle one empty


def _parts(bounds=BOUNDS):
    return DeviceParts([(object(), lo, hi) for lo, hi in zip(bounds[:-1], bounds[1:])])


def test_parts_iterate_as_tuples():
    engines = [object(), object()]
    parts = DeviceParts([(engines[0], np.int64(0), np.int64(4)), (engines[1], 4, 9)])
    assert [(e, lo, hi) for e, lo, hi in parts] == [(engines[0], 0, 4), (engines[1], 4, 9)]
    assert len(parts) == 2 and parts[1] == (engines[1], 4, 9)
    assert list(DeviceParts(parts)) == list(parts)
    np.testing.assert_array_equal(parts.all_cells(), np.arange(9))
    assert parts.all_cells().dtype == np.int64


def test_no_parts_is_refused():
    with pytest.raises(InvalidInputError, match="^identify_variants: no device parts$"):
        DeviceParts([])


@pytest.mark.parametrize("max_cells", [None, 2])
def test_split(max_cells):
    parts = _parts()
    cells = np.array([5, -1, 0, 2, 5, 6, -1, 3, 1, 0, 4, 2, -1], np.int64)  # repeats, zero rows, out of order
    calls = parts.split(cells) if max_cells is None else parts.split(cells, max_cells)
    assert len(calls) == 3 and calls[1] == []
    seen = []
    for d, ((_, lo, hi), chunks) in enumerate(zip(parts, calls)):
        assert np.all(np.diff(np.concatenate([ix for ix, _ in chunks] + [[]])) > 0)  # in population order
        for ix, loc in chunks:
            assert ix.size == loc.size and loc.dtype == np.int32
            assert max_cells is None or ix.size <= max_cells
            own = cells[ix]
            np.testing.assert_array_equal(loc, np.where(own >= 0, own - lo, -1))
            assert np.all((own < 0) | ((own >= lo) & (own < hi)))
            assert d == 0 or np.all(own >= 0)  # the zero rows go with the first part
            seen.append(ix)
    np.testing.assert_array_equal(np.sort(np.concatenate(seen)), np.arange(cells.size))  # each exactly once
    if max_cells == 2:
        assert [len(ch) for ch in calls] == [4, 0, 3]  # 8 and 5 cells in calls of 2


def test_split_empty_population():
    assert _parts().split(np.zeros(0, np.int64)) == [[], [], []]


def test_split_refuses_a_cell_of_no_part():
    with pytest.raises(InvalidInputError,
                       match="^identify_variants: a cell of the population is on no device part$"):
        _parts().split(np.array([0, 7], np.int64))


@pytest.mark.parametrize("bounds", [BOUNDS, [0, 5], [2, 4, 9, 10]])
def test_owner_and_local_against_a_loop(bounds):
    parts = _parts(bounds)
    cells = np.arange(bounds[0], bounds[-1], dtype=np.int64)  # every lo and every hi - 1 among them
    want = np.array([next(d for d, (_, lo, hi) in enumerate(parts) if lo <= c < hi) for c in cells.tolist()])
    np.testing.assert_array_equal(parts.owner(cells), want)
    mixed = np.concatenate([cells[::-1], [-1, bounds[-1], bounds[-1] + 5]])
    for d, (_, lo, hi) in enumerate(parts):
        loop = np.array([c - lo if lo <= c < hi else -1 for c in mixed.tolist()])
        np.testing.assert_array_equal(parts.local(d, mixed), loop)


def test_map_keeps_part_order_and_raises():
    one = _parts([0, 4])
    assert one.map(lambda d: threading.current_thread()) == [threading.current_thread()]  # serial
    parts = _parts()
    gate = threading.Barrier(3)  # (passes only if the three parts run concurrently)

    def fn(d):
        gate.wait(timeout=30)
        return 10 * d

    assert parts.map(fn) == [0, 10, 20]

    def failing(d):
        if d == 1:
            raise KeyError("part 1")
        return d

    with pytest.raises(KeyError, match="part 1"):
        parts.map(failing)


# ---- the rows target of the streamed paths ----------------------------------------------------

def test_rows_target_layout(monkeypatch):
    from test_pipeline import HostBuf

    from mgatk2_amd.processing import processors

    monkeypatch.setattr(processors, "PinnedBuffer", HostBuf)
    n, L, nw = 5, 40, 3
    rows = processors._RowsTarget(n, L, (nw, 16)).take()
    assert isinstance(rows, Rows16) and rows.window_width == 16
    assert [(a.shape, a.dtype) for a in (rows.counts, rows.tn5, rows.depth, rows.wide)] == \
        [((n, L, 8), np.uint16), ((n, L, 2), np.uint16), ((n, L), np.uint16), ((n, nw), np.uint8)]
    for k, a in enumerate((rows.counts, rows.tn5, rows.depth, rows.wide)):  # four disjoint arrays
        a[...] = k + 1
    assert [int(a.min()) for a in (rows.counts, rows.tn5, rows.depth, rows.wide)] == [1, 2, 3, 4]
    view = processors._rows_slice(rows, 1, 3)
    assert view.counts.shape == (2, L, 8) and view.wide.shape == (2, nw) and view.window_width == 16
    assert np.shares_memory(view.depth, rows.depth[1:3])


def test_rows_target_raises_at_the_take(monkeypatch):
    """The allocator's exception is the caller's when it takes the rows, and `ready` answers
    without waiting for the allocation."""
    from mgatk2_amd.processing import processors

    started, release = threading.Event(), threading.Event()

    class Failing:
        def __init__(self, nbytes):
            started.set()
            assert release.wait(timeout=30)
            raise MemoryError("no pinned memory")

    monkeypatch.setattr(processors, "PinnedBuffer", Failing)
    target = processors._RowsTarget(4, 10, (1, 1275))  # (nothing is raised on this thread yet)
    assert started.wait(timeout=30)
    assert target.ready() is False  # the allocation is still held up: answered at once
    release.set()
    with pytest.raises(MemoryError, match="no pinned memory"):
        target.take()
    assert target.ready() is True
    with pytest.raises(MemoryError, match="no pinned memory"):  # every device thread sees it
        target.take()


# ---- the post-run tail's seconds and the result's declared fields ------------------------------

def test_after_run_reports_the_enabled_steps(tmp_path):
    from mgatk2_amd.config import PipelineConfig
    from mgatk2_amd.processing.processors import CellProcessor

    res = EngineResult.alloc(3, 8, dense=False)
    parts = [(object(), 0, 3)]
    proc = CellProcessor(PipelineConfig(), tmp_path)
    assert proc._after_run(res, parts) == {"txt_device": 0.0, "h5_device": 0.0}
    assert proc._after_run(res, parts, writers=False) == {}
    proc.enable_coverage()
    proc.enable_variants()
    assert set(proc._after_run(res, [])) == {"txt_device", "h5_device", "coverage", "variants"}
    assert set(proc._after_run(res, [], writers=False)) == {"coverage", "variants"}
    assert res.coverage is None and res.variants is None  # a run without cells has no parts: nothing made


def test_result_declares_the_run_fields():
    res = EngineResult.alloc(2, 4)
    for k in ("txt_gz_cells", "h5_tiles", "coverage", "variants", "allele_freq", "variant_cells", "variant_seconds",
              "clusters", "neighbors"):
        assert getattr(res, k) is None, k
    positional = EngineResult(*[getattr(res, k) for k in ("counts", "tn5", "depth", "n_reads", "any_paired", "passed",
                                                          "covered", "depth_sum", "depth_max", "median_lo",
                                                          "median_hi", "first_read", "ref_tally", "stats")])
    assert positional.variants is None and positional.h5_tiles is None
