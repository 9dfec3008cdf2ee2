"""GPU: the paced rows kernels (k_rows_to_host / k_rows_to_host8 with MGP_ROWS_SPREAD).

A streaming segment's rows leave on a schedule (a fraction of the interval between two
segments' rows kernels); the run's last segment and a resident run's rows run free. The
rows must be what they were, whatever the schedule: small odd shapes (mito_len 2601: three
windows of 872, 872 and 857 positions, so a window starts off every line and the last is
short), fewer cells than the grid and a count it does not divide, streamed in 4 batches and
resident, twice on one context, with MGP_ROWS_SPREAD at 0 (unpaced), unset (the default) and
0.9. Guard bytes around every plane of both pinned targets stay untouched."""

from __future__ import annotations

import functools
from dataclasses import replace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 2601
RUN = dict(min_baseq=20, min_mapq=30, dedup_mode="alignment_and_fragment_length", min_reads=1)
GUARD = 64
FILL = 0xAB
SPREADS = ["0", None, "0.9"]  # MGP_ROWS_SPREAD (None: unset, the default)


@functools.lru_cache(maxsize=None)
def _case(nc):
    """The reads of `nc` cells at 40-320 depth (as test_rows8_target_equals_the_exact_rows:
    800k reads for 8 cells of 16569 positions) and their exact resident results, ungated
    and gated at the median read count; computed once per cell count."""
    from mgatk2_amd import engine
    from mgatk2_amd.synth import synth_reads

    soa = synth_reads(717, max(2000, 800_000 * nc * L // (8 * 16569)), nc, mito_len=L, pack=True)
    cfg = engine.EngineConfig(n_cells=nc, mito_len=L, **RUN)
    with engine.Engine(cfg) as eng:
        eng.push(soa)
        eng.run()
        ungated = eng.fetch()
        nw, W = eng.windows()
    assert (nw, W) == (3, 872) and L - 2 * W == 857
    big = np.maximum(ungated.depth, ungated.tn5.max(axis=2))
    fits = np.array([[big[c, k * W:(k + 1) * W].max() <= 255 for k in range(nw)] for c in range(nc)])
    gcfg = replace(cfg, min_reads=max(2, int(np.sort(ungated.n_reads)[nc // 2])))
    with engine.Engine(gcfg) as eng:
        eng.push(soa)
        eng.run()
        gated = eng.fetch()
    for a in (ungated, gated):
        for k in ("counts", "tn5", "depth"):
            getattr(a, k).setflags(write=False)
    return soa, cfg, gcfg, ungated, gated, fits, nw, W


class Guarded:
    """Arrays in one pinned buffer, each plane on a 64-byte line of its own with GUARD
    bytes before and after it; everything prefilled with FILL."""

    def __init__(self, planes):
        from mgatk2_amd.engine import PinnedBuffer

        off, self.spans = GUARD, []
        for shape, dt in planes:
            nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
            self.spans.append((off, nbytes, shape, dt))
            off = (off + nbytes + GUARD + 63) // 64 * 64
        self.buf = PinnedBuffer(off)
        self.raw = self.buf.array((off,), np.uint8, 0)
        self.arrays = [self.buf.array(shape, dt, o) for o, _, shape, dt in self.spans]

    def fill(self):
        self.raw.fill(FILL)

    def check_guards(self, what):
        mask = np.ones(self.raw.shape[0], bool)
        for o, nbytes, _, _ in self.spans:
            mask[o:o + nbytes] = False
        assert mask.sum() >= GUARD * (len(self.spans) + 1)
        assert (self.raw[mask] == FILL).all(), f"{what}: bytes outside the planes were written"


def _targets(nc, nw, W, with8):
    from mgatk2_amd.engine import Rows8, Rows16

    planes = [((nc, L, 8), np.uint16), ((nc, L, 2), np.uint16), ((nc, L), np.uint16), ((nc, nw), np.uint8)]
    if with8:
        planes += [((nc, L, 8), np.uint8), ((nc, L, 2), np.uint8), ((nc, L), np.uint8), ((nc, nw), np.uint8)]
    g = Guarded(planes)
    t16 = Rows16(*g.arrays[:4], W)
    t8 = Rows8(*g.arrays[4:]) if with8 else None
    return g, t16, t8


def _set_spread(monkeypatch, spread):
    if spread is None:
        monkeypatch.delenv("MGP_ROWS_SPREAD", raising=False)
    else:
        monkeypatch.setenv("MGP_ROWS_SPREAD", spread)


def _run_twice(engine_lib, cfg, soa, streamed, t16, t8, g, check):
    scfg = replace(cfg, stream=True, reserve_reads=soa.n, reserve_payload=int(soa.payload.shape[0]) + 4096) \
        if streamed else cfg
    with engine_lib.Engine(scfg) as eng:
        if t8 is None:
            eng.set_rows16_target(t16)
        else:
            eng.set_rows_target(t16, t8)
        for rep in range(2):
            g.fill()
            eng.reset()
            cuts = np.linspace(0, soa.n, 5).astype(int)
            for a, b in zip(cuts[:-1], cuts[1:]):
                eng.push(soa.slice(int(a), int(b)))
            eng.run()
            got = eng.fetch()
            if streamed:
                assert eng.stream_info()[1], "the run did not stream"
            check(got, f"rep {rep}")
            g.check_guards(f"rep {rep}")
        if t8 is None:
            eng.set_rows16_target(None)
        else:
            eng.set_rows_target(None)


@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("streamed", [False, True])
@pytest.mark.parametrize("nc", [1, 3, 67])
def test_paced_rows_equal_the_exact_rows(engine_lib, monkeypatch, nc, streamed, spread):
    """Both targets: every (cell, window) in exactly one of them, `narrow` iff its values
    fit a byte, nothing wide; the merged rows equal the exact u32 rows of a resident run."""
    from mgatk2_amd.engine import merge_rows

    soa, cfg, _, want, _, fits, nw, W = _case(nc)
    if nc >= 3:
        assert fits.any() and not fits.all()  # both kinds of window
    _set_spread(monkeypatch, spread)
    g, t16, t8 = _targets(nc, nw, W, True)

    def check(got, what):
        np.testing.assert_array_equal(t8.narrow.astype(bool), fits, err_msg=f"narrow flags {what}")
        assert not t16.wide.any()
        m = merge_rows(t16, t8, 0, nc)
        for k in ("counts", "tn5", "depth"):
            np.testing.assert_array_equal(m[k], getattr(want, k), err_msg=f"{k} {what}")
            np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=f"fetch {k} {what}")

    _run_twice(engine_lib, cfg, soa, streamed, t16, t8, g, check)


@pytest.mark.parametrize("spread", SPREADS)
def test_paced_rows16_target_alone(engine_lib, monkeypatch, spread):
    """The 16-bit target alone (k_rows_to_host, the product's streamed path)."""
    nc = 67
    soa, cfg, _, want, _, _, nw, W = _case(nc)
    _set_spread(monkeypatch, spread)
    g, t16, _ = _targets(nc, nw, W, False)

    def check(got, what):
        assert not t16.wide.any()
        np.testing.assert_array_equal(t16.counts, want.counts, err_msg=f"counts {what}")
        np.testing.assert_array_equal(t16.tn5, want.tn5, err_msg=f"tn5 {what}")
        np.testing.assert_array_equal(t16.depth, want.depth, err_msg=f"depth {what}")

    _run_twice(engine_lib, cfg, soa, True, t16, None, g, check)


@pytest.mark.parametrize("spread", SPREADS)
def test_paced_rows_with_the_gate(engine_lib, monkeypatch, spread):
    """min_reads at the cells' median read count: k_gate_fixup zeroes the dropped cells'
    rows in the targets after the paced stores of the earlier segments."""
    from mgatk2_amd.engine import merge_rows

    nc = 67
    soa, _, gcfg, _, want, fits, nw, W = _case(nc)
    assert (want.passed == 0).any() and want.passed.any()
    _set_spread(monkeypatch, spread)
    g, t16, t8 = _targets(nc, nw, W, True)

    def check(got, what):
        np.testing.assert_array_equal(t8.narrow.astype(bool), fits, err_msg=f"narrow flags {what}")
        assert not t16.wide.any()
        m = merge_rows(t16, t8, 0, nc)
        for k in ("counts", "tn5", "depth"):
            np.testing.assert_array_equal(m[k], getattr(want, k), err_msg=f"{k} {what}")
        np.testing.assert_array_equal(got.passed, want.passed, err_msg=f"passed {what}")

    _run_twice(engine_lib, gcfg, soa, True, t16, t8, g, check)
