"""Variant statistics and heteroplasmy: the host side (analysis/variants.py), its output
files, the CLI options and the ABI additions. No GPU.

The oracle below is a short numpy restatement of the definitions (identify_variants and
calculate_allele_freq of the reference's R functions), working directly from per-cell
arrays: np.corrcoef on the selected cells (NaN -> 0) and np.var(af, ddof=1). It is not
built from the moments. tests/test_gpu_variants.py uses it against the device.

Tolerances. Integer moments, n_cells_detected, n_cells_conf_detected, mean and the
heteroplasmy matrix are integer sums plus one correctly rounded fp64 division: bit-equal.
The variance and the strand correlation get atol = rtol = 16 n 2^-53 (n the population):
af is in [0, 1] and |cor| <= 1, any summation order of n such terms stays within a small
multiple of n 2^-53 absolutely, and 16 is the margin.
"""

from __future__ import annotations

import gzip
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
INT_FIELDS = ("n_det", "n_conf", "s_total", "s_cov", "m", "sf", "sr", "sff", "srr", "sfr", "n_low")
NEW_SYMBOLS = ("mgp_variant_moments_run", "mgp_variant_dev2_run", "mgp_allele_freq_run", "mgp_variant_moments_rows",
               "mgp_variant_dev2_rows", "mgp_allele_freq_rows")


def tol(n: int) -> float:
    return 16.0 * n * 2.0 ** -53


# ---- the oracle ----------------------------------------------------------------------
def population(counts, depth, cells=None):
    """The population's u32 rows: row cells[k] of (counts [n, L, 8], depth [n, L]), zeros for -1."""
    counts, depth = np.asarray(counts), np.asarray(depth)
    if cells is None:
        return counts, depth
    cells = np.asarray(cells, np.int64)
    c = np.zeros((cells.size,) + counts.shape[1:], counts.dtype)
    d = np.zeros((cells.size,) + depth.shape[1:], depth.dtype)
    ok = cells >= 0
    c[ok], d[ok] = counts[cells[ok]], depth[cells[ok]]
    return c, d


def per_cell(counts, depth):
    """f, r [n, L, 4] and cov [n, L] as int64, af [n, L, 4] = (f + r) / cov in fp64 (0 where cov == 0)."""
    f = counts[:, :, 0::2].astype(np.int64)
    r = counts[:, :, 1::2].astype(np.int64)
    cov = depth.astype(np.int64)
    tot = (f + r).astype(np.float64)
    c = np.broadcast_to(cov[:, :, None].astype(np.float64), tot.shape)
    af = np.divide(tot, c, out=np.zeros_like(tot), where=c > 0)
    return f, r, cov, af


def oracle_moments(counts, depth, thr=0):
    """Pass 1's fields straight from the per-cell arrays (exact Python-width integers in uint64)."""
    f, r, cov, af = per_cell(counts, depth)
    sel = f > 0
    low = cov < thr
    u = lambda a: a.astype(np.uint64)  # noqa: E731
    return {
        "n_det": u((f + r > 0).sum(0)), "n_conf": u(((f >= 2) & (r >= 2)).sum(0)), "s_total": u((f + r).sum(0)),
        "s_cov": u(cov.sum(0)), "m": u(sel.sum(0)), "sf": u((f * sel).sum(0)), "sr": u((r * sel).sum(0)),
        "sff": (u(f) * u(f) * sel).sum(0, dtype=np.uint64), "srr": (u(r) * u(r) * sel).sum(0, dtype=np.uint64),
        "sfr": (u(f) * u(r) * sel).sum(0, dtype=np.uint64), "n_low": u(low.sum(0)),
        "s_af": (af * ~low[:, :, None]).sum(0),
    }


def oracle_dev2(counts, depth, mu, thr=0):
    """Pass 2 straight from the per-cell arrays."""
    _, _, cov, af = per_cell(counts, depth)
    keep = ~(cov < thr)[:, :, None]
    return (((af - np.asarray(mu)[None]) ** 2) * keep).sum(0)


def oracle_table(counts, depth, ref, thr=0, min_cells=0, min_strand_cor=0, min_vmr=0):
    """{(0-based position, base): dict(mean, variance, vmr, n_det, n_conf, cor)} of the rows
    identify_variants keeps, and their order (vmr descending, then position, then base)."""
    f, r, cov, af = per_cell(counts, depth)
    n, L = cov.shape
    s_tot, s_cov = (f + r).sum(0), cov.sum(0)
    out = {}
    if n < 2:
        return out, []
    for p in range(L):
        if s_cov[p] == 0:
            continue
        for b in range(4):
            if "ACGT"[b] == ref[p] or s_tot[p, b] == 0:
                continue
            mean = float(s_tot[p, b]) / float(s_cov[p])
            x = np.where(cov[:, p] < thr, mean, af[:, p, b])
            var = float(np.var(x, ddof=1))
            vmr = var / mean
            sel = f[:, p, b] > 0
            cor = 0.0
            if sel.sum() >= 2:
                with np.errstate(divide="ignore", invalid="ignore"):
                    cor = float(np.corrcoef(f[sel, p, b], r[sel, p, b])[0, 1])
                cor = 0.0 if np.isnan(cor) else cor
            n_conf = int(((f[:, p, b] >= 2) & (r[:, p, b] >= 2)).sum())
            if n_conf >= min_cells and cor >= min_strand_cor and vmr > min_vmr:
                out[(p, b)] = dict(mean=mean, variance=var, vmr=vmr, n_det=int((f[:, p, b] + r[:, p, b] > 0).sum()),
                                   n_conf=n_conf, cor=cor)
    order = sorted(out, key=lambda k: (-out[k]["vmr"], k[0], k[1]))
    return out, order


def oracle_allele_freq(counts, depth, pairs, min_coverage=1):
    _, _, cov, af = per_cell(counts, depth)
    return np.stack([np.where(cov[:, p] >= min_coverage, af[:, p, b], 0.0) for p, b in pairs]) if len(pairs) \
        else np.zeros((0, cov.shape[0]))


def check_table(table, want, n, what=""):
    """A VariantTable against oracle_table's rows: the same variants, the exact columns
    bit-equal, variance and correlation within tol(n), vmr = variance / mean exactly, and
    the table's own order."""
    got = table.pairs()
    assert sorted(got) == sorted(want), (what, set(got) ^ set(want))
    t = tol(n)
    for i, k in enumerate(got):
        w = want[k]
        assert table.mean[i] == w["mean"], (what, k)
        assert int(table.n_cells_detected[i]) == w["n_det"] and int(table.n_cells_conf_detected[i]) == w["n_conf"]
        np.testing.assert_allclose(table.variance[i], w["variance"], rtol=t, atol=t, err_msg=f"{what} variance {k}")
        np.testing.assert_allclose(table.strand_correlation[i], w["cor"], rtol=t, atol=t, err_msg=f"{what} cor {k}")
        assert table.vmr[i] == table.variance[i] / table.mean[i]
        assert table.position[i] == k[0] + 1 and table.variant[i] == f"{k[0] + 1}{table.ref[i]}>{'ACGT'[k[1]]}"
        assert table.nucleotide[i] == f"{table.ref[i]}>{'ACGT'[k[1]]}"
    keys = [(-float(v), int(p), int(b)) for v, p, b in zip(table.vmr, table.position, table.base)]
    assert keys == sorted(keys), what


def ref_of(counts):
    """ref_alleles() of the rows' own tally (fwd + rev per base summed over the cells)."""
    from mgatk2_amd.file_io.writers import ref_alleles

    c = np.asarray(counts).astype(np.int64)
    return ref_alleles((c[:, :, 0::2] + c[:, :, 1::2]).sum(0))


def crafted_rows(n=40, L=300, seed=7):
    """u32 rows with the cases that matter: see tests/test_gpu_variants.py::test_crafted_rows."""
    rng = np.random.default_rng(seed)
    counts = np.zeros((n, L, 8), np.uint32)
    refb = rng.integers(0, 4, L)
    for p in range(L):  # the reference allele on both strands, depth 0..60, and sparse alternative reads
        counts[:, p, 2 * refb[p]] = rng.integers(0, 31, n)
        counts[:, p, 2 * refb[p] + 1] = rng.integers(0, 31, n)
        alt = (refb[p] + 1 + rng.integers(0, 3)) % 4
        hit = rng.random(n) < 0.2
        counts[hit, p, 2 * alt] = rng.integers(0, 6, int(hit.sum()))
        counts[hit, p, 2 * alt + 1] = rng.integers(0, 6, int(hit.sum()))

    def alt_of(p, k=1):
        return (refb[p] + k) % 4

    def clear_alts(p):
        for k in (1, 2, 3):
            counts[:, p, 2 * alt_of(p, k):2 * alt_of(p, k) + 2] = 0

    if n >= 40 and L >= 60:  # (smaller sets: the random part only)
        for p in (5, 6, 7, 8, 9, 10):
            clear_alts(p)
        counts[11, 5, 2 * alt_of(5)] = 4  # one cell only: m = 1, correlation 0
        counts[11, 5, 2 * alt_of(5) + 1] = 3
        counts[:10, 6, 2 * alt_of(6)] = 3  # constant f over its cells: vf = 0
        counts[:10, 6, 2 * alt_of(6) + 1] = np.arange(10)
        counts[:12, 7, 2 * alt_of(7)] = np.arange(1, 13)  # perfectly correlated strands
        counts[:12, 7, 2 * alt_of(7) + 1] = 2 * np.arange(1, 13)
        counts[:12, 8, 2 * alt_of(8)] = np.arange(1, 13)  # anti-correlated
        counts[:12, 8, 2 * alt_of(8) + 1] = 50 - np.arange(1, 13)
        counts[20:24, 9, 2 * alt_of(9)] = [70_000, 100_000, 65_536, 3_000_000]  # above 65,535
        counts[20:24, 9, 2 * alt_of(9) + 1] = [90_000, 65_535, 200_000, 2_999_999]
        counts[30:38, 10, 2 * alt_of(10)] = np.arange(2, 10)  # f >= 2, r = 1: detected, not confident
        counts[30:38, 10, 2 * alt_of(10) + 1] = 1
        counts[:, 20] = 0  # an all-zero position: reference "N"
        counts[[3, 17]] = 0  # cells without any coverage
        counts[25:30, 40:60] = 0  # and cells with cov = 0 at some positions
    depth = counts.astype(np.int64).sum(axis=2).astype(np.uint32)
    return counts, depth


# ---- variant_table from numpy-made moments ---------------------------------------------
@pytest.mark.parametrize("thr", [0, 1, 10])
@pytest.mark.parametrize("filters", [(0, 0, 0), (1, 0.3, 0.005), (0, -1.0, 0.0)])
def test_variant_table_matches_the_oracle(thr, filters):
    from mgatk2_amd.analysis.variants import mean_af, variant_table

    counts, depth = crafted_rows()
    n = counts.shape[0]
    ref = ref_of(counts)
    ref[22] = "N"  # a covered position without a reference allele: candidates for all four bases
    mom = oracle_moments(counts, depth, thr)
    dev2 = oracle_dev2(counts, depth, mean_af(mom, n), thr)
    table = variant_table(mom, dev2, ref, n, *filters)
    want, order = oracle_table(counts, depth, ref, thr, *filters)
    assert len(want) > 0
    check_table(table, want, n)
    if filters == (0, -1.0, 0.0):  # (R's default min_strand_cor = 0 drops the anti-correlated rows)
        assert sum(1 for p, _ in want if p == 22) == 2 and ref[20] == "N" and not any(p == 20 for p, _ in want)
        cor = {k: table.strand_correlation[i] for i, k in enumerate(table.pairs())}
        alt = lambda p: next(b for (q, b) in want if q == p)  # noqa: E731
        assert cor[(5, alt(5))] == 0.0 and cor[(6, alt(6))] == 0.0
        assert abs(cor[(7, alt(7))] - 1.0) <= tol(n) and abs(cor[(8, alt(8))] + 1.0) <= tol(n)
        i10 = table.pairs().index((10, alt(10)))
        assert table.n_cells_detected[i10] == 8 and table.n_cells_conf_detected[i10] == 0
    # where no two vmr lie within the tolerance of each other the order is the oracle's
    # (a vmr is its variance, known to tol(n), over the exact mean)
    v = np.array([want[k]["vmr"] for k in order])
    err = np.array([tol(n) * (1.0 + want[k]["variance"]) / want[k]["mean"] for k in order])
    clear = np.abs(np.diff(v)) > err[:-1] + err[1:]
    got = table.pairs()
    for i in np.flatnonzero(clear).tolist():
        assert got.index(order[i]) < got.index(order[i + 1])
    assert clear.sum() >= len(order) // 2


def test_variant_table_drop_rules():
    from mgatk2_amd.analysis.variants import mean_af, variant_table

    counts, depth = crafted_rows(n=6, L=12, seed=3)
    ref = ref_of(counts)
    one = (counts[:1], depth[:1])  # n < 2: nothing
    mom = oracle_moments(*one)
    assert len(variant_table(mom, oracle_dev2(*one, mean_af(mom, 1)), ref, 1)) == 0
    mom = oracle_moments(counts, depth)
    dev2 = oracle_dev2(counts, depth, mean_af(mom, 6))
    full = variant_table(mom, dev2, ref, 6)
    assert len(full) > 0 and len(variant_table(mom, dev2, ref, 6, min_cells=10 ** 6)) == 0
    assert len(variant_table(mom, dev2, ref, 6, min_strand_cor=1.5)) == 0
    assert len(variant_table(mom, dev2, ref, 6, min_vmr=1e9)) == 0
    for p, b in full.pairs():  # never the reference allele, never an uncovered position
        assert "ACGT"[b] != ref[p] and mom["s_cov"][p] > 0 and mom["s_total"][p, b] > 0


def test_strand_correlation_uses_integer_variances():
    from mgatk2_amd.analysis.variants import strand_correlation

    assert strand_correlation(1, 5, 5, 25, 25, 25) == 0.0
    assert strand_correlation(3, 9, 6, 27, 14, 18) == 0.0  # f constant: vf == 0 exactly
    big = 3_000_000  # sums whose float squares would round: the zero test stays exact
    assert strand_correlation(3, 3 * big, 6, 3 * big * big, 14, 6 * big) == 0.0
    f, r = np.array([1, 2, 3, 7]), np.array([2, 1, 5, 9])
    got = strand_correlation(4, f.sum(), r.sum(), (f * f).sum(), (r * r).sum(), (f * r).sum())
    assert abs(got - np.corrcoef(f, r)[0, 1]) <= tol(4)


def test_merge_moments_adds_parts():
    from mgatk2_amd.analysis.variants import mean_af, merge_moments

    counts, depth = crafted_rows(n=10, L=20, seed=5)
    whole = oracle_moments(counts, depth, 10)
    parts = [oracle_moments(counts[:4], depth[:4], 10), oracle_moments(counts[4:], depth[4:], 10)]
    got = merge_moments(parts)
    for k in INT_FIELDS:
        np.testing.assert_array_equal(got[k], whole[k], err_msg=k)
        assert got[k].dtype == np.uint64
    np.testing.assert_array_equal(got["s_af"], parts[0]["s_af"] + parts[1]["s_af"])
    np.testing.assert_allclose(mean_af(got, 10), mean_af(whole, 10), rtol=tol(10), atol=tol(10))


# ---- the output files --------------------------------------------------------------------
def _small_table():
    from mgatk2_amd.analysis.variants import mean_af, variant_table

    counts, depth = crafted_rows(n=9, L=30, seed=11)
    mom = oracle_moments(counts, depth)
    table = variant_table(mom, oracle_dev2(counts, depth, mean_af(mom, 9)), ref_of(counts), 9)
    af = oracle_allele_freq(counts, depth, table.pairs())
    return table, af, [f"BC{j:03d}-1" for j in range(9)]


def test_variant_files_round_trip(tmp_path):
    from mgatk2_amd import h5lite
    from mgatk2_amd.analysis.variants import TSV_COLUMNS, read_variant_stats, write_variant_outputs

    table, af, names = _small_table()
    assert len(table) > 3
    for fmt in ("hdf5", "txt"):
        vdir = write_variant_outputs(table, af, names, tmp_path / fmt, fmt)
        lines = (vdir / "variant_stats.tsv").read_text().splitlines()
        assert lines[0].split("\t") == list(TSV_COLUMNS) and len(lines) == len(table) + 1
        got = read_variant_stats(vdir / "variant_stats.tsv")
        assert got["position"] == table.position.tolist() and got["variant"] == table.variant
        assert got["nucleotide"] == table.nucleotide
        for k in ("mean", "vmr", "strand_correlation"):  # repr: every float comes back bit-equal
            assert got[k] == getattr(table, k).tolist(), k
        assert got["n_cells_detected"] == table.n_cells_detected.tolist()
        assert got["n_cells_conf_detected"] == table.n_cells_conf_detected.tolist()
    with h5lite.File(tmp_path / "hdf5" / "variants" / "allele_freq.h5", "r") as f:
        m = f["allele_freq"][...]
        assert m.dtype == np.float64 and f["allele_freq"].compression == "gzip"
        np.testing.assert_array_equal(m, af)
        assert [x.decode() for x in f["variant"][...].tolist()] == [v.replace(">", "-") for v in table.variant]
        assert [x.decode() for x in f["barcode"][...].tolist()] == names
    assert not (tmp_path / "hdf5" / "variants" / "output.allele_freq.txt.gz").exists()
    text = gzip.decompress((tmp_path / "txt" / "variants" / "output.allele_freq.txt.gz").read_bytes()).decode()
    want = [f"{table.variant[v]},{names[j]},{float(af[v, j])!r}" for v in range(len(table)) for j in range(9)
            if af[v, j] > 0]
    assert text.splitlines() == want and len(want) > 0
    assert [float(ln.rsplit(",", 1)[1]) for ln in text.splitlines()] == [af[v, j] for v in range(len(table))
                                                                         for j in range(9) if af[v, j] > 0]


def test_empty_table_writes_the_header_only(tmp_path):
    from mgatk2_amd.analysis.variants import TSV_COLUMNS, mean_af, variant_table, write_variant_outputs

    counts, depth = crafted_rows(n=9, L=30, seed=11)
    mom = oracle_moments(counts, depth)
    table = variant_table(mom, oracle_dev2(counts, depth, mean_af(mom, 9)), ref_of(counts), 9, min_cells=10 ** 6)
    for fmt in ("hdf5", "txt"):
        vdir = write_variant_outputs(table, np.zeros((0, 9)), ["x"] * 9, tmp_path / fmt, fmt)
        assert (vdir / "variant_stats.tsv").read_text() == "\t".join(TSV_COLUMNS) + "\n"
        assert sorted(p.name for p in vdir.iterdir()) == ["variant_stats.tsv"]


# ---- CLI -----------------------------------------------------------------------------------
def _invoke(monkeypatch, tmp_path, args):
    from click.testing import CliRunner

    from mgatk2_amd import cli as cli_mod
    from mgatk2_amd import pipeline
    from mgatk2_amd.bam import soa_to_bam
    from golden_io import Golden

    g = Golden("kat_run")
    bam = tmp_path / "x.bam"
    if not bam.exists():
        soa_to_bam(bam, g.soa, g.whitelist)
        (tmp_path / "bc.tsv").write_text("".join(b + "\n" for b in g.whitelist))
    seen = {}
    monkeypatch.setattr(pipeline, "run_pipeline", lambda **kw: seen.update(kw) or {})
    r = CliRunner().invoke(cli_mod.cli, [args[0], "-i", str(bam), "-b", str(tmp_path / "bc.tsv"), "-o",
                                         str(tmp_path / "out"), *args[1:]])
    assert r.exit_code == 0, r.output
    return seen


@pytest.mark.parametrize("cmd", ["run", "tenx"])
def test_cli_variant_options_reach_run_pipeline(cmd, tmp_path, monkeypatch):
    seen = _invoke(monkeypatch, tmp_path, [cmd])
    assert seen and not any(k.startswith("variant_") or k == "call_variants" for k in seen)  # off unless asked for
    seen = _invoke(monkeypatch, tmp_path, [cmd, "--variants"])
    assert seen["call_variants"] is True and seen["variant_min_cells"] == 5 and seen["variant_min_strand_cor"] == 0.65
    assert seen["variant_min_vmr"] == 0.01 and seen["variant_stabilize"] is False
    assert seen["variant_low_coverage"] == 10 and seen["variant_min_coverage"] == 1
    seen = _invoke(monkeypatch, tmp_path, [cmd, "--variants", "--variant-min-cells", "2", "--variant-min-strand-cor",
                                           "0.5", "--variant-min-vmr", "0.002", "--variant-stabilize",
                                           "--variant-low-coverage", "7", "--variant-min-coverage", "3"])
    assert (seen["variant_min_cells"], seen["variant_min_strand_cor"], seen["variant_min_vmr"],
            seen["variant_stabilize"], seen["variant_low_coverage"], seen["variant_min_coverage"]) == \
        (2, 0.5, 0.002, True, 7, 3)
    seen = _invoke(monkeypatch, tmp_path, [cmd, "--variants", "--dry-run"])
    assert seen == {} and not (tmp_path / "out" / "variants").exists()


def test_cli_call_takes_the_variant_options(tmp_path, monkeypatch):
    from click.testing import CliRunner

    from mgatk2_amd import cli as cli_mod
    from mgatk2_amd import pipeline
    from mgatk2_amd.bam import soa_to_bam
    from golden_io import Golden

    g = Golden("kat_run")
    (tmp_path / "bams").mkdir()
    soa_to_bam(tmp_path / "bams" / "cell1.bam", g.soa, g.whitelist)
    seen = []
    monkeypatch.setattr(pipeline, "run_pipeline", lambda **kw: seen.append(kw) or {})
    r = CliRunner().invoke(cli_mod.cli, ["call", "-i", str(tmp_path / "bams"), "-o", str(tmp_path / "o"), "--variants",
                                         "--variant-min-cells", "1"])
    assert r.exit_code == 0, r.output
    assert len(seen) == 1 and seen[0]["call_variants"] is True and seen[0]["variant_min_cells"] == 1


def test_pipeline_keywords_default_off(tmp_path):
    import inspect

    from mgatk2_amd.pipeline import MtDNAPipeline, run_pipeline

    want = dict(call_variants=False, variant_min_cells=5, variant_min_strand_cor=0.65, variant_min_vmr=0.01,
                variant_stabilize=False, variant_low_coverage=10, variant_min_coverage=1)
    for fn in (run_pipeline, MtDNAPipeline.__init__):
        sig = inspect.signature(fn).parameters
        assert {k: sig[k].default for k in want} == want


# ---- ABI -----------------------------------------------------------------------------------
def test_header_and_abi_symbols_list_the_new_names():
    from mgatk2_amd import engine

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mgpileup.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(mgp_[a-z_0-9]+)\s*\(", text))
    for s in NEW_SYMBOLS:
        assert s in declared and s in engine.ABI_SYMBOLS, s
    lib = engine.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.mgp_abi_version() == 7


def test_variant_struct_layouts_match_header(tmp_path):
    import ctypes as C

    from mgatk2_amd import engine

    structs = {"mgp_variant_job": engine.mgp_variant_job, "mgp_variant_moments": engine.mgp_variant_moments}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/mgpileup.h"', "int main(){"]
    for name, cls in structs.items():
        lines.append(f'printf("%zu\\n", sizeof({name}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("%zu\\n", offsetof({name}, {fname}));')
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True,
                                          check=True).stdout.split()]
    want = []
    for cls in structs.values():
        want.append(C.sizeof(cls))
        want.extend(getattr(cls, f).offset for f, _ in cls._fields_)
    assert got == want
    assert [f for f, _ in engine.mgp_variant_moments._fields_] == list(engine.MOMENT_FIELDS)
