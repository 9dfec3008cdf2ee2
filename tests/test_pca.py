"""Principal components of the heteroplasmy matrix, host side (no GPU): the Python model of mgp_pca's definition
(tests/pca_model.py) against numpy, the ABI and its refusals, the options and checkers, and the file writers.

tests/test_gpu_pca.py compares the device with the model.
"""

from __future__ import annotations

import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import pca_model
from test_cluster import _cli

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("mgp_pca", "mgp_sym_eig")
PCA_FILES = ["variants/cell_pca.tsv", "variants/pca_variance.tsv", "variants/variant_loadings.tsv"]
ULP = 2.0 ** -52


def planted_matrix(n, m, rank, noise, seed):
    """x [m][n]: a rank-`rank` part (unit-scale factors times descending weights) plus noise."""
    rng = np.random.default_rng(seed)
    w = np.array([3.0, 2.0, 1.5, 1.2, 1.0, 0.8][:rank])
    x = (rng.standard_normal((m, rank)) * w) @ rng.standard_normal((rank, n))
    return x + noise * rng.standard_normal((m, n))


# ---- the model against numpy -------------------------------------------------------------
@pytest.mark.parametrize("scale", [False, True])
def test_model_against_numpy(scale):
    """On a 40 x 6 planted matrix the model's cov equals numpy.cov and its scores from numpy.linalg.eigh's
    vectors (sign rule applied) equal the matrix product, within 4 ulp-scale relative error: 4 * 2^-52 relative
    to the sum of the magnitudes of the terms each number is a sum of (the scale at which two orders of the
    same sum differ), the model's own z standing for both sides' terms."""
    n, m = 40, 6
    x = planted_matrix(n, m, 2, 0.05, 7)
    mod = pca_model.model(x, scale)
    z, cov = mod["z"], mod["cov"]
    ref_z = x - x.mean(axis=1, keepdims=True)
    np.testing.assert_allclose(mod["mean"], x.mean(axis=1), rtol=0, atol=4 * ULP * np.abs(x).sum(axis=1).max() / n)
    if scale:
        ref_z = ref_z / x.std(axis=1, ddof=1, keepdims=True)
        np.testing.assert_allclose(mod["sd"], x.std(axis=1, ddof=1), rtol=4 * ULP)
    np.testing.assert_allclose(z, ref_z, rtol=0, atol=4 * ULP * np.abs(x).max() / (mod["sd"].min() if scale else 1.0))
    ref_cov = np.cov(ref_z)
    assert np.all(np.abs(cov - ref_cov) <= 4 * ULP * (np.abs(z) @ np.abs(z).T) / (n - 1))
    assert np.array_equal(cov, cov.T)
    w, v = np.linalg.eigh(cov)
    w, vec = pca_model.order_and_sign(w, v.T)
    assert np.all(np.diff(w) <= 0) and pca_model.sign_rule_holds(vec)
    got = pca_model.scores(z, vec[:3])
    want = vec[:3] @ ref_z
    assert got.shape == (3, n) and np.all(np.abs(got - want) <= 4 * ULP * (np.abs(vec[:3]) @ np.abs(z)))


def test_model_order_sign_and_zero_signs():
    w, v = pca_model.order_and_sign([1.0, 3.0, 1.0, -2.0], [[1, -2, 2], [-3, 1, 3], [0.5, 0.5, -0.5], [0, -1, 0]])
    assert w.tolist() == [3.0, 1.0, 1.0, -2.0]
    # ties keep the lower index first; the largest magnitude's lowest index decides the sign
    assert v.tolist() == [[3, -1, -3], [-1, 2, -2], [0.5, 0.5, -0.5], [0, 1, 0]]
    assert pca_model.sign_rule_holds(v) and not pca_model.sign_rule_holds([[1, -2]])
    assert pca_model.fma(0.0, 5.0, -0.0).hex() == (0.0 * 5.0 + -0.0).hex()
    assert np.signbit(pca_model.fma(-0.0, 5.0, -0.0)) and not np.signbit(pca_model.fma(2.0, 3.0, -6.0))
    assert pca_model.fma(1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0) == 2.0 ** -29 + 2.0 ** -60  # one rounding
    # a slab is 1,024 items: 1,025 ones are 1024 + 1, each slab from 0.0
    big = np.full((1, 1025), 0.1)
    assert pca_model.means(big)[0] == (sum([0.1] * 1024) + 0.1) / 1025


# ---- ABI -----------------------------------------------------------------------------------
def test_header_and_abi_symbols_list_the_new_names():
    from mgatk2_amd import engine
    from mgatk2_amd.build import HIP_SOURCES, build_engine

    assert "mgp_pca.hip" in HIP_SOURCES
    build_engine()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mgpileup.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(mgp_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    for s in NEW_SYMBOLS:
        assert s in declared and s in engine.ABI_SYMBOLS and hasattr(lib, s), s
        assert not s.endswith("_rows")
    assert lib.mgp_abi_version() == engine.ABI_VERSION == 7
    assert callable(engine.pca) and callable(engine.sym_eig)
    assert "EngineResult" in dir(engine) and engine.EngineResult.alloc(1, 4).pca is None


def test_pca_calls_refuse_bad_arguments_before_any_device_call():
    """Null or negative arguments and sizes outside the bounds: MGP_E_INVALID with the call's own message,
    before any allocation or device call (so this runs without a device)."""
    import ctypes as C

    from mgatk2_amd import engine
    from mgatk2_amd.build import build_engine

    build_engine()
    lib = engine.load_library()
    n, m, k = 6, 3, 2
    x = np.zeros((m, n))
    mean, sd, eig, cov = np.full(m, -7.0), np.full(m, -7.0), np.full(m, -7.0), np.full((m, m), -7.0)
    load, sc = np.full((k, m), -7.0), np.full((k, n), -7.0)
    sweeps = C.c_int32(99)
    p = lambda a: a.ctypes.data  # noqa: E731
    sw = C.byref(sweeps)

    def refused(name, text, *args):
        rc = getattr(lib, name)(0, *args)
        assert rc == engine.MGP_E_INVALID, (name, args, rc)
        assert lib.mgp_last_error().decode().startswith(f"{name}: {text}"), (name, args, lib.mgp_last_error())

    # mgp_pca(device, x, n, m, scale, n_comp, mean, sd, eig, loadings, scores, cov, sweeps)
    outs = (p(mean), p(sd), p(eig), p(load), p(sc), p(cov), sw)
    for at in (0, 2, 3, 4, 6):  # mean, eig, loadings, scores, sweeps: never optional
        bad = list(outs)
        bad[at] = None
        refused("mgp_pca", "bad arguments", p(x), n, m, 0, k, *bad)
    refused("mgp_pca", "bad arguments", None, n, m, 0, k, *outs)
    refused("mgp_pca", "bad arguments", p(x), n, m, 1, k, p(mean), None, *outs[2:])  # sd with scale
    refused("mgp_pca", "bad arguments", p(x), -n, m, 0, k, *outs)
    refused("mgp_pca", "bad arguments", p(x), n, -m, 0, k, *outs)
    refused("mgp_pca", "more than 2^20 items in one call", p(x), (1 << 20) + 1, m, 0, k, *outs)
    refused("mgp_pca", "more than 2048 features in one call", p(x), n, 2049, 0, k, *outs)
    for few in (0, 1):
        refused("mgp_pca", "at least 2 items are needed", p(x), few, m, 0, k, *outs)
    for kk in (0, -1):
        refused("mgp_pca", "n_comp must be at least 1", p(x), n, m, 0, kk, *outs)
    for nn, mm, kk in ((n, m, m + 1), (3, m, 3), (2, m, 2), (n, 0, 1)):
        refused("mgp_pca", "n_comp must be at most min(n_feat, n_items - 1)", p(x), nn, mm, 0, kk, *outs)
    # mgp_sym_eig(device, a, m, eig, vec, sweeps)
    a, vec = np.eye(m), np.full((m, m), -7.0)
    for args in ((None, m, p(eig), p(vec), sw), (p(a), m, None, p(vec), sw), (p(a), m, p(eig), None, sw),
                 (p(a), m, p(eig), p(vec), None), (p(a), -1, p(eig), p(vec), sw), (None, 0, None, None, None)):
        refused("mgp_sym_eig", "bad arguments", *args)
    refused("mgp_sym_eig", "more than 2048 features in one call", p(a), 2049, p(eig), p(vec), sw)
    for out in (mean, sd, eig, cov, load, sc, vec):
        assert np.all(out == -7.0)
    # m = 0: nothing is launched (so this too runs without a device)
    assert lib.mgp_sym_eig(0, None, 0, None, None, sw) == engine.MGP_OK and sweeps.value == 0
    # the wrappers pass a refusal on as InvalidInputError without allocating for it
    from mgatk2_amd.exceptions import InvalidInputError

    for call in (lambda: engine.pca(np.zeros((2, 5)), 3), lambda: engine.pca(np.zeros((2, 1)), 1),
                 lambda: engine.sym_eig(np.zeros((2, 3)))):
        with pytest.raises(InvalidInputError):
            call()


# ---- options and checkers ------------------------------------------------------------------
def test_check_pca_ranges():
    from mgatk2_amd.analysis.pca import PCA_MAX_COMP, check_pca
    from mgatk2_amd.exceptions import InvalidInputError

    assert PCA_MAX_COMP == 50
    assert [check_pca(v) for v in (1, 5, 50, "7", 3.0, np.int64(9))] == [1, 5, 50, 7, 3, 9]
    for bad in (0, -1, 51, 2.5, "x", None, True):
        with pytest.raises(InvalidInputError):
            check_pca(bad)


@pytest.mark.parametrize("cmd", ["run", "tenx"])
def test_cli_pca_options(cmd, tmp_path, monkeypatch):
    r, seen = _cli(tmp_path, monkeypatch, [cmd, "--variants"])
    assert r.exit_code == 0 and "pca" not in seen and "pca_scale" not in seen  # off unless asked for
    r, seen = _cli(tmp_path, monkeypatch, [cmd, "--variants", "--pca", "5"])
    assert r.exit_code == 0 and seen["pca"] == 5 and "pca_scale" not in seen
    r, seen = _cli(tmp_path, monkeypatch, [cmd, "--variants", "--pca", "50", "--pca-scale"])
    assert r.exit_code == 0 and seen["pca"] == 50 and seen["pca_scale"] is True
    for args, text in ((["--pca", "5"], "--pca requires --variants"),
                       (["--variants", "--pca-scale"], "--pca-scale requires --pca"),
                       (["--variants", "--pca", "0"], "--pca"), (["--variants", "--pca", "51"], "--pca")):
        r, seen = _cli(tmp_path, monkeypatch, [cmd, *args])
        assert r.exit_code == 2 and text in r.output and seen == {}, (args, r.output)
    r, _ = _cli(tmp_path, monkeypatch, [cmd, "--help"])
    assert "--pca" in r.output and "--pca-scale" in r.output


def test_cli_call_and_analyze_take_the_pca_options(tmp_path, monkeypatch):
    from click.testing import CliRunner

    from golden_io import Golden
    from mgatk2_amd import cli as cli_mod
    from mgatk2_amd import pipeline
    from mgatk2_amd.bam import soa_to_bam

    g = Golden("kat_run")
    (tmp_path / "bams").mkdir()
    soa_to_bam(tmp_path / "bams" / "cell1.bam", g.soa, g.whitelist)
    seen = []
    monkeypatch.setattr(pipeline, "run_pipeline", lambda **kw: seen.append(kw) or {})
    monkeypatch.setattr(pipeline, "analyze_outputs", lambda *a, **kw: seen.append(kw) or {})
    call = ["call", "-i", str(tmp_path / "bams"), "-o", str(tmp_path / "o")]
    analyze = ["analyze", "-i", str(tmp_path)]
    for base in (call, analyze):
        seen.clear()
        r = CliRunner().invoke(cli_mod.cli, [*base, "--variants", "--pca", "4", "--pca-scale"])
        assert r.exit_code == 0, r.output
        assert len(seen) == 1 and seen[0]["pca"] == 4 and seen[0]["pca_scale"] is True
        for args, text in ((["--pca", "5"], "--pca requires --variants"),
                           (["--variants", "--pca-scale"], "--pca-scale requires --pca")):
            r = CliRunner().invoke(cli_mod.cli, [*base, *args])
            assert r.exit_code == 2 and text in r.output and len(seen) == 1, (base[0], args, r.output)
        r = CliRunner().invoke(cli_mod.cli, [base[0], "--help"])
        assert "--pca" in r.output and "--pca-scale" in r.output


def test_cli_dry_run_prints_the_setting(tmp_path, monkeypatch, caplog):
    import logging

    with caplog.at_level(logging.INFO, logger="mgatk2_amd"):
        r, seen = _cli(tmp_path, monkeypatch, ["run", "--variants", "--pca", "7", "--pca-scale", "--dry-run"])
    assert r.exit_code == 0 and seen == {}
    assert "Principal components:   7, scaled True" in caplog.text


def test_pipeline_keywords_default_off_and_checked(tmp_path):
    from mgatk2_amd.exceptions import InvalidInputError
    from mgatk2_amd.pipeline import MtDNAPipeline, analyze_outputs, pca_settings, run_pipeline
    from mgatk2_amd.processing.processors import CellProcessor

    # (analysis_settings' keywords end with the groups', pinned by tests/test_group_tests.py: the PCA's are
    # checked beside them by pca_settings, which the three entry points call)
    for fn in (run_pipeline, MtDNAPipeline.__init__, pca_settings):
        sig = inspect.signature(fn).parameters
        assert list(sig)[-2:] == ["pca", "pca_scale"]  # appended after the existing keywords
        assert sig["pca"].default is None and sig["pca_scale"].default is False
    sig = inspect.signature(analyze_outputs).parameters
    assert sig["pca"].default is None and sig["pca_scale"].default is False
    assert pca_settings() == {"pca": None, "pca_scale": False}
    assert pca_settings(True, pca="5", pca_scale=1) == {"pca": 5, "pca_scale": True}
    for kw in (dict(pca=5), dict(call_variants=True, pca=0), dict(call_variants=True, pca=51),
               dict(call_variants=True, pca_scale=True)):
        with pytest.raises(InvalidInputError):
            pca_settings(**kw)
        with pytest.raises(InvalidInputError):
            MtDNAPipeline("no.bam", ["A"], tmp_path, **kw)
        with pytest.raises(InvalidInputError):
            analyze_outputs(tmp_path, **kw)
    (tmp_path / "bc.tsv").write_text("A\n")
    with pytest.raises(InvalidInputError, match="pca requires call_variants"):
        run_pipeline("no.bam", str(tmp_path / "bc.tsv"), str(tmp_path), pca=5)
    with pytest.raises(InvalidInputError, match="pca requires call_variants"):
        analyze_outputs(tmp_path, pca=5)
    proc = CellProcessor(None, tmp_path)
    assert proc.pca_opt is None and proc.pca_result(None) is None
    with pytest.raises(InvalidInputError, match="pca requires call_variants"):
        proc.enable_pca(5)
    proc.enable_variants()
    for bad in (0, 51):
        with pytest.raises(InvalidInputError):
            proc.enable_pca(bad)
    proc.enable_pca(12, scale=1)
    assert proc.pca_opt == {"n_comp": 12, "scale": True}


def test_small_cases_need_no_device(caplog):
    """Fewer than 2 cells or no variant: an empty result and a log line, nothing launched."""
    import logging

    from mgatk2_amd.analysis.pca import pca, principal_components
    from mgatk2_amd.exceptions import InvalidInputError

    with caplog.at_level(logging.INFO, logger="mgatk2_amd"):
        for af in (np.zeros((3, 1)), np.zeros((0, 9)), None):
            r = principal_components(af, n_comp=5)
            assert r.scores is None and r.loadings is None and r.n_comp == 0
    assert caplog.text.count("PCA skipped") == 3
    assert pca(np.zeros((4, 1)), 2).scores is None
    for call in (lambda: principal_components(np.zeros((3, 5)), n_comp=0), lambda: pca(np.zeros((3, 5)), 0),
                 lambda: pca(np.zeros(5), 1), lambda: principal_components(np.zeros((2049, 3)), n_comp=2),
                 lambda: principal_components(np.zeros((3, 5)), barcodes=["a"], n_comp=2)):
        with pytest.raises(InvalidInputError):
            call()


# ---- the pipeline's plumbing, numpy standing in for the device call -------------------------------
def stand_in_device(monkeypatch):
    """engine.pca replaced by numpy (eigh with the order and sign rule); returns the list of calls made."""
    from mgatk2_amd import engine

    calls = []

    def pca(x, n_comp, scale=False, device=0, want_cov=False):
        x = np.ascontiguousarray(x, np.float64)
        calls.append((x.shape, int(n_comp), bool(scale), device))
        mean = x.mean(axis=1)
        z = x - mean[:, None]
        if scale:
            sd = z.std(axis=1, ddof=1)
            z = np.divide(z, sd[:, None], out=np.zeros_like(z), where=sd[:, None] != 0)
        cov = np.atleast_2d(np.cov(z))
        w, v = np.linalg.eigh(cov)
        w, vec = pca_model.order_and_sign(w, v.T)
        return {"mean": mean, "sd": sd if scale else np.sqrt(np.diag(cov)), "eigenvalues": w,
                "loadings": vec[:n_comp], "scores": vec[:n_comp] @ z, "sweeps": 1}

    monkeypatch.setattr(engine, "pca", pca)
    return calls


def test_pipeline_writes_the_pca_files(tmp_path, oracle_lib, monkeypatch):
    """run_pipeline(call_variants, pca=5, pca_scale) with the oracle engine and the stand-in: the three files
    with the matrix's shapes, the variants in genomic order, and nothing else changed; no files without pca;
    more variants than one call takes are refused after every other output was written."""
    from test_cluster import LOW, _files, _patch_run, _pipeline, written_matrix

    from mgatk2_amd.exceptions import InvalidInputError

    _patch_run(monkeypatch, oracle_lib)
    calls = stand_in_device(monkeypatch)
    g, plain = _pipeline(tmp_path, "plain", **LOW)
    assert calls == [] and not any("pca" in f or "loadings" in f for f in _files(plain))
    _, out = _pipeline(tmp_path, "pca", pca=5, pca_scale=True, **LOW)
    names, af = written_matrix(out, g.whitelist)
    nv, nc = af.shape
    assert 5 <= nv <= 2048 and calls == [((nv, nc), 5, True, 0)]
    assert [f for f in _files(out) if f not in _files(plain)] == PCA_FILES
    for rel in _files(plain):
        if not rel.endswith(("summary.txt", "output.log")):
            assert (out / rel).read_bytes() == (plain / rel).read_bytes(), rel
    table = lambda name: [line.split("\t") for line in (out / "variants" / name).read_text().splitlines()]  # noqa: E731
    cells, load, var = table("cell_pca.tsv"), table("variant_loadings.tsv"), table("pca_variance.tsv")
    pcs = [f"PC{c + 1}" for c in range(5)]
    assert cells[0] == ["barcode", *pcs] and [r[0] for r in cells[1:]] == list(g.whitelist)
    assert load[0] == ["variant", "mean", "sd", *pcs] and [r[0] for r in load[1:]] == names
    assert [float(r[1]) for r in load[1:]] == af.mean(axis=1).tolist()  # the rows are the genomic order's
    assert [r[0] for r in var[1:]] == pcs and len(var[0]) == 5
    scores = np.array([[float(v) for v in r[1:]] for r in cells[1:]]).T
    np.testing.assert_allclose(scores.var(axis=1, ddof=1), [float(r[1]) for r in var[1:]], rtol=1e-9)
    # the unfiltered table has more variants than one call's 2,048: refused, every other output written
    calls.clear()
    wide = dict(LOW, variant_min_vmr=0.0)
    with pytest.raises(InvalidInputError, match="more than 2048 in one call"):
        _pipeline(tmp_path, "wide", pca=5, **wide)
    _, wide_plain = _pipeline(tmp_path, "wideplain", **wide)
    assert calls == [] and _files(tmp_path / "wide" / "out") == _files(wide_plain)


# ---- the writers ---------------------------------------------------------------------------
class _Table:
    """A variant table in vmr order whose genomic order differs (as heteroplasmy_matrix takes it)."""

    variant = ["200C>T", "10A>G"]
    position = np.array([200, 10])
    base = np.array([3, 2])

    def __len__(self):
        return 2


def test_writers_exact_text(tmp_path):
    from mgatk2_amd.analysis.pca import PcaResult, variance_table, write_pca_outputs

    res = PcaResult(n=3, n_comp=2, mean=np.array([0.25, 0.5]), sd=np.array([0.1, 2.0]),
                    eigenvalues=np.array([3.0, 1.0]), loadings=np.array([[0.6, 0.8], [0.8, -0.6]]),
                    scores=np.array([[1.5, -0.5, -1.0], [0.25, 0.0, -0.25]]), sweeps=2)
    vdir = write_pca_outputs(res, ["AAA-1", "CCC-1", "GGG-1"], _Table(), tmp_path)
    assert vdir == tmp_path / "variants" and sorted(p.name for p in vdir.iterdir()) == sorted(
        Path(f).name for f in PCA_FILES)
    assert (vdir / "cell_pca.tsv").read_text() == (
        "barcode\tPC1\tPC2\n" "AAA-1\t1.5\t0.25\n" "CCC-1\t-0.5\t0.0\n" "GGG-1\t-1.0\t-0.25\n")
    # the loadings' columns are the variants in genomic order: 10A>G first
    assert (vdir / "variant_loadings.tsv").read_text() == (
        "variant\tmean\tsd\tPC1\tPC2\n" "10A>G\t0.25\t0.1\t0.6\t0.8\n" "200C>T\t0.5\t2.0\t0.8\t-0.6\n")
    assert (vdir / "pca_variance.tsv").read_text() == (
        "component\teigenvalue\tsdev\tvariance_fraction\tcumulative\n"
        f"PC1\t3.0\t{3.0 ** 0.5!r}\t0.75\t0.75\n" "PC2\t1.0\t1.0\t0.25\t1.0\n")
    # a negative rounding-level eigenvalue: sdev 0, the fractions over the sum of all of them
    sdev, frac, cum = variance_table([2.0, 1.0, 1.0, -2.0 ** -60], 2)
    assert sdev == [2.0 ** 0.5, 1.0] and frac == [2.0 / (4.0 - 2.0 ** -60), 1.0 / (4.0 - 2.0 ** -60)]
    assert cum == [frac[0], frac[0] + frac[1]] and variance_table([0.0, -0.0], 2)[1] == [0.0, 0.0]
    assert variance_table([1.0, -4.0], 2)[0] == [1.0, 0.0]
    # without a table the variants are numbered; an empty result writes nothing
    write_pca_outputs(res, ["a", "b", "c"], None, tmp_path / "n")
    assert (tmp_path / "n" / "variants" / "variant_loadings.tsv").read_text().splitlines()[1].startswith("V1\t")
    write_pca_outputs(PcaResult(1, 0), ["a"], None, tmp_path / "e")
    assert list((tmp_path / "e" / "variants").iterdir()) == []
    from mgatk2_amd.exceptions import InvalidInputError

    with pytest.raises(InvalidInputError):
        write_pca_outputs(res, ["a", "b"], None, tmp_path / "x")
