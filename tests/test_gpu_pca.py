"""mgp_pca / mgp_sym_eig on the device (mgp_pca.hip) against the Python model of tests/pca_model.py and numpy.

Means, standard deviations, the covariance and the scores are defined as chains of single fp64 operations, so
they are compared bit for bit with the model. The eigenpairs are compared with numpy.linalg.eigh's by residual,
orthogonality and eigenvalue: both methods are backward stable at O(m eps |A|), so ours may be 8 x numpy's (the
margin for Jacobi's ten or so sweeps against LAPACK's single reduction) with a floor of 8 m 2^-53 max|lambda|.

The sizes follow the kernels' shapes: the slab of 1,024 items (n = 1023, 1024, 1025, 2049: under, at, over one
slab and over two), the covariance's tile edges 16, 32 and 64 and the Jacobi step's 16 (m = 33 and 65, 16, 17, 63,
64, 65), the slab sums' 64 features a workgroup (m = 65), the scores' 8 components a workgroup (k = 3, 50).
Every figure is printed before it is asserted (pytest -s shows them).
"""

from __future__ import annotations

import numpy as np
import pytest

import pca_model
from test_gpu_variants import _files, _pipeline, _same_file
from test_pca import PCA_FILES, planted_matrix

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SHAPES = [(2, 1), (3, 2), (1023, 3), (1024, 3), (1025, 5), (2049, 4), (300, 33), (70, 65)]

_data = {}


def sparse_matrix(n, m):
    """x [m][n]: 90 % zeros, the rest uniform in (0, 1], and (m >= 2) one constant variant: 0.5, whose sums
    are exact, so its mean is 0.5 and its centred row exactly 0. Made once per shape and left unchanged."""
    if (n, m) not in _data:
        rng = np.random.default_rng(1000 * n + m)
        x = np.where(rng.random((m, n)) < 0.9, 0.0, 1.0 - rng.random((m, n)))
        if m >= 2:
            x[m // 2] = 0.5
        x.setflags(write=False)
        _data[n, m] = x
    return _data[n, m]


def same_bits(got, want, what):
    assert got.shape == want.shape, what
    diff = np.flatnonzero(pca_model.bits(got).ravel() != pca_model.bits(want).ravel())
    assert diff.size == 0, (what, diff[:5], got.ravel()[diff[:5]], want.ravel()[diff[:5]])


# ---- 1. means, sd, covariance --------------------------------------------------------------
@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("n,m", SHAPES)
def test_mean_sd_cov_equal_the_model_bit_for_bit(engine_lib, n, m, scale):
    x = sparse_matrix(n, m)
    out = engine_lib.pca(x, 1, scale, want_cov=True)
    mod = pca_model.model(x, scale)
    same_bits(out["mean"], mod["mean"], "mean")
    same_bits(out["sd"], mod["sd"], "sd")
    same_bits(out["cov"], mod["cov"], "cov")
    assert np.array_equal(out["cov"], out["cov"].T)
    if m >= 2:
        c = m // 2
        assert out["mean"][c] == 0.5 and out["sd"][c] == 0.0
        assert not out["cov"][c].any() and not out["cov"][:, c].any()
    assert out["eigenvalues"].shape == (m,) and out["loadings"].shape == (1, m) and out["scores"].shape == (1, n)


# ---- 2. the symmetric eigensolver -------------------------------------------------------------
def spectrum_matrix(lam, seed):
    """Q diag(lam) Q^T with a random orthogonal Q, symmetrised exactly."""
    m = len(lam)
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((m, m)))
    a = (q * np.asarray(lam)) @ q.T
    return (a + a.T) / 2.0


def eig_case(kind, m):
    """(matrix, the repeated eigenvalue's (value, multiplicity, gap to the rest) or None)."""
    rng = np.random.default_rng(17 * m + len(kind))
    separated = np.linspace(-2.0, 5.0, m) if m > 1 else np.array([3.0])
    if kind == "separated":
        return spectrum_matrix(separated, m), None
    if kind == "diagonal":
        d = rng.permutation(np.arange(1.0, m + 1.0))
        d[0] = -1.5
        return np.diag(d), None
    if kind == "zero":
        return np.zeros((m, m)), None
    if kind == "zero_row":
        a = spectrum_matrix(separated, m + 1)
        a[m // 2, :] = 0.0
        a[:, m // 2] = 0.0
        return a, None
    mult = min(3, m)
    lam = np.concatenate([np.full(mult, 5.0), np.linspace(-2.0, 3.0, m - mult)])
    return spectrum_matrix(lam, m + 2), (5.0, mult, 2.0 if m > mult else np.inf)


def eig_quality(a, w, rows):
    """(max|A V - V L|, max|V^T V - I|) of eigenvalues w and eigenvectors as rows."""
    v = rows.T
    return float(np.abs(a @ v - v * w).max()), float(np.abs(v.T @ v - np.eye(len(w))).max())


@pytest.mark.parametrize("kind", ["separated", "diagonal", "zero", "zero_row", "repeated"])
@pytest.mark.parametrize("m", [1, 2, 3, 16, 17, 63, 64, 65, 200])
def test_sym_eig_against_numpy(engine_lib, m, kind):
    a, repeated = eig_case(kind, m)
    w, vec, sweeps = engine_lib.sym_eig(a)
    w2, vec2, sweeps2 = engine_lib.sym_eig(a)
    assert w.tobytes() == w2.tobytes() and vec.tobytes() == vec2.tobytes() and sweeps == sweeps2
    wn, vn = np.linalg.eigh(a)
    wn, vn = wn[::-1], vn[:, ::-1].T
    floor = 8 * m * EPS * float(np.abs(wn).max())
    res, orth = eig_quality(a, w, vec)
    res_np, orth_np = eig_quality(a, wn, vn)
    err = float(np.abs(w - wn).max())
    print(f"\nsym_eig m={m} {kind}: sweeps {sweeps}, residual {res:.3e} (numpy {res_np:.3e}, "
          f"ratio {res / res_np if res_np else 0.0:.2f}), orthogonality {orth:.3e} (numpy {orth_np:.3e}, "
          f"ratio {orth / orth_np if orth_np else 0.0:.2f}), eigenvalues {err:.3e}, floor {floor:.3e}")
    assert res <= max(8 * res_np, floor)
    assert orth <= max(8 * orth_np, floor)
    assert err <= floor
    assert np.all(np.diff(w) <= 0) and pca_model.sign_rule_holds(vec)
    if not np.any(a - np.diag(np.diag(a))):  # diagonal (the zero matrix, m = 1 and a zeroed row of m = 2 too)
        assert sweeps == 0 and (kind in ("zero", "diagonal") or m <= 2)
        order = sorted(range(m), key=lambda i: (-a[i, i], i))  # ties: the lower diagonal place first
        assert w.tolist() == [a[i, i] for i in order] and np.array_equal(vec, np.eye(m)[order])
    else:  # (a repeated spectrum of m <= 3 is 5 I up to rounding: it may take no rotation either)
        assert (1 if kind == "separated" else 0) <= sweeps < 30
    if kind == "zero_row" and m >= 2:
        z = m // 2
        at = int(np.flatnonzero(vec[:, z] != 0.0)[0])  # the one vector on the zero row's axis: exact
        assert np.array_equal(vec[at], np.eye(m)[z]) and w[at] == 0.0 and np.count_nonzero(vec[:, z]) == 1
    if repeated is not None:
        lam, mult, gap = repeated
        sel = np.abs(w - lam) <= floor
        assert int(sel.sum()) == mult and np.array_equal(sel, np.abs(wn - lam) <= floor)
        # each side's eigenspace is that of A + E with |E| <= floor: sin(theta) <= floor / gap each (Davis-Kahan),
        # the projectors differ by at most the sum, twice over for the entry-wise reading of a 2-norm bound
        tol = 4 * floor / gap + 8 * m * EPS
        diff = float(np.abs(vec[sel].T @ vec[sel] - vn[sel].T @ vn[sel]).max())
        print(f"  projector of lambda = {lam} (x{mult}): max difference {diff:.3e}, bound {tol:.3e}")
        assert diff <= tol


def test_sym_eig_refuses_bad_matrices(engine_lib):
    from mgatk2_amd.exceptions import InvalidInputError

    a = spectrum_matrix(np.linspace(1.0, 2.0, 20), 3)
    for at, value, text in (((3, 7), 9.0, "not symmetric"), ((19, 0), np.nextafter(a[19, 0], 9.0), "not symmetric"),
                            ((5, 5), np.inf, "not finite"), ((2, 4), np.nan, "not finite")):
        b = a.copy()
        b[at] = value
        if text == "not finite":
            b[at[::-1]] = value
        with pytest.raises(InvalidInputError, match=text):
            engine_lib.sym_eig(b)
    with pytest.raises(InvalidInputError, match="not finite"):
        x = np.array(sparse_matrix(300, 33))
        x[32, 299] = -np.inf
        engine_lib.pca(x, 2)


# ---- 3. scores -------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("n,m,k", [(1025, 5, 3), (70, 65, 50), (3, 2, 2)])
def test_scores_equal_the_model_on_the_calls_own_loadings(engine_lib, n, m, k, scale):
    x = sparse_matrix(n, m)
    out = engine_lib.pca(x, k, scale, want_cov=True)
    z, _, _ = pca_model.standardized(x, scale, out["mean"], out["sd"] if scale else None)
    same_bits(z, pca_model.model(x, scale)["z"], "z")
    same_bits(out["scores"], pca_model.scores(z, out["loadings"]), "scores")
    w, vec, sweeps = engine_lib.sym_eig(out["cov"])
    assert out["eigenvalues"].tobytes() == w.tobytes() and out["loadings"].tobytes() == vec[:k].tobytes()
    assert out["sweeps"] == sweeps


# ---- 4. the whole call -------------------------------------------------------------------------
def test_planted_rank_three(engine_lib, monkeypatch):
    from mgatk2_amd.analysis.pca import pca, variance_table

    n, m, k = 2049, 40, 5
    x = planted_matrix(n, m, 3, 1e-3, 11)
    monkeypatch.delenv("MGP_PCA_TILE", raising=False)
    r = pca(x, k)
    assert (r.n, r.n_comp, r.scores.shape, r.loadings.shape, r.eigenvalues.shape) == (n, k, (k, n), (k, m), (m,))
    _, frac, cum = variance_table(r.eigenvalues, k)
    print(f"\nplanted rank 3: fractions {frac[:4]}, sweeps {r.sweeps}")
    assert sum(frac[:3]) > 0.99 and cum[2] > 0.99 and frac[3] < 1e-5
    floor = 8 * m * EPS * float(np.abs(r.eigenvalues).max())
    var = r.scores.var(axis=1, ddof=1)
    print(f"  score variance - eigenvalue: {np.abs(var - r.eigenvalues[:k]).tolist()}, floor {floor:.3e}")
    assert np.all(np.abs(var - r.eigenvalues[:k]) <= floor)
    # the covariance's tile edge changes no byte
    base = engine_lib.pca(x, k, True, want_cov=True)
    for tile in ("16", "32", "64"):
        monkeypatch.setenv("MGP_PCA_TILE", tile)
        again = engine_lib.pca(x, k, True, want_cov=True)
        for key in ("mean", "sd", "eigenvalues", "loadings", "scores", "cov"):
            assert again[key].tobytes() == base[key].tobytes(), (tile, key)
        assert again["sweeps"] == base["sweeps"]


def test_components_are_clipped(engine_lib, caplog):
    import logging

    from mgatk2_amd.analysis.pca import principal_components

    x = planted_matrix(10, 3, 2, 0.1, 5)
    with caplog.at_level(logging.INFO, logger="mgatk2_amd"):
        r = principal_components(x, n_comp=5)
    assert r.n_comp == 3 and r.scores.shape == (3, 10) and "clipped to 3" in caplog.text
    assert principal_components(x[:, :3], n_comp=5).n_comp == 2  # the other items bound it too


# ---- 5. the pipeline -----------------------------------------------------------------------------
# (thresholds lowered so that variants pass at this depth, as tests/test_cluster.py's: with min_vmr = 1 some
# hundred of them; at min_vmr = 0 there are 3,230, more than one call's 2,048)
LOW = dict(call_variants=True, variant_min_cells=0, variant_min_strand_cor=-1.0, variant_min_vmr=1.0)


def test_pipeline_pca(tmp_path, engine_lib, monkeypatch):
    """run_pipeline(call_variants, pca=5, pca_scale) on the synth_run_h5 golden reads, the thresholds lowered as
    in test_cluster so that variants pass: the three files have the matrix's shapes and hold what engine.pca
    gives for the matrix the run wrote (variants in genomic order); every other file is what a run without the
    flag writes; analyze on the run's output writes the same cell_pca.tsv."""
    from click.testing import CliRunner

    from mgatk2_amd import cli, h5lite
    from mgatk2_amd.pipeline import analyze_outputs

    g, out = _pipeline(tmp_path, "pca", "hdf5", monkeypatch, pca=5, pca_scale=True, **LOW)
    _, plain = _pipeline(tmp_path, "plain", "hdf5", monkeypatch, **LOW)
    assert [f for f in _files(out) if f not in _files(plain)] == PCA_FILES
    assert [f for f in _files(out) if f not in PCA_FILES] == _files(plain)
    for rel in _files(plain):
        _same_file(out, plain, rel)
    rows = [line.split("\t") for line in (out / "variants" / "variant_stats.tsv").read_text().splitlines()[1:]]
    order = sorted(range(len(rows)), key=lambda r: (int(rows[r][0]), "ACGT".index(rows[r][1][-1])))
    with h5lite.File(out / "variants" / "allele_freq.h5", "r") as f:
        af = np.asarray(f["allele_freq"][...], np.float64)[order]
    nv, nc = af.shape
    assert nv == len(rows) and nc == len(g.whitelist) and 2 <= nv <= 2048
    k = min(5, nv, nc - 1)
    want = engine_lib.pca(af, k, True)
    table = lambda name: [line.split("\t") for line in (out / "variants" / name).read_text().splitlines()]  # noqa: E731
    cells, load, var = table("cell_pca.tsv"), table("variant_loadings.tsv"), table("pca_variance.tsv")
    pcs = [f"PC{c + 1}" for c in range(k)]
    assert cells[0] == ["barcode", *pcs] and [r[0] for r in cells[1:]] == list(g.whitelist)
    assert [r[1:] for r in cells[1:]] == [[repr(v) for v in col] for col in want["scores"].T.tolist()]
    assert load[0] == ["variant", "mean", "sd", *pcs] and [r[0] for r in load[1:]] == [rows[r][2] for r in order]
    assert [r[1] for r in load[1:]] == [repr(v) for v in want["mean"].tolist()]
    assert [r[2] for r in load[1:]] == [repr(v) for v in want["sd"].tolist()]
    assert [r[3:] for r in load[1:]] == [[repr(v) for v in col] for col in want["loadings"].T.tolist()]
    assert var[0] == ["component", "eigenvalue", "sdev", "variance_fraction", "cumulative"]
    assert [r[0] for r in var[1:]] == pcs and [r[1] for r in var[1:]] == [repr(v) for v in want["eigenvalues"][:k].tolist()]
    assert 0.0 < float(var[-1][4]) <= 1.0 + 1e-12
    # analyze on the finished run: the same file, by the keyword and by the command
    analyze_outputs(out, tmp_path / "again", pca=5, pca_scale=True, **LOW)
    _same_file(out, tmp_path / "again", "variants/cell_pca.tsv")
    r = CliRunner().invoke(cli.cli, ["analyze", "-i", str(out), "-o", str(tmp_path / "cmd"), "--variants",
                                     "--variant-min-cells", "0", "--variant-min-strand-cor", "-1", "--variant-min-vmr",
                                     "1", "--pca", "5", "--pca-scale"])
    assert r.exit_code == 0, r.output
    for rel in PCA_FILES:
        _same_file(out, tmp_path / "cmd", rel)
    # without --pca-scale the components differ (the flag reaches the device)
    analyze_outputs(out, tmp_path / "plainpca", pca=5, **LOW)
    assert (tmp_path / "plainpca" / "variants" / "cell_pca.tsv").read_bytes() != (
        out / "variants" / "cell_pca.tsv").read_bytes()
