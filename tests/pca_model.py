"""The definition of mgp_pca (include/mgpileup.h) in Python: every chain step in exact Fraction arithmetic,
rounded once to fp64, in the order the definition fixes; the eigenvalues' order and the eigenvectors' sign rule.
Not a test file: tests/test_pca.py checks the model against numpy, tests/test_gpu_pca.py the device against it.
The eigensolver itself is not restated: given cov, the device's eigenpairs are compared with numpy.linalg.eigh's
by residual and orthogonality, and the scores are modelled from the loadings the call returned.
"""

from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

SLAB = 1024  # items of a slab: part of the definition


def _f(x: float) -> Fraction:
    return Fraction(float(x))


def add(a: float, b: float) -> float:
    """a + b rounded once (the float sum is that already; restated for the chain's reading)."""
    return float(a) + float(b)


def sub(a: float, b: float) -> float:
    return float(a) - float(b)


def fma(a: float, b: float, c: float) -> float:
    """a * b + c with one rounding. An exact zero takes IEEE's sign: that of the float expression when the
    product itself is zero, +0.0 when a non-zero product cancels c."""
    a, b, c = float(a), float(b), float(c)
    prod = _f(a) * _f(b)
    exact = prod + _f(c)
    if exact == 0:
        return a * b + c if prod == 0 else 0.0
    return float(exact)


def slab_chain(step, n: int) -> float:
    """The slab sums of a chain added in ascending slab order from 0.0. step(s, i) -> the chain's next s."""
    total = 0.0
    for lo in range(0, n, SLAB):
        s = 0.0
        for i in range(lo, min(n, lo + SLAB)):
            s = step(s, i)
        total = add(total, s)
    return total


def means(x: np.ndarray) -> np.ndarray:
    m, n = x.shape
    rows = x.tolist()
    return np.array([slab_chain(lambda s, i, r=rows[f]: add(s, r[i]), n) / n for f in range(m)], np.float64)


def centred(x: np.ndarray, mean: np.ndarray) -> np.ndarray:
    return x - mean[:, None]  # one subtraction each: numpy's is the rounded one


def sds(xc: np.ndarray) -> np.ndarray:
    """sqrt(var), var the slab-chained fma sum of xc^2 over n - 1."""
    m, n = xc.shape
    rows = xc.tolist()
    var = [slab_chain(lambda s, i, r=rows[f]: fma(r[i], r[i], s), n) / (n - 1) for f in range(m)]
    return np.array([math.sqrt(v) for v in var], np.float64)


def standardized(x: np.ndarray, scale: bool, mean: np.ndarray | None = None, sd: np.ndarray | None = None):
    """(z, mean, sd or None): z = x - mean, divided by sd with scale (0 where sd == 0)."""
    x = np.ascontiguousarray(x, np.float64)
    mean = means(x) if mean is None else np.asarray(mean, np.float64)
    xc = centred(x, mean)
    if not scale:
        return xc, mean, None
    sd = sds(xc) if sd is None else np.asarray(sd, np.float64)
    z = np.zeros_like(xc)
    nz = sd != 0.0
    z[nz] = xc[nz] / sd[nz, None]
    return z, mean, sd


def covariance(z: np.ndarray) -> np.ndarray:
    """cov[a][b]: the slab-chained fma sum of z[a][i] z[b][i] over n - 1; one triangle, mirrored."""
    m, n = z.shape
    rows = z.tolist()
    cov = np.zeros((m, m), np.float64)
    for a in range(m):
        for b in range(a, m):
            cov[a, b] = cov[b, a] = slab_chain(lambda s, i, p=rows[a], q=rows[b]: fma(p[i], q[i], s), n) / (n - 1)
    return cov


def scores(z: np.ndarray, loadings: np.ndarray) -> np.ndarray:
    """score[c][i]: s = fma(z[f][i], vec[c][f], s) in ascending f from 0.0."""
    m, n = z.shape
    cols, vecs = z.T.tolist(), np.asarray(loadings, np.float64).tolist()
    out = np.zeros((len(vecs), n), np.float64)
    for c, v in enumerate(vecs):
        for i, col in enumerate(cols):
            s = 0.0
            for f in range(m):
                s = fma(col[f], v[f], s)
            out[c, i] = s
    return out


@functools.lru_cache(maxsize=None)
def _model(key: bytes, shape: tuple, scale: bool):
    x = np.frombuffer(key, np.float64).reshape(shape)
    z, mean, sd = standardized(x, scale)
    cov = covariance(z)
    for a in (z, mean, cov):
        a.setflags(write=False)
    if sd is None:
        sd = np.sqrt(np.diag(cov))
    sd.setflags(write=False)
    return {"z": z, "mean": mean, "sd": sd, "cov": cov}


def model(x: np.ndarray, scale: bool) -> dict:
    """z, mean, sd (without scale: the square root of cov's diagonal, as mgp_pca reports it) and cov of
    x [m][n], computed once per (matrix, scale) and shared read-only."""
    x = np.ascontiguousarray(x, np.float64)
    return _model(x.tobytes(), x.shape, bool(scale))


def order_and_sign(eigenvalues, vectors):
    """(eigenvalues descending, ties to the lower index; vectors as rows in that order, each flipped so its
    entry of largest magnitude, the lowest index among equals, is positive). vectors: row c belongs to
    eigenvalues[c]."""
    w, v = np.asarray(eigenvalues, np.float64), np.asarray(vectors, np.float64)
    order = sorted(range(len(w)), key=lambda i: (-w[i], i))
    w, v = w[order], v[order].copy()
    for row in v:
        lead = int(np.argmax(np.abs(row)))  # (argmax returns the first of equals)
        if row[lead] < 0:
            row *= -1.0
    return w, v


def sign_rule_holds(vectors) -> bool:
    v = np.asarray(vectors, np.float64)
    return all(row[int(np.argmax(np.abs(row)))] > 0 for row in v)


def bits(a) -> np.ndarray:
    """The fp64 bit patterns, for comparisons that tell -0.0 from 0.0."""
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
