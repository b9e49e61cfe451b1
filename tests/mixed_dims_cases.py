"""Problems whose two dimensions differ in kernel family, basis, m and n (TEST INFRASTRUCTURE, shared by tests/test_oracle.py and
tests/test_gpu_mixed_dims.py): the dimension descriptions, their translation into oracle/kron.py factors and oracle/dense.py
arguments, and the transposed twin of a problem.

A dimension is Dim(kind, basis, grid) with `grid` in oracle/kron.py's layout (Factor.grid).  Every case uses s1 != s2, ell1 != ell2,
m1 != m2 and n1 != n2, so that no exchange of the two dimensions' attributes can cancel."""
from collections import namedtuple

import numpy as np
import torch

from oracle import dense as D
from oracle import kron as Kr

Dim = namedtuple("Dim", "kind basis grid")
SWAP = [1, 0, 3, 2, 4]                       # theta of the transposed problem


def vff(nfreq, a=-0.1, b=1.1):
    """m = 2 nfreq + 1 Fourier features on [a, b]."""
    return Dim("matern12", "vff", np.concatenate([[a, b], D.vff_omegas(nfreq, a, b).double().numpy()]))


def b0(m):
    return Dim("matern12", "b0", np.linspace(0, 1, m + 1))


def b1(m, pad=2):
    """m hat functions on the knots of a B0 mesh over [0, 1] padded by `pad` knots on either side (what the gridded read-out needs)."""
    d = 1.0 / (m - 1 - 2 * pad)
    return Dim("matern12", "b1", np.linspace(-pad * d, 1 + pad * d, m))


def pts(kind, m, lo=0.0, hi=1.0):
    return Dim(kind, "points", np.linspace(lo, hi, m))


def irregular(kind, m, seed=3):
    """Irregular inducing points as in test_zgrad_vs_oracle."""
    return Dim(kind, "points", np.sort(np.random.default_rng(seed).uniform(0.02, 0.98, m)))


def factor(d: Dim, x) -> Kr.Factor:
    return Kr.Factor(d.basis, d.kind, np.asarray(d.grid, float), np.asarray(x, float))


def dense_grid(d: Dim):
    """The grid argument of oracle/dense.py DenseKron for this dimension."""
    g = np.asarray(d.grid, float)
    return (float(g[0]), float(g[1]), len(g) - 3) if d.basis == "vff" else torch.tensor(g)


def dense(X, y, d1: Dim, d2: Dim, theta, mask=None) -> D.DenseKron:
    return D.DenseKron(X, y, (d1.basis, d2.basis), (d1.kind, d2.kind), dense_grid(d1), dense_grid(d2),
                       raw=D.raw_from_constrained(theta), mask=mask)


def plan_args(d1: Dim, x1, d2: Dim, x2):
    """Positional arguments of Engine.plan."""
    return d1.kind, d1.basis, d1.grid, x1, d2.kind, d2.basis, d2.grid, x2


# name -> (dimension 1, dimension 2, (n1, n2), theta): the four full-grid combinations.  The RBF lengthscale is 40 times the spacing of
# its eleven inducing points (h / ell = 0.025: the pivots of the unit RBF factor fall by ~(h / ell)^2 each, the last five are rounding
# noise), so that factor needs the jitter 1e-8 while the VFF factor takes none: the step's jitter pair has two different entries
# (asserted in tests/test_oracle.py).  Points spread over the data range keep the two float64 oracles within 1e-13 of each other; the
# same ratio from points crowded into [0.45, 0.55] leaves them 9e-10 / 3e-9 apart -- too ill-conditioned for the bounds.
FULL = {
    "rbf_pts11-m12_vff9": (pts("rbf", 11), vff(4), (40, 28), np.array([4.0, 0.2, 1.3, 0.7, 0.01])),
    "m12_b09-m32_pts7": (b0(9), pts("matern32", 7), (40, 33), np.array([0.25, 0.2, 1.3, 0.7, 0.01])),
    "m12_b115-m52_pts6": (b1(15), pts("matern52", 6), (40, 33), np.array([0.25, 0.2, 1.3, 0.7, 0.01])),
    "m32_pts9-m52_pts12": (pts("matern32", 9), pts("matern52", 12), (40, 33), np.array([0.25, 0.2, 1.3, 0.7, 0.01])),
}
ORDERS = ("ab", "ba")


def grid_problem(d1, d2, n, theta, order="ab"):
    """-> (d1, d2, x1, x2, Y [n2, n1], X (N, 2), y (N,), theta); order 'ba' is the transposed twin: the dimensions exchanged, Y
    transposed, theta permuted -- the same model, so the same ELBO."""
    X, y, x1, x2 = D.gen_grid(*n)
    Y = y.reshape(n[1], n[0])
    theta = np.asarray(theta, float)
    if order == "ab":
        return d1, d2, x1, x2, Y, X, y, theta
    Yt = np.ascontiguousarray(Y.T)
    X1, X2 = np.meshgrid(x2, x1)
    return d2, d1, x2, x1, Yt, np.vstack([X1.ravel(), X2.ravel()]).T, Yt.reshape(-1), theta[SWAP]


def gl_cells(d: Dim, mesh, ell):
    """Unit-outputscale Cov(v, u) (mv x m) of B0 cells on `mesh` with B0 inducing features, by 8-point Gauss-Legendre integration of
    the closed-form Kuf over every output cell, and the unit diagonal of Kvv (the read-out is linear algebra in these arrays; the
    code under test and the oracle receive the same ones)."""
    assert d.basis == "b0"
    xg, wg = np.polynomial.legendre.leggauss(8)
    mesh = np.asarray(mesh, float)
    mid, half = 0.5 * (mesh[1:] + mesh[:-1]), 0.5 * (mesh[1:] - mesh[:-1])
    t = mid[:, None] + half[:, None] * xg[None, :]                                    # (mv, 8)
    A = Kr.b0_A(np.asarray(d.grid, float), t.reshape(-1), ell)[0].reshape(-1, len(mid), 8)
    C = (A * (half[:, None] * wg[None, :])[None]).sum(2).T
    kd = np.full(len(mid), Kr.b0_K(len(mid), float(mesh[1] - mesh[0]), ell)[0][0, 0])
    return C, kd
