"""Specification of the joint samples on the DENSE masked / scattered states (TEST HELPER, numpy float64, CPU):
vggp_tri_t_apply, vggp_qv_sample_masked and vggp_posterior_raster_sample_masked, and the problems their tests share.

The dense steps (oracle.kron.elbo_step_masked / elbo_step_scattered) assemble Sigma~ = I + rho Phi in M-space (MaskedState.Sig) and
factor it, Sigma~ = L L^T.  With E_s standard normal over the M = m1 m2 cells the whitened coefficient draw is
    X_s = L^-T E_s,     Cov(vec X_s) = L^-T L^-1 = Sigma~^-1,
the draw tests/qv_sample_spec.py takes from the eigenbasis (full grid) or from a block PCG solve (iterative states) -- another root of
the same Sigma~^-1, so another set of numbers with the same distribution.  Everything after X_s is imported, not copied:
    q(v)     V_s = mean + sqrt(s1^e1 s2^e2) L0_1 X_s L0_2^T                           (the formula of qv_sample_spec)
    raster   F_s = mu + B1^T (X_s B2 + sqrt(s2) H_s C2^T) + sqrt(s1 s2) C1 G_s Kc2^T   (raster_sample_spec.axes / combine / nugget_terms)
Noise: E stream 0, G stream 2, H stream 3 of qv_sample_spec's generator, the index spaces of the other samplers.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.linalg as sla

import mixed_dims_cases as Mx
import qv_sample_spec as S
import raster_sample_spec as R
from oracle import dense as D
from oracle import kron as Kr


# ---- the product on its own ------------------------------------------------------------------------------------------------------------------
def tri_t_apply(Xl: np.ndarray, E: np.ndarray, cn: int) -> np.ndarray:
    """Xl [M, M] (only its lower triangle counts), E [m1, nbc, m2] -> out [m1, nbc, m2]: out(u, c) = sum_{k >= u} Xl[k, u] E(k, c) for
    c < cn, zeros for c >= cn.  Works on integer arrays as well (the kernel test's exact reference)."""
    m1, nbc, m2 = E.shape
    cells = np.transpose(E, (0, 2, 1)).reshape(m1 * m2, nbc)                  # [u, c]
    out = np.tril(Xl).T @ cells
    out[:, cn:] = 0
    return np.ascontiguousarray(np.transpose(out.reshape(m1, m2, nbc), (0, 2, 1)))


# ---- the samplers -----------------------------------------------------------------------------------------------------------------------------
def coeff_draw(st: Kr.MaskedState, eps_u: np.ndarray) -> np.ndarray:
    """X_s = L^-T E_s with L = chol(Sigma~): eps_u [S, m1, m2] -> [S, m1, m2]."""
    S_, m1, m2 = eps_u.shape
    L = np.linalg.cholesky(st.Sig)
    X = sla.solve_triangular(L, eps_u.reshape(S_, m1 * m2).T, lower=True, trans="T")
    return np.ascontiguousarray(X.T).reshape(S_, m1, m2)


def sample_qv(st: Kr.MaskedState, f1: Kr.Factor, f2: Kr.Factor, eps_u: np.ndarray) -> np.ndarray:
    """eps_u [S, m1, m2] -> samples of q(v) [S, m1, m2] (st.d_d.L: the unit-outputscale factors L0_d)."""
    mean, _ = Kr.q_v_masked(st, f1, f2)
    return mean[None] + S._scale(st.theta, f1, f2) * (st.d1.L @ coeff_draw(st, eps_u) @ st.d2.L.T)


def raster_axes(st: Kr.MaskedState, f1: Kr.Factor, f2: Kr.Factor, g1, g2) -> R.Axes:
    return R.axes(f1, f2, st.d1.L, st.d2.L, st.theta, g1, g2)


def raster_mean(st: Kr.MaskedState, ax: R.Axes) -> np.ndarray:
    _, _, s1, s2, v = [float(t) for t in st.theta]
    return (s1 * s2 / v) * (ax.U1.T @ st.A0 @ ax.U2)


def sample_raster(st: Kr.MaskedState, f1: Kr.Factor, f2: Kr.Factor, g1, g2, eps_u, eps_g, eps_h):
    """-> (F [S, p1, p2], root levels)."""
    ax = raster_axes(st, f1, f2, g1, g2)
    return R.combine(ax, st.theta, raster_mean(st, ax), coeff_draw(st, eps_u), eps_g, eps_h), ax.levels


def sigma_scattered(X: np.ndarray, f1: Kr.Factor, f2: Kr.Factor, theta) -> np.ndarray:
    """Sigma~ of the dense scattered step alone, assembled as oracle.kron.elbo_step_scattered assembles it (for sizes at which the
    whole oracle step would take too long)."""
    ell1, ell2, s1, s2, v = [float(t) for t in theta]
    g1 = Kr.Factor(f1.basis, f1.kind, f1.grid, X[:, 0].copy(), f1.f32_kdelta)
    g2 = Kr.Factor(f2.basis, f2.kind, f2.grid, X[:, 1].copy(), f2.f32_kdelta)
    B1, B2 = Kr.dim_prepare(g1, ell1, 1.0).B, Kr.dim_prepare(g2, ell2, 1.0).B
    Zt = (B1[:, None, :] * B2[None, :, :]).reshape(B1.shape[0] * B2.shape[0], len(X))
    return np.eye(len(Zt)) + (s1 * s2 / v) * (Zt @ Zt.T)


# ---- the problems ----------------------------------------------------------------------------------------------------------------------------
THETA = [0.2, 0.3, 1.0, 0.8, 0.01]
THETA_PTS = [0.2, 0.22, 1.3, 0.7, 0.01]           # s1 != s2, ell1 != ell2: no exchange of the dimensions' attributes cancels
N1, N2, NPTS = 24, 20, 400
# the 7 x 5 raster of tests/test_raster_sample_spec.py: aligned with nothing
A1 = np.array([0.013, 0.171, 0.3337, 0.52, 0.649, 0.803, 0.987])
A2 = np.array([0.041, 0.29, 0.4777, 0.71, 0.962])
# name -> (kind of data, dimension 1, dimension 2, theta)
CASES = {"masked-b0-9x7": ("masked", Mx.b0(9), Mx.b0(7), THETA),                       # 24 x 20 grid, 30 % missing, Matern-1/2 B0
         "scattered-rbf-8x9": ("scattered", Mx.pts("rbf", 8), Mx.pts("rbf", 9), THETA_PTS),
         "scattered-m32pts8-vff9": ("scattered", Mx.pts("matern32", 8), Mx.vff(4), THETA_PTS),   # e_2 = -1
         "masked-b0-3x4": ("masked", Mx.b0(3), Mx.b0(4), THETA)}                       # M = 12: fewer cells than a block has columns


def grid_data():
    """-> Y [n2, n1], W [n2, n1] (0/1, 30 % missing), x1, x2."""
    _, y, x1, x2 = D.gen_grid(N1, N2)
    W = (np.random.default_rng(1).uniform(size=(N2, N1)) < 0.7).astype(np.float64)
    return y.reshape(N2, N1), W, x1, x2


def scattered_data(n: int = NPTS, seed: int = 3):
    """-> X [N, 2], y [N]."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, 2))
    y = np.asarray(D.latent_2d(X[:, 0], X[:, 1])) + 0.05 * rng.standard_normal(n)
    return X, y


@functools.lru_cache(maxsize=None)
def problem(name: str):
    """-> dict(kind, d1, d2, theta, f1, f2, st = the oracle's dense state, and the data: Y, W, x1, x2 or X, y).  Computed once."""
    kind, d1, d2, theta = CASES[name]
    if kind == "masked":
        Y, W, x1, x2 = grid_data()
        f1, f2 = Mx.factor(d1, x1), Mx.factor(d2, x2)
        return dict(kind=kind, d1=d1, d2=d2, theta=theta, f1=f1, f2=f2, Y=Y, W=W, x1=x1, x2=x2, st=Kr.elbo_step_masked(Y, W, f1, f2, theta))
    X, y = scattered_data()
    f1, f2 = Mx.factor(d1, X[:, 0].copy()), Mx.factor(d2, X[:, 1].copy())
    return dict(kind=kind, d1=d1, d2=d2, theta=theta, f1=f1, f2=f2, X=X, y=y, st=Kr.elbo_step_scattered(X, y, f1, f2, theta))
