"""Specification of the joint samples of posterior(x*) on a raster (TEST HELPER, numpy float64, CPU): vggp_posterior_raster_sample,
vggp_posterior_raster_sample_masked_iter, vggp_posterior_raster_sample_scattered_iter.

On cartesian_prod(g1, g2) the posterior covariance (kronecker_structure.py:223-229) is the q(u) part plus the prior residual,
    K** + Kuf*^T Sigma^-1 Kuf* - Kuf*^T Kuu^-1 Kuf*  =  (B1 (x) B2)^T Sigma~^-1 (B1 (x) B2)  +  s1 s2 (k1 (x) k2 - q1 (x) q2),
and the residual, a difference of two Kronecker products, is the sum of two positive semi-definite ones:
    k1 (x) k2 - q1 (x) q2  =  (k1 - q1) (x) k2  +  q1 (x) (k2 - q2).
With U_d = L0_d^-1 A0_d(g_d), B_d = sqrt(s_d) U_d, k_d the unit point kernel on the axis, r_d = k_d - U_d^T U_d,
C_d = chol(r_d + eta I), Kc2 = chol(k_2 + eta I), eta = ETA, and X_s the whitened coefficient draw of tests/qv_sample_spec.py
(Cov(vec X_s) = Sigma~^-1):
    F_s = mu + B1^T W_s + sqrt(s1 s2) C1 T_s,     W_s = X_s B2 + sqrt(s2) H_s C2^T,     T_s = G_s Kc2^T
    Cov(vec F_s) = (B1 (x) B2)^T Sigma~^-1 (B1 (x) B2) + s1 s2 (r1 + eta I) (x) (k2 + eta I) + (B1^T B1) (x) s2 (r2 + eta I).
Noise: E, F as the samplers of q(v); G_s [p1][p2] stream 2, idx = s p1 p2 + a p2 + b; H_s [m1][p2] stream 3, idx = s m1 p2 + i p2 + b.
B1 hats are refused: k_d - q_d is indefinite there.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.linalg as sla

import masked_iter_readout_spec as MS
import qv_sample_spec as S
import scattered_iter_variance_spec as SS
from oracle import kron as Kr

ETA = 1e-8
LEVELS = (0.0, 1e-8, 1e-7, 1e-6)          # the jitter schedule of vggp_cholesky_inverse, on top of the nugget


def noise_g(seed: int, first: int, n: int, p1: int, p2: int) -> np.ndarray:
    return S.normal_fill(seed, 2, first * p1 * p2, n * p1 * p2).reshape(n, p1, p2)


def noise_h(seed: int, first: int, n: int, m1: int, p2: int) -> np.ndarray:
    return S.normal_fill(seed, 3, first * m1 * p2, n * m1 * p2).reshape(n, m1, p2)


def noise_pred(seed: int, first: int, n: int, P: int) -> np.ndarray:
    """Stream 4: the observation noise of posterior_predictive_grid().sample(), [n, P]."""
    return S.normal_fill(seed, 4, first * P, n * P).reshape(n, P)


def root(A: np.ndarray):
    """chol(A + level I) at the first level of the schedule that succeeds -> (factor, level)."""
    for lvl in LEVELS:
        try:
            C = np.linalg.cholesky(A + lvl * np.eye(A.shape[0]))
            if np.isfinite(C).all():
                return C, lvl
        except np.linalg.LinAlgError:
            pass
    raise np.linalg.LinAlgError("a residual root is not positive definite after jitter 1e-6")


@dataclass
class Axes:
    U1: np.ndarray          # [m1, p1]
    U2: np.ndarray
    k1: np.ndarray          # [p1, p1]
    k2: np.ndarray
    r1: np.ndarray
    r2: np.ndarray
    C1: np.ndarray
    C2: np.ndarray
    Kc2: np.ndarray
    levels: tuple           # (C1, C2, Kc2)


def axes(f1: Kr.Factor, f2: Kr.Factor, L01: np.ndarray, L02: np.ndarray, theta, g1, g2) -> Axes:
    """L0_d: the unit-outputscale factor of the step (at its jitter level)."""
    if "b1" in (f1.basis, f2.basis):
        raise NotImplementedError("B1 hats: the prior residual k - q is indefinite, the raster covariance has no Kronecker root")
    out = []
    for f, L0, ell, g in ((f1, L01, theta[0], g1), (f2, L02, theta[1], g2)):
        g = np.asarray(g, float)
        A0 = f.build(float(ell), x=g)[2]
        U = sla.solve_triangular(L0, A0, lower=True)
        k = Kr.kappa_and_dell(f.kind, np.abs(g[:, None] - g[None, :]), float(ell))[0]
        out.append((U, k, k - U.T @ U))
    (U1, k1, r1), (U2, k2, r2) = out
    C1, l1 = root(r1 + ETA * np.eye(len(r1)))
    C2, l2 = root(r2 + ETA * np.eye(len(r2)))
    Kc2, l3 = root(k2 + ETA * np.eye(len(k2)))
    return Axes(U1, U2, k1, k2, r1, r2, C1, C2, Kc2, (l1, l2, l3))


def combine(ax: Axes, theta, mu: np.ndarray, X: np.ndarray, eps_g: np.ndarray, eps_h: np.ndarray) -> np.ndarray:
    """mu [p1, p2], X [S, m1, m2], eps_g [S, p1, p2], eps_h [S, m1, p2] -> F [S, p1, p2]."""
    _, _, s1, s2, _ = [float(t) for t in theta]
    W = np.sqrt(s2) * (X @ ax.U2 + eps_h @ ax.C2.T)
    T = eps_g @ ax.Kc2.T
    return mu[None] + np.sqrt(s1) * (ax.U1.T @ W) + np.sqrt(s1 * s2) * (ax.C1 @ T)


def nugget_terms(ax: Axes, theta) -> np.ndarray:
    """What the nugget adds to Cov(vec F): s1 s2 eta (I (x) k2 + r1 (x) I + eta I (x) I) + s1 s2 eta (U1^T U1) (x) I."""
    _, _, s1, s2, _ = [float(t) for t in theta]
    I1, I2 = np.eye(len(ax.k1)), np.eye(len(ax.k2))
    return s1 * s2 * ETA * (np.kron(I1, ax.k2) + np.kron(ax.r1, I2) + ETA * np.kron(I1, I2) + np.kron(ax.U1.T @ ax.U1, I2))


def _unit_L0(d: Kr.DimState, f: Kr.Factor, s: float) -> np.ndarray:
    """oracle.kron.elbo_step keeps L_d = s_d^(e_d/2) L0_d."""
    return d.L * np.sqrt(s) if f.inverse else d.L / np.sqrt(s)


def x_full(st: Kr.StepState, eps_u: np.ndarray) -> np.ndarray:
    """The full grid's coefficient draw X_s = Q1 ((Q1^T E_s Q2) o D^-1/2) Q2^T (qv_sample_spec.sample_full's)."""
    Q1, Q2 = st.d1.Q, st.d2.Q
    return Q1 @ ((Q1.T @ eps_u @ Q2) / np.sqrt(st.D)) @ Q2.T


def axes_full(st: Kr.StepState, f1: Kr.Factor, f2: Kr.Factor, g1, g2) -> Axes:
    return axes(f1, f2, _unit_L0(st.d1, f1, st.theta[2]), _unit_L0(st.d2, f2, st.theta[3]), st.theta, g1, g2)


def mean_full(st: Kr.StepState, f1: Kr.Factor, f2: Kr.Factor, g1, g2) -> np.ndarray:
    g1, g2 = np.asarray(g1, float), np.asarray(g2, float)
    xs = np.stack([np.repeat(g1, len(g2)), np.tile(g2, len(g1))], axis=1)
    return Kr.posterior(st, f1, f2, xs)[0].reshape(len(g1), len(g2))


def sample_full(st: Kr.StepState, f1: Kr.Factor, f2: Kr.Factor, g1, g2, eps_u, eps_g, eps_h):
    """Full grid, from oracle.kron.elbo_step's state -> (F [S, p1, p2], root levels)."""
    ax = axes_full(st, f1, f2, g1, g2)
    return combine(ax, st.theta, mean_full(st, f1, f2, g1, g2), x_full(st, eps_u), eps_g, eps_h), ax.levels


def _sample_iter(st, ax: Axes, Z: np.ndarray, solve, eps_g, eps_h, block, tol, maxit):
    _, _, s1, s2, v = [float(t) for t in st.theta]
    X, info = S._blocks(solve, Z, block, tol, maxit)
    mu = (s1 * s2 / v) * (ax.U1.T @ st.A0 @ ax.U2)
    info["levels"] = ax.levels
    return combine(ax, st.theta, mu, X, eps_g, eps_h), info


def sample_masked(st: MS.IterState, f1: Kr.Factor, f2: Kr.Factor, g1, g2, eps_u, eps_obs, eps_g, eps_h, block: int = 64, tol: float = 1e-10,
                  maxit: int = 100):
    """Grid with holes, from masked_iter_readout_spec.prepare's state; eps_obs [S, n2, n1] -> (F [S, p1, p2], info)."""
    ax = axes(f1, f2, st.d1.L, st.d2.L, st.theta, g1, g2)
    F = st.Wt[None] * np.transpose(eps_obs, (0, 2, 1))
    Z = eps_u + np.sqrt(st.rho) * np.einsum("ai,sij,bj->sab", st.d1.B, F, st.d2.B, optimize=True)
    return _sample_iter(st, ax, Z, lambda T, t, m: MS.block_solve(st, T, t, m), eps_g, eps_h, block, tol, maxit)


def sample_scattered(st: SS.IterState, f1: Kr.Factor, f2: Kr.Factor, g1, g2, eps_u, eps_obs, eps_g, eps_h, block: int = 64, tol: float = 1e-10,
                     maxit: int = 100):
    """Scattered points, from scattered_iter_variance_spec.prepare's state; eps_obs [S, N] -> (F [S, p1, p2], info)."""
    ax = axes(f1, f2, st.d1.L, st.d2.L, st.theta, g1, g2)
    Z = eps_u + np.sqrt(st.rho) * np.einsum("ak,sk,bk->sab", st.d1.B, eps_obs, st.d2.B, optimize=True)
    return _sample_iter(st, ax, Z, lambda T, t, m: SS.block_solve(st, T, t, m), eps_g, eps_h, block, tol, maxit)


def unit_noise_egh(m1: int, m2: int, p1: int, p2: int):
    """The unit vectors of (E, G, H) as explicit noise plus one column of zeros: S = m1 m2 + p1 p2 + m1 p2 + 1."""
    nE, nG, nH = m1 * m2, p1 * p2, m1 * p2
    S_ = nE + nG + nH + 1
    E, G, H = np.zeros((S_, nE)), np.zeros((S_, nG)), np.zeros((S_, nH))
    E[np.arange(nE), np.arange(nE)] = 1.0
    G[nE + np.arange(nG), np.arange(nG)] = 1.0
    H[nE + nG + np.arange(nH), np.arange(nH)] = 1.0
    return E.reshape(S_, m1, m2), G.reshape(S_, p1, p2), H.reshape(S_, m1, p2)


def cartesian(g1, g2) -> np.ndarray:
    g1, g2 = np.asarray(g1, float), np.asarray(g2, float)
    return np.stack([np.repeat(g1, len(g2)), np.tile(g2, len(g1))], axis=1)
