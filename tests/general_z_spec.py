"""M-space specification of the paired (general) inducing points -- GriddedMatern12SVGP with any Z (TEST HELPER, float64, CPU).

kernel = kernel_1 * kernel_2 on active dims 0 / 1 (gridded_kronecker_structure.py:235-264):
    Kuu = s (K1 o K2) + eps I (eps: psd_safe_cholesky on Kuu itself),  Kuf = s B,  B[i, k] = k1(z_i1, x_k1) k2(z_i2, x_k2),  s = s1 s2
    P0 = B B^T, b = B y (full grid: P0 = (A1 A1^T) o (A2 A2^T), b_i = sum_b (A1 Y^T)[i, b] A2[i, b]),  Sigma = Kj + s^2 P0 / v
    ELBO = -1/2 [N log 2 pi v + log|Sigma| - log|Kj| + y^T y / v - c^T Sigma^-1 c / v^2] - (N s - tr(Kj^-1 Phi)) / (2 v),  c = s b
Read-outs: q(u) mean Kj alpha / v, cov Kj Sigma^-1 Kj (alpha = Sigma^-1 c); q(v) on B0 cells with Kvu = s (C1 face-split C2);
posterior(x*) with k(x*, Z).  Differentiable in theta and Z (torch autograd): the gradients of the engine are checked against it.
"""
from __future__ import annotations

import math

import torch

from oracle.dense import DT, kappa, psd_safe_cholesky


def unit_k(kind, a, b, ell):
    return kappa(kind, torch.abs(a[:, None] - b[None, :]) / ell)


def _parts(kinds, Z, theta, y, X=None, grid=None):
    """-> Kj, P0, b, N, yy, eps.  X (N, 2) scattered points, or grid = (x1, x2) with y as Y [n2][n1]."""
    k1, k2 = kinds
    ell1, ell2, s1, s2, v = theta[0], theta[1], theta[2], theta[3], theta[4]
    s = s1 * s2
    Kuu = s * unit_k(k1, Z[:, 0], Z[:, 0], ell1) * unit_k(k2, Z[:, 1], Z[:, 1], ell2)
    eps = psd_safe_cholesky(Kuu.detach())[1]
    Kj = Kuu + eps * torch.eye(Z.shape[0], dtype=DT)
    if grid is None:
        B = unit_k(k1, Z[:, 0], X[:, 0], ell1) * unit_k(k2, Z[:, 1], X[:, 1], ell2)
        P0, b, N = B @ B.T, B @ y, X.shape[0]
    else:
        x1, x2 = grid
        A1, A2 = unit_k(k1, Z[:, 0], x1, ell1), unit_k(k2, Z[:, 1], x2, ell2)
        P0 = (A1 @ A1.T) * (A2 @ A2.T)
        b = ((A1 @ y.T) * A2).sum(1)
        N = x1.shape[0] * x2.shape[0]
    return Kj, P0, b, N, (y * y).sum(), eps


def elbo(kinds, Z, theta, y, X=None, grid=None):
    """-> (ELBO, jitter)."""
    Kj, P0, b, N, yy, eps = _parts(kinds, Z, theta, y, X, grid)
    s, v = theta[2] * theta[3], theta[4]
    Sig = Kj + (s * s / v) * P0
    Lk, Ls = torch.linalg.cholesky(Kj), torch.linalg.cholesky(Sig)
    c = s * b
    alpha = torch.cholesky_solve(c[:, None], Ls)[:, 0]
    trKP = s * s * torch.trace(torch.cholesky_solve(P0, Lk))
    e = -0.5 * (N * torch.log(2 * math.pi * v) + 2 * torch.log(torch.diagonal(Ls)).sum() - 2 * torch.log(torch.diagonal(Lk)).sum()
                + yy / v - (c * alpha).sum() / (v * v)) - (N * s - trKP) / (2 * v)
    return e, eps


def state(kinds, Z, theta, y, X=None, grid=None):
    """Detached M-space state for the read-outs: dict(Kj, Kinv, Sinv, alpha, P0, s, v)."""
    with torch.no_grad():
        Kj, P0, b, N, yy, eps = _parts(kinds, Z, theta, y, X, grid)
        s, v = theta[2] * theta[3], theta[4]
        Sinv = torch.linalg.inv(Kj + (s * s / v) * P0)
        Kinv = torch.linalg.inv(Kj)
        return dict(Kj=Kj, Kinv=Kinv, Sinv=Sinv, alpha=Sinv @ (s * b), P0=P0, s=s, v=v)


def q_u(st):
    Kj = st["Kj"]
    return Kj @ st["alpha"] / st["v"], Kj @ st["Sinv"] @ Kj


def q_v(st, C1, C2, kd1, kd2, literal=True):
    """C_d [mv_d, M] unit-outputscale Cov(v, u) along d, kd_d [mv_d] unit diag(Kvv_d) -> mean, var [mv1 mv2] (flat a mv2 + b)."""
    s, v = st["s"], st["v"]
    F = (C1[:, None, :] * C2[None, :, :]).reshape(-1, C1.shape[1])
    Q = s * s * st["Kinv"] @ st["P0"] @ st["Kinv"] / v if literal else st["Sinv"] - st["Kinv"]
    mean = (s / v) * F @ st["alpha"]
    var = s * (kd1[:, None] * kd2[None, :]).reshape(-1) + s * s * ((F @ Q) * F).sum(1)
    return mean, var


def posterior(st, kinds, Z, theta, xs):
    s, v = st["s"], st["v"]
    with torch.no_grad():
        Bs = unit_k(kinds[0], Z[:, 0], xs[:, 0], theta[0]) * unit_k(kinds[1], Z[:, 1], xs[:, 1], theta[1])
        mean = (s / v) * Bs.T @ st["alpha"]
        prior = s * unit_k(kinds[0], xs[:, 0], xs[:, 0], theta[0]) * unit_k(kinds[1], xs[:, 1], xs[:, 1], theta[1])
        cov = prior + s * s * Bs.T @ (st["Sinv"] - st["Kinv"]) @ Bs
    return mean, cov
