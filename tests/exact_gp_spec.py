"""Specification of the exact GP on scattered 2-D points (TEST HELPER, float64, CPU): the reference's Matern12GP / Matern32GP /
Matern52GP (src/models/exact/bivariate_structure.py) and GriddedMatern12ExactGP (gridded_kronecker_structure.py:21-211).

kernel = kernel_1 * kernel_2 on active dims 0 / 1, theta = (ell1, ell2, s1, s2, v), s = s1 s2:
    K0[i, j] = k1(|x_i1 - x_j1| / ell1) k2(|x_i2 - x_j2| / ell2),  Sigma = s K0 + (v + eps) I  (eps: psd_safe_cholesky on Sigma itself)
    MLL = -1/2 [y^T Sigma^-1 y + log|Sigma| + N log 2 pi]
posterior(x*): mean s B*^T alpha, cov s K0** - s^2 B*^T Sigma^-1 B*;  q(v) on B0 cells with Kvx = s (C1 face-split C2), flat a mv2 + b:
mean Kvx alpha, var s kd1 kd2 + diag(Kvx Kxv) / v (literal) or s kd1 kd2 - diag(Kvx Sigma^-1 Kxv) (conditional).
Differentiable in theta (torch autograd): the engine's gradient is checked against it.
"""
from __future__ import annotations

import math

import torch

from oracle.dense import DT, b0_Kuf_along_dim, b0_Kuu_along_dim, kappa, psd_safe_cholesky


def unit_k(kind, a, b, ell):
    return kappa(kind, torch.abs(a[:, None] - b[None, :]) / ell)


def K0(kinds, X, theta, X2=None):
    X2 = X if X2 is None else X2
    return unit_k(kinds[0], X[:, 0], X2[:, 0], theta[0]) * unit_k(kinds[1], X[:, 1], X2[:, 1], theta[1])


def sigma(kinds, X, theta):
    """-> (Sigma with its jitter, jitter)."""
    S = theta[2] * theta[3] * K0(kinds, X, theta) + theta[4] * torch.eye(X.shape[0], dtype=DT)
    eps = psd_safe_cholesky(S.detach())[1]
    return S + eps * torch.eye(X.shape[0], dtype=DT), eps


def mll(kinds, X, theta, y):
    """-> (log marginal likelihood, jitter)."""
    S, eps = sigma(kinds, X, theta)
    L = torch.linalg.cholesky(S)
    z = torch.linalg.solve_triangular(L, y[:, None], upper=False)[:, 0]
    return -0.5 * ((z * z).sum() + 2.0 * torch.log(torch.diagonal(L)).sum() + X.shape[0] * math.log(2.0 * math.pi)), eps


def analytic_grad(kinds, X, theta, y):
    """The formulas the engine implements: W = alpha alpha^T - Sigma^-1, dMLL/dell_d = (s / 2) <W, dK0/dell_d>,
    dMLL/ds1 = <W, K0> s2 / 2, dMLL/dv = tr W / 2 (dK0/dell_d by autograd of the unit kernel alone)."""
    th = theta.detach()
    s = th[2] * th[3]
    Sinv = torch.linalg.inv(sigma(kinds, X, th)[0])
    alpha = Sinv @ y
    W = alpha[:, None] * alpha[None, :] - Sinv
    ell = th[:2].clone().requires_grad_(True)
    k = K0(kinds, X, ell)
    g1, g2 = torch.autograd.grad((W * k).sum(), ell)[0]
    wk = (W * k.detach()).sum()
    return torch.stack([0.5 * s * g1, 0.5 * s * g2, 0.5 * wk * th[3], 0.5 * wk * th[2], 0.5 * torch.trace(W)])


def state(kinds, X, theta, y):
    """Detached state for the read-outs: dict(Sinv, alpha, s, v, eps)."""
    with torch.no_grad():
        S, eps = sigma(kinds, X, theta)
        Sinv = torch.linalg.inv(S)
        return dict(Sinv=Sinv, alpha=Sinv @ y, s=theta[2] * theta[3], v=theta[4], eps=eps)


def posterior(st, kinds, X, theta, xs):
    """-> mean [ns], cov [ns, ns] (the predictive distribution adds v to the diagonal)."""
    s = st["s"]
    with torch.no_grad():
        Bs = K0(kinds, X, theta, xs)
        return s * Bs.T @ st["alpha"], s * K0(kinds, xs, theta) - s * s * Bs.T @ st["Sinv"] @ Bs


def b0_operands(X, mesh1, mesh2, theta):
    """C_d [mv_d, N] unit-outputscale Cov(v, f(x_i)) along d (:52-101) and kd_d [mv_d] unit diag(Kvv_d) (:111-149)."""
    one = torch.tensor(1.0, dtype=DT)
    out = []
    for d, mesh in ((0, mesh1), (1, mesh2)):
        out.append(b0_Kuf_along_dim(mesh, theta[d], one, X[:, d].contiguous()))
    kd = [torch.diagonal(b0_Kuu_along_dim(mesh.shape[0] - 1, mesh[1] - mesh[0], theta[d], one)).clone()
          for d, mesh in ((0, mesh1), (1, mesh2))]
    return out[0], out[1], kd[0], kd[1]


def q_v(st, C1, C2, kd1, kd2, literal=True):
    """-> mean, var [mv1 mv2] (flat a mv2 + b)."""
    s, v = st["s"], st["v"]
    F = s * (C1[:, None, :] * C2[None, :, :]).reshape(-1, C1.shape[1])
    prior = s * (kd1[:, None] * kd2[None, :]).reshape(-1)
    var = prior + (F * F).sum(1) / v if literal else prior - ((F @ st["Sinv"]) * F).sum(1)
    return F @ st["alpha"], var


def q_v_cov_as_written(kinds, X, theta, mesh1, mesh2):
    """The reference's q_v covariance literally (:177-191): Kvv - Kvx Kxx^-1 Kxv + Kvx P^-1 Kxv, P = Kxx - Kxx Sigma^-1 Kxx, with Kxx
    inverted WITHOUT noise (toy sizes only), Kvv = Kvv_1 (x) Kvv_2 in the flat order a mv2 + b of Kvx."""
    one = torch.tensor(1.0, dtype=DT)
    s, v = theta[2] * theta[3], theta[4]
    Kxx = s * K0(kinds, X, theta)
    C1, C2, _, _ = b0_operands(X, mesh1, mesh2, theta)
    Kvx = s * (C1[:, None, :] * C2[None, :, :]).reshape(-1, X.shape[0])
    Kvv = s * torch.kron(b0_Kuu_along_dim(mesh1.shape[0] - 1, mesh1[1] - mesh1[0], theta[0], one),
                         b0_Kuu_along_dim(mesh2.shape[0] - 1, mesh2[1] - mesh2[0], theta[1], one))
    Sig = Kxx + v * torch.eye(X.shape[0], dtype=DT)
    P = Kxx - Kxx @ torch.linalg.solve(Sig, Kxx)
    return Kvv - Kvx @ torch.linalg.solve(Kxx, Kvx.T) + Kvx @ torch.linalg.solve(P, Kvx.T), Kxx
