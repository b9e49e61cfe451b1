"""Specification of the variance read-outs of the iterative scattered step (TEST HELPER, numpy float64, CPU): what
vggp_qv_var_scattered_iter / vggp_posterior_var_scattered_iter compute.

tests/masked_iter_readout_spec.py with the operator and preconditioner of tests/scattered_iter_spec.py (whose data sets, theta_a /
theta_b and factor helpers are imported; its operator and preconditioner are local to its step function and are restated here in
the same words).  Everything at unit outputscale, rho = s1 s2 / sigma^2, B_d = L0_d^-1 A0_d(x_d) (m_d x N):
    operator         Sigma~ V = V + rho sum_k b1_k (b1_k^T V b2_k) b2_k^T
    preconditioner   P = I + (rho / N) G1 (x) G2,  G_d = B_d B_d^T = Q_d diag(lam_d) Q_d^T
Every read-out quantity belongs to a rank-one whitened column t = u1 (x) u2 (T = u1 u2^T as a matrix):
    mean = (s1 s2 / sigma^2) <T, A0>,      var = s1 s2 (kappa - |T|^2 + <T, Sigma~^-1 T>),      A0 = Sigma~^-1 c0,  c0 = B1 diag(y) B2^T
    posterior(x*)      u_d = L0_d^-1 a_d(x*_d),  kappa = 1
    q(v) at (i1, i2)   u_d = row i_d of L0_d,    kappa = |T|^2  ->  var = s1^e1 s2^e2 <T, Sigma~^-1 T>   (e_d = -1 for VFF / B1)
    q(v) mean          (s1^((1+e1)/2) s2^((1+e2)/2) / sigma^2) L0_1 A0 L0_2^T                             (no solve)
<T, Sigma~^-1 T> comes from block PCG solves Sigma~ X = T over `block` columns at a time, each column stopping on its own at
|r| <= tol |r0|.  No probes: deterministic.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.linalg as sla

from oracle import kron as Kr

from scattered_iter_spec import THETA_A, THETA_B, b0_factors, rand20k, trk  # noqa: F401  (the data sets of the tests)


@dataclass
class IterState:
    theta: np.ndarray
    d1: Kr.DimState            # unit outputscale: L = L0, B = L0^-1 A0 at the points
    d2: Kr.DimState
    Q1: np.ndarray
    Q2: np.ndarray
    dP: np.ndarray             # 1 + (rho / N) lam1 lam2^T
    rho: float
    chunk: int
    A0: np.ndarray = None      # Sigma~^-1 c0  (m1 x m2)
    iters: int = 0


def _rot(st: IterState, V, w):
    return st.Q1 @ ((st.Q1.T @ V @ st.Q2) * w) @ st.Q2.T


def _op(st: IterState, V):
    """Sigma~ V for V [nc, m1, m2]: field F[c, k] = b1_k^T V_c b2_k, back sum_k F[c, k] b1_k b2_k^T, over chunks of points."""
    B1, B2 = st.d1.B, st.d2.B
    out = np.zeros_like(V)
    for o in range(0, B1.shape[1], st.chunk):
        L, R = B1[:, o:o + st.chunk], B2[:, o:o + st.chunk]
        F = (L[None] * (V @ R)).sum(axis=1)                    # [c, k]
        out += (L[None] * F[:, None, :]) @ R.T                 # [c, a, k] @ [k, b]
    return V + st.rho * out


def block_solve(st: IterState, T: np.ndarray, tol: float = 1e-10, maxit: int = 100):
    """Sigma~ X = T for a block T [nc, m1, m2] by preconditioned CG; -> (X, iterations, all columns converged).  A zero column
    (the padding of a ragged last block) starts inactive."""
    dots = lambda A, B: (A * B).sum(axis=(1, 2))
    X = np.zeros_like(T)
    R = T.copy()
    Zp = _rot(st, R, 1.0 / st.dP)
    Pd = Zp.copy()
    rz = dots(R, Zp)
    r02 = dots(R, R)
    active = r02 > 0.0
    its = 0
    for its in range(1, maxit + 1):
        if not active.any():
            its -= 1
            break
        AP = _op(st, Pd)
        pAp = dots(Pd, AP)
        al = np.where(active & (pAp > 0), rz / np.where(pAp > 0, pAp, 1.0), 0.0)
        X += al[:, None, None] * Pd
        R -= al[:, None, None] * AP
        Zp = _rot(st, R, 1.0 / st.dP)
        rz_new = dots(R, Zp)
        be = np.where(active & (rz > 0), rz_new / np.where(rz > 0, rz, 1.0), 0.0)
        Pd = Zp + be[:, None, None] * Pd
        rz = rz_new
        active &= dots(R, R) > tol * tol * r02
    return X, its, not active.any()


def prepare(X, y, f1: Kr.Factor, f2: Kr.Factor, theta, tol: float = 1e-10, maxit: int = 100, chunk: int = 8192) -> IterState:
    """What the iterative scattered step leaves behind for the read-outs: factors at the points, preconditioner basis,
    A0 = Sigma~^-1 c0 (by the same PCG)."""
    ell1, ell2, s1, s2, v = [float(t) for t in theta]
    X = np.asarray(X, float)
    y = np.asarray(y, float).reshape(-1)
    g1 = Kr.Factor(f1.basis, f1.kind, f1.grid, X[:, 0].copy(), f1.f32_kdelta)
    g2 = Kr.Factor(f2.basis, f2.kind, f2.grid, X[:, 1].copy(), f2.f32_kdelta)
    d1, d2 = Kr.dim_prepare(g1, ell1, 1.0), Kr.dim_prepare(g2, ell2, 1.0)
    lam1, Q1 = np.linalg.eigh(d1.B @ d1.B.T)
    lam2, Q2 = np.linalg.eigh(d2.B @ d2.B.T)
    rho = s1 * s2 / v
    dP = 1.0 + (rho / len(y)) * np.outer(np.maximum(lam1, 0.0), np.maximum(lam2, 0.0))
    st = IterState(theta=np.asarray(theta, float), d1=d1, d2=d2, Q1=Q1, Q2=Q2, dP=dP, rho=rho, chunk=chunk)
    c0 = (d1.B * y[None, :]) @ d2.B.T
    Xs, st.iters, ok = block_solve(st, c0[None], tol, maxit)
    assert ok, "the PCG for a0 did not converge"
    st.A0 = Xs[0]
    return st


def _chunks(st: IterState, U1: np.ndarray, U2: np.ndarray, block: int, tol: float, maxit: int):
    """lin, nrm, quad of the columns t_c = U1[:, c] (x) U2[:, c], `block` columns per solve; info = (max iterations, solves,
    every column converged)."""
    nc = U1.shape[1]
    lin, nrm, quad = np.empty(nc), np.empty(nc), np.empty(nc)
    most, solves, conv = 0, 0, True
    for off in range(0, nc, block):
        cn = min(block, nc - off)
        T = np.zeros((min(block, nc), U1.shape[0], U2.shape[0]))
        T[:cn] = np.einsum("ac,bc->cab", U1[:, off:off + cn], U2[:, off:off + cn])
        X, its, ok = block_solve(st, T, tol, maxit)
        most, solves, conv = max(most, its), solves + 1, conv and ok
        lin[off:off + cn] = (T[:cn] * st.A0[None]).sum(axis=(1, 2))
        nrm[off:off + cn] = (T[:cn] * T[:cn]).sum(axis=(1, 2))
        quad[off:off + cn] = (T[:cn] * X[:cn]).sum(axis=(1, 2))
    return lin, nrm, quad, {"rounds": most, "solves": solves, "converged": conv}


def q_v(st: IterState, f1: Kr.Factor, f2: Kr.Factor, cells=None, block: int = 64, tol: float = 1e-10, maxit: int = 100):
    """-> mean (m1, m2) of every cell, var [len(cells)] (cells: flat indices i1*m2 + i2; None: every cell), info."""
    _, _, s1, s2, v = st.theta
    L1, L2 = st.d1.L, st.d2.L
    e1, e2 = (-1 if f1.inverse else 1), (-1 if f2.inverse else 1)
    mean = (s1 ** ((1 + e1) / 2) * s2 ** ((1 + e2) / 2) / v) * (L1 @ st.A0 @ L2.T)
    m2 = L2.shape[0]
    cells = np.arange(L1.shape[0] * m2) if cells is None else np.asarray(cells, dtype=np.int64)
    _, _, quad, info = _chunks(st, L1[cells // m2].T, L2[cells % m2].T, block, tol, maxit)
    return mean, (s1 ** e1) * (s2 ** e2) * quad, info


def posterior(st: IterState, f1: Kr.Factor, f2: Kr.Factor, x_star: np.ndarray, block: int = 64, tol: float = 1e-10, maxit: int = 100):
    """-> mean [ns], var [ns], info at x_star (ns, 2)."""
    ell1, ell2, s1, s2, v = st.theta
    U = []
    for f, d, ell, col in ((f1, st.d1, ell1, 0), (f2, st.d2, ell2, 1)):
        _, _, A0, _ = f.build(ell, x=np.asarray(x_star[:, col], float))
        U.append(sla.solve_triangular(d.L, A0, lower=True))
    lin, nrm, quad, info = _chunks(st, U[0], U[1], block, tol, maxit)
    return (s1 * s2 / v) * lin, s1 * s2 * (1.0 - nrm + quad), info
