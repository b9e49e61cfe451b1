"""Specification of the gridded read-out q(v) after an iterative step (TEST HELPER, numpy float64, CPU): what
vggp_readout_masked_iter / vggp_readout_scattered_iter compute -- the algebra of vggp_readout_masked (oracle/kron.py readout on the dense
M-space state) with Sigma~^-1 applied instead of stored.

Everything at unit outputscale, as scattered_iter_spec / masked_iter_readout_spec: Sigma~ = I + rho Phi, rho = s1 s2 / sigma^2,
    scattered   Phi V = sum_k b1_k (b1_k^T V b2_k) b2_k^T                  P = I + (rho / N) G1 (x) G2
    masked      Phi V = B1 (W^T o (B1^T V B2)) B2^T                         P = I + rho p G1 (x) G2, p = observed fraction
U_d = L0_d^-1 C_d^T (m_d x mv_d); output cell (a, b) owns the rank-one column t = U1[:, a] (x) U2[:, b]; P_d = U_d^T B_d (mv_d x n_d):
    mean          rho U1^T A0 U2                                             all cells, no solve
    literal       s1 s2 (kd1_a kd2_b - |t|^2 + t^T Sigma~ t) = s1 s2 (kd1_a kd2_b + rho S[a, b])       no solve
                  scattered S = (P1 o P1)(P2 o P2)^T,   masked S = (P1 o P1) W^T (P2 o P2)^T  (W [n2][n1])
    conditional   s1 s2 (kd1_a kd2_b - |t|^2 + t^T Sigma~^-1 t)              block PCG solves Sigma~ X = T, `block` cells at a time
The scaling is the same for every basis (VFF and B1 included: L^-1 Kuv = sqrt(s) L0^-1 C^T whether Kuu carries s or 1 / s).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import numpy as np
import scipy.linalg as sla

import masked_iter_readout_spec as MS
from oracle import kron as Kr


@dataclass
class State:
    theta: np.ndarray
    d1: Kr.DimState            # unit outputscale: L = L0, B = L0^-1 A0 at the data
    d2: Kr.DimState
    Q1: np.ndarray
    Q2: np.ndarray
    dP: np.ndarray
    rho: float
    op: Callable               # V [nc, m1, m2] -> Sigma~ V
    Wt: np.ndarray = None      # masked: [n1][n2]; scattered: None
    A0: np.ndarray = None
    iters: int = 0


def _rot(st: State, V, w):
    return st.Q1 @ ((st.Q1.T @ V @ st.Q2) * w) @ st.Q2.T


def block_solve(st: State, T: np.ndarray, tol: float = 1e-10, maxit: int = 100):
    """masked_iter_readout_spec.block_solve with the state's own operator: -> (X, iterations, all columns converged)."""
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
        AP = st.op(Pd)
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


def prepare_scattered(X, y, f1: Kr.Factor, f2: Kr.Factor, theta, tol: float = 1e-10, maxit: int = 100, chunk: int = 8192) -> State:
    """What vggp_elbo_step_scattered_iter leaves behind for the read-outs (scattered_iter_spec's operator and preconditioner; a0 by the
    same PCG without the probe columns)."""
    ell1, ell2, s1, s2, v = [float(t) for t in theta]
    X = np.asarray(X, float)
    y = np.asarray(y, float).reshape(-1)
    N = len(y)
    g1 = Kr.Factor(f1.basis, f1.kind, f1.grid, X[:, 0].copy(), f1.f32_kdelta)
    g2 = Kr.Factor(f2.basis, f2.kind, f2.grid, X[:, 1].copy(), f2.f32_kdelta)
    d1, d2 = Kr.dim_prepare(g1, ell1, 1.0), Kr.dim_prepare(g2, ell2, 1.0)
    B1, B2 = d1.B, d2.B
    rho = s1 * s2 / v

    def op(V):
        out = V.copy()
        for o in range(0, N, chunk):
            L, R = B1[:, o:o + chunk], B2[:, o:o + chunk]
            F = np.einsum("ak,cak->ck", L, np.einsum("cab,bk->cak", V, R, optimize=True), optimize=True)
            out += rho * np.einsum("ak,ck,bk->cab", L, F, R, optimize=True)
        return out

    lam1, Q1 = np.linalg.eigh(B1 @ B1.T)
    lam2, Q2 = np.linalg.eigh(B2 @ B2.T)
    dP = 1.0 + (rho / N) * np.outer(np.maximum(lam1, 0.0), np.maximum(lam2, 0.0))
    st = State(theta=np.asarray(theta, float), d1=d1, d2=d2, Q1=Q1, Q2=Q2, dP=dP, rho=rho, op=op)
    c0 = (B1 * y[None, :]) @ B2.T
    Xs, st.iters, ok = block_solve(st, c0[None], tol, maxit)
    assert ok, "the PCG for a0 did not converge"
    st.A0 = Xs[0]
    return st


def prepare_masked(Y: np.ndarray, W: np.ndarray, f1: Kr.Factor, f2: Kr.Factor, theta, tol: float = 1e-10, maxit: int = 100) -> State:
    """The state masked_iter_readout_spec.prepare builds (Y, W [n2][n1]), with its operator."""
    ms = MS.prepare(Y, W, f1, f2, theta, tol, maxit)
    return State(theta=ms.theta, d1=ms.d1, d2=ms.d2, Q1=ms.Q1, Q2=ms.Q2, dP=ms.dP, rho=ms.rho, op=lambda V: MS._op(ms, V), Wt=ms.Wt,
                 A0=ms.A0, iters=ms.iters)


def whitened_cross(st: State, C1: np.ndarray, C2: np.ndarray):
    """U_d = L0_d^-1 C_d^T for unit-outputscale cross-covariances C_d (mv_d x m_d)."""
    return (sla.solve_triangular(st.d1.L, np.asarray(C1, float).T, lower=True),
            sla.solve_triangular(st.d2.L, np.asarray(C2, float).T, lower=True))


def sqgram(st: State, U1: np.ndarray, U2: np.ndarray) -> np.ndarray:
    """S[a, b] = t_ab^T Phi t_ab for every cell, as one Gram product over the data."""
    P1, P2 = U1.T @ st.d1.B, U2.T @ st.d2.B
    if st.Wt is None:
        return (P1 * P1) @ (P2 * P2).T
    return (P1 * P1) @ st.Wt @ (P2 * P2).T


def readout(st: State, C1, C2, kd1, kd2, literal: bool = True, cells=None, block: int = 64, tol: float = 1e-10, maxit: int = 100):
    """-> mean (mv1, mv2) of every cell, var [len(cells)] (cells: flat indices a*mv2 + b; None: every cell), info with the largest
    PCG count ("rounds") and the number of block solves ("solves": 0 on the literal path)."""
    _, _, s1, s2, v = st.theta
    U1, U2 = whitened_cross(st, C1, C2)
    mv1, mv2 = U1.shape[1], U2.shape[1]
    mean = st.rho * (U1.T @ st.A0 @ U2)
    cells = np.arange(mv1 * mv2) if cells is None else np.asarray(cells, dtype=np.int64)
    a, b = cells // mv2, cells % mv2
    kk = np.asarray(kd1, float)[a] * np.asarray(kd2, float)[b]
    if literal:
        return mean, s1 * s2 * (kk + st.rho * sqgram(st, U1, U2)[a, b]), {"rounds": 0, "solves": 0}
    nc = len(cells)
    nrm, quad = np.empty(nc), np.empty(nc)
    most, solves = 0, 0
    for off in range(0, nc, block):
        cn = min(block, nc - off)
        T = np.zeros((min(block, nc), U1.shape[0], U2.shape[0]))
        T[:cn] = np.einsum("ic,jc->cij", U1[:, a[off:off + cn]], U2[:, b[off:off + cn]])
        X, its, ok = block_solve(st, T, tol, maxit)
        assert ok, "a read-out column did not converge"
        most, solves = max(most, its), solves + 1
        nrm[off:off + cn] = (T[:cn] * T[:cn]).sum(axis=(1, 2))
        quad[off:off + cn] = (T[:cn] * X[:cn]).sum(axis=(1, 2))
    return mean, s1 * s2 * (kk - nrm + quad), {"rounds": most, "solves": solves}


def dense_sigma(st: State) -> np.ndarray:
    """Sigma~ as an M x M matrix (small M only): the reference the block solves are checked against."""
    m1, m2 = st.d1.B.shape[0], st.d2.B.shape[0]
    if st.Wt is None:
        K = (st.d1.B[:, None, :] * st.d2.B[None, :, :]).reshape(m1 * m2, -1)
        Phi = K @ K.T
    else:
        n1, n2 = st.Wt.shape
        K = (st.d1.B[:, None, :, None] * st.d2.B[None, :, None, :]).reshape(m1 * m2, n1 * n2)
        Phi = (K * st.Wt.reshape(-1)[None, :]) @ K.T
    return np.eye(m1 * m2) + st.rho * Phi


def readout_dense(st: State, C1, C2, kd1, kd2, literal: bool):
    """The same read-out through the dense Sigma~ (t^T Sigma~ t resp. t^T Sigma~^-1 t for every cell): -> var (mv1 mv2,)."""
    _, _, s1, s2, _ = st.theta
    U1, U2 = whitened_cross(st, C1, C2)
    T = np.einsum("ia,jb->ijab", U1, U2).reshape(U1.shape[0] * U2.shape[0], -1)
    Sg = dense_sigma(st)
    ST = Sg @ T if literal else np.linalg.solve(Sg, T)
    kk = np.outer(kd1, kd2).reshape(-1)
    return s1 * s2 * (kk - (T * T).sum(0) + (T * ST).sum(0))
