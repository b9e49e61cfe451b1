"""Specification of the joint samples of q(v) (TEST HELPER, numpy float64, CPU): the counter-based normal generator
(vggp_normal_fill) and the three samplers vggp_qv_sample, vggp_qv_sample_masked_iter, vggp_qv_sample_scattered_iter.

All read-outs share one whitened form (tests/masked_iter_readout_spec.py):
    Cov q(v) = s1^e1 s2^e2 (L0_1 (x) L0_2) Sigma~^-1 (L0_1 (x) L0_2)^T,   Sigma~ = I + rho Phi,   rho = s1 s2 / sigma^2,
so sample s is  V_s = mean + sqrt(s1^e1 s2^e2) L0_1 X_s L0_2^T  with Cov(vec X_s) = Sigma~^-1.
    full grid   X_s = Sigma~^-1/2 E_s = Q1 ((Q1^T E_s Q2) o D^-1/2) Q2^T, D = 1 + rho lam1 lam2^T: the symmetric root, which does not
                depend on the signs, order or cluster bases of the eigenvectors
    iterative   Z_s = E_s + sqrt(rho) K F_s,  X_s = Sigma~^-1 Z_s by the block PCG of the read-out specifications;
                K F = B1 (W^T o F) B2^T on a grid with holes, sum_k F_k b1_k b2_k^T on scattered points; Cov(vec Z_s) = Sigma~ (W o W = W)
Noise: E_s standard normal [m1][m2]; F_s standard normal over the nodes [n2][n1] (the layout of Y and W) or the points [N].

Generator: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl increments 0x9E3779B9, 0xBB67AE85), key = (seed lo, seed hi),
counter = (c lo, c hi, stream, 0), c = idx >> 1; a = w0 << 21 | w1 >> 11, u1 = (a + 0.5) 2^-53, b = w2 << 21 | w3 >> 11,
u2 = (b + 0.5) 2^-53, r = sqrt(-2 ln u1); element idx = r cos(2 pi u2) (even idx), r sin(2 pi u2) (odd idx).
Index spaces: stream 0 (E) idx = s M + i1 m2 + i2; stream 1 (F) idx = s n1 n2 + j n1 + i (grid), s N + k (points); s = first + local.
"""
from __future__ import annotations

import numpy as np

import masked_iter_readout_spec as MS
import scattered_iter_variance_spec as SS
from oracle import kron as Kr

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (or [2]) of 32-bit words -> the four output words [..., 4] (uint64 holding 32-bit values)."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., k] & MASK32 for k in range(4)]
    key = np.asarray(key, dtype=np.uint64)
    k0, k1 = key[..., 0] & MASK32, key[..., 1] & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                   # 32 x 32 -> 64 bit, exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK32, p1 >> np.uint64(32), p1 & MASK32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return np.stack(c, axis=-1)


def normals_at(seed: int, stream: int, idx) -> np.ndarray:
    """The elements idx (any integer array) of the sequence (seed, stream)."""
    idx = np.asarray(idx, dtype=np.uint64)
    cnt = idx >> np.uint64(1)
    ctr = np.stack([cnt & MASK32, cnt >> np.uint64(32), np.full_like(cnt, stream), np.zeros_like(cnt)], axis=-1)
    seed = int(seed) & (2**64 - 1)
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    a = (w[..., 0] << np.uint64(21)) | (w[..., 1] >> np.uint64(11))
    b = (w[..., 2] << np.uint64(21)) | (w[..., 3] >> np.uint64(11))
    u1 = (a.astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = (b.astype(np.float64) + 0.5) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return np.where((idx & np.uint64(1)) == 0, r * np.cos(ang), r * np.sin(ang))


def normal_fill(seed: int, stream: int, first: int, n: int) -> np.ndarray:
    return normals_at(seed, stream, np.arange(first, first + n, dtype=np.uint64))


def noise_u(seed: int, first: int, S: int, m1: int, m2: int) -> np.ndarray:
    """E of samples first .. first + S: [S, m1, m2]."""
    return normal_fill(seed, 0, first * m1 * m2, S * m1 * m2).reshape(S, m1, m2)


def noise_obs_grid(seed: int, first: int, S: int, n1: int, n2: int) -> np.ndarray:
    """F of samples first .. first + S on a grid: [S, n2, n1], the layout of Y and W."""
    return normal_fill(seed, 1, first * n1 * n2, S * n1 * n2).reshape(S, n2, n1)


def noise_obs_points(seed: int, first: int, S: int, N: int) -> np.ndarray:
    return normal_fill(seed, 1, first * N, S * N).reshape(S, N)


def _scale(theta, f1: Kr.Factor, f2: Kr.Factor) -> float:
    _, _, s1, s2, _ = theta
    return float(np.sqrt(s1 ** (-1 if f1.inverse else 1) * s2 ** (-1 if f2.inverse else 1)))


def sample_full(st: Kr.StepState, eps_u: np.ndarray) -> np.ndarray:
    """Full grid, from oracle.kron.elbo_step's state (its L, lam carry the outputscales: L_d = s_d^(e_d/2) L0_d, D = 1 + lam1 lam2^T / v
    = 1 + rho lam0_1 lam0_2^T).  eps_u [S, m1, m2] -> [S, m1, m2]."""
    Q1, Q2 = st.d1.Q, st.d2.Q
    mean, _ = Kr.q_v(st)
    X = Q1 @ ((Q1.T @ eps_u @ Q2) / np.sqrt(st.D)) @ Q2.T
    return mean[None] + st.d1.L @ X @ st.d2.L.T


def _blocks(solve, Z: np.ndarray, block: int, tol: float, maxit: int):
    S = Z.shape[0]
    X = np.empty_like(Z)
    most, solves, conv = 0, 0, True
    for off in range(0, S, block):
        cn = min(block, S - off)
        T = np.zeros((min(block, S),) + Z.shape[1:])
        T[:cn] = Z[off:off + cn]
        Xb, its, ok = solve(T, tol, maxit)
        X[off:off + cn] = Xb[:cn]
        most, solves, conv = max(most, its), solves + 1, conv and ok
    return X, {"rounds": most, "solves": solves, "converged": conv}


def sample_masked(st: MS.IterState, f1: Kr.Factor, f2: Kr.Factor, eps_u: np.ndarray, eps_obs: np.ndarray, block: int = 64,
                  tol: float = 1e-10, maxit: int = 100):
    """Grid with holes, from masked_iter_readout_spec.prepare's state.  eps_u [S, m1, m2], eps_obs [S, n2, n1] -> ([S, m1, m2], info)."""
    mean, _, _ = MS.q_v(st, f1, f2, cells=[0], tol=tol, maxit=maxit)
    F = st.Wt[None] * np.transpose(eps_obs, (0, 2, 1))                                  # [S, n1, n2], unobserved nodes drop out
    Z = eps_u + np.sqrt(st.rho) * np.einsum("ai,sij,bj->sab", st.d1.B, F, st.d2.B, optimize=True)
    X, info = _blocks(lambda T, t, m: MS.block_solve(st, T, t, m), Z, block, tol, maxit)
    return mean[None] + _scale(st.theta, f1, f2) * (st.d1.L @ X @ st.d2.L.T), info


def sample_scattered(st: SS.IterState, f1: Kr.Factor, f2: Kr.Factor, eps_u: np.ndarray, eps_obs: np.ndarray, block: int = 64,
                     tol: float = 1e-10, maxit: int = 100):
    """Scattered points, from scattered_iter_variance_spec.prepare's state.  eps_u [S, m1, m2], eps_obs [S, N] -> ([S, m1, m2], info)."""
    mean, _, _ = SS.q_v(st, f1, f2, cells=[0], tol=tol, maxit=maxit)
    Z = eps_u + np.sqrt(st.rho) * np.einsum("ak,sk,bk->sab", st.d1.B, eps_obs, st.d2.B, optimize=True)
    X, info = _blocks(lambda T, t, m: SS.block_solve(st, T, t, m), Z, block, tol, maxit)
    return mean[None] + _scale(st.theta, f1, f2) * (st.d1.L @ X @ st.d2.L.T), info
