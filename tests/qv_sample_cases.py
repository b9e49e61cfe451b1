"""The small problems the joint-sample tests share (TEST HELPER): M = m1 m2 = 24 inducing features (6 x 4) on a 14 x 11 grid with
30 % of the nodes missing, and on 150 scattered points; three kernel-evaluated bases and one inter-domain basis (e_d = -1)."""
from __future__ import annotations

import numpy as np

from oracle import dense as D
from oracle import kron as Kr

THETA = [0.2, 0.3, 1.0, 0.8, 0.01]
N1, N2, NPTS = 14, 11, 150
# id -> (basis, kind, grid_1 (m1 = 6), grid_2 (m2 = 4))
BASES = {"b0-matern12": ("b0", "matern12", np.linspace(0, 1, 7), np.linspace(0, 1, 5)),
         "points-matern32": ("points", "matern32", np.linspace(0, 1, 6), np.linspace(0, 1, 4)),
         "points-rbf": ("points", "rbf", np.linspace(0, 1, 6), np.linspace(0, 1, 4)),
         "b1-matern12": ("b1", "matern12", np.linspace(0, 1, 6), np.linspace(0, 1, 4))}       # hats: Kuu_d = K0 / s_d, e_d = -1
KERNEL_BASES = ["b0-matern12", "points-matern32", "points-rbf"]


def grid_data():
    """-> Y [n2, n1], W [n2, n1] (0/1), x1, x2."""
    _, y, x1, x2 = D.gen_grid(N1, N2)
    W = (np.random.default_rng(1).uniform(size=(N2, N1)) < 0.7).astype(np.float64)
    return y.reshape(N2, N1), W, x1, x2


def scattered_data():
    """-> X [N, 2], y [N]."""
    rng = np.random.default_rng(2)
    X = rng.uniform(0, 1, (NPTS, 2))
    y = np.asarray(D.latent_2d(X[:, 0], X[:, 1])) + 0.05 * rng.standard_normal(NPTS)
    return X, y


def factors(case: str, x1, x2):
    basis, kind, g1, g2 = BASES[case]
    return Kr.Factor(basis, kind, g1, np.asarray(x1, float)), Kr.Factor(basis, kind, g2, np.asarray(x2, float))


def unit_noise(m1: int, m2: int, n_obs_nodes):
    """The unit vectors of (E, F) as explicit noise: eps_u [S, m1, m2], eps_obs [S, *n_obs_nodes], S = m1 m2 + prod(n_obs_nodes);
    sample s < M has E = e_s, F = 0, sample M + t has E = 0, F = e_t."""
    M, No = m1 * m2, int(np.prod(n_obs_nodes))
    eps_u = np.zeros((M + No, M))
    eps_u[np.arange(M), np.arange(M)] = 1.0
    eps_obs = np.zeros((M + No, No))
    eps_obs[M + np.arange(No), np.arange(No)] = 1.0
    return eps_u.reshape(M + No, m1, m2), eps_obs.reshape((M + No,) + tuple(n_obs_nodes))


def outer_sum(samples: np.ndarray, mean: np.ndarray) -> np.ndarray:
    """sum_s (V_s - mean)(V_s - mean)^T, [M, M]."""
    Dv = (samples - mean[None]).reshape(samples.shape[0], -1)
    return Dv.T @ Dv


def rel(a, b) -> float:
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
