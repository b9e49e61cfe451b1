"""Specification of the iterative exact GP (TEST HELPER, numpy float64, CPU): what vggp_exact_step_iter, vggp_exact_posterior_iter and
vggp_exact_readout_iter compute.  exact_gp_spec.py is the dense truth it is measured against.

    Sigma = s K0 + v I (no jitter: positive definite for v > 0),  theta = (ell1, ell2, s1, s2, v),  s = s1 s2
    K0[i, j] = p1(a) p2(b) exp(-(g1(a) + g2(b))),  a = |d1| / ell1, b = |d2| / ell2: ONE exp per element, as the engine generates it
    preconditioner   Nystroem on r = min(rank, N) strided landmarks idx_j = ((2 j + 1) N) // (2 r):
                         Lz Lz^T = s K0[idx, idx] (+ psd_safe jitter),  L = s K0[:, idx] Lz^-T,  P = v I + L L^T,
                         L^T L = V diag(lam) V^T (lam_i <= 1e-14 lam_max dropped),  Q = L V lam^-1/2,
                         P^w = v^w (I + Q diag((1 + lam / v)^w - 1) Q^T),  log|P| = N log v + sum log1p(lam / v);  rank 0: P = v I
    block            column 0: y;  columns c >= 1: z_c = P^1/2 z0_c, z0_c the engine's counter-based Rademacher probes keyed on (c, i)
                     (scattered_iter_spec.probes with m2 = 1: vgi_probe_kernel's hash and seed)
    PCG scalars      as vgi_pcg_scalars_kernel keeps them (masked_iter_spec.py): active = r0^2 > 0 at the start, alpha / beta zero for
                     inactive columns and non-positive denominators, a column stops once NOT |r|^2 > tol^2 |r0|^2
    log|Sigma|       log|P| + mean_c N e1^T log(T_c) e1, T_c the Lanczos tridiagonal of the PCG coefficients of column c
    traces           tr(Sigma^-1 D) ~ mean_c u_c^T D w_c,  u_c = Sigma^-1 z_c (the PCG solution),  w_c = P^-1 z_c
    MLL = -1/2 [y^T alpha + log|Sigma| + N log 2 pi],  dMLL/d ell_d = (s / 2) [alpha^T d_d K0 alpha - tr_d],
    dMLL/d s1 = (s2 / 2) [alpha^T K0 alpha - tr_K] (s2 symmetric),  dMLL/d v = 1/2 [alpha^T alpha - tr_I]
    wide=True        every sum over the N points (kernel products, Q^T x, column dots) accumulates in numpy.longdouble

Points: synthetic along-track positions in the unit box (datagen.generate_track on a 600 x 600 field, every point moved inside its
cell by default_rng(seed): no duplicates), y = latent_2d + 0.05 noise.

CASES are shared by tests/test_exact_iter_spec.py (CPU) and tests/test_gpu_exact_iter.py (GPU).  Seeds: for every case the first of
1, 2, .. at which (i) the landmark factor takes no jitter and no eigenvalue of L^T L lies within a factor 10 of the 1e-14 cut, (ii) the
iteration count is a property of the algorithm and not of round-off (count_robust: every column still active in the last iteration ends
it with |r|^2 <= 0.8 of its threshold, and some column entered it with >= 1.25) and is the same under wide=True, (iii)
100 D_case <= 1e-8, (iv) for the 48-probe cases E_case <= 2e-2 (MLL) and <= 0.1 (gradient) -- asserted in test_exact_iter_spec.py.
FLOORS holds per case (D_case, E_mll, E_grad):
    D_case   the specification's own round-off floor: the largest MLL / gradient discrepancy between the specification as written and
             (a) wide=True, (b) tol = 1e-12
    E_case   the estimator's error against exact_gp_spec.mll / analytic_grad: MLL scaled by max(|MLL|, N), gradient by its largest
             component
`python tests/exact_iter_spec.py` measures them again and rewrites the table.

Measured on one MI355X: the engine against this file MLL 3e-16 .. 4e-12, gradient 2e-16 .. 3e-12, equal iteration counts in every case
(tests/test_gpu_exact_iter.py has the per-case print-out).
"""
from __future__ import annotations

import functools
import math
import os
import sys
from dataclasses import dataclass, field

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:          # (for `python tests/exact_iter_spec.py`; under pytest the conftest has done it)
    sys.path.insert(0, _ROOT)

import exact_gp_spec as E  # noqa: E402
from scattered_iter_spec import probes as _probes  # noqa: E402

CAP_MLL, CAP_GRAD = 1e-8, 1e-6
JITTER = (0.0, 1e-8, 1e-7, 1e-6)
EIG_CUT = 1e-14
LD = np.longdouble


# ---- kernel ---------------------------------------------------------------------------------------------------------------------
def _profile(kind: str, r: np.ndarray):
    """k(r) = p exp(-g), dk/d ell = q exp(-g) / ell."""
    if kind == "matern12":
        return np.ones_like(r), r, r
    if kind == "matern32":
        a = 1.7320508075688772 * r
        return 1.0 + a, a * a, a
    if kind == "matern52":
        a = 2.23606797749979 * r
        a3 = a * a * (1.0 / 3.0)
        return 1.0 + a + a3, a3 * (1.0 + a), a
    r2 = r * r
    return np.ones_like(r), r2, 0.5 * r2


def kmat(kinds, Xa, Xb, ell1: float, ell2: float, der: bool = False):
    """K0(Xa, Xb) at unit outputscale (and dK0/d ell1, dK0/d ell2): one exp per element."""
    inv1, inv2 = 1.0 / ell1, 1.0 / ell2
    p1, q1, g1 = _profile(kinds[0], np.abs(Xa[:, None, 0] - Xb[None, :, 0]) * inv1)
    p2, q2, g2 = _profile(kinds[1], np.abs(Xa[:, None, 1] - Xb[None, :, 1]) * inv2)
    Ex = np.exp(-(g1 + g2))
    K = (p1 * p2) * Ex
    if not der:
        return K
    return K, (q1 * inv1) * p2 * Ex, p1 * (q2 * inv2) * Ex


def _mm(A, B, wide: bool):
    if wide:
        return np.matmul(A.astype(LD), B.astype(LD)).astype(np.float64)
    return A @ B


def _dots(A, B, wide: bool):
    if wide:
        return (A.astype(LD) * B.astype(LD)).sum(axis=0).astype(np.float64)
    return (A * B).sum(axis=0)


# ---- preconditioner -------------------------------------------------------------------------------------------------------------
def landmarks(N: int, rank: int) -> np.ndarray:
    r = min(rank, N)
    return (((2 * np.arange(r, dtype=np.int64) + 1) * N) // (2 * r)) if r > 0 else np.zeros(0, dtype=np.int64)


@dataclass
class Precond:
    v: float
    Q: np.ndarray             # [N, r'] orthonormal columns (r' kept eigenvalues)
    lam: np.ndarray           # [r']
    jitter: float = 0.0
    lam_all: np.ndarray = None
    kzz_eig: np.ndarray = None
    N: int = 0

    @property
    def logdet(self) -> float:
        return self.N * math.log(self.v) + float(np.log1p(self.lam / self.v).sum())

    def apply(self, X: np.ndarray, w: float, wide: bool = False) -> np.ndarray:
        """P^w X for a block X [N, nb]."""
        if self.Q.shape[1] == 0:
            return self.v ** w * X
        T = _mm(self.Q.T, X, wide) * ((1.0 + self.lam / self.v) ** w - 1.0)[:, None]
        return self.v ** w * (X + self.Q @ T)


def precond(kinds, X, theta, rank: int) -> Precond:
    ell1, ell2, s1, s2, v = [float(t) for t in theta]
    N, s = X.shape[0], s1 * s2
    idx = landmarks(N, rank)
    if len(idx) == 0:
        return Precond(v, np.zeros((N, 0)), np.zeros(0), 0.0, np.zeros(0), np.zeros(0), N)
    Kzz = s * kmat(kinds, X[idx], X[idx], ell1, ell2)
    Lz, jit = None, -1.0
    for eps in JITTER:
        try:
            Lz = np.linalg.cholesky(Kzz + eps * np.eye(len(idx)))
            jit = eps
            break
        except np.linalg.LinAlgError:
            continue
    if Lz is None:
        raise np.linalg.LinAlgError("landmark factor not positive definite after jitter 1e-6")
    L = s * kmat(kinds, X, X[idx], ell1, ell2) @ np.linalg.inv(Lz).T
    lam, V = np.linalg.eigh(L.T @ L)
    keep = lam > EIG_CUT * lam.max()
    Q = (L @ V[:, keep]) / np.sqrt(lam[keep])[None, :]
    return Precond(v, Q, lam[keep], jit, lam, np.linalg.eigvalsh(Kzz), N)


# ---- block PCG ------------------------------------------------------------------------------------------------------------------
@dataclass
class PcgResult:
    X: np.ndarray
    al_h: np.ndarray
    be_h: np.ndarray
    kcol: np.ndarray
    converged: bool
    ratio: np.ndarray         # ratio[k][c] = |r|^2 / (tol^2 |r0|^2) after k iterations

    @property
    def iters(self) -> int:
        return int(self.kcol.max())

    def count_robust(self, lo: float = 0.8, hi: float = 1.25) -> bool:
        """The iteration count (largest over the columns) does not hinge on round-off in a residual norm."""
        k = self.iters
        if not self.converged or k == 0:
            return bool(self.converged)
        last_cols = self.kcol == k
        return bool((self.ratio[k][last_cols] <= lo).all() and (self.ratio[k - 1][last_cols] >= hi).any())


def pcg(Aop, pc: Precond, RHS: np.ndarray, tol: float, maxit: int, wide: bool = False) -> PcgResult:
    X = np.zeros_like(RHS)
    R = RHS.copy()
    Zp = pc.apply(R, -1.0, wide)
    Pd = Zp.copy()
    rz = _dots(R, Zp, wide)
    r02 = _dots(R, R, wide)
    active = r02 > 0.0
    kcol = np.zeros(RHS.shape[1], int)
    thr = tol * tol * r02
    al_h, be_h = [], []
    ratio = [np.where(r02 > 0, 1.0 / (tol * tol), 0.0)]
    for _ in range(maxit):
        if not active.any():
            break
        AP = Aop(Pd)
        pAp = _dots(Pd, AP, wide)
        al = np.where(active & (pAp > 0), rz / np.where(pAp > 0, pAp, 1.0), 0.0)
        X += al[None, :] * Pd
        R -= al[None, :] * AP
        Zp = pc.apply(R, -1.0, wide)
        rz_new = _dots(R, Zp, wide)
        be = np.where(active & (rz > 0), rz_new / np.where(rz > 0, rz, 1.0), 0.0)
        al_h.append(al)
        be_h.append(be)
        kcol += active
        Pd = Zp + be[None, :] * Pd
        rz = rz_new
        rr = _dots(R, R, wide)
        ratio.append(rr / np.where(thr > 0, thr, 1.0))
        active = active & (rr > thr)
    nb = RHS.shape[1]
    return PcgResult(X, np.array(al_h).reshape(-1, nb), np.array(be_h).reshape(-1, nb), kcol, not active.any(), np.array(ratio))


def slq(al: np.ndarray, be: np.ndarray, k: int) -> float:
    """e1^T log(T) e1 of the Lanczos tridiagonal of k PCG iterations."""
    T = np.zeros((k, k))
    for j in range(k):
        T[j, j] = 1.0 / al[j] + (be[j - 1] / al[j - 1] if j > 0 else 0.0)
        if j + 1 < k:
            T[j, j + 1] = T[j + 1, j] = math.sqrt(be[j]) / al[j]
    w, U = np.linalg.eigh(T)
    return float((U[0] ** 2) @ np.log(w))


# ---- the step -------------------------------------------------------------------------------------------------------------------
@dataclass
class ExactIterState:
    kinds: tuple
    X: np.ndarray
    theta: np.ndarray
    alpha: np.ndarray
    pc: Precond
    res: PcgResult
    logdet: float = 0.0
    yalpha: float = 0.0
    mll: float = 0.0
    grad: np.ndarray = field(default_factory=lambda: np.zeros(5))

    @property
    def iters(self) -> int:
        return self.res.iters


def defaults(n_probes: int = 0, rank: int = -1, tol: float = 0.0, max_iter: int = 0):
    return (16 if n_probes <= 0 else n_probes, 64 if rank < 0 else rank, 1e-10 if tol <= 0 else tol, 1000 if max_iter <= 0 else max_iter)


def probes(N: int, nprobe: int) -> np.ndarray:
    """Z0 [N, nprobe] of +-1, column c - 1 = engine column c."""
    return _probes(N, 1, nprobe)[:, :, 0].T.copy()


def step(kinds, X, y, theta, nprobe: int = 16, rank: int = 64, tol: float = 1e-10, maxit: int = 1000, wide: bool = False) -> ExactIterState:
    ell1, ell2, s1, s2, v = [float(t) for t in theta]
    X, y = np.asarray(X, float), np.asarray(y, float)
    N, s = X.shape[0], s1 * s2
    K, D1, D2 = kmat(kinds, X, X, ell1, ell2, der=True)

    def Aop(V):
        return s * _mm(K, V, wide) + v * V

    pc = precond(kinds, X, theta, rank)
    Z0 = probes(N, nprobe)
    Zs = pc.apply(Z0, 0.5, wide)
    Wz = pc.apply(Zs, -1.0, wide)
    res = pcg(Aop, pc, np.concatenate([y[:, None], Zs], axis=1), tol, maxit, wide)
    ld = sum(N * slq(res.al_h[:, c], res.be_h[:, c], res.kcol[c]) for c in range(1, nprobe + 1))
    logdet = pc.logdet + ld / nprobe
    alpha = res.X[:, 0].copy()
    B = np.concatenate([alpha[:, None], Wz], axis=1)                   # [alpha, w_1 .. w_p]: ONE derivative-mode product
    dK, d1, d2 = (_dots(res.X, _mm(M, B, wide), wide) for M in (K, D1, D2))
    dI = _dots(res.X, B, wide)

    def tr(d):
        return float(d[1:].sum()) / nprobe
    yalpha = float(_dots(y[:, None], alpha[:, None], wide)[0])
    st = ExactIterState(tuple(kinds), X, np.asarray(theta, float), alpha, pc, res, logdet, yalpha)
    st.mll = -0.5 * (yalpha + logdet + N * math.log(2.0 * math.pi))
    gK = dK[0] - tr(dK)
    st.grad = np.array([0.5 * s * (d1[0] - tr(d1)), 0.5 * s * (d2[0] - tr(d2)), 0.5 * s2 * gK, 0.5 * s1 * gK, 0.5 * (dI[0] - tr(dI))])
    return st


# ---- read-outs ------------------------------------------------------------------------------------------------------------------
def _solve_cols(st: ExactIterState, B: np.ndarray, tol: float, maxit: int) -> np.ndarray:
    """Sigma^-1 B in blocks of 64 columns (a column's numbers do not depend on its neighbours or on the block width)."""
    ell1, ell2, s1, s2, v = st.theta
    K = kmat(st.kinds, st.X, st.X, ell1, ell2)
    out = np.empty_like(B)
    for c0 in range(0, B.shape[1], 64):
        r = pcg(lambda V: s1 * s2 * (K @ V) + v * V, st.pc, B[:, c0:c0 + 64], tol, maxit)
        if not r.converged:
            raise RuntimeError("read-out PCG did not converge")
        out[:, c0:c0 + 64] = r.X
    return out


def posterior(st: ExactIterState, xs, tol: float = 1e-10, maxit: int = 1000, variance: bool = True):
    """-> mean [ns], var [ns] (None without variance)."""
    ell1, ell2, s1, s2, v = st.theta
    s = s1 * s2
    Bs = kmat(st.kinds, st.X, np.asarray(xs, float), ell1, ell2)      # [N, ns]
    mean = s * (Bs.T @ st.alpha)
    if not variance:
        return mean, None
    return mean, s - s * s * (Bs * _solve_cols(st, Bs, tol, maxit)).sum(0)


def q_v(st: ExactIterState, C1, C2, kd1, kd2, literal: bool = True, cells=None, tol: float = 1e-10, maxit: int = 1000):
    """-> mean [mv1, mv2] and var: literal [mv1, mv2] (no solve); conditional at the listed cells [n_cells]."""
    ell1, ell2, s1, s2, v = st.theta
    s = s1 * s2
    C1, C2, kd1, kd2 = (np.asarray(t, float) for t in (C1, C2, kd1, kd2))
    mean = s * (C1 * st.alpha[None, :]) @ C2.T
    if literal:
        return mean, s * np.outer(kd1, kd2) + (s * s / v) * ((C1 * C1) @ (C2 * C2).T)
    cells = np.asarray(cells, dtype=np.int64)
    a, b = cells // C2.shape[0], cells % C2.shape[0]
    F = s * (C1[a] * C2[b]).T                                          # [N, n_cells]
    return mean, s * kd1[a] * kd2[b] - (F * _solve_cols(st, F, tol, maxit)).sum(0)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
THETA = np.array([0.3, 0.25, 1.3, 0.8, 0.05])
THETA_SHORT = np.array([0.02, 0.016, 1.3, 0.8, 0.05])                   # the kernel matrix is nearly diagonal: P = v I is adequate
THETA_LONG = np.array([1.0, 0.8, 1.3, 0.8, 0.05])                       # a handful of landmarks capture a very smooth RBF


@functools.lru_cache(maxsize=None)
def track_points(N: int, seed: int):
    """-> X [N, 2] in the unit box along synthetic tracks (in track order), y [N]."""
    from oracle import dense as D
    from variational_gridded_gaussian_processes_amd import datagen
    lon, lat = datagen.generate_track(600, 600, 2, 0.5)
    pts = np.unique(np.stack([lon, lat], 1), axis=0)
    pts = pts[np.lexsort((pts[:, 1], pts[:, 0]))]
    pick = pts[(np.arange(N, dtype=np.int64) * len(pts)) // N]
    rng = np.random.default_rng(seed)
    X = (pick + rng.random((N, 2))) / 600.0
    y = D.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(N)
    return X, y


# name -> (N, (kind1, kind2), rank, probes, seed, theta).  Without a preconditioner that deflates the large eigenvalues of s K0 the
# Lanczos process behind the PCG loses orthogonality as soon as a Ritz value converges, and from then on the late iterates -- and
# with them the iteration count, by one to six out of a hundred -- depend on round-off (measured: wide=True against the specification
# as written at THETA with rank 0 or 8).  Rank 0 and rank 8 therefore run where they are adequate (THETA_SHORT, THETA_LONG); with
# rank 64 at THETA the two variants agree in every column's count.
CASES = {
    "n196_m12_r0_p16": (196, ("matern12", "matern12"), 0, 16, 1, THETA_SHORT),
    "n196_rbf_r8_p1": (196, ("rbf", "rbf"), 8, 1, 1, THETA_LONG),
    "n600_rbf_r8_p16": (600, ("rbf", "rbf"), 8, 16, 1, THETA_LONG),
    "n600_m32_r64_p16": (600, ("matern32", "matern32"), 64, 16, 3, THETA),
    "n600_m12_r64_p48": (600, ("matern12", "matern12"), 64, 48, 2, THETA),
    "n777_m52_r64_p48": (777, ("matern52", "matern52"), 64, 48, 1, THETA),
    "n777_m32xrbf_r64_p16": (777, ("matern32", "rbf"), 64, 16, 1, THETA),
    "n777_m12_r64_p16": (777, ("matern12", "matern12"), 64, 16, 2, THETA),
    "n1500_m52_r64_p16": (1500, ("matern52", "matern52"), 64, 16, 1, THETA),
    "n1500_m12_r0_p1": (1500, ("matern12", "matern12"), 0, 1, 2, THETA_SHORT),
}
DENSE_CASES = [n for n, c in CASES.items() if c[3] == 48]              # compared with the dense step
RANK_N = (200, ("matern12", "matern12"), 200, 4, 1, THETA)             # all points are landmarks: P = Sigma, one iteration


def case_data(name: str):
    N, kinds, rank, nprobe, seed, theta = CASES[name]
    return (kinds,) + track_points(N, seed) + (rank, nprobe, theta)


@functools.lru_cache(maxsize=None)
def case_spec(name: str) -> ExactIterState:
    kinds, X, y, rank, nprobe, theta = case_data(name)
    return step(kinds, X, y, theta, nprobe=nprobe, rank=rank)


@functools.lru_cache(maxsize=None)
def dense_ref(name: str):
    """(mll, grad[5]) of exact_gp_spec on the case's data."""
    import torch
    kinds, X, y, _, _, theta = case_data(name)
    Xt, yt, th = torch.tensor(X), torch.tensor(y), torch.tensor(theta)
    val, eps = E.mll(kinds, Xt, th, yt)
    assert eps == 0.0
    return float(val), E.analytic_grad(kinds, Xt, th, yt).numpy()


def errors(mll, grad, ref_mll, ref_grad, N):
    """MLL error relative to max(|MLL|, N); gradient error relative to its largest component."""
    return abs(mll - ref_mll) / max(abs(ref_mll), N), float(np.abs(np.asarray(grad) - ref_grad).max() / np.abs(ref_grad).max())


def floor_case(name: str):
    """(D_case, the iteration count under wide=True)."""
    kinds, X, y, rank, nprobe, theta = case_data(name)
    st = case_spec(name)
    wide = step(kinds, X, y, theta, nprobe=nprobe, rank=rank, wide=True)
    tight = step(kinds, X, y, theta, nprobe=nprobe, rank=rank, tol=1e-12)
    return max(max(errors(o.mll, o.grad, st.mll, st.grad, len(y))) for o in (wide, tight)), wide.iters


def estimator_error(name: str):
    st = case_spec(name)
    return errors(st.mll, st.grad, *dense_ref(name), st.X.shape[0])


def bounds(d_case: float):
    """(MLL bound, gradient bound) of the GPU comparison."""
    b = max(100.0 * d_case, 1e-12)
    return min(b, CAP_MLL), min(b, CAP_GRAD)


# FLOORS-BEGIN (python tests/exact_iter_spec.py rewrites this block)
FLOORS = {
    'n196_m12_r0_p16': (2.84e-12, 3.33e-03, 3.22e-02),
    'n196_rbf_r8_p1': (9.32e-14, 7.00e-04, 4.43e-03),
    'n600_rbf_r8_p16': (3.47e-12, 6.31e-04, 4.13e-04),
    'n600_m32_r64_p16': (6.61e-13, 1.14e-03, 2.48e-03),
    'n600_m12_r64_p48': (1.27e-12, 4.44e-03, 2.47e-03),
    'n777_m52_r64_p48': (1.42e-12, 4.11e-04, 4.41e-04),
    'n777_m32xrbf_r64_p16': (6.50e-12, 1.20e-03, 4.11e-03),
    'n777_m12_r64_p16': (1.05e-12, 1.21e-02, 1.38e-02),
    'n1500_m52_r64_p16': (6.49e-13, 1.03e-03, 2.37e-03),
    'n1500_m12_r0_p1': (5.21e-12, 1.33e-02, 6.49e-03),
}
# FLOORS-END


def _regenerate():
    lines = ["FLOORS = {"]
    for name in CASES:
        e = estimator_error(name)
        lines.append(f"    {name!r}: ({floor_case(name)[0]:.2e}, {e[0]:.2e}, {e[1]:.2e}),")
    lines.append("}")
    path = os.path.abspath(__file__)
    src = open(path).read()
    head, rest = src.split("# FLOORS-BEGIN", 1)
    first, tail = rest.split("\n", 1)[0], rest.split("# FLOORS-END", 1)[1]
    open(path, "w").write(head + "# FLOORS-BEGIN" + first + "\n" + "\n".join(lines) + "\n# FLOORS-END" + tail)
    print("\n".join(lines))


if __name__ == "__main__":
    _regenerate()
