"""Specification of the B0 cell-integral factors under the Matern-3/2 and Matern-5/2 kernels (VGGP_BASIS_B0K, csrc/factor_elem.h
vg_b0k_edge / vg_b0k_K_consts): numpy float64 closed forms, their summand scales S, and the oracle Factor that carries them.

Definitions (unit outputscale; mesh of m + 1 equispaced knots, cell k = (g_k, g_k+1], x <= g_0 counts as below):

    A0[k, p] = int_{cell k} kappa(x_p - t) dt                K0[i, j] = int_{cell i} int_{cell j} kappa(s - t) dt ds

with kappa(d) = (1 + u) e^{-u}, u = sqrt(3) |d| / ell (nu = 3/2) or (1 + u + u^2 / 3) e^{-u}, u = sqrt(5) |d| / ell (nu = 5/2).
tests/golden/b0_kinds_hp.npz holds 50-digit values of these integrals by quadrature (tests/golden/make_b0_kinds_hp.py); the closed
forms below are what is tested against them.  c = sqrt(3) / ell or sqrt(5) / ell throughout, c ell = kappa0.

A0 through the edge function E(g) = int_{|x - g|}^inf kappa = P(u_g) e^{-u_g} / c, u_g = c |x - g|:
    P(u) = 2 + u (3/2),  (8 + 5 u + u^2) / 3 (5/2)                           int_0^inf kappa = P(0) / c
    x outside the cell:  +-(E(a) - E(b))            x inside:  2 P(0) / c - E(a) - E(b)
    dE / d ell = Q(u) e^{-u} / kappa0,   Q = P + u (P - P') = 2 + 2 u + u^2 (3/2),  (8 + 8 u + 4 u^2 + u^3) / 3 (5/2)
Only differences of decaying edge terms occur: a far cell keeps its relative accuracy (F(b - x) - F(a - x) with the
antiderivative F = +-(P(0) - P e^{-u}) / c does not: 3e-7 at 18 lengthscales).

K0 is Toeplitz in k = |i - j|: G((k+1) delta) - 2 G(k delta) + G((k-1) delta), G'' = kappa, G even:
    c^2 G = 2 u + g(u) - 3,  g = (3 + u) e^{-u} (3/2);       3 c^2 G = 8 u + g(u) - 15,  g = (15 + 7 u + u^2) e^{-u} (5/2)
The linear term cancels for k >= 1.  With t = c delta, x = e^{-t}, em1 = expm1(-t), q = em1^2, e2 = expm1(-2 t), s2 = x^2 + 1
and E = e^{-(k-1) t}, the second difference of g is E times a polynomial in k whose coefficients are constants of the mesh:
    3/2:  F_k = E (a0 + k a1),             a0 = 3 q + t e2,                 a1 = t q
    5/2:  F_k = E (a0 + k a1 + k^2 a2),    a0 = 15 q + 7 t e2 + t^2 s2,     a1 = 7 t q + 2 t^2 e2,     a2 = t^2 q
    K0_k = C F_k,  C = 1 / c^2 (3/2), 1 / (3 c^2) (5/2);  no factor grows with t: finite for every t > 0
    k = 0:  F_0 = 2 c^2 G(delta) (x 3 for 5/2) = 2 ((3 + t) em1 + 3 t)  (3/2),   2 ((15 + 7 t + t^2) em1 + 15 t + t^2)  (5/2)
d / d ell (dt / d ell = -t / ell, dC / d ell = 2 C / ell):  dK0_k = 2 K0_k / ell - (t / ell) C dF_k / dt,
    dF_k / dt = E (d0 + k d1 + k^2 d2 [+ k^3 d3]),   d_i = a_i + b_i - a_{i-1},   b_i = d a_i / dt   (a_{-1} = 0, a_n = b_n = 0 past the last)
    3/2:  b0 = -6 x em1 + e2 - 2 t x^2,                                  b1 = q - 2 t x em1
    5/2:  b0 = -30 x em1 + 7 e2 - 14 t x^2 + 2 t s2 - 2 t^2 x^2,         b1 = 7 q - 14 t x em1 + 4 t e2 - 4 t^2 x^2,     b2 = 2 t q - 2 t^2 x em1
    k = 0:  dF_0 / dt = -2 ((2 + t) em1 + t)  (3/2),   -2 ((8 + 5 t + t^2) em1 + 5 t + t^2)  (5/2)

S_* return, in the style of factor_hp_cases.S_b0_A / S_b0_K, the sum of the absolute values of the summands of these forms as written,
every transcendental weighted by 1 + its condition number (exp(-u): 1 + u; expm1(-t): 1 + t e^{-t} / |expm1(-t)|), a product carrying
the product of its factors' weights, and every exponential's value floored at the smallest normal double.
"""
import contextlib
import functools
import math
import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np

from oracle import kron as Kr

KAPPA0 = {"matern32": Kr.SQ3, "matern52": Kr.SQ5}
TINY = np.finfo(np.float64).tiny


def _fl(e):
    return np.maximum(e, TINY)


def _P(kind, u):
    return 2.0 + u if kind == "matern32" else (8.0 + u * (5.0 + u)) / 3.0


def _Q(kind, u):
    return 2.0 + u * (2.0 + u) if kind == "matern32" else (8.0 + u * (8.0 + u * (4.0 + u))) / 3.0


# ---- A0 ----------------------------------------------------------------------------------------------------------------------
def b0k_A(kind, mesh, x, ell):
    """-> A0, dA0 / d ell  (m x len(x)); Matern-1/2 is oracle.kron.b0_A itself"""
    mesh, x = np.asarray(mesh, np.float64), np.asarray(x, np.float64)
    if kind == "matern12":
        return Kr.b0_A(mesh, x, ell)
    k0 = KAPPA0[kind]
    c = k0 / ell
    a, b, xx = mesh[:-1, None], mesh[1:, None], x[None, :]
    ua, ub = c * np.abs(xx - a), c * np.abs(xx - b)
    with np.errstate(under="ignore"):
        ea, eb = np.exp(-ua), np.exp(-ub)
        Ea, Eb = _P(kind, ua) * ea / c, _P(kind, ub) * eb / c
        dEa, dEb = _Q(kind, ua) * ea / k0, _Q(kind, ub) * eb / k0
    P0 = _P(kind, 0.0)
    inside = (xx > a) & (xx <= b)
    sign = np.where(xx <= a, 1.0, -1.0)
    A = np.where(inside, 2.0 * P0 / c - (Ea + Eb), sign * (Ea - Eb))
    dA = np.where(inside, 2.0 * P0 / k0 - (dEa + dEb), sign * (dEa - dEb))
    return A, dA


def S_b0k_A(kind, mesh, x, ell):
    mesh, x = np.asarray(mesh, np.float64), np.asarray(x, np.float64)
    if kind == "matern12":
        import factor_hp_cases as H
        return H.S_b0_A(mesh, x, ell)
    k0 = KAPPA0[kind]
    c = k0 / ell
    a, b, xx = mesh[:-1, None], mesh[1:, None], x[None, :]
    ua, ub = c * np.abs(xx - a), c * np.abs(xx - b)
    with np.errstate(under="ignore"):
        ea, eb = _fl(np.exp(-ua)) * (1 + ua), _fl(np.exp(-ub)) * (1 + ub)
    P0 = _P(kind, 0.0)
    inside = (xx > a) & (xx <= b)
    S = _P(kind, ua) * ea / c + _P(kind, ub) * eb / c + np.where(inside, 2.0 * P0 / c, 0.0)
    dS = _Q(kind, ua) * ea / k0 + _Q(kind, ub) * eb / k0 + np.where(inside, 2.0 * P0 / k0, 0.0)
    return S, dS


# ---- K0 ----------------------------------------------------------------------------------------------------------------------
def b0k_consts(kind, delta, ell):
    """the constants of a mesh: C, t, the coefficients a_i of F_k / E and d_i of (dF_k / dt) / E, F_0 and dF_0 / dt -- and the summand
    scale of each (second tuple)"""
    k0 = KAPPA0[kind]
    c = k0 / ell
    t = c * delta
    with np.errstate(under="ignore"):
        x, em1, e2 = math.exp(-t), math.expm1(-t), math.expm1(-2.0 * t)
    q, x2 = em1 * em1, x * x
    s2 = x2 + 1.0
    # scales: |value| (1 + condition number) of each transcendental; products multiply
    Sx = max(x, TINY) * (1 + t)
    Sem = abs(em1) * (1 + t * x / abs(em1))
    Se2 = abs(e2) * (1 + 2 * t * x2 / abs(e2))
    Sq, Sx2 = Sem * Sem, Sx * Sx
    Ss2 = Sx2 + 1.0
    if kind == "matern32":
        C = 1.0 / (c * c)
        a = [3.0 * q + t * e2, t * q]
        b = [-6.0 * x * em1 + e2 - 2.0 * t * x2, q - 2.0 * t * x * em1]
        Sa = [3.0 * Sq + t * Se2, t * Sq]
        Sb = [6.0 * Sx * Sem + Se2 + 2.0 * t * Sx2, Sq + 2.0 * t * Sx * Sem]
        F0, dF0 = 2.0 * ((3.0 + t) * em1 + 3.0 * t), -2.0 * ((2.0 + t) * em1 + t)
        SF0, SdF0 = 2.0 * ((3.0 + t) * Sem + 3.0 * t), 2.0 * ((2.0 + t) * Sem + t)
    else:
        C = 1.0 / (3.0 * c * c)
        t2 = t * t
        a = [15.0 * q + 7.0 * t * e2 + t2 * s2, 7.0 * t * q + 2.0 * t2 * e2, t2 * q]
        b = [-30.0 * x * em1 + 7.0 * e2 - 14.0 * t * x2 + 2.0 * t * s2 - 2.0 * t2 * x2,
             7.0 * q - 14.0 * t * x * em1 + 4.0 * t * e2 - 4.0 * t2 * x2, 2.0 * t * q - 2.0 * t2 * x * em1]
        Sa = [15.0 * Sq + 7.0 * t * Se2 + t2 * Ss2, 7.0 * t * Sq + 2.0 * t2 * Se2, t2 * Sq]
        Sb = [30.0 * Sx * Sem + 7.0 * Se2 + 14.0 * t * Sx2 + 2.0 * t * Ss2 + 2.0 * t2 * Sx2,
              7.0 * Sq + 14.0 * t * Sx * Sem + 4.0 * t * Se2 + 4.0 * t2 * Sx2, 2.0 * t * Sq + 2.0 * t2 * Sx * Sem]
        F0, dF0 = 2.0 * ((15.0 + 7.0 * t + t2) * em1 + 15.0 * t + t2), -2.0 * ((8.0 + 5.0 * t + t2) * em1 + 5.0 * t + t2)
        SF0, SdF0 = 2.0 * ((15.0 + 7.0 * t + t2) * Sem + 15.0 * t + t2), 2.0 * ((8.0 + 5.0 * t + t2) * Sem + 5.0 * t + t2)
    n = len(a)
    d = [(a[i] + b[i]) - (a[i - 1] if i else 0.0) for i in range(n)] + [-a[n - 1]]
    Sd = [Sa[i] + Sb[i] + (Sa[i - 1] if i else 0.0) for i in range(n)] + [Sa[n - 1]]
    return (C, t, a, d, F0, dF0), (Sa, Sd, SF0, SdF0)


def _horner(coef, k):
    """coef[0] + k (coef[1] + k (coef[2] + ...)): the order in which the kernel evaluates the polynomial in k"""
    out = np.full_like(k, coef[-1])
    for cf in coef[-2::-1]:
        out = cf + k * out
    return out


def _toeplitz(r, dr):
    m = len(r)
    idx = np.abs(np.arange(m)[:, None] - np.arange(m)[None, :])
    return r[idx], dr[idx]


def b0k_K(kind, m, delta, ell):
    """-> K0, dK0 / d ell  (m x m); Matern-1/2 is oracle.kron.b0_K itself"""
    if kind == "matern12":
        return Kr.b0_K(m, delta, ell)
    (C, t, a, d, F0, dF0), _ = b0k_consts(kind, delta, ell)
    k = np.arange(m, dtype=np.float64)
    with np.errstate(under="ignore"):
        E = np.exp(-np.maximum(k - 1.0, 0.0) * t)
        F, dF = E * _horner(a, k), E * _horner(d, k)
    F[0], dF[0] = F0, dF0
    v = C * F
    dv = 2.0 * v / ell - (t / ell) * (C * dF)
    return _toeplitz(v, dv)


def S_b0k_K(kind, m, delta, ell):
    if kind == "matern12":
        import factor_hp_cases as H
        return H.S_b0_K(m, delta, ell)
    (C, t, _, _, _, _), (Sa, Sd, SF0, SdF0) = b0k_consts(kind, delta, ell)
    k = np.arange(m, dtype=np.float64)
    km = np.maximum(k - 1.0, 0.0)
    with np.errstate(under="ignore"):
        SE = _fl(np.exp(-km * t)) * (1 + km * t)
    SF, SdF = SE * _horner(Sa, k), SE * _horner(Sd, k)
    SF[0], SdF[0] = SF0, SdF0
    Sv = C * SF
    Sdv = 2.0 * Sv / ell + (t / ell) * (C * SdF)
    return _toeplitz(Sv, Sdv)


# ---- the oracle's factor -----------------------------------------------------------------------------------------------------
@dataclass
class B0KFactor(Kr.Factor):
    """oracle.kron.Factor of a B0K dimension: basis "b0" (so .m and .inverse are those of the cell basis), build() from this file.
    B0KFactor("b0", kind, mesh, x)"""

    def build(self, ell: float, x: Optional[np.ndarray] = None):
        if self.basis != "b0":
            return super().build(ell, x)
        x = self.x if x is None else x
        g = np.asarray(self.grid, dtype=np.float64)
        K, dK = b0k_K(self.kind, len(g) - 1, float(g[1] - g[0]), ell)
        A, dA = b0k_A(self.kind, g, np.asarray(x, dtype=np.float64), ell)
        return K, dK, A, dA


def factor(kind, mesh, x):
    return B0KFactor("b0", kind, np.asarray(mesh, np.float64), np.asarray(x, np.float64))


@contextlib.contextmanager
def _oracle_rebuilds_b0k_factors():
    old, Kr.Factor = Kr.Factor, B0KFactor
    try:
        yield
    finally:
        Kr.Factor = old


def elbo_step_scattered(X, y, f1, f2, theta):
    """oracle.kron.elbo_step_scattered with B0KFactor dimensions.  That function does not call f.build: it re-creates its factors at the
    points as oracle.kron.Factor(f.basis, f.kind, f.grid, X[:, d]), which drops the subclass (and with it the kernel: Factor's "b0"
    is Matern-1/2 whatever the kind).  The oracle is not edited, so the call runs with that name bound to B0KFactor, whose build() is
    Factor's own for every basis but "b0" and for Matern-1/2."""
    with _oracle_rebuilds_b0k_factors():
        return Kr.elbo_step_scattered(X, y, f1, f2, theta)


# ---- reader of tests/golden/b0_kinds_hp.npz ------------------------------------------------------------------------------------
EPS = 2.0 ** -52
OUTPUTS = ("A0", "dA0", "K0", "dK0")
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "b0_kinds_hp.npz")


@functools.lru_cache(maxsize=None)
def cases():
    z = np.load(PATH)
    out = []
    for i in range(int(z["ncases"])):
        pre = f"c{i:03d}_"
        c = SimpleNamespace(index=i, kind=str(z[pre + "kind"]), ratio=str(z[pre + "ratio"]), grid=z[pre + "grid"], x=z[pre + "x"],
                            ell=float(z[pre + "ell"]), Aidx=z[pre + "Aidx"], Kidx=z[pre + "Kidx"], R_oracle=float(z[pre + "R_oracle"]),
                            R_outputs=z[pre + "R_outputs"], hp={k: z[pre + k] for k in OUTPUTS}, S={k: z[pre + "S_" + k] for k in OUTPUTS})
        c.id = f"b0k-{c.kind}-{c.ratio.replace('/', 'over')}"
        out.append(c)
    return out


def case_ids():
    return [c.id for c in cases()]


def spec_outputs(kind, mesh, x, ell):
    """-> A0, dA0, K0, dK0 of this specification"""
    A, dA = b0k_A(kind, mesh, x, ell)
    K, dK = b0k_K(kind, len(mesh) - 1, float(mesh[1] - mesh[0]), ell)
    return A, dA, K, dK


def spec_scales(kind, mesh, x, ell):
    SA, SK = S_b0k_A(kind, mesh, x, ell), S_b0k_K(kind, len(mesh) - 1, float(mesh[1] - mesh[0]), ell)
    return SA[0], SA[1], SK[0], SK[1]


def sample(c, mats):
    A, dA, K, dK = mats
    return {"A0": A[c.Aidx[:, 0], c.Aidx[:, 1]], "dA0": dA[c.Aidx[:, 0], c.Aidx[:, 1]],
            "K0": K[c.Kidx[:, 0], c.Kidx[:, 1]], "dK0": dK[c.Kidx[:, 0], c.Kidx[:, 1]]}


def ratio_to_bound(got, hp, S):
    """worst |got - hp| / (eps S) over the elements (factor_hp_cases.ratio_to_bound)"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - hp)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / (EPS * S))
    return float(np.max(q)) if np.isfinite(got).all() else float("nan")


def tolerance_constant(c):
    """|got - hp| <= c eps S with c = 4 max(R_oracle, 1): the rule of tests/factor_hp_cases.py"""
    return 4.0 * max(c.R_oracle, 1.0)


def family_constant(kind):
    """whole matrices of the kernel against this float64 specification (both sides round): 8 max(R, 1), R the worst R_oracle of the
    kernel family over the fixture"""
    return 8.0 * max(max(c.R_oracle for c in cases() if c.kind == kind), 1.0)
