"""Reader of tests/golden/factor_hp.npz (50-digit factor elements, written by tests/golden/make_factor_hp.py) and the tolerance
rule shared by tests/test_factor_hp.py (numpy oracle, CPU) and tests/test_gpu_factor_paths.py (HIP kernel).

    |got - hp| <= c eps S,   c = 4 max(R_oracle, 1)

S (stored per element) is the sum of the absolute values of the summands of the float64 closed form, every transcendental counted
with 1 + its condition number and every exponential's value floored at the smallest normal double; R_oracle (stored per case) is
the numpy oracle's worst err / (eps S) on that case, measured when the fixture was generated; the factor 4 allows the device's
exp / expm1 / cos a couple of ulp more than libm.  An element with S = 0 (a structural zero) must be exact."""
import functools
import os
from types import SimpleNamespace

import numpy as np

from oracle import kron as Kr

EPS = 2.0 ** -52
OUTPUTS = ("A0", "dA0", "K0", "dK0")
FLAG_B0_F32_KDELTA = 1
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factor_hp.npz")


@functools.lru_cache(maxsize=None)
def cases():
    z = np.load(PATH)
    out = []
    for i in range(int(z["ncases"])):
        pre = f"c{i:03d}_"
        c = SimpleNamespace(index=i, kind=str(z[pre + "kind"]), basis=str(z[pre + "basis"]), ratio=str(z[pre + "ratio"]),
                            grid=z[pre + "grid"], x=z[pre + "x"], ell=float(z[pre + "ell"]), flags=int(z[pre + "flags"]),
                            Aidx=z[pre + "Aidx"], Kidx=z[pre + "Kidx"], R_oracle=float(z[pre + "R_oracle"]),
                            R_outputs=z[pre + "R_outputs"], hp={k: z[pre + k] for k in OUTPUTS}, S={k: z[pre + "S_" + k] for k in OUTPUTS})
        c.id = f"{c.basis}{'_f32' if c.flags & FLAG_B0_F32_KDELTA else ''}-{c.kind}-{c.ratio.replace('/', 'over')}"
        out.append(c)
    return out


def case_ids():
    return [c.id for c in cases()]


def oracle_outputs(kind, basis, grid, x, ell, flags=0):
    """-> A0, dA0, K0, dK0 of the numpy oracle"""
    f = Kr.Factor(basis, kind, np.asarray(grid, np.float64), np.asarray(x, np.float64), bool(flags & FLAG_B0_F32_KDELTA))
    K, dK, A, dA = f.build(float(ell))
    return A, dA, K, dK


def sample(c, mats):
    """the four matrices (A0, dA0, K0, dK0) at the fixture's sampled indices"""
    A, dA, K, dK = mats
    return {"A0": A[c.Aidx[:, 0], c.Aidx[:, 1]], "dA0": dA[c.Aidx[:, 0], c.Aidx[:, 1]],
            "K0": K[c.Kidx[:, 0], c.Kidx[:, 1]], "dK0": dK[c.Kidx[:, 0], c.Kidx[:, 1]]}


def ratio_to_bound(got, hp, S):
    """worst |got - hp| / (eps S) over the elements (0 where got == hp, inf where S == 0 and got != hp, nan for a NaN)"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - hp)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / (EPS * S))
    return float(np.max(q)) if np.isfinite(got).all() else float("nan")


def tolerance_constant(c):
    return 4.0 * max(c.R_oracle, 1.0)


def family_constant(basis, kind, flags=0):
    """c for a whole-matrix comparison of the kernel with the float64 ORACLE (both sides carry rounding, so the constant is
    doubled): 8 max(R, 1), R the worst R_oracle over the fixture's cases of that basis / kernel family"""
    R = max(c.R_oracle for c in cases() if (c.basis, c.kind, c.flags) == (basis, kind, flags))
    return 8.0 * max(R, 1.0)


# ---- the same summand scales S in float64 numpy, for whole matrices (checked against the stored 50-digit S by test_factor_hp.py) ----
TINY = np.finfo(np.float64).tiny


def _fl(e):
    return np.maximum(e, TINY)


def S_points(kind, z, x, ell):
    """-> S of kappa, S of d kappa / d ell for the pairwise profiles (oracle.kron.kappa_and_dell, vg_kappa)"""
    r = np.abs(np.asarray(z)[:, None] - np.asarray(x)[None, :]) / ell
    with np.errstate(under="ignore"):
        if kind == "matern12":
            e, f = _fl(np.exp(-r)), 1 + r
            return e * f, e * r / ell * f
        if kind == "matern32":
            a = Kr.SQ3 * r
            e, f = _fl(np.exp(-a)), 1 + a
            return f * e * f, a * a * e / ell * f
        if kind == "matern52":
            a = Kr.SQ5 * r
            e, f = _fl(np.exp(-a)), 1 + a
            return (1 + a + a * a / 3) * e * f, (a * a / 3) * (1 + a) * e / ell * f
        arg = 0.5 * r * r
        e, f = _fl(np.exp(-arg)), 1 + arg
        return e * f, e * r * r / ell * f


def S_b0_A(mesh, x, ell):
    a, b, xx = mesh[:-1, None], mesh[1:, None], np.asarray(x)[None, :]
    ua, ub = np.abs(xx - a), np.abs(xx - b)
    with np.errstate(under="ignore"):
        ea, eb = _fl(np.exp(-ua / ell)), _fl(np.exp(-ub / ell))
    fa, fb = 1 + ua / ell, 1 + ub / ell
    inside = (xx > a) & (xx <= b)
    return ell * ea * fa + ell * eb * fb + np.where(inside, 2 * ell, 0.0), ea * fa * fa + eb * fb * fb + np.where(inside, 2.0, 0.0)


def S_b0_K(m, delta, ell):
    t = delta / ell
    k = np.arange(m, dtype=np.float64)
    with np.errstate(under="ignore"):
        em1, em2 = abs(np.expm1(-t)), abs(np.expm1(-2 * t))
        c1, c2 = 1 + t * np.exp(-t) / em1, 1 + 2 * t * np.exp(-2 * t) / em2
        E = _fl(np.exp(-np.maximum(k - 1, 0) * t)) * (1 + np.maximum(k - 1, 0) * t)
    q = em1 * em1 * c1 * c1
    sr, sdr = E * q, (t / ell) * E * (k * q + em2 * c2)
    sr[0], sdr[0] = 2 * (em1 * c1 + t), (2 * t / ell) * em1 * c1
    idx = np.abs(np.arange(m)[:, None] - np.arange(m)[None, :])
    sr, sdr = sr[idx], sdr[idx]
    return ell * ell * sr, 2 * ell * sr + ell * ell * sdr
