"""Regenerates tests/golden/b0_kinds_hp.npz: 50-digit values of the B0 cell-integral factors under the Matern-3/2 and Matern-5/2
kernels (VGGP_BASIS_B0K; tests/b0_kinds_spec.py) at sampled (row, column) indices, for ell / delta from 1/2000 to 3.2e4.

    python tests/golden/make_b0_kinds_hp.py          (needs mpmath; only this generator does -- the tests read the .npz)

Everything comes from the DEFINITION, by quadrature -- no closed form of a cell integral is typed in here:
  A0[k, p] = int_{cell k} kappa(x_p - t) dt, mp.quad on the cell, split at x_p when x_p lies inside and at geometric break points
             measured from the end nearest to x_p (an integrand that decays over thousands of lengthscales is still resolved)
  K0[i, j] = int_{cell i} int_{cell j} kappa(s - t) dt ds.  The integrand depends on d = s - t alone, so the area integral is the
             line integral of kappa(d) against the length of the segment {s - t = d} inside the square, the triangle
             w(d) = delta - |d - k delta| on |d - k delta| <= delta (k = |i - j|; a change of variables, not a property of kappa).
             It is split at the kink d = k delta -- for k = 0 that is the diagonal s = t, where kappa has its own kink -- and at
             geometric break points from the end nearest to d = 0.  main() checks this reduction against the nested mp.quad over
             the square (split on the diagonal) on one mesh per kernel.
  d / d ell  mp.diff of the value function throughout.
Per element the file also stores the summand scale S of the float64 closed form (b0_kinds_spec.S_b0k_A / S_b0k_K, rounded up),
and per case R_oracle = the specification's worst err / (eps S), the constant the tolerances are built from
(|got - hp| <= 4 max(R_oracle, 1) eps S, as tests/factor_hp_cases.py).
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import b0_kinds_spec as B  # noqa: E402
import factor_hp_cases as H  # noqa: E402  (ratio_to_bound: the same err / (eps S) the tests use)

mp.dps = 50
RATIOS = [1.0 / 2000, 1.0 / 700, 1.0 / 100, 1.0, 30.0, 320.0, 3.2e4]
RATIO_TAGS = ["1/2000", "1/700", "1/100", "1", "30", "320", "3.2e4"]
OUTPUTS = ("A0", "dA0", "K0", "dK0")


def profile(kind, u):
    """kappa / e^{-u} at scaled distance u >= 0"""
    return 1 + u if kind == "matern32" else 1 + u + u * u / 3


def cscale(kind, ell):
    return (mp.sqrt(3) if kind == "matern32" else mp.sqrt(5)) / ell


def breaks(length, ell):
    """0 = near end .. length = far end, geometric steps from the near end (in units of length)"""
    pts, step = [mpf(0)], 2 * ell
    while pts[-1] + step < length and len(pts) < 40:
        pts.append(pts[-1] + step)
        step *= 4
    return pts + [length]


def weighted_piece(kind, near, length, ell, weight):
    """int_0^length kappa(near + r) weight(r) dr for near >= 0.  mp.quad stops on an ABSOLUTE error estimate: the integrand is scaled to
    order 1 (e^{-c near} taken out, r and the weight in units of ell) and the factors are put back afterwards."""
    if length <= 0:
        return mpf(0)
    c = cscale(kind, ell)
    f = lambda r: profile(kind, c * (near + r)) * mp.exp(-c * r) * weight(r)  # noqa: E731
    return mp.quad(f, breaks(length, ell)) * mp.exp(-c * near)


def A_val(kind, a, b, x, ell):
    one = lambda r: mpf(1)  # noqa: E731
    if a < x < b:
        return weighted_piece(kind, mpf(0), x - a, ell, one) + weighted_piece(kind, mpf(0), b - x, ell, one)
    near = min(abs(x - a), abs(x - b))
    return weighted_piece(kind, near, b - a, ell, one)


def K_val(kind, kd, delta, ell):
    """the double cell integral as the line integral against the triangle w (module docstring)"""
    rising = lambda r: r  # noqa: E731                       w on [(k-1) delta, k delta], r measured from (k-1) delta
    falling = lambda r: delta - r  # noqa: E731              w on [k delta, (k+1) delta], r measured from k delta
    if kd == 0:
        return 2 * weighted_piece(kind, mpf(0), delta, ell, falling)
    return weighted_piece(kind, (kd - 1) * delta, delta, ell, rising) + weighted_piece(kind, kd * delta, delta, ell, falling)


def K_val_nested(kind, kd, delta, ell):
    """the area integral itself, cells [0, delta] and [kd delta, (kd + 1) delta]; the diagonal cell split on s = t"""
    c = cscale(kind, ell)
    kap = lambda d: profile(kind, c * abs(d)) * mp.exp(-c * abs(d))  # noqa: E731
    if kd == 0:
        return 2 * mp.quad(lambda s: mp.quad(lambda t: kap(s - t), [0, s]), [0, delta])
    return mp.quad(lambda s: mp.quad(lambda t: kap(s - t), [0, delta]), [kd * delta, (kd + 1) * delta])


def coords(lo, hi, knots, ell, extra):
    """columns: both ends, interior knots exactly, generic interior points, points outside on both sides (near, far, and at
    distances where exp underflows to a subnormal and to zero) -- the columns of make_factor_hp.py"""
    span = hi - lo
    xs = [lo, hi] + list(knots) + list(extra) + [lo - 0.3 * span, hi + 0.7 * span, lo - 1e-9 * span, np.nextafter(hi, 9.0),
                                                lo - 720.0 * ell, hi + 735.0 * ell, lo - 800.0 * ell]
    return np.array(xs, dtype=np.float64)


def build_cases():
    cases = []
    mesh = np.linspace(0, 1, 33)
    for kind in ("matern32", "matern52"):
        for ri, ratio in enumerate(RATIOS):
            ell = float(ratio * (mesh[1] - mesh[0]))
            x = coords(0.0, 1.0, [mesh[5], mesh[16], mesh[31]], ell, [0.013, 0.4999, 0.77, float(mesh[5]) + 1.7 * ell, float(mesh[16]) - 0.3 * ell])
            Aidx = []
            for p, xv in enumerate(x):
                cell = int(np.searchsorted(mesh, xv, side="left")) - 1
                rows = {0, 15, 31} | {c for c in (cell - 1, cell, cell + 1) if 0 <= c < 32}
                Aidx += [(k, p) for k in sorted(rows)]
            Kidx = [(0, 0), (0, 1), (1, 0), (5, 7), (7, 5), (3, 17), (31, 0), (0, 31), (30, 31), (31, 31), (12, 9), (16, 16)]
            cases.append(dict(kind=kind, grid=mesh, x=x, ell=ell, ratio=RATIO_TAGS[ri], Aidx=Aidx, Kidx=Kidx))
    return cases


def hp_case(c):
    mp.dps = 50
    kind, ell, g, x = c["kind"], mpf(c["ell"]), c["grid"], c["x"]
    delta = mpf(float(g[1] - g[0]))
    A, K, seen = [], [], {}
    for k, p in c["Aidx"]:
        a, b, xv = mpf(float(g[k])), mpf(float(g[k + 1])), mpf(float(x[p]))
        A.append((A_val(kind, a, b, xv, ell), mp.diff(lambda l: A_val(kind, a, b, xv, l), ell)))
    for k, p in c["Kidx"]:
        kd = abs(k - p)
        if kd not in seen:
            seen[kd] = (K_val(kind, kd, delta, ell), mp.diff(lambda l: K_val(kind, kd, delta, l), ell))
        K.append(seen[kd])
    tof = lambda col, L: np.array([float(e[col]) for e in L], dtype=np.float64)  # noqa: E731
    Aidx, Kidx = np.array(c["Aidx"], np.int64), np.array(c["Kidx"], np.int64)
    SA, SK = B.S_b0k_A(kind, g, x, c["ell"]), B.S_b0k_K(kind, len(g) - 1, float(g[1] - g[0]), c["ell"])
    up = lambda S, idx: np.nextafter(S[idx[:, 0], idx[:, 1]], np.inf)  # noqa: E731
    out = dict(A0=tof(0, A), dA0=tof(1, A), K0=tof(0, K), dK0=tof(1, K),
               S_A0=up(SA[0], Aidx), S_dA0=up(SA[1], Aidx), S_K0=up(SK[0], Kidx), S_dK0=up(SK[1], Kidx))
    gotA, gotK = B.b0k_A(kind, g, x, c["ell"]), B.b0k_K(kind, len(g) - 1, float(g[1] - g[0]), c["ell"])
    got = dict(A0=gotA[0][Aidx[:, 0], Aidx[:, 1]], dA0=gotA[1][Aidx[:, 0], Aidx[:, 1]],
               K0=gotK[0][Kidx[:, 0], Kidx[:, 1]], dK0=gotK[1][Kidx[:, 0], Kidx[:, 1]])
    R = np.array([H.ratio_to_bound(got[k], out[k], out["S_" + k]) for k in OUTPUTS])
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.array([np.max(np.where(np.abs(out[k]) > 1e-290, np.abs(got[k] - out[k]) / np.abs(out[k]), 0.0)) for k in OUTPUTS])
    return out, R, rel


def check_reduction():
    """the line-integral form of K0 against the nested area integral (25 digits are plenty for the comparison and much faster)"""
    mp.dps = 25
    delta, ell = mpf(1) / 32, mpf(1) / 20
    for kind in ("matern32", "matern52"):
        for kd in (0, 1, 2, 5):
            a, b = K_val(kind, kd, delta, ell), K_val_nested(kind, kd, delta, ell)
            assert abs(a - b) <= mpf(10) ** -18 * abs(b), (kind, kd, a, b)
    mp.dps = 50


def main():
    check_reduction()
    cases = build_cases()
    with ProcessPoolExecutor(max_workers=min(len(cases), os.cpu_count() or 1)) as ex:
        results = list(ex.map(hp_case, cases))
    out = {"ncases": np.int64(len(cases))}
    for i, (c, (hp, R, rel)) in enumerate(zip(cases, results)):
        pre = f"c{i:03d}_"
        out[pre + "kind"], out[pre + "ratio"] = np.str_(c["kind"]), np.str_(c["ratio"])
        out[pre + "grid"], out[pre + "x"], out[pre + "ell"] = np.asarray(c["grid"], np.float64), c["x"], np.float64(c["ell"])
        out[pre + "Aidx"], out[pre + "Kidx"] = np.array(c["Aidx"], np.int64), np.array(c["Kidx"], np.int64)
        for k, v in hp.items():
            out[pre + k] = v
        out[pre + "R_outputs"], out[pre + "R_oracle"] = R, np.float64(R.max())
        print(f"{i:3d} {c['kind']:8s} ell/delta {c['ratio']:>6s}  R(A0, dA0, K0, dK0) = " + " ".join(f"{r:8.2f}" for r in R)
              + "   worst relative error " + " ".join(f"{r:8.1e}" for r in rel), flush=True)
    np.savez_compressed(os.path.join(HERE, "b0_kinds_hp.npz"), **out)


if __name__ == "__main__":
    main()
