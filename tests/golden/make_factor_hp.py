"""Regenerates tests/golden/factor_hp.npz: 50-digit values of the per-dimension factor elements A0, dA0/d ell, K0, dK0/d ell
(vggp_factor_build, oracle/kron.py) at sampled (row, column) indices, for every basis and a range of lengthscales.

    python tests/golden/make_factor_hp.py          (needs mpmath; only this generator does -- the tests read the .npz)

Reference values come from the DEFINITION where there is one, never from the float64 formulas under test:
  points   kappa(|z_k - x_p| / ell) of the Matern-1/2, -3/2, -5/2 and RBF profiles
  b0       A0[k, p] = int_{cell k} exp(-|x_p - t| / ell) dt by mp.quad (split at x_p and at geometric break points measured
           from the end of the piece nearest to x_p, so that an integrand that decays over thousands of lengthscales is
           still resolved); K0 = ell^2 (e^{-(k-1)t} + e^{-(k+1)t} - 2 e^{-kt}), t = delta/ell (the double cell integral in
           closed form), 2 ell^2 (e^{-t} + t - 1) on the diagonal
  b0 with VGGP_FLAG_B0_F32_KDELTA: the same three-exponential form with the products (k-1) delta, k delta, (k+1) delta and
           delta rounded to float32 -- that rounding IS the definition of the flag
  vff      cos / sin features inside [a, b), exp(-dist/ell) tails outside; Kuu = diag(alpha) + beta beta^T
  b1       hat functions of the uniform mesh (spacing d = g_1 - g_0, as the builders define it); Kuu = (A ell + B/ell + BC)/2
d/d ell is mp.diff of the value function throughout (no derivative formula is typed in here).

Per element the file also stores the summand scale S of the float64 closed form AS THE KERNEL WRITES IT: the sum of the
absolute values of its summands, every transcendental counted with the factor (1 + its condition number) -- for exp(-u) that is
(1 + |u|); for expm1(-t) it is (1 + t e^{-t} / |expm1(-t)|) <= 2; for cos z, sin z the absolute form |cos z| + |z sin z| -- and
every exponential's VALUE floored at the smallest normal double (below it exp() has the absolute error of one subnormal
quantum = eps * DBL_MIN, not a relative one).  A correct float64 evaluation errs by a small multiple of eps * S; that multiple,
measured for the numpy oracle on each case (R_oracle = worst err / (eps S)), is written into the file too and is the constant
the GPU tolerance is built from (tests/test_gpu_factor_paths.py: c = 4 max(R_oracle, 1)).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import factor_hp_cases as H  # noqa: E402  (the reader the tests use: same oracle call, same err / (eps S))

mp.dps = 60
DBL_MIN = mpf(2) ** -1022
RATIOS = [1.0 / 2000, 1.0 / 700, 1.0 / 100, 1.0, 30.0, 320.0, 3.2e4]
RATIO_TAGS = ["1/2000", "1/700", "1/100", "1", "30", "320", "3.2e4"]
FLAG_B0_F32_KDELTA = 1


def fl(e):
    """value of an exponential as it enters S: floored at the smallest normal double"""
    return max(abs(e), DBL_MIN)


def dd(f, ell):
    return mp.diff(f, ell)


# ---------------------------------------------------------------------------------------------------------------------------
# pairwise profiles
def kappa(kind, dist, ell):
    r = dist / ell
    if kind == "matern12":
        return mp.exp(-r)
    if kind == "matern32":
        a = mp.sqrt(3) * r
        return (1 + a) * mp.exp(-a)
    if kind == "matern52":
        a = mp.sqrt(5) * r
        return (1 + a + a * a / 3) * mp.exp(-a)
    return mp.exp(-r * r / 2)


def kappa_S(kind, dist, ell):
    """(S_v, S_dv) of oracle.kron.kappa_and_dell / vg_kappa"""
    r = dist / ell
    if kind == "matern12":
        e, arg = fl(mp.exp(-r)), r
        return e * (1 + arg), e * r / ell * (1 + arg)
    if kind == "matern32":
        a = mp.sqrt(3) * r
        e = fl(mp.exp(-a))
        return (1 + a) * e * (1 + a), a * a * e / ell * (1 + a)
    if kind == "matern52":
        a = mp.sqrt(5) * r
        e = fl(mp.exp(-a))
        return (1 + a + a * a / 3) * e * (1 + a), (a * a / 3) * (1 + a) * e / ell * (1 + a)
    arg = r * r / 2
    e = fl(mp.exp(-arg))
    return e * (1 + arg), e * r * r / ell * (1 + arg)


def points_elem(kind, g, x, ell):
    dist = abs(mpf(g) - mpf(x))
    v = kappa(kind, dist, ell)
    dv = mpf(0) if dist == 0 else dd(lambda l: kappa(kind, dist, l), ell)
    sv, sdv = kappa_S(kind, dist, ell)
    return v, dv, sv, (mpf(0) if dist == 0 else sdv)


# ---------------------------------------------------------------------------------------------------------------------------
# B0 cell integrals
def _piece(lo, hi, x, ell):
    """int_lo^hi exp(-|x - t| / ell) dt for a piece on one side of x"""
    if hi <= lo:
        return mpf(0)
    near, far = (lo, hi) if abs(lo - x) <= abs(hi - x) else (hi, lo)
    sgn = 1 if far > near else -1
    pts, step = [near], 2 * ell
    while abs(pts[-1] + sgn * step - near) < abs(far - near) and len(pts) < 40:
        pts.append(near + sgn * step)
        step *= 4
    pts.append(far)
    # mp.quad stops on an ABSOLUTE error estimate: integrate the integrand scaled to 1 at the near end in units of ell, and
    # put the factor ell exp(-d0/ell) back afterwards
    d0 = abs(x - near)
    val = mp.quad(lambda t: mp.exp(-(abs(x - t) - d0) / ell) / ell, pts)
    return abs(val) * ell * mp.exp(-d0 / ell)


def b0_A_val(a, b, x, ell):
    if a < x < b:
        return _piece(a, x, x, ell) + _piece(x, b, x, ell)
    return _piece(a, b, x, ell)


def b0_A_closed(a, b, x, ell):
    """the closed form in 50 digits: only used to CHECK the quadrature"""
    ua, ub = abs(x - a), abs(x - b)
    E1, E2 = ell * mp.exp(-ua / ell), ell * mp.exp(-ub / ell)
    if a < x <= b:
        return 2 * ell - (E1 + E2)
    return abs(E1 - E2)


def b0_A_elem(a, b, x, ell):
    a, b, x = mpf(a), mpf(b), mpf(x)
    v = b0_A_val(a, b, x, ell)
    dv = dd(lambda l: b0_A_val(a, b, x, l), ell)
    chk = b0_A_closed(a, b, x, ell)
    assert abs(v - chk) <= mpf(10) ** -45 * max(abs(chk), mpf(10) ** -400), (a, b, x, ell, v, chk)
    dchk = dd(lambda l: b0_A_closed(a, b, x, l), ell)
    assert abs(dv - dchk) <= mpf(10) ** -30 * max(abs(dchk), mpf(10) ** -400), (a, b, x, ell, dv, dchk)
    ua, ub = abs(x - a), abs(x - b)
    ea, eb = fl(mp.exp(-ua / ell)), fl(mp.exp(-ub / ell))
    fa, fb = 1 + ua / ell, 1 + ub / ell
    sv = ell * ea * fa + ell * eb * fb
    sdv = ea * fa * fa + eb * fb * fb
    if a < x <= b:
        sv, sdv = sv + 2 * ell, sdv + 2
    return v, dv, sv, sdv


def b0_K_val(kd, delta, ell):
    t = delta / ell
    if kd == 0:
        return 2 * ell * ell * (mp.exp(-t) + t - 1)
    return ell * ell * (mp.exp(-(kd - 1) * t) + mp.exp(-(kd + 1) * t) - 2 * mp.exp(-kd * t))


def b0_K_elem(kd, delta, ell):
    delta = mpf(delta)
    v, dv = b0_K_val(kd, delta, ell), dd(lambda l: b0_K_val(kd, delta, l), ell)
    t = delta / ell
    em1, em2 = abs(mp.expm1(-t)), abs(mp.expm1(-2 * t))
    c1, c2 = 1 + t * mp.exp(-t) / em1, 1 + 2 * t * mp.exp(-2 * t) / em2
    l2 = ell * ell
    if kd == 0:
        sr = 2 * (em1 * c1 + t)
        sdr = (2 * t / ell) * em1 * c1
    else:
        E = fl(mp.exp(-(kd - 1) * t)) * (1 + (kd - 1) * t)
        q = em1 * em1 * c1 * c1
        sr = E * q
        sdr = (t / ell) * E * (kd * q + em2 * c2)
    return v, dv, l2 * sr, 2 * ell * sr + l2 * sdr


def f32(v):
    return mpf(float(np.float32(v)))


def b0_K_f32_val(kd, df, ell):
    if kd == 0:
        t = df / ell
        return 2 * ell * ell * (mp.exp(-t) + t - 1)
    a0, a1, a2 = f32(np.float32(kd - 1) * np.float32(df)), f32(np.float32(kd + 1) * np.float32(df)), f32(np.float32(kd) * np.float32(df))
    return ell * ell * (mp.exp(-a0 / ell) + mp.exp(-a1 / ell) - 2 * mp.exp(-a2 / ell))


def b0_K_f32_elem(kd, delta, ell):
    df = f32(delta)
    v, dv = b0_K_f32_val(kd, df, ell), dd(lambda l: b0_K_f32_val(kd, df, l), ell)
    l2 = ell * ell
    if kd == 0:
        t = df / ell
        e = fl(mp.exp(-t)) * (1 + t)
        sr = 2 * (e + t + 1)
        sdr = 2 * (e * t / ell + t / ell)
    else:
        aa = [f32(np.float32(c) * np.float32(df)) for c in (kd - 1, kd + 1, kd)]
        ee = [fl(mp.exp(-a / ell)) * (1 + a / ell) for a in aa]
        sr = ee[0] + ee[1] + 2 * ee[2]
        sdr = (ee[0] * aa[0] + ee[1] * aa[1] + 2 * ee[2] * aa[2]) / l2
    return v, dv, l2 * sr, 2 * ell * sr + l2 * sdr


# ---------------------------------------------------------------------------------------------------------------------------
# VFF and B1
def vff_A_elem(grid, k, x, ell):
    a, b, x = mpf(grid[0]), mpf(grid[1]), mpf(x)
    M = (len(grid) - 3)
    w = mpf(grid[2 + (k if k <= M else k - M)])
    if a <= x < b:
        z = w * (x - a)
        if k <= M:
            return mp.cos(z), mpf(0), abs(mp.cos(z)) + abs(z * mp.sin(z)), mpf(0)
        return mp.sin(z), mpf(0), abs(mp.sin(z)) + abs(z * mp.cos(z)), mpf(0)
    if k > M:
        return mpf(0), mpf(0), mpf(0), mpf(0)
    r = min(abs(x - a), abs(x - b))
    v, dv = mp.exp(-r / ell), dd(lambda l: mp.exp(-r / l), ell)
    e = fl(v) * (1 + r / ell)
    return v, dv, e, r / (ell * ell) * e


def vff_K_elem(grid, k, p, ell):
    a, b = mpf(grid[0]), mpf(grid[1])
    M = (len(grid) - 3)
    w = mpf(grid[2 + (k if k <= M else k - M)])
    cc = (b - a) / 4 * (2 if k == 0 else 1)
    one = mpf(1) if (k <= M and p <= M) else mpf(0)
    if k != p:
        return one, mpf(0), one, mpf(0)
    val = lambda l: one + cc * (1 / l + w * w * l)  # noqa: E731
    return val(ell), dd(val, ell), one + cc * (1 / ell + w * w * ell), cc * (1 / (ell * ell) + w * w)


def b1_A_elem(mesh, k, x):
    g0, g1, gl, gk, x = mpf(mesh[0]), mpf(mesh[1]), mpf(mesh[-1]), mpf(mesh[k]), mpf(x)
    if x < g0 or x > gl:
        return mpf(0), mpf(0), mpf(0), mpf(0)
    u = abs(x - gk) / (g1 - g0)
    return max(mpf(0), 1 - u), mpf(0), 1 + u, mpf(0)


def b1_K_elem(mesh, k, p, ell):
    m, d = len(mesh), mpf(mesh[1]) - mpf(mesh[0])
    kd, end = abs(k - p), (k == 0 or k == m - 1)
    A = B = BC = mpf(0)
    if kd == 0:
        A, B, BC = (d / 3, 1 / d, mpf(1)) if end else (2 * d / 3, 2 / d, mpf(0))
    elif kd == 1:
        A, B = d / 6, -1 / d
    val = lambda l: (A * l + B / l + BC) / 2  # noqa: E731
    return val(ell), (dd(val, ell) if kd <= 1 else mpf(0)), (abs(A) * ell + abs(B) / ell + BC) / 2, (abs(A) + abs(B) / (ell * ell)) / 2


# ---------------------------------------------------------------------------------------------------------------------------
def coords(lo, hi, knots, ell, extra):
    """columns: both ends, interior knots exactly, generic interior points, points outside on both sides (near, far, and at
    distances where exp underflows to a subnormal and to zero)"""
    span = hi - lo
    xs = [lo, hi] + list(knots) + list(extra) + [lo - 0.3 * span, hi + 0.7 * span, lo - 1e-9 * span, np.nextafter(hi, 9.0),
                                                lo - 720.0 * ell, hi + 735.0 * ell, lo - 800.0 * ell]
    return np.array(xs, dtype=np.float64)


def build_cases():
    pins = np.load(os.path.join(HERE, "ref_pins_basis.npz"))
    cases = []
    z = np.linspace(0, 1, 40)
    for kind in ("matern12", "matern32", "matern52", "rbf"):
        for ri, ratio in enumerate(RATIOS):
            ell = float(ratio * (z[1] - z[0]))
            x = coords(0.0, 1.0, [z[7], z[20], z[38]], ell, [0.013, 0.4999, 0.77, float(z[7]) + 1.7 * ell, float(z[20]) - 41.0 * ell])
            Aidx = [(k, p) for p in range(len(x)) for k in (0, 7, 19, 20, 39)]
            Kidx = [(0, 0), (0, 1), (1, 0), (7, 7), (3, 17), (39, 0), (0, 39), (20, 21), (38, 39), (39, 39), (12, 10), (5, 30)]
            cases.append(dict(kind=kind, basis="points", grid=z, x=x, ell=ell, flags=0, ratio=RATIO_TAGS[ri], Aidx=Aidx, Kidx=Kidx))
    mesh = np.linspace(0, 1, 33)
    for flags in (0, FLAG_B0_F32_KDELTA):
        for ri, ratio in enumerate(RATIOS):
            ell = float(ratio * (mesh[1] - mesh[0]))
            x = coords(0.0, 1.0, [mesh[5], mesh[16], mesh[31]], ell, [0.013, 0.4999, 0.77, float(mesh[5]) + 1.7 * ell, float(mesh[16]) - 0.3 * ell])
            Aidx = []
            for p, xv in enumerate(x):
                cell = int(np.searchsorted(mesh, xv, side="left")) - 1
                rows = {0, 15, 31} | {c for c in (cell - 1, cell, cell + 1) if 0 <= c < 32}
                Aidx += [(k, p) for k in sorted(rows)]
            Kidx = [(0, 0), (0, 1), (1, 0), (5, 7), (7, 5), (3, 17), (31, 0), (0, 31), (30, 31), (31, 31), (12, 9), (16, 16)]
            cases.append(dict(kind="matern12", basis="b0", grid=mesh, x=x, ell=ell, flags=flags, ratio=RATIO_TAGS[ri], Aidx=Aidx, Kidx=Kidx))
    for tag in ("vff_a", "vff_b"):
        M, a, b = int(pins[tag + "_M"]), float(pins[tag + "_a"]), float(pins[tag + "_b"])
        grid = np.concatenate([[a, b], pins[tag + "_omegas"].astype(np.float64)])
        m = 2 * M + 1
        for ri, ratio in enumerate(RATIOS):
            ell = float(ratio * (b - a) / M)
            x = coords(a, b, [], ell, list(pins[tag + "_x"][::6]) + [a + 0.5 * (b - a)])
            rows = sorted({0, 1, M, M + 1, m - 1})
            Aidx = [(k, p) for p in range(len(x)) for k in rows]
            Kidx = [(0, 0), (0, 1), (1, 1), (M, M), (M, M + 1), (M + 1, M + 1), (m - 1, m - 1), (m - 1, 0), (2, M), (M + 1, m - 1)]
            cases.append(dict(kind="matern12", basis="vff", grid=grid, x=x, ell=ell, flags=0, ratio=RATIO_TAGS[ri], Aidx=Aidx, Kidx=Kidx))
    for tag in ("b1_f64", "b1_f32"):
        g = pins[tag + "_mesh"].astype(np.float64)
        m = len(g)
        for ri, ratio in enumerate(RATIOS):
            ell = float(ratio * (g[1] - g[0]))
            x = coords(float(g[0]), float(g[-1]), [g[1], g[m // 2], g[m - 2]], ell, list(pins[tag + "_x"][::7]))
            Aidx = [(k, p) for p in range(len(x)) for k in range(m)]
            Kidx = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (0, 2), (m - 1, m - 1), (m - 2, m - 1), (m - 1, 0), (m // 2, m // 2)]
            cases.append(dict(kind="matern12", basis="b1", grid=g, x=x, ell=ell, flags=0, ratio=RATIO_TAGS[ri], Aidx=Aidx, Kidx=Kidx))
    return cases


def hp_case(c):
    ell, g, x, basis = mpf(c["ell"]), c["grid"], c["x"], c["basis"]
    A, K = [], []
    for k, p in c["Aidx"]:
        if basis == "points":
            A.append(points_elem(c["kind"], g[k], x[p], ell))
        elif basis == "b0":
            A.append(b0_A_elem(g[k], g[k + 1], x[p], ell))
        elif basis == "vff":
            A.append(vff_A_elem(g, k, x[p], ell))
        else:
            A.append(b1_A_elem(g, k, x[p]))
    for k, p in c["Kidx"]:
        if basis == "points":
            K.append(points_elem(c["kind"], g[k], g[p], ell))
        elif basis == "b0":
            K.append((b0_K_f32_elem if c["flags"] & FLAG_B0_F32_KDELTA else b0_K_elem)(abs(k - p), float(g[1] - g[0]), ell))
        elif basis == "vff":
            K.append(vff_K_elem(g, k, p, ell))
        else:
            K.append(b1_K_elem(g, k, p, ell))
    tof = lambda col, L: np.array([float(e[col]) for e in L], dtype=np.float64)  # noqa: E731
    # S is rounded UP to a double so that a stored scale is never below the true one
    up = lambda col, L: np.array([float(np.nextafter(float(e[col]), np.inf)) if e[col] > 0 else 0.0 for e in L])  # noqa: E731
    return dict(A0=tof(0, A), dA0=tof(1, A), S_A0=up(2, A), S_dA0=up(3, A), K0=tof(0, K), dK0=tof(1, K), S_K0=up(2, K), S_dK0=up(3, K))


def oracle_R(c, hp):
    """worst err / (eps S) of the numpy oracle per output; an element with S = 0 must be exact (inf otherwise)"""
    ns = SimpleNamespace(Aidx=np.array(c["Aidx"]), Kidx=np.array(c["Kidx"]))
    got = H.sample(ns, H.oracle_outputs(c["kind"], c["basis"], c["grid"], c["x"], c["ell"], c["flags"]))
    return np.array([H.ratio_to_bound(got[k], hp[k], hp["S_" + k]) for k in H.OUTPUTS])


def main():
    cases = build_cases()
    out = {"ncases": np.int64(len(cases))}
    for i, c in enumerate(cases):
        hp = hp_case(c)
        R = oracle_R(c, hp)
        pre = f"c{i:03d}_"
        out[pre + "kind"], out[pre + "basis"], out[pre + "ratio"] = np.str_(c["kind"]), np.str_(c["basis"]), np.str_(c["ratio"])
        out[pre + "grid"], out[pre + "x"] = np.asarray(c["grid"], np.float64), c["x"]
        out[pre + "ell"], out[pre + "flags"] = np.float64(c["ell"]), np.int64(c["flags"])
        out[pre + "Aidx"], out[pre + "Kidx"] = np.array(c["Aidx"], np.int64), np.array(c["Kidx"], np.int64)
        for k, v in hp.items():
            out[pre + k] = v
        out[pre + "R_outputs"], out[pre + "R_oracle"] = R, np.float64(R.max())
        print(f"{i:3d} {c['basis']:6s} {c['kind']:8s} flags {c['flags']} ell/spacing {c['ratio']:>6s}  R(A0, dA0, K0, dK0) = "
              + " ".join(f"{r:8.2f}" for r in R), flush=True)
    np.savez_compressed(os.path.join(HERE, "factor_hp.npz"), **out)


if __name__ == "__main__":
    main()
