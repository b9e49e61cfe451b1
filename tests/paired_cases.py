"""Case tables, split replica and reference side of the paired inducing-point path (VGGP_FLAG_PAIRED_Z; TEST HELPER, float64, CPU).

tests/test_gpu_paired_paths.py runs every case of these tables on the GPU; tests/test_paired_cases.py checks their premises on the
CPU: that each shape still reaches the tile / split path it was chosen for (`split_scattered`, `split_grid`), that Kuu takes no jitter
and stays below cond 1e8, and that the recorded round-off floors of the reference (`FLOORS`) are reproduced.

Reference: tests/general_z_spec.py (elbo / state / q_u / q_v / posterior) in float64 with torch autograd.

ELBO comparisons are made on the data-dependent part  ELBO - C0,  C0 = -(N log(2 pi sigma2) + yy / sigma2) / 2  (`c0`): at small M the
constant C0 is nearly all of the ELBO (-3.7e7 at M = 8, N = 524 353) and a wrong tile would hide behind it.

FLOORS[case][quantity]: the reference's own round-off, max-norm relative (`rel`), the larger of
    (1) specification against the dense restatement DensePaired (tests/test_general_z_spec.py) -- equal kinds only (it takes one
        kind), where N M <= 1e6 and its N x N evidence covariance is affordable (N <= DENSE_MAX_N);
    (2) specification against itself with the point order reversed and Z permuted (results permuted back): how far the reference
        moves under another order of summation.  Every case.
The bound used on the GPU is `bound(case, quantity)` = max(100 FLOORS, 1e-12), never above CEIL (the path's existing tolerances); the
factor 100 over the reference's own floor is the margin tests/test_gpu_exact_iter.py uses.  `PYTHONPATH=. python tests/paired_cases.py`
measures the floors again and prints the table.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import general_z_spec as S
from oracle import dense as D

KINDS = ("matern12", "matern32", "matern52", "rbf")
EQUAL = tuple((k, k) for k in KINDS)
MIXED = (("matern12", "matern52"), ("matern32", "rbf"), ("rbf", "matern12"))
M12 = ("matern12", "matern12")
THETA = (0.15, 0.2, 0.9, 1.1, 0.01)
DENSE_NM = 1_000_000         # DensePaired where N M <= 1e6 ...
DENSE_MAX_N = 3200           # ... and N <= 3200: it factors an N x N evidence covariance (82 MB at 3150; 4.6 GB at the 600 x 40 grid)

CEIL = dict(elbo=1e-7, grad_theta=1e-6, grad_z=1e-6)
Q_STEP = ("elbo", "grad_theta", "grad_z")
Q_READ = ("qu_mean", "qu_var", "qu_cov", "post_mean", "post_var", "post_cov", "qv_mean_lit", "qv_var_lit", "qv_mean_cond", "qv_var_cond")
for _q in Q_READ:
    CEIL[_q] = 1e-7

NS_POST = (1, 63, 64, 65, 130)           # COL1 column-tile edges of the posterior read-out
NS_COV = (1, 65)
MV = ((1, 1), (7, 9), (5, 13), (9, 8))   # 63 and 65 cells straddle the tile; mv2 divides into PzFace::val non-trivially


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- split replica -----------------------------------------------------------------------------------------------------------
# Mirrors, in csrc/paired.hip and csrc/gen_gemm.h:  pz_pass1_split (ns1),  the kchunk rounding of pz_gen_gemm,  tn_per2 / runs2 of
# vg_paired_plan,  pz_gram_split (gsplit).  PZ_T = 64, PZ_BK = 16, PZ_MB = 128.
PZ_T, PZ_BK, PZ_MB = 64, 16, 128


def _cdiv(a, b):
    return (a + b - 1) // b


def split_scattered(M, N):
    """-> (ns1, kchunk, empty_slabs, tn_per, runs2) of a scattered paired plan."""
    tn = _cdiv(M, PZ_T)
    tiles = tn * (tn + 1) // 2
    s = _cdiv(1024, tiles)
    s = min(s, max(1, N // (PZ_BK * 32)))
    ns1 = max(1, min(s, 128))
    kchunk = _cdiv(_cdiv(N, ns1), PZ_BK) * PZ_BK
    empty = sum(1 for ks in range(ns1) if ks * kchunk >= N)
    tiles_m, tiles_n = _cdiv(M, PZ_T), _cdiv(N, PZ_T)
    runs = max(1, min(tiles_n, 8192 // tiles_m))
    tn_per = _cdiv(tiles_n, runs)
    runs2 = _cdiv(tiles_n, tn_per)
    return ns1, kchunk, empty, tn_per, runs2


def last_run(N, tn_per):
    """-> (column tiles of pass 2's last run, points of its last tile)."""
    tiles_n = _cdiv(N, PZ_T)
    return tiles_n - (_cdiv(tiles_n, tn_per) - 1) * tn_per, N - (tiles_n - 1) * PZ_T


def _gram_split(M, n):
    t = _cdiv(M, 64)
    s = _cdiv(1024, 3 * t * t)
    s = min(s, max(1, n // 256))
    return max(1, min(s, 16))


def split_grid(M, n1, n2):
    """-> (gsplit1, gsplit2) of a full-grid paired plan."""
    return _gram_split(M, n1), _gram_split(M, n2)


# ---- case tables -------------------------------------------------------------------------------------------------------------
def _case(layout, kinds, M, shape, seed=0, coincide=False, readouts=False):
    return dict(layout=layout, kinds=tuple(kinds), M=M, shape=shape, seed=seed, coincide=coincide, readouts=readouts)


def _kn(kinds):
    return kinds[0][-2:] + kinds[1][-2:] if "rbf" not in kinds else "_".join(k.replace("matern", "") for k in kinds)


# A: scattered step, tile and split edges.  name -> expected (ns1, kchunk, empty_slabs, tn_per, runs2)
A_EXPECT = {
    (1, 1): (1, 16, 0, 1, 1),
    (2, 3): (1, 16, 0, 1, 1),
    (15, 1030): (2, 528, 0, 1, 17), (16, 1030): (2, 528, 0, 1, 17), (17, 1030): (2, 528, 0, 1, 17),
    (63, 1000): (1, 1008, 0, 1, 16), (64, 1000): (1, 1008, 0, 1, 16), (65, 1000): (1, 1008, 0, 1, 16),
    (64, 1024): (2, 512, 0, 1, 16),
    (127, 700): (1, 704, 0, 1, 11), (128, 700): (1, 704, 0, 1, 11), (129, 700): (1, 704, 0, 1, 11),
    (257, 2100): (4, 528, 0, 1, 33),
    (20, 32769): (64, 528, 1, 1, 513),
    (130, 65537): (128, 528, 3, 1, 1025),
    (8, 524289): (128, 4112, 0, 2, 4097),          # 8193 column tiles: the last run holds ONE tile, and that tile one point
    (8, 524353): (128, 4112, 0, 2, 4097),
    (8, 1048641): (128, 8208, 0, 3, 5462),
    (65, 262209): (128, 2064, 0, 2, 2049),
}
A_CASES = {}
for (_M, _N) in A_EXPECT:
    _kinds = ("matern32", "rbf") if (_M, _N) == (65, 262209) else M12
    A_CASES[f"A_{_M}_{_N}"] = _case("scattered", _kinds, _M, _N, readouts=(_N, _M) in ((1030, 17), (700, 129)))

# B: kinds.  Scattered M = 65, N = 1000 and full grid M = 65, 70 x 45; all with every read-out of D
B_CASES = {}
for _kinds in EQUAL + MIXED:
    B_CASES[f"B_s_{_kn(_kinds)}"] = _case("scattered", _kinds, 65, 1000, seed=1, readouts=True)
    B_CASES[f"B_g_{_kn(_kinds)}"] = _case("grid", _kinds, 65, (70, 45), seed=1, readouts=True)
B_CASES["B_s_coincide"] = _case("scattered", ("matern12", "matern52"), 65, 1000, seed=2, coincide=True, readouts=True)
B_CASES["B_g_coincide"] = _case("grid", ("matern12", "matern52"), 65, (70, 45), seed=2, coincide=True, readouts=True)

# C: full-grid shapes, random Z.  name -> expected gsplit
C_EXPECT = {(1, (1, 1)): (1, 1), (20, (600, 40)): (2, 1), (65, (513, 1)): (2, 1), (129, (37, 300)): (1, 1), (64, (70, 45)): (1, 1)}
C_CASES = {f"C_{_M}_{_s[0]}x{_s[1]}": _case("grid", M12, _M, _s, seed=3) for (_M, _s) in C_EXPECT}
C_TWIN = "C_64_70x45"            # ... also planned scattered on its 3150 grid nodes: the two GPU routes must agree

# D: read-outs at M in {17, 129} scattered for the kinds of B (M = 65 scattered and grid: the B cases themselves)
D_CASES = {}
for _kinds in EQUAL + MIXED:
    if _kinds != M12:            # (Matern-1/2 at these two shapes: A_17_1030 and A_129_700)
        D_CASES[f"D_17_{_kn(_kinds)}"] = _case("scattered", _kinds, 17, 1030, seed=4, readouts=True)
        D_CASES[f"D_129_{_kn(_kinds)}"] = _case("scattered", _kinds, 129, 700, seed=4, readouts=True)

CASES = {**A_CASES, **B_CASES, **C_CASES, **D_CASES}
READOUT_CASES = tuple(n for n, c in CASES.items() if c["readouts"])


ELL = {"matern12": (0.15, 0.2), "matern32": (0.1, 0.13), "matern52": (0.08, 0.1), "rbf": (0.06, 0.07)}


def theta_for(kinds, M):
    """theta of the tables: [0.15, 0.2, 0.9, 1.1, 0.01] for Matern-1/2.  An RBF dimension takes the short lengthscale of the existing tests
    (0.06 / 0.07 at M = 60) so that Kuu takes no jitter and stays below cond 1e8; the smoother Matern kinds take shorter ones as well, and
    all three shrink with the point spacing 1 / sqrt(M) above M = 60: with the table's 0.15 / 0.2 the reference's own floor of the
    read-outs at M = 129 (3e-7 for Matern-3/2, 1e-7 for Matern-5/2) left no factor 100 below the 1e-7 ceiling."""
    th = list(THETA)
    for d in (0, 1):
        th[d] = ELL[kinds[d]][d] * (1.0 if kinds[d] == "matern12" else min(1.0, math.sqrt(60.0 / M)))
    return th


# ---- problems ----------------------------------------------------------------------------------------------------------------
def problem(layout, kinds, M, shape, seed, coincide=False):
    """-> dict(Z [M, 2], theta [5], y (flat, x1 fastest on a grid), and X [N, 2] (scattered) or x1, x2 (grid axes)).
    coincide: the first M // 2 inducing points are data points (scattered) / have grid-node coordinates (grid): d = 0 occurs."""
    rng = np.random.default_rng([seed, M, 11])
    Z = rng.random((M, 2))
    out = dict(layout=layout, kinds=tuple(kinds), M=M, theta=theta_for(kinds, M))
    if layout == "scattered":
        N = int(shape)
        X = rng.random((N, 2))
        y = D.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(N)
        if coincide:
            h = min(M // 2, N)
            Z[:h] = X[:h]
        out.update(X=X, y=y, N=N)
    else:
        n1, n2 = shape
        _, y, x1, x2 = D.gen_grid(n1, n2, seed=seed)
        if coincide:
            h = min(M // 2, n1 * n2)
            nodes = rng.choice(n1 * n2, h, replace=False)          # (distinct nodes: no two inducing points coincide)
            Z[:h, 0] = x1[nodes % n1]
            Z[:h, 1] = x2[nodes // n1]
        out.update(x1=x1, x2=x2, y=y, N=n1 * n2, n1=n1, n2=n2)
    out["Z"] = Z
    out["yy"] = float((y * y).sum())
    return out


def case_problem(name):
    c = CASES[name]
    return problem(c["layout"], c["kinds"], c["M"], c["shape"], c["seed"], c["coincide"])


def grid_points(p):
    """The grid nodes of a grid problem as scattered points, in the order of y (x1 fastest)."""
    X1, X2 = np.meshgrid(p["x1"], p["x2"])
    return np.stack([X1.ravel(), X2.ravel()], axis=1)


def c0(N, yy, sigma2):
    return -(N * math.log(2.0 * math.pi * sigma2) + yy / sigma2) / 2.0


def duplicate_problem():
    """Two identical inducing points: Kuu is singular and the jitter schedule steps in (the one case with jitter > 0)."""
    p = problem("scattered", M12, 30, 300, seed=6)
    p["Z"][1] = p["Z"][0]
    p["theta"] = [0.3, 0.3, 0.5, 0.5, 0.01]          # s = 0.25: the duplicated pivot is exactly zero
    return p


def readout_inputs(M, seed=9):
    """-> xs [130, 2], {(mv1, mv2): (C1 [mv1, M], C2 [mv2, M], kd1 [mv1], kd2 [mv2])}: any matrices serve the C entry."""
    rng = np.random.default_rng([seed, M, 12])
    xs = rng.random((max(NS_POST), 2))
    mats = {}
    for mv1, mv2 in MV:
        mats[(mv1, mv2)] = (rng.random((mv1, M)), rng.random((mv2, M)), 0.5 + rng.random(mv1), 0.5 + rng.random(mv2))
    return xs, mats


# ---- reference ---------------------------------------------------------------------------------------------------------------
def _spec_kw(p, reverse=False):
    """y and the X= / grid= arguments of general_z_spec for a problem (reverse: the points in the opposite order)."""
    if p["layout"] == "scattered":
        X, y = (p["X"][::-1].copy(), p["y"][::-1].copy()) if reverse else (p["X"], p["y"])
        return torch.tensor(y), dict(X=torch.tensor(X))
    Y = p["y"].reshape(p["n2"], p["n1"])
    x1, x2 = p["x1"], p["x2"]
    if reverse:
        Y, x1, x2 = Y[::-1, ::-1].copy(), x1[::-1].copy(), x2[::-1].copy()
    return torch.tensor(Y), dict(grid=(torch.tensor(x1), torch.tensor(x2)))


def spec_step(p, perm=None, reverse=False, as_points=False):
    """Specification of the step -> dict(elbo (the part ELBO - C0), grad_theta [5], grad_z [M, 2], jitter).  perm: Z rows in that order
    (results permuted back); as_points: a grid problem through the X= form on its nodes."""
    Z = p["Z"] if perm is None else p["Z"][perm]
    th = torch.tensor(p["theta"], dtype=torch.float64, requires_grad=True)
    Zt = torch.tensor(Z, requires_grad=True)
    if as_points:
        y, kw = torch.tensor(p["y"]), dict(X=torch.tensor(grid_points(p)))
    else:
        y, kw = _spec_kw(p, reverse)
    e, jit = S.elbo(p["kinds"], Zt, th, y, **kw)
    g, gz = torch.autograd.grad(e, [th, Zt])
    gz = gz.numpy()
    if perm is not None:
        back = np.empty_like(gz)
        back[perm] = gz
        gz = back
    return dict(elbo=e.item() - c0(p["N"], p["yy"], p["theta"][4]), grad_theta=g.numpy(), grad_z=gz, jitter=jit)


def spec_readouts(p, perm=None, reverse=False):
    """Specification of every read-out of section D -> flat dict of numpy arrays (keys `readout_keys()`)."""
    M = p["M"]
    idx = np.arange(M) if perm is None else np.asarray(perm)
    inv = np.empty(M, dtype=np.int64)
    inv[idx] = np.arange(M)
    Zt, th = torch.tensor(p["Z"][idx]), torch.tensor(p["theta"], dtype=torch.float64)
    y, kw = _spec_kw(p, reverse)
    st = S.state(p["kinds"], Zt, th, y, **kw)
    out = {}
    mu, cov = S.q_u(st)
    out["qu_mean"], out["qu_cov"] = mu.numpy()[inv], cov.numpy()[np.ix_(inv, inv)]
    out["qu_var"] = np.diagonal(out["qu_cov"]).copy()
    xs, mats = readout_inputs(M)
    pm, pc = S.posterior(st, p["kinds"], Zt, th, torch.tensor(xs))
    out["post_mean"], out["post_cov"] = pm.numpy(), pc.numpy()
    out["post_var"] = np.diagonal(out["post_cov"]).copy()
    for (mv1, mv2), (C1, C2, kd1, kd2) in mats.items():
        for literal in (True, False):
            m, v = S.q_v(st, torch.tensor(C1[:, idx]), torch.tensor(C2[:, idx]), torch.tensor(kd1), torch.tensor(kd2), literal=literal)
            tag = "lit" if literal else "cond"
            out[f"qv_mean_{tag}_{mv1}x{mv2}"], out[f"qv_var_{tag}_{mv1}x{mv2}"] = m.numpy(), v.numpy()
    return out


def readout_floor(a, b):
    """Floors of the read-out quantities between two evaluations a, b of spec_readouts: the worst over the sizes the GPU tests use."""
    f = {q: rel(a[q], b[q]) for q in ("qu_mean", "qu_var", "qu_cov")}
    f["post_mean"] = max(rel(a["post_mean"][:ns], b["post_mean"][:ns]) for ns in NS_POST)
    f["post_var"] = max(rel(a["post_var"][:ns], b["post_var"][:ns]) for ns in NS_POST)
    f["post_cov"] = max(rel(a["post_cov"][:ns, :ns], b["post_cov"][:ns, :ns]) for ns in NS_COV)
    for tag in ("lit", "cond"):
        for q in ("mean", "var"):
            f[f"qv_{q}_{tag}"] = max(rel(a[f"qv_{q}_{tag}_{m1}x{m2}"], b[f"qv_{q}_{tag}_{m1}x{m2}"]) for m1, m2 in MV)
    return f


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference of a case, computed once and shared by the tests (treat as read-only): dict(p, step, read (or None))."""
    p = case_problem(name)
    return dict(p=p, step=spec_step(p), read=spec_readouts(p) if CASES[name]["readouts"] else None)


def _dense(p):
    """DensePaired on a problem (theta as a leaf, so that its gradient is d/d theta)."""
    from test_general_z_spec import DensePaired
    X = p["X"] if p["layout"] == "scattered" else grid_points(p)
    th = torch.tensor(p["theta"], dtype=torch.float64, requires_grad=True)
    return DensePaired(X, p["y"], p["kinds"][0], p["Z"], theta=th), th


def measure_floors(name):
    """FLOORS[name], measured again (CPU; on one thread, so that the BLAS summation order -- and with it the measured round-off -- does
    not depend on the number of cores)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        p = case_problem(name)
        return _measure_floors(name, dict(p=p, step=spec_step(p), read=spec_readouts(p) if CASES[name]["readouts"] else None))
    finally:
        torch.set_num_threads(n)


def _measure_floors(name, ref):
    c = CASES[name]
    p, M = ref["p"], c["M"]
    perm = np.random.default_rng([M, 13]).permutation(M)
    other = spec_step(p, perm=perm, reverse=True)
    f = {q: rel(other[q], ref["step"][q]) for q in Q_STEP}
    use_dense = c["kinds"][0] == c["kinds"][1] and p["N"] * M <= DENSE_NM and p["N"] <= DENSE_MAX_N
    if use_dense:
        dm, th = _dense(p)
        e = dm._elbo()
        g, gz = torch.autograd.grad(e, [th, dm.Z])
        f["elbo"] = max(f["elbo"], rel(e.item() - c0(p["N"], p["yy"], p["theta"][4]), ref["step"]["elbo"]))
        f["grad_theta"] = max(f["grad_theta"], rel(g.numpy(), ref["step"]["grad_theta"]))
        f["grad_z"] = max(f["grad_z"], rel(gz.numpy(), ref["step"]["grad_z"]))
    if c["readouts"]:
        f.update(readout_floor(spec_readouts(p, perm=perm, reverse=True), ref["read"]))
        if use_dense:
            with torch.no_grad():
                dm, _ = _dense(p)
                qd = dm.q_v()
                xs, _ = readout_inputs(M)
                pd = dm.posterior(torch.tensor(xs))
            r = ref["read"]
            f["qu_mean"] = max(f["qu_mean"], rel(qd.mean.numpy(), r["qu_mean"]))
            f["qu_cov"] = max(f["qu_cov"], rel(qd.covariance_matrix.numpy(), r["qu_cov"]))
            f["qu_var"] = max(f["qu_var"], rel(qd.variance.numpy(), r["qu_var"]))
            f["post_mean"] = max(f["post_mean"], rel(pd.mean.numpy(), r["post_mean"]))
            f["post_cov"] = max(f["post_cov"], rel(pd.covariance_matrix.numpy(), r["post_cov"]))
            f["post_var"] = max(f["post_var"], rel(pd.variance.numpy(), r["post_var"]))
    if name == C_TWIN:           # the specification's grid= against its X= form: the floor of the two GPU routes' agreement
        pts = spec_step(p, as_points=True)
        for q in Q_STEP:
            f["twin_" + q] = rel(pts[q], ref["step"][q])
    return f


def bound(name, q):
    """The GPU tests' bound: 100 times the reference's floor, at least 1e-12, at most the path's ceiling."""
    ceil = CEIL[q[5:] if q.startswith("twin_") else q]
    return min(max(100.0 * FLOORS[name][q], 1e-12), ceil)


def kuu_cond(p):
    th = p["theta"]
    Z = torch.tensor(p["Z"])
    K = th[2] * th[3] * S.unit_k(p["kinds"][0], Z[:, 0], Z[:, 0], th[0]) * S.unit_k(p["kinds"][1], Z[:, 1], Z[:, 1], th[1])
    return float(torch.linalg.cond(K))


# measured by this file's __main__ (one thread)
FLOORS = {
    "A_1_1": {"elbo": 0.0e+00, "grad_theta": 1.0e-18, "grad_z": 4.3e-16},
    "A_2_3": {"elbo": 6.0e-16, "grad_theta": 4.3e-16, "grad_z": 1.3e-15},
    "A_15_1030": {"elbo": 3.0e-14, "grad_theta": 7.9e-15, "grad_z": 3.7e-14},
    "A_16_1030": {"elbo": 2.0e-15, "grad_theta": 3.5e-16, "grad_z": 5.5e-14},
    "A_17_1030": {"elbo": 8.1e-15, "grad_theta": 3.5e-15, "grad_z": 1.8e-14, "qu_mean": 4.0e-15, "qu_var": 1.2e-14, "qu_cov": 1.2e-14, "post_mean": 6.2e-15, "post_var": 4.5e-16, "post_cov": 7.9e-16, "qv_mean_lit": 8.1e-15, "qv_var_lit": 7.1e-16, "qv_mean_cond": 8.1e-15, "qv_var_cond": 5.0e-16},
    "A_63_1000": {"elbo": 3.9e-16, "grad_theta": 5.0e-15, "grad_z": 1.9e-13},
    "A_64_1000": {"elbo": 1.0e-15, "grad_theta": 1.9e-15, "grad_z": 1.8e-13},
    "A_65_1000": {"elbo": 6.4e-16, "grad_theta": 3.8e-15, "grad_z": 6.3e-13},
    "A_64_1024": {"elbo": 7.7e-16, "grad_theta": 1.9e-15, "grad_z": 8.4e-14},
    "A_127_700": {"elbo": 1.8e-15, "grad_theta": 8.0e-15, "grad_z": 2.5e-12},
    "A_128_700": {"elbo": 4.8e-16, "grad_theta": 2.0e-15, "grad_z": 4.9e-13},
    "A_129_700": {"elbo": 9.8e-16, "grad_theta": 4.0e-15, "grad_z": 5.3e-13, "qu_mean": 3.5e-12, "qu_var": 1.9e-12, "qu_cov": 1.9e-12, "post_mean": 2.5e-12, "post_var": 1.6e-14, "post_cov": 1.6e-14, "qv_mean_lit": 6.8e-12, "qv_var_lit": 4.5e-14, "qv_mean_cond": 6.8e-12, "qv_var_cond": 2.2e-13},
    "A_257_2100": {"elbo": 3.0e-15, "grad_theta": 1.2e-14, "grad_z": 7.7e-12},
    "A_20_32769": {"elbo": 1.3e-13, "grad_theta": 5.0e-15, "grad_z": 1.4e-13},
    "A_130_65537": {"elbo": 1.6e-15, "grad_theta": 8.6e-15, "grad_z": 2.0e-10},
    "A_8_524289": {"elbo": 9.3e-15, "grad_theta": 1.4e-15, "grad_z": 1.2e-14},
    "A_8_524353": {"elbo": 3.5e-15, "grad_theta": 3.7e-16, "grad_z": 5.1e-15},
    "A_8_1048641": {"elbo": 2.3e-15, "grad_theta": 1.2e-16, "grad_z": 5.9e-15},
    "A_65_262209": {"elbo": 7.9e-15, "grad_theta": 1.6e-14, "grad_z": 1.6e-12},
    "B_s_1212": {"elbo": 2.0e-15, "grad_theta": 4.2e-15, "grad_z": 5.8e-13, "qu_mean": 1.1e-12, "qu_var": 1.0e-12, "qu_cov": 1.0e-12, "post_mean": 9.3e-13, "post_var": 6.3e-15, "post_cov": 5.5e-15, "qv_mean_lit": 1.4e-12, "qv_var_lit": 3.0e-14, "qv_mean_cond": 1.4e-12, "qv_var_cond": 3.1e-13},
    "B_g_1212": {"elbo": 3.7e-16, "grad_theta": 2.3e-15, "grad_z": 5.7e-13, "qu_mean": 1.5e-12, "qu_var": 2.5e-12, "qu_cov": 2.5e-12, "post_mean": 1.2e-12, "post_var": 7.7e-15, "post_cov": 7.7e-15, "qv_mean_lit": 1.9e-11, "qv_var_lit": 9.5e-14, "qv_mean_cond": 1.9e-11, "qv_var_cond": 1.0e-13},
    "B_s_3232": {"elbo": 4.3e-15, "grad_theta": 1.2e-14, "grad_z": 2.3e-12, "qu_mean": 6.0e-12, "qu_var": 1.4e-12, "qu_cov": 1.4e-12, "post_mean": 6.6e-12, "post_var": 1.0e-13, "post_cov": 1.0e-13, "qv_mean_lit": 2.7e-11, "qv_var_lit": 2.4e-12, "qv_mean_cond": 2.7e-11, "qv_var_cond": 6.1e-14},
    "B_g_3232": {"elbo": 6.9e-15, "grad_theta": 9.4e-15, "grad_z": 4.7e-12, "qu_mean": 4.7e-12, "qu_var": 2.8e-12, "qu_cov": 2.8e-12, "post_mean": 5.1e-12, "post_var": 3.2e-14, "post_cov": 4.4e-14, "qv_mean_lit": 2.2e-11, "qv_var_lit": 7.0e-12, "qv_mean_cond": 2.2e-11, "qv_var_cond": 1.3e-13},
    "B_s_5252": {"elbo": 4.4e-15, "grad_theta": 9.8e-15, "grad_z": 2.7e-12, "qu_mean": 3.1e-12, "qu_var": 9.3e-13, "qu_cov": 9.4e-13, "post_mean": 3.8e-12, "post_var": 4.7e-14, "post_cov": 5.4e-14, "qv_mean_lit": 2.8e-12, "qv_var_lit": 7.5e-13, "qv_mean_cond": 2.8e-12, "qv_var_cond": 8.3e-14},
    "B_g_5252": {"elbo": 1.3e-14, "grad_theta": 1.9e-14, "grad_z": 7.6e-12, "qu_mean": 1.6e-12, "qu_var": 1.4e-12, "qu_cov": 1.4e-12, "post_mean": 1.8e-12, "post_var": 5.1e-14, "post_cov": 5.1e-14, "qv_mean_lit": 2.2e-12, "qv_var_lit": 3.8e-12, "qv_mean_cond": 2.2e-12, "qv_var_cond": 7.8e-14},
    "B_s_rbf_rbf": {"elbo": 3.9e-15, "grad_theta": 2.6e-15, "grad_z": 1.3e-12, "qu_mean": 8.6e-13, "qu_var": 4.4e-13, "qu_cov": 4.4e-13, "post_mean": 1.1e-12, "post_var": 6.9e-14, "post_cov": 1.2e-13, "qv_mean_lit": 9.7e-13, "qv_var_lit": 5.5e-13, "qv_mean_cond": 9.7e-13, "qv_var_cond": 2.0e-13},
    "B_g_rbf_rbf": {"elbo": 6.1e-15, "grad_theta": 8.6e-15, "grad_z": 1.3e-12, "qu_mean": 1.0e-12, "qu_var": 6.7e-13, "qu_cov": 6.7e-13, "post_mean": 1.1e-12, "post_var": 8.7e-14, "post_cov": 8.7e-14, "qv_mean_lit": 1.1e-12, "qv_var_lit": 2.8e-13, "qv_mean_cond": 1.1e-12, "qv_var_cond": 2.1e-13},
    "B_s_1252": {"elbo": 0.0e+00, "grad_theta": 5.0e-16, "grad_z": 1.0e-13, "qu_mean": 2.4e-12, "qu_var": 1.1e-12, "qu_cov": 1.1e-12, "post_mean": 1.9e-12, "post_var": 7.3e-15, "post_cov": 9.6e-15, "qv_mean_lit": 1.9e-12, "qv_var_lit": 3.7e-14, "qv_mean_cond": 1.9e-12, "qv_var_cond": 1.7e-13},
    "B_g_1252": {"elbo": 6.1e-16, "grad_theta": 1.4e-15, "grad_z": 1.5e-13, "qu_mean": 1.6e-12, "qu_var": 1.4e-12, "qu_cov": 1.4e-12, "post_mean": 1.8e-12, "post_var": 9.9e-15, "post_cov": 9.9e-15, "qv_mean_lit": 1.3e-12, "qv_var_lit": 4.9e-14, "qv_mean_cond": 1.3e-12, "qv_var_cond": 3.6e-14},
    "B_s_32_rbf": {"elbo": 1.3e-15, "grad_theta": 2.2e-15, "grad_z": 3.1e-13, "qu_mean": 1.9e-12, "qu_var": 7.7e-13, "qu_cov": 9.4e-13, "post_mean": 1.4e-12, "post_var": 1.0e-13, "post_cov": 1.0e-13, "qv_mean_lit": 2.1e-12, "qv_var_lit": 5.3e-13, "qv_mean_cond": 2.1e-12, "qv_var_cond": 1.2e-13},
    "B_g_32_rbf": {"elbo": 6.7e-15, "grad_theta": 8.6e-15, "grad_z": 4.8e-12, "qu_mean": 3.3e-12, "qu_var": 3.4e-12, "qu_cov": 3.9e-12, "post_mean": 2.3e-12, "post_var": 5.2e-14, "post_cov": 2.2e-14, "qv_mean_lit": 1.2e-11, "qv_var_lit": 3.3e-12, "qv_mean_cond": 1.2e-11, "qv_var_cond": 4.6e-14},
    "B_s_rbf_12": {"elbo": 1.7e-15, "grad_theta": 4.1e-15, "grad_z": 1.1e-12, "qu_mean": 2.0e-12, "qu_var": 4.1e-13, "qu_cov": 4.6e-13, "post_mean": 2.7e-12, "post_var": 1.5e-14, "post_cov": 1.6e-14, "qv_mean_lit": 5.2e-11, "qv_var_lit": 4.1e-13, "qv_mean_cond": 5.2e-11, "qv_var_cond": 6.8e-14},
    "B_g_rbf_12": {"elbo": 5.4e-15, "grad_theta": 1.7e-14, "grad_z": 8.0e-12, "qu_mean": 3.6e-12, "qu_var": 9.7e-13, "qu_cov": 9.7e-13, "post_mean": 3.7e-12, "post_var": 2.1e-14, "post_cov": 2.1e-14, "qv_mean_lit": 2.1e-11, "qv_var_lit": 1.9e-12, "qv_mean_cond": 2.1e-11, "qv_var_cond": 1.3e-13},
    "B_s_coincide": {"elbo": 2.7e-15, "grad_theta": 7.5e-15, "grad_z": 3.8e-12, "qu_mean": 9.9e-13, "qu_var": 3.9e-13, "qu_cov": 3.9e-13, "post_mean": 1.3e-12, "post_var": 7.9e-14, "post_cov": 4.1e-14, "qv_mean_lit": 8.8e-12, "qv_var_lit": 9.4e-13, "qv_mean_cond": 8.8e-12, "qv_var_cond": 1.3e-13},
    "B_g_coincide": {"elbo": 2.1e-15, "grad_theta": 1.8e-15, "grad_z": 3.6e-13, "qu_mean": 1.4e-13, "qu_var": 3.4e-13, "qu_cov": 3.4e-13, "post_mean": 1.2e-13, "post_var": 3.5e-15, "post_cov": 3.5e-15, "qv_mean_lit": 3.7e-13, "qv_var_lit": 8.5e-14, "qv_mean_cond": 3.7e-13, "qv_var_cond": 4.9e-15},
    "C_1_1x1": {"elbo": 5.7e-16, "grad_theta": 3.4e-19, "grad_z": 0.0e+00},
    "C_20_600x40": {"elbo": 1.2e-14, "grad_theta": 2.4e-15, "grad_z": 7.8e-14},
    "C_65_513x1": {"elbo": 9.4e-16, "grad_theta": 6.1e-15, "grad_z": 1.6e-13},
    "C_129_37x300": {"elbo": 3.6e-16, "grad_theta": 1.6e-15, "grad_z": 1.1e-12},
    "C_64_70x45": {"elbo": 3.4e-15, "grad_theta": 4.7e-15, "grad_z": 3.2e-13, "twin_elbo": 6.5e-16, "twin_grad_theta": 8.5e-16, "twin_grad_z": 2.2e-13},
    "D_17_3232": {"elbo": 3.8e-15, "grad_theta": 1.4e-15, "grad_z": 5.1e-14, "qu_mean": 7.6e-15, "qu_var": 1.1e-14, "qu_cov": 1.1e-14, "post_mean": 5.7e-15, "post_var": 6.7e-16, "post_cov": 6.7e-16, "qv_mean_lit": 1.3e-14, "qv_var_lit": 7.5e-16, "qv_mean_cond": 1.3e-14, "qv_var_cond": 5.2e-16},
    "D_129_3232": {"elbo": 1.4e-15, "grad_theta": 2.6e-15, "grad_z": 4.6e-12, "qu_mean": 2.7e-12, "qu_var": 1.0e-12, "qu_cov": 1.0e-12, "post_mean": 3.3e-12, "post_var": 1.4e-13, "post_cov": 7.1e-14, "qv_mean_lit": 3.2e-12, "qv_var_lit": 9.6e-13, "qv_mean_cond": 3.2e-12, "qv_var_cond": 1.1e-12},
    "D_17_5252": {"elbo": 1.5e-14, "grad_theta": 7.9e-16, "grad_z": 5.5e-14, "qu_mean": 1.8e-15, "qu_var": 3.1e-15, "qu_cov": 3.1e-15, "post_mean": 1.2e-15, "post_var": 8.3e-16, "post_cov": 9.0e-16, "qv_mean_lit": 9.0e-14, "qv_var_lit": 7.5e-16, "qv_mean_cond": 9.0e-14, "qv_var_cond": 5.4e-16},
    "D_129_5252": {"elbo": 1.3e-15, "grad_theta": 1.2e-15, "grad_z": 1.2e-12, "qu_mean": 3.0e-12, "qu_var": 4.7e-13, "qu_cov": 4.7e-13, "post_mean": 3.5e-12, "post_var": 2.0e-13, "post_cov": 2.0e-13, "qv_mean_lit": 2.5e-12, "qv_var_lit": 3.8e-13, "qv_mean_cond": 2.5e-12, "qv_var_cond": 3.9e-13},
    "D_17_rbf_rbf": {"elbo": 2.5e-14, "grad_theta": 6.5e-15, "grad_z": 4.8e-14, "qu_mean": 1.9e-15, "qu_var": 2.7e-15, "qu_cov": 3.1e-15, "post_mean": 1.9e-15, "post_var": 4.5e-16, "post_cov": 5.6e-16, "qv_mean_lit": 8.1e-15, "qv_var_lit": 5.2e-16, "qv_mean_cond": 8.1e-15, "qv_var_cond": 7.0e-16},
    "D_129_rbf_rbf": {"elbo": 3.1e-15, "grad_theta": 4.2e-15, "grad_z": 7.3e-14, "qu_mean": 2.6e-13, "qu_var": 5.8e-14, "qu_cov": 5.8e-14, "post_mean": 3.2e-13, "post_var": 4.5e-14, "post_cov": 9.2e-14, "qv_mean_lit": 3.8e-13, "qv_var_lit": 4.4e-13, "qv_mean_cond": 3.8e-13, "qv_var_cond": 2.4e-14},
    "D_17_1252": {"elbo": 1.9e-15, "grad_theta": 5.0e-16, "grad_z": 3.2e-15, "qu_mean": 3.1e-15, "qu_var": 6.7e-15, "qu_cov": 6.7e-15, "post_mean": 3.1e-15, "post_var": 4.5e-16, "post_cov": 3.4e-16, "qv_mean_lit": 2.5e-14, "qv_var_lit": 5.5e-16, "qv_mean_cond": 2.5e-14, "qv_var_cond": 4.0e-16},
    "D_129_1252": {"elbo": 9.9e-16, "grad_theta": 1.0e-15, "grad_z": 9.1e-13, "qu_mean": 7.7e-12, "qu_var": 2.7e-12, "qu_cov": 2.7e-12, "post_mean": 8.1e-12, "post_var": 4.4e-14, "post_cov": 1.1e-14, "qv_mean_lit": 5.9e-12, "qv_var_lit": 5.6e-14, "qv_mean_cond": 5.9e-12, "qv_var_cond": 2.3e-12},
    "D_17_32_rbf": {"elbo": 0.0e+00, "grad_theta": 1.4e-16, "grad_z": 7.7e-16, "qu_mean": 1.4e-15, "qu_var": 1.6e-15, "qu_cov": 1.6e-15, "post_mean": 1.2e-15, "post_var": 3.4e-16, "post_cov": 4.5e-16, "qv_mean_lit": 7.4e-15, "qv_var_lit": 6.6e-16, "qv_mean_cond": 7.4e-15, "qv_var_cond": 5.2e-16},
    "D_129_32_rbf": {"elbo": 3.1e-15, "grad_theta": 3.5e-15, "grad_z": 2.5e-12, "qu_mean": 1.0e-12, "qu_var": 3.9e-13, "qu_cov": 3.9e-13, "post_mean": 1.0e-12, "post_var": 7.0e-14, "post_cov": 4.0e-14, "qv_mean_lit": 2.7e-12, "qv_var_lit": 1.4e-12, "qv_mean_cond": 2.7e-12, "qv_var_cond": 1.1e-12},
    "D_17_rbf_12": {"elbo": 2.8e-14, "grad_theta": 3.0e-16, "grad_z": 1.2e-14, "qu_mean": 8.4e-15, "qu_var": 4.1e-15, "qu_cov": 5.7e-15, "post_mean": 7.9e-15, "post_var": 5.7e-16, "post_cov": 5.7e-16, "qv_mean_lit": 6.0e-14, "qv_var_lit": 4.0e-16, "qv_mean_cond": 6.0e-14, "qv_var_cond": 4.2e-16},
    "D_129_rbf_12": {"elbo": 2.7e-15, "grad_theta": 2.8e-15, "grad_z": 1.8e-12, "qu_mean": 4.8e-12, "qu_var": 9.1e-13, "qu_cov": 9.1e-13, "post_mean": 5.9e-12, "post_var": 9.1e-14, "post_cov": 2.9e-14, "qv_mean_lit": 5.2e-11, "qv_var_lit": 4.9e-13, "qv_mean_cond": 5.2e-11, "qv_var_cond": 8.3e-13},
}


if __name__ == "__main__":
    print("FLOORS = {")
    for _name in CASES:
        _f = measure_floors(_name)
        print(f'    "{_name}": {{' + ", ".join(f'"{k}": {v:.1e}' for k, v in _f.items()) + "},", flush=True)
    print("}")
