"""Case tables, host-decision replica and reference side of the dense masked and scattered steps (csrc/masked.hip,
csrc/masked_readout.hip; TEST HELPER, float64, CPU).

tests/test_gpu_masked_dense_paths.py runs every case of these tables on the GPU; tests/test_masked_dense_cases.py checks their
premises on the CPU: that each shape still reaches the launch edge, slab count, panel count or chunk count it was chosen for, that
the slab scratch of the step holds what its users write, and that the recorded round-off floors of the reference are reproduced.

Reference: oracle/kron.py (elbo_step_masked, elbo_step_scattered, q_v_masked, q_v_cov_masked, posterior_masked, posterior_cov_masked,
readout_masked, z_grad_scattered).

ELBO comparisons are made on the data-dependent part  ELBO - C0,  C0 = -(N log(2 pi sigma2) + yy / sigma2) / 2  (`c0`), as in
tests/paired_cases.py.  The gradient is compared PER COMPONENT (`rel_each`), each component relative to its own reference magnitude:
d/dsigma2 is ~1e3 times the lengthscale components, so one max-norm over the five lets a wrong d/dell through (`rel` is that
max-norm; the read-out arrays, whose entries are of one kind, keep it).

FLOORS[case][quantity]: the reference's own round-off, the larger of
    (1) oracle/kron.py against the dense restatement oracle/dense.py (DenseKron on the observed subset), where the number of
        observations is at most DENSE_MAX_N;
    (2) oracle/kron.py against its transposed twin: the dimensions exchanged, W^T, Y^T, theta permuted by mixed_dims_cases.SWAP, the
        results permuted back (scattered cases: the points in reverse order).  Every case.
The bound used on the GPU is `bound(case, quantity)` = max(100 FLOORS, 1e-12), never above CEIL (the path's existing tolerances); the
factor 100 is the margin of the exact-iterative and paired pins.  `PYTHONPATH=. python tests/masked_dense_cases.py` measures the
floors again and prints the table.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import mixed_dims_cases as MX
from oracle import dense as D
from oracle import kron as Kr

SWAP = MX.SWAP
THETA = (0.2, 0.3, 1.1, 0.8, 0.02)
DENSE_MAX_N = 3000
GRAD = ("g_l1", "g_l2", "g_s1", "g_s2", "g_v")
Q_STEP = ("elbo",) + GRAD
Q_QV = ("qv_mean", "qv_var")
Q_READ = Q_QV + ("qv_cov", "post_mean", "post_var", "post_cov", "ro_mean_lit", "ro_var_lit", "ro_mean_cond", "ro_var_cond")
Q_ZGRAD = ("zg1", "zg2")

M_E = 35                                   # the read-out states: m = (7, 5)
NS_POST = (1, M_E - 1, M_E, M_E + 1, 2 * M_E + 1)
NS_COV = (1, M_E)
MV = ((1, 1), (5, 7), (6, 6), (9, 8))      # ns = 1, M, M + 1 and above 2 M cells


def _cdiv(a, b):
    return (a + b - 1) // b


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def rel_each(a, b):
    """Per-component relative error of a gradient: |a_i - b_i| / |b_i|."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


def c0(N, yy, sigma2):
    return -(N * math.log(2.0 * math.pi * sigma2) + yy / sigma2) / 2.0


# ---- replica of the host decisions -------------------------------------------------------------------------------------------
# Mirrors, in csrc/masked.hip, csrc/masked_readout.hip and csrc/gemm.hip:  gemm_longk / vg_longk_slabs with vg_gemm_add's "drop empty
# splits",  the slab launch of vgm_colstats,  the panels of vg_blocked_chol_inverse,  the chunks of the read-outs,  vgm_layout's T.
VG_BK, VG_MB, ARENA = 16, 128, 32          # k-tile, Cholesky panel width, doubles per 256-byte arena step


def longk_slabs(K):
    """Slabs a long-K product of reduction length K writes (1: no split, no scratch)."""
    ks = min(K // 512, 256)
    if ks < 2:
        return 1
    ktiles = _cdiv(K, VG_BK)
    per = _cdiv(ktiles, ks)
    return _cdiv(ktiles, per)


def wcol_slabs(n2, m2):
    """-> (nslab, rows per slab, empty slabs) of vgm_wcol_part_kernel."""
    nslab = min(m2 * m2, 64)
    per = _cdiv(n2, nslab)
    return nslab, per, sum(1 for k in range(nslab) if k * per >= n2)


def chol_panels(M):
    return _cdiv(M, VG_MB)


def readout_chunks(ns, M):
    return _cdiv(ns, min(ns, M))


def scratch_users(n1, n2, m1, m2):
    """Doubles each user of the dense masked step's T buffer writes."""
    s1, s2 = longk_slabs(n1), longk_slabs(n2)
    return dict(assembly=n1 * m2 * m2, PT1=s1 * m1 * m1 if s1 > 1 else 0, PT2=s2 * m2 * m2 if s2 > 1 else 0,
                colstats=min(m2 * m2, 64) * n1)


def scratch_need(n1, n2, m1, m2):
    return max(scratch_users(n1, n2, m1, m2).values())


def parent_capacity(n1, n2, m1, m2):
    """What T held before it was sized for its users: the assembly's n1 x m2^2 alone."""
    return n1 * m2 * m2


def new_capacity(n1, n2, m1, m2):
    """vgm_layout: max over the assembly, the two long-K products (one slab counted where they do not split) and vgm_colstats."""
    return max(n1 * m2 * m2, longk_slabs(n1) * m1 * m1, longk_slabs(n2) * m2 * m2, min(m2 * m2, 64) * n1)


def _arena(n):
    return _cdiv(n, ARENA) * ARENA


def parent_room_to_Zb(n1, n2, m1, m2):
    """Doubles from the start of T to the start of Zb in the parent's arena: T, Tv, UB, UV, each on a 256-byte step."""
    return 2 * _arena(n1 * m2 * m2) + 2 * _arena(m1 * n2)


def masked_arena_growth_bytes(n1, n2, m1, m2):
    return 8 * (_arena(new_capacity(n1, n2, m1, m2)) - _arena(parent_capacity(n1, n2, m1, m2)))


# ---- case tables -------------------------------------------------------------------------------------------------------------
def _b0(m1, m2):
    return MX.b0(m1), MX.b0(m2)


def _masked(n1, n2, dims, mask=("bernoulli", 0.3, 1), theta=THETA, read=None, twin=False):
    return dict(layout="masked", n=(n1, n2), dims=dims, mask=mask, theta=tuple(theta), read=read, twin=twin)


def _scattered(N, dims, theta=THETA, read=None, points="unit", seed=11):
    return dict(layout="scattered", n=N, dims=dims, theta=tuple(theta), read=read, points=points, seed=seed, twin=False)


# A: grid shape of the masked step (n1, n2 | m1, m2); every case also as its transposed twin (name + "_T"): PT1 / wcol and PT2 / wrow
# are different code
A_SHAPES = (
    [(n1, 3, 5, 4) for n1 in (255, 256, 257)]                    # 1-D launches and the 256-stride of vgm_wrow_kernel
    + [(40, n2, 6, 8) for n2 in (1, 2, 63, 65)]                  # vgm_wcol_part: fewer rows than its 64 slabs, one short, one over
    + [(n1, 8, 6, 3) for n1 in (1023, 1024, 1535, 1536)]         # long-K threshold (1024) and the step from 2 to 3 slabs
    + [(1024, 32, 96, 2), (1024, 16, 48, 1), (3, 4096, 4, 16), (2, 2048, 4, 32)])     # slab scratch larger than the assembly's T
SLAB_SCRATCH = ("A_1024x32_96x2", "A_1024x16_48x1", "A_3x4096_4x16", "A_2x2048_4x32")
A_CASES = {}
for (_n1, _n2, _m1, _m2) in A_SHAPES:
    _name = f"A_{_n1}x{_n2}_{_m1}x{_m2}"
    A_CASES[_name] = _masked(_n1, _n2, _b0(_m1, _m2))
    A_CASES[_name + "_T"] = dict(A_CASES[_name], twin=True)

# B: masks on 40 x 36 | 7, 5
MASKS = ("ones", "one_cell", "empty_row", "empty_col", "single_row", "checker", "half_plane", "track", "few")
B_CASES = {f"B_{_k}": _masked(40, 36, _b0(7, 5), mask=(_k,)) for _k in MASKS}
B_CASES["B_bernoulli"] = _masked(40, 36, _b0(7, 5), read="all")           # the masked read-out state of E

# C: the blocked factor as the step wires it (log-det on stride M + 1, Sinv, both partial traces), grids 48 x 50
C_CASES = {
    "C_128": _masked(48, 50, _b0(8, 16), read="qv"),
    "C_129": _masked(48, 50, _b0(3, 43), read="qv"),
    "C_258": _masked(48, 50, _b0(6, 43), read="qv"),
    "C_129_pts32": _masked(48, 50, (MX.pts("matern32", 3), MX.pts("matern32", 43)), theta=(0.3, 0.04, 1.1, 0.8, 0.02), read="qv"),
}

# D: scattered step
D_N = (1, 2, 5, 255, 256, 257, 1023, 1024, 1536, 131072, 131584)          # the last two reach and pass the 256-slab cap
D_CASES = {f"D_{_N}": _scattered(_N, _b0(6, 3)) for _N in D_N}
D_CASES["D_1024_96x2"] = _scattered(1024, _b0(96, 2))
D_CASES["D_1024_2x96"] = _scattered(1024, _b0(2, 96))
D_CASES["D_dup_outside"] = _scattered(700, _b0(6, 3), points="dup_outside")
D_CASES["D_vff_b0"] = _scattered(700, (MX.vff(3), MX.b0(5)), read="qvcov")                       # e = (-1, +1)
D_CASES["D_pts_b1"] = _scattered(700, (MX.pts("matern12", 6), MX.b1(9)), read="qvcov")           # e = (+1, -1)

# E: read-outs from the masked state B_bernoulli and a scattered state, M = 35; the Z-gradient of the scattered step
E_CASES = {"E_scattered": _scattered(1536, _b0(7, 5), read="all")}
for _N in (1023, 1536):
    for _kind, _ell in (("matern32", (0.2, 0.3)), ("rbf", (0.12, 0.16))):
        E_CASES[f"E_zgrad_{_N}_{_kind}"] = _scattered(_N, (MX.irregular(_kind, 7, seed=3), MX.irregular(_kind, 5, seed=4)),
                                                      theta=_ell + THETA[2:], read="zgrad")
E_MASKED, E_SCATTERED = "B_bernoulli", "E_scattered"

CASES = {**A_CASES, **B_CASES, **C_CASES, **D_CASES, **E_CASES}

CEIL_MASKED = dict(elbo=1e-7, qv_mean=1e-7, qv_var=1e-7, post_mean=1e-7, post_var=1e-6, qv_cov=1e-7, post_cov=1e-6,
                   ro_mean_lit=1e-7, ro_var_lit=1e-6, ro_mean_cond=1e-7, ro_var_cond=1e-6, **{g: 1e-7 for g in GRAD})
CEIL_SCATTERED = dict(elbo=1e-7, **{g: 1e-7 for g in GRAD}, **{q: 1e-6 for q in Q_READ})


def ceil(name, q):
    """The path's existing tolerances: 1e-7 for ELBO, gradient, q(v) and posterior mean of the masked step, 1e-6 for its variances and
    for every scattered read-out; the Z-gradient 1e-6, with an RBF dimension 1e-4."""
    c = CASES[name]
    if q in Q_ZGRAD:
        return 1e-4 if "rbf" in (c["dims"][0].kind, c["dims"][1].kind) else 1e-6
    return (CEIL_MASKED if c["layout"] == "masked" else CEIL_SCATTERED)[q]


def quantities(name):
    c = CASES[name]
    return Q_STEP + {None: (), "qv": Q_QV, "qvcov": Q_QV + ("qv_cov",), "all": Q_READ, "zgrad": Q_ZGRAD}[c["read"]]


# ---- problems ----------------------------------------------------------------------------------------------------------------
def mask(kind, n1, n2):
    """W [n2, n1] of family B (and the Bernoulli mask of every other masked case)."""
    W = (np.random.default_rng(1).uniform(size=(n2, n1)) > 0.3).astype(np.float64)
    k = kind[0]
    if k == "bernoulli":
        return (np.random.default_rng(kind[2]).uniform(size=(n2, n1)) > kind[1]).astype(np.float64)
    if k == "ones":
        return np.ones((n2, n1))
    if k == "one_cell":
        W[:] = 0.0
        W[n2 // 2 - 1, n1 // 2 + 3] = 1.0
    elif k == "empty_row":
        W[5, :] = 0.0
    elif k == "empty_col":
        W[:, 7] = 0.0
    elif k == "single_row":
        W[:] = 0.0
        W[11, :] = 1.0
    elif k == "checker":
        W = ((np.arange(n2)[:, None] + np.arange(n1)[None, :]) % 2).astype(np.float64)
    elif k == "half_plane":
        W = ((np.arange(n2)[:, None] / n2 + np.arange(n1)[None, :] / n1) < 0.9).astype(np.float64)
    elif k == "track":
        from variational_gridded_gaussian_processes_amd import datagen
        W = datagen.track_mask(n1, n2, trajectory_gradient=2, track_sparsity=2.0)      # tracks 8 columns apart (the default 0.1
        # degrees of 10 is one track per 0.4 columns on 40 of them: every cell observed)
    elif k == "few":                                  # fewer observations than M = 35
        W[:] = 0.0
        W.reshape(-1)[np.random.default_rng(2).choice(n1 * n2, 20, replace=False)] = 1.0
    else:
        raise KeyError(k)
    return W


def _transpose(p):
    """The transposed twin of a masked problem: the same model, so the same ELBO, and the gradient permuted by SWAP."""
    return dict(p, d1=p["d2"], d2=p["d1"], x1=p["x2"], x2=p["x1"], n1=p["n2"], n2=p["n1"], Y=np.ascontiguousarray(p["Y"].T),
                W=np.ascontiguousarray(p["W"].T), theta=tuple(np.asarray(p["theta"])[SWAP]))


def _reverse(p):
    return dict(p, X=p["X"][::-1].copy(), y=p["y"][::-1].copy())


@functools.lru_cache(maxsize=None)
def case_problem(name):
    """masked: dict(d1, d2, x1, x2, n1, n2, Y [n2, n1], W [n2, n1], theta, N, yy);  scattered: dict(d1, d2, X [N, 2], y, theta, N, yy).
    Treat as read-only."""
    c = CASES[name]
    d1, d2 = c["dims"]
    if c["layout"] == "masked":
        n1, n2 = c["n"]
        _, y, x1, x2 = D.gen_grid(n1, n2)
        Y, W = y.reshape(n2, n1), mask(c["mask"], n1, n2)
        p = dict(layout="masked", d1=d1, d2=d2, x1=x1, x2=x2, n1=n1, n2=n2, Y=Y, W=W, theta=c["theta"], N=int(W.sum()),
                 yy=float(((Y * W) ** 2).sum()))
        return _transpose(p) if c["twin"] else p
    N = c["n"]
    rng = np.random.default_rng([c["seed"], N])
    X = rng.random((N, 2))
    if c["points"] == "dup_outside":                  # exact duplicates, and points on either side of the B0 mesh over [0, 1]
        X = -0.15 + 1.3 * X
        X[N // 2:N // 2 + 40] = X[:40]
        assert (X.min(0) < 0).all() and (X.max(0) > 1).all()
    y = D.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(N)
    return dict(layout="scattered", d1=d1, d2=d2, X=X, y=y, theta=c["theta"], N=N, yy=float(y @ y))


def factors(p):
    if p["layout"] == "masked":
        return MX.factor(p["d1"], p["x1"]), MX.factor(p["d2"], p["x2"])
    return MX.factor(p["d1"], np.zeros(1)), MX.factor(p["d2"], np.zeros(1))


def readout_inputs(seed=9):
    """-> xs [2 M + 1, 2], {(mv1, mv2): (C1 [mv1, 7], C2 [mv2, 5], kd1 [mv1], kd2 [mv2])}: any matrices serve the C entry."""
    rng = np.random.default_rng([seed, M_E])
    xs = rng.random((max(NS_POST), 2))
    mats = {}
    for mv1, mv2 in MV:
        mats[(mv1, mv2)] = (rng.random((mv1, 7)), rng.random((mv2, 5)), 0.5 + rng.random(mv1), 0.5 + rng.random(mv2))
    return xs, mats


# ---- reference ---------------------------------------------------------------------------------------------------------------
def _step(p):
    f1, f2 = factors(p)
    if p["layout"] == "masked":
        return Kr.elbo_step_masked(p["Y"], p["W"], f1, f2, p["theta"]), f1, f2
    return Kr.elbo_step_scattered(p["X"], p["y"], f1, f2, p["theta"]), f1, f2


def _evaluate(p, read, swapped=False):
    """Every quantity of a case from oracle/kron.py -> flat dict.  swapped: p is a transposed twin; the results are permuted back."""
    st, f1, f2 = _step(p)
    g = st.grad[SWAP] if swapped else st.grad
    out = dict(elbo=st.elbo - c0(p["N"], p["yy"], p["theta"][4]), grad=np.array(g), **{k: float(v) for k, v in zip(GRAD, g)})
    T = (lambda a: np.ascontiguousarray(np.asarray(a).T)) if swapped else (lambda a: np.asarray(a))
    if read in ("qv", "qvcov", "all"):
        m, v = Kr.q_v_masked(st, f1, f2)
        out["qv_mean"], out["qv_var"] = T(m), T(v)
    if read in ("qvcov", "all"):
        cov = Kr.q_v_cov_masked(st, f1, f2)
        if swapped:                                   # rows / columns (i2, i1) -> (i1, i2)
            ma, mb = f1.m, f2.m
            cov = cov.reshape(ma, mb, ma, mb).transpose(1, 0, 3, 2).reshape(ma * mb, ma * mb)
        out["qv_cov"] = cov
    if read == "all":
        xs, mats = readout_inputs()
        xq = xs[:, ::-1].copy() if swapped else xs
        out["post_mean"], out["post_var"] = Kr.posterior_masked(st, f1, f2, xq)
        out["post_cov"] = Kr.posterior_cov_masked(st, f1, f2, xq[:max(NS_COV)])
        for (mv1, mv2), (C1, C2, kd1, kd2) in mats.items():
            for literal in (True, False):
                a = (C2, C1, kd2, kd1) if swapped else (C1, C2, kd1, kd2)
                m, v = Kr.readout_masked(st, *a, literal=literal)
                tag = "lit" if literal else "cond"
                out[f"ro_mean_{tag}_{mv1}x{mv2}"], out[f"ro_var_{tag}_{mv1}x{mv2}"] = T(m), T(v)
    if read == "zgrad":
        out["zg1"], out["zg2"] = Kr.z_grad_scattered(st, p["X"], p["y"], f1, f2)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference of a case, computed once and shared by the tests (treat as read-only)."""
    return _evaluate(case_problem(name), CASES[name]["read"])


def compare(name, got, want, q):
    """The error measure of quantity q between two evaluations: per-component for the gradient (its own key each), max-norm relative
    for the ELBO part and the read-out arrays (the worst over the sizes the GPU tests use)."""
    if q in ("ro_mean_lit", "ro_var_lit", "ro_mean_cond", "ro_var_cond"):
        return max(rel(got[f"{q}_{a}x{b}"], want[f"{q}_{a}x{b}"]) for a, b in MV)
    if q in GRAD or q == "elbo":
        return float(rel_each(got[q], want[q]))
    return rel(got[q], want[q])


def _dense_evaluate(name, p):
    """The dense restatement on the observed subset -> the quantities it has (raw-gradient components are the theta-gradient's times
    one positive factor each, so their relative errors are the same)."""
    c = CASES[name]
    theta = np.asarray(p["theta"], float)
    if p["layout"] == "masked":
        X1, X2 = np.meshgrid(p["x1"], p["x2"])
        X, y, m = np.vstack([X1.ravel(), X2.ravel()]).T, p["Y"].reshape(-1), p["W"].reshape(-1) > 0
    else:
        X, y, m = p["X"], p["y"], None
    dm = MX.dense(X, y, p["d1"], p["d2"], theta, mask=m)
    e, g = dm.elbo_and_grad()
    g = g.numpy() / (Kr.grad_raw(np.ones(5), D.raw_from_constrained(theta).numpy()))
    out = dict(elbo=e.item() - c0(p["N"], p["yy"], theta[4]), **{k: float(v) for k, v in zip(GRAD, g)})
    if c["read"] in ("qv", "qvcov", "all"):
        with torch.no_grad():
            q = dm.q_v()
            out["qv_mean"], out["qv_var"] = q.mean.numpy(), q.variance.numpy()
            if c["read"] != "qv":
                out["qv_cov"] = q.covariance_matrix.numpy()
            if c["read"] == "all":
                xs, _ = readout_inputs()
                po = dm.posterior(xs)
                out["post_mean"], out["post_var"] = po.mean.numpy(), po.variance.numpy()
                out["post_cov"] = dm.posterior(xs[:max(NS_COV)]).covariance_matrix.numpy()
    return out


def measure_floors(name):
    """FLOORS[name], measured again (CPU; on one thread, so that the BLAS summation order -- and with it the measured round-off -- does
    not depend on the number of cores)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _measure_floors(name)
    finally:
        torch.set_num_threads(n)


def _measure_floors(name):
    c, p, ref = CASES[name], case_problem(name), reference(name)
    if c["layout"] == "masked":
        # (a twin case's twin is its base case: the same pair of evaluations gives both floors)
        other = name[:-2] if c["twin"] else name + "_T"
        twin = reference(other) if other in CASES else _evaluate(_transpose(p), c["read"], swapped=True)
        if other in CASES:
            twin = dict(twin, **{k: float(v) for k, v in zip(GRAD, twin["grad"][SWAP])})
    else:
        twin = _evaluate(_reverse(p), c["read"])
    f = {q: compare(name, twin, ref, q) for q in quantities(name)}
    if p["N"] <= DENSE_MAX_N:
        dn = _dense_evaluate(name, p)
        for q in f:
            if q in dn:
                a, b = np.asarray(dn[q], float).reshape(-1), np.asarray(ref[q], float).reshape(-1)
                f[q] = max(f[q], float(rel_each(a[0], b[0])) if a.size == 1 else rel(a, b))
    return f


def bound(name, q):
    """The GPU tests' bound: 100 times the reference's floor, at least 1e-12, at most the path's ceiling."""
    return min(max(100.0 * FLOORS[name][q], 1e-12), ceil(name, q))


# measured by this file's __main__ (one thread)
FLOORS = {
    "A_255x3_5x4": {"elbo": 1.9e-14, "g_l1": 4.9e-13, "g_l2": 4.7e-13, "g_s1": 1.4e-15, "g_s2": 1.4e-15, "g_v": 9.7e-14},
    "A_255x3_5x4_T": {"elbo": 1.9e-14, "g_l1": 4.7e-13, "g_l2": 4.9e-13, "g_s1": 2.2e-15, "g_s2": 2.5e-15, "g_v": 9.7e-14},
    "A_256x3_5x4": {"elbo": 3.7e-14, "g_l1": 8.2e-13, "g_l2": 7.5e-13, "g_s1": 2.9e-15, "g_s2": 2.3e-15, "g_v": 1.9e-13},
    "A_256x3_5x4_T": {"elbo": 3.7e-14, "g_l1": 7.5e-13, "g_l2": 8.2e-13, "g_s1": 1.7e-15, "g_s2": 2.0e-15, "g_v": 1.9e-13},
    "A_257x3_5x4": {"elbo": 1.3e-14, "g_l1": 3.6e-13, "g_l2": 9.4e-14, "g_s1": 1.6e-15, "g_s2": 1.8e-15, "g_v": 6.8e-14},
    "A_257x3_5x4_T": {"elbo": 1.3e-14, "g_l1": 5.3e-14, "g_l2": 3.6e-13, "g_s1": 3.5e-15, "g_s2": 3.2e-15, "g_v": 6.8e-14},
    "A_40x1_6x8": {"elbo": 2.5e-15, "g_l1": 8.8e-14, "g_l2": 1.8e-14, "g_s1": 2.0e-15, "g_s2": 2.0e-15, "g_v": 2.5e-14},
    "A_40x1_6x8_T": {"elbo": 3.3e-15, "g_l1": 1.8e-14, "g_l2": 1.4e-13, "g_s1": 2.2e-15, "g_s2": 2.0e-15, "g_v": 3.8e-14},
    "A_40x2_6x8": {"elbo": 1.8e-15, "g_l1": 6.1e-14, "g_l2": 2.1e-14, "g_s1": 4.2e-16, "g_s2": 1.8e-15, "g_v": 1.7e-14},
    "A_40x2_6x8_T": {"elbo": 3.3e-15, "g_l1": 2.1e-14, "g_l2": 1.0e-13, "g_s1": 8.1e-16, "g_s2": 5.6e-16, "g_v": 3.1e-14},
    "A_40x63_6x8": {"elbo": 3.5e-16, "g_l1": 3.3e-15, "g_l2": 3.5e-14, "g_s1": 8.0e-15, "g_s2": 1.0e-14, "g_v": 1.5e-15},
    "A_40x63_6x8_T": {"elbo": 1.7e-15, "g_l1": 6.9e-15, "g_l2": 3.3e-15, "g_s1": 3.7e-15, "g_s2": 3.3e-15, "g_v": 6.9e-15},
    "A_40x65_6x8": {"elbo": 1.0e-15, "g_l1": 1.1e-15, "g_l2": 1.5e-14, "g_s1": 4.7e-15, "g_s2": 5.3e-15, "g_v": 4.1e-15},
    "A_40x65_6x8_T": {"elbo": 6.7e-16, "g_l1": 2.1e-15, "g_l2": 8.8e-15, "g_s1": 4.9e-15, "g_s2": 6.2e-15, "g_v": 2.9e-15},
    "A_1023x8_6x3": {"elbo": 5.2e-16, "g_l1": 5.3e-15, "g_l2": 1.9e-15, "g_s1": 3.1e-16, "g_s2": 0.0e+00, "g_v": 3.5e-16},
    "A_1023x8_6x3_T": {"elbo": 5.2e-16, "g_l1": 1.9e-15, "g_l2": 5.3e-15, "g_s1": 0.0e+00, "g_s2": 3.1e-16, "g_v": 3.5e-16},
    "A_1024x8_6x3": {"elbo": 2.6e-16, "g_l1": 1.3e-14, "g_l2": 1.6e-15, "g_s1": 1.2e-15, "g_s2": 1.3e-15, "g_v": 3.5e-16},
    "A_1024x8_6x3_T": {"elbo": 2.6e-16, "g_l1": 1.6e-15, "g_l2": 1.3e-14, "g_s1": 1.3e-15, "g_s2": 1.2e-15, "g_v": 3.5e-16},
    "A_1535x8_6x3": {"elbo": 1.4e-15, "g_l1": 3.6e-14, "g_l2": 9.8e-15, "g_s1": 4.1e-16, "g_s2": 3.0e-16, "g_v": 1.4e-15},
    "A_1535x8_6x3_T": {"elbo": 1.4e-15, "g_l1": 9.8e-15, "g_l2": 3.6e-14, "g_s1": 3.0e-16, "g_s2": 4.1e-16, "g_v": 1.4e-15},
    "A_1536x8_6x3": {"elbo": 1.8e-16, "g_l1": 6.7e-15, "g_l2": 1.9e-15, "g_s1": 6.1e-16, "g_s2": 5.9e-16, "g_v": 2.3e-16},
    "A_1536x8_6x3_T": {"elbo": 1.8e-16, "g_l1": 1.9e-15, "g_l2": 6.7e-15, "g_s1": 5.9e-16, "g_s2": 6.1e-16, "g_v": 2.3e-16},
    "A_1024x32_96x2": {"elbo": 1.3e-15, "g_l1": 5.0e-13, "g_l2": 2.6e-15, "g_s1": 3.5e-16, "g_s2": 3.8e-16, "g_v": 8.0e-16},
    "A_1024x32_96x2_T": {"elbo": 1.3e-15, "g_l1": 2.6e-15, "g_l2": 5.0e-13, "g_s1": 3.8e-16, "g_s2": 3.5e-16, "g_v": 8.0e-16},
    "A_1024x16_48x1": {"elbo": 6.4e-15, "g_l1": 8.3e-14, "g_l2": 5.7e-16, "g_s1": 0.0e+00, "g_s2": 1.6e-16, "g_v": 4.1e-16},
    "A_1024x16_48x1_T": {"elbo": 6.4e-15, "g_l1": 5.7e-16, "g_l2": 8.3e-14, "g_s1": 1.6e-16, "g_s2": 0.0e+00, "g_v": 4.1e-16},
    "A_3x4096_4x16": {"elbo": 2.8e-13, "g_l1": 8.3e-13, "g_l2": 6.8e-12, "g_s1": 0.0e+00, "g_s2": 1.3e-16, "g_v": 4.0e-13},
    "A_3x4096_4x16_T": {"elbo": 2.8e-13, "g_l1": 6.8e-12, "g_l2": 8.3e-13, "g_s1": 1.3e-16, "g_s2": 0.0e+00, "g_v": 4.0e-13},
    "A_2x2048_4x32": {"elbo": 4.0e-14, "g_l1": 2.0e-14, "g_l2": 8.0e-13, "g_s1": 7.8e-15, "g_s2": 8.3e-15, "g_v": 1.9e-14},
    "A_2x2048_4x32_T": {"elbo": 4.0e-14, "g_l1": 8.0e-13, "g_l2": 2.6e-14, "g_s1": 8.1e-15, "g_s2": 6.9e-15, "g_v": 1.9e-14},
    "B_ones": {"elbo": 2.2e-15, "g_l1": 2.1e-14, "g_l2": 4.7e-15, "g_s1": 1.9e-15, "g_s2": 1.7e-15, "g_v": 7.9e-15},
    "B_one_cell": {"elbo": 3.0e-15, "g_l1": 4.3e-16, "g_l2": 2.0e-14, "g_s1": 2.9e-15, "g_s2": 3.1e-15, "g_v": 4.3e-15},
    "B_empty_row": {"elbo": 1.5e-15, "g_l1": 5.4e-15, "g_l2": 4.0e-15, "g_s1": 1.6e-15, "g_s2": 1.3e-15, "g_v": 6.0e-15},
    "B_empty_col": {"elbo": 7.7e-16, "g_l1": 2.2e-14, "g_l2": 1.1e-14, "g_s1": 8.0e-15, "g_s2": 6.0e-15, "g_v": 2.7e-15},
    "B_single_row": {"elbo": 2.4e-15, "g_l1": 1.9e-14, "g_l2": 2.5e-14, "g_s1": 7.0e-15, "g_s2": 6.0e-15, "g_v": 1.3e-14},
    "B_checker": {"elbo": 6.5e-16, "g_l1": 1.4e-14, "g_l2": 5.1e-15, "g_s1": 2.8e-15, "g_s2": 3.0e-15, "g_v": 2.0e-15},
    "B_half_plane": {"elbo": 1.2e-15, "g_l1": 2.7e-14, "g_l2": 1.7e-14, "g_s1": 8.5e-15, "g_s2": 9.2e-15, "g_v": 5.5e-15},
    "B_track": {"elbo": 1.2e-15, "g_l1": 6.0e-15, "g_l2": 1.2e-14, "g_s1": 2.4e-15, "g_s2": 3.4e-15, "g_v": 2.7e-15},
    "B_few": {"elbo": 6.9e-16, "g_l1": 2.7e-15, "g_l2": 1.3e-14, "g_s1": 3.5e-15, "g_s2": 3.6e-15, "g_v": 2.0e-15},
    "B_bernoulli": {"elbo": 1.2e-15, "g_l1": 3.8e-15, "g_l2": 5.0e-15, "g_s1": 4.3e-15, "g_s2": 4.8e-15, "g_v": 6.1e-15, "qv_mean": 2.2e-14, "qv_var": 1.3e-13, "qv_cov": 1.3e-13, "post_mean": 3.1e-14, "post_var": 5.5e-15, "post_cov": 4.7e-15, "ro_mean_lit": 6.6e-15, "ro_var_lit": 1.4e-15, "ro_mean_cond": 6.6e-15, "ro_var_cond": 5.9e-16},
    "C_128": {"elbo": 1.6e-15, "g_l1": 8.9e-15, "g_l2": 4.7e-14, "g_s1": 2.2e-15, "g_s2": 2.6e-15, "g_v": 1.3e-14, "qv_mean": 5.0e-13, "qv_var": 1.5e-11},
    "C_129": {"elbo": 8.6e-15, "g_l1": 1.5e-14, "g_l2": 4.9e-13, "g_s1": 1.1e-14, "g_s2": 1.2e-14, "g_v": 1.9e-14, "qv_mean": 2.1e-12, "qv_var": 9.7e-12},
    "C_258": {"elbo": 1.3e-15, "g_l1": 1.2e-14, "g_l2": 6.4e-13, "g_s1": 2.5e-14, "g_s2": 2.3e-14, "g_v": 8.9e-15, "qv_mean": 1.1e-11, "qv_var": 1.4e-10},
    "C_129_pts32": {"elbo": 1.2e-15, "g_l1": 1.1e-15, "g_l2": 5.1e-14, "g_s1": 2.1e-15, "g_s2": 7.7e-16, "g_v": 2.5e-15, "qv_mean": 4.5e-14, "qv_var": 3.2e-13},
    "D_1": {"elbo": 1.1e-15, "g_l1": 1.5e-15, "g_l2": 3.2e-15, "g_s1": 1.4e-15, "g_s2": 1.5e-15, "g_v": 7.6e-15},
    "D_2": {"elbo": 1.8e-15, "g_l1": 1.7e-14, "g_l2": 6.8e-15, "g_s1": 1.2e-15, "g_s2": 1.2e-15, "g_v": 7.7e-15},
    "D_5": {"elbo": 1.4e-16, "g_l1": 2.8e-15, "g_l2": 4.1e-15, "g_s1": 8.1e-16, "g_s2": 8.4e-16, "g_v": 8.4e-16},
    "D_255": {"elbo": 1.7e-15, "g_l1": 4.9e-15, "g_l2": 2.0e-15, "g_s1": 1.5e-15, "g_s2": 2.6e-15, "g_v": 3.2e-15},
    "D_256": {"elbo": 3.6e-15, "g_l1": 9.8e-15, "g_l2": 5.2e-15, "g_s1": 5.6e-15, "g_s2": 6.1e-15, "g_v": 9.2e-15},
    "D_257": {"elbo": 8.1e-16, "g_l1": 1.0e-14, "g_l2": 1.5e-15, "g_s1": 4.5e-15, "g_s2": 4.5e-15, "g_v": 1.2e-15},
    "D_1023": {"elbo": 7.3e-16, "g_l1": 6.8e-15, "g_l2": 4.9e-15, "g_s1": 4.4e-15, "g_s2": 4.9e-15, "g_v": 6.0e-16},
    "D_1024": {"elbo": 2.0e-15, "g_l1": 3.7e-15, "g_l2": 5.5e-15, "g_s1": 2.0e-15, "g_s2": 2.7e-15, "g_v": 1.5e-15},
    "D_1536": {"elbo": 3.8e-15, "g_l1": 8.4e-15, "g_l2": 8.9e-15, "g_s1": 5.1e-15, "g_s2": 5.4e-15, "g_v": 8.1e-15},
    "D_131072": {"elbo": 3.2e-15, "g_l1": 3.5e-15, "g_l2": 8.3e-16, "g_s1": 5.8e-16, "g_s2": 5.0e-16, "g_v": 3.3e-15},
    "D_131584": {"elbo": 1.5e-15, "g_l1": 2.8e-15, "g_l2": 2.5e-15, "g_s1": 5.8e-16, "g_s2": 5.0e-16, "g_v": 1.5e-15},
    "D_1024_96x2": {"elbo": 4.6e-13, "g_l1": 5.6e-11, "g_l2": 7.9e-14, "g_s1": 5.6e-14, "g_s2": 6.1e-14, "g_v": 1.9e-13},
    "D_1024_2x96": {"elbo": 1.9e-13, "g_l1": 2.4e-14, "g_l2": 2.9e-10, "g_s1": 9.2e-14, "g_s2": 9.2e-14, "g_v": 1.8e-13},
    "D_dup_outside": {"elbo": 2.6e-15, "g_l1": 2.4e-14, "g_l2": 7.4e-15, "g_s1": 3.6e-15, "g_s2": 3.2e-15, "g_v": 1.5e-15},
    "D_vff_b0": {"elbo": 2.2e-15, "g_l1": 5.3e-15, "g_l2": 2.5e-14, "g_s1": 2.0e-15, "g_s2": 1.6e-15, "g_v": 9.8e-15, "qv_mean": 3.6e-14, "qv_var": 1.7e-14, "qv_cov": 1.6e-14},
    "D_pts_b1": {"elbo": 2.3e-14, "g_l1": 1.8e-14, "g_l2": 1.1e-12, "g_s1": 3.6e-14, "g_s2": 2.8e-14, "g_v": 5.2e-14, "qv_mean": 2.0e-13, "qv_var": 3.6e-13, "qv_cov": 3.6e-13},
    "E_scattered": {"elbo": 2.0e-16, "g_l1": 1.4e-14, "g_l2": 6.3e-15, "g_s1": 2.1e-15, "g_s2": 2.0e-15, "g_v": 1.0e-15, "qv_mean": 2.5e-14, "qv_var": 8.4e-14, "qv_cov": 8.4e-14, "post_mean": 3.1e-14, "post_var": 5.5e-15, "post_cov": 4.6e-15, "ro_mean_lit": 1.5e-14, "ro_var_lit": 5.7e-16, "ro_mean_cond": 1.5e-14, "ro_var_cond": 9.8e-17},
    "E_zgrad_1023_matern32": {"elbo": 2.0e-15, "g_l1": 1.6e-14, "g_l2": 1.7e-14, "g_s1": 7.0e-15, "g_s2": 7.4e-15, "g_v": 6.2e-15, "zg1": 1.2e-13, "zg2": 9.4e-15},
    "E_zgrad_1023_rbf": {"elbo": 5.9e-15, "g_l1": 5.7e-14, "g_l2": 3.3e-14, "g_s1": 1.4e-13, "g_s2": 1.2e-13, "g_v": 5.5e-15, "zg1": 2.7e-14, "zg2": 3.2e-15},
    "E_zgrad_1536_matern32": {"elbo": 2.0e-15, "g_l1": 7.3e-15, "g_l2": 1.1e-14, "g_s1": 3.4e-14, "g_s2": 3.9e-14, "g_v": 1.2e-14, "zg1": 8.7e-14, "zg2": 9.4e-15},
    "E_zgrad_1536_rbf": {"elbo": 5.7e-15, "g_l1": 3.6e-14, "g_l2": 2.1e-14, "g_s1": 1.2e-13, "g_s2": 9.8e-14, "g_v": 1.8e-14, "zg1": 5.1e-14, "zg2": 4.5e-15},
}


if __name__ == "__main__":
    import sys
    import time
    print("FLOORS = {")
    for _name in (sys.argv[1:] or CASES):
        _t = time.time()
        _f = measure_floors(_name)
        print(f'    "{_name}": {{' + ", ".join(f'"{k}": {v:.1e}' for k, v in _f.items()) + f"}},   # {time.time() - _t:.1f} s", flush=True)
    print("}")
