"""Joint samples of posterior(x*) on a raster on the GPU: vggp_raster_sample_contract on every tile edge (integer-exact), and
vggp_posterior_raster_sample / _masked_iter / _scattered_iter against tests/raster_sample_spec.py, the dense GPU covariances, the dense
oracles, the samplers of q(v), and through the models.

Bounds (none of them comes from what the code gives):
    kernel edges                    equality: small-integer data, every product and partial sum is an integer far below 2^53
    covariance by unit noise        1e-7 relative, the project's read-out bound (test_*_covariance_by_unit_noise of test_gpu_qv_sample.py)
    same noise against the spec     1e-9, the bound of test_*_same_noise_vs_spec there (the residual roots of these B0 problems have
                                    condition numbers <= 200)
    seed path / grouping            the seed path is the explicit path (same numbers, same launches: equality); sample 5 of a seed drawn
                                    alone against row 5 of 70: 1e-12, the full-grid bound of vggp_qv_sample (another block width
                                    reorders GEMM tiles)
    one joint draw with q(v)        1e-7 (read-out bound)
    first Cholesky columns          1e-9
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import masked_iter_readout_spec as MS
import qv_sample_cases as Cs
import qv_sample_spec as S
import raster_sample_spec as R
import scattered_iter_variance_spec as SS
from oracle import kron as Kr
from test_gpu_qv_sample import (G1, G2, GN1, GN2, SN, code_of, dev, grid40, host, plan24, points1500, step_grid40, step_masked_iter,
                                step_points1500)
from variational_gridded_gaussian_processes_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
rel = Cs.rel
EINVAL, ESTATE = _lib.VGGP_EINVAL, _lib.VGGP_ESTATE

# the 7 x 5 raster of tests/test_raster_sample_spec.py: aligned with nothing
A1 = np.array([0.013, 0.171, 0.3337, 0.52, 0.649, 0.803, 0.987])
A2 = np.array([0.041, 0.29, 0.4777, 0.71, 0.962])
# the 37 x 29 raster of the same-noise tests
B1AX, B2AX = np.linspace(0.013, 0.987, 37), np.linspace(0.013, 0.987, 29)


# ---- 1. the kernel on its own: every edge, integer-exact ---------------------------------------------------------------------------------
SENTINEL = -777.25
BAND = 193
PS = [1, 63, 64, 65, 130]


def guarded_in(X, fill=float("nan")):
    parent = torch.full((X.numel() + 2 * 37,), fill, dtype=torch.float64, device=DEV)
    view = parent[37:37 + X.numel()].view(*X.shape)
    view.copy_(X)
    return view


def guarded_out(*shape):
    n = int(np.prod(shape))
    parent = torch.full((n + 2 * BAND,), SENTINEL, dtype=torch.float64, device=DEV)
    return parent, parent[BAND:BAND + n].view(*shape)


@pytest.mark.parametrize("q", [1, 3, 4, 5, 20])
def test_contract_kernel_is_exact_on_every_edge(engine, q):
    """out = mean + B1^T Wt[s] + c tril(C1) Tt[s] with NaN above the diagonal of C1, NaN around every operand and sentinel bands around
    the output.  The variants (mean or NULL, c = 2, -1, 0) rotate over the shapes so that each meets every kind of edge."""
    k = 0
    for P1 in PS:
        for P2 in PS:
            for S_ in (1, 3):
                variant = k % 3
                k += 1
                g = torch.Generator(device="cpu").manual_seed(100000 * q + 1000 * P1 + 10 * P2 + S_)
                B1 = torch.randint(-4, 5, (q, P1), generator=g)
                Wt = torch.randint(-4, 5, (S_, q, P2), generator=g)
                C1 = torch.tril(torch.randint(-3, 4, (P1, P1), generator=g))
                Tt = torch.randint(-4, 5, (S_, P1, P2), generator=g)
                mean = torch.randint(-50, 51, (P1, P2), generator=g)
                c = (2.0, -1.0, 0.0)[variant]
                with_mean = variant != 1
                ref = torch.einsum("ia,sib->sab", B1, Wt) + int(c) * torch.einsum("ak,skb->sab", C1, Tt)
                if with_mean:
                    ref = ref + mean[None]
                c1 = C1.double()
                c1[torch.triu(torch.ones(P1, P1, dtype=torch.bool), diagonal=1)] = float("nan")
                parent, out = guarded_out(S_, P1, P2)
                engine.raster_sample_contract(guarded_in(B1.double()), guarded_in(Wt.double()), guarded_in(c1), guarded_in(Tt.double()), c,
                                              guarded_in(mean.double()) if with_mean else None, out=out)
                what = (q, P1, P2, S_, c, with_mean)
                assert torch.equal(out.cpu(), ref.double()), (what, int((out.cpu() != ref.double()).sum()))
                assert bool((parent[:BAND] == SENTINEL).all()) and bool((parent[-BAND:] == SENTINEL).all()), what


def test_contract_refuses_bad_arguments(engine):
    t = torch.zeros(4, 4, dtype=torch.float64, device=DEV)
    t3 = torch.zeros(1, 4, 4, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda x: x.data_ptr()
    lib, h = engine.lib, engine._h
    for args in ((None, p(t3), p(t), p(t3), 1, 4, 4, 4, 1.0, None, p(t3)), (p(t), p(t3), p(t), p(t3), 1, 4, 4, 4, 1.0, None, None),
                 (p(t), p(t3), p(t), p(t3), 0, 4, 4, 4, 1.0, None, p(t3)), (p(t), p(t3), p(t), p(t3), 1, 0, 4, 4, 1.0, None, p(t3)),
                 (p(t), p(t3), p(t), p(t3), 1, 4, 4, 2**20 + 1, 1.0, None, p(t3)), (p(t), p(t3), p(t), p(t3), 65536, 4, 4, 4, 1.0, None, p(t3))):
        assert lib.vggp_raster_sample_contract(h, *args, st) == EINVAL, args


# ---- 2. covariance by unit noise on the M = 24 problems ------------------------------------------------------------------------------------
def unit_noise(m1, m2, p1, p2, obs_shape=None):
    """Unit columns over E, (F,) G, H and one column of zeros -> dict of explicit noise arrays."""
    nE, nG, nH = m1 * m2, p1 * p2, m1 * p2
    nF = int(np.prod(obs_shape)) if obs_shape else 0
    S_ = nE + nF + nG + nH + 1
    out, off = {}, 0
    for key, n, shape in (("eps_u", nE, (m1, m2)), ("eps_obs", nF, obs_shape), ("eps_g", nG, (p1, p2)), ("eps_h", nH, (m1, p2))):
        if n == 0:
            continue
        a = np.zeros((S_, n))
        a[off + np.arange(n), np.arange(n)] = 1.0
        out[key] = dev(a.reshape((S_,) + tuple(shape)))
        off += n
    return S_, out


def dense_cov_masked(engine, xs, M):
    """engine.posterior_cov(xs, masked=True) for more points than the M per call the dense states take: a covariance cannot be chunked over
    its points, but every PAIR of points lies in the union of two of three groups of <= M / 2 points -- three calls fill the matrix."""
    ns = len(xs)
    if ns <= M:
        return host(engine.posterior_cov(dev(xs), masked=True))
    groups = np.array_split(np.arange(ns), 3)
    assert all(len(g) <= M // 2 for g in groups)
    cov = np.full((ns, ns), np.nan)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        idx = np.concatenate([groups[i], groups[j]])
        cov[np.ix_(idx, idx)] = host(engine.posterior_cov(dev(xs[idx]), masked=True))
    assert np.isfinite(cov).all()
    return cov


def judge_cov(tag, F, mu, cov_gpu, cov_or, nug):
    got = Cs.outer_sum(F, mu)
    e_gpu, e_or = rel(got, cov_gpu + nug), rel(got, cov_or + nug)
    print(f"{tag}: {F.shape[0]} unit samples vs the GPU's dense covariance + nugget {e_gpu:.1e}, vs the oracle {e_or:.1e} "
          f"(the nugget terms alone: {rel(cov_or + nug, cov_or):.1e})")
    assert e_gpu <= 1e-7 and e_or <= 1e-7


@pytest.mark.parametrize("case", Cs.KERNEL_BASES)
def test_full_grid_covariance_by_unit_noise(engine, case):
    p = plan24(engine, case)
    f1, f2 = Cs.factors(case, p["x1"], p["x2"])
    engine.elbo_step(p["Y"], p["yy_full"], Cs.THETA)
    S_, noise = unit_noise(f1.m, f2.m, len(A1), len(A2))
    mu, _ = engine.posterior_raster(dev(A1), dev(A2), want_var=False)
    F, info = engine.posterior_raster_sample(A1, A2, S_, **noise)
    assert torch.equal(F[-1], mu) and info["jitter"] == (0.0, 0.0)                  # zero noise: the raster mean, bit for bit
    xs = R.cartesian(A1, A2)
    st = Kr.elbo_step(p["Yn"], f1, f2, Cs.THETA)
    nug = R.nugget_terms(R.axes_full(st, f1, f2, A1, A2), Cs.THETA)
    judge_cov(f"{case} full grid", host(F[:-1]), host(mu), host(engine.posterior_cov(dev(xs))), Kr.posterior_cov(st, f1, f2, xs), nug)


@pytest.mark.parametrize("case", Cs.KERNEL_BASES)
def test_masked_covariance_by_unit_noise(engine, case):
    p = plan24(engine, case)
    f1, f2 = Cs.factors(case, p["x1"], p["x2"])
    xs = R.cartesian(A1, A2)
    engine.elbo_step_masked(p["Ym"], p["W"], p["nobs"], p["yy"], Cs.THETA)
    cov_gpu = dense_cov_masked(engine, xs, f1.m * f2.m)
    cov_or = Kr.posterior_cov_masked(Kr.elbo_step_masked(p["Yn"], p["Wn"], f1, f2, Cs.THETA), f1, f2, xs)
    step_masked_iter(engine, p)
    S_, noise = unit_noise(f1.m, f2.m, len(A1), len(A2), (Cs.N2, Cs.N1))
    mu, _ = engine.posterior_raster(dev(A1), dev(A2), want_var=False)
    F, info = engine.posterior_raster_sample_masked_iter(A1, A2, p["W"], p["nobs"], S_, **noise)
    assert torch.equal(F[-1], mu) and info["jitter"] == (0.0, 0.0)
    assert info["sweeps"][0] == -(-S_ // 64) and 0 < info["rounds"][0] < 40
    st = MS.prepare(p["Yn"], p["Wn"], f1, f2, Cs.THETA)
    nug = R.nugget_terms(R.axes(f1, f2, st.d1.L, st.d2.L, Cs.THETA, A1, A2), Cs.THETA)
    judge_cov(f"{case} masked", host(F[:-1]), host(mu), cov_gpu, cov_or, nug)


@pytest.mark.parametrize("case", Cs.KERNEL_BASES)
def test_scattered_covariance_by_unit_noise(engine, case):
    p = plan24(engine, case, scattered=True)
    X = p["X"]
    f1, f2 = Cs.factors(case, X[:, 0], X[:, 1])
    xs = R.cartesian(A1, A2)
    engine.elbo_step_scattered(p["y"], p["yy"], Cs.THETA)
    cov_gpu = dense_cov_masked(engine, xs, f1.m * f2.m)
    cov_or = Kr.posterior_cov_masked(Kr.elbo_step_scattered(X, p["yn"], f1, f2, Cs.THETA), f1, f2, xs)
    engine.elbo_step_scattered_iter(p["y"], p["yy"], Cs.THETA)
    S_, noise = unit_noise(f1.m, f2.m, len(A1), len(A2), (Cs.NPTS,))
    mu, _ = engine.posterior_raster(dev(A1), dev(A2), want_var=False)
    F, info = engine.posterior_raster_sample_scattered_iter(A1, A2, S_, **noise)
    assert torch.equal(F[-1], mu) and info["jitter"] == (0.0, 0.0) and info["sweeps"][0] == -(-S_ // 64)
    st = SS.prepare(X, p["yn"], f1, f2, Cs.THETA)
    nug = R.nugget_terms(R.axes(f1, f2, st.d1.L, st.d2.L, Cs.THETA, A1, A2), Cs.THETA)
    judge_cov(f"{case} scattered", host(F[:-1]), host(mu), cov_gpu, cov_or, nug)


# ---- 3. the same noise against the numpy specification: 20 x 12 B0 features, a 37 x 29 raster -------------------------------------------------
def random_noise(S_, obs_shape):
    rng = np.random.default_rng(200 + S_)
    return (rng.standard_normal((S_, 20, 12)), rng.standard_normal((S_,) + obs_shape), rng.standard_normal((S_, 37, 29)),
            rng.standard_normal((S_, 20, 29)))


@pytest.mark.parametrize("S_", [1, 64, 65])
def test_full_grid_same_noise_vs_spec(engine, S_):
    Y, _, x1, x2, f1, f2, _ = grid40()
    engine.plan("matern12", "b0", G1, x1, "matern12", "b0", G2, x2)
    Yd = dev(Y)
    engine.elbo_step(Yd, engine.sumsq(Yd), Cs.THETA)
    eu, _, eg, eh = random_noise(S_, (1,))
    want, levels = R.sample_full(full40_state(), f1, f2, B1AX, B2AX, eu, eg, eh)
    out, info = engine.posterior_raster_sample(B1AX, B2AX, S_, eps_u=dev(eu), eps_g=dev(eg), eps_h=dev(eh))
    err = rel(host(out), want)
    print(f"full grid S = {S_}: vs spec {err:.1e}; root levels {info['jitter']} (spec {levels})")
    assert err <= 1e-9 and info["jitter"] == (0.0, 0.0)


_FULL40 = []


def full40_state():
    if not _FULL40:
        Y, _, _, _, f1, f2, _ = grid40()
        _FULL40.append(Kr.elbo_step(Y, f1, f2, Cs.THETA))
    return _FULL40[0]


@pytest.mark.parametrize("S_", [1, 64, 65])
def test_masked_same_noise_vs_spec(engine, S_):
    Y, W, x1, x2, f1, f2, st = grid40()
    Wd, _, nobs, _, _ = step_grid40(engine)
    eu, eo, eg, eh = random_noise(S_, (GN2, GN1))
    want, winfo = R.sample_masked(st, f1, f2, B1AX, B2AX, eu, eo, eg, eh)
    out, info = engine.posterior_raster_sample_masked_iter(B1AX, B2AX, Wd, nobs, S_, eps_u=dev(eu), eps_obs=dev(eo), eps_g=dev(eg), eps_h=dev(eh))
    err = rel(host(out), want)
    print(f"masked S = {S_}: vs spec {err:.1e}; iterations {info['rounds'][0]} (spec {winfo['rounds']}), solves {info['sweeps'][0]}")
    assert err <= 1e-9
    assert abs(info["rounds"][0] - winfo["rounds"]) <= 1 and info["sweeps"][0] == winfo["solves"] == -(-S_ // 64)


@pytest.mark.parametrize("S_", [1, 64, 65])
def test_scattered_same_noise_vs_spec(engine, S_):
    X, y, f1, f2, st = points1500()
    step_points1500(engine)
    eu, eo, eg, eh = random_noise(S_, (SN,))
    want, winfo = R.sample_scattered(st, f1, f2, B1AX, B2AX, eu, eo, eg, eh)
    out, info = engine.posterior_raster_sample_scattered_iter(B1AX, B2AX, S_, eps_u=dev(eu), eps_obs=dev(eo), eps_g=dev(eg), eps_h=dev(eh))
    err = rel(host(out), want)
    print(f"scattered S = {S_}: vs spec {err:.1e}; iterations {info['rounds'][0]} (spec {winfo['rounds']}), solves {info['sweeps'][0]}")
    assert err <= 1e-9
    assert abs(info["rounds"][0] - winfo["rounds"]) <= 1 and info["sweeps"][0] == winfo["solves"] == -(-S_ // 64)


# ---- 4. the seed path, and independence of the grouping -------------------------------------------------------------------------------------
def seeded_noise(engine, seed, first, n, obs_n=None, obs_shape=None):
    p1, p2, m1, m2 = 37, 29, 20, 12
    out = dict(eps_u=engine.normal_fill(seed, 0, first * m1 * m2, n * m1 * m2).reshape(n, m1, m2),
               eps_g=engine.normal_fill(seed, 2, first * p1 * p2, n * p1 * p2).reshape(n, p1, p2),
               eps_h=engine.normal_fill(seed, 3, first * m1 * p2, n * m1 * p2).reshape(n, m1, p2))
    if obs_n:
        out["eps_obs"] = engine.normal_fill(seed, 1, first * obs_n, n * obs_n).reshape((n,) + obs_shape)
    return out


def check_seed_and_grouping(tag, engine, call, obs_n=None, obs_shape=None):
    seed, first, n = 11, 3, 5
    a = call(n, seed=seed, first=first)
    b = call(n, **seeded_noise(engine, seed, first, n, obs_n, obs_shape))
    assert torch.equal(a, b)                                       # the seed path IS the explicit path on the generator's numbers
    w70 = call(70, seed=seed)
    one = call(1, seed=seed, first=5)
    e1, e2 = rel(host(one[0]), host(w70[5])), rel(host(a), host(w70[3:8]))
    print(f"{tag}: first = 5, n = 1 vs row 5 of n = 70: {e1:.1e}; rows 3..7 drawn as a block of 5: {e2:.1e}")
    assert e1 <= 1e-12 and e2 <= 1e-12
    assert not torch.equal(w70[0], w70[1])
    return w70


def test_seed_path_and_grouping_full_grid(engine):
    Y, _, x1, x2, f1, f2, _ = grid40()
    engine.plan("matern12", "b0", G1, x1, "matern12", "b0", G2, x2)
    Yd = dev(Y)
    engine.elbo_step(Yd, engine.sumsq(Yd), Cs.THETA)
    w70 = check_seed_and_grouping("full grid", engine, lambda n, **kw: engine.posterior_raster_sample(B1AX, B2AX, n, **kw)[0])
    # ... and against the specification with the specification's own generator
    want, _ = R.sample_full(full40_state(), f1, f2, B1AX, B2AX, S.noise_u(11, 0, 3, 20, 12), R.noise_g(11, 0, 3, 37, 29), R.noise_h(11, 0, 3, 20, 29))
    assert rel(host(w70[:3]), want) <= 1e-9


def test_seed_path_and_grouping_masked(engine):
    Wd, _, nobs, _, _ = step_grid40(engine)
    call = lambda n, **kw: engine.posterior_raster_sample_masked_iter(B1AX, B2AX, Wd, nobs, n, **kw)[0]
    w70 = check_seed_and_grouping("masked", engine, call, GN1 * GN2, (GN2, GN1))
    n16, i16 = engine.posterior_raster_sample_masked_iter(B1AX, B2AX, Wd, nobs, 70, seed=11, block=16)
    assert i16["sweeps"][0] == 5 and rel(host(n16), host(w70)) <= 1e-12


def test_seed_path_and_grouping_scattered(engine):
    step_points1500(engine)
    call = lambda n, **kw: engine.posterior_raster_sample_scattered_iter(B1AX, B2AX, n, **kw)[0]
    w70 = check_seed_and_grouping("scattered", engine, call, SN, (SN,))
    n16, i16 = engine.posterior_raster_sample_scattered_iter(B1AX, B2AX, 70, seed=11, block=16)
    assert i16["sweeps"][0] == 5 and rel(host(n16), host(w70)) <= 1e-12


# ---- 5. one joint draw with q(v) ----------------------------------------------------------------------------------------------------------
def test_raster_samples_and_qv_samples_are_one_joint_draw(engine):
    """Inducing POINTS, raster axes = the inducing coordinates, G = H = 0: f at the inducing points IS v, so raster sample s is sample s
    of vggp_qv_sample from the same eps_u -- the two entries share the coefficient draw X_s."""
    case = "points-matern32"
    p = plan24(engine, case)
    _, _, g1, g2 = Cs.BASES[case]
    engine.elbo_step(p["Y"], p["yy_full"], Cs.THETA)
    rng = np.random.default_rng(4)
    S_, m1, m2 = 9, len(g1), len(g2)
    eu = dev(rng.standard_normal((S_, m1, m2)))
    V = engine.qv_sample(S_, eps_u=eu)
    F, _ = engine.posterior_raster_sample(g1, g2, S_, eps_u=eu, eps_g=dev(np.zeros((S_, m1, m2))), eps_h=dev(np.zeros((S_, m1, m2))))
    err = rel(host(F), host(V))
    print(f"raster samples at the inducing points vs q(v) samples from the same eps_u: {err:.1e}")
    assert err <= 1e-7
    # the seed path shares stream 0 with vggp_qv_sample: the coefficient part of the seeded raster sample is the seeded q(v) sample
    Vs = engine.qv_sample(3, seed=21, first=2)
    Fs, _ = engine.posterior_raster_sample(g1, g2, 3, eps_u=engine.normal_fill(21, 0, 2 * m1 * m2, 3 * m1 * m2).reshape(3, m1, m2),
                                           eps_g=dev(np.zeros((3, m1, m2))), eps_h=dev(np.zeros((3, m1, m2))))
    assert rel(host(Fs), host(Vs)) <= 1e-7


# ---- 6. a large raster: the blocked Cholesky, several tiles with the triangular skip --------------------------------------------------------
def test_large_raster_first_cholesky_columns(engine):
    Y, _, x1, x2, f1, f2, _ = grid40()
    engine.plan("matern12", "b0", G1, x1, "matern12", "b0", G2, x2)
    Yd = dev(Y)
    engine.elbo_step(Yd, engine.sumsq(Yd), Cs.THETA)
    p1, p2, m1, m2 = 300, 130, 20, 12
    a1, a2 = np.linspace(0.004, 0.996, p1), np.linspace(0.007, 0.993, p2)
    rng = np.random.default_rng(6)
    eu, eg, eh = np.zeros((3, m1, m2)), np.zeros((3, p1, p2)), np.zeros((3, m1, p2))
    eg[0, 0, 0] = 1.0                                              # unit G noise at (0, 0)
    eh[1, 0, 0] = 1.0                                              # unit H noise at (0, 0)
    eu[2], eg[2], eh[2] = rng.standard_normal((m1, m2)), rng.standard_normal((p1, p2)), rng.standard_normal((m1, p2))
    F, info = engine.posterior_raster_sample(a1, a2, 3, eps_u=dev(eu), eps_g=dev(eg), eps_h=dev(eh))
    mu, _ = engine.posterior_raster(dev(a1), dev(a2), want_var=False)
    assert bool(torch.isfinite(F).all()) and info["jitter"] == (0.0, 0.0)
    _, _, s1, s2, _ = Cs.THETA
    st = full40_state()
    L01, L02 = R._unit_L0(st.d1, f1, s1), R._unit_L0(st.d2, f2, s2)
    import scipy.linalg as sla
    U1 = sla.solve_triangular(L01, f1.build(Cs.THETA[0], x=a1)[2], lower=True)
    U2 = sla.solve_triangular(L02, f2.build(Cs.THETA[1], x=a2)[2], lower=True)
    k1 = Kr.kappa_and_dell("matern12", np.abs(a1[:, None] - a1[None, :]), Cs.THETA[0])[0]
    k2 = Kr.kappa_and_dell("matern12", np.abs(a2[:, None] - a2[None, :]), Cs.THETA[1])[0]
    r1p, r2p, k2p = k1 - U1.T @ U1 + R.ETA * np.eye(p1), k2 - U2.T @ U2 + R.ETA * np.eye(p2), k2 + R.ETA * np.eye(p2)
    want_g = np.sqrt(s1 * s2) * np.outer(r1p[:, 0], k2p[:, 0]) / np.sqrt(r1p[0, 0] * k2p[0, 0])
    want_h = np.sqrt(s2) * np.outer(np.sqrt(s1) * U1[0, :], r2p[:, 0]) / np.sqrt(r2p[0, 0])
    e_g, e_h = rel(host(F[0] - mu), want_g), rel(host(F[1] - mu), want_h)
    # (the differences are taken from samples of size |mu| ~ 1: their rounding, 1e-16 |mu|, is far below 1e-9 of the columns' 0.1 .. 1)
    print(f"300 x 130 raster: unit G noise vs the first Cholesky columns {e_g:.1e}, unit H noise {e_h:.1e}")
    assert e_g <= 1e-9 and e_h <= 1e-9
    # the random sample against the whole specification (blocked roots included): the read-out bound
    want, _ = R.sample_full(st, f1, f2, a1, a2, eu[2:], eg[2:], eh[2:])
    assert rel(host(F[2]), want[0]) <= 1e-7


# ---- 7. state and arguments -------------------------------------------------------------------------------------------------------------------
def test_state_and_arguments(engine):
    from variational_gridded_gaussian_processes_amd import Engine
    p = plan24(engine, "b0-matern12")
    W, nobs = p["W"], p["nobs"]
    full = lambda **kw: engine.posterior_raster_sample(kw.pop("g1", A1), kw.pop("g2", A2), kw.pop("n", 2), **kw)
    masked = lambda **kw: engine.posterior_raster_sample_masked_iter(kw.pop("g1", A1), kw.pop("g2", A2), W, nobs, kw.pop("n", 2), **kw)
    scat = lambda **kw: engine.posterior_raster_sample_scattered_iter(kw.pop("g1", A1), kw.pop("g2", A2), kw.pop("n", 2), **kw)
    # a fresh plan: nothing to read; the wrong plan kind is an argument error with or without a step
    assert code_of(full)[0] == ESTATE and code_of(masked)[0] == ESTATE and code_of(scat)[0] == EINVAL
    engine.elbo_step(p["Y"], p["yy_full"], Cs.THETA)
    assert code_of(masked)[0] == ESTATE and full()[0].shape == (2, 7, 5)
    before = engine.posterior_raster(dev(A1), dev(A2))
    z = lambda *s: dev(np.zeros(s))
    empty, long_axis = np.zeros(0), np.linspace(0, 1, 8193)
    bad_full = [dict(n=0), dict(first=-1), dict(g1=empty), dict(g2=empty), dict(g1=long_axis), dict(g2=long_axis),
                dict(eps_u=z(2, 6, 4)), dict(eps_g=z(2, 7, 5)), dict(eps_h=z(2, 6, 5)), dict(eps_u=z(2, 6, 4), eps_g=z(2, 7, 5)),
                dict(eps_g=z(2, 7, 5), eps_h=z(2, 6, 5))]
    for kw in bad_full:
        assert code_of(lambda: full(**dict(kw)))[0] == EINVAL, list(kw)
    # NULL out, and nothing is written on a refusal: the C entry itself, on a sentinel-filled output
    guard = torch.full((2, 7, 5), SENTINEL, dtype=torch.float64, device=DEV)
    a1, a2 = dev(A1), dev(A2)
    st = torch.cuda.current_stream().cuda_stream
    lib, h = engine.lib, engine._h
    assert lib.vggp_posterior_raster_sample(h, a1.data_ptr(), 7, a2.data_ptr(), 5, 2, 1, 0, None, None, None, None, None, st) == EINVAL
    assert lib.vggp_posterior_raster_sample(h, a1.data_ptr(), 7, a2.data_ptr(), 5, 2, 1, -1, None, None, None, guard.data_ptr(), None, st) == EINVAL
    assert lib.vggp_posterior_raster_sample(h, a1.data_ptr(), 7, a2.data_ptr(), 8193, 2, 1, 0, None, None, None, guard.data_ptr(), None, st) == EINVAL
    assert lib.vggp_posterior_raster_sample(h, a1.data_ptr(), 7, a2.data_ptr(), 5, 2, 1, 0, z(2, 6, 4).data_ptr(), None, None, guard.data_ptr(),
                                            None, st) == EINVAL
    assert bool((guard == SENTINEL).all())
    after = engine.posterior_raster(dev(A1), dev(A2))                            # the step's state is still readable: the same bits
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    # the dense masked step is not the matching step; the iterative one is
    engine.elbo_step_masked(p["Ym"], W, nobs, p["yy"], Cs.THETA)
    assert code_of(masked)[0] == ESTATE and code_of(full)[0] == ESTATE
    step_masked_iter(engine, p)
    assert code_of(full)[0] == ESTATE and masked()[0].shape == (2, 7, 5)
    mean_before, _ = engine.posterior_raster(dev(A1), dev(A2), want_var=False)
    eo = z(2, Cs.N2, Cs.N1)
    for kw in (dict(n=0), dict(block=65), dict(first=-1), dict(g1=empty), dict(g2=long_axis), dict(eps_u=z(2, 6, 4)), dict(eps_obs=eo),
               dict(eps_u=z(2, 6, 4), eps_obs=eo), dict(eps_u=z(2, 6, 4), eps_obs=eo, eps_g=z(2, 7, 5)), dict(eps_g=z(2, 7, 5), eps_h=z(2, 6, 5))):
        assert code_of(lambda: masked(**dict(kw)))[0] == EINVAL, list(kw)
    assert torch.equal(engine.posterior_raster(dev(A1), dev(A2), want_var=False)[0], mean_before)
    ps = plan24(engine, "b0-matern12", scattered=True)
    assert code_of(scat)[0] == ESTATE and code_of(full)[0] == ESTATE
    engine.elbo_step_scattered(ps["y"], ps["yy"], Cs.THETA)
    assert code_of(scat)[0] == ESTATE
    engine.elbo_step_scattered_iter(ps["y"], ps["yy"], Cs.THETA)
    assert scat()[0].shape == (2, 7, 5)
    for kw in (dict(n=0), dict(block=65), dict(g1=empty), dict(eps_u=z(2, 6, 4)), dict(eps_u=z(2, 6, 4), eps_g=z(2, 7, 5), eps_h=z(2, 6, 5))):
        assert code_of(lambda: scat(**dict(kw)))[0] == EINVAL, list(kw)
    # B1 hats: refused before anything is launched, on every entry, and the message names the indefinite residual
    pb = plan24(engine, "b1-matern12")
    engine.elbo_step(pb["Y"], pb["yy_full"], Cs.THETA)
    qv_before = engine.qv()
    code, msg = code_of(full)
    assert code == EINVAL and "indefinite" in msg
    assert all(torch.equal(a, b) for a, b in zip(engine.qv(), qv_before))
    step_masked_iter(engine, pb)
    code, msg = code_of(lambda: engine.posterior_raster_sample_masked_iter(A1, A2, pb["W"], pb["nobs"], 2))
    assert code == EINVAL and "indefinite" in msg
    # paired inducing points
    Z = np.random.default_rng(0).uniform(0, 1, (10, 2))
    engine.plan_paired("matern12", Z, p["x1"], p["x2"])
    engine.elbo_step(p["Y"], p["yy_full"], Cs.THETA)
    for call in (full, masked, scat):
        code, msg = code_of(call)
        assert code == EINVAL and "PAIRED" in msg
    # multi-rank contexts: refused, and the message says so
    eng2 = Engine(0, n_ranks=2, rank=0, allreduce=lambda buf: None)
    try:
        basis, kind, g1, g2 = Cs.BASES["b0-matern12"]
        eng2.plan(kind, basis, g1, p["x1"], kind, basis, g2, p["x2"])
        for call in (lambda: eng2.posterior_raster_sample_masked_iter(A1, A2, W, nobs, 2), lambda: eng2.posterior_raster_sample(A1, A2, 2)):
            code, msg = code_of(call)
            assert code == EINVAL and "multi-rank" in msg
        X = ps["X"]
        eng2.plan(kind, basis, g1, X[:, 0], kind, basis, g2, X[:, 1], scattered=True)
        code, msg = code_of(lambda: eng2.posterior_raster_sample_scattered_iter(A1, A2, 2))
        assert code == EINVAL and "multi-rank" in msg
    finally:
        eng2.close()


# ---- 8. neutrality ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["full_cold", "full_thin", "iter_masked", "iter_scattered"])
def test_sampling_between_two_steps_leaves_the_second_unchanged(engine, kind):
    import test_gpu_readout_states as RS
    theta2 = [0.25, 0.28, 1.1, 0.9, 0.012]

    def run(with_samples):
        if kind == "full_cold":
            p = plan24(engine, "b0-matern12")
            engine.elbo_step(p["Y"], p["yy_full"], Cs.THETA)
            sample = lambda: engine.posterior_raster_sample(B1AX, B2AX, 70, seed=1)
            step2 = lambda: engine.elbo_step(p["Y"], p["yy_full"], theta2)
        elif kind == "full_thin":                        # the cold range finder + thin chain: the state holds range directions only
            S_ = RS.STATES["rbf96_cold_thin"]
            pl, k, _, _, _ = RS._drive(engine, S_)
            sample = lambda: engine.posterior_raster_sample(A1, A2, 3, seed=1)
            step2 = lambda: pl.step(S_["path"](k + 1))
        elif kind == "iter_masked":
            Wd, Ym, nobs, yy, _ = step_grid40(engine)
            sample = lambda: engine.posterior_raster_sample_masked_iter(B1AX, B2AX, Wd, nobs, 70, seed=1, block=16)
            step2 = lambda: engine.elbo_step_masked_iter(Ym, Wd, nobs, yy, theta2)
        else:
            yd, yy, _ = step_points1500(engine)
            sample = lambda: engine.posterior_raster_sample_scattered_iter(B1AX, B2AX, 70, seed=1)
            step2 = lambda: engine.elbo_step_scattered_iter(yd, yy, theta2)
        if with_samples:
            out, _ = sample()
            assert bool(torch.isfinite(out).all())
        elbo, grad, info = step2()
        return elbo, grad, info["rounds"]
    a, b = run(False), run(True)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2], (a, b)


# ---- 9. models ----------------------------------------------------------------------------------------------------------------------------------
def check_grid_sampler(model, engine):
    a1, a2 = torch.tensor(A1), torch.tensor(A2)
    P = len(A1) * len(A2)
    pg = model.posterior_grid(a1, a2)
    a = pg.sample(torch.Size([8]), seed=3)
    assert a.shape == (8, P) and a.dtype == torch.float64 and bool(torch.isfinite(a).all())
    assert torch.equal(a, model.posterior_grid(a1, a2).sample(torch.Size([8]), seed=3))           # repeatable with the seed
    assert pg.sample(torch.Size([2, 3]), seed=3).shape == (2, 3, P) and pg.sample(seed=3).shape == (P,)
    assert rel(pg.sample(seed=3), a[0]) <= 1e-12                                               # sample 0 of the seed, however many are drawn
    b, c = pg.sample(torch.Size([8])), pg.sample(torch.Size([8]))
    assert not torch.equal(b, c)                                                              # without a seed the sequence continues
    again = model.posterior_grid(a1, a2)
    again._seed0 = pg._seed0
    assert rel(again.sample(torch.Size([16]))[8:], c) <= 1e-12                                 # ... one sequence: samples 8 .. 15 of its seed
    # predictive = latent + sqrt(noise) * stream 4
    pred = model.posterior_predictive_grid(a1, a2).sample(torch.Size([8]), seed=3)
    noise = float(model.likelihood.noise.detach().double())
    eps4 = engine.normal_fill(3, 4, 0, 8 * P).reshape(8, P).cpu()
    err = rel(pred - a, np.sqrt(noise) * eps4)
    print(f"{type(model).__name__}: predictive - latent samples vs sqrt(noise) * stream 4: {err:.1e}")
    assert err <= 1e-7
    # flat index a P2 + b: zero-variance directions aside, the sample mean of many draws follows the raster mean's layout
    assert pg.mean.shape == (P,)
    return pg, a


def test_models_sample_maps(engine):
    from oracle import dense as D
    from test_gpu_qv_sample import masked_xy
    from variational_gridded_gaussian_processes_amd.models import GriddedMatern12SVGP, Matern12B1SplineASVGP, Matern12GriddedGP
    Xf, yf, _, _ = D.gen_grid(24, 20)
    full = Matern12GriddedGP(torch.tensor(Xf), torch.tensor(yf), 9, (0, 1), (0, 1), engine=engine).to(torch.float64)
    pg, a = check_grid_sampler(full, engine)
    # the spread of the samples is the spread of the map: 8 samples cannot leave mean +- 8 sigma
    assert bool(((a - pg.mean).abs() <= 8.0 * pg.stddev + 1e-12).all())
    Xm, ym = masked_xy(24, 20)
    it = Matern12GriddedGP(Xm, ym, 9, (0, 1), (0, 1), engine=engine, solver="iterative").to(torch.float64)
    assert it.last_readout_info is None
    check_grid_sampler(it, engine)
    assert it._iter and it.last_readout_info["sweeps"][0] == 1 and it.last_readout_info["rounds"][0] > 0
    rng = np.random.default_rng(3)
    Xs = rng.uniform(0, 1, (400, 2))
    ys = np.asarray(D.latent_2d(Xs[:, 0], Xs[:, 1])) + 0.05 * rng.standard_normal(400)
    sc = Matern12GriddedGP(torch.tensor(Xs), torch.tensor(ys), 9, (0, 1), (0, 1), engine=engine, scattered_solver="iterative").to(torch.float64)
    check_grid_sampler(sc, engine)
    assert sc._siter and sc.last_readout_info["sweeps"][0] == 1
    # the refusals
    a1, a2 = torch.tensor(A1), torch.tensor(A2)
    de = Matern12GriddedGP(Xm, ym, 9, (0, 1), (0, 1), engine=engine, solver="dense").to(torch.float64)
    with pytest.raises(NotImplementedError, match="solver='iterative'"):
        de.posterior_grid(a1, a2).sample()
    ds = Matern12GriddedGP(torch.tensor(Xs), torch.tensor(ys), 9, (0, 1), (0, 1), engine=engine).to(torch.float64)
    with pytest.raises(NotImplementedError, match="scattered_solver='iterative'"):
        ds.posterior_predictive_grid(a1, a2).sample()
    b1 = Matern12B1SplineASVGP(torch.tensor(Xf), torch.tensor(yf), 9, (0, 1), (0, 1), engine=engine).to(torch.float64)
    with pytest.raises(NotImplementedError, match="indefinite"):
        b1.posterior_grid(a1, a2).sample()
    Z = torch.tensor(np.random.default_rng(0).uniform(0, 1, (12, 2)))
    pa = GriddedMatern12SVGP(torch.tensor(Xf), torch.tensor(yf), Z, 8, (0, 1), (0, 1), inducing="general", engine=engine).to(torch.float64)
    with pytest.raises(NotImplementedError, match="paired"):
        pa.posterior_grid(a1, a2)
    with pytest.raises(NotImplementedError, match="joint samples"):
        full.posterior(torch.tensor(Xf[:5])).sample()
