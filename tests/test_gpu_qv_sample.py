"""Joint samples of q(v) on the GPU: vggp_normal_fill, vggp_qv_sample (full grid), vggp_qv_sample_masked_iter and
vggp_qv_sample_scattered_iter against tests/qv_sample_spec.py, the dense GPU steps and the dense oracles, and through the models.

Bounds (none taken from what the code gives):
  normal_fill vs the spec   5e-14 absolute: the uniforms are bit-exact, what differs is the rounding of log / sqrt / sincos and the spec's
                            rounding of 2 pi u2, a few ulp each, times |z| <= 8.66
  covariance by unit noise  1e-7 of the largest entry: the existing GPU bound for read-out means against the dense oracle
  same noise vs the spec    1e-9 of the largest entry of the sample: the bound of tests/test_gpu_masked_iter_spec.py for a solved block
  grouping                  bitwise on the iterative entries (the solver guarantees it for read-out columns), 1e-12 on the full grid
"""
import functools

import numpy as np
import pytest
import torch

import masked_iter_readout_spec as MS
import qv_sample_cases as Cs
import qv_sample_spec as S
import scattered_iter_variance_spec as SS
from oracle import dense as D
from oracle import kron as Kr
from variational_gridded_gaussian_processes_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
rel = Cs.rel


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def host(t):
    return t.cpu().numpy()


def code_of(call):
    try:
        call()
    except _lib.VggpError as e:
        return e.code, str(e)
    return 0, ""


# ---- the generator -------------------------------------------------------------------------------------------------------------------------
def test_normal_fill_vs_spec(engine):
    worst = 0.0
    for seed, stream, first, n in ((12345, 0, 0, 20000), (7, 1, 999, 4097), (2**63 + 11, 0, 2**40 + 3, 1000), (0, 5, 1, 1)):
        got = host(engine.normal_fill(seed, stream, first, n))
        want = S.normal_fill(seed, stream, first, n)
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"normal_fill vs spec: max abs difference {worst:.2e}")
    assert worst <= 5e-14
    whole = engine.normal_fill(7, 1, 0, 3000)
    parts = torch.cat([engine.normal_fill(7, 1, 0, 1037), engine.normal_fill(7, 1, 1037, 1963)])          # split at an odd index
    assert torch.equal(whole, parts)
    assert engine.normal_fill(7, 1, 0, 0).numel() == 0
    assert code_of(lambda: engine.normal_fill(7, -1, 0, 4))[0] == _lib.VGGP_EINVAL
    assert code_of(lambda: engine.normal_fill(7, 0, -1, 4))[0] == _lib.VGGP_EINVAL


# ---- the M = 24 problems: plans and steps ------------------------------------------------------------------------------------------------------
def plan24(engine, case, scattered=False):
    basis, kind, g1, g2 = Cs.BASES[case]
    if scattered:
        X, y = Cs.scattered_data()
        engine.plan(kind, basis, g1, X[:, 0], kind, basis, g2, X[:, 1], scattered=True)
        yd = dev(y)
        return dict(y=yd, yy=float((yd * yd).sum().item()), X=X, yn=y)
    Y, W, x1, x2 = Cs.grid_data()
    engine.plan(kind, basis, g1, x1, kind, basis, g2, x2)
    Wd, Yd = dev(W), dev(Y)
    Ym = Yd * Wd
    return dict(Y=Yd, yy_full=engine.sumsq(Yd), W=Wd, Ym=Ym, nobs=float(W.sum()), yy=engine.sumsq(Ym), Yn=Y, Wn=W, x1=x1, x2=x2)


def step_masked_iter(engine, p):
    return engine.elbo_step_masked_iter(p["Ym"], p["W"], p["nobs"], p["yy"], Cs.THETA)


# ---- covariance by unit noise ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Cs.KERNEL_BASES + ["b1-matern12"])
def test_full_grid_covariance_by_unit_noise(engine, case):
    p = plan24(engine, case)
    f1, f2 = Cs.factors(case, p["x1"], p["x2"])
    m1, m2 = f1.m, f2.m
    M = m1 * m2
    engine.elbo_step(p["Y"], p["yy_full"], Cs.THETA)
    eps = np.zeros((M + 1, M))
    eps[np.arange(M), np.arange(M)] = 1.0                       # (the M eps_u columns, and one of zero noise)
    out = engine.qv_sample(M + 1, eps_u=dev(eps.reshape(M + 1, m1, m2)))
    mean, _ = engine.qv()
    assert torch.equal(out[M], mean)                            # zero noise: the mean, bit for bit
    got = Cs.outer_sum(host(out[:M]), host(mean))
    e_gpu, e_or = rel(got, host(engine.qv_cov())), rel(got, Kr.q_v_cov(Kr.elbo_step(p["Yn"], f1, f2, Cs.THETA)))
    print(f"{case}: full grid, unit noise vs qv_cov {e_gpu:.1e}, vs oracle {e_or:.1e}")
    assert e_gpu <= 1e-7 and e_or <= 1e-7


@pytest.mark.parametrize("case", Cs.KERNEL_BASES + ["b1-matern12"])
def test_masked_covariance_by_unit_noise(engine, case):
    p = plan24(engine, case)
    f1, f2 = Cs.factors(case, p["x1"], p["x2"])
    m1, m2 = f1.m, f2.m
    M = m1 * m2
    engine.elbo_step_masked(p["Ym"], p["W"], p["nobs"], p["yy"], Cs.THETA)
    cov_gpu = host(engine.qv_cov_masked())
    cov_or = Kr.q_v_cov_masked(Kr.elbo_step_masked(p["Yn"], p["Wn"], f1, f2, Cs.THETA), f1, f2)
    step_masked_iter(engine, p)
    eps_u, eps_obs = Cs.unit_noise(m1, m2, (Cs.N2, Cs.N1))
    out, info = engine.qv_sample_masked_iter(p["W"], p["nobs"], eps_u.shape[0], eps_u=dev(eps_u), eps_obs=dev(eps_obs))
    mean, _, _ = engine.qv_masked_iter(p["W"], p["nobs"], variance=False)
    got = Cs.outer_sum(host(out), host(mean))
    e_gpu, e_or = rel(got, cov_gpu), rel(got, cov_or)
    print(f"{case}: masked, {eps_u.shape[0]} unit samples vs qv_cov_masked {e_gpu:.1e}, vs oracle {e_or:.1e}; "
          f"{info['rounds'][0]} iterations, {info['sweeps'][0]} solves")
    assert e_gpu <= 1e-7 and e_or <= 1e-7
    assert info["sweeps"][0] == 3 and 0 < info["rounds"][0] < 40
    dead = M + np.flatnonzero(p["Wn"].reshape(-1) == 0)         # noise on unobserved nodes: a zero right-hand side, the mean bit for bit
    assert len(dead) > 0 and all(torch.equal(out[s], mean) for s in dead)


@pytest.mark.parametrize("case", Cs.KERNEL_BASES + ["b1-matern12"])
def test_scattered_covariance_by_unit_noise(engine, case):
    p = plan24(engine, case, scattered=True)
    X = p["X"]
    f1, f2 = Cs.factors(case, X[:, 0], X[:, 1])
    m1, m2 = f1.m, f2.m
    engine.elbo_step_scattered(p["y"], p["yy"], Cs.THETA)
    cov_gpu = host(engine.qv_cov_masked())
    cov_or = Kr.q_v_cov_masked(Kr.elbo_step_scattered(X, p["yn"], f1, f2, Cs.THETA), f1, f2)
    engine.elbo_step_scattered_iter(p["y"], p["yy"], Cs.THETA)
    eps_u, eps_obs = Cs.unit_noise(m1, m2, (Cs.NPTS,))
    eps_u, eps_obs = np.concatenate([eps_u, np.zeros((1, m1, m2))]), np.concatenate([eps_obs, np.zeros((1, Cs.NPTS))])
    out, info = engine.qv_sample_scattered_iter(eps_u.shape[0], eps_u=dev(eps_u), eps_obs=dev(eps_obs))
    mean = engine.qv_scattered_iter()
    assert torch.equal(out[-1], mean)
    got = Cs.outer_sum(host(out[:-1]), host(mean))
    e_gpu, e_or = rel(got, cov_gpu), rel(got, cov_or)
    print(f"{case}: scattered, {eps_u.shape[0] - 1} unit samples vs qv_cov_masked {e_gpu:.1e}, vs oracle {e_or:.1e}; "
          f"{info['rounds'][0]} iterations, {info['sweeps'][0]} solves")
    assert e_gpu <= 1e-7 and e_or <= 1e-7 and info["sweeps"][0] == 3


# ---- same noise against the numpy specification: 20 x 12 features, shapes that are no multiple of 16 ----------------------------------------------
G1, G2 = np.linspace(0, 1, 21), np.linspace(0, 1, 13)          # B0 meshes: m1 = 20, m2 = 12
GN1, GN2, SN = 40, 36, 1500


@functools.lru_cache(maxsize=None)
def grid40():
    _, y, x1, x2 = D.gen_grid(GN1, GN2)
    W = (np.random.default_rng(1).uniform(size=(GN2, GN1)) < 0.7).astype(np.float64)
    f1, f2 = Kr.Factor("b0", "matern12", G1, x1), Kr.Factor("b0", "matern12", G2, x2)
    Y = y.reshape(GN2, GN1)
    return Y, W, x1, x2, f1, f2, MS.prepare(Y, W, f1, f2, Cs.THETA)


@functools.lru_cache(maxsize=None)
def points1500():
    rng = np.random.default_rng(5)
    X = rng.uniform(0, 1, (SN, 2))
    y = np.asarray(D.latent_2d(X[:, 0], X[:, 1])) + 0.05 * rng.standard_normal(SN)
    f1, f2 = Kr.Factor("b0", "matern12", G1, X[:, 0].copy()), Kr.Factor("b0", "matern12", G2, X[:, 1].copy())
    return X, y, f1, f2, SS.prepare(X, y, f1, f2, Cs.THETA)


def random_noise(S_, obs_shape):
    rng = np.random.default_rng(100 + S_)
    return rng.standard_normal((S_, 20, 12)), rng.standard_normal((S_,) + obs_shape)


def step_grid40(engine):
    Y, W, x1, x2, f1, f2, st = grid40()
    engine.plan("matern12", "b0", G1, x1, "matern12", "b0", G2, x2)
    Wd = dev(W)
    Ym = dev(Y) * Wd
    nobs, yy = float(W.sum()), engine.sumsq(Ym)
    res = engine.elbo_step_masked_iter(Ym, Wd, nobs, yy, Cs.THETA)
    return Wd, Ym, nobs, yy, res


def step_points1500(engine):
    X, y, f1, f2, st = points1500()
    engine.plan("matern12", "b0", G1, X[:, 0], "matern12", "b0", G2, X[:, 1], scattered=True)
    yd = dev(y)
    yy = float((yd * yd).sum().item())
    return yd, yy, engine.elbo_step_scattered_iter(yd, yy, Cs.THETA)


@pytest.mark.parametrize("S_", [1, 64, 65])
def test_masked_same_noise_vs_spec(engine, S_):
    Y, W, x1, x2, f1, f2, st = grid40()
    Wd, _, nobs, _, _ = step_grid40(engine)
    eu, eo = random_noise(S_, (GN2, GN1))
    want, winfo = S.sample_masked(st, f1, f2, eu, eo)
    out, info = engine.qv_sample_masked_iter(Wd, nobs, S_, eps_u=dev(eu), eps_obs=dev(eo))
    err = rel(host(out), want)
    print(f"masked S = {S_}: vs spec {err:.1e}; iterations {info['rounds'][0]} (spec {winfo['rounds']}), solves {info['sweeps'][0]}")
    assert err <= 1e-9
    assert abs(info["rounds"][0] - winfo["rounds"]) <= 1 and info["sweeps"][0] == winfo["solves"] == -(-S_ // 64)


@pytest.mark.parametrize("S_", [1, 64, 65])
def test_scattered_same_noise_vs_spec(engine, S_):
    X, y, f1, f2, st = points1500()
    step_points1500(engine)
    eu, eo = random_noise(S_, (SN,))
    want, winfo = S.sample_scattered(st, f1, f2, eu, eo)
    out, info = engine.qv_sample_scattered_iter(S_, eps_u=dev(eu), eps_obs=dev(eo))
    err = rel(host(out), want)
    print(f"scattered S = {S_}: vs spec {err:.1e}; iterations {info['rounds'][0]} (spec {winfo['rounds']}), solves {info['sweeps'][0]}")
    assert err <= 1e-9
    assert abs(info["rounds"][0] - winfo["rounds"]) <= 1 and info["sweeps"][0] == winfo["solves"] == -(-S_ // 64)


@pytest.mark.parametrize("S_", [1, 64, 65])
def test_full_grid_same_noise_vs_spec(engine, S_):
    Y, _, x1, x2, f1, f2, _ = grid40()
    engine.plan("matern12", "b0", G1, x1, "matern12", "b0", G2, x2)
    Yd = dev(Y)
    engine.elbo_step(Yd, engine.sumsq(Yd), Cs.THETA)
    eu, _ = random_noise(S_, (1,))
    want = S.sample_full(Kr.elbo_step(Y, f1, f2, Cs.THETA), eu)
    err = rel(host(engine.qv_sample(S_, eps_u=dev(eu))), want)
    print(f"full grid S = {S_}: vs spec {err:.1e}")
    assert err <= 1e-9


# ---- the seed path, and independence of the grouping ----------------------------------------------------------------------------------------------
def test_seed_path_is_the_explicit_path_and_grouping_masked(engine):
    Wd, _, nobs, _, _ = step_grid40(engine)
    M, nn = 20 * 12, GN1 * GN2
    seed, first, n = 11, 3, 5
    eu = engine.normal_fill(seed, 0, first * M, n * M).reshape(n, 20, 12)
    eo = engine.normal_fill(seed, 1, first * nn, n * nn).reshape(n, GN2, GN1)
    a, _ = engine.qv_sample_masked_iter(Wd, nobs, n, seed=seed, first=first)
    b, _ = engine.qv_sample_masked_iter(Wd, nobs, n, eps_u=eu, eps_obs=eo)
    assert torch.equal(a, b)
    want = S.sample_masked(grid40()[6], grid40()[4], grid40()[5], S.noise_u(seed, first, n, 20, 12), S.noise_obs_grid(seed, first, n, GN1, GN2))[0]
    print(f"masked seed path vs spec with the spec's own generator: {rel(host(a), want):.1e}")
    assert rel(host(a), want) <= 1e-9
    w70, i64 = engine.qv_sample_masked_iter(Wd, nobs, 70, seed=seed, block=64)
    n16, i16 = engine.qv_sample_masked_iter(Wd, nobs, 70, seed=seed, block=16)
    one, _ = engine.qv_sample_masked_iter(Wd, nobs, 1, seed=seed, first=5)
    assert (i64["sweeps"][0], i16["sweeps"][0]) == (2, 5)
    assert torch.equal(w70, n16) and torch.equal(one[0], w70[5])
    assert not torch.equal(w70[0], w70[1])


def test_seed_path_is_the_explicit_path_and_grouping_scattered(engine):
    step_points1500(engine)
    M = 20 * 12
    seed, first, n = 11, 3, 5
    eu = engine.normal_fill(seed, 0, first * M, n * M).reshape(n, 20, 12)
    eo = engine.normal_fill(seed, 1, first * SN, n * SN).reshape(n, SN)
    a, _ = engine.qv_sample_scattered_iter(n, seed=seed, first=first)
    b, _ = engine.qv_sample_scattered_iter(n, eps_u=eu, eps_obs=eo)
    assert torch.equal(a, b)
    w70, i64 = engine.qv_sample_scattered_iter(70, seed=seed, block=64)
    n16, i16 = engine.qv_sample_scattered_iter(70, seed=seed, block=16)
    one, _ = engine.qv_sample_scattered_iter(1, seed=seed, first=5)
    assert (i64["sweeps"][0], i16["sweeps"][0]) == (2, 5)
    assert torch.equal(w70, n16) and torch.equal(one[0], w70[5])


def test_seed_path_is_the_explicit_path_and_grouping_full_grid(engine):
    Y, _, x1, x2, _, _, _ = grid40()
    engine.plan("matern12", "b0", G1, x1, "matern12", "b0", G2, x2)
    Yd = dev(Y)
    engine.elbo_step(Yd, engine.sumsq(Yd), Cs.THETA)
    M = 20 * 12
    a = engine.qv_sample(5, seed=11, first=3)
    b = engine.qv_sample(5, eps_u=engine.normal_fill(11, 0, 3 * M, 5 * M).reshape(5, 20, 12))
    assert torch.equal(a, b)
    w70 = engine.qv_sample(70, seed=11)
    one = engine.qv_sample(1, seed=11, first=5)
    print(f"full grid: first = 5, n = 1 vs row 5 of n = 70: {rel(host(one[0]), host(w70[5])):.1e}")
    assert rel(host(one[0]), host(w70[5])) <= 1e-12 and rel(host(a), host(w70[3:8])) <= 1e-12


# ---- beyond the dense limit ---------------------------------------------------------------------------------------------------------------------
def test_beyond_the_dense_limit(engine):
    """M = 136 * 128 = 17408 > 16384 on an all-observed 272 x 256 grid: the preconditioner is exact there."""
    n1, n2, m1, m2 = 272, 256, 136, 128
    _, y, x1, x2 = D.gen_grid(n1, n2)
    g1, g2 = np.linspace(0, 1, m1 + 1), np.linspace(0, 1, m2 + 1)
    f1, f2 = Kr.Factor("b0", "matern12", g1, x1), Kr.Factor("b0", "matern12", g2, x2)
    Y, W = y.reshape(n2, n1), np.ones((n2, n1))
    engine.plan("matern12", "b0", g1, x1, "matern12", "b0", g2, x2)
    Wd, Yd = dev(W), dev(Y)
    engine.elbo_step_masked_iter(Yd, Wd, float(n1 * n2), engine.sumsq(Yd), Cs.THETA)
    rng = np.random.default_rng(8)
    eu, eo = rng.standard_normal((3, m1, m2)), rng.standard_normal((3, n2, n1))
    out, info = engine.qv_sample_masked_iter(Wd, float(n1 * n2), 3, eps_u=dev(eu), eps_obs=dev(eo))
    st = MS.prepare(Y, W, f1, f2, Cs.THETA)
    want, winfo = S.sample_masked(st, f1, f2, eu, eo)
    err = rel(host(out), want)
    print(f"M = {m1 * m2}: vs spec {err:.1e}; iterations {info['rounds'][0]} (spec {winfo['rounds']})")
    assert err <= 1e-9 and info["rounds"][0] <= 3


# ---- state and arguments ------------------------------------------------------------------------------------------------------------------------
def test_state_and_arguments(engine):
    from variational_gridded_gaussian_processes_amd import Engine
    EINVAL, ESTATE = _lib.VGGP_EINVAL, _lib.VGGP_ESTATE
    p = plan24(engine, "b0-matern12")
    W, nobs = p["W"], p["nobs"]
    full = lambda **kw: engine.qv_sample(kw.pop("n", 2), **kw)
    masked = lambda **kw: engine.qv_sample_masked_iter(W, nobs, kw.pop("n", 2), **kw)
    scat = lambda **kw: engine.qv_sample_scattered_iter(kw.pop("n", 2), **kw)
    # a fresh plan: nothing to read; the wrong plan kind is an argument error with or without a step
    assert code_of(full)[0] == ESTATE and code_of(masked)[0] == ESTATE
    assert code_of(scat)[0] == EINVAL
    engine.elbo_step(p["Y"], p["yy_full"], Cs.THETA)
    assert code_of(masked)[0] == ESTATE and full().shape == (2, 6, 4)
    engine.elbo_step_masked(p["Ym"], W, nobs, p["yy"], Cs.THETA)                 # the dense masked step is not the matching step
    assert code_of(masked)[0] == ESTATE
    step_masked_iter(engine, p)
    assert code_of(full)[0] == ESTATE and masked()[0].shape == (2, 6, 4)
    eu, eo = dev(np.zeros((2, 6, 4))), dev(np.zeros((2, Cs.N2, Cs.N1)))
    for bad in (lambda: masked(n=0), lambda: masked(block=65), lambda: masked(first=-1), lambda: masked(eps_u=eu),
                lambda: masked(eps_obs=eo)):
        assert code_of(bad)[0] == EINVAL
    assert code_of(lambda: full(n=0))[0] == ESTATE                               # (the state is tested first, as vggp_qv_cov does)
    engine.elbo_step(p["Y"], p["yy_full"], Cs.THETA)
    assert code_of(lambda: full(n=0))[0] == EINVAL and code_of(lambda: full(first=-1))[0] == EINVAL
    ps = plan24(engine, "b0-matern12", scattered=True)
    Wsq = dev(np.ones((Cs.NPTS, Cs.NPTS)))                                       # (a mask of the planned shape: the entry itself refuses)
    assert code_of(scat)[0] == ESTATE and code_of(lambda: engine.qv_sample_masked_iter(Wsq, 1.0, 2))[0] == EINVAL
    engine.elbo_step_scattered(ps["y"], ps["yy"], Cs.THETA)
    assert code_of(scat)[0] == ESTATE
    engine.elbo_step_scattered_iter(ps["y"], ps["yy"], Cs.THETA)
    assert scat()[0].shape == (2, 6, 4)
    for bad in (lambda: scat(n=0), lambda: scat(block=65), lambda: scat(eps_u=eu)):
        assert code_of(bad)[0] == EINVAL
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
        for call in (lambda: eng2.qv_sample_masked_iter(W, nobs, 2), lambda: eng2.qv_sample(2)):
            code, msg = code_of(call)
            assert code == EINVAL and "multi-rank" in msg
        X = ps["X"]
        eng2.plan(kind, basis, g1, X[:, 0], kind, basis, g2, X[:, 1], scattered=True)
        code, msg = code_of(lambda: eng2.qv_sample_scattered_iter(2))
        assert code == EINVAL and "multi-rank" in msg
    finally:
        eng2.close()


def test_sampling_between_two_steps_leaves_the_second_unchanged(engine):
    theta2 = [0.25, 0.28, 1.1, 0.9, 0.012]
    # full grid
    p = plan24(engine, "b0-matern12")
    engine.elbo_step(p["Y"], p["yy_full"], Cs.THETA)
    e_a, g_a, _ = engine.elbo_step(p["Y"], p["yy_full"], theta2)
    p = plan24(engine, "b0-matern12")
    engine.elbo_step(p["Y"], p["yy_full"], Cs.THETA)
    engine.qv_sample(70, seed=1)
    e_b, g_b, _ = engine.elbo_step(p["Y"], p["yy_full"], theta2)
    assert e_a == e_b and np.array_equal(g_a, g_b)
    # iterative masked
    Wd, Ym, nobs, yy, _ = step_grid40(engine)
    e_a, g_a, i_a = engine.elbo_step_masked_iter(Ym, Wd, nobs, yy, theta2)
    Wd, Ym, nobs, yy, _ = step_grid40(engine)
    engine.qv_sample_masked_iter(Wd, nobs, 70, seed=1, block=16)
    e_b, g_b, i_b = engine.elbo_step_masked_iter(Ym, Wd, nobs, yy, theta2)
    assert e_a == e_b and np.array_equal(g_a, g_b) and i_a["rounds"] == i_b["rounds"]
    # iterative scattered
    yd, yy, _ = step_points1500(engine)
    e_a, g_a, i_a = engine.elbo_step_scattered_iter(yd, yy, theta2)
    yd, yy, _ = step_points1500(engine)
    engine.qv_sample_scattered_iter(70, seed=1)
    e_b, g_b, i_b = engine.elbo_step_scattered_iter(yd, yy, theta2)
    assert e_a == e_b and np.array_equal(g_a, g_b) and i_a["rounds"] == i_b["rounds"]


# ---- models ------------------------------------------------------------------------------------------------------------------------------------
def masked_xy(n1, n2, frac=0.7):
    X, y, _, _ = D.gen_grid(n1, n2)
    keep = np.random.default_rng(1).uniform(size=n1 * n2) < frac
    return torch.tensor(X[keep]), torch.tensor(y[keep])


def check_sampler(model, M):
    qv = model.q_v()
    a = qv.sample(torch.Size([8]), seed=3)
    assert a.shape == (8, M) and a.dtype == torch.float64 and bool(torch.isfinite(a).all())
    assert torch.equal(a, model.q_v().sample(torch.Size([8]), seed=3))          # repeatable with the seed
    assert qv.sample(torch.Size([2, 3]), seed=3).shape == (2, 3, M) and qv.sample(seed=3).shape == (M,)
    assert rel(qv.sample(seed=3), a[0]) <= 1e-12                                # sample 0 of the seed, however many are drawn with it
    b, c = qv.sample(torch.Size([8])), qv.sample(torch.Size([8]))
    assert not torch.equal(b, c)                                               # without a seed the sequence continues
    assert not hasattr(qv, "rsample")
    return qv, a


def test_models_sample(engine):
    from variational_gridded_gaussian_processes_amd.models import GriddedMatern12VFFGP, Matern12GriddedGP, MultivariateNormal, _symmetric_root
    Xf, yf, _, _ = D.gen_grid(24, 20)
    full = Matern12GriddedGP(torch.tensor(Xf), torch.tensor(yf), 9, (0, 1), (0, 1), engine=engine).to(torch.float64)
    qv, a = check_sampler(full, 64)
    # the spread of the samples is the spread of q(v): 8 samples cannot leave mean +- 8 sigma
    assert bool(((a - qv.mean).abs() <= 8.0 * qv.stddev + 1e-12).all())
    Xm, ym = masked_xy(24, 20)
    it = Matern12GriddedGP(Xm, ym, 9, (0, 1), (0, 1), engine=engine, solver="iterative").to(torch.float64)
    assert it.last_readout_info is None
    check_sampler(it, 64)
    assert it._iter and it.last_readout_info["sweeps"][0] == 1 and it.last_readout_info["rounds"][0] > 0
    rng = np.random.default_rng(3)
    Xs = rng.uniform(0, 1, (400, 2))
    ys = np.asarray(D.latent_2d(Xs[:, 0], Xs[:, 1])) + 0.05 * rng.standard_normal(400)
    sc = Matern12GriddedGP(torch.tensor(Xs), torch.tensor(ys), 9, (0, 1), (0, 1), engine=engine, scattered_solver="iterative").to(torch.float64)
    check_sampler(sc, 64)
    assert sc._siter and sc.last_readout_info["sweeps"][0] == 1
    # the dense masked state at small M: samples from the dense covariance through its symmetric root, the engine's normals
    de = Matern12GriddedGP(Xm, ym, 9, (0, 1), (0, 1), engine=engine, solver="dense").to(torch.float64)
    qd, s = check_sampler(de, 64)
    root = _symmetric_root(qd.covariance_matrix)
    assert rel(root @ root, qd.covariance_matrix) <= 1e-12 and rel(root, root.T) <= 1e-12
    eps = engine.normal_fill(3, 0, 0, 8 * 64).reshape(8, 64).cpu()
    assert rel(s, qd.mean[None] + eps @ root) <= 1e-12
    # dense and iterative states describe the same distribution: the same noise E alone does not pin the sample (F differs), the mean does
    assert rel(it.q_v().mean, qd.mean) <= 1e-7
    # no sampler: the gridded q_v() of the Gridded* classes, posterior(x*), a plain distribution; too large a dense state
    with pytest.raises(NotImplementedError, match="joint samples"):
        full.posterior(torch.tensor(Xf[:5])).sample()
    with pytest.raises(NotImplementedError, match="joint samples"):
        MultivariateNormal(torch.zeros(3), torch.ones(3)).sample()
    gv = GriddedMatern12VFFGP(torch.tensor(Xf), torch.tensor(yf), 4, (-0.1, 1.1), (-0.1, 1.1), 8, (0, 1), (0, 1), engine=engine).to(torch.float64)
    with pytest.raises(NotImplementedError, match="joint samples"):
        gv.q_v().sample()
    assert gv.q_u().sample(torch.Size([2]), seed=1).shape == (2, gv.q_u().mean.numel())
    big = MultivariateNormal(torch.zeros(4097), torch.ones(4097), cov_fn=lambda: torch.eye(4097, dtype=torch.float64))
    big._sample_fn = de._dense_sampler(big)
    with pytest.raises(NotImplementedError, match="solver='iterative'"):
        big.sample()
