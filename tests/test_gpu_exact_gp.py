"""The exact GP on the MI355X (vggp_exact_*, exact.py) against its specification (tests/exact_gp_spec.py).  Points
default_rng(seed).random((N, 2)), y = latent_2d + 0.05 noise, theta = (0.3, 0.25, 1.3, 0.8, 0.05): cond(Sigma) <= 5e4 up to N = 1500 and
two float64 routes to every quantity agree within 6e-11 on the CPU, so the standing C-ABI tolerance 1e-7 holds with room (relative
for scalars, max-norm `rel` for vectors)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import exact_gp_spec as E
from oracle import dense as D

pytestmark = pytest.mark.gpu

THETA = [0.3, 0.25, 1.3, 0.8, 0.05]
KINDS = ["matern12", "matern32", "matern52", "rbf"]
TOL = 1e-7


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@functools.lru_cache(maxsize=None)
def _data(N, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.random((N, 2))
    y = D.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(N)
    return X, y


@functools.lru_cache(maxsize=None)
def _spec(kinds, N, seed=0):
    """(mll, grad[5] wrt theta, jitter, read-out state) of the specification, computed once per case."""
    X, y = _data(N, seed)
    Xt, yt = torch.tensor(X), torch.tensor(y)
    th = torch.tensor(THETA, dtype=torch.float64, requires_grad=True)
    val, eps = E.mll(kinds, Xt, th, yt)
    (g,) = torch.autograd.grad(val, th)
    return val.item(), g.numpy(), eps, E.state(kinds, Xt, th.detach(), yt)


def _step(engine, kinds, N, seed=0):
    X, y = _data(N, seed)
    engine.exact_plan(kinds[0], kinds[1], X[:, 0], X[:, 1])
    yd = torch.tensor(y, device=engine.device)
    return engine.exact_step(yd, THETA), yd


@pytest.mark.parametrize("N", [50, 130, 333])
@pytest.mark.parametrize("kind", KINDS)
def test_step(engine, kind, N):
    """N = 50: below one 64-tile; 130: across the 128-wide Cholesky panel with a ragged tile; 333: several panels."""
    (mll, g, info), _ = _step(engine, (kind, kind), N)
    m_s, g_s, eps, _ = _spec((kind, kind), N)
    print(kind, N, "mll", abs(mll - m_s) / abs(m_s), "grad", np.abs(g - g_s) / np.abs(g_s))
    assert info["jitter"][0] == 0.0 and eps == 0.0
    assert abs(mll - m_s) <= TOL * abs(m_s)
    assert np.all(np.abs(g - g_s) <= TOL * np.abs(g_s))


def test_step_mixed_kinds(engine):
    kinds = ("matern32", "rbf")
    (mll, g, info), _ = _step(engine, kinds, 130)
    m_s, g_s, eps, _ = _spec(kinds, 130)
    assert info["jitter"][0] == 0.0 and eps == 0.0
    assert abs(mll - m_s) <= TOL * abs(m_s)
    assert np.all(np.abs(g - g_s) <= TOL * np.abs(g_s))


def _set_theta(model):
    model.kernel_1.base_kernel.lengthscale = THETA[0]
    model.kernel_2.base_kernel.lengthscale = THETA[1]
    model.kernel_1.outputscale = THETA[2]
    model.kernel_2.outputscale = THETA[3]
    model.likelihood.noise = THETA[4]


def _raw(model):
    return torch.tensor([model.kernel_1.base_kernel.raw_lengthscale.item(), model.kernel_2.base_kernel.raw_lengthscale.item(),
                         model.kernel_1.raw_outputscale.item(), model.kernel_2.raw_outputscale.item(),
                         model.likelihood.raw_noise.item()], dtype=torch.float64)


def _raw_grad(model):
    return np.array([model.kernel_1.base_kernel.raw_lengthscale.grad.item(), model.kernel_2.base_kernel.raw_lengthscale.grad.item(),
                     model.kernel_1.raw_outputscale.grad.item(), model.kernel_2.raw_outputscale.grad.item(),
                     model.likelihood.raw_noise.grad.item()])


def _model(name, engine, N=130, **kw):
    from variational_gridded_gaussian_processes_amd import exact
    X, y = _data(N)
    args = (10, (0, 1), (0, 1)) if name == "GriddedMatern12ExactGP" else ()
    m = getattr(exact, name)(torch.tensor(X), torch.tensor(y), *args, engine=engine, **kw).to(torch.float64)
    _set_theta(m)
    return m


@pytest.mark.parametrize("name,kind", [("Matern12GP", "matern12"), ("Matern32GP", "matern32"), ("Matern52GP", "matern52"),
                                       ("RBFGP", "rbf")])
def test_model_classes(engine, name, kind):
    N = 130
    model = _model(name, engine, N)
    X, y = _data(N)
    raw = _raw(model).requires_grad_(True)
    val, _ = E.mll((kind, kind), torch.tensor(X), D.constrained_from_raw(raw), torch.tensor(y))
    (g_raw,) = torch.autograd.grad(-val / N, raw)
    model.zero_grad()
    loss = -model.mll()
    loss.backward()
    assert abs(loss.item() + val.item() / N) <= TOL * abs(val.item() / N)
    assert np.all(np.abs(_raw_grad(model) - g_raw.numpy()) <= TOL * np.abs(g_raw.numpy()))
    lml = model.log_marginal_likelihood().item()
    assert abs(model.mll().item() * N - lml) <= 1e-14 * abs(lml)
    assert set(n for n, _ in model.named_parameters()) == {"likelihood.raw_noise", "kernel_1.raw_outputscale", "kernel_2.raw_outputscale",
                                                           "kernel_1.base_kernel.raw_lengthscale", "kernel_2.base_kernel.raw_lengthscale"}
    assert model.train_inputs[0].shape == (N, 2) and model.train_targets.shape == (N,)
    assert model.prior(torch.tensor(X[:5])).covariance_matrix.shape == (5, 5)


@pytest.mark.parametrize("ns", [50, 70])
@pytest.mark.parametrize("name,kind", [("Matern12GP", "matern12"), ("Matern32GP", "matern32"), ("Matern52GP", "matern52"),
                                       ("RBFGP", "rbf")])
def test_posterior(engine, name, kind, ns):
    N = 130
    model = _model(name, engine, N)
    X, _ = _data(N)
    xs = torch.tensor(np.random.default_rng(5).random((ns, 2)))
    th = torch.tensor(THETA, dtype=torch.float64)
    mean_s, cov_s = E.posterior(_spec((kind, kind), N)[3], (kind, kind), torch.tensor(X), th, xs)
    p = model.posterior(xs)
    assert rel(p.mean.numpy(), mean_s.numpy()) <= TOL
    assert rel(p.variance.numpy(), torch.diagonal(cov_s).numpy()) <= TOL
    assert rel(p.covariance_matrix.numpy(), cov_s.numpy()) <= TOL
    pp = model.posterior_predictive(xs)
    assert rel(pp.variance.numpy(), (torch.diagonal(cov_s) + THETA[4]).numpy()) <= TOL
    assert torch.equal(pp.mean, p.mean)


def test_gridded_readout(engine):
    N = 333
    model = _model("GriddedMatern12ExactGP", engine, N)
    X, _ = _data(N)
    kinds = ("matern12", "matern12")
    st = _spec(kinds, N)[3]
    th = torch.tensor(THETA, dtype=torch.float64)
    ops = E.b0_operands(torch.tensor(X), model.b0_mesh_1.double(), model.b0_mesh_2.double(), th)
    qs = {}
    for literal in (True, False):
        mean_s, var_s = E.q_v(st, *ops, literal=literal)
        qv = qs[literal] = model.q_v(literal=literal)
        assert qv.mean.shape == (100,)
        assert rel(qv.mean.numpy(), mean_s.numpy()) <= TOL
        assert rel(qv.variance.numpy(), var_s.numpy()) <= TOL
        with pytest.raises(NotImplementedError):
            qv.covariance_matrix
    assert bool((qs[False].variance > 0).all())
    cells = [3, 57, 99, 10]
    for literal in (True, False):
        qc = model.q_v_cells(cells, literal=literal)
        assert torch.equal(qc.mean, qs[literal].mean[cells]) and torch.equal(qc.variance, qs[literal].variance[cells])
    # C-ABI level: a non-square cell grid
    m1 = torch.linspace(0, 1, 8).double()
    m2 = torch.linspace(0, 1, 13).double()
    C1, C2, kd1, kd2 = E.b0_operands(torch.tensor(X), m1, m2, th)
    for literal in (True, False):
        mean, var = engine.exact_readout(C1, C2, kd1, kd2, literal=literal)
        mean_s, var_s = E.q_v(st, C1, C2, kd1, kd2, literal=literal)
        assert mean.shape == (7, 12)
        assert rel(mean.reshape(-1).cpu().numpy(), mean_s.numpy()) <= TOL
        assert rel(var.reshape(-1).cpu().numpy(), var_s.numpy()) <= TOL


def test_matches_the_paired_scattered_step_with_z_equal_x(engine):
    N = 150
    X, y = _data(N)
    (mll, _, _), yd = _step(engine, ("matern12", "matern12"), N)
    engine.plan_paired("matern12", X, X[:, 0], X[:, 1], scattered=True)
    e, _, info = engine.elbo_step_scattered(yd, float((yd * yd).sum()), THETA)
    print("exact vs paired(Z = X):", abs(mll - e) / abs(mll), "paired jitter", info["jitter"][0])
    assert abs(mll - e) <= TOL * abs(mll)


def test_repeatable_bitwise(engine):
    (m1, g1, _), yd = _step(engine, ("matern52", "matern52"), 333)
    m2, g2, _ = engine.exact_step(yd, THETA)
    assert m1 == m2 and np.array_equal(g1, g2)
    xs = torch.tensor(np.random.default_rng(5).random((70, 2)))
    a, b = engine.exact_posterior(xs), engine.exact_posterior(xs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_isolation_from_the_planned_model(engine):
    rng = np.random.default_rng(7)
    Xs = rng.random((300, 2))
    ys = torch.tensor(D.latent_2d(Xs[:, 0], Xs[:, 1]) + 0.05 * rng.standard_normal(300), device=engine.device)
    z = np.linspace(0.0, 1.0, 6)
    th = [0.2, 0.25, 0.9, 1.1, 0.02]

    def sparse_step():
        engine.plan("matern12", "points", z, Xs[:, 0], "matern12", "points", z, Xs[:, 1], scattered=True)
        return engine.elbo_step_scattered(ys, float((ys * ys).sum()), th)
    sparse_step()
    mean0, var0 = [t.clone() for t in engine.qv_masked()]
    sparse_step()
    (mll, _, _), _ = _step(engine, ("matern12", "matern12"), 130)
    xs = torch.tensor(rng.random((20, 2)))
    pm, pv = engine.exact_posterior(xs)
    mean1, var1 = engine.qv_masked()
    assert torch.equal(mean0, mean1) and torch.equal(var0, var1)
    # ... and the exact state survives a later plan of the sparse model
    sparse_step()
    pm2, pv2 = engine.exact_posterior(xs)
    assert torch.equal(pm, pm2) and torch.equal(pv, pv2)
    assert abs(mll - _spec(("matern12", "matern12"), 130)[0]) <= TOL * abs(mll)


def test_errors(engine):
    from variational_gridded_gaussian_processes_amd import VggpError, _lib
    X, y = _data(50)
    engine.exact_plan("matern12", "matern12", X[:, 0], X[:, 1])
    xs = torch.tensor(X[:4])
    with pytest.raises(VggpError) as ei:          # read-out before a step on the current plan
        engine.exact_posterior(xs)
    assert ei.value.code == _lib.VGGP_ESTATE
    yd = torch.tensor(y, device=engine.device)
    with pytest.raises(VggpError) as ei:
        engine.exact_step(yd, [0.3, 0.25, 1.3, 0.8, 0.0])
    assert ei.value.code == _lib.VGGP_EINVAL
    free0 = torch.cuda.mem_get_info(engine.device)[0]
    big = np.zeros(16385)
    with pytest.raises(VggpError) as ei:          # refused before anything is allocated
        engine.exact_plan("matern12", "matern12", big, big)
    assert ei.value.code == _lib.VGGP_EINVAL
    assert torch.cuda.mem_get_info(engine.device)[0] >= free0
    engine.exact_step(yd, THETA)                  # (the refused plan left the current one alone)
    with pytest.raises(VggpError) as ei:
        engine.exact_posterior_cov(torch.zeros(8193, 2, dtype=torch.float64))
    assert ei.value.code == _lib.VGGP_EINVAL
    with pytest.raises(VggpError) as ei:
        engine.exact_plan("matern12", "matern12", np.array([0.1, np.nan]), np.array([0.1, 0.2]))
    assert ei.value.code == _lib.VGGP_EINVAL


def test_single_point(engine):
    X, y = np.array([[0.3, 0.6]]), np.array([0.7])
    engine.exact_plan("matern12", "matern12", X[:, 0], X[:, 1])
    mll, g, info = engine.exact_step(torch.tensor(y, device=engine.device), THETA)
    th = torch.tensor(THETA, dtype=torch.float64, requires_grad=True)
    val, _ = E.mll(("matern12", "matern12"), torch.tensor(X), th, torch.tensor(y))
    (gs,) = torch.autograd.grad(val, th)
    assert abs(mll - val.item()) <= TOL * abs(val.item())
    assert rel(g, gs.numpy()) <= TOL          # (the lengthscale components are exactly zero at N = 1)
    assert g[0] == 0.0 and g[1] == 0.0
