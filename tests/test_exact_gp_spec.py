"""CPU tests of the exact-GP specification (tests/exact_gp_spec.py) and of the C-ABI surface of the exact entries (no GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_gp_spec as E
import general_z_spec as S
from oracle import dense as D

THETA = [0.3, 0.25, 1.3, 0.8, 0.05]
KINDS = ["matern12", "matern32", "matern52", "rbf"]


def _data(N, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.random((N, 2))
    y = D.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(N)
    return torch.tensor(X), torch.tensor(y)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_literal_q_v_identity():
    """The reference's q_v covariance as written (:177-191) equals Kvv + Kvx Kxv / v (P^-1 = Kxx^-1 + I / v): N = 40 Matern-1/2
    points, where Kxx can still be inverted without noise."""
    X, y = _data(40)
    th = torch.tensor(THETA, dtype=torch.float64)
    mesh = torch.linspace(0, 1, 7).double()
    kinds = ("matern12", "matern12")
    cov, Kxx = E.q_v_cov_as_written(kinds, X, th, mesh, mesh)
    print("cond(Kxx) =", float(torch.linalg.cond(Kxx)))
    C1, C2, kd1, kd2 = E.b0_operands(X, mesh, mesh, th)
    _, var = E.q_v(E.state(kinds, X, th, y), C1, C2, kd1, kd2, literal=True)
    r = rel(torch.diagonal(cov).numpy(), var.numpy())
    print("literal identity, diagonal:", r)
    assert r <= 1e-10
    s, v = th[2] * th[3], th[4]
    F = s * (C1[:, None, :] * C2[None, :, :]).reshape(-1, 40)
    one = torch.tensor(1.0, dtype=torch.float64)
    Kvv = s * torch.kron(D.b0_Kuu_along_dim(6, mesh[1] - mesh[0], th[0], one), D.b0_Kuu_along_dim(6, mesh[1] - mesh[0], th[1], one))
    r = rel(cov.numpy(), (Kvv + F @ F.T / v).numpy())
    print("literal identity, full covariance:", r)
    assert r <= 1e-10


@pytest.mark.parametrize("kind", KINDS)
def test_analytic_gradient_matches_autograd(kind):
    X, y = _data(90, seed=1)
    th = torch.tensor(THETA, dtype=torch.float64, requires_grad=True)
    val, eps = E.mll((kind, kind), X, th, y)
    (g,) = torch.autograd.grad(val, th)
    ga = E.analytic_grad((kind, kind), X, th, y)
    assert eps == 0.0
    r = float(((ga - g).abs() / g.abs()).max())
    print(kind, "analytic vs autograd, worst component:", r)
    assert r <= 1e-10


def test_analytic_gradient_mixed_kinds():
    X, y = _data(90, seed=2)
    th = torch.tensor(THETA, dtype=torch.float64, requires_grad=True)
    kinds = ("matern32", "rbf")
    (g,) = torch.autograd.grad(E.mll(kinds, X, th, y)[0], th)
    assert float(((E.analytic_grad(kinds, X, th, y) - g).abs() / g.abs()).max()) <= 1e-10


@pytest.mark.parametrize("N", [150, 400])
def test_collapsed_bound_with_z_equal_x_is_the_exact_mll(N):
    """Link to the existing specification: with Z = X the Titsias bound is tight."""
    X, y = _data(N, seed=3)
    th = torch.tensor(THETA, dtype=torch.float64)
    kinds = ("matern12", "matern12")
    e, jit = S.elbo(kinds, X, th, y, X=X)
    m, eps = E.mll(kinds, X, th, y)
    print(N, "elbo(Z = X) vs mll:", abs(e.item() - m.item()) / abs(m.item()), "jitter", jit, eps)
    assert jit == 0.0 and eps == 0.0
    assert abs(e.item() - m.item()) <= 1e-10 * abs(m.item())


def test_sparse_bound_stays_below_the_exact_mll():
    X, y = _data(400, seed=3)
    th = torch.tensor(THETA, dtype=torch.float64)
    kinds = ("matern12", "matern12")
    Z = torch.tensor(np.random.default_rng(4).random((60, 2)))
    e, _ = S.elbo(kinds, Z, th, y, X=X)
    m, _ = E.mll(kinds, X, th, y)
    assert e.item() < m.item()


def test_posterior_at_the_data_and_state():
    """posterior(X) mean = K alpha and the predictive variance stays above the noise floor's share: the spec's own consistency."""
    X, y = _data(60, seed=5)
    th = torch.tensor(THETA, dtype=torch.float64)
    kinds = ("matern52", "matern52")
    st = E.state(kinds, X, th, y)
    mean, cov = E.posterior(st, kinds, X, th, X)
    K = st["s"] * E.K0(kinds, X, th)
    assert rel(mean.numpy(), (K @ st["alpha"]).numpy()) <= 1e-12
    # K - K Sigma^-1 K = v (I - v Sigma^-1): positive semi-definite with diagonal below v
    d = torch.diagonal(cov)
    assert bool((d > 0).all()) and bool((d < st["v"]).all())


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from variational_gridded_gaussian_processes_amd import _lib
    return _lib.load()


EXACT = ["vggp_exact_plan", "vggp_exact_step", "vggp_exact_posterior", "vggp_exact_posterior_cov", "vggp_exact_readout"]


def test_exact_symbols_exported_bound_and_null_safe(lib):
    from variational_gridded_gaussian_processes_amd import _lib
    for name in EXACT:
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name) is not None
    x = (C.c_double * 4)(0.1, 0.2, 0.3, 0.4)
    th = (C.c_double * 5)(*THETA)
    out, grad = C.c_double(), (C.c_double * 5)()
    assert lib.vggp_exact_plan(None, 0, 0, x, x, 4) < 0
    assert b"null context" in lib.vggp_last_error()
    assert lib.vggp_exact_step(None, None, th, C.byref(out), grad, None, None) < 0
    assert lib.vggp_exact_posterior(None, None, None, 3, None, None, None) < 0
    assert lib.vggp_exact_posterior_cov(None, None, None, 3, None, None) < 0
    assert lib.vggp_exact_readout(None, None, 2, None, 2, None, None, None, None, 0, None) < 0


def test_exact_models_are_importable_without_a_gpu():
    from variational_gridded_gaussian_processes_amd import exact
    for name in ("Matern12GP", "Matern32GP", "Matern52GP", "RBFGP", "GriddedMatern12ExactGP"):
        assert hasattr(exact, name)
    from variational_gridded_gaussian_processes_amd import Engine
    for name in ("exact_plan", "exact_step", "exact_posterior", "exact_posterior_cov", "exact_readout"):
        assert callable(getattr(Engine, name))
