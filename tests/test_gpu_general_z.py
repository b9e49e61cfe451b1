"""GriddedMatern12SVGP with general (non-grid) inducing points on the MI355X: the paired path (VGGP_FLAG_PAIRED_Z) against the
dense restatement (tests/test_general_z_spec.py DensePaired) and the M-space specification (tests/general_z_spec.py)."""

import numpy as np
import pytest
import torch

import general_z_spec as S
from oracle import dense as D
from test_general_z_spec import DensePaired

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _model(X, y, Z, engine, **kw):
    from variational_gridded_gaussian_processes_amd.models import GriddedMatern12SVGP
    return GriddedMatern12SVGP(torch.tensor(X), torch.tensor(y), torch.as_tensor(Z), 10, (0, 1), (0, 1), engine=engine, **kw).to(torch.float64)


def _raw_grad(model):
    return np.array([model.kernel_1.base_kernel.raw_lengthscale.grad.item(), model.kernel_2.base_kernel.raw_lengthscale.grad.item(),
                     model.kernel_1.raw_outputscale.grad.item(), model.kernel_2.raw_outputscale.grad.item(),
                     model.likelihood.raw_noise.grad.item()])


def _raw(model):
    return torch.tensor([model.kernel_1.base_kernel.raw_lengthscale.item(), model.kernel_2.base_kernel.raw_lengthscale.item(),
                         model.kernel_1.raw_outputscale.item(), model.kernel_2.raw_outputscale.item(),
                         model.likelihood.raw_noise.item()], dtype=torch.float64)


def _compare(model, X, y, Z, tol=1e-7, tol_z=1e-6, mask=None):
    model.zero_grad()
    loss = -model._elbo()
    loss.backward()
    dm = DensePaired(X, y, "matern12", Z, raw=_raw(model), mask=mask)
    e_d, g_d, gz_d = dm.elbo_grads()
    assert abs(-loss.item() - e_d.item()) <= tol * abs(e_d.item())
    assert rel(-_raw_grad(model), g_d.numpy()) <= tol
    assert rel(-model.Z.grad.numpy(), gz_d.numpy()) <= tol_z
    qu, qd = model.q_u(), dm.q_v()
    assert rel(qu.mean.numpy(), qd.mean.detach().numpy()) <= tol
    assert rel(qu.variance.numpy(), qd.variance.detach().numpy()) <= tol
    assert rel(qu.covariance_matrix.numpy(), qd.covariance_matrix.detach().numpy()) <= tol
    for literal in (True, False):
        qv, qvd = model.q_v(literal=literal), dm.q_v_paired(model.b0_mesh_1.double(), model.b0_mesh_2.double(), literal=literal)
        assert rel(qv.mean.numpy(), qvd.mean.detach().numpy()) <= tol
        assert rel(qv.variance.numpy(), qvd.variance.detach().numpy()) <= tol
    xs = torch.tensor(np.random.default_rng(5).random((50, 2)))
    p, pd = model.posterior(xs), dm.posterior(xs)
    assert rel(p.mean.numpy(), pd.mean.detach().numpy()) <= tol
    assert rel(p.variance.numpy(), pd.variance.detach().numpy()) <= tol
    assert rel(p.covariance_matrix.numpy(), pd.covariance_matrix.detach().numpy()) <= tol
    pp = model.posterior_predictive(xs)
    assert rel(pp.variance.numpy(), (pd.variance + dm.theta()[4]).detach().numpy()) <= tol


def test_notebook5_random_z(engine):
    """Notebook 5 (cells 12-13): 25 x 25 gen_2d grid, Z = rand(100, 2), 10 splines."""
    X, y, _, _ = D.gen_grid(25, 25)
    Z = np.random.default_rng(0).random((100, 2))
    model = _model(X, y, Z, engine)
    assert model.inducing == "general" and model.Z.requires_grad
    _compare(model, X, y, Z)


def test_track_and_masked_grid(engine):
    from variational_gridded_gaussian_processes_amd import datagen
    rng = np.random.default_rng(1)
    lon, lat = np.linspace(0, 1, 120), np.linspace(0, 1, 110)
    field = D.latent_2d(lon[None, :], lat[:, None])
    tx, ty, tv = datagen.track_points(field, lon, lat, 2, 0.4)
    P = np.unique(np.stack([tx, ty, tv], axis=1), axis=0)[:2000]
    X, y = P[:, :2].copy(), P[:, 2] + 0.05 * rng.standard_normal(len(P))
    Z = rng.random((150, 2))
    _compare(_model(X, y, Z, engine), X, y, Z)
    # a 30 x 30 grid with 30 % holes
    Xg, yg, _, _ = D.gen_grid(30, 30)
    keep = rng.random(900) > 0.3
    Z = rng.random((60, 2))
    _compare(_model(Xg[keep], yg[keep], Z, engine), Xg[keep], yg[keep], Z)


@pytest.mark.parametrize("kind", ["matern32", "matern52", "rbf"])
def test_engine_kinds_and_set_inducing(engine, kind):
    rng = np.random.default_rng(2)
    X = rng.random((700, 2))
    y = D.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(700)
    Z = rng.random((60, 2))
    # (RBF: a shorter lengthscale keeps Kuu of 60 random points well conditioned, as in the CPU spec test)
    theta = [0.06, 0.07, 0.9, 1.1, 0.01] if kind == "rbf" else [0.15, 0.2, 0.9, 1.1, 0.01]
    dev = engine.device
    yt = torch.tensor(y, device=dev)
    engine.plan_paired(kind, Z, X[:, 0], X[:, 1], scattered=True)
    e, g, info = engine.elbo_step_scattered(yt, float((yt * yt).sum()), theta)
    gz1, gz2 = engine.zgrad_scattered(yt)
    th = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    Zt = torch.tensor(Z, requires_grad=True)
    es, jit = S.elbo((kind, kind), Zt, th, torch.tensor(y), X=torch.tensor(X))
    gs, gzs = torch.autograd.grad(es, [th, Zt])
    assert info["jitter"][0] == jit
    assert abs(e - es.item()) <= 1e-7 * abs(es.item())
    assert rel(g, gs.numpy()) <= 1e-6
    assert rel(torch.stack([gz1, gz2], 1).cpu().numpy(), gzs.numpy()) <= 1e-6
    # moving Z in place == a fresh plan
    Z2 = Z + 0.01 * rng.standard_normal(Z.shape)
    engine.set_inducing(0, Z2[:, 0])
    engine.set_inducing(1, Z2[:, 1])
    e1, g1, _ = engine.elbo_step_scattered(yt, float((yt * yt).sum()), theta)
    engine.plan_paired(kind, Z2, X[:, 0], X[:, 1], scattered=True)
    e2, g2, _ = engine.elbo_step_scattered(yt, float((yt * yt).sum()), theta)
    assert e1 == e2 and np.array_equal(g1, g2)


def test_general_on_cartesian_z_equals_grid_path(engine):
    X, y, _, _ = D.gen_grid(128, 96)
    z1, z2 = torch.linspace(0.02, 0.98, 12).double(), torch.linspace(0.03, 0.97, 10).double()
    Z = torch.cartesian_prod(z1, z2)
    mg = _model(X, y, Z, engine, inducing="grid")
    mp = _model(X, y, Z, engine, inducing="general", train_z=False)
    assert mg.inducing == "grid" and mp.inducing == "general"
    outs = []
    for m in (mg, mp):
        m.zero_grad()
        loss = -m._elbo()
        loss.backward()
        outs.append((loss.item(), _raw_grad(m), m.q_v()))
    assert abs(outs[0][0] - outs[1][0]) <= 1e-8 * abs(outs[0][0])
    assert rel(outs[1][1], outs[0][1]) <= 1e-8
    assert rel(outs[1][2].mean.numpy(), outs[0][2].mean.numpy()) <= 1e-8
    assert rel(outs[1][2].variance.numpy(), outs[0][2].variance.numpy()) <= 1e-8


@pytest.mark.parametrize("shape", ["grid512_M1024", "scattered100k_M500"])
def test_at_size_against_spec(engine, shape):
    rng = np.random.default_rng(4)
    theta = [0.3, 0.25, 0.8, 1.2, 0.01]
    dev = engine.device
    if shape.startswith("grid"):
        n, M = 512, 1024
        X, y, x1, x2 = D.gen_grid(n, n)
        Z = rng.random((M, 2))
        Y = torch.tensor(y, device=dev).reshape(n, n).contiguous()
        engine.plan_paired("matern12", Z, x1, x2)
        step = lambda: engine.elbo_step(Y, float((Y * Y).sum()), theta)
        zg = lambda: engine.zgrad(Y)
        spec_kw = dict(grid=(torch.tensor(x1), torch.tensor(x2)))
        ys = torch.tensor(y).reshape(n, n)
    else:
        N, M = 100_000, 500
        X = rng.random((N, 2))
        y = D.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(N)
        Z = rng.random((M, 2))
        yt = torch.tensor(y, device=dev)
        engine.plan_paired("matern12", Z, X[:, 0], X[:, 1], scattered=True)
        step = lambda: engine.elbo_step_scattered(yt, float((yt * yt).sum()), theta)
        zg = lambda: engine.zgrad_scattered(yt)
        spec_kw = dict(X=torch.tensor(X))
        ys = torch.tensor(y)
    e, g, _ = step()
    gz = torch.stack(zg(), 1).cpu().numpy()
    e2, g2, _ = step()
    gz2 = torch.stack(zg(), 1).cpu().numpy()
    assert e == e2 and np.array_equal(g, g2) and np.array_equal(gz, gz2)        # bitwise repeatable
    th = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    Zt = torch.tensor(Z, requires_grad=True)
    es, _ = S.elbo(("matern12", "matern12"), Zt, th, ys, **spec_kw)
    gs, gzs = torch.autograd.grad(es, [th, Zt])
    assert abs(e - es.item()) <= 1e-7 * abs(es.item())
    assert rel(g, gs.numpy()) <= 1e-6
    assert rel(gz, gzs.numpy()) <= 1e-6


def test_training_notebook5(engine):
    X, y, _, _ = D.gen_grid(25, 25)
    Z = np.random.default_rng(0).random((100, 2))
    model = _model(X, y, Z, engine)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = -model._elbo()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0]
    assert float((model.Z.detach() - torch.tensor(Z)).abs().max()) > 1e-3
    _compare(model, X, y, model.Z.detach().numpy().copy())


def test_errors(engine):
    from variational_gridded_gaussian_processes_amd import Engine, _lib
    from variational_gridded_gaussian_processes_amd._lib import VggpError
    rng = np.random.default_rng(6)
    X = rng.random((300, 2))
    y = torch.tensor(D.latent_2d(X[:, 0], X[:, 1]), device=engine.device)
    theta = [0.3, 0.3, 1.0, 1.0, 0.01]
    # multi-rank context (host-callback transport): the paired step is single-rank only
    e2 = Engine(0, n_ranks=2, rank=0, allreduce=lambda buf: None)
    e2.plan_paired("matern12", rng.random((20, 2)), X[:, 0], X[:, 1], scattered=True)
    with pytest.raises(VggpError) as ei:
        e2.elbo_step_scattered(y, 1.0, theta)
    assert ei.value.code == _lib.VGGP_EINVAL and "single-rank" in str(ei.value)
    e2.close()
    # Kronecker read-outs after a paired step
    engine.plan_paired("matern12", rng.random((20, 2)), X[:, 0], X[:, 1], scattered=True)
    engine.elbo_step_scattered(y, float((y * y).sum()), theta)
    for call in (lambda: engine.qv(),
                 lambda: engine.readout(torch.ones(3, 20), torch.ones(3, 20), torch.ones(3), torch.ones(3))):
        with pytest.raises(VggpError) as ei:
            call()
        assert ei.value.code == _lib.VGGP_EINVAL and "PAIRED_Z" in str(ei.value)
    # M beyond the dense solver
    with pytest.raises(VggpError) as ei:
        engine.plan_paired("matern12", rng.random((16385, 2)), X[:, 0], X[:, 1], scattered=True)
    assert ei.value.code == _lib.VGGP_EINVAL
    # two identical inducing points: Kuu is singular, the jitter schedule steps in exactly as in the dense restatement
    Z = rng.random((30, 2))
    Z[1] = Z[0]
    theta = [0.3, 0.3, 0.5, 0.5, 0.01]          # s = 0.25: the duplicated pivot is exactly zero in both factorisations
    engine.plan_paired("matern12", Z, X[:, 0], X[:, 1], scattered=True)
    e, _, info = engine.elbo_step_scattered(y, float((y * y).sum()), theta)
    dm = DensePaired(X, y.cpu().numpy(), "matern12", Z, theta=theta)
    ed = dm._elbo().item()
    assert info["jitter"][0] == dm._jit > 0
    assert abs(e - ed) <= 1e-6 * abs(ed)
