"""Read-outs of the iterative masked step on the GPU: vggp_qv_masked_iter / vggp_posterior_masked_iter (block PCG on rank-one
right-hand sides, no M x M matrix) against the dense masked oracle, the dense GPU step, the Kronecker path, and through the model
classes (solver="iterative").  Tolerances as the dense masked read-outs in test_gpu_elbo.py: means 1e-7, variances 1e-6 of the
largest entry."""
import functools

import numpy as np
import pytest
import torch

from oracle import dense as D
from oracle import kron as Kr
from variational_gridded_gaussian_processes_amd import _lib
from variational_gridded_gaussian_processes_amd import datagen as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
THETA = [0.2, 0.3, 1.0, 0.8, 0.01]


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


N = 96
BASES = {"b0-matern12": ("b0", "matern12", np.linspace(0, 1, 13)), "points-matern32": ("points", "matern32", np.linspace(0, 1, 10)),
         "points-rbf": ("points", "rbf", np.linspace(0, 1, 10)), "b1-matern12": ("b1", "matern12", np.linspace(0, 1, 12))}
XS = np.random.default_rng(9).uniform(0, 1, (70, 2))


@functools.lru_cache(maxsize=None)
def mask96(name):
    return (np.random.default_rng(1).uniform(size=(N, N)) < 0.7).astype(np.float64) if name == "bernoulli" else G.track_mask(N, N, 2, 0.5)


@functools.lru_cache(maxsize=None)
def oracle96(bname, mname):
    """The dense masked oracle's read-outs, computed once per case."""
    basis, kind, g = BASES[bname]
    _, y, x1, x2 = D.gen_grid(N, N)
    f1, f2 = Kr.Factor(basis, kind, g, x1), Kr.Factor(basis, kind, g, x2)
    ref = Kr.elbo_step_masked(y.reshape(N, N), mask96(mname), f1, f2, THETA)
    return Kr.q_v_masked(ref, f1, f2), Kr.posterior_masked(ref, f1, f2, XS)


def iter_step96(engine, bname, mname):
    basis, kind, g = BASES[bname]
    _, y, x1, x2 = D.gen_grid(N, N)
    Wn = mask96(mname)
    engine.plan(kind, basis, g, x1, kind, basis, g, x2)
    W = dev(Wn)
    Ym = dev(y.reshape(N, N)) * W
    nobs = float(Wn.sum())
    yy = engine.sumsq(Ym)
    out = engine.elbo_step_masked_iter(Ym, W, nobs, yy, THETA, n_probes=16)
    return W, Ym, nobs, yy, out


# the e_d = -1 scaling of q(v) (inter-domain features) is covered by the B1 case
CASES = [(b, m) for b in ("b0-matern12", "points-matern32", "points-rbf") for m in ("bernoulli", "track")] + [("b1-matern12", "bernoulli")]


@pytest.mark.parametrize("bname,mname", CASES, ids=lambda v: v)
def test_readouts_vs_dense_masked_oracle(engine, bname, mname):
    (rm, rv), (om, ov) = oracle96(bname, mname)
    W, _, nobs, _, _ = iter_step96(engine, bname, mname)
    mean, var, info = engine.qv_masked_iter(W, nobs)
    pm, pv, pinfo = engine.posterior_masked_iter(dev(XS), W, nobs)
    errs = (rel(mean.cpu().numpy(), rm), rel(var.cpu().numpy(), rv.reshape(-1)), rel(pm.cpu().numpy(), om), rel(pv.cpu().numpy(), ov))
    print(f"{bname}-{mname}: q(v) mean {errs[0]:.1e} var {errs[1]:.1e}; posterior mean {errs[2]:.1e} var {errs[3]:.1e}; "
          f"iterations {info['rounds'][0]} / {pinfo['rounds'][0]}, solves {info['sweeps'][0]} / {pinfo['sweeps'][0]}")
    assert errs[0] <= 1e-7 and errs[2] <= 1e-7
    assert errs[1] <= 1e-6 and errs[3] <= 1e-6
    M = mean.numel()
    assert info["sweeps"][0] == -(-M // 64) and pinfo["sweeps"][0] == 2 and 0 < info["rounds"][0] < 60


def test_chunking_and_cell_subsets(engine):
    """block = 16 on 37 columns is three block solves with a ragged last one.  The results are BITWISE equal to those of block = 64
    (one solve), and a list of cells gives the same bits as the same entries of the all-cell call: a column's numbers do not depend on
    its neighbours in the block -- every GEMM of the solve reduces over the same index in the same order whatever the block width,
    the per-column dot products run in a fixed order, and each column stops on its own residual."""
    W, _, nobs, _, _ = iter_step96(engine, "b0-matern12", "bernoulli")
    xs = dev(XS[:37])
    cells = np.random.default_rng(4).choice(144, size=37, replace=False)
    m16, v16, i16 = engine.posterior_masked_iter(xs, W, nobs, block=16)
    m64, v64, i64 = engine.posterior_masked_iter(xs, W, nobs, block=64)
    assert (i16["sweeps"][0], i64["sweeps"][0]) == (3, 1)
    print("posterior block 16 vs 64:", rel(m16.cpu(), m64.cpu()), rel(v16.cpu(), v64.cpu()))
    assert torch.equal(m16, m64) and torch.equal(v16, v64)
    qm16, q16, j16 = engine.qv_masked_iter(W, nobs, cells=cells, block=16)
    qm64, q64, j64 = engine.qv_masked_iter(W, nobs, cells=cells, block=64)
    qm, qall, _ = engine.qv_masked_iter(W, nobs)
    assert (j16["sweeps"][0], j64["sweeps"][0]) == (3, 1)
    print("q(v) block 16 vs 64:", rel(q16.cpu(), q64.cpu()), "subset vs all:", rel(q16.cpu(), qall.cpu()[cells]))
    assert torch.equal(qm16, qm) and torch.equal(qm64, qm)              # the mean is the same two GEMMs in every call
    assert torch.equal(q16, q64)
    assert torch.equal(q16.cpu(), qall.cpu()[cells])
    mean_only, none, info = engine.qv_masked_iter(W, nobs, variance=False)
    assert none is None and torch.equal(mean_only, qm) and info["sweeps"][0] == 0


def test_readouts_vs_dense_gpu_step_at_M4096(engine):
    n, m = 256, 64
    _, y, x1, x2 = D.gen_grid(n, n)
    Wn = (np.random.default_rng(1).uniform(size=(n, n)) < 0.7).astype(np.float64)
    W = dev(Wn)
    Ym = dev(y.reshape(n, n)) * W
    nobs = float(Wn.sum())
    theta = [0.2, 0.2, 1.0, 1.0, 0.0025]
    mesh = np.linspace(0, 1, m + 1)
    rng = np.random.default_rng(11)
    cells = rng.choice(m * m, size=256, replace=False)
    xs = dev(rng.uniform(0, 1, (200, 2)))
    engine.plan("matern12", "b0", mesh, x1, "matern12", "b0", mesh, x2)
    yy = engine.sumsq(Ym)
    engine.elbo_step_masked(Ym, W, nobs, yy, theta)
    dm, dv = engine.qv_masked()
    dpm, dpv = engine.posterior_masked(xs)
    engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta, n_probes=16)
    im, iv, info = engine.qv_masked_iter(W, nobs, cells=cells)
    ipm, ipv, pinfo = engine.posterior_masked_iter(xs, W, nobs)
    errs = (rel(im.cpu(), dm.cpu()), rel(iv.cpu(), dv.cpu().reshape(-1)[cells]), rel(ipm.cpu(), dpm.cpu()), rel(ipv.cpu(), dpv.cpu()))
    print("M = 4096:", errs, info["rounds"], pinfo["rounds"])
    assert errs[0] <= 1e-7 and errs[2] <= 1e-7
    assert errs[1] <= 1e-6 and errs[3] <= 1e-6
    with pytest.raises(_lib.VggpError) as e:                   # the dense read-outs still need the dense step
        engine.qv_masked()
    assert e.value.code == _lib.VGGP_ESTATE


def test_readouts_beyond_the_dense_solver(engine):
    """M = 18496 > 16384: the dense step refuses.  With everything observed the preconditioner is exact (PCG converges at once) and
    the read-outs equal the Kronecker path's; with 30 % missing they are finite, positive and converge."""
    n, m = 512, 136
    _, y, x1, x2 = D.gen_grid(n, n)
    Yf = dev(y.reshape(n, n))
    ones = torch.ones_like(Yf)
    theta = [0.2, 0.2, 1.0, 1.0, 0.0025]
    mesh = np.linspace(0, 1, m + 1)
    rng = np.random.default_rng(12)
    cells = rng.choice(m * m, size=128, replace=False)
    xs = dev(rng.uniform(0, 1, (64, 2)))
    engine.plan("matern12", "b0", mesh, x1, "matern12", "b0", mesh, x2)
    yyf = engine.sumsq(Yf)
    with pytest.raises(_lib.VggpError):
        engine.elbo_step_masked(Yf, ones, float(n * n), yyf, theta)
    engine.elbo_step_masked_iter(Yf, ones, float(n * n), yyf, theta, n_probes=8)
    im, iv, info = engine.qv_masked_iter(ones, float(n * n), cells=cells)
    ipm, ipv, pinfo = engine.posterior_masked_iter(xs, ones, float(n * n))
    engine.elbo_step(Yf, yyf, theta)
    km, kv = engine.qv()
    kpm, kpv = engine.posterior(xs)
    errs = (rel(im.cpu(), km.cpu()), rel(iv.cpu(), kv.cpu().reshape(-1)[cells]), rel(ipm.cpu(), kpm.cpu()), rel(ipv.cpu(), kpv.cpu()))
    print("M = 18496, W = 1:", errs, info["rounds"], pinfo["rounds"])
    assert errs[0] <= 1e-7 and errs[2] <= 1e-7
    assert errs[1] <= 1e-6 and errs[3] <= 1e-6
    assert info["rounds"][0] <= 3 and pinfo["rounds"][0] <= 3
    Wn = (np.random.default_rng(1).uniform(size=(n, n)) < 0.7).astype(np.float64)
    W = dev(Wn)
    Ym = Yf * W
    engine.elbo_step_masked_iter(Ym, W, float(Wn.sum()), engine.sumsq(Ym), theta, n_probes=8)
    im, iv, info = engine.qv_masked_iter(W, float(Wn.sum()), cells=cells)
    ipm, ipv, pinfo = engine.posterior_masked_iter(xs, W, float(Wn.sum()))
    for t in (im, iv, ipm, ipv):
        assert bool(torch.isfinite(t).all())
    assert bool((iv > 0).all()) and bool((ipv > 0).all())
    assert info["rounds"][0] < 80 and pinfo["rounds"][0] < 80


def code_of(fn, *a, **kw):
    with pytest.raises(_lib.VggpError) as e:
        fn(*a, **kw)
    return e.value.code


def test_state_and_arguments(engine):
    from variational_gridded_gaussian_processes_amd import Engine
    basis, kind, g = BASES["b0-matern12"]
    _, y, x1, x2 = D.gen_grid(N, N)
    Wn = mask96("bernoulli")
    W = dev(Wn)
    Yf = dev(y.reshape(N, N))
    Ym = Yf * W
    nobs = float(Wn.sum())
    xs = dev(XS[:5])
    fresh = Engine(0)
    try:
        fresh.plan(kind, basis, g, x1, kind, basis, g, x2)                           # before any step
        assert code_of(fresh.qv_masked_iter, W, nobs) == _lib.VGGP_ESTATE
        assert code_of(fresh.posterior_masked_iter, xs, W, nobs) == _lib.VGGP_ESTATE
    finally:
        fresh.close()
    engine.plan(kind, basis, g, x1, kind, basis, g, x2)
    yy = engine.sumsq(Ym)
    engine.elbo_step_masked_iter(Ym, W, nobs, yy, THETA)
    engine.elbo_step_masked(Ym, W, nobs, yy, THETA)                                  # after a dense masked step
    assert code_of(engine.qv_masked_iter, W, nobs) == _lib.VGGP_ESTATE
    engine.elbo_step_masked_iter(Ym, W, nobs, yy, THETA)
    engine.elbo_step(Yf, engine.sumsq(Yf), THETA)                                    # after a full-grid step
    assert code_of(engine.posterior_masked_iter, xs, W, nobs) == _lib.VGGP_ESTATE
    engine.elbo_step_masked_iter(Ym, W, nobs, yy, THETA)
    engine.plan(kind, basis, g, x1, kind, basis, g, x2)                              # after plan
    assert code_of(engine.qv_masked_iter, W, nobs) == _lib.VGGP_ESTATE
    engine.elbo_step_masked_iter(Ym, W, nobs, yy, THETA)
    for bad in ([144], [-1], [3, 10 ** 12]):
        assert code_of(engine.qv_masked_iter, W, nobs, cells=bad) == _lib.VGGP_EINVAL
    assert code_of(engine.qv_masked_iter, W, nobs, cells=[3], block=65) == _lib.VGGP_EINVAL
    assert code_of(engine.posterior_masked_iter, xs, W, nobs, block=65) == _lib.VGGP_EINVAL
    _, v, _ = engine.qv_masked_iter(W, nobs, cells=[3])                              # (the refused calls left the state readable)
    assert bool(torch.isfinite(v).all())
    rng = np.random.default_rng(2)
    ps = rng.uniform(0, 1, (60, 2))
    engine.plan(kind, "points", np.linspace(0, 1, 6), ps[:, 0], kind, "points", np.linspace(0, 1, 6), ps[:, 1], scattered=True)
    w1 = torch.ones(60, 60, dtype=torch.float64, device=DEV)
    assert code_of(engine.qv_masked_iter, w1, 60.0) == _lib.VGGP_EINVAL
    assert code_of(engine.posterior_masked_iter, xs, w1, 60.0) == _lib.VGGP_EINVAL


def test_readouts_leave_the_next_step_unchanged(engine):
    """The read-outs work in a workspace of their own: the step after them reuses the kept preconditioner basis and returns the
    same bits as without them."""
    theta2 = [t * 1.01 for t in THETA]
    W, Ym, nobs, yy, _ = iter_step96(engine, "b0-matern12", "bernoulli")
    e_a, g_a, i_a = engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta2)
    W, Ym, nobs, yy, _ = iter_step96(engine, "b0-matern12", "bernoulli")
    engine.qv_masked_iter(W, nobs)
    engine.posterior_masked_iter(dev(XS), W, nobs, block=16)
    e_b, g_b, i_b = engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta2)
    assert e_b == e_a and np.array_equal(g_b, g_a) and i_b["rounds"] == i_a["rounds"]


def masked_xy(n, frac=0.7, seed=1):
    X, y, _, _ = D.gen_grid(n, n)
    keep = np.random.default_rng(seed).uniform(size=n * n) < frac
    return torch.tensor(X[keep]), torch.tensor(y[keep])


def test_models_on_the_iterative_solver(engine):
    from variational_gridded_gaussian_processes_amd.models import Matern12GriddedGP
    X, y = masked_xy(N)
    it = Matern12GriddedGP(X, y, 13, (0, 1), (0, 1), engine=engine, solver="iterative").to(torch.float64)
    de = Matern12GriddedGP(X, y, 13, (0, 1), (0, 1), engine=engine, solver="dense").to(torch.float64)
    cells = [0, 7, 77, 143, 12]
    xs = torch.tensor(XS)
    qi, qd = it.q_v(), de.q_v()
    assert callable(qi._variance)                              # lazy: no block solve has run for the variance yet
    assert rel(qi.mean, qd.mean) <= 1e-7
    assert rel(qi.variance, qd.variance) <= 1e-6 and not callable(qi._variance)
    lo, hi = qi.confidence_region()
    assert bool((hi >= lo).all())
    with pytest.raises(NotImplementedError):
        qi.covariance_matrix
    ai, ad = it.q_v_at(cells), de.q_v_at(cells)
    assert rel(ai.mean, ad.mean) <= 1e-7 and rel(ai.variance, ad.variance) <= 1e-6
    assert rel(ai.mean, qd.mean[cells]) <= 1e-7 and rel(ai.variance, qd.variance[cells]) <= 1e-6
    pi, pd = it.posterior(xs), de.posterior(xs)
    assert rel(pi.mean, pd.mean) <= 1e-7 and rel(pi.variance, pd.variance) <= 1e-6
    ppi, ppd = it.posterior_predictive(xs), de.posterior_predictive(xs)
    assert rel(ppi.variance, ppd.variance) <= 1e-6
    with pytest.raises(NotImplementedError):
        pi.covariance_matrix
    (-it._elbo()).backward()
    grads = [p.grad for p in it.parameters()]
    assert len(grads) == 5 and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert it.last_info["sweeps"][0] == 16                     # the step that ran was the iterative one (its probes)


def test_model_solver_keyword(engine):
    from variational_gridded_gaussian_processes_amd.models import Matern12GriddedGP
    rng = np.random.default_rng(3)
    Xs, ys = torch.tensor(rng.uniform(0, 1, (50, 2))), torch.tensor(rng.normal(size=50))
    with pytest.raises(ValueError):
        Matern12GriddedGP(Xs, ys, 9, (0, 1), (0, 1), engine=engine, solver="iterative")
    with pytest.raises(ValueError):
        Matern12GriddedGP(Xs, ys, 9, (0, 1), (0, 1), engine=engine, solver="pcg")
    # a grid with holes and M = 129^2 = 16641 > 16384: the default solver takes the iterative path instead of raising
    X, y = masked_xy(160)
    big = Matern12GriddedGP(X, y, 130, (0, 1), (0, 1), engine=engine).to(torch.float64)
    qv = big.q_v()
    assert big._iter and qv.mean.shape == (129 * 129,) and bool(torch.isfinite(qv.mean).all())
    at = big.q_v_at([0, 5000, 16640])
    assert bool(torch.isfinite(at.variance).all()) and bool((at.variance > 0).all())
