"""The iterative exact GP on the MI355X (vggp_exact_kmv, vggp_exact_*_iter, exact.py solver="iterative") against its same-probe numpy
specification (tests/exact_iter_spec.py), the dense exact step (vggp_exact_step) and the dense read-outs.

Bounds.  Kernel product: 1e-11 max|ref| (at most 1500 fp64 terms of bounded size, a few ulp per generated element, two orders of
margin).  Step against the specification: max(100 D_case, 1e-12), never above 1e-8 (MLL) / 1e-6 (gradient), D_case the
specification's own round-off floor (exact_iter_spec.FLOORS).  Step against the dense step: 3 E_case (the estimator's error, same
table).  Read-outs at N = 777 (Matern-1/2, rank 64) against the dense engine: 100 times the discrepancy of the specification to the
dense specification measured on the CPU, never above 1e-5 --
    posterior mean 7.6e-11, posterior variance 6.7e-11, q(v) mean 6.6e-11, literal variance 3.8e-16, conditional variance 6.5e-10
(max-norm relative; tests/exact_iter_spec.py posterior / q_v against exact_gp_spec.posterior / q_v).
"""
import functools

import numpy as np
import pytest
import torch

import exact_gp_spec as E
import exact_iter_spec as S

pytestmark = pytest.mark.gpu

KINDS = ["matern12", "matern32", "matern52", "rbf"]
PAIRS = [(k, k) for k in KINDS] + [("matern32", "rbf")]
SHAPES = [(1, 1, 1), (63, 63, 1), (200, 333, 17), (777, 777, 33), (1500, 130, 64)]
READOUT_CASE = "n777_m12_r64_p16"
B_POST_MEAN, B_POST_VAR, B_QV_MEAN, B_LIT_VAR, B_COND_VAR = 7.6e-9, 6.7e-9, 6.6e-9, 3.8e-14, 6.5e-8


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@functools.lru_cache(maxsize=None)
def _kmv_data(Nr, Nc, nb):
    rng = np.random.default_rng(1000 * Nr + Nc)
    xr = rng.random((Nr, 2))
    xc = xr if Nr == Nc else rng.random((Nc, 2))
    return xr, xc, rng.standard_normal((Nc, nb))


# ---- kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kinds", PAIRS, ids=lambda k: "x".join(k))
def test_kmv(engine, kinds, shape):
    """(1, 1, 1): one element; 63: below a row tile and a column chunk; (200, 333, 17): ragged in rows, columns and block width (two
    accumulators); (777, 777, 33): the square case, three accumulators; (1500, 130, 64): several workgroups, four accumulators."""
    Nr, Nc, nb = shape
    xr, xc, V = _kmv_data(Nr, Nc, nb)
    ell1, ell2 = 0.3, 0.25
    ref = [M @ V for M in S.kmat(kinds, xr, xc, ell1, ell2, der=True)]
    xrd, xcd, Vd = (torch.tensor(t, device=engine.device) for t in (xr, xc, V))
    o = engine.exact_kmv(kinds[0], kinds[1], ell1, ell2, xrd, xcd, Vd, derivatives=True)
    for got, want, what in zip(o, ref, ("value", "d ell1", "d ell2")):
        err = np.abs(got.cpu().numpy() - want).max()
        print(kinds, shape, what, err / max(np.abs(want).max(), 1e-300))
        assert got.shape == (Nr, nb)
        assert err <= 1e-11 * np.abs(want).max()
    o2 = engine.exact_kmv(kinds[0], kinds[1], ell1, ell2, xrd, xcd, Vd, derivatives=True)
    assert all(torch.equal(a, b) for a, b in zip(o, o2))                      # a second call is bitwise equal
    v = engine.exact_kmv(kinds[0], kinds[1], ell1, ell2, xrd, xcd, Vd)
    assert torch.equal(v, o[0])                                               # value-only = out0 of the derivative mode, bit for bit


# ---- the step -------------------------------------------------------------------------------------------------------------------
def _plan_case(engine, name):
    kinds, X, y, rank, nprobe, theta = S.case_data(name)
    engine.exact_iter_plan(kinds[0], kinds[1], X[:, 0], X[:, 1])
    return torch.tensor(y, device=engine.device), rank, nprobe, theta


def _alpha(engine, X, yd, theta):
    """alpha = (y - posterior mean at the training points) / sigma2:  s K0 alpha + sigma2 alpha = y."""
    mean, _, _ = engine.exact_posterior_iter(torch.tensor(X), variance=False)
    return (yd - mean) / theta[4]


@pytest.mark.parametrize("case", list(S.CASES))
def test_step_against_the_specification(engine, case):
    yd, rank, nprobe, theta = _plan_case(engine, case)
    st = S.case_spec(case)
    N = st.X.shape[0]
    b_mll, b_grad = S.bounds(S.FLOORS[case][0])
    mll, g, info = engine.exact_step_iter(yd, theta, n_probes=nprobe, rank=rank)
    e_mll, e_grad = S.errors(mll, g, st.mll, st.grad, N)
    print(f"{case}: iterations {info['rounds'][0]} (spec {st.iters}) MLL {e_mll:.2e} (bound {b_mll:.1e}) gradient {e_grad:.2e} ({b_grad:.1e})")
    assert info["status"] == 0 and info["jitter"][0] == 0.0
    assert info["rounds"][0] == st.iters and info["sweeps"][0] == nprobe
    assert e_mll <= b_mll
    assert e_grad <= b_grad
    a = _alpha(engine, st.X, yd, theta).cpu().numpy()
    assert rel(a, st.alpha) <= 1e-7
    r2 = engine.exact_step_iter(yd, theta, n_probes=nprobe, rank=rank)
    r3 = engine.exact_step_iter(yd, theta, n_probes=nprobe, rank=rank)
    assert r2[0] == r3[0] == mll and np.array_equal(r2[1], r3[1]) and np.array_equal(r2[1], g)      # calls two and three: the same bits


@pytest.mark.parametrize("case", S.DENSE_CASES)
def test_step_against_the_dense_step(engine, case):
    kinds, X, y, rank, nprobe, theta = S.case_data(case)
    N = len(y)
    yd = torch.tensor(y, device=engine.device)
    engine.exact_plan(kinds[0], kinds[1], X[:, 0], X[:, 1])
    mll_d, g_d, _ = engine.exact_step(yd, theta)
    mean_d, _ = engine.exact_posterior(torch.tensor(X))
    engine.exact_iter_plan(kinds[0], kinds[1], X[:, 0], X[:, 1])
    mll, g, info = engine.exact_step_iter(yd, theta, n_probes=nprobe, rank=rank)
    mean, _, _ = engine.exact_posterior_iter(torch.tensor(X), variance=False)
    e_mll, e_grad = S.errors(mll, g, mll_d, g_d, N)
    _, c_mll, c_grad = S.FLOORS[case]
    print(f"{case}: against the dense step MLL {e_mll:.2e} (3 E_case {3 * c_mll:.1e}) gradient {e_grad:.2e} ({3 * c_grad:.1e})")
    a_d, a_i = ((yd - m) / theta[4] for m in (mean_d, mean))                   # alpha through the posterior mean at the training points
    assert rel(a_i.cpu().numpy(), a_d.cpu().numpy()) <= 1e-7
    assert e_mll <= 3.0 * c_mll
    assert e_grad <= 3.0 * c_grad


def test_rank_n_is_one_iteration(engine):
    N, kinds, rank, nprobe, seed, theta = S.RANK_N
    X, y = S.track_points(N, seed)
    yd = torch.tensor(y, device=engine.device)
    engine.exact_plan(kinds[0], kinds[1], X[:, 0], X[:, 1])
    mll_d, _, _ = engine.exact_step(yd, theta)
    engine.exact_iter_plan(kinds[0], kinds[1], X[:, 0], X[:, 1])
    mll, _, info = engine.exact_step_iter(yd, theta, n_probes=nprobe, rank=rank)
    print("rank = N:", info, abs(mll - mll_d) / abs(mll_d))
    assert info["rounds"][0] == 1 and info["jitter"][0] == 0.0
    assert abs(mll - mll_d) <= 1e-9 * abs(mll_d)


# ---- read-outs against the dense exact read-outs -------------------------------------------------------------------------------------
def test_readouts_against_the_dense_engine(engine):
    kinds, X, y, rank, nprobe, theta = S.case_data(READOUT_CASE)
    th = torch.tensor(theta)
    Xt = torch.tensor(X)
    yd = torch.tensor(y, device=engine.device)
    xs = torch.tensor(np.random.default_rng(5).random((70, 2)))              # a full block of 64 and a ragged one
    ops = E.b0_operands(Xt, torch.linspace(0, 1, 10).double(), torch.linspace(0, 1, 8).double(), th)      # 9 x 7 cells
    cells = [0, 13, 31, 44, 62]
    engine.exact_plan(kinds[0], kinds[1], X[:, 0], X[:, 1])
    engine.exact_step(yd, theta)
    pm_d, pv_d = engine.exact_posterior(xs)
    qm_d, lit_d = engine.exact_readout(*ops, literal=True)
    _, cond_d = engine.exact_readout(*ops, literal=False)
    engine.exact_iter_plan(kinds[0], kinds[1], X[:, 0], X[:, 1])
    engine.exact_step_iter(yd, theta, n_probes=nprobe, rank=rank)
    pm, pv, info = engine.exact_posterior_iter(xs)
    assert info["sweeps"][0] == 2 and 1 <= info["rounds"][0] < 1000
    qm, lit, _ = engine.exact_readout_iter(*ops, literal=True)
    qm2, cond, info = engine.exact_readout_iter(*ops, literal=False, cells=cells)
    assert info["sweeps"][0] == 1 and qm.shape == (9, 7) and lit.shape == (9, 7) and cond.shape == (5,)
    errs = dict(post_mean=rel(pm.cpu(), pm_d.cpu()), post_var=rel(pv.cpu(), pv_d.cpu()), qv_mean=rel(qm.cpu(), qm_d.cpu()),
                lit_var=rel(lit.cpu(), lit_d.cpu()), cond_var=rel(cond.cpu(), cond_d.reshape(-1).cpu()[cells]))
    print(errs)
    assert torch.equal(qm, qm2)
    assert errs["post_mean"] <= min(B_POST_MEAN, 1e-5)
    assert errs["post_var"] <= min(B_POST_VAR, 1e-5)
    assert errs["qv_mean"] <= min(B_QV_MEAN, 1e-5)
    assert errs["lit_var"] <= min(B_LIT_VAR, 1e-5)
    assert errs["cond_var"] <= min(B_COND_VAR, 1e-5)
    # a column's numbers do not depend on its neighbours or on the block width
    pm1, pv1, _ = engine.exact_posterior_iter(xs[3:4])
    assert torch.equal(pm1, pm[3:4]) and torch.equal(pv1, pv[3:4])
    _, c1, _ = engine.exact_readout_iter(*ops, literal=False, cells=cells[2:3])
    assert torch.equal(c1, cond[2:3])


# ---- beyond the dense solver ------------------------------------------------------------------------------------------------------
def test_beyond_the_dense_solver(engine):
    from variational_gridded_gaussian_processes_amd import exact
    N = 16385
    kinds = ("matern12", "matern12")
    X, y = S.track_points(N, 1)
    yd = torch.tensor(y, device=engine.device)
    engine.exact_iter_plan(kinds[0], kinds[1], X[:, 0], X[:, 1])
    mll, g, info = engine.exact_step_iter(yd, S.THETA, n_probes=4)
    print("N = 16385:", mll, g, info)
    assert info["status"] == 0 and 1 <= info["rounds"][0] < 1000
    assert np.isfinite(mll) and np.isfinite(g).all()
    Xd = torch.tensor(X, device=engine.device)
    alpha = engine.exact_iter_alpha(S.THETA)          # (the posterior-mean identity of _alpha would add s K0 r / sigma2 to the residual r)
    assert rel(_alpha(engine, X, yd, S.THETA).cpu(), alpha.cpu()) <= 1e-6
    Ka = engine.exact_kmv(kinds[0], kinds[1], S.THETA[0], S.THETA[1], Xd, Xd, alpha.reshape(-1, 1).contiguous())[:, 0]
    res = S.THETA[2] * S.THETA[3] * Ka + S.THETA[4] * alpha - yd
    print("|Sigma alpha - y| / |y| =", float(res.norm() / yd.norm()))
    assert float(res.norm()) <= 1e-9 * float(yd.norm())
    model = exact.Matern12GP(torch.tensor(X), torch.tensor(y), engine=engine, n_probes=4).to(torch.float64)          # solver="auto"
    assert model._iterative
    (-model.mll()).backward()
    grads = [p.grad for p in model.parameters()]
    assert len(grads) == 5 and all(gr is not None and bool(torch.isfinite(gr).all()) for gr in grads)


# ---- model classes --------------------------------------------------------------------------------------------------------------
def test_model_iterative_adam_steps(engine):
    from variational_gridded_gaussian_processes_amd import exact
    X, y = S.track_points(600, 3)
    model = exact.Matern32GP(torch.tensor(X), torch.tensor(y), engine=engine, solver="iterative").to(torch.float64)
    hist = model.fit(n_iter=3, lr=0.01)
    assert hist.shape == (3,) and bool(torch.isfinite(hist).all()) and model.last_info["rounds"][0] >= 1
    p = model.posterior(torch.tensor(X[:70]))
    assert p.mean.shape == (70,) and callable(p._variance)                    # the mean at once, the variance on first access
    assert p.variance.shape == (70,) and bool((p.variance > 0).all()) and model.last_readout_info["sweeps"][0] == 2
    with pytest.raises(NotImplementedError):
        p.covariance_matrix
    g = exact.GriddedMatern12ExactGP(torch.tensor(X), torch.tensor(y), 6, (0, 1), (0, 1), engine=engine, solver="iterative").to(torch.float64)
    qv = g.q_v()
    qc = g.q_v_cells([0, 7, 35])
    assert qv.mean.shape == (36,) and qv.variance.shape == (36,) and torch.equal(qc.mean, qv.mean[[0, 7, 35]])
    assert bool((qc.variance > 0).all()) and bool((qc.variance < qv.variance[[0, 7, 35]]).all())
    with pytest.raises(NotImplementedError):
        g.q_v(literal=False)


def test_auto_is_the_dense_path_bit_for_bit(engine):
    from variational_gridded_gaussian_processes_amd import exact
    X, y = S.track_points(600, 3)
    out = []
    for kw in (dict(), dict(solver="auto"), dict(solver="dense")):
        m = exact.Matern32GP(torch.tensor(X), torch.tensor(y), engine=engine, **kw).to(torch.float64)
        assert not m._iterative
        loss = -m.mll()
        loss.backward()
        out.append((loss.item(), [p.grad.clone() for p in m.parameters()], m.posterior(torch.tensor(X[:9])).variance))
    for o in out[1:]:
        assert o[0] == out[0][0] and all(torch.equal(a, b) for a, b in zip(o[1], out[0][1])) and torch.equal(o[2], out[0][2])
    with pytest.raises(ValueError):
        exact.Matern32GP(torch.tensor(X), torch.tensor(y), engine=engine, solver="cg")


# ---- errors, state and isolation ------------------------------------------------------------------------------------------------
def test_errors_and_state(engine):
    from variational_gridded_gaussian_processes_amd import Engine, VggpError, _lib
    X, y = S.track_points(196, 1)
    yd = torch.tensor(y, device=engine.device)
    xs = torch.tensor(X[:4])

    def raises(code, fn, *a, **kw):
        with pytest.raises(VggpError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code

    fresh = Engine(0)
    fresh.exact_iter_n = 196
    raises(_lib.VGGP_ESTATE, fresh.exact_step_iter, yd, S.THETA)                                         # no plan
    raises(_lib.VGGP_ESTATE, fresh.exact_posterior_iter, xs)
    with pytest.raises(KeyError):
        engine.exact_iter_plan("matern72", "matern12", X[:, 0], X[:, 1])
    c1, c2 = X[:, 0].copy(), X[:, 1].copy()
    assert engine.lib.vggp_exact_iter_plan(engine._h, 4, 0, c1.ctypes.data, c2.ctypes.data, 196) == _lib.VGGP_EINVAL          # bad kind
    raises(_lib.VGGP_EINVAL, engine.exact_iter_plan, "matern12", "matern12", np.array([0.1, np.inf]), np.array([0.1, 0.2]))
    engine.exact_iter_plan("matern32", "matern32", X[:, 0], X[:, 1])
    raises(_lib.VGGP_ESTATE, engine.exact_posterior_iter, xs)                                            # read-out before a step
    raises(_lib.VGGP_EINVAL, engine.exact_step_iter, yd, [0.3, 0.25, 1.3, 0.8, 0.0])
    raises(_lib.VGGP_EINVAL, engine.exact_step_iter, yd, S.THETA, n_probes=64)
    raises(_lib.VGGP_EINVAL, engine.exact_step_iter, yd, S.THETA, rank=257)
    raises(_lib.VGGP_ENOCONV, engine.exact_step_iter, yd, S.THETA, rank=0, max_iter=2)
    raises(_lib.VGGP_ESTATE, engine.exact_posterior_iter, xs)                                            # ... which ended the state
    engine.exact_step_iter(yd, S.THETA)
    th = torch.tensor(S.THETA)
    ops = E.b0_operands(torch.tensor(X), torch.linspace(0, 1, 5).double(), torch.linspace(0, 1, 4).double(), th)
    raises(_lib.VGGP_EINVAL, engine.exact_readout_iter, *ops, literal=False, cells=[0])                  # cells on a Matern-3/2 plan
    engine.exact_posterior_iter(xs)                                                                      # (the state survived the refusals)
    engine.exact_iter_plan("matern12", "matern12", X[:, 0], X[:, 1])
    engine.exact_step_iter(yd, S.THETA)
    raises(_lib.VGGP_EINVAL, engine.exact_readout_iter, *ops, literal=False, cells=[12])                 # 4 x 3 cells: 12 is out of range
    raises(_lib.VGGP_EINVAL, engine.exact_readout_iter, *ops, literal=False, cells=[-1])
    raises(_lib.VGGP_EINVAL, engine.exact_readout_iter, *ops, literal=False)                             # conditional variance without cells
    Xd = torch.tensor(X, device=engine.device)
    V = torch.ones(196, 65, dtype=torch.float64, device=engine.device)
    raises(_lib.VGGP_EINVAL, engine.exact_kmv, "matern12", "matern12", 0.3, 0.25, Xd, Xd, V)             # nb > 64
    raises(_lib.VGGP_EINVAL, engine.exact_kmv, "matern12", "matern12", 0.0, 0.25, Xd, Xd, V[:, :3].contiguous())
    multi = Engine(0, n_ranks=2, rank=0, allreduce=lambda buf: None)                                     # multi-rank context
    raises(_lib.VGGP_EINVAL, multi.exact_iter_plan, "matern12", "matern12", X[:, 0], X[:, 1])
    raises(_lib.VGGP_EINVAL, multi.exact_kmv, "matern12", "matern12", 0.3, 0.25, Xd, Xd, V[:, :3].contiguous())


def test_isolation_from_the_planned_model_and_the_dense_state(engine):
    from oracle import dense as D
    rng = np.random.default_rng(7)
    Xs = rng.random((300, 2))
    ys = torch.tensor(D.latent_2d(Xs[:, 0], Xs[:, 1]) + 0.05 * rng.standard_normal(300), device=engine.device)
    z = np.linspace(0.0, 1.0, 6)
    engine.plan("matern12", "points", z, Xs[:, 0], "matern12", "points", z, Xs[:, 1], scattered=True)
    engine.elbo_step_scattered(ys, float((ys * ys).sum()), [0.2, 0.25, 0.9, 1.1, 0.02])
    mean0, var0 = [t.clone() for t in engine.qv_masked()]
    X, y = S.track_points(196, 1)
    yd = torch.tensor(y, device=engine.device)
    xs = torch.tensor(rng.random((20, 2)))
    engine.exact_plan("matern12", "matern12", X[:, 0], X[:, 1])
    engine.exact_step(yd, S.THETA)
    pm0, pv0 = [t.clone() for t in engine.exact_posterior(xs)]
    engine.exact_iter_plan("matern12", "matern12", X[:, 0], X[:, 1])
    engine.exact_step_iter(yd, S.THETA)
    ops = E.b0_operands(torch.tensor(X), torch.linspace(0, 1, 5).double(), torch.linspace(0, 1, 4).double(), torch.tensor(S.THETA))
    engine.exact_posterior_iter(xs)
    engine.exact_readout_iter(*ops, literal=False, cells=[1, 5])
    mean1, var1 = engine.qv_masked()
    pm1, pv1 = engine.exact_posterior(xs)
    assert torch.equal(mean0, mean1) and torch.equal(var0, var1)              # the planned sparse model: the same bits
    assert torch.equal(pm0, pm1) and torch.equal(pv0, pv1)                    # the dense exact state: the same bits
