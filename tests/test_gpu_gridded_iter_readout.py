"""The gridded read-out q(v) after an iterative step on the GPU: vg_kr_sqgram alone against numpy, vggp_readout_scattered_iter /
vggp_readout_masked_iter against the dense GPU path (vggp_readout_masked after the dense step on the same plan), beyond the dense
solver's limit against the Kronecker path on a full grid, their state and argument checks, and the Gridded* model classes on both
iterative solvers against the same models on the dense ones.  Tolerances as test_gpu_masked_iter_readout.py: means 1e-7, variances
1e-6 of the largest reference entry (the conditional variance cancels heavily -- kd1 kd2 ~ 1.0e-4 against |t|^2 ~ 9.8e-5 for a result
of ~1e-6 -- so entries are compared relative to the largest one, not one by one).

Measured on one MI355X: kernel <= 1.9e-15 (bitwise equal across calls); scattered against the dense GPU path mean <= 3.5e-10, variances
<= 1.9e-14, 9-10 iterations; masked mean 9.8e-11, variances <= 7.7e-16, 17 iterations; beyond the dense limit mean <= 2.2e-11, variances
<= 2.7e-12, 1 iteration."""
import functools

import numpy as np
import pytest
import torch

from oracle import dense as D
from oracle import kron as Kr
from variational_gridded_gaussian_processes_amd import _lib
from variational_gridded_gaussian_processes_amd._lib import VggpError

import scattered_iter_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIMS = (-0.1, 1.1)
CELLS5 = [0, 71, 17, 40, 63]                # of 9 x 8 = 72: the first and the last cell among them


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def code_of(fn, *a, **kw):
    with pytest.raises(VggpError) as e:
        fn(*a, **kw)
    return e.value.code


# ---- 1: the kernel alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv1,mv2,N", [(1, 1, 1), (64, 64, 256), (65, 3, 1000), (130, 70, 100003)], ids=lambda v: str(v))
def test_kr_sqgram_vs_numpy(engine, mv1, mv2, N):
    rng = np.random.default_rng(mv1 * 1000 + N)
    P1, P2 = rng.standard_normal((mv1, N)), rng.standard_normal((mv2, N))
    ref = (P1 * P1) @ (P2 * P2).T
    P1d, P2d = dev(P1), dev(P2)
    got = engine.kr_sqgram(P1d, P2d)
    err = rel(got.cpu().numpy(), ref)
    print(f"({mv1}, {mv2}, {N}): {err:.2e} of the largest entry")
    assert tuple(got.shape) == (mv1, mv2)
    assert err <= 1e-13
    assert torch.equal(got, engine.kr_sqgram(P1d, P2d))          # slabs summed in fixed order: the same bits


# ---- 2, 3: scattered points against the dense GPU path --------------------------------------------------------------------------------------
def vff_grid(nf):
    return np.concatenate([[LIMS[0], LIMS[1]], D.vff_omegas(nf, *LIMS).double().numpy()])


@functools.lru_cache(maxsize=None)
def trk400():
    return S.trk(400, 0.5)


def operands(f1, f2, mv1, mv2, theta):
    (C1, kd1), (C2, kd2) = Kr.cross_b0(f1, np.linspace(0, 1, mv1 + 1), theta[0]), Kr.cross_b0(f2, np.linspace(0, 1, mv2 + 1), theta[1])
    return dev(C1), dev(C2), dev(kd1), dev(kd2)


def plan_trk_vff(engine):
    X, y = trk400()
    g1, g2 = vff_grid(6), vff_grid(5)
    engine.plan("matern12", "vff", g1, X[:, 0], "matern12", "vff", g2, X[:, 1], scattered=True)
    assert (engine.m1, engine.m2) == (13, 11)
    e = np.empty(0)
    return dev(y), float(y @ y), Kr.Factor("vff", "matern12", g1, e), Kr.Factor("vff", "matern12", g2, e)


def test_scattered_vs_dense_gpu_path(engine):
    theta = S.THETA_B
    yd, yy, f1, f2 = plan_trk_vff(engine)
    ops = operands(f1, f2, 9, 8, theta)
    engine.elbo_step_scattered(yd, yy, theta)
    ref = {lit: [t.cpu().numpy() for t in engine.readout(*ops, literal=lit, masked=True)] for lit in (True, False)}
    engine.elbo_step_scattered_iter(yd, yy, theta)
    mean, var, info = engine.readout_scattered_iter(*ops, literal=True)
    e_m, e_v = rel(mean.cpu().numpy(), ref[True][0]), rel(var.cpu().numpy(), ref[True][1].reshape(-1))
    print(f"literal: mean {e_m:.1e} var {e_v:.1e}")
    assert tuple(mean.shape) == (9, 8) and tuple(var.shape) == (72,)
    assert info["sweeps"][0] == 0 and info["rounds"][0] == 0
    assert e_m <= 1e-7
    assert e_v <= 1e-6
    for block, solves in ((64, 2), (16, 5)):
        mean, var, info = engine.readout_scattered_iter(*ops, literal=False, block=block)
        e_m, e_v = rel(mean.cpu().numpy(), ref[False][0]), rel(var.cpu().numpy(), ref[False][1].reshape(-1))
        print(f"conditional, block {block}: mean {e_m:.1e} var {e_v:.1e}, most iterations {info['rounds'][0]}")
        assert info["sweeps"][0] == solves and 0 < info["rounds"][0] < 30
        assert e_m <= 1e-7
        assert e_v <= 1e-6
    for lit in (True, False):
        _, vc, info = engine.readout_scattered_iter(*ops, literal=lit, cells=CELLS5)
        assert info["sweeps"][0] == (0 if lit else 1)
        assert rel(vc.cpu().numpy(), ref[lit][1].reshape(-1)[CELLS5]) <= 1e-6
    mean_only, none, info = engine.readout_scattered_iter(*ops, variance=False)
    assert none is None and info["sweeps"][0] == 0 and rel(mean_only.cpu().numpy(), ref[True][0]) <= 1e-7


def test_output_grid_larger_than_a_tile(engine):
    theta = S.THETA_B
    yd, yy, f1, f2 = plan_trk_vff(engine)
    ops = operands(f1, f2, 70, 130, theta)
    cells = [0, 70 * 130 - 1, 64 * 130 + 64, 69 * 130, 129]
    engine.elbo_step_scattered(yd, yy, theta)
    ref = {lit: [t.cpu().numpy() for t in engine.readout(*ops, literal=lit, masked=True)] for lit in (True, False)}
    engine.elbo_step_scattered_iter(yd, yy, theta)
    mean, var, info = engine.readout_scattered_iter(*ops, literal=True)
    e_m, e_v = rel(mean.cpu().numpy(), ref[True][0]), rel(var.cpu().numpy(), ref[True][1].reshape(-1))
    print(f"70 x 130 cells, literal: mean {e_m:.1e} var {e_v:.1e}")
    assert tuple(mean.shape) == (70, 130) and info["sweeps"][0] == 0
    assert e_m <= 1e-7
    assert e_v <= 1e-6
    _, vc, info = engine.readout_scattered_iter(*ops, literal=False, cells=cells)
    e_c = float(np.abs(vc.cpu().numpy() - ref[False][1].reshape(-1)[cells]).max() / np.abs(ref[False][1]).max())
    print(f"70 x 130 cells, conditional at 5 cells: var {e_c:.1e}, iterations {info['rounds'][0]}")
    assert info["sweeps"][0] == 1 and e_c <= 1e-6


def test_literal_accumulates_over_chunks_of_points(engine):
    """N = 70 001 > 65 536: P_d is formed for two chunks of points (the second ragged) and the partial S are added in chunk order."""
    from variational_gridded_gaussian_processes_amd import datagen
    rng = np.random.default_rng(8)
    X = rng.random((70001, 2))
    y = datagen.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(len(X))
    z1, z2 = np.linspace(0, 1, 8), np.linspace(0, 1, 7)
    engine.plan("matern12", "points", z1, X[:, 0], "matern12", "points", z2, X[:, 1], scattered=True)
    yd, yy, theta = dev(y), float(y @ y), S.THETA_B
    e = np.empty(0)
    ops = operands(Kr.Factor("points", "matern12", z1, e), Kr.Factor("points", "matern12", z2, e), 9, 8, theta)
    engine.elbo_step_scattered(yd, yy, theta)
    rm, rv = [t.cpu().numpy() for t in engine.readout(*ops, literal=True, masked=True)]
    engine.elbo_step_scattered_iter(yd, yy, theta)
    mean, var, info = engine.readout_scattered_iter(*ops, literal=True)
    e_m, e_v = rel(mean.cpu().numpy(), rm), rel(var.cpu().numpy(), rv.reshape(-1))
    print(f"70 001 points, literal: mean {e_m:.1e} var {e_v:.1e}")
    assert info["sweeps"][0] == 0
    assert e_m <= 1e-7
    assert e_v <= 1e-6
    assert torch.equal(var, engine.readout_scattered_iter(*ops, literal=True)[1])


# ---- 4: a grid with holes against the dense GPU path ----------------------------------------------------------------------------------------
def masked_case():
    n1, n2 = 40, 36
    _, y, x1, x2 = D.gen_grid(n1, n2)
    Wn = (np.random.default_rng(1).uniform(size=(n2, n1)) < 0.7).astype(np.float64)
    z1, z2 = np.linspace(0, 1, 12), np.linspace(0, 1, 10)
    return y.reshape(n2, n1), Wn, x1, x2, z1, z2


def test_masked_vs_dense_gpu_path(engine):
    theta = S.THETA_B
    Y, Wn, x1, x2, z1, z2 = masked_case()
    engine.plan("matern12", "points", z1, x1, "matern12", "points", z2, x2)
    W = dev(Wn)
    Ym = dev(Y) * W
    nobs, yy = float(Wn.sum()), engine.sumsq(Ym)
    ops = operands(Kr.Factor("points", "matern12", z1, x1), Kr.Factor("points", "matern12", z2, x2), 7, 9, theta)
    engine.elbo_step_masked(Ym, W, nobs, yy, theta)
    ref = {lit: [t.cpu().numpy() for t in engine.readout(*ops, literal=lit, masked=True)] for lit in (True, False)}
    engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta)
    for lit in (True, False):
        mean, var, info = engine.readout_masked_iter(*ops, W, nobs, literal=lit)
        e_m, e_v = rel(mean.cpu().numpy(), ref[lit][0]), rel(var.cpu().numpy(), ref[lit][1].reshape(-1))
        print(f"masked, literal={lit}: mean {e_m:.1e} var {e_v:.1e}, solves {info['sweeps'][0]}, iterations {info['rounds'][0]}")
        assert tuple(mean.shape) == (7, 9) and info["sweeps"][0] == (0 if lit else 1)
        assert e_m <= 1e-7
        assert e_v <= 1e-6
    _, vc, _ = engine.readout_masked_iter(*ops, W, nobs, literal=False, cells=[0, 62, 31])
    assert rel(vc.cpu().numpy(), ref[False][1].reshape(-1)[[0, 62, 31]]) <= 1e-6


# ---- 5: beyond the dense limit ----------------------------------------------------------------------------------------------------------------
def random_operands(m1, m2):
    rng = np.random.default_rng(21)
    return dev(rng.standard_normal((5, m1))), dev(rng.standard_normal((6, m2))), dev(rng.uniform(0.5, 1.5, 5)), dev(rng.uniform(0.5, 1.5, 6))


@pytest.mark.parametrize("kind", ["scattered", "masked"])
def test_beyond_the_dense_limit(engine, kind):
    """M > 16384 on fully observed data, where the preconditioner is exact: the Kronecker path's vggp_readout is the reference."""
    n, m1, m2 = 160, 136, (128 if kind == "scattered" else 136)
    theta = S.THETA_A
    X, y, x1, x2 = D.gen_grid(n, n)
    g1, g2 = np.linspace(0, 1, m1 + 1), np.linspace(0, 1, m2 + 1)
    ops = random_operands(m1, m2)
    Y = dev(y.reshape(n, n))
    engine.plan("matern12", "b0", g1, x1, "matern12", "b0", g2, x2)
    engine.elbo_step(Y, engine.sumsq(Y), theta)
    ref = {lit: [t.cpu().numpy() for t in engine.readout(*ops, literal=lit)] for lit in (True, False)}
    if kind == "scattered":
        engine.plan("matern12", "b0", g1, X[:, 0], "matern12", "b0", g2, X[:, 1], scattered=True)
        engine.elbo_step_scattered_iter(dev(y), float(y @ y), theta)
        run = lambda lit: engine.readout_scattered_iter(*ops, literal=lit)
    else:
        ones = torch.ones_like(Y)
        engine.elbo_step_masked_iter(Y, ones, float(n * n), engine.sumsq(Y), theta)
        run = lambda lit: engine.readout_masked_iter(*ops, ones, float(n * n), literal=lit)
    for lit in (True, False):
        mean, var, info = run(lit)
        e_m, e_v = rel(mean.cpu().numpy(), ref[lit][0]), rel(var.cpu().numpy(), ref[lit][1].reshape(-1))
        print(f"{kind}, M = {m1 * m2}, literal={lit}: mean {e_m:.1e} var {e_v:.1e}, solves {info['sweeps'][0]}, iterations {info['rounds'][0]}")
        assert info["sweeps"][0] == (0 if lit else 1) and info["rounds"][0] <= 3
        assert e_m <= 1e-7
        assert e_v <= 1e-6


# ---- 6: state and errors ------------------------------------------------------------------------------------------------------------------------
def test_state_and_errors(engine):
    from variational_gridded_gaussian_processes_amd import Engine
    theta = S.THETA_B
    Y, Wn, x1, x2, z1, z2 = masked_case()
    W = dev(Wn)
    Ym = dev(Y) * W
    nobs = float(Wn.sum())
    f1, f2 = Kr.Factor("points", "matern12", z1, x1), Kr.Factor("points", "matern12", z2, x2)
    ops = operands(f1, f2, 7, 9, theta)
    X, y = S.rand20k()
    X, y = X[:600], y[:600]
    yd, yy = dev(y), float(y @ y)
    plan_s = lambda e: e.plan("matern12", "points", z1, X[:, 0], "matern12", "points", z2, X[:, 1], scattered=True)
    plan_m = lambda e: e.plan("matern12", "points", z1, x1, "matern12", "points", z2, x2)
    fresh = Engine(0)
    try:                                                                             # before any step
        plan_s(fresh)
        assert code_of(fresh.readout_scattered_iter, *ops) == _lib.VGGP_ESTATE
        plan_m(fresh)
        assert code_of(fresh.readout_masked_iter, *ops, W, nobs) == _lib.VGGP_ESTATE
    finally:
        fresh.close()
    plan_s(engine)
    engine.elbo_step_scattered_iter(yd, yy, theta)
    assert code_of(engine.readout_masked_iter, *ops, torch.ones(600, 600, dtype=torch.float64, device=DEV), 600.0) == _lib.VGGP_EINVAL  # wrong plan kind
    for bad in ([63], [-1], [3, 10 ** 12]):                                          # 7 x 9 cells: [0, 63)
        assert code_of(engine.readout_scattered_iter, *ops, cells=bad) == _lib.VGGP_EINVAL
        assert code_of(engine.readout_scattered_iter, *ops, cells=bad, literal=False) == _lib.VGGP_EINVAL
    assert code_of(engine.readout_scattered_iter, *ops, literal=False, block=65) == _lib.VGGP_EINVAL
    _, v, _ = engine.readout_scattered_iter(*ops, cells=[3], literal=False)          # (the refused calls left the state readable)
    assert bool(torch.isfinite(v).all())
    engine.elbo_step_scattered(yd, yy, theta)                                        # after a dense step
    assert code_of(engine.readout_scattered_iter, *ops) == _lib.VGGP_ESTATE
    engine.elbo_step_scattered_iter(yd, yy, theta)
    plan_s(engine)                                                                   # after plan
    assert code_of(engine.readout_scattered_iter, *ops) == _lib.VGGP_ESTATE
    plan_m(engine)
    yym = engine.sumsq(Ym)
    engine.elbo_step_masked_iter(Ym, W, nobs, yym, theta)
    assert code_of(engine.readout_scattered_iter, *ops) == _lib.VGGP_EINVAL         # wrong plan kind
    assert code_of(engine.readout_masked_iter, *ops, W, nobs, cells=[63]) == _lib.VGGP_EINVAL
    assert code_of(engine.readout_masked_iter, *ops, W, nobs, literal=False, block=65) == _lib.VGGP_EINVAL
    engine.elbo_step_masked(Ym, W, nobs, yym, theta)                                 # after a dense step
    assert code_of(engine.readout_masked_iter, *ops, W, nobs) == _lib.VGGP_ESTATE
    engine.elbo_step_masked_iter(Ym, W, nobs, yym, theta)
    plan_m(engine)                                                                   # after plan
    assert code_of(engine.readout_masked_iter, *ops, W, nobs) == _lib.VGGP_ESTATE


@pytest.mark.parametrize("kind", ["scattered", "masked"])
def test_readout_leaves_the_next_step_unchanged(engine, kind):
    """A read-out between two steps: the second step reuses the kept preconditioner basis and returns the bits of a run without it."""
    theta = S.THETA_B
    theta2 = [t * 1.01 for t in theta]
    if kind == "scattered":
        yd, yy, f1, f2 = plan_trk_vff(engine)
        ops = operands(f1, f2, 9, 8, theta)
        replan = lambda: plan_trk_vff(engine)
        step = lambda th: engine.elbo_step_scattered_iter(yd, yy, th)
        read = lambda lit: engine.readout_scattered_iter(*ops, literal=lit, block=16)
    else:
        Y, Wn, x1, x2, z1, z2 = masked_case()
        W = dev(Wn)
        Ym = dev(Y) * W
        nobs = float(Wn.sum())
        replan = lambda: engine.plan("matern12", "points", z1, x1, "matern12", "points", z2, x2)
        replan()
        yym = engine.sumsq(Ym)
        ops = operands(Kr.Factor("points", "matern12", z1, x1), Kr.Factor("points", "matern12", z2, x2), 7, 9, theta)
        step = lambda th: engine.elbo_step_masked_iter(Ym, W, nobs, yym, th)
        read = lambda lit: engine.readout_masked_iter(*ops, W, nobs, literal=lit, block=16)
    replan()
    step(theta)
    e_a, g_a, i_a = step(theta2)
    replan()
    step(theta)
    read(True)
    read(False)
    e_b, g_b, i_b = step(theta2)
    assert e_b == e_a and np.array_equal(g_b, g_a) and i_b["rounds"] == i_a["rounds"]


# ---- 7: models --------------------------------------------------------------------------------------------------------------------------------
def small(data):
    """A 24 x 20 grid with 30 % missing, as it is ("masked") or jittered off the grid ("scattered")."""
    X, y, _, _ = D.gen_grid(24, 20)
    rng = np.random.default_rng(5)
    keep = rng.random(len(y)) > 0.3
    X, y = X[keep], y[keep]
    if data == "scattered":
        X = np.clip(X + rng.normal(scale=4e-3, size=X.shape), 0.0, 1.0)
    return torch.tensor(X), torch.tensor(y)


def make(cls, X, y, engine, **kw):
    import variational_gridded_gaussian_processes_amd.models as M
    ns = 7
    if cls == "vff":
        return M.GriddedMatern12VFFGP(X, y, 5, LIMS, LIMS, ns, (0, 1), (0, 1), engine=engine, **kw).to(torch.float64)
    if cls == "svgp":
        z1, z2 = torch.linspace(0, 1, 6, dtype=torch.float64), torch.linspace(0, 1, 5, dtype=torch.float64)
        Z = torch.cartesian_prod(z1, z2)[torch.randperm(30, generator=torch.Generator().manual_seed(3))]          # rows in any order
        return M.GriddedMatern12SVGP(X, y, Z, ns, (0, 1), (0, 1), engine=engine, **kw).to(torch.float64)
    return M.GriddedMatern12ASVGP(X, y, ns, 2, (0, 1), (0, 1), engine=engine, **kw).to(torch.float64)


@pytest.mark.parametrize("cls", ["vff", "svgp", "asvgp"])
@pytest.mark.parametrize("data", ["masked", "scattered"])
def test_models_on_the_iterative_solvers(engine, data, cls):
    X, y = small(data)
    kw = "solver" if data == "masked" else "scattered_solver"
    it, de = make(cls, X, y, engine, **{kw: "iterative"}), make(cls, X, y, engine, **{kw: "dense"})
    cells = [0, 48, 17, 30]
    ql, qld = it.q_v(literal=True), de.q_v(literal=True)
    assert (it._siter if data == "scattered" else it._iter) and not (de._siter or de._iter)
    assert not callable(ql._variance) and it.last_readout_info["sweeps"][0] == 0      # mean and variance at once, no solve
    assert ql.mean.shape == (49,) and rel(ql.mean, qld.mean) <= 1e-7 and rel(ql.variance, qld.variance) <= 1e-6
    qc, qcd = it.q_v(literal=False), de.q_v(literal=False)
    assert callable(qc._variance)                                                      # lazy: no block solve has run yet
    assert rel(qc.mean, qcd.mean) <= 1e-7
    assert rel(qc.variance, qcd.variance) <= 1e-6 and it.last_readout_info["sweeps"][0] == 1
    with pytest.raises(NotImplementedError):
        qc.covariance_matrix
    for lit in (False, True):
        a, ad = it.q_v_cells(cells, literal=lit), de.q_v_cells(cells, literal=lit)
        ref = (qld if lit else qcd)
        assert rel(a.mean, ref.mean[cells]) <= 1e-7 and rel(ad.mean, ref.mean[cells]) <= 1e-12
        assert float((a.variance - ref.variance[cells]).abs().max() / ref.variance.abs().max()) <= 1e-6
        assert torch.equal(ad.variance, ref.variance[cells])
    assert rel(it.q_u().mean, de.q_u().mean) <= 1e-7                                  # (SVGP: in the row order of Z, without touching the variance)
    if data == "scattered":
        with pytest.raises(NotImplementedError, match="follow-up"):
            it.q_u().variance


def test_model_auto_beyond_the_dense_limit(engine):
    """scattered_solver='auto' at M = 136 * 128 = 17408 takes the iterative scattered step; the gridded q_v() is there."""
    import variational_gridded_gaussian_processes_amd.models as M
    X, y, _, _ = D.gen_grid(160, 160)
    X = np.clip(X + np.random.default_rng(6).normal(scale=5e-4, size=X.shape), 0.0, 1.0)      # off the grid: scattered points
    Z = torch.cartesian_prod(torch.linspace(0, 1, 136, dtype=torch.float64), torch.linspace(0, 1, 128, dtype=torch.float64))
    m = M.GriddedMatern12SVGP(torch.tensor(X), torch.tensor(y), Z, 7, (0, 1), (0, 1), engine=engine).to(torch.float64)
    qv = m.q_v()
    assert m._scattered and m._siter and m.last_info["rounds"][0] < 100
    assert qv.mean.shape == (49,) and bool(torch.isfinite(qv.mean).all()) and bool(torch.isfinite(qv.variance).all())
    assert bool((qv.variance > 0).all())
