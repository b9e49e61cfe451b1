"""The iterative scattered step on the GPU: the two Khatri-Rao kernels alone (against numpy.einsum, forward bound of a length-K fp64 dot
product), vggp_elbo_step_scattered_iter against its numpy specification (identical probes: ELBO 1e-8, gradient 1e-6) and against the
dense scattered step (the caps of tests/test_scattered_iter_spec.py), its mean read-outs against the dense ones (1e-7), beyond the
dense solver's limit of M = 16384 against the Kronecker path on a full grid, and through the model classes (scattered_solver=).
The ELBO / gradient caps are asserted in the data-rich regime (N / M >= 60) only: no tolerance is stated where N is about M.

Measured on one MI355X: kernels 0.000 .. 0.027 of the forward bound; step against the specification 1e-15 .. 1e-13 (same iteration
counts); against the dense step ELBO 1.5e-7 .. 6.9e-6, gradient 1.3e-7 .. 4.3e-6, mean read-outs <= 1.9e-9; the 160 x 160 grid as points
1 iteration, 2e-12 / 3e-12 / 8e-13 against the Kronecker path; track points at N / M = 0.92: 117 iterations (not converged at 100).
"""
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
U = 2.0 ** -52


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- B: the two kernels alone ---------------------------------------------------------------------------------------------------------
KR_SHAPES = [(5, 7, 37, 3), (16, 16, 64, 1), (17, 33, 1000, 6), (48, 20, 16090, 17), (136, 128, 4099, 17), (256, 256, 515, 64)]


def _field_ref(L, R, V):
    return np.einsum("ak,cak->ck", L, np.einsum("acb,bk->cak", V, R, optimize=True), optimize=True)


def _back_ref(L, R, F):
    return np.einsum("ak,cbk->acb", L, F[:, None, :] * R[None, :, :], optimize=True)


@pytest.mark.parametrize("m1,m2,N,nb", KR_SHAPES, ids=lambda v: str(v))
def test_kr_kernels_vs_einsum(engine, m1, m2, N, nb):
    rng = np.random.default_rng(m1 * 1000 + N)
    L, R, V, F = rng.standard_normal((m1, N)), rng.standard_normal((m2, N)), rng.standard_normal((m1, nb, m2)), rng.standard_normal((nb, N))
    Ld, Rd = dev(L), dev(R)
    got_f = engine.kr_field(Ld, Rd, dev(V)).cpu().numpy()
    ref_f, abs_f = _field_ref(L, R, V), _field_ref(np.abs(L), np.abs(R), np.abs(V))
    worst_f = float((np.abs(got_f - ref_f) / (m1 * m2 * U * abs_f)).max())
    Fd = dev(F)
    got_b = engine.kr_back(Ld, Rd, Fd)
    ref_b, abs_b = _back_ref(L, R, F), _back_ref(np.abs(L), np.abs(R), np.abs(F))
    worst_b = float((np.abs(got_b.cpu().numpy() - ref_b) / (N * U * abs_b)).max())
    print(f"({m1}, {m2}, {N}, {nb}): field {worst_f:.3f}, back {worst_b:.3f} of the forward bound K 2^-52 |.|")
    assert got_f.shape == (nb, N) and tuple(got_b.shape) == (m1, nb, m2)
    assert worst_f <= 1.0
    assert worst_b <= 1.0
    assert torch.equal(got_b, engine.kr_back(Ld, Rd, Fd))          # split reduction in fixed order: bitwise equal across calls


# ---- C: the step against its specification and against the dense step ---------------------------------------------------------------------
def _vff_grid():
    a, b = -0.1, 1.1
    return np.concatenate([[a, b], D.vff_omegas(6, a, b).double().numpy()])


STEP_CASES = {
    "trk400_m12_a": ("trk400", "b0", "matern12", 12, S.THETA_A),
    "trk400_m12_b": ("trk400", "b0", "matern12", 12, S.THETA_B),
    "trk400_m16_b": ("trk400", "b0", "matern12", 16, S.THETA_B),
    "trk600_m24_b": ("trk600", "b0", "matern12", 24, S.THETA_B),
    "rand20k_m8_a": ("rand20k", "b0", "matern12", 8, S.THETA_A),
    "trk400_points_matern32_m16_b": ("trk400", "points", "matern32", 16, S.THETA_B),
    "trk400_vff_m13_b": ("trk400", "vff", "matern12", 13, S.THETA_B),
}
XS = np.random.default_rng(9).uniform(0, 1, (50, 2))


@functools.lru_cache(maxsize=None)
def data(name):
    return {"trk400": lambda: S.trk(400, 0.5), "trk600": lambda: S.trk(600, 0.25), "rand20k": S.rand20k}[name]()


def grid_of(basis, m):
    return np.linspace(0.0, 1.0, m + 1) if basis == "b0" else (_vff_grid() if basis == "vff" else np.linspace(0.0, 1.0, m))


@functools.lru_cache(maxsize=None)
def spec(case):
    dname, basis, kind, m, theta = STEP_CASES[case]
    X, y = data(dname)
    g = grid_of(basis, m)
    e = np.empty(0)
    return S.elbo_step_scattered_iter(X, y, Kr.Factor(basis, kind, g, e), Kr.Factor(basis, kind, g, e), theta)


def plan_case(engine, case):
    dname, basis, kind, m, theta = STEP_CASES[case]
    X, y = data(dname)
    g = grid_of(basis, m)
    engine.plan(kind, basis, g, X[:, 0], kind, basis, g, X[:, 1], scattered=True)          # a fresh plan: cold basis
    yd = dev(y)
    return yd, float(y @ y), theta, len(y)


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_step_vs_spec_and_dense(engine, case):
    yd, yy, theta, N = plan_case(engine, case)
    assert engine.m1 == STEP_CASES[case][3]
    elbo, grad, info = engine.elbo_step_scattered_iter(yd, yy, theta)
    st = spec(case)
    e_elbo, e_grad = S.errors(elbo, grad, st.elbo, st.grad, N)
    print(f"{case}: iterations {info['rounds'][0]} (spec {st.iters}); against the spec: ELBO {e_elbo:.2e} gradient {e_grad:.2e}")
    assert info["rounds"][0] == st.iters and info["sweeps"][0] == 16
    assert e_elbo <= 1e-8
    assert e_grad <= 1e-6
    qm = engine.qv_scattered_iter().cpu().numpy()
    pm = engine.posterior_scattered_iter(dev(XS)).cpu().numpy()
    # the dense read-outs have nothing to read after the iterative step
    with pytest.raises(VggpError) as ei:
        engine.qv_masked()
    assert ei.value.code == _lib.VGGP_ESTATE
    # second and third call (kept basis, Rayleigh quotients): the third equals the second bit for bit
    e2, g2, i2 = engine.elbo_step_scattered_iter(yd, yy, theta)
    e3, g3, i3 = engine.elbo_step_scattered_iter(yd, yy, theta)
    assert e3 == e2 and np.array_equal(g3, g2) and i3["rounds"] == i2["rounds"]
    assert S.errors(e2, g2, elbo, grad, N)[0] <= 1e-8
    # against the dense step on the same context
    de, dg, _ = engine.elbo_step_scattered(yd, yy, theta)
    d_elbo, d_grad = S.errors(elbo, grad, de, dg, N)
    dqm, _ = engine.qv_masked()
    dpm, _ = engine.posterior_masked(dev(XS))
    e_q, e_p = rel(qm, dqm.cpu().numpy()), rel(pm, dpm.cpu().numpy())
    print(f"{case}: against the dense step: ELBO {d_elbo:.2e} gradient {d_grad:.2e} q(v) mean {e_q:.2e} posterior mean {e_p:.2e}")
    assert info["rounds"][0] < 30
    assert d_elbo <= 1e-4
    assert d_grad <= 2e-4
    assert e_q <= 1e-7
    assert e_p <= 1e-7
    with pytest.raises(VggpError) as ei:          # ... and the iterative read-outs nothing after the dense step
        engine.qv_scattered_iter()
    assert ei.value.code == _lib.VGGP_ESTATE
    with pytest.raises(VggpError) as ei:
        engine.posterior_scattered_iter(dev(XS))
    assert ei.value.code == _lib.VGGP_ESTATE


# ---- D: beyond the dense limit ------------------------------------------------------------------------------------------------------------
def test_beyond_dense_limit(engine):
    n, m1, m2 = 160, 136, 128
    theta = S.THETA_A
    X, y, x1, x2 = D.gen_grid(n, n)
    g1, g2 = np.linspace(0, 1, m1 + 1), np.linspace(0, 1, m2 + 1)
    # the Kronecker path on the grid
    engine.plan("matern12", "b0", g1, x1, "matern12", "b0", g2, x2)
    Y = dev(y.reshape(n, n))
    ke, kg, _ = engine.elbo_step(Y, engine.sumsq(Y), theta)
    kq = engine.qv()[0].cpu().numpy()
    # the same observations as 25 600 scattered points
    engine.plan("matern12", "b0", g1, X[:, 0], "matern12", "b0", g2, X[:, 1], scattered=True)
    yd, yy = dev(y), float(y @ y)
    with pytest.raises(VggpError):
        engine.elbo_step_scattered(yd, yy, theta)                     # M = 17408 > 16384
    elbo, grad, info = engine.elbo_step_scattered_iter(yd, yy, theta)
    e_elbo, e_grad = S.errors(elbo, grad, ke, kg, n * n)
    e_q = rel(engine.qv_scattered_iter().cpu().numpy(), kq)
    print(f"full grid as points, M = {m1 * m2}: iterations {info['rounds'][0]}, ELBO {e_elbo:.2e} gradient {e_grad:.2e} q(v) mean {e_q:.2e}")
    assert info["rounds"][0] <= 3                                     # the preconditioner is exact on a full grid
    assert e_elbo <= 1e-8
    assert e_grad <= 1e-6
    assert e_q <= 1e-7


def test_track_points_beyond_dense_limit(engine):
    """Along-track points on the basis of test_beyond_dense_limit (N = 16090 < M = 17408: the data-poor regime, where no accuracy is
    stated and the PCG is expected to need many iterations -- it gets the largest max_iter the engine accepts): finite, converged
    before max_iter, and the same bits from a second freshly planned run."""
    m1, m2, theta, max_iter = 136, 128, S.THETA_A, 128
    g1, g2 = np.linspace(0, 1, m1 + 1), np.linspace(0, 1, m2 + 1)
    Xt, yt = data("trk400")
    ytd, yyt = dev(yt), float(yt @ yt)
    runs = []
    for _ in range(2):
        engine.plan("matern12", "b0", g1, Xt[:, 0], "matern12", "b0", g2, Xt[:, 1], scattered=True)
        runs.append(engine.elbo_step_scattered_iter(ytd, yyt, theta, max_iter=max_iter))
    (e1, gr1, i1), (e2, gr2, i2) = runs
    print(f"track points, N = {len(yt)}, M = {m1 * m2}: iterations {i1['rounds'][0]}, ELBO {e1:.6f}")
    assert np.isfinite(e1) and np.isfinite(gr1).all() and 0 < i1["rounds"][0] < max_iter
    assert e2 == e1 and np.array_equal(gr2, gr1) and i2["rounds"] == i1["rounds"]
    assert torch.isfinite(engine.qv_scattered_iter()).all() and torch.isfinite(engine.posterior_scattered_iter(dev(XS))).all()


# ---- E: models and error paths ------------------------------------------------------------------------------------------------------------
def _grads(model):
    return [model.kernel_1.base_kernel.raw_lengthscale.grad, model.kernel_2.base_kernel.raw_lengthscale.grad,
            model.kernel_1.raw_outputscale.grad, model.kernel_2.raw_outputscale.grad, model.likelihood.raw_noise.grad]


def test_models_scattered_solver(engine):
    from variational_gridded_gaussian_processes_amd.models import Matern12GriddedGP
    X, y = data("trk400")
    Xt, yt, xs = torch.tensor(X), torch.tensor(y), torch.tensor(XS)
    mi = Matern12GriddedGP(Xt, yt, 17, (0, 1), (0, 1), engine=engine, scattered_solver="iterative").to(torch.float64)
    md = Matern12GriddedGP(Xt, yt, 17, (0, 1), (0, 1), engine=engine, scattered_solver="dense").to(torch.float64)
    qi, pi = mi.q_v(), mi.posterior(xs)
    assert mi._scattered and mi._siter and mi.last_info["sweeps"][0] == 16
    ei = mi._elbo()
    ei.backward()
    gi = _grads(mi)
    qd, pd = md.q_v(), md.posterior(xs)
    assert not md._siter
    ed = md._elbo()
    e_q, e_p = rel(qi.mean.numpy(), qd.mean.numpy()), rel(pi.mean.numpy(), pd.mean.numpy())
    e_elbo = abs(ei.item() - ed.item()) / max(abs(ed.item()), len(y) / 2.0)
    print(f"models: q(v) mean {e_q:.2e} posterior mean {e_p:.2e} ELBO {e_elbo:.2e}")
    assert qi.mean.shape == (256,) and e_q <= 1e-7 and e_p <= 1e-7
    assert e_elbo <= 1e-4
    assert len(gi) == 5 and all(g is not None and bool(torch.isfinite(g).all()) for g in gi)
    for dist in (qi, pi):
        with pytest.raises(NotImplementedError, match="follow-up"):
            dist.variance
        with pytest.raises(NotImplementedError, match="follow-up"):
            dist.covariance_matrix
    # 137 x 129 knots (M = 136 * 128 = 17408) on the same track points: the model sees a 400 x 400 grid with holes there, which `solver`
    # governs (iterative masked step, as before); it runs
    ma = Matern12GriddedGP(Xt, yt, 137, (0, 1), (0, 1), engine=engine, scattered_solver="auto").to(torch.float64)
    ma.mesh_2 = ma.b0_mesh_2 = torch.linspace(0, 1, 129)
    assert np.isfinite(ma._elbo().item()) and ma.last_info["rounds"][0] < 100 and not ma._siter
    # ... and on every second of them, which no grid holds any more (scattered X): "auto" takes the iterative scattered step where the
    # dense path raises
    Xs, ys = Xt[::2], yt[::2]
    mb = Matern12GriddedGP(Xs, ys, 137, (0, 1), (0, 1), engine=engine, scattered_solver="auto").to(torch.float64)
    mb.mesh_2 = mb.b0_mesh_2 = torch.linspace(0, 1, 129)
    assert mb._scattered
    eb = mb._elbo()
    eb.backward()
    assert mb._siter and np.isfinite(eb.item()) and mb.last_info["rounds"][0] < 100
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in _grads(mb))
    assert mb.q_v().mean.shape == (136 * 128,) and bool(torch.isfinite(mb.posterior(xs).mean).all())
    mdl = Matern12GriddedGP(Xs, ys, 137, (0, 1), (0, 1), engine=engine, scattered_solver="dense").to(torch.float64)
    mdl.mesh_2 = mdl.b0_mesh_2 = torch.linspace(0, 1, 129)
    with pytest.raises(ValueError, match="16384"):
        mdl._elbo()
    msm = Matern12GriddedGP(Xs, ys, 17, (0, 1), (0, 1), engine=engine)                 # auto, small M: dense
    assert msm._scattered and not msm._use_scattered_iterative(*msm._basis())
    with pytest.raises(ValueError):          # `solver` keeps its meaning: no iterative MASKED solver for scattered X
        Matern12GriddedGP(Xs, ys, 17, (0, 1), (0, 1), engine=engine, solver="iterative")
    with pytest.raises(ValueError):
        Matern12GriddedGP(Xt, yt, 17, (0, 1), (0, 1), engine=engine, scattered_solver="pcg")



def test_error_paths(engine):
    from variational_gridded_gaussian_processes_amd import Engine
    X, y = data("rand20k")
    X, y = X[:500], y[:500]
    g = np.linspace(0, 1, 9)
    yd, yy, xs = dev(y), float(y @ y), dev(XS)

    def codes(e, yv):
        out = []
        for call in (lambda: e.elbo_step_scattered_iter(yv, yy, S.THETA_A), e.qv_scattered_iter, lambda: e.posterior_scattered_iter(xs)):
            with pytest.raises(VggpError) as ei:
                call()
            out.append(ei.value.code)
        return out

    fresh = Engine(0)
    fresh.m1 = fresh.m2 = 8
    fresh.n1 = 500
    assert codes(fresh, yd) == [_lib.VGGP_ESTATE] * 3                                  # unplanned
    x1 = np.linspace(0, 1, 25)
    fresh.plan("matern12", "b0", g, x1, "matern12", "b0", g, x1[:20])                  # planned for a grid
    fresh.n1 = 500
    assert codes(fresh, yd) == [_lib.VGGP_EINVAL] * 3
    Z = np.random.default_rng(2).uniform(0, 1, (30, 2))
    fresh.plan_paired("matern12", Z, X[:, 0], X[:, 1], scattered=True)                 # paired inducing points
    assert codes(fresh, yd) == [_lib.VGGP_EINVAL] * 3
    fresh.close()
    multi = Engine(0, n_ranks=2, rank=0, allreduce=lambda buf: None)                   # multi-rank context
    multi.plan("matern12", "b0", g, X[:, 0], "matern12", "b0", g, X[:, 1], scattered=True, n_total=1000)
    assert codes(multi, yd) == [_lib.VGGP_EINVAL] * 3
    multi.close()
    # read-outs need the last finished step to be a successful iterative scattered one
    engine.plan("matern12", "b0", g, X[:, 0], "matern12", "b0", g, X[:, 1], scattered=True)
    for call in (engine.qv_scattered_iter, lambda: engine.posterior_scattered_iter(xs)):
        with pytest.raises(VggpError) as ei:
            call()
        assert ei.value.code == _lib.VGGP_ESTATE
    engine.elbo_step_scattered_iter(yd, yy, S.THETA_A)
    assert tuple(engine.qv_scattered_iter().shape) == (8, 8) and tuple(engine.posterior_scattered_iter(xs).shape) == (50,)
    with pytest.raises(VggpError) as ei:
        engine.elbo_step_scattered_iter(yd, yy, S.THETA_A, n_probes=64)
    assert ei.value.code == _lib.VGGP_EINVAL
    with pytest.raises(VggpError) as ei:                                               # ... and a failed step ends the state
        engine.qv_scattered_iter()
    assert ei.value.code == _lib.VGGP_ESTATE
    with pytest.raises(VggpError) as ei:
        engine.kr_field(dev(np.ones((3, 4))), dev(np.ones((3, 4))), dev(np.ones((3, 65, 3))))
    assert ei.value.code == _lib.VGGP_EINVAL
