"""VGGP_BASIS_B0K -- B0 cells under the Matern-3/2 and Matern-5/2 kernels -- from the factor kernel up to the model classes.

References: tests/golden/b0_kinds_hp.npz (50-digit quadrature of the cell integrals) and tests/b0_kinds_spec.py (the float64 closed
forms, pinned on that file by tests/test_b0_kinds_spec.py, and oracle.kron.Factor carrying them: B0KFactor), so every step, read-out
and model test below is the suite's usual comparison with oracle/kron.py, at the tolerances of the test it mirrors.

Factor tolerances (tests/factor_hp_cases.py's rule): |got - hp| <= 4 max(R, 1) eps S on the fixture's elements, 8 max(R, 1) eps S for
whole matrices against the float64 specification (both sides round); S the summand scale of the closed form, R the specification's
own measured constant (<= 1.7 over the fixture).  No element is skipped.
"""

import numpy as np
import pytest
import torch

import b0_kinds_spec as B
from oracle import dense as D, kron as Kr
from variational_gridded_gaussian_processes_amd import _lib
from variational_gridded_gaussian_processes_amd._lib import BASIS, KIND, VGGP_EINVAL, VGGP_OK

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.25
KINDS = ("matern32", "matern52")
RTOL = 1e-7                                   # tests/test_gpu_elbo.py


def dev(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def raw(engine, kind, basis, x, n, grid, m, ell, flags, outs):
    return engine.lib.vggp_factor_build(engine._h, KIND[kind], BASIS[basis], x, n, grid, m, float(ell), int(flags),
                                        outs[0], outs[1], outs[2], outs[3], torch.cuda.current_stream().cuda_stream)


# ---- 1. the factor kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", B.cases(), ids=B.case_ids())
def test_kernel_vs_50_digits(engine, c):
    outs = engine.factor_build(c.kind, "b0k", dev(c.x), dev(c.grid), c.ell)
    mats = [o.cpu().numpy() for o in outs]
    got = B.sample(c, mats)
    q = {k: B.ratio_to_bound(got[k], c.hp[k], c.S[k]) for k in B.OUTPUTS}
    with np.errstate(divide="ignore", invalid="ignore"):
        relerr = {k: float(np.nanmax(np.where(np.abs(c.hp[k]) > 1e-290, np.abs(got[k] - c.hp[k]) / np.abs(c.hp[k]), 0.0))) for k in B.OUTPUTS}
    print(f"{c.id}: err / (eps S) " + " ".join(f"{k} {q[k]:.2f}" for k in B.OUTPUTS) + f" (bound {B.tolerance_constant(c):.1f}); worst relative error "
          + " ".join(f"{k} {relerr[k]:.1e}" for k in B.OUTPUTS))
    for k, mat in zip(B.OUTPUTS, mats):
        assert np.isfinite(mat).all(), f"{k} is not finite"
    for k in B.OUTPUTS:
        assert q[k] <= B.tolerance_constant(c), (k, q[k])


# (m, n): A-part path / K-part path (csrc/factor_build.hip; every launch here has < 2^18 elements -> tmw = 2 but the last)
#   9 x 21       TALL, scalar stores (odd ncols) / K 9 x 9 scalar
#   33 x 130     TALL, 16-byte stores, two column tiles / K 33 x 33 scalar, five row groups
#   20 x 1024    WIDE, 16-byte stores / K 20 x 20 16-byte
#   20 x 1027    WIDE, scalar stores, the last tile holds three columns
#   64 x 4100    tmw = 4, WIDE 16-byte / K 64 x 64 TALL
SHAPES = [(9, 21), (33, 130), (20, 1024), (20, 1027), (64, 4100)]


def path_inputs(m, n):
    """every mesh knot is a column (so are the knots where a wave's and a tile's row group starts and the rolling-edge walk restarts),
    then points inside the mesh and outside it on both sides -- the columns of tests/test_gpu_factor_paths.py's B0 cases"""
    rng = np.random.default_rng(1000 * m + n)
    grid = np.linspace(0.0, 1.0, m + 1)
    x = np.concatenate([grid, rng.uniform(-0.1, 1.1, n - len(grid))])
    assert (x < 0).any() and (x > 1).any()
    return grid, x, 3.3 / m


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n", SHAPES, ids=[f"{m}x{n}" for m, n in SHAPES])
def test_every_tile_path_vs_spec(engine, m, n, kind):
    total = m * n + m * m
    assert (4 if total >= 1 << 18 else 2) == (4 if m == 64 else 2)
    grid, x, ell = path_inputs(m, n)
    xd, gd = dev(x), dev(grid)
    outs = engine.factor_build(kind, "b0k", xd, gd, ell)
    for o, o2 in zip(outs, engine.factor_build(kind, "b0k", xd, gd, ell)):
        assert torch.equal(o, o2)                       # bitwise repeatable
    ref, S, c = B.spec_outputs(kind, grid, x, ell), B.spec_scales(kind, grid, x, ell), B.family_constant(kind)
    worst = {}
    for k, o, r, s in zip(B.OUTPUTS, outs, ref, S):
        got = o.cpu().numpy()
        assert got.shape == r.shape
        worst[k] = B.ratio_to_bound(got, r, s)
    print(f"{m} x {n} {kind}: err / (eps S) " + " ".join(f"{k} {worst[k]:.2f}" for k in B.OUTPUTS) + f" (bound {c:.1f})")
    for k in B.OUTPUTS:
        assert worst[k] <= c, (k, worst[k])
    # only K, only A (and each single output): the requested ones to the bit, the others keep their sentinel
    for mask in ((False, False, True, True), (True, True, False, False), (True, False, False, False), (False, False, False, True)):
        bufs = [torch.full_like(f, SENTINEL) for f in outs]
        rc = raw(engine, kind, "b0k", xd.data_ptr(), n, gd.data_ptr(), m, ell, 0, [b.data_ptr() if w else None for b, w in zip(bufs, mask)])
        assert rc == VGGP_OK, mask
        torch.cuda.synchronize()
        for b, f, w in zip(bufs, outs, mask):
            assert torch.equal(b, f) if w else bool((b == SENTINEL).all()), mask


# ---- 2. Matern-1/2 under B0K is B0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(33, 130), (20, 1027)])
def test_b0k_equals_b0_for_matern12(engine, m, n):
    grid, x, ell = path_inputs(m, n)
    a = engine.factor_build("matern12", "b0k", dev(x), dev(grid), ell)
    b = engine.factor_build("matern12", "b0", dev(x), dev(grid), ell)
    for o, o2 in zip(a, b):
        assert torch.equal(o, o2)


# ---- 3. contract ---------------------------------------------------------------------------------------------------------------
def test_contract(engine):
    """VGGP_EINVAL from vggp_factor_build and vggp_plan for RBF cells and for VGGP_FLAG_B0_F32_KDELTA with B0K; nothing is written, and
    the context's plan stays what it was.  VGGP_BASIS_B0 keeps refusing the other kernels (tests/test_gpu_factor_paths.py)."""
    m, n = 9, 21
    xn, meshn = np.linspace(0, 1, n), np.linspace(0, 1, m + 1)
    x, mesh = dev(xn), dev(meshn)
    bufs = [torch.full((m, n), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(2)] + \
           [torch.full((m, m), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(2)]
    ptrs = [b.data_ptr() for b in bufs]
    assert raw(engine, "rbf", "b0k", x.data_ptr(), n, mesh.data_ptr(), m, 0.3, 0, ptrs) == VGGP_EINVAL
    for kind in ("matern12", "matern32", "matern52"):
        assert raw(engine, kind, "b0k", x.data_ptr(), n, mesh.data_ptr(), m, 0.3, _lib.FLAG_B0_F32_KDELTA, ptrs) == VGGP_EINVAL
    assert raw(engine, "matern32", "b0k", x.data_ptr(), n, mesh.data_ptr(), m, 0.0, 0, ptrs) == VGGP_EINVAL
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in bufs)
    engine.plan("matern32", "b0k", meshn, xn, "matern32", "b0k", meshn, xn)
    token = engine.plan_token
    for args, kw in ((("rbf", "b0k", meshn, xn, "rbf", "b0k", meshn, xn), {}),
                     (("matern32", "b0k", meshn, xn, "rbf", "b0k", meshn, xn), {}),
                     (("matern32", "b0k", meshn, xn, "matern32", "b0k", meshn, xn), {"b0_f32_kdelta": True}),
                     (("matern12", "b0", meshn, xn, "matern52", "b0k", meshn, xn), {"b0_f32_kdelta": True}),
                     (("matern32", "b0", meshn, xn, "matern32", "b0", meshn, xn), {})):
        with pytest.raises(_lib.VggpError) as e:
            engine.plan(*args, **kw)
        assert e.value.code == VGGP_EINVAL
    assert engine.plan_token == token
    Y = dev(np.sin(3 * xn)[None, :] * np.cos(2 * xn)[:, None])
    elbo, grad, info = engine.elbo_step(Y, engine.sumsq(Y), [0.3, 0.3, 1.0, 1.0, 0.1])      # the earlier plan still steps
    assert info["status"] == 0 and np.isfinite(elbo)
    assert raw(engine, "matern52", "b0k", x.data_ptr(), n, mesh.data_ptr(), m, 0.3, 0, ptrs) == VGGP_OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.stack([b.sum() for b in bufs])).all())


# ---- 4. full-grid step ---------------------------------------------------------------------------------------------------------
def b0k(kind, knots):
    return ("b0k", kind, np.linspace(0, 1, knots))


def pts(kind, m):
    return ("points", kind, np.linspace(0, 1, m))


def oracle_factor(d, x):
    basis, kind, g = d
    return B.factor(kind, g, x) if basis == "b0k" else Kr.Factor(basis, kind, np.asarray(g, float), x)


# the shapes of tests/test_gpu_elbo.py::test_elbo_step_vs_oracle's two B0 cases (the second at the default-initialised theta), and a
# step whose dimensions differ in kernel and basis
STEP_CASES = [(24, 20, b0k(k, 8), b0k(k, 10), [0.2, 0.3, 1.0, 0.8, 0.01]) for k in KINDS] + \
             [(200, 300, b0k(k, 33), b0k(k, 21), [0.6931, 0.6931, 0.6931, 0.6931, 0.6932]) for k in KINDS] + \
             [(40, 33, b0k("matern32", 13), pts("matern52", 12), [0.25, 0.2, 1.3, 0.7, 0.01])]


@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: f"{c[2][0]}-{c[2][1]}-x-{c[3][0]}-{c[3][1]}-{c[0]}x{c[1]}")
def test_elbo_step_vs_oracle(engine, case):
    n1, n2, d1, d2, theta = case
    X, y, x1, x2 = D.gen_grid(n1, n2)
    f1, f2 = oracle_factor(d1, x1), oracle_factor(d2, x2)
    st = Kr.elbo_step(y.reshape(n2, n1), f1, f2, theta)
    engine.plan(d1[1], d1[0], d1[2], x1, d2[1], d2[0], d2[2], x2)
    Y = torch.tensor(y.reshape(n2, n1), device=DEV)
    elbo, grad, info = engine.elbo_step(Y, engine.sumsq(Y), theta)
    mean, var = engine.qv()
    rm, rv = Kr.q_v(st)
    xs = np.random.default_rng(5).uniform(0, 1, (1000, 2))
    pm, pv = engine.posterior(torch.tensor(xs, device=DEV))
    om, ov = Kr.posterior(st, f1, f2, xs)
    print(f"jitter {info['jitter']} (oracle {(st.d1.jit, st.d2.jit)}), sweeps {info['sweeps']}; ELBO {abs(elbo - st.elbo) / abs(st.elbo):.1e} "
          f"grad {rel(grad, st.grad):.1e} qv {rel(mean.cpu().numpy(), rm):.1e} {rel(var.cpu().numpy(), rv):.1e} "
          f"posterior {rel(pm.cpu().numpy(), om):.1e} {rel(pv.cpu().numpy(), ov):.1e}")
    assert info["status"] == 0
    assert info["jitter"] == (st.d1.jit, st.d2.jit)
    assert abs(elbo - st.elbo) <= RTOL * abs(st.elbo)
    assert rel(grad, st.grad) < RTOL
    assert rel(mean.cpu().numpy(), rm) < RTOL
    assert rel(var.cpu().numpy(), rv) < RTOL
    assert rel(pm.cpu().numpy(), om) < RTOL
    assert rel(pv.cpu().numpy(), ov) < 1e-6


# ---- 5. warm trajectory --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_warm_trajectory_stays_on_the_oracle(engine, kind):
    """12 warm-started steps on a 64 x 64 grid, 32 cells per dimension, along the path of tests/test_gpu_elbo.py::
    test_long_warm_trajectory_stays_on_the_oracle and at its tolerances (ELBO 1e-9, gradient and q(v) 1e-8), every step checked: the
    refinement / polish / Newton chains of the step meet the spectra of these factors here.  A step may fall back to sweeps; its
    numbers may not move."""
    n, knots = 64, 33
    X, y, x1, x2 = D.gen_grid(n, n)
    d = b0k(kind, knots)
    f1, f2 = oracle_factor(d, x1), oracle_factor(d, x2)
    engine.plan(kind, "b0k", d[2], x1, kind, "b0k", d[2], x2, warm_start=True)
    Y = torch.tensor(y.reshape(n, n), device=DEV)
    yy = engine.sumsq(Y)
    th0 = np.array([0.2, 0.25, 1.0, 1.1, 0.01])
    for k in range(12):
        th = th0 * (1 + 0.01 * k + 0.003 * np.sin(k))
        elbo, grad, info = engine.elbo_step(Y, yy, th)
        ref = Kr.elbo_step(y.reshape(n, n), f1, f2, th)
        print(f"step {k}: sweeps {info['sweeps']} rounds {info['rounds']} polished {info['polished']} jitter {info['jitter']}; "
              f"ELBO {abs(elbo - ref.elbo) / abs(ref.elbo):.1e} grad {rel(grad, ref.grad):.1e}")
        assert info["status"] == 0 and info["jitter"] == (ref.d1.jit, ref.d2.jit), k
        assert abs(elbo - ref.elbo) <= 1e-9 * abs(ref.elbo), k
        assert rel(grad, ref.grad) < 1e-8, k
    mean, var = engine.qv()
    rm, rv = Kr.q_v(ref)
    assert rel(mean.cpu().numpy(), rm) < 1e-8 and rel(var.cpu().numpy(), rv) < 1e-8


# ---- 6. dense masked and scattered steps -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_masked_step_vs_oracle(engine, kind):
    """32 x 32 grid, 30 % missing, 8 cells per dimension: tests/test_gpu_elbo.py::test_masked_step_vs_oracle's B0 case and tolerances"""
    n1 = n2 = 32
    d, theta = b0k(kind, 9), [0.25, 0.2, 1.0, 1.2, 0.01]
    X, y, x1, x2 = D.gen_grid(n1, n2)
    Wn = (np.random.default_rng(1).uniform(size=(n2, n1)) > 0.3).astype(np.float64)
    f1, f2 = oracle_factor(d, x1), oracle_factor(d, x2)
    st = Kr.elbo_step_masked(y.reshape(n2, n1), Wn, f1, f2, theta)
    engine.plan(kind, "b0k", d[2], x1, kind, "b0k", d[2], x2)
    W = torch.tensor(Wn, device=DEV)
    Ym = torch.tensor(y.reshape(n2, n1), device=DEV) * W
    elbo, grad, info = engine.elbo_step_masked(Ym, W, float(Wn.sum()), engine.sumsq(Ym), theta)
    assert info["status"] == 0
    assert abs(elbo - st.elbo) <= RTOL * abs(st.elbo)
    assert rel(grad, st.grad) < RTOL
    mean, var = engine.qv_masked()
    rm, rv = Kr.q_v_masked(st)
    assert rel(mean.cpu().numpy(), rm) < RTOL and rel(var.cpu().numpy(), rv) < RTOL
    xs = np.random.default_rng(9).uniform(0, 1, (3 * 81 + 5, 2))
    pm, pv = engine.posterior_masked(torch.tensor(xs, device=DEV))
    om, ov = Kr.posterior_masked(st, f1, f2, xs)
    assert rel(pm.cpu().numpy(), om) < RTOL and rel(pv.cpu().numpy(), ov) < 1e-6


@pytest.mark.parametrize("kind", KINDS)
def test_scattered_step_vs_oracle(engine, kind):
    """500 points that form no grid, 7 x 9 cells: tests/test_gpu_elbo.py::test_scattered_step_vs_oracle's problem and tolerances"""
    N = 500
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (N, 2))
    y = np.sin(5 * X[:, 0]) * np.cos(3 * X[:, 1]) + 0.1 * rng.standard_normal(N)
    th = np.array([0.3, 0.25, 1.2, 0.8, 0.05])
    g1, g2 = np.linspace(0, 1, 8), np.linspace(0, 1, 10)
    f1, f2 = B.factor(kind, g1, np.zeros(1)), B.factor(kind, g2, np.zeros(1))
    ref = B.elbo_step_scattered(X, y, f1, f2, th)
    engine.plan(kind, "b0k", g1, X[:, 0].copy(), kind, "b0k", g2, X[:, 1].copy(), scattered=True)
    elbo, grad, info = engine.elbo_step_scattered(torch.tensor(y, device=DEV), float(y @ y), th)
    assert abs(elbo - ref.elbo) <= RTOL * abs(ref.elbo)
    assert rel(grad, ref.grad) < RTOL
    mean, var = engine.qv_masked()
    rm, rv = Kr.q_v_masked(ref, f1, f2)
    assert rel(mean.cpu().numpy(), rm) < 1e-6 and rel(var.cpu().numpy(), rv) < 1e-6
    xs = rng.uniform(0, 1, (40, 2))
    pm, pv = engine.posterior_masked(torch.tensor(xs))
    qm, qv = Kr.posterior_masked(ref, f1, f2, xs)
    assert rel(pm.cpu().numpy(), qm) < 1e-6 and rel(pv.cpu().numpy(), qv) < 1e-6


# ---- 7. iterative masked step ----------------------------------------------------------------------------------------------------
ITER_N, ITER_CELLS = 96, 12


def test_iterative_masked_step_vs_dense(engine):
    """vggp_elbo_step_masked_iter against the dense masked step of the same context on the problem of tests/test_gpu_elbo.py::
    test_iterative_masked_step_vs_dense_small (96 x 96 grid, 12 cells per dimension, a Bernoulli(0.7) and a track-shaped mask, the
    relative tolerance taken on max(|ELBO|, N / 2), repeated calls deterministic) with Matern-3/2 cells, at the estimator's stated
    tolerances: ELBO 1e-5, gradient 1e-4 of its largest component.  Measured on the MI355X (fixed probes: the same bits every run):
    Bernoulli 9.1e-6 / 2.8e-5, tracks 1.3e-6 / 4.8e-5 -- the differences are the probe estimator's noise, which is what those two
    figures bound (Matern-1/2 cells on the same problem: 8.5e-6 / 7.3e-6 and 8.6e-7 / 7.5e-7)."""
    from variational_gridded_gaussian_processes_amd import datagen as G
    n = ITER_N
    X, y, x1, x2 = D.gen_grid(n, n)
    theta = [0.2, 0.3, 1.0, 0.8, 0.01]
    masks = [(np.random.default_rng(1).uniform(size=(n, n)) < 0.7).astype(np.float64), G.track_mask(n, n, 2, 0.5)]
    g = np.linspace(0, 1, ITER_CELLS + 1)
    engine.plan("matern32", "b0k", g, x1, "matern32", "b0k", g, x2)
    for Wn in masks:
        W = torch.tensor(Wn, device=DEV)
        Ym = torch.tensor(y.reshape(n, n), device=DEV) * W
        yy, nobs = engine.sumsq(Ym), float(Wn.sum())
        e_d, g_d, _ = engine.elbo_step_masked(Ym, W, nobs, yy, theta)
        elbo, grad, info = engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta, n_probes=16)
        print(f"observed {nobs / n / n:.2f}: PCG rounds {info['rounds'][0]}; ELBO {abs(elbo - e_d) / max(abs(e_d), 0.5 * nobs):.1e} "
              f"grad {np.abs(grad - g_d).max() / np.abs(g_d).max():.1e}")
        assert info["status"] == 0 and 0 < info["rounds"][0] < 60
        assert abs(elbo - e_d) <= 1e-5 * max(abs(e_d), 0.5 * nobs), (elbo, e_d)
        assert np.abs(grad - g_d).max() <= 1e-4 * np.abs(g_d).max(), (grad, g_d)
        e2, g2, _ = engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta, n_probes=16)
        e3, g3, _ = engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta, n_probes=16)
        assert e3 == e2 and np.array_equal(g3, g2)


# ---- 8. model classes ------------------------------------------------------------------------------------------------------------
def track_problem(N=400):
    rng = np.random.default_rng(4)
    t = np.linspace(0, 1, N)
    X = np.stack([(0.5 + 0.45 * np.sin(9 * t) + 0.01 * rng.standard_normal(N)).clip(0, 1),
                  (t + 0.02 * rng.standard_normal(N)).clip(0, 1)], axis=1)          # a wiggly track (tests/test_gpu_models.py)
    y = np.sin(5 * X[:, 0]) * np.cos(3 * X[:, 1]) + 0.05 * rng.standard_normal(N)
    return X, y


def raw_grads(model):
    return np.array([model.kernel_1.base_kernel.raw_lengthscale.grad.item(), model.kernel_2.base_kernel.raw_lengthscale.grad.item(),
                     model.kernel_1.raw_outputscale.grad.item(), model.kernel_2.raw_outputscale.grad.item(),
                     model.likelihood.raw_noise.grad.item()])


def test_matern32_gridded_model_on_scattered_points(engine):
    import variational_gridded_gaussian_processes_amd.models as M
    X, y = track_problem()
    nk = 9
    model = M.Matern32GriddedGP(torch.tensor(X), torch.tensor(y), nk, (0, 1), (0, 1), engine=engine).to(torch.float64)
    assert model._scattered and model._basis()[0] == "b0k" and M.Matern32B0SplineGriddedGP is M.Matern32GriddedGP
    mesh = torch.linspace(0, 1, nk).double().numpy()                 # the model's float32-born knots, as doubles
    f1, f2 = B.factor("matern32", mesh, np.zeros(1)), B.factor("matern32", mesh, np.zeros(1))
    raw0 = np.zeros(5)
    ref = B.elbo_step_scattered(X, y, f1, f2, Kr.theta_from_raw(raw0))
    (-model._elbo()).backward()
    assert rel(-raw_grads(model), Kr.grad_raw(ref.grad, raw0)) < 1e-6
    qv = model.q_v()
    rm, rv = Kr.q_v_masked(ref, f1, f2)
    assert rel(qv.mean.numpy(), rm.reshape(-1)) < 1e-6 and rel(qv.variance.numpy(), rv.reshape(-1)) < 1e-6      # (flat index a * m2 + b)
    a1, a2 = torch.linspace(0.02, 0.97, 23, dtype=torch.float64), torch.linspace(-0.05, 1.05, 17, dtype=torch.float64)
    pg, pp = model.posterior_grid(a1, a2), model.posterior(torch.cartesian_prod(a1, a2))
    om, ov = Kr.posterior_masked(ref, f1, f2, torch.cartesian_prod(a1, a2).numpy())
    assert rel(pp.mean.numpy(), om) < 1e-6 and rel(pp.variance.numpy(), ov) < 1e-6
    assert rel(pg.mean.numpy(), pp.mean.numpy()) < 1e-6          # tests/test_gpu_posterior_raster.py, scattered state
    # the basis object evaluates the cells of the model's kernel
    Phi = model.basis_1.cell_integrals(torch.tensor(X[:50, 0]), 0.3).numpy()
    assert B.ratio_to_bound(Phi, B.b0k_A("matern32", mesh, X[:50, 0], 0.3)[0], B.S_b0k_A("matern32", mesh, X[:50, 0], 0.3)[0]) <= B.family_constant("matern32")


def test_matern52_gridded_model_takes_a_step(engine):
    import variational_gridded_gaussian_processes_amd.models as M
    X, y, x1, x2 = D.gen_grid(24, 20)
    model = M.Matern52B0SplineGriddedGP(torch.tensor(X), torch.tensor(y), 9, (0, 1), (0, 1), engine=engine).to(torch.float64)
    assert type(model) is M.Matern52GriddedGP and model.kind == "matern52" and not model._scattered
    mesh = torch.linspace(0, 1, 9).double().numpy()
    ref = Kr.elbo_step(y.reshape(20, 24), B.factor("matern52", mesh, x1), B.factor("matern52", mesh, x2), Kr.theta_from_raw(np.zeros(5)))
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    opt.zero_grad()
    loss = -model._elbo()
    loss.backward()
    assert abs(-loss.item() - ref.elbo) <= 1e-6 * abs(ref.elbo)
    assert rel(-raw_grads(model), Kr.grad_raw(ref.grad, np.zeros(5))) < 1e-6
    opt.step()
    qv = model.q_v()
    assert qv.mean.shape == (64,) and bool(torch.isfinite(qv.variance).all()) and float(qv.variance.min()) > 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_univariate_twin(engine, kind):
    """univariate.Matern32 / Matern52B0SplineGriddedGP: the same engine with a trivial second factor"""
    from variational_gridded_gaussian_processes_amd.models import univariate
    n, nknots = 130, 17
    x = np.linspace(0, 2 * np.pi, n)
    y = np.sin(x) + np.cos(x) + 0.05 * np.random.default_rng(0).standard_normal(n)
    cls = univariate.Matern32B0SplineGriddedGP if kind == "matern32" else univariate.Matern52B0SplineGriddedGP
    model = cls(torch.tensor(x), torch.tensor(y), nknots, (0, 2 * np.pi), engine=engine).to(torch.float64)
    mesh = torch.linspace(0, 2 * np.pi, nknots).double().numpy()
    th = model._theta().detach().numpy()
    ref = Kr.elbo_step(y.reshape(1, n), B.factor(kind, mesh, x), Kr.Factor("one", "matern12", np.ones(1), np.zeros(1)), th)
    e = model._elbo()
    assert abs(e.item() - ref.elbo) <= 1e-6 * abs(ref.elbo)
    qv = model.q_v()
    rm, rv = Kr.q_v(ref)
    assert rel(qv.mean.numpy(), rm.reshape(-1)) < 1e-6 and rel(qv.variance.numpy(), rv.reshape(-1)) < 1e-6


# ---- 9. one size case ------------------------------------------------------------------------------------------------------------
def test_size_case_matern32_256x256_128_cells(engine):
    """256 x 256 grid, 128 cells per dimension, Matern-3/2, against the structured oracle at the tolerances of tests/test_gpu_elbo.py::
    test_config3_full_size_matern32_vs_structured_oracle (jitter equal, ELBO 1e-8, gradient and q(v) 1e-6)"""
    n, m = 256, 128
    X, y, x1, x2 = D.gen_grid(n, n)
    d = b0k("matern32", m + 1)
    f1, f2 = oracle_factor(d, x1), oracle_factor(d, x2)
    theta = [0.2, 0.2, 1.0, 1.0, 0.0025]
    ref = Kr.elbo_step(y.reshape(n, n), f1, f2, theta)
    engine.plan("matern32", "b0k", d[2], x1, "matern32", "b0k", d[2], x2)
    Y = torch.tensor(y.reshape(n, n), device=DEV)
    elbo, grad, info = engine.elbo_step(Y, engine.sumsq(Y), theta)
    mean, var = engine.qv()
    rm, rv = Kr.q_v(ref)
    print(f"jitter {info['jitter']} (oracle {(ref.d1.jit, ref.d2.jit)}); ELBO {abs(elbo - ref.elbo) / abs(ref.elbo):.1e} grad {rel(grad, ref.grad):.1e} "
          f"qv {rel(mean.cpu().numpy(), rm):.1e} {rel(var.cpu().numpy(), rv):.1e}")
    assert (info["jitter"][0], info["jitter"][1]) == (ref.d1.jit, ref.d2.jit)
    assert abs(elbo - ref.elbo) <= 1e-8 * abs(ref.elbo)
    assert rel(grad, ref.grad) < 1e-6
    assert rel(mean.cpu().numpy(), rm) < 1e-6 and rel(var.cpu().numpy(), rv) < 1e-6
