"""Steps whose two dimensions use different kernel families, bases, m and n, against oracle/kron.py (per-dimension throughout; for
these combinations checked against the per-dimension dense restatement on the CPU, tests/test_oracle.py).

Every other GPU test plans the same kind and the same basis in both dimensions, so a line of csrc/ that reads dimension 1's
attribute where it means dimension 2's is invisible to them.  Here s1 != s2, ell1 != ell2, m1 != m2 (and n1 != n2 wherever the grid
is not prescribed), so that no exchange can cancel.  Every bound is the bound an existing test uses for the same entry point; the
docstrings name it."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mixed_dims_cases as MX
import scattered_iter_spec as S
from oracle import dense as D
from oracle import kron as Kr
from test_gpu_readout_states import TOL_PM, TOL_PV, TOL_QV, _cells, _check
from variational_gridded_gaussian_processes_amd import datagen as G
from variational_gridded_gaussian_processes_amd._lib import VggpError, check

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-7                                   # test_gpu_elbo.py
XS = np.random.default_rng(2).uniform(-0.05, 1.05, (64, 2))          # a few points outside the data range


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def _np(t):
    return t.cpu().numpy()


# ---- the gridded read-out's operands for any dimension ---------------------------------------------------------------------------------
def _mesh(d, slot):
    """Output mesh of a dimension: the B1 hats' inner knots (as the reference pads them), else 7 or 5 cells by the dimension's slot."""
    if d.basis == "b1":
        return np.asarray(d.grid, float)[2:-2]
    return (np.linspace(0, 1, 8), np.linspace(0.1, 0.9, 6))[slot]


def _cross(d, f, mesh, ell):
    """Kr.cross_b0 where it exists, Gauss-Legendre cell integrals for the other kinds and for B0 inducing features."""
    return MX.gl_cells(d, mesh, ell) if d.basis == "b0" else _cells(f, mesh, ell)


def _operands(d1, d2, f1, f2, theta, slots=(0, 1)):
    C1, kd1 = _cross(d1, f1, _mesh(d1, slots[0]), theta[0])
    C2, kd2 = _cross(d2, f2, _mesh(d2, slots[1]), theta[1])
    assert C1.shape == (len(kd1), f1.m) and C2.shape == (len(kd2), f2.m) and len(kd1) != len(kd2)
    return C1, C2, kd1, kd2


# ---- full-grid problems -----------------------------------------------------------------------------------------------------------------
def _grid(d1, d2, n, theta, order="ab"):
    a1, a2, x1, x2, Y, _, _, th = MX.grid_problem(d1, d2, n, theta, order)
    return SimpleNamespace(d1=a1, d2=a2, x1=x1, x2=x2, Y=Y, theta=th, f1=MX.factor(a1, x1), f2=MX.factor(a2, x2),
                           slots=(0, 1) if order == "ab" else (1, 0), xs=XS if order == "ab" else XS[:, ::-1].copy())


def _full_reference(P, st, theta):
    """Every read-out of the full-grid step from the oracle's state."""
    ops = _operands(P.d1, P.d2, P.f1, P.f2, theta, P.slots)
    M = P.f1.m * P.f2.m
    return dict(ops=ops, qv=Kr.q_v(st), qv_cov=Kr.q_v_cov(st) if M <= 4096 else None, post=Kr.posterior(st, P.f1, P.f2, P.xs),
                post_cov=Kr.posterior_cov(st, P.f1, P.f2, P.xs), ro={lit: Kr.readout(st, P.f1, P.f2, *ops, literal=lit) for lit in (True, False)})


def _full_readouts(engine, P, R, tag=""):
    """qv, posterior, qv_cov, posterior_cov and both gridded read-outs -> [(label, error, bound)], bounds of test_gpu_readout_states."""
    xs = dev(P.xs)
    mean, var = engine.qv()
    pm, pv = engine.posterior(xs)
    figs = [(tag + "qv mean", rel(_np(mean), R["qv"][0]), TOL_QV), (tag + "qv var", rel(_np(var), R["qv"][1]), TOL_QV),
            (tag + "posterior mean", rel(_np(pm), R["post"][0]), TOL_PM), (tag + "posterior var", rel(_np(pv), R["post"][1]), TOL_PV)]
    if R["qv_cov"] is not None:
        figs.append((tag + "qv_cov", rel(_np(engine.qv_cov()), R["qv_cov"]), TOL_QV))
    figs.append((tag + "posterior_cov", rel(_np(engine.posterior_cov(xs)), R["post_cov"]), TOL_PV))
    ops = [torch.tensor(a) for a in R["ops"]]
    for lit in (True, False):
        m_, v_ = engine.readout(*ops, literal=lit)
        rm, rv = R["ro"][lit]
        assert tuple(m_.shape) == rm.shape and rm.shape[0] != rm.shape[1]
        name = tag + ("readout literal" if lit else "readout conditional")
        figs += [(name + " mean", rel(_np(m_), rm), TOL_QV), (name + " var", rel(_np(v_), rv), TOL_PV)]
    return figs, (mean, var, pm, pv)


@functools.lru_cache(maxsize=None)
def _cold_case(name, order):
    d1, d2, n, theta = MX.FULL[name]
    P = _grid(d1, d2, n, theta, order)
    P.st = Kr.elbo_step(P.Y, P.f1, P.f2, P.theta)
    P.R = _full_reference(P, P.st, P.theta)
    return P


def _cold_step(engine, P):
    engine.plan(*MX.plan_args(P.d1, P.x1, P.d2, P.x2))
    Y = dev(P.Y)
    return engine.elbo_step(Y, engine.sumsq(Y), P.theta)


# ---- a: the cold full-grid step and all its read-outs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", MX.ORDERS)
@pytest.mark.parametrize("name", list(MX.FULL))
def test_cold_step_and_readouts(engine, name, order):
    """RBF-points x VFF, B0 x Matern-3/2 points, B1 x Matern-5/2 points, Matern-3/2 x Matern-5/2 points, each in both orders: status,
    the jitter pair (two different entries for RBF x VFF), ELBO, gradient at the 1e-7 of test_elbo_step_vs_oracle; qv, posterior (points
    inside and slightly outside the unit square), qv_cov, posterior_cov and the literal / conditional gridded read-out on output
    meshes of different sizes at the bounds of test_gpu_readout_states."""
    P = _cold_case(name, order)
    st = P.st
    elbo, grad, info = _cold_step(engine, P)
    assert info["status"] == 0
    assert info["jitter"] == (st.d1.jit, st.d2.jit), info
    if name.startswith("rbf"):
        assert info["jitter"][0] != info["jitter"][1]
    figs = [("elbo", abs(elbo - st.elbo) / abs(st.elbo), RTOL), ("grad", rel(grad, st.grad), RTOL)]
    figs += _full_readouts(engine, P, P.R)[0]
    _check(figs, f"{name}/{order}")


@pytest.mark.parametrize("name", list(MX.FULL))
def test_transposed_twin(engine, name):
    """The B x A plan on Y^T with theta[[1, 0, 3, 2, 4]] is the same model as the A x B plan: same ELBO, gradient permuted, q(v)
    transposed, the posterior at column-swapped points equal.  Each side is within its bound of the oracle (the test above), so the
    direct comparison gets the sum of the two bounds."""
    out = {}
    for order in MX.ORDERS:
        P = _cold_case(name, order)
        elbo, grad, info = _cold_step(engine, P)
        assert info["status"] == 0
        mean, var = engine.qv()
        pm, pv = engine.posterior(dev(P.xs))
        out[order] = (elbo, grad, _np(mean), _np(var), _np(pm), _np(pv))
    a, b = out["ab"], out["ba"]
    _check([("elbo", abs(b[0] - a[0]) / abs(a[0]), 2 * RTOL), ("grad", rel(b[1][MX.SWAP], a[1]), 2 * RTOL),
            ("qv mean", rel(b[2].T, a[2]), 2 * TOL_QV), ("qv var", rel(b[3].T, a[3]), 2 * TOL_QV),
            ("posterior mean", rel(b[4], a[4]), 2 * TOL_PM), ("posterior var", rel(b[5], a[5]), 2 * TOL_PV)], f"{name}: B x A on Y^T against A x B")


# ---- b: the inducing-point gradient with exactly one points dimension -----------------------------------------------------------------------
GUARD = 64
ZGRAD = {"m32_pts7-b0_9": (MX.irregular("matern32", 7), MX.b0(9)), "b0_9-m32_pts7": (MX.b0(9), MX.irregular("matern32", 7)),
         "vff_9-m52_pts6": (MX.vff(4), MX.irregular("matern52", 6))}


def _zgrad_raw(engine, fn, data):
    """The raw C call with outputs of m_d doubles each followed by a guard, all pre-filled with NaN: -> (g1 [m1], g2 [m2]) after checking
    that nothing behind the m_d-th entry was written."""
    bufs = [torch.full((m + GUARD,), float("nan"), dtype=torch.float64, device=DEV) for m in (engine.m1, engine.m2)]
    check(fn(engine._h, data.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(), torch.cuda.current_stream(engine.device).cuda_stream))
    torch.cuda.synchronize()
    out = []
    for b, m in zip(bufs, (engine.m1, engine.m2)):
        assert bool(torch.isnan(b[m:]).all()), "written beyond m entries"
        out.append(_np(b[:m]))
    return out


def _assert_one_sided(got, ref, fs, tol, what):
    for d in (0, 1):
        if fs[d].basis == "points":
            err = rel(got[d], ref[d])
            print(f"{what}: zgrad {d + 1}: {err:.3e} (bound {tol:.0e})")
            assert err < tol, (what, d, err)
        else:
            assert got[d].shape == (fs[d].m,) and not ref[d].any()
            assert np.array_equal(got[d], np.zeros(fs[d].m)), (what, d, got[d])          # zeros, exactly -- not NaN, not small


@pytest.mark.parametrize("name", list(ZGRAD))
def test_zgrad_with_one_points_dimension(engine, name):
    """vggp_zgrad when only one dimension has inducing points (irregular, as in test_zgrad_vs_oracle): the points dimension against
    Kr.z_grad at that test's 1e-6, the other output all zeros, exactly m long; cold and after three warm steps.  vggp_set_inducing on
    the dimension without points must refuse."""
    d1, d2 = ZGRAD[name]
    n1, n2 = 40, 33
    _, y, x1, x2 = D.gen_grid(n1, n2)
    Yn = y.reshape(n2, n1)
    f1, f2 = MX.factor(d1, x1), MX.factor(d2, x2)
    engine.plan(*MX.plan_args(d1, x1, d2, x2), warm_start=True)
    Y = dev(Yn)
    yy = engine.sumsq(Y)
    th0 = np.array([0.21, 0.27, 1.2, 0.9, 0.02])
    for k in range(4):
        th = th0 * (1 + 0.01 * k)
        elbo, grad, info = engine.elbo_step(Y, yy, th)
        assert info["status"] == 0
        if k in (0, 3):
            ref = Kr.elbo_step(Yn, f1, f2, th)
            assert abs(elbo - ref.elbo) <= 1e-8 * abs(ref.elbo) and rel(grad, ref.grad) < 1e-6
            got = _zgrad_raw(engine, engine.lib.vggp_zgrad, Y)
            _assert_one_sided(got, Kr.z_grad(ref, f1, f2, Yn), (f1, f2), 1e-6, f"{name} step {k}")
    other = 0 if d1.basis != "points" else 1
    with pytest.raises(VggpError):
        engine.set_inducing(other, np.linspace(0, 1, (f1, f2)[other].m))


@pytest.mark.parametrize("name", list(ZGRAD))
def test_zgrad_scattered_with_one_points_dimension(engine, name):
    """The same for vggp_zgrad_scattered on 2000 scattered points, at the 1e-6 test_zgrad_scattered_vs_oracle uses for Matern kernels."""
    d1, d2 = ZGRAD[name]
    rng = np.random.default_rng(8)
    N = 2000
    X = rng.uniform(0, 1, (N, 2))
    y = np.sin(5 * X[:, 0]) * np.cos(4 * X[:, 1]) + 0.05 * rng.normal(size=N)
    th = np.array([0.21, 0.27, 1.2, 0.9, 0.02])
    f1, f2 = MX.factor(d1, X[:, 0].copy()), MX.factor(d2, X[:, 1].copy())
    engine.plan(*MX.plan_args(d1, X[:, 0].copy(), d2, X[:, 1].copy()), scattered=True)
    yd = dev(y)
    ref = Kr.elbo_step_scattered(X, y, f1, f2, th)
    elbo, grad, info = engine.elbo_step_scattered(yd, float(y @ y), th)
    assert info["status"] == 0 and abs(elbo - ref.elbo) <= 1e-8 * abs(ref.elbo)
    got = _zgrad_raw(engine, engine.lib.vggp_zgrad_scattered, yd)
    _assert_one_sided(got, Kr.z_grad_scattered(ref, X, y, f1, f2), (f1, f2), 1e-6, name)
    other = 0 if d1.basis != "points" else 1
    with pytest.raises(VggpError):
        engine.set_inducing(other, np.linspace(0, 1, (f1, f2)[other].m))


# ---- c: the dense masked and scattered steps --------------------------------------------------------------------------------------------------
PAIRS = {"m12_vff9-m12_pts8": (MX.vff(4), MX.pts("matern12", 8)), "rbf_pts6-m32_pts5": (MX.pts("rbf", 6), MX.pts("matern32", 5))}
THETA_C = np.array([0.3, 0.25, 1.3, 0.7, 0.02])


def _dense_readouts(engine, st, d1, d2, f1, f2, xs, tol_q, tol_pm, tol_pv, what):
    """qv_masked, posterior_masked, the two dense covariances (which share their diagonals with them: the same bounds) and, for a
    Matern-1/2 pair, readout_masked -- from the M-space state of a dense masked or scattered step."""
    mean, var = engine.qv_masked()
    rm, rv = Kr.q_v_masked(st, f1, f2)
    pm, pv = engine.posterior_masked(dev(xs))
    om, ov = Kr.posterior_masked(st, f1, f2, xs)
    figs = [("qv mean", rel(_np(mean), rm), tol_q), ("qv var", rel(_np(var), rv), tol_q),
            ("posterior mean", rel(_np(pm), om), tol_pm), ("posterior var", rel(_np(pv), ov), tol_pv),
            ("qv_cov", rel(_np(engine.qv_cov_masked()), Kr.q_v_cov_masked(st, f1, f2)), tol_q),
            # (vggp_posterior_cov_masked takes at most M points per call; M = 30 for the smaller pair)
            ("posterior_cov", rel(_np(engine.posterior_cov(dev(xs[:24]), masked=True)), Kr.posterior_cov_masked(st, f1, f2, xs[:24])), tol_pv)]
    if d1.kind == d2.kind == "matern12":
        ops = _operands(d1, d2, f1, f2, st.theta)
        for lit in (True, False):
            m_, v_ = engine.readout(*[torch.tensor(a) for a in ops], literal=lit, masked=True)
            qm, qv = Kr.readout_masked(st, *ops, literal=lit)
            assert tuple(m_.shape) == qm.shape == (7, 5)
            figs += [(f"readout literal={lit} mean", rel(_np(m_), qm), tol_q), (f"readout literal={lit} var", rel(_np(v_), qv), tol_pv)]
    _check(figs, what)


@pytest.mark.parametrize("name", list(PAIRS))
def test_masked_step_mixed(engine, name):
    """vggp_elbo_step_masked on a 40 x 36 grid with 30 % missing: ELBO, gradient, qv_masked, posterior_masked at the bounds of
    test_masked_step_vs_oracle (1e-7; posterior variance 1e-6), the dense covariances and readout_masked with them."""
    d1, d2 = PAIRS[name]
    n1, n2 = 40, 36
    _, y, x1, x2 = D.gen_grid(n1, n2)
    Wn = (np.random.default_rng(1).uniform(size=(n2, n1)) > 0.3).astype(np.float64)
    f1, f2 = MX.factor(d1, x1), MX.factor(d2, x2)
    st = Kr.elbo_step_masked(y.reshape(n2, n1), Wn, f1, f2, THETA_C)
    engine.plan(*MX.plan_args(d1, x1, d2, x2))
    W = dev(Wn)
    Ym = dev(y.reshape(n2, n1)) * W
    elbo, grad, info = engine.elbo_step_masked(Ym, W, float(Wn.sum()), engine.sumsq(Ym), THETA_C)
    assert info["status"] == 0
    _check([("elbo", abs(elbo - st.elbo) / abs(st.elbo), RTOL), ("grad", rel(grad, st.grad), RTOL)], f"masked {name}")
    xs = np.random.default_rng(9).uniform(0, 1, (3 * f1.m * f2.m + 5, 2))
    _dense_readouts(engine, st, d1, d2, f1, f2, xs, RTOL, RTOL, 1e-6, f"masked {name}")


@pytest.mark.parametrize("name", list(PAIRS))
def test_scattered_step_mixed(engine, name):
    """vggp_elbo_step_scattered on 1500 points: ELBO and gradient 1e-7, the read-outs 1e-6 (test_scattered_step_vs_oracle)."""
    d1, d2 = PAIRS[name]
    rng = np.random.default_rng(11)
    N = 1500
    X = rng.uniform(0, 1, (N, 2))
    y = np.sin(5 * X[:, 0]) * np.cos(3 * X[:, 1]) + 0.1 * rng.standard_normal(N)
    f1, f2 = MX.factor(d1, np.zeros(1)), MX.factor(d2, np.zeros(1))
    st = Kr.elbo_step_scattered(X, y, f1, f2, THETA_C)
    engine.plan(*MX.plan_args(d1, X[:, 0].copy(), d2, X[:, 1].copy()), scattered=True)
    elbo, grad, info = engine.elbo_step_scattered(dev(y), float(y @ y), THETA_C)
    assert info["status"] == 0
    _check([("elbo", abs(elbo - st.elbo) / abs(st.elbo), RTOL), ("grad", rel(grad, st.grad), RTOL)], f"scattered {name}")
    _dense_readouts(engine, st, d1, d2, f1, f2, rng.uniform(0, 1, (40, 2)), 1e-6, 1e-6, 1e-6, f"scattered {name}")


# ---- d: the iterative masked step and its read-outs on a non-square grid ----------------------------------------------------------------------
ITER = {"m12_b0_12-m32_pts10": (MX.b0(12), MX.pts("matern32", 10)), "m12_vff9-m12_pts12": (MX.vff(4), MX.pts("matern12", 12))}
N_ITER = (96, 80)
THETA_D = np.array([0.2, 0.3, 1.3, 0.7, 0.01])
XS_D = np.random.default_rng(9).uniform(0, 1, (70, 2))


@functools.lru_cache(maxsize=None)
def _mask(mname):
    n1, n2 = N_ITER
    return (np.random.default_rng(1).uniform(size=(n2, n1)) < 0.7).astype(np.float64) if mname == "bernoulli" else G.track_mask(n1, n2, 2, 0.5)


@functools.lru_cache(maxsize=None)
def _masked_oracle(name, mname):
    d1, d2 = ITER[name]
    _, y, x1, x2 = D.gen_grid(*N_ITER)
    f1, f2 = MX.factor(d1, x1), MX.factor(d2, x2)
    return f1, f2, y.reshape(N_ITER[1], N_ITER[0]), Kr.elbo_step_masked(y.reshape(N_ITER[1], N_ITER[0]), _mask(mname), f1, f2, THETA_D)


@pytest.mark.parametrize("mname", ["bernoulli", "track"])
@pytest.mark.parametrize("name", list(ITER))
def test_iterative_masked_step_and_readouts_mixed(engine, name, mname):
    """vggp_elbo_step_masked_iter on a 96 x 80 grid (the operator B1 (W^T o (B1^T V B2)) B2^T is where a transposition hides on square
    shapes), B0(12) x Matern-3/2 points(10) and VFF(9) x Matern-1/2 points(12) (an inverse-scaled and a direct basis side by side),
    Bernoulli and track masks, against the dense masked oracle: the bounds and the max(|ELBO|, N / 2) scaling of
    test_iterative_masked_step_vs_dense_small (2e-4 at this M, as explained there), status, 0 < rounds < 60, calls 2 and 3 bitwise
    equal; qv_masked_iter and posterior_masked_iter at the 1e-7 / 1e-6 of test_readouts_vs_dense_masked_oracle; for the Matern-1/2
    pair readout_masked_iter (literal and conditional, 7 x 5 cells) at the 1e-7 / 1e-6 of test_masked_vs_dense_gpu_path."""
    d1, d2 = ITER[name]
    f1, f2, Yn, ref = _masked_oracle(name, mname)
    Wn = _mask(mname)
    assert Wn.shape == (N_ITER[1], N_ITER[0])
    engine.plan(*MX.plan_args(d1, f1.x, d2, f2.x))
    W = dev(Wn)
    Ym = dev(Yn) * W
    nobs, yy = float(Wn.sum()), engine.sumsq(Ym)
    elbo, grad, info = engine.elbo_step_masked_iter(Ym, W, nobs, yy, THETA_D, n_probes=16)
    print(f"{name}/{mname}: iterations {info['rounds'][0]}")
    assert info["status"] == 0 and 0 < info["rounds"][0] < 60, info
    figs = [("elbo", abs(elbo - ref.elbo) / max(abs(ref.elbo), 0.5 * nobs), 2e-4), ("grad", rel(grad, ref.grad), 2e-4)]
    mean, var, qi = engine.qv_masked_iter(W, nobs)
    pm, pv, _ = engine.posterior_masked_iter(dev(XS_D), W, nobs)
    rm, rv = Kr.q_v_masked(ref, f1, f2)
    om, ov = Kr.posterior_masked(ref, f1, f2, XS_D)
    figs += [("qv mean", rel(_np(mean), rm), 1e-7), ("qv var", rel(_np(var), rv.reshape(-1)), 1e-6),
             ("posterior mean", rel(_np(pm), om), 1e-7), ("posterior var", rel(_np(pv), ov), 1e-6)]
    if d1.kind == d2.kind == "matern12":
        ops = _operands(d1, d2, f1, f2, THETA_D)
        for lit in (True, False):
            m_, v_, ri = engine.readout_masked_iter(*[dev(a) for a in ops], W, nobs, literal=lit)
            qm, qv = Kr.readout_masked(ref, *ops, literal=lit)
            assert tuple(m_.shape) == qm.shape == (7, 5) and ri["sweeps"][0] == (0 if lit else 1)
            figs += [(f"readout literal={lit} mean", rel(_np(m_), qm), 1e-7), (f"readout literal={lit} var", rel(_np(v_), qv.reshape(-1)), 1e-6)]
    _check(figs, f"iterative masked {name}/{mname}")
    e2, g2, _ = engine.elbo_step_masked_iter(Ym, W, nobs, yy, THETA_D, n_probes=16)
    e3, g3, _ = engine.elbo_step_masked_iter(Ym, W, nobs, yy, THETA_D, n_probes=16)
    assert e3 == e2 and np.array_equal(g3, g2)


# ---- e: the iterative scattered step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ITER))
def test_iterative_scattered_step_and_readouts_mixed(engine, name):
    """vggp_elbo_step_scattered_iter on 20 000 random points, M = 120 / 108 (N / M > 160): against its numpy specification at 1e-8 / 1e-6
    with the same iteration count, and against the dense scattered oracle at 1e-4 / 2e-4 (ELBO relative to max(|ELBO|, N / 2)), q(v) and
    posterior means 1e-7 -- the bounds of test_step_vs_spec_and_dense, whose rand20k case has N / M = 312; readout_scattered_iter
    (literal and conditional) at the 1e-7 / 1e-6 of test_scattered_vs_dense_gpu_path."""
    d1, d2 = ITER[name]
    X, y = S.rand20k()
    N = len(y)
    theta = S.THETA_A * np.array([1.0, 1.0, 1.3, 0.875, 1.0])          # s1 = 1.3, s2 = 0.7
    e = np.empty(0)
    f1, f2 = MX.factor(d1, e), MX.factor(d2, e)
    ref = Kr.elbo_step_scattered(X, y, f1, f2, theta)
    spec = S.elbo_step_scattered_iter(X, y, f1, f2, theta)
    engine.plan(*MX.plan_args(d1, X[:, 0].copy(), d2, X[:, 1].copy()), scattered=True)
    yd = dev(y)
    elbo, grad, info = engine.elbo_step_scattered_iter(yd, float(y @ y), theta)
    print(f"{name}: iterations {info['rounds'][0]} (spec {spec.iters})")
    assert info["status"] == 0 and info["rounds"][0] == spec.iters < 30
    s_elbo, s_grad = S.errors(elbo, grad, spec.elbo, spec.grad, N)
    d_elbo, d_grad = S.errors(elbo, grad, ref.elbo, ref.grad, N)
    figs = [("elbo vs spec", s_elbo, 1e-8), ("grad vs spec", s_grad, 1e-6), ("elbo vs dense", d_elbo, 1e-4), ("grad vs dense", d_grad, 2e-4)]
    qm = _np(engine.qv_scattered_iter())
    pm = _np(engine.posterior_scattered_iter(dev(XS_D)))
    figs += [("qv mean", rel(qm, Kr.q_v_masked(ref, f1, f2)[0]), 1e-7), ("posterior mean", rel(pm, Kr.posterior_masked(ref, f1, f2, XS_D)[0]), 1e-7)]
    ops = _operands(d1, d2, f1, f2, theta)
    for lit in (True, False):
        m_, v_, _ = engine.readout_scattered_iter(*[dev(a) for a in ops], literal=lit)
        rm, rv = Kr.readout_masked(ref, *ops, literal=lit)
        assert tuple(m_.shape) == rm.shape
        figs += [(f"readout literal={lit} mean", rel(_np(m_), rm), 1e-7), (f"readout literal={lit} var", rel(_np(v_), rv.reshape(-1)), 1e-6)]
    _check(figs, f"iterative scattered {name}")


# ---- f: warm trajectories -----------------------------------------------------------------------------------------------------------------------
def _path(th0):
    return lambda k: th0 * (1 + 0.01 * k)


# name -> dimension 1, dimension 2, (n1, n2), theta of step 0, steps before the read-outs
WARM = {
    "rbf48-m32_48": (MX.pts("rbf", 48), MX.pts("matern32", 48), (96, 96), np.array([0.2, 0.3, 1.3, 0.7, 0.02]), 8),
    "m12_160-rbf24": (MX.pts("matern12", 160), MX.pts("rbf", 24), (320, 96), np.array([0.25, 0.2, 1.3, 0.7, 0.02]), 8),
    "m12_vff33-m12_pts32": (MX.vff(16), MX.pts("matern12", 32), (96, 96), np.array([0.25, 0.3, 1.3, 0.7, 0.02]), 8),
}
WARM_CASES = [("rbf48-m32_48", "ab"), ("rbf48-m32_48", "ba"), ("m12_160-rbf24", "ab"), ("m12_160-rbf24", "ba"), ("m12_vff33-m12_pts32", "ab")]


@pytest.mark.parametrize("name,order", WARM_CASES)
def test_warm_trajectory_mixed(engine, name, order):
    """Eight warm steps with theta moving 1 % per step (sigma^2 = 0.02: a Matern dimension is present, see test_gpu_readout_states), every
    step against the oracle at the (1e-8, 1e-6) of that file with status 0; all read-outs of the cold test after the last step; two
    more steps from the basis the read-outs left behind.  The reverse order is the transposed twin.  rounds / sweeps / polished are
    printed per step.  Every warm step must take fewer rotation rounds than step 0 (the warm start is in use in both dimensions).

    What the diagnostics showed on an MI355X (rounds of dimension 1 / 2; the reverse order gives the same figures exchanged):
    rbf48-m32_48 (96 x 96; one dimension rank deficient, the other of full rank): step 0 the full Jacobi solve, 362 / 509 rounds.  Warm
        steps: the RBF dimension runs the extrapolated start followed by rotation rounds (131 - 197, never polished), the Matern-3/2
        dimension ends in the first-order polish (137 rounds at step 1, 47 from step 2 on).  No step without rotation rounds: neither
        the thin nor the subspace chain runs with only one RBF dimension.  Step 8, the first after the read-outs, repeats the figures
        of step 1 (197 / 137): the read-outs rebuilt the state and the warm start resumed one step back.
    m12_160-rbf24 (320 x 96; m1 > 128 >= m2, `big` through one dimension only): step 0 2010 / 189 rounds; every warm step 439 rounds
        in 4 sweeps for m = 160 (a fixed number of refinement sweeps) and 66 - 110 for the RBF dimension; nothing polished, no Newton
        chain (a Newton step has no rotation rounds).  The read-outs leave the warm start in place (step 8: 439 / 110).
    m12_vff33-m12_pts32 (96 x 96; an inverse-scaled and a direct basis side by side): step 0 171 / 246 rounds, both dimensions polished
        from step 1 on, no rotation round at all from step 3 to step 7; step 8 repeats step 1 (64 / 62) after the read-outs."""
    d1, d2, n, th0, steps = WARM[name]
    path = _path(th0)
    P = _grid(d1, d2, n, th0, order)
    perm = (lambda t: t) if order == "ab" else (lambda t: t[MX.SWAP])
    engine.plan(*MX.plan_args(P.d1, P.x1, P.d2, P.x2), warm_start=True)
    Y = dev(P.Y)
    yy = engine.sumsq(Y)
    figs, rounds = [], []
    for k in range(steps + 2):
        th = perm(path(k))
        elbo, grad, info = engine.elbo_step(Y, yy, th)
        assert info["status"] == 0, (k, info)
        st = Kr.elbo_step(P.Y, P.f1, P.f2, th)
        figs += [(f"step {k} elbo", abs(elbo - st.elbo) / abs(st.elbo), 1e-8), (f"step {k} grad", rel(grad, st.grad), 1e-6)]
        print(f"{name}/{order}: step {k}: rounds {info['rounds']}, sweeps {info['sweeps']}, polished {info['polished']}")
        rounds.append(sum(info["rounds"]))
        if k == steps - 1:
            figs += _full_readouts(engine, P, _full_reference(P, st, th), "after the last step: ")[0]
    print(f"{name}/{order}: rounds of the trajectory {rounds}")
    _check(figs, f"{name}/{order}")
    assert all(r < rounds[0] for r in rounds[1:]), rounds


@pytest.mark.parametrize("order", MX.ORDERS)
def test_cold_step_with_one_rbf_dimension_does_not_take_the_range_finder(engine, order):
    """RBF-points(96) x Matern-3/2 points(96) on 192 x 192, one cold step: the cold range finder + thin chain is for plans whose two
    dimensions are both RBF and must be refused here -- the rounds bound by which test_cold_rbf_steps_take_the_range_finder recognises
    it (fewer than 400) must NOT hold; value and gradient at (1e-8, 1e-6), q(v) and posterior at the bounds of test_gpu_readout_states.
    Measured on an MI355X: 714 rounds for the RBF dimension, 1225 for the Matern-3/2 one -- the full Jacobi solve in both."""
    P = _grid(MX.pts("rbf", 96), MX.pts("matern32", 96), (192, 192), np.array([0.2, 0.3, 1.3, 0.7, 0.02]), order)
    st = Kr.elbo_step(P.Y, P.f1, P.f2, P.theta)
    elbo, grad, info = _cold_step(engine, P)
    print(f"rbf96-m32_96/{order}: rounds {info['rounds']}, sweeps {info['sweeps']}, polished {info['polished']}")
    assert info["status"] == 0
    mean, var = engine.qv()
    pm, pv = engine.posterior(dev(P.xs))
    rm, rv = Kr.q_v(st)
    om, ov = Kr.posterior(st, P.f1, P.f2, P.xs)
    _check([("elbo", abs(elbo - st.elbo) / abs(st.elbo), 1e-8), ("grad", rel(grad, st.grad), 1e-6),
            ("qv mean", rel(_np(mean), rm), TOL_QV), ("qv var", rel(_np(var), rv), TOL_QV),
            ("posterior mean", rel(_np(pm), om), TOL_PM), ("posterior var", rel(_np(pv), ov), TOL_PV)], f"rbf96-m32_96/{order}")
    assert sum(info["rounds"]) >= 400, info
