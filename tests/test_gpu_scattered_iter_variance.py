"""Point-wise variances of q(v) and posterior(x*) after the iterative scattered step on the GPU: vggp_qv_var_scattered_iter /
vggp_posterior_var_scattered_iter (block PCG on rank-one right-hand sides with the Khatri-Rao operator) against the dense scattered
step on the same context, the dense CPU oracle, the Kronecker path beyond the dense limit, and through the model classes
(scattered_variances=True); the two-column field kernel (vggp_kr_field2) bit for bit against the four-column one.  Tolerances are the
iterative masked read-outs': means 1e-7, variances 1e-6 of the largest entry -- conditions a PCG tolerance of 1e-10 has to meet.

Measured on one MI355X: vggp_kr_field2 bitwise equal to vggp_kr_field on all five shapes, 0.000 .. 0.019 of the forward bound.  Against
the dense GPU step: q(v) mean 1.7e-11 .. 4.8e-10 (B1: 2.0e-8), q(v) variance 7.8e-14 .. 2.7e-12, posterior mean 1.3e-11 .. 3.5e-10,
posterior variance 1.8e-15 .. 1.7e-13, 7 .. 10 iterations; rand20k against the CPU oracle 5.3e-11 / 9.2e-15 / 7.1e-11 / 5.0e-15.  block = 16
against block = 64 and listed cells against all cells: the same bits.  The 160 x 160 grid as points (M = 17408) against the Kronecker
path: 7.9e-13 / 5.7e-13 / 8.1e-13 / 3.6e-12, 1 iteration.  Models: posterior mean 1.2e-10, variance 1.8e-14, predictive variance 9.1e-16;
NLPD of the held-out tenth 0.756428166 on both solvers; q(u) variance of the Gridded* classes 5.1e-16 .. 2.4e-15 (9 .. 11 iterations).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import dense as D
from oracle import kron as Kr
from variational_gridded_gaussian_processes_amd import _lib, utils
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


def code_of(fn, *a, **kw):
    with pytest.raises(VggpError) as e:
        fn(*a, **kw)
    return e.value.code


# ---- the two-column field kernel --------------------------------------------------------------------------------------------------------
KR_SHAPES = [(5, 7, 37, 3), (16, 16, 64, 1), (17, 33, 1000, 7), (136, 128, 4099, 17), (256, 256, 515, 64)]


@pytest.mark.parametrize("m1,m2,N,nb", KR_SHAPES, ids=lambda v: str(v))
def test_kr_field2_equals_kr_field(engine, m1, m2, N, nb):
    """Odd nb with a ragged column group, N no multiple of 64, several row tiles, m_d no multiple of 16.  A column's accumulators, k
    order, epilogue and butterfly do not depend on the columns per workgroup: the same bits."""
    rng = np.random.default_rng(m1 * 1000 + N)
    L, R, V = rng.standard_normal((m1, N)), rng.standard_normal((m2, N)), rng.standard_normal((m1, nb, m2))
    Ld, Rd, Vd = dev(L), dev(R), dev(V)
    two, four = engine.kr_field(Ld, Rd, Vd, cols_per_wg=2), engine.kr_field(Ld, Rd, Vd)
    assert tuple(two.shape) == (nb, N)
    assert torch.equal(two, four)
    ref = np.einsum("ak,cak->ck", L, np.einsum("acb,bk->cak", V, R, optimize=True), optimize=True)
    bound = np.einsum("ak,cak->ck", np.abs(L), np.einsum("acb,bk->cak", np.abs(V), np.abs(R), optimize=True), optimize=True)
    worst = float((np.abs(two.cpu().numpy() - ref) / (m1 * m2 * U * bound)).max())
    print(f"({m1}, {m2}, {N}, {nb}): field2 {worst:.3f} of the forward bound K 2^-52 |.|")
    assert worst <= 1.0


def test_kr_field2_rejects_65_columns(engine):
    ones = dev(np.ones((3, 4)))
    assert code_of(engine.kr_field, ones, ones, dev(np.ones((3, 65, 3))), cols_per_wg=2) == _lib.VGGP_EINVAL


# ---- against the dense GPU step on the same context ---------------------------------------------------------------------------------------
CASES = {
    "trk400_m12_a": ("trk400", "b0", "matern12", 12, S.THETA_A),
    "trk400_m12_b": ("trk400", "b0", "matern12", 12, S.THETA_B),
    "trk400_m16_b": ("trk400", "b0", "matern12", 16, S.THETA_B),
    "rand20k_m8_a": ("rand20k", "b0", "matern12", 8, S.THETA_A),
    "trk400_points_matern32_m16_b": ("trk400", "points", "matern32", 16, S.THETA_B),
    "trk400_b1_m12_b": ("trk400", "b1", "matern12", 12, S.THETA_B),          # the e_d = -1 scaling of q(v)
}
XS = np.random.default_rng(9).uniform(0, 1, (70, 2))


@functools.lru_cache(maxsize=None)
def data(name):
    return {"trk400": lambda: S.trk(400, 0.5), "rand20k": S.rand20k}[name]()


def grid_of(basis, m):
    return np.linspace(0.0, 1.0, m + 1) if basis == "b0" else np.linspace(0.0, 1.0, m)


def plan_case(engine, case):
    dname, basis, kind, m, theta = CASES[case]
    X, y = data(dname)
    g = grid_of(basis, m)
    engine.plan(kind, basis, g, X[:, 0], kind, basis, g, X[:, 1], scattered=True)
    return dev(y), float(y @ y), theta


@functools.lru_cache(maxsize=None)
def oracle_rand20k():
    X, y = data("rand20k")
    f1, f2 = S.b0_factors(8)
    ref = Kr.elbo_step_scattered(X, y, f1, f2, S.THETA_A)
    return Kr.q_v_masked(ref, f1, f2), Kr.posterior_masked(ref, f1, f2, XS)


@pytest.mark.parametrize("case", list(CASES))
def test_variances_vs_dense_step(engine, case):
    yd, yy, theta = plan_case(engine, case)
    assert engine.m1 == CASES[case][3]
    xs = dev(XS)
    engine.elbo_step_scattered(yd, yy, theta)
    dm, dv = engine.qv_masked()
    dpm, dpv = engine.posterior_masked(xs)
    engine.elbo_step_scattered_iter(yd, yy, theta)
    mean, var, info = engine.qv_var_scattered_iter()
    pm, pv, pinfo = engine.posterior_var_scattered_iter(xs)
    errs = (rel(mean.cpu(), dm.cpu()), rel(var.cpu(), dv.cpu().reshape(-1)), rel(pm.cpu(), dpm.cpu()), rel(pv.cpu(), dpv.cpu()))
    print(f"{case}: q(v) mean {errs[0]:.1e} var {errs[1]:.1e}; posterior mean {errs[2]:.1e} var {errs[3]:.1e}; "
          f"iterations {info['rounds'][0]} / {pinfo['rounds'][0]}, solves {info['sweeps'][0]} / {pinfo['sweeps'][0]}")
    assert errs[0] <= 1e-7 and errs[2] <= 1e-7
    assert errs[1] <= 1e-6 and errs[3] <= 1e-6
    assert info["sweeps"][0] == -(-mean.numel() // 64) and pinfo["sweeps"][0] == 2
    assert 0 < info["rounds"][0] < 30 and 0 < pinfo["rounds"][0] < 30
    assert torch.equal(mean, engine.qv_scattered_iter())          # the mean read-out's two GEMMs
    if case == "rand20k_m8_a":          # ... and against the CPU oracle
        (rm, rv), (om, ov) = oracle_rand20k()
        oerr = (rel(mean.cpu(), rm), rel(var.cpu(), rv.reshape(-1)), rel(pm.cpu(), om), rel(pv.cpu(), ov))
        print(f"{case}: against the CPU oracle: q(v) mean {oerr[0]:.1e} var {oerr[1]:.1e}; posterior mean {oerr[2]:.1e} var {oerr[3]:.1e}")
        assert oerr[0] <= 1e-7 and oerr[2] <= 1e-7
        assert oerr[1] <= 1e-6 and oerr[3] <= 1e-6


def test_chunking_and_cell_subsets(engine):
    """block = 16 on 37 columns is three block solves with a ragged last one.  The results are BITWISE equal to those of block = 64
    (one solve), and a list of cells gives the same bits as the same entries of the all-cell call: a column's numbers do not depend on
    its neighbours in the block or on the block's width."""
    yd, yy, theta = plan_case(engine, "trk400_m12_b")
    engine.elbo_step_scattered_iter(yd, yy, theta)
    xs = dev(XS[:37])
    cells = np.random.default_rng(4).choice(144, size=37, replace=False)
    m16, v16, i16 = engine.posterior_var_scattered_iter(xs, block=16)
    m64, v64, i64 = engine.posterior_var_scattered_iter(xs, block=64)
    assert (i16["sweeps"][0], i64["sweeps"][0]) == (3, 1)
    print("posterior block 16 vs 64:", rel(m16.cpu(), m64.cpu()), rel(v16.cpu(), v64.cpu()))
    assert torch.equal(m16, m64) and torch.equal(v16, v64)
    qm16, q16, j16 = engine.qv_var_scattered_iter(cells=cells, block=16)
    qm64, q64, j64 = engine.qv_var_scattered_iter(cells=cells, block=64)
    qm, qall, _ = engine.qv_var_scattered_iter()
    assert (j16["sweeps"][0], j64["sweeps"][0]) == (3, 1)
    print("q(v) block 16 vs 64:", rel(q16.cpu(), q64.cpu()), "subset vs all:", rel(q16.cpu(), qall.cpu()[cells]))
    assert torch.equal(qm16, qm) and torch.equal(qm64, qm)
    assert torch.equal(q16, q64)
    assert torch.equal(q16.cpu(), qall.cpu()[cells])
    mean_only, none, info = engine.qv_var_scattered_iter(variance=False)
    assert none is None and torch.equal(mean_only, engine.qv_scattered_iter()) and info["sweeps"][0] == 0


def test_beyond_dense_limit(engine):
    """The 160 x 160 grid as 25 600 points, M = 136 * 128 = 17408 > 16384: the preconditioner is exact there, and the variances equal
    the Kronecker path's."""
    n, m1, m2 = 160, 136, 128
    theta = S.THETA_A
    X, y, x1, x2 = D.gen_grid(n, n)
    g1, g2 = np.linspace(0, 1, m1 + 1), np.linspace(0, 1, m2 + 1)
    rng = np.random.default_rng(12)
    cells = rng.choice(m1 * m2, size=100, replace=False)
    xs = dev(rng.uniform(0, 1, (70, 2)))
    engine.plan("matern12", "b0", g1, x1, "matern12", "b0", g2, x2)
    Y = dev(y.reshape(n, n))
    engine.elbo_step(Y, engine.sumsq(Y), theta)
    km, kv = engine.qv()
    kpm, kpv = engine.posterior(xs)
    engine.plan("matern12", "b0", g1, X[:, 0], "matern12", "b0", g2, X[:, 1], scattered=True)
    engine.elbo_step_scattered_iter(dev(y), float(y @ y), theta)
    im, iv, info = engine.qv_var_scattered_iter(cells=cells)
    ipm, ipv, pinfo = engine.posterior_var_scattered_iter(xs)
    errs = (rel(im.cpu(), km.cpu()), rel(iv.cpu(), kv.cpu().reshape(-1)[cells]), rel(ipm.cpu(), kpm.cpu()), rel(ipv.cpu(), kpv.cpu()))
    print(f"full grid as points, M = {m1 * m2}:", errs, info["rounds"], pinfo["rounds"], info["sweeps"], pinfo["sweeps"])
    assert errs[0] <= 1e-7 and errs[2] <= 1e-7
    assert errs[1] <= 1e-6 and errs[3] <= 1e-6
    assert info["rounds"][0] <= 3 and pinfo["rounds"][0] <= 3
    assert info["sweeps"][0] == 2 and pinfo["sweeps"][0] == 2


def test_state_and_errors(engine):
    from variational_gridded_gaussian_processes_amd import Engine
    X, y = data("rand20k")
    X, y = X[:500], y[:500]
    g = np.linspace(0, 1, 9)
    yd, yy, xs = dev(y), float(y @ y), dev(XS[:5])

    def both(e):
        return [code_of(e.qv_var_scattered_iter), code_of(e.qv_var_scattered_iter, cells=[3]), code_of(e.posterior_var_scattered_iter, xs)]

    fresh = Engine(0)
    try:
        fresh.plan("matern12", "b0", g, X[:, 0], "matern12", "b0", g, X[:, 1], scattered=True)          # before any step
        assert both(fresh) == [_lib.VGGP_ESTATE] * 3
        x1 = np.linspace(0, 1, 25)
        fresh.plan("matern12", "b0", g, x1, "matern12", "b0", g, x1[:20])                                # planned for a grid
        assert both(fresh) == [_lib.VGGP_EINVAL] * 3
    finally:
        fresh.close()
    multi = Engine(0, n_ranks=2, rank=0, allreduce=lambda buf: None)                                     # multi-rank context
    try:
        multi.plan("matern12", "b0", g, X[:, 0], "matern12", "b0", g, X[:, 1], scattered=True, n_total=1000)
        assert both(multi) == [_lib.VGGP_EINVAL] * 3
    finally:
        multi.close()
    engine.plan("matern12", "b0", g, X[:, 0], "matern12", "b0", g, X[:, 1], scattered=True)
    engine.elbo_step_scattered_iter(yd, yy, S.THETA_A)
    engine.elbo_step_scattered(yd, yy, S.THETA_A)                                                        # after the dense scattered step
    assert both(engine) == [_lib.VGGP_ESTATE] * 3
    engine.elbo_step_scattered_iter(yd, yy, S.THETA_A)
    engine.plan("matern12", "b0", g, X[:, 0], "matern12", "b0", g, X[:, 1], scattered=True)              # after plan
    assert both(engine) == [_lib.VGGP_ESTATE] * 3
    engine.elbo_step_scattered_iter(yd, yy, S.THETA_A)
    for bad in ([-1], [64], [3, 10 ** 12]):
        assert code_of(engine.qv_var_scattered_iter, cells=bad) == _lib.VGGP_EINVAL
    assert code_of(engine.qv_var_scattered_iter, cells=[3], block=65) == _lib.VGGP_EINVAL
    assert code_of(engine.posterior_var_scattered_iter, xs, block=65) == _lib.VGGP_EINVAL
    _, v, info = engine.qv_var_scattered_iter(cells=[3, 63])                                             # (the refused calls left the state readable)
    assert bool(torch.isfinite(v).all()) and bool((v > 0).all()) and info["sweeps"][0] == 1


def test_readouts_leave_the_next_step_unchanged(engine):
    """The read-outs work in a workspace of their own: the step after them reuses the kept preconditioner basis and returns the same
    bits as without them."""
    theta2 = [t * 1.01 for t in S.THETA_B]
    yd, yy, theta = plan_case(engine, "trk400_m12_b")
    engine.elbo_step_scattered_iter(yd, yy, theta)
    e_a, g_a, i_a = engine.elbo_step_scattered_iter(yd, yy, theta2)
    yd, yy, theta = plan_case(engine, "trk400_m12_b")
    engine.elbo_step_scattered_iter(yd, yy, theta)
    engine.qv_var_scattered_iter()
    engine.posterior_var_scattered_iter(dev(XS), block=16)
    e_b, g_b, i_b = engine.elbo_step_scattered_iter(yd, yy, theta2)
    assert e_b == e_a and np.array_equal(g_b, g_a) and i_b["rounds"] == i_a["rounds"]


# ---- models -----------------------------------------------------------------------------------------------------------------------------
def test_models_scattered_variances(engine):
    from variational_gridded_gaussian_processes_amd.models import Matern12GriddedGP
    X, y = data("trk400")
    held = np.arange(len(y)) % 10 == 0
    Xt, yt = torch.tensor(X[~held]), torch.tensor(y[~held])
    xh, yh = torch.tensor(X[held]), torch.tensor(y[held])
    xs = torch.tensor(XS)
    cells = [0, 100, 255]

    def make(**kw):
        return Matern12GriddedGP(Xt, yt, 17, (0, 1), (0, 1), engine=engine, **kw).to(torch.float64)
    de = make(scattered_solver="dense")
    off = make(scattered_solver="iterative")
    on = make(scattered_solver="iterative", scattered_variances=True)
    qd, ad, pd, ppd, phd = de.q_v(), de.q_v_at(cells), de.posterior(xs), de.posterior_predictive(xs), de.posterior_predictive(xh)
    assert not de._siter
    # the default: means only, but q_v_at is an explicit request
    assert off.scattered_variances is False
    for dist in (off.q_v(), off.posterior(xs)):
        with pytest.raises(NotImplementedError, match="follow-up"):
            dist.variance
    ao = off.q_v_at(cells)
    assert off._siter and off.last_readout_info["sweeps"][0] == 1
    assert rel(ao.mean, ad.mean) <= 1e-6 and rel(ao.variance, ad.variance) <= 1e-6
    # the switch
    qi = on.q_v()
    assert on._siter and on.scattered_variances is True and callable(qi._variance)          # lazy: no block solve has run yet
    assert rel(qi.mean, qd.mean) <= 1e-6
    assert rel(qi.variance, qd.variance) <= 1e-6 and not callable(qi._variance)
    assert on.last_readout_info["sweeps"][0] == 4 and 0 < on.last_readout_info["rounds"][0] < 30
    lo, hi = qi.confidence_region()
    assert bool((hi >= lo).all())
    ai = on.q_v_at(cells)
    assert rel(ai.mean, ad.mean) <= 1e-6 and rel(ai.variance, ad.variance) <= 1e-6
    pi, ppi = on.posterior(xs), on.posterior_predictive(xs)
    assert on.last_readout_info["sweeps"][0] == 2
    errs = (rel(pi.mean, pd.mean), rel(pi.variance, pd.variance), rel(ppi.variance, ppd.variance))
    print("models: posterior mean, variance, predictive variance:", errs)
    assert max(errs) <= 1e-6
    for dist in (qi, pi, ppi):
        with pytest.raises(NotImplementedError):
            dist.covariance_matrix
    phi = on.posterior_predictive(xh)
    col = lambda t: t.reshape(-1, 1)          # (utils.nlpd keeps the reference's contract: 2-D tensors of one shape)
    n_i = utils.nlpd(col(yh), col(phi.mean), col(phi.variance)).item()
    n_d = utils.nlpd(col(yh), col(phd.mean), col(phd.variance)).item()
    print(f"models: NLPD of the held-out tenth: iterative {n_i:.9f} dense {n_d:.9f}")
    assert abs(n_i - n_d) <= 1e-6 * abs(n_d)


def small_scattered():
    """The small data of tests/test_gpu_gridded_iter_readout.py: a 24 x 20 grid with 30 % missing, jittered off the grid."""
    X, y, _, _ = D.gen_grid(24, 20)
    rng = np.random.default_rng(5)
    keep = rng.random(len(y)) > 0.3
    X, y = X[keep], y[keep]
    X = np.clip(X + rng.normal(scale=4e-3, size=X.shape), 0.0, 1.0)
    return torch.tensor(X), torch.tensor(y)


def make_gridded(cls, X, y, engine, **kw):
    import variational_gridded_gaussian_processes_amd.models as M
    ns, lims = 7, (-0.1, 1.1)
    if cls == "vff":
        return M.GriddedMatern12VFFGP(X, y, 5, lims, lims, ns, (0, 1), (0, 1), engine=engine, **kw).to(torch.float64)
    if cls == "svgp":
        z1, z2 = torch.linspace(0, 1, 6, dtype=torch.float64), torch.linspace(0, 1, 5, dtype=torch.float64)
        Z = torch.cartesian_prod(z1, z2)[torch.randperm(30, generator=torch.Generator().manual_seed(3))]          # rows in any order
        return M.GriddedMatern12SVGP(X, y, Z, ns, (0, 1), (0, 1), engine=engine, **kw).to(torch.float64)
    return M.GriddedMatern12ASVGP(X, y, ns, 2, (0, 1), (0, 1), engine=engine, **kw).to(torch.float64)


@pytest.mark.parametrize("cls", ["vff", "svgp", "asvgp"])
def test_gridded_models_q_u_variance(engine, cls):
    X, y = small_scattered()
    it = make_gridded(cls, X, y, engine, scattered_solver="iterative", scattered_variances=True)
    de = make_gridded(cls, X, y, engine, scattered_solver="dense")
    qi, qd = it.q_u(), de.q_u()
    assert it._siter and not de._siter and callable(qi._variance)
    e_m, e_v = rel(qi.mean, qd.mean), rel(qi.variance, qd.variance)
    print(f"{cls}: q(u) mean {e_m:.1e} variance {e_v:.1e}, iterations {it.last_readout_info['rounds'][0]}")
    assert e_m <= 1e-6 and e_v <= 1e-6
    with pytest.raises(NotImplementedError):
        qi.covariance_matrix


def test_model_auto_beyond_the_dense_limit(engine):
    """scattered_solver='auto' at M = 136 * 128 = 17408 takes the iterative scattered step; with scattered_variances=True the
    variances are there: finite, positive, and for the posterior at most the prior's s1 s2."""
    import variational_gridded_gaussian_processes_amd.models as M
    X, y, _, _ = D.gen_grid(160, 160)
    X = np.clip(X + np.random.default_rng(6).normal(scale=5e-4, size=X.shape), 0.0, 1.0)      # off the grid: scattered points
    Z = torch.cartesian_prod(torch.linspace(0, 1, 136, dtype=torch.float64), torch.linspace(0, 1, 128, dtype=torch.float64))
    m = M.GriddedMatern12SVGP(torch.tensor(X), torch.tensor(y), Z, 7, (0, 1), (0, 1), engine=engine,
                              scattered_variances=True).to(torch.float64)
    at = m.q_v_at([0, 5000, 16640])
    assert m._scattered and m._siter and m.last_readout_info["sweeps"][0] == 1
    assert bool(torch.isfinite(at.variance).all()) and bool((at.variance > 0).all())
    pv = m.posterior(torch.tensor(XS)).variance
    ss = (m.kernel_1.outputscale * m.kernel_2.outputscale).item()
    print(f"M = 17408: q(v) variances {at.variance.tolist()}, posterior variance in [{pv.min().item():.3e}, {pv.max().item():.3e}], s1 s2 {ss:.3f}")
    assert bool(torch.isfinite(pv).all()) and bool((pv > 0).all()) and bool((pv <= ss).all())
