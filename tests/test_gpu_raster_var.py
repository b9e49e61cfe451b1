"""vggp_kron_quadform / vggp_posterior_raster_var_masked / posterior_grid(raster_variance=True): the variance of posterior(x*) on a
raster after the dense masked and scattered steps, from the separable contraction against the state's dense Sinv (csrc/raster_var.hip).

1. The building block on integer operands (tests/raster_var_cases.py): every fp64 sum is exact in any order, so the result must equal
   numpy's int64 einsum BIT FOR BIT -- at every tile, k and chunk edge, with and without the epilogue, into NaN-poisoned output and
   scratch, twice.
2. The entry on the small read-out states of tests/masked_dense_cases.py (m = (7, 5): E_scattered, B_bernoulli) against
   oracle/dense.py's posterior variance under the project's ceiling for post_var on that state kind (1e-6), and against
   vggp_posterior_masked at the same points under the same ceiling (the two routes sum one form in different orders); the mean bit-equal
   to vggp_posterior_raster's.  Each figure is printed before it is asserted (`pytest -s`): "RASTER_VAR case raster quantity error bound".
3. Neutrality and state rules.
4. Model level: posterior_grid(..., raster_variance=True).

Measured on the MI355X, worst over the two states and two rasters: against the oracle 5.9e-15 (E_scattered,
70 x 3; the point-wise entry there: 6.2e-15), against vggp_posterior_masked 1.6e-15; model level 3.5e-15.  Bound 1e-6.
"""
import functools

import numpy as np
import pytest
import torch

import masked_dense_cases as P
import mixed_dims_cases as MX
import raster_var_cases as RV
import test_gpu_posterior_raster as PR
from oracle import dense as D
from variational_gridded_gaussian_processes_amd import VggpError
from variational_gridded_gaussian_processes_amd._lib import VGGP_EINVAL, VGGP_ESTATE

pytestmark = pytest.mark.gpu
dev, rel, code_of = PR.dev, PR.rel, PR.code_of
NAN = float("nan")


# ---- 1. the building block ---------------------------------------------------------------------------------------------------------
def _ops(shape):
    (S, U1, U2, n1, n2), ref = RV.case(*shape)
    return [dev(a) for a in (S, U1, U2, n1, n2)], (S, U1, U2, n1, n2), ref


def _same_value_bits(got, want_int):
    """Bit for bit against the int64 reference (an exact zero sum is +0.0 on both sides: accumulators start at +0.0, round to nearest)."""
    want = np.asarray(want_int, dtype=np.float64)
    assert np.array_equal(np.asarray(want_int), want.astype(np.int64))            # (the reference itself is exact in fp64)
    return np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("shape", RV.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_quadform_is_bitwise_numpy_int64_einsum(engine, shape):
    (S, U1, U2, n1, n2), (hS, hU1, hU2, hn1, hn2), ref = _ops(shape)
    P1, P2 = hU1.shape[1], hU2.shape[1]
    # poison: a first call on a NaN matrix leaves NaN in every word of the scratch this shape uses and in `out`
    out = torch.full((P1, P2), NAN, dtype=torch.float64, device=engine.device)
    engine.kron_quadform(torch.full_like(S, NAN), U1, U2, out=out)
    assert bool(torch.isnan(out).all())
    engine.kron_quadform(S, U1, U2, out=out)                          # the bare form: everything written, nothing stale read
    assert bool(torch.isfinite(out).all())
    assert _same_value_bits(out, ref), np.abs(out.cpu().numpy() - ref).max()
    again = engine.kron_quadform(S, U1, U2)
    assert torch.equal(again, out) and np.array_equal(again.cpu().numpy().view(np.int64), out.cpu().numpy().view(np.int64))
    # the epilogue, integer-valued as well: 2 (3 - n1[a] n2[b] + quad)
    epi = engine.kron_quadform(S, U1, U2, n1, n2, kd=3.0, scale=2.0)
    assert _same_value_bits(epi, 2 * (3 - hn1[:, None] * hn2[None, :] + ref))
    # a quadratic form does not see the antisymmetric part of S: the transposed matrix, read through the transposed view, gives the same
    # integers -- and the operands are not symmetric (tests/test_raster_var_cases.py), so no triangle is assumed
    assert _same_value_bits(engine.kron_quadform(S.t().contiguous(), U1, U2), ref)


@pytest.mark.parametrize("P1", RV.chunk_edge_P1(RV.CHUNK_EDGE_M[0]))
def test_quadform_across_the_chunk_edges(engine, P1):
    m1, m2 = RV.CHUNK_EDGE_M
    (S, U1, U2, n1, n2), host, ref = _ops((m1, m2, P1, RV.CHUNK_EDGE_P2))
    out = torch.full((P1, RV.CHUNK_EDGE_P2), NAN, dtype=torch.float64, device=engine.device)
    engine.kron_quadform(S, U1, U2, n1, n2, kd=1.0, scale=1.0, out=out)
    assert _same_value_bits(out, 1 - host[3][:, None] * host[4][None, :] + ref)
    # a column's numbers do not depend on the chunk it falls into: the first columns alone give the same bits
    if P1 > 1:
        head = engine.kron_quadform(S, U1[:, :1].contiguous(), U2, n1[:1].contiguous(), n2, kd=1.0, scale=1.0)
        assert torch.equal(head[0], out[0])


def test_quadform_refuses_bad_arguments(engine):
    (S, U1, U2, n1, n2), _, _ = _ops((5, 7, 6, 9))
    lib, h, st = engine.lib, engine._h, torch.cuda.current_stream(engine.device).cuda_stream
    out = torch.empty(6, 9, dtype=torch.float64, device=engine.device)
    a = [S.data_ptr(), 5, 7, U1.data_ptr(), 6, U2.data_ptr(), 9, None, None, 0.0, 1.0, out.data_ptr(), st]
    assert lib.vggp_kron_quadform(h, *a) == 0
    for k, v in ((0, None), (3, None), (5, None), (11, None), (7, n1.data_ptr()), (4, 0), (6, 0), (1, 0), (2, 1 << 15)):
        b = list(a)
        b[k] = v
        assert lib.vggp_kron_quadform(h, *b) == VGGP_EINVAL, k


# ---- 2. the entry against the point-wise entry and the oracle ------------------------------------------------------------------------
_rng = np.random.default_rng(23)
RASTERS = {"37x21": (PR.G1, PR.G2),                                     # non-square, no multiples of 64, P1 < m1^2 = 49
           "70x3": (_rng.uniform(0.0, 1.0, 70), _rng.uniform(0.0, 1.0, 3))}          # P1 > m1^2: two chunks, and more than one tile


def _pts(g1, g2):
    return np.stack([np.repeat(g1, len(g2)), np.tile(g2, len(g1))], axis=1)       # point a * P2 + b = (g1[a], g2[b])


@functools.lru_cache(maxsize=None)
def oracle_variance(name, raster):
    """oracle/dense.py's posterior variance of the case at the raster's points (once, shared, read-only)."""
    p = P.case_problem(name)
    theta = np.asarray(p["theta"], float)
    if p["layout"] == "masked":
        X1, X2 = np.meshgrid(p["x1"], p["x2"])
        X, y, m = np.vstack([X1.ravel(), X2.ravel()]).T, p["Y"].reshape(-1), p["W"].reshape(-1) > 0
    else:
        X, y, m = p["X"], p["y"], None
    dm = MX.dense(X, y, p["d1"], p["d2"], theta, mask=m)
    with torch.no_grad():
        return dm.posterior(_pts(*RASTERS[raster])).variance.numpy()


def _step(engine, name):
    """Plan and step a case of tests/masked_dense_cases.py -> a function that repeats the step (optionally at another theta)."""
    p = P.case_problem(name)
    if p["layout"] == "masked":
        engine.plan(*MX.plan_args(p["d1"], p["x1"], p["d2"], p["x2"]))
        W, Ym = dev(p["W"]), dev(p["Y"] * p["W"])
        step = lambda th=p["theta"]: engine.elbo_step_masked(Ym, W, float(p["N"]), p["yy"], th)
    else:
        engine.plan(*MX.plan_args(p["d1"], p["X"][:, 0].copy(), p["d2"], p["X"][:, 1].copy()), scattered=True)
        y = dev(p["y"])
        step = lambda th=p["theta"]: engine.elbo_step_scattered(y, p["yy"], th)
    assert step()[2]["status"] == 0
    return step


def _ceiling(name):
    return (P.CEIL_MASKED if P.CASES[name]["layout"] == "masked" else P.CEIL_SCATTERED)["post_var"]


@pytest.mark.parametrize("raster", list(RASTERS))
@pytest.mark.parametrize("name", [P.E_SCATTERED, P.E_MASKED])
def test_raster_variance_vs_pointwise_entry_and_oracle(engine, name, raster):
    g1, g2 = RASTERS[raster]
    assert P.M_E == 35 and (len(g1) > 49) == (raster == "70x3")          # m = (7, 5): chunk = 49
    _step(engine, name)
    bound = _ceiling(name)
    mean, var = engine.posterior_raster_var_masked(dev(g1), dev(g2))
    assert tuple(mean.shape) == (len(g1), len(g2)) and tuple(var.shape) == (len(g1), len(g2))
    m0, none = engine.posterior_raster(dev(g1), dev(g2), want_var=False)
    assert none is None and torch.equal(mean, m0)                      # the same launches: the same bits
    pm, pv = engine.posterior_masked(dev(_pts(g1, g2)))
    ov = oracle_variance(name, raster)
    e_o, e_p, e_po = rel(PR._np(var), ov), rel(PR._np(var), PR._np(pv)), rel(PR._np(pv), ov)
    print(f"RASTER_VAR {name} {raster} var_vs_oracle {e_o:.3e} {bound:.0e}")
    print(f"RASTER_VAR {name} {raster} var_vs_pointwise {e_p:.3e} {bound:.0e}   (point-wise entry vs oracle {e_po:.3e})")
    assert e_o < bound and e_p < bound
    assert float(var.min()) > 0.0
    # flat ordering a * P2 + b at single points, and the transposed reading is wrong
    scale = float(pv.abs().max())
    for a, b in ((0, 0), (len(g1) - 1, 1), (3, len(g2) - 1), (17, 2)):
        one = engine.posterior_masked(dev(np.array([[g1[a], g2[b]]])))[1]
        assert abs(var[a, b].item() - one.item()) <= bound * scale, (a, b)
    assert rel(var.cpu().numpy(), pv.cpu().numpy().reshape(len(g2), len(g1)).T) > 1e-3
    again = engine.posterior_raster_var_masked(dev(g1), dev(g2))
    assert torch.equal(again[0], mean) and torch.equal(again[1], var)          # bitwise repeatable


# ---- 3. neutrality and state rules ---------------------------------------------------------------------------------------------------
G1, G2, PTS = PR.G1, PR.G2, PR.PTS


def _var_call(engine, g1=None, g2=None):
    return engine.posterior_raster_var_masked(dev(G1) if g1 is None else g1, dev(G2) if g2 is None else g2)


@pytest.mark.parametrize("name", [P.E_SCATTERED, P.E_MASKED])
def test_pointwise_readout_has_the_same_bits_before_and_after(engine, name):
    _step(engine, name)
    before = engine.posterior_masked(dev(PTS))
    qv_before = engine.qv_masked()
    _var_call(engine)
    after = engine.posterior_masked(dev(PTS))
    qv_after = engine.qv_masked()
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    assert all(torch.equal(a, b) for a, b in zip(qv_after, qv_before))


@pytest.mark.parametrize("name", [P.E_SCATTERED, P.E_MASKED])
def test_a_raster_variance_call_between_two_steps_changes_no_bit_of_the_second(engine, name):
    def run(with_call):
        step = _step(engine, name)
        if with_call:
            _var_call(engine)
        elbo, grad, info = step(np.asarray(P.case_problem(name)["theta"]) * 1.01)
        assert info["status"] == 0
        return elbo, grad
    a, b = run(False), run(True)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]), (a, b)


def test_state_rules(engine):
    # planned, no step yet
    d1, d2, n, theta, _, _ = PR.SMALL["cold_b0"]
    X, y, x1, x2 = D.gen_grid(*n)
    engine.plan(*MX.plan_args(d1, x1, d2, x2))
    assert code_of(_var_call, engine) == VGGP_ESTATE
    # a full-grid step: no Sinv
    Y = dev(y.reshape(n[1], n[0]))
    engine.elbo_step(Y, engine.sumsq(Y), theta)
    before = engine.posterior(dev(PTS))
    assert code_of(_var_call, engine) == VGGP_ESTATE
    after = engine.posterior(dev(PTS))
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    # an iterative masked step: no Sinv either
    (Ym, W, nobs, yy), _ = PR.masked_step(engine, True)
    before = engine.posterior_masked_iter(dev(PTS), W, nobs)[:2]
    assert code_of(_var_call, engine) == VGGP_ESTATE
    after = engine.posterior_masked_iter(dev(PTS), W, nobs)[:2]
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    # the dense masked step on the same plan: served; an empty axis is refused and leaves the state as it is
    (Ym, W, nobs, yy), _ = PR.masked_step(engine, False)
    before = engine.posterior_masked(dev(PTS))
    mean, var = _var_call(engine)
    assert rel(PR._np(var), PR._np(before[1])) < 1e-6
    empty = torch.empty(0, dtype=torch.float64, device=engine.device)
    assert code_of(_var_call, engine, empty, dev(G2)) == VGGP_EINVAL               # p1 = 0
    assert code_of(_var_call, engine, dev(G1), empty) == VGGP_EINVAL               # p2 = 0
    after = engine.posterior_masked(dev(PTS))
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    # a dense step that is followed by an iterative one is no longer the last step
    PR.masked_step(engine, True)
    assert code_of(_var_call, engine) == VGGP_ESTATE


def test_raster_variance_is_refused_on_a_paired_context(engine):
    X, y, x1, x2 = D.gen_grid(16, 12)
    Z = np.random.default_rng(3).uniform(0.05, 0.95, (12, 2))
    engine.plan_paired("matern32", Z, x1, x2)
    Y = dev(y.reshape(12, 16))
    elbo, grad, info = engine.elbo_step(Y, engine.sumsq(Y), [0.3, 0.25, 0.9, 1.2, 0.02])
    assert info["status"] == 0
    before = engine.posterior_masked(dev(PTS))
    with pytest.raises(VggpError) as ei:
        _var_call(engine)
    assert ei.value.code == VGGP_EINVAL and "paired" in str(ei.value)
    after = engine.posterior_masked(dev(PTS))
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])


# ---- 4. model level --------------------------------------------------------------------------------------------------------------------
def test_posterior_grid_raster_variance_on_scattered_data(engine):
    from variational_gridded_gaussian_processes_amd.models import Matern12GriddedGP
    X, y = PR.scattered_problem()
    model = Matern12GriddedGP(torch.tensor(X), torch.tensor(y), 9, (0, 1), (0, 1), engine=engine).to(torch.float64)
    assert model._scattered
    a1, a2 = PR._axes()
    pp = model.posterior(torch.cartesian_prod(a1, a2))
    pg = model.posterior_grid(a1, a2, raster_variance=True)
    e_v = rel(pg.variance.numpy(), pp.variance.numpy())
    print(f"RASTER_VAR model scattered 37x21 var_vs_pointwise {e_v:.3e} 1e-06")
    assert pg.variance.shape == (len(G1) * len(G2),) and e_v < 1e-6
    assert rel(pg.mean.numpy(), pp.mean.numpy()) < 1e-6
    assert torch.equal(model.posterior_grid(a1, a2).variance, pp.variance)            # the default: the point-wise route, bit for bit
    noise = model.likelihood.noise.detach().double()
    pred = model.posterior_predictive_grid(a1, a2, raster_variance=True)
    assert torch.equal(pred.variance, pg.variance + noise)
    assert torch.equal(model.posterior_predictive_grid(a1, a2).variance, pp.variance + noise)
    with pytest.raises(NotImplementedError):
        pg.covariance_matrix


def test_posterior_grid_raster_variance_changes_nothing_on_a_full_grid(engine):
    from variational_gridded_gaussian_processes_amd.models import Matern12GriddedGP
    X, y, x1, x2 = D.gen_grid(24, 20)
    model = Matern12GriddedGP(torch.tensor(X), torch.tensor(y), 9, (0, 1), (0, 1), engine=engine).to(torch.float64)
    a1, a2 = PR._axes()
    plain, kw = model.posterior_grid(a1, a2), model.posterior_grid(a1, a2, raster_variance=True)
    # (each call's refresh is one more warm-started step at the same hyper-parameters: the same bounds, not the same bits)
    assert rel(kw.mean.numpy(), plain.mean.numpy()) < 1e-7 and rel(kw.variance.numpy(), plain.variance.numpy()) < 1e-6


def test_posterior_grid_raster_variance_is_refused_on_the_iterative_solver(engine):
    from variational_gridded_gaussian_processes_amd.models import Matern12GriddedGP
    X, y = PR.scattered_problem()
    model = Matern12GriddedGP(torch.tensor(X), torch.tensor(y), 9, (0, 1), (0, 1), engine=engine,
                              scattered_solver="iterative").to(torch.float64)
    a1, a2 = PR._axes()
    with pytest.raises(NotImplementedError, match=r"posterior\("):
        model.posterior_grid(a1, a2, raster_variance=True)
    with pytest.raises(NotImplementedError, match=r"posterior\("):
        model.posterior_predictive_grid(a1, a2, raster_variance=True)
    assert model.posterior_grid(a1, a2).mean.shape == (len(G1) * len(G2),)            # the default is served as before
