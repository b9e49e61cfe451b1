"""Joint samples on the dense masked / scattered states on the GPU: vggp_tri_t_apply on every edge (integer-exact), and
vggp_qv_sample_masked / vggp_posterior_raster_sample_masked against tests/dense_sample_spec.py, the GPU's own dense covariances, the
dense oracles, each other, and through the models (dense_samples=True).

Bounds (none of them comes from what the code gives):
    kernel edges                 equality: small-integer data, every product and partial sum is an integer far below 2^53
    covariance by unit noise     1e-7 of the largest entry, the bound of test_gpu_qv_sample.py and test_gpu_raster_sample.py for the same
                                 check on the other states; the diagonal against posterior_raster_var_masked at test_gpu_raster_var.py's 1e-6
    same noise against the spec  1e-7 of the largest entry, the project's bound for dense-state read-outs against the oracle
    one joint draw with q(v)     1e-10: both sides are the same GPU draw X_s pushed through well-conditioned B0 factors (cond(L0_d) < 100)
    seeds and blocks             bit for bit on q(v) (one wave sums each element of X in a fixed order; the tail is the iterative
                                 sampler's, bitwise there too), 1e-12 on the raster (another block width reorders GEMM tiles: its rule)
"""
from __future__ import annotations

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import dense_sample_spec as Ds
import mixed_dims_cases as Mx
import qv_sample_cases as Cs
import qv_sample_spec as S
import raster_sample_spec as R
from oracle import kron as Kr
from test_gpu_qv_sample import check_sampler, code_of, dev, host, masked_xy, plan24
from test_gpu_raster_sample import SENTINEL, check_grid_sampler, dense_cov_masked, guarded_in, guarded_out, judge_cov
from variational_gridded_gaussian_processes_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
rel = Cs.rel
EINVAL, ESTATE = _lib.VGGP_EINVAL, _lib.VGGP_ESTATE
A1, A2 = Ds.A1, Ds.A2
MAIN = ["masked-b0-9x7", "scattered-rbf-8x9", "scattered-m32pts8-vff9"]


# ---- 1. the kernel on its own: every edge, integer-exact ---------------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 4), (9, 7), (8, 9), (12, 11), (5, 33), (33, 5), (16, 16), (31, 67)]
BLOCKS = [(64, 64), (64, 1), (7, 5), (1, 1)]


def poisoned(Xl: torch.Tensor) -> torch.Tensor:
    x = Xl.double().clone()
    M = x.shape[0]
    x[torch.triu(torch.ones(M, M, dtype=torch.bool), diagonal=1)] = float("nan")
    return x


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tri_t_apply_is_exact_on_every_edge(engine, shape):
    """out = tril(Xl)^T E on small integers, NaN above the diagonal of Xl and around every operand, sentinel bands around the output:
    M = 1, M < nbc, M = 12, 63, 72, 132, 165 (165 both ways round: tiles that straddle i1 boundaries), 256 and 2077 (65 tiles: 32 mirror
    pairs and the odd one out)."""
    m1, m2 = shape
    M = m1 * m2
    g = torch.Generator(device="cpu").manual_seed(1000 * m1 + m2)
    Xl = torch.randint(-3, 4, (M, M), generator=g)
    xl = guarded_in(poisoned(Xl))
    for nbc, cn in BLOCKS:
        E = torch.randint(-4, 5, (m1, nbc, m2), generator=g)
        ref = Ds.tri_t_apply(Xl.numpy(), E.numpy(), cn)
        parent, out = guarded_out(m1, nbc, m2)
        engine.tri_t_apply(xl, guarded_in(E.double()), cn, out=out)
        got = out.cpu().numpy()
        what = (m1, m2, nbc, cn)
        assert np.isfinite(got).all(), what
        assert np.array_equal(got, ref.astype(np.float64)), (what, int((got != ref).sum()))
        assert not got[:, cn:, :].any(), what                                           # the dead columns are written, as zeros
        band = parent.numel() - out.numel()
        assert bool((parent[:band // 2] == SENTINEL).all()) and bool((parent[-(band // 2):] == SENTINEL).all()), what


@pytest.mark.parametrize("shape", [(9, 7), (31, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tri_t_apply_bits_do_not_depend_on_the_block(engine, shape):
    """Real-valued data: a column's bits are the same in a block of 64 and alone, in a ragged block, and from call to call."""
    m1, m2 = shape
    M = m1 * m2
    g = torch.Generator(device="cpu").manual_seed(7)
    xl = poisoned(torch.randn(M, M, generator=g, dtype=torch.float64)).to(DEV)
    E = torch.randn(m1, 64, m2, generator=g, dtype=torch.float64).to(DEV)
    full = engine.tri_t_apply(xl, E)
    assert torch.equal(full, engine.tri_t_apply(xl, E)) and bool(torch.isfinite(full).all())
    ref = np.tril(np.nan_to_num(host(xl))).T @ host(E).transpose(0, 2, 1).reshape(M, 64)
    assert rel(host(full).transpose(0, 2, 1).reshape(M, 64), ref) <= 1e-12
    for c in (0, 17, 48, 63):
        alone = engine.tri_t_apply(xl, E[:, c:c + 1, :].contiguous())
        assert torch.equal(alone[:, 0, :], full[:, c, :]), c
    ragged = engine.tri_t_apply(xl, E[:, :7, :].contiguous(), cn=5)
    assert torch.equal(ragged[:, :5, :], full[:, :5, :]) and not bool(ragged[:, 5:, :].any())


def test_tri_t_apply_refuses_bad_arguments(engine):
    t = torch.zeros(12, 12, dtype=torch.float64, device=DEV)
    e = torch.full((3, 2, 4), SENTINEL, dtype=torch.float64, device=DEV)
    o = torch.full((3, 2, 4), SENTINEL, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda x: x.data_ptr()
    lib, h = engine.lib, engine._h
    for args in ((p(t), 3, 4, p(e), 2, 2, p(e)),                                        # in place
                 (None, 3, 4, p(e), 2, 2, p(o)), (p(t), 3, 4, None, 2, 2, p(o)), (p(t), 3, 4, p(e), 2, 2, None),
                 (p(t), 0, 4, p(e), 2, 2, p(o)), (p(t), 3, 0, p(e), 2, 2, p(o)), (p(t), 129, 128, p(e), 2, 2, p(o)),
                 (p(t), 3, 4, p(e), 2, 0, p(o)), (p(t), 3, 4, p(e), 2, 3, p(o)), (p(t), 3, 4, p(e), 65, 2, p(o))):
        assert lib.vggp_tri_t_apply(h, *args, st) == EINVAL, args
    assert lib.vggp_tri_t_apply(None, p(t), 3, 4, p(e), 2, 2, p(o), st) == EINVAL
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all()) and bool((e == SENTINEL).all())


# ---- the dense states ----------------------------------------------------------------------------------------------------------------------------
def plan_step(engine, name):
    """Plan the problem and take its dense step -> (problem, step(theta) for a further step on the same data)."""
    p = Ds.problem(name)
    if p["kind"] == "masked":
        engine.plan(*Mx.plan_args(p["d1"], p["x1"], p["d2"], p["x2"]))
        Wd = dev(p["W"])
        Ym = dev(p["Y"]) * Wd
        nobs, yy = float(p["W"].sum()), engine.sumsq(Ym)
        step = lambda theta: engine.elbo_step_masked(Ym, Wd, nobs, yy, theta)
    else:
        X = p["X"]
        engine.plan(*Mx.plan_args(p["d1"], X[:, 0], p["d2"], X[:, 1]), scattered=True)
        yd = dev(p["y"])
        yy = float((yd * yd).sum().item())
        step = lambda theta: engine.elbo_step_scattered(yd, yy, theta)
    step(p["theta"])
    return p, step


def dense_cov_any(engine, xs, M):
    """dense_cov_masked (three groups of <= M / 2 points) for any number of points: with groups of <= M / 2 points every pair of points
    lies in the union of two groups, one posterior_cov call per pair of groups."""
    if len(xs) <= 3 * (M // 2):
        return dense_cov_masked(engine, xs, M)
    groups = np.array_split(np.arange(len(xs)), -(-len(xs) // (M // 2)))
    cov = np.full((len(xs), len(xs)), np.nan)
    for i in range(len(groups)):
        for j in range(i + 1, len(groups)):
            idx = np.concatenate([groups[i], groups[j]])
            cov[np.ix_(idx, idx)] = host(engine.posterior_cov(dev(xs[idx]), masked=True))
    assert np.isfinite(cov).all()
    return cov


def padded(a: np.ndarray, n: int) -> np.ndarray:
    """Zero-noise samples appended up to n samples."""
    return a if len(a) >= n else np.concatenate([a, np.zeros((n - len(a),) + a.shape[1:])])


# ---- 2. covariance by unit noise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MAIN + ["masked-b0-3x4"])
def test_covariance_by_unit_noise(engine, name):
    """M unit vectors as eps_u (then G and H as well): the outer sum of the samples about the mean IS the covariance.  The M = 12
    problem draws 70 samples, more columns in its first block than it has cells."""
    p, _ = plan_step(engine, name)
    st, f1, f2, theta = p["st"], p["f1"], p["f2"], p["theta"]
    m1, m2, p1, p2 = f1.m, f2.m, len(A1), len(A2)
    M, nmin = m1 * m2, 70 if name == "masked-b0-3x4" else 0
    _, _, s1, s2, _ = theta
    # q(v)
    E = padded(np.concatenate([np.eye(M), np.zeros((1, M))]).reshape(M + 1, m1, m2), nmin)
    V, info = engine.qv_sample_masked(len(E), eps_u=dev(E))
    mean, _ = engine.qv_masked()
    assert torch.equal(V[-1], mean) and torch.equal(V[M], mean)                          # zero noise: the mean, bit for bit
    assert info["rounds"] == (0, 0) and info["sweeps"] == (0, 0)
    got = Cs.outer_sum(host(V), host(mean))
    e_gpu, e_or = rel(got, host(engine.qv_cov_masked())), rel(got, Kr.q_v_cov_masked(st, f1, f2))
    print(f"{name}: q(v), {len(E)} samples vs qv_cov_masked {e_gpu:.1e}, vs the oracle {e_or:.1e}")
    assert e_gpu <= 1e-7 and e_or <= 1e-7
    # the raster: eps_u alone gives the q(u) part of posterior_cov_masked
    xs = R.cartesian(A1, A2)
    ax = Ds.raster_axes(st, f1, f2, A1, A2)
    nug = R.nugget_terms(ax, theta)
    cov_gpu = dense_cov_any(engine, xs, M)                                                # (M = 12 < 35 points: by pairs of groups)
    cov_or = Kr.posterior_cov_masked(st, f1, f2, xs)
    resid = s1 * s2 * (np.kron(ax.k1, ax.k2) - np.kron(ax.U1.T @ ax.U1, ax.U2.T @ ax.U2))
    mu, _ = engine.posterior_raster(dev(A1), dev(A2), want_var=False)
    Eu = padded(np.eye(M).reshape(M, m1, m2), nmin)
    Fu, info = engine.posterior_raster_sample_masked(A1, A2, len(Eu), eps_u=dev(Eu), eps_g=dev(np.zeros((len(Eu), p1, p2))),
                                                     eps_h=dev(np.zeros((len(Eu), m1, p2))))
    assert info["rounds"] == (0, 0) and info["sweeps"] == (0, 0) and info["jitter"] == (0.0, 0.0)
    got = Cs.outer_sum(host(Fu), host(mu))
    T = np.einsum("ip,jq->ijpq", ax.U1, ax.U2).reshape(M, p1 * p2)
    e_or = rel(got, s1 * s2 * (T.T @ st.Sinv @ T))
    e_gpu = rel(got, cov_gpu - resid)
    print(f"{name}: raster, eps_u alone vs the q(u) part of the GPU's posterior_cov_masked {e_gpu:.1e}, of the oracle's {e_or:.1e}")
    assert e_gpu <= 1e-7 and e_or <= 1e-7
    # ... and E, G, H together the whole covariance plus the nugget terms
    E, G, H = (padded(a, nmin) for a in R.unit_noise_egh(m1, m2, p1, p2))
    F, _ = engine.posterior_raster_sample_masked(A1, A2, len(E), eps_u=dev(E), eps_g=dev(G), eps_h=dev(H))
    assert torch.equal(F[-1], mu)
    judge_cov(name, host(F), host(mu), cov_gpu, cov_or, nug)
    _, var = engine.posterior_raster_var_masked(dev(A1), dev(A2))
    e_d = rel(np.diag(Cs.outer_sum(host(F), host(mu))), host(var).reshape(-1) + np.diag(nug))
    print(f"{name}: diagonal vs posterior_raster_var_masked + nugget {e_d:.1e}")
    assert e_d <= 1e-6


# ---- 3. the same noise against the numpy specification --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MAIN)
def test_same_noise_vs_spec(engine, name):
    """Explicit noise (65 samples: two blocks, the second ragged) and generated noise (seed 3) against the specification fed the same
    numbers.  Measured on the MI355X: DESIGN.md section 7j."""
    p, _ = plan_step(engine, name)
    st, f1, f2 = p["st"], p["f1"], p["f2"]
    m1, m2, p1, p2, S_ = f1.m, f2.m, len(A1), len(A2), 65
    rng = np.random.default_rng(300)
    eu, eg, eh = rng.standard_normal((S_, m1, m2)), rng.standard_normal((S_, p1, p2)), rng.standard_normal((S_, m1, p2))
    V, _ = engine.qv_sample_masked(S_, eps_u=dev(eu))
    F, info = engine.posterior_raster_sample_masked(A1, A2, S_, eps_u=dev(eu), eps_g=dev(eg), eps_h=dev(eh))
    want_f, levels = Ds.sample_raster(st, f1, f2, A1, A2, eu, eg, eh)
    e_v, e_f = rel(host(V), Ds.sample_qv(st, f1, f2, eu)), rel(host(F), want_f)
    print(f"{name}: explicit noise, {S_} samples vs spec: q(v) {e_v:.1e}, raster {e_f:.1e}; root levels {info['jitter']} (spec {levels})")
    assert e_v <= 1e-7 and e_f <= 1e-7 and info["jitter"] == (0.0, 0.0)
    seed, first, n = 3, 2, 5
    Vs, _ = engine.qv_sample_masked(n, seed=seed, first=first)
    Fs, _ = engine.posterior_raster_sample_masked(A1, A2, n, seed=seed, first=first)
    su, sg, sh = S.noise_u(seed, first, n, m1, m2), R.noise_g(seed, first, n, p1, p2), R.noise_h(seed, first, n, m1, p2)
    e_v, e_f = rel(host(Vs), Ds.sample_qv(st, f1, f2, su)), rel(host(Fs), Ds.sample_raster(st, f1, f2, A1, A2, su, sg, sh)[0])
    print(f"{name}: seed {seed}, samples {first}..{first + n - 1} vs the spec with the spec's own generator: q(v) {e_v:.1e}, raster {e_f:.1e}")
    assert e_v <= 1e-7 and e_f <= 1e-7


def test_raster_samples_and_qv_samples_are_one_joint_draw(engine):
    """eps_g = eps_h = 0: raster sample minus mu is B1^T X_s B2 for the very X_s behind the q(v) sample of the same eps_u, recovered
    from that sample through the (well-conditioned B0) factors L0_d."""
    p, _ = plan_step(engine, "masked-b0-9x7")
    st, f1, f2 = p["st"], p["f1"], p["f2"]
    m1, m2, p1, p2, S_ = f1.m, f2.m, len(A1), len(A2), 9
    _, _, s1, s2, _ = p["theta"]
    eu = dev(np.random.default_rng(4).standard_normal((S_, m1, m2)))
    V, _ = engine.qv_sample_masked(S_, eps_u=eu)
    F, _ = engine.posterior_raster_sample_masked(A1, A2, S_, eps_u=eu, eps_g=dev(np.zeros((S_, p1, p2))), eps_h=dev(np.zeros((S_, m1, p2))))
    mean, _ = engine.qv_masked()
    mu, _ = engine.posterior_raster(dev(A1), dev(A2), want_var=False)
    Y = host(V - mean[None]) / S._scale(st.theta, f1, f2)                                # L0_1 X L0_2^T
    X = np.stack([sla.solve_triangular(st.d2.L, sla.solve_triangular(st.d1.L, y, lower=True).T, lower=True).T for y in Y])
    ax = Ds.raster_axes(st, f1, f2, A1, A2)
    want = np.sqrt(s1 * s2) * (ax.U1.T @ X @ ax.U2)
    err = rel(host(F - mu[None]), want)
    print(f"raster sample - mu vs B1^T X_s B2 with the X_s of the q(v) sample: {err:.1e}")
    assert err <= 1e-10
    # the seed path shares stream 0: the seeded raster sample's coefficient part is the seeded q(v) sample's
    Vs, _ = engine.qv_sample_masked(3, seed=21, first=2)
    Ve, _ = engine.qv_sample_masked(3, eps_u=engine.normal_fill(21, 0, 2 * m1 * m2, 3 * m1 * m2).reshape(3, m1, m2))
    assert torch.equal(Vs, Ve)


# ---- 4. seeds and blocks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["masked-b0-9x7", "scattered-m32pts8-vff9"])
def test_seeds_and_blocks(engine, name):
    p, _ = plan_step(engine, name)
    m1, m2, p1, p2 = p["f1"].m, p["f2"].m, len(A1), len(A2)
    M = m1 * m2
    qv = lambda n, **kw: engine.qv_sample_masked(n, **kw)[0]
    w70 = qv(70, seed=11)
    assert torch.equal(qv(1, seed=11, first=5)[0], w70[5]) and torch.equal(qv(5, seed=11, first=3), w70[3:8])
    assert torch.equal(qv(70, seed=11, block=7), w70) and torch.equal(qv(70, seed=11, block=64), w70)
    assert torch.equal(qv(70, eps_u=engine.normal_fill(11, 0, 0, 70 * M).reshape(70, m1, m2)), w70)   # the seed path IS the explicit path
    assert not torch.equal(w70[0], w70[1]) and not torch.equal(w70, qv(70, seed=12))
    ra = lambda n, **kw: engine.posterior_raster_sample_masked(A1, A2, n, **kw)[0]
    r70 = ra(70, seed=11)
    e1, e2, e3 = rel(host(ra(1, seed=11, first=5)[0]), host(r70[5])), rel(host(ra(5, seed=11, first=3)), host(r70[3:8])), \
        rel(host(ra(70, seed=11, block=7)), host(r70))
    print(f"{name}: raster, first = 5 alone vs row 5 of 70: {e1:.1e}; rows 3..7 as a block of 5: {e2:.1e}; block = 7: {e3:.1e}")
    assert e1 <= 1e-12 and e2 <= 1e-12 and e3 <= 1e-12
    explicit = ra(5, eps_u=engine.normal_fill(11, 0, 3 * M, 5 * M).reshape(5, m1, m2),
                  eps_g=engine.normal_fill(11, 2, 3 * p1 * p2, 5 * p1 * p2).reshape(5, p1, p2),
                  eps_h=engine.normal_fill(11, 3, 3 * m1 * p2, 5 * m1 * p2).reshape(5, m1, p2))
    assert torch.equal(explicit, ra(5, seed=11, first=3))
    # zero noise: the means of vggp_qv_masked and vggp_posterior_raster, bit for bit
    z = lambda *s: dev(np.zeros(s))
    assert torch.equal(qv(2, eps_u=z(2, m1, m2))[1], engine.qv_masked()[0])
    assert torch.equal(ra(2, eps_u=z(2, m1, m2), eps_g=z(2, p1, p2), eps_h=z(2, m1, p2))[1], engine.posterior_raster(dev(A1), dev(A2), want_var=False)[0])


# ---- 5. state and refusals ------------------------------------------------------------------------------------------------------------------------
def raw_calls(engine, guard_q, guard_r):
    """The two C entries on sentinel-filled outputs: keyword overrides -> return code."""
    lib, h = engine.lib, engine._h
    st = torch.cuda.current_stream().cuda_stream
    a1, a2 = dev(A1), dev(A2)
    ptr = lambda t: None if t is None else t.data_ptr()

    def qv(n=2, first=0, eps_u=None, block=0, out=guard_q):
        return lib.vggp_qv_sample_masked(h, n, 1, first, ptr(eps_u), block, ptr(out), None, st)

    def ra(n=2, first=0, eps_u=None, eps_g=None, eps_h=None, block=0, out=guard_r, g1=a1, g2=a2, p1=len(A1), p2=len(A2)):
        return lib.vggp_posterior_raster_sample_masked(h, ptr(g1), p1, ptr(g2), p2, n, 1, first, ptr(eps_u), ptr(eps_g), ptr(eps_h), block,
                                                       ptr(out), None, st)
    return qv, ra, (a1, a2)


def test_state_and_refusals(engine):
    from test_gpu_qv_sample import step_masked_iter
    from variational_gridded_gaussian_processes_amd import Engine
    p = plan24(engine, "b0-matern12")                                                    # 6 x 4 features, 14 x 11 grid with holes
    W, nobs = p["W"], p["nobs"]
    guard_q = torch.full((2, 6, 4), SENTINEL, dtype=torch.float64, device=DEV)
    guard_r = torch.full((2, 7, 5), SENTINEL, dtype=torch.float64, device=DEV)
    qv, ra, keep = raw_calls(engine, guard_q, guard_r)
    untouched = lambda: bool((guard_q == SENTINEL).all()) and bool((guard_r == SENTINEL).all())
    # VGGP_ESTATE: a plan alone, a full-grid step, an iterative step, a re-plan after a dense step
    assert qv() == ESTATE and ra() == ESTATE
    engine.elbo_step(p["Y"], p["yy_full"], Cs.THETA)
    assert qv() == ESTATE and ra() == ESTATE
    step_masked_iter(engine, p)
    assert qv() == ESTATE and ra() == ESTATE
    engine.elbo_step_masked(p["Ym"], W, nobs, p["yy"], Cs.THETA)
    plan24(engine, "b0-matern12")
    assert qv() == ESTATE and ra() == ESTATE
    assert "dense masked" in engine.lib.vggp_last_error().decode()
    # VGGP_EINVAL, in the matching state, before anything is written
    engine.elbo_step_masked(p["Ym"], W, nobs, p["yy"], Cs.THETA)
    z = lambda *s: dev(np.zeros(s))
    eu, eg, eh = z(2, 6, 4), z(2, 7, 5), z(2, 6, 5)
    long_axis = dev(np.linspace(0, 1, 8193))
    for kw in (dict(n=0), dict(n=-3), dict(first=-1), dict(out=None), dict(block=65)):
        assert qv(**kw) == EINVAL, kw
        assert ra(**kw) == EINVAL, kw
    for kw in (dict(g1=None), dict(g2=None), dict(p1=0), dict(p2=0), dict(g1=long_axis, p1=8193), dict(g2=long_axis, p2=8193),
               dict(eps_u=eu), dict(eps_g=eg), dict(eps_h=eh), dict(eps_u=eu, eps_g=eg), dict(eps_u=eu, eps_h=eh), dict(eps_g=eg, eps_h=eh)):
        assert ra(**kw) == EINVAL, list(kw)
    torch.cuda.synchronize()
    assert untouched()
    assert qv() == 0 and ra() == 0 and qv(eps_u=eu) == 0 and ra(eps_u=eu, eps_g=eg, eps_h=eh, block=64) == 0
    assert engine.qv_sample_masked(3, seed=1)[0].shape == (3, 6, 4) and engine.posterior_raster_sample_masked(A1, A2, 3, seed=1)[0].shape == (3, 7, 5)
    # B1 hats: q(v) samples exist (e_d = -1), the raster refuses and names the indefinite residual
    pb = plan24(engine, "b1-matern12")
    engine.elbo_step_masked(pb["Ym"], pb["W"], pb["nobs"], pb["yy"], Cs.THETA)
    guard_q.fill_(SENTINEL), guard_r.fill_(SENTINEL)
    qv, ra, keep = raw_calls(engine, guard_q, guard_r)
    assert ra() == EINVAL and "indefinite" in engine.lib.vggp_last_error().decode() and untouched()
    assert qv() == 0
    # paired inducing points
    Z = np.random.default_rng(0).uniform(0, 1, (10, 2))
    engine.plan_paired("matern12", Z, p["x1"], p["x2"])
    engine.elbo_step(p["Y"], p["yy_full"], Cs.THETA)
    guard_q.fill_(SENTINEL), guard_r.fill_(SENTINEL)
    qv, ra, keep = raw_calls(engine, guard_q, guard_r)
    for call in (qv, ra):
        assert call() == EINVAL and "PAIRED" in engine.lib.vggp_last_error().decode()
    assert untouched()
    # multi-rank contexts: refused, and the message says so
    eng2 = Engine(0, n_ranks=2, rank=0, allreduce=lambda buf: None)
    try:
        basis, kind, g1, g2 = Cs.BASES["b0-matern12"]
        eng2.plan(kind, basis, g1, p["x1"], kind, basis, g2, p["x2"])
        for call in (lambda: eng2.qv_sample_masked(2), lambda: eng2.posterior_raster_sample_masked(A1, A2, 2)):
            code, msg = code_of(call)
            assert code == EINVAL and "multi-rank" in msg
    finally:
        eng2.close()


@pytest.mark.parametrize("name", ["masked-b0-9x7", "scattered-rbf-8x9"])
def test_sampling_leaves_the_state_and_the_next_step_unchanged(engine, name):
    theta2 = [0.25, 0.28, 1.1, 0.9, 0.012]
    xs = dev(R.cartesian(A1, A2))

    def readouts():
        return engine.qv_masked() + engine.posterior_masked(xs) + engine.posterior_raster_var_masked(dev(A1), dev(A2))

    def run(with_samples):
        _, step = plan_step(engine, name)
        before = readouts()
        if with_samples:
            V, _ = engine.qv_sample_masked(70, seed=1)
            F, _ = engine.posterior_raster_sample_masked(A1, A2, 70, seed=1, block=16)
            assert bool(torch.isfinite(V).all()) and bool(torch.isfinite(F).all())
            after = readouts()
            assert all(torch.equal(a, b) for a, b in zip(before, after))                 # the point-wise read-outs: the same bits
        elbo, grad, _ = step(theta2)
        return elbo, grad
    a, b = run(False), run(True)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]), (a, b)


# ---- 6. models -------------------------------------------------------------------------------------------------------------------------------------
def scattered_xy(n, seed):
    X, y = Ds.scattered_data(n, seed)
    return torch.tensor(X), torch.tensor(y)


def test_models_dense_samples(engine):
    """dense_samples=True on a grid with holes (solver='dense') and on 400 scattered points: q_v().sample and posterior_grid().sample are
    the Engine calls, reproducible, one joint draw; the predictive variant adds sqrt(noise) times stream 4 (check_grid_sampler)."""
    from variational_gridded_gaussian_processes_amd.models import Matern12GriddedGP
    a1, a2 = torch.tensor(A1), torch.tensor(A2)
    Xm, ym = masked_xy(24, 20)
    Xs, ys = scattered_xy(400, 3)
    for tag, model in (("masked", Matern12GriddedGP(Xm, ym, 9, (0, 1), (0, 1), engine=engine, solver="dense", dense_samples=True)),
                       ("scattered", Matern12GriddedGP(Xs, ys, 9, (0, 1), (0, 1), engine=engine, dense_samples=True))):
        model = model.to(torch.float64)
        assert model.dense_samples and not (model._iter or model._siter)
        qv, a = check_sampler(model, 64)
        assert bool(((a - qv.mean).abs() <= 8.0 * qv.stddev + 1e-12).all())               # 8 samples cannot leave mean +- 8 sigma
        assert model.last_readout_info["sweeps"] == (0, 0) and model.last_readout_info["rounds"] == (0, 0)
        assert torch.equal(a, engine.qv_sample_masked(8, 3, 0)[0].reshape(8, -1).cpu())
        assert rel(qv.mean, engine.qv_masked()[0].reshape(-1).cpu()) == 0.0
        pg, f = check_grid_sampler(model, engine)
        assert bool(((f - pg.mean).abs() <= 8.0 * pg.stddev + 1e-12).all())
        assert torch.equal(f, engine.posterior_raster_sample_masked(a1, a2, 8, 3, 0)[0].reshape(8, -1).cpu())
        # the covariance of the dense state, whatever root draws from it: the model's covariance_matrix against 64 unit draws
        V, _ = engine.qv_sample_masked(64, eps_u=dev(np.eye(64).reshape(64, 8, 8)))
        e = rel(Cs.outer_sum(host(V), qv.mean.numpy().reshape(8, 8)), qv.covariance_matrix.numpy())
        print(f"{tag} model: unit draws vs q_v().covariance_matrix {e:.1e}")
        assert e <= 1e-7


def test_models_beyond_the_old_cap(engine):
    """m = 65 x 65 = 4225 > 4096 B0 features on 600 scattered points (Sigma~ factors without jitter: test_dense_sample_spec.py)."""
    from variational_gridded_gaussian_processes_amd.models import Matern12GriddedGP
    X, y = scattered_xy(600, 7)
    big = Matern12GriddedGP(X, y, 66, (0, 1), (0, 1), engine=engine, dense_samples=True).to(torch.float64)
    qv = big.q_v()
    s = qv.sample(torch.Size([2]), seed=1)
    assert s.shape == (2, 4225) and bool(torch.isfinite(s).all()) and not torch.equal(s[0], s[1])
    assert not (big._iter or big._siter)
    zero, _ = engine.qv_sample_masked(1, eps_u=dev(np.zeros((1, 65, 65))))
    assert torch.equal(zero[0], engine.qv_masked()[0]) and torch.equal(zero[0].reshape(-1).cpu(), qv.mean)
    assert bool(((s - qv.mean).abs() <= 8.0 * qv.stddev + 1e-12).all())


def test_models_without_the_flag_and_refusals(engine):
    """dense_samples=False (the default): the symmetric-root sample of the dense covariance (the model's nknots gives m = 8 x 8, M = 64),
    NotImplementedError above M = 4096, and the raster refusals with their messages -- as test_models_sample / test_models_sample_maps pin
    them.  With the flag, B1 hats still refuse on the raster and paired inducing points have no sampler."""
    from oracle import dense as D
    from variational_gridded_gaussian_processes_amd.models import (GriddedMatern12SVGP, Matern12B1SplineASVGP, Matern12GriddedGP,
                                                                   MultivariateNormal, _symmetric_root)
    a1, a2 = torch.tensor(A1), torch.tensor(A2)
    Xm, ym = masked_xy(24, 20)
    Xs, ys = scattered_xy(400, 3)
    de = Matern12GriddedGP(Xm, ym, 9, (0, 1), (0, 1), engine=engine, solver="dense").to(torch.float64)
    assert de.dense_samples is False
    qd = de.q_v()
    s = qd.sample(torch.Size([8]), seed=3)
    eps = engine.normal_fill(3, 0, 0, 8 * 64).reshape(8, 64).cpu()
    assert rel(s, qd.mean[None] + eps @ _symmetric_root(qd.covariance_matrix)) <= 1e-12
    big = MultivariateNormal(torch.zeros(4097), torch.ones(4097), cov_fn=lambda: torch.eye(4097, dtype=torch.float64))
    big._sample_fn = de._dense_sampler(big)
    with pytest.raises(NotImplementedError, match="solver='iterative'"):
        big.sample()
    with pytest.raises(NotImplementedError, match="solver='iterative'"):
        de.posterior_grid(a1, a2).sample()
    ds = Matern12GriddedGP(Xs, ys, 9, (0, 1), (0, 1), engine=engine).to(torch.float64)
    with pytest.raises(NotImplementedError, match="scattered_solver='iterative'"):
        ds.posterior_predictive_grid(a1, a2).sample()
    # the flag changes nothing on a full grid and on the iterative solvers
    Xf, yf, _, _ = D.gen_grid(24, 20)
    full = Matern12GriddedGP(torch.tensor(Xf), torch.tensor(yf), 9, (0, 1), (0, 1), engine=engine, dense_samples=True).to(torch.float64)
    plain = Matern12GriddedGP(torch.tensor(Xf), torch.tensor(yf), 9, (0, 1), (0, 1), engine=engine).to(torch.float64)
    assert torch.equal(full.q_v().sample(torch.Size([3]), seed=2), plain.q_v().sample(torch.Size([3]), seed=2))
    it = Matern12GriddedGP(Xm, ym, 9, (0, 1), (0, 1), engine=engine, solver="iterative", dense_samples=True).to(torch.float64)
    assert it.q_v().sample(torch.Size([2]), seed=2).shape == (2, 64) and it._iter and it.last_readout_info["sweeps"][0] == 1
    # with the flag: B1 hats refuse on the raster, paired inducing points have no sampler at all
    b1 = Matern12B1SplineASVGP(Xm, ym, 9, (0, 1), (0, 1), engine=engine, dense_samples=True).to(torch.float64)
    with pytest.raises(NotImplementedError, match="indefinite"):
        b1.posterior_grid(a1, a2).sample()
    Z = torch.tensor(np.random.default_rng(0).uniform(0, 1, (12, 2)))
    pa = GriddedMatern12SVGP(torch.tensor(Xf), torch.tensor(yf), Z, 8, (0, 1), (0, 1), inducing="general", engine=engine,
                             dense_samples=True).to(torch.float64)
    with pytest.raises(NotImplementedError, match="paired"):
        pa.posterior_grid(a1, a2)
    with pytest.raises(NotImplementedError, match="joint samples"):
        pa.q_u().sample()
