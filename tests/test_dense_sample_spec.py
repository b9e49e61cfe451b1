"""CPU check of the specification of the joint samples on the dense masked / scattered states (tests/dense_sample_spec.py): the
coefficient draw is a root of Sigma~^-1, the unit-noise outer sums reproduce the oracle's dense covariances of q(v) and of the raster,
the product's reference honours the triangle and the interleaved layout, and the M = 4225 problem of the model test factors."""
from __future__ import annotations

import numpy as np
import pytest
import scipy.linalg as sla

import dense_sample_spec as Ds
import mixed_dims_cases as Mx
import qv_sample_cases as Cs
import raster_sample_spec as R
from oracle import kron as Kr

A1, A2 = Ds.A1, Ds.A2


@pytest.mark.parametrize("name", list(Ds.CASES))
def test_the_draw_is_a_root_of_sigma_inverse(name):
    p = Ds.problem(name)
    st = p["st"]
    M = st.Sig.shape[0]
    Xg = sla.solve_triangular(np.linalg.cholesky(st.Sig), np.eye(M), lower=True)            # L^-1, what the dense step keeps
    assert np.abs(np.triu(Xg, 1)).max() == 0.0
    err = Cs.rel(Xg.T @ Xg @ st.Sig, np.eye(M))
    # the draw by unit noise IS Xg^T: column s of the coefficients of E = e_s
    m1, m2 = p["f1"].m, p["f2"].m
    X = Ds.coeff_draw(st, np.eye(M).reshape(M, m1, m2)).reshape(M, M)                        # [s, u]
    e2 = Cs.rel(X, Xg)                                                                       # X[s, u] = (L^-T e_s)[u] = Xg[s, u]
    print(f"{name}: M = {M}, |Xg^T Xg Sigma~ - I| {err:.1e}, draw of unit noise vs L^-1 {e2:.1e}, cond(Sigma~) {np.linalg.cond(st.Sig):.1e}")
    assert err <= 1e-10 and e2 <= 1e-12
    assert Cs.rel(Xg.T @ Xg, st.Sinv) <= 1e-10


@pytest.mark.parametrize("name", list(Ds.CASES))
def test_unit_noise_reproduces_the_dense_covariances(name):
    p = Ds.problem(name)
    st, f1, f2 = p["st"], p["f1"], p["f2"]
    m1, m2, p1, p2 = f1.m, f2.m, len(A1), len(A2)
    M = m1 * m2
    # q(v)
    E = np.concatenate([np.eye(M), np.zeros((1, M))]).reshape(M + 1, m1, m2)
    V = Ds.sample_qv(st, f1, f2, E)
    mean, _ = Kr.q_v_masked(st, f1, f2)
    assert np.array_equal(V[-1], mean)                                                       # zero noise: the mean, bit for bit
    e_qv = Cs.rel(Cs.outer_sum(V[:-1], mean), Kr.q_v_cov_masked(st, f1, f2))
    # raster: E, G, H
    E, G, H = R.unit_noise_egh(m1, m2, p1, p2)
    F, levels = Ds.sample_raster(st, f1, f2, A1, A2, E, G, H)
    ax = Ds.raster_axes(st, f1, f2, A1, A2)
    mu = Ds.raster_mean(st, ax)
    xs = R.cartesian(A1, A2)
    assert np.array_equal(F[-1], mu)
    assert Cs.rel(mu.reshape(-1), Kr.posterior_masked(st, f1, f2, xs)[0]) <= 1e-12
    bare = Kr.posterior_cov_masked(st, f1, f2, xs)
    e_r = Cs.rel(Cs.outer_sum(F[:-1], mu), bare + R.nugget_terms(ax, st.theta))
    # the q(u) part alone: E only
    Z = np.zeros_like
    Fu, _ = Ds.sample_raster(st, f1, f2, A1, A2, E[:M], Z(G[:M]), Z(H[:M]))
    _, _, s1, s2, _ = st.theta
    T = np.einsum("ip,jq->ijpq", ax.U1, ax.U2).reshape(M, p1 * p2)
    e_u = Cs.rel(Cs.outer_sum(Fu, mu), s1 * s2 * (T.T @ st.Sinv @ T))
    print(f"{name}: unit noise vs q_v_cov_masked {e_qv:.1e}, vs posterior_cov_masked + nugget {e_r:.1e}, q(u) part {e_u:.1e}; levels {levels}")
    assert e_qv <= 1e-10 and e_r <= 1e-10 and e_u <= 1e-10
    assert levels == (0.0, 0.0, 0.0)


def test_product_reference_layout_and_triangle():
    rng = np.random.default_rng(0)
    m1, m2, nbc, cn = 3, 4, 7, 5
    M = m1 * m2
    Xl = rng.integers(-3, 4, (M, M)).astype(np.float64)
    E = rng.integers(-4, 5, (m1, nbc, m2)).astype(np.float64)
    poisoned = Xl.copy()
    poisoned[np.triu_indices(M, 1)] = np.nan
    out = Ds.tri_t_apply(poisoned, E, cn)
    for u in (0, 5, 11):
        for c in (0, 4):
            want = sum(Xl[k, u] * E[k // m2, c, k % m2] for k in range(u, M))
            assert out[u // m2, c, u % m2] == want
    assert np.all(out[:, cn:, :] == 0) and np.isfinite(out).all()


def test_the_large_model_problem_factors_without_jitter():
    """M = 65 x 65 = 4225 B0 features on 600 scattered points, the model test beyond the old M = 4096 cap, at the model's default
    hyper-parameters: Sigma~ = I + rho Phi has no eigenvalue below 1, its Cholesky needs no jitter and the draw stays finite."""
    X, _ = Ds.scattered_data(600, 7)
    d = Mx.b0(65)
    f1, f2 = Mx.factor(d, X[:, 0].copy()), Mx.factor(d, X[:, 1].copy())
    Sig = Ds.sigma_scattered(X, f1, f2, Kr.theta_from_raw(np.zeros(5)))
    L = np.linalg.cholesky(Sig)                                                              # raises LinAlgError if it does not factor
    assert np.isfinite(L).all() and np.diag(L).min() >= 1.0 - 1e-12
