"""CPU check of the specification of the joint raster samples (tests/raster_sample_spec.py): its covariance by unit noise over
(E, G, H) against oracle.kron.posterior_cov on cartesian_prod(g1, g2) plus the nugget terms, the jitter levels of the roots, the
refusal of B1 hats, and the index spaces of the two new noise streams."""
from __future__ import annotations

import numpy as np
import pytest

import qv_sample_cases as Cs
import qv_sample_spec as S
import raster_sample_spec as R
from oracle import kron as Kr

# a 7 x 5 raster whose axes are aligned with nothing: neither the data nodes, nor the meshes, nor the inducing points
A1 = np.array([0.013, 0.171, 0.3337, 0.52, 0.649, 0.803, 0.987])
A2 = np.array([0.041, 0.29, 0.4777, 0.71, 0.962])
# VFF, e_d = -1: [a, b, omega_0 .. omega_Mf]; m1 = 2 * 3 + 1 = 7, m2 = 2 * 2 + 1 = 5
VFF1 = np.concatenate([[-0.2, 1.2], 2.0 * np.pi * np.arange(4) / 1.4])
VFF2 = np.concatenate([[-0.2, 1.2], 2.0 * np.pi * np.arange(3) / 1.4])


def factors(case, x1, x2):
    if case == "vff-matern12":
        return Kr.Factor("vff", "matern12", VFF1, np.asarray(x1, float)), Kr.Factor("vff", "matern12", VFF2, np.asarray(x2, float))
    return Cs.factors(case, x1, x2)


@pytest.mark.parametrize("case", ["b0-matern12", "points-matern32", "points-rbf", "vff-matern12"])
def test_covariance_by_unit_noise_is_the_posterior_covariance(case):
    Y, _, x1, x2 = Cs.grid_data()
    f1, f2 = factors(case, x1, x2)
    st = Kr.elbo_step(Y, f1, f2, Cs.THETA)
    m1, m2, p1, p2 = f1.m, f2.m, len(A1), len(A2)
    E, G, H = R.unit_noise_egh(m1, m2, p1, p2)
    F, levels = R.sample_full(st, f1, f2, A1, A2, E, G, H)
    mu = R.mean_full(st, f1, f2, A1, A2)
    assert np.array_equal(F[-1], mu)                                     # zero noise: the mean, bit for bit
    got = Cs.outer_sum(F[:-1], mu)
    ax = R.axes_full(st, f1, f2, A1, A2)
    bare = Kr.posterior_cov(st, f1, f2, R.cartesian(A1, A2))
    want = bare + R.nugget_terms(ax, st.theta)
    err = Cs.rel(got, want)
    lo = [float(np.linalg.eigvalsh(r).min()) for r in (ax.r1, ax.r2)]
    cond = [float(np.linalg.cond(r + R.ETA * np.eye(len(r)))) for r in (ax.r1, ax.r2)]
    print(f"{case}: unit noise vs posterior_cov + nugget {err:.1e} (nugget alone {Cs.rel(want, bare):.1e}); "
          f"smallest eigenvalues of r_d {lo[0]:.2e} {lo[1]:.2e}; cond(r_d + eta I) {cond[0]:.1e} {cond[1]:.1e}; levels {levels}")
    assert err <= 1e-10
    assert levels == (0.0, 0.0, 0.0)                                     # every root at jitter level 0
    assert min(lo) > -1e-12                                              # the residuals are PSD to rounding


def test_b1_hats_are_refused_and_their_residual_is_indefinite():
    Y, _, x1, x2 = Cs.grid_data()
    f1, f2 = Cs.factors("b1-matern12", x1, x2)
    st = Kr.elbo_step(Y, f1, f2, Cs.THETA)
    E, G, H = R.unit_noise_egh(f1.m, f2.m, len(A1), len(A2))
    with pytest.raises(NotImplementedError, match="indefinite"):
        R.sample_full(st, f1, f2, A1, A2, E, G, H)
    # the reason: k_d - q_d has negative eigenvalues for hats (the covariance of that basis is no Schur complement)
    import scipy.linalg as sla
    L0 = R._unit_L0(st.d1, f1, st.theta[2])
    U = sla.solve_triangular(L0, f1.build(Cs.THETA[0], x=A1)[2], lower=True)
    k = Kr.kappa_and_dell("matern12", np.abs(A1[:, None] - A1[None, :]), Cs.THETA[0])[0]
    assert np.linalg.eigvalsh(k - U.T @ U).min() < -1e-3


def test_noise_streams_and_index_spaces():
    seed, first, n, p1, p2, m1 = 11, 3, 4, 7, 5, 6
    G, H = R.noise_g(seed, first, n, p1, p2), R.noise_h(seed, first, n, m1, p2)
    # sample s of a seed is the same numbers whatever call asks for it
    assert np.array_equal(G[2], R.noise_g(seed, first + 2, 1, p1, p2)[0]) and np.array_equal(H[1], R.noise_h(seed, first + 1, 1, m1, p2)[0])
    s, a, b = 2, 4, 3
    assert G[s, a, b] == S.normals_at(seed, 2, (first + s) * p1 * p2 + a * p2 + b)
    assert H[s, a, b] == S.normals_at(seed, 3, (first + s) * m1 * p2 + a * p2 + b)
    assert R.noise_pred(seed, first, n, p1 * p2)[s, a * p2 + b] == S.normals_at(seed, 4, (first + s) * p1 * p2 + a * p2 + b)
    # the streams are distinct sequences
    assert not np.array_equal(G.reshape(-1)[:20], S.normal_fill(seed, 3, first * p1 * p2, 20))
