"""The specification of the B0 cells under the Matern-3/2 and Matern-5/2 kernels (tests/b0_kinds_spec.py, what VGGP_BASIS_B0K is tested
against on the GPU) pinned on the CPU:

  * against 50-digit quadrature of the defining integrals (tests/golden/b0_kinds_hp.npz, written by tests/golden/make_b0_kinds_hp.py
    without any closed form), |spec - hp| <= c eps S per element, c = 4 max(R_oracle, 1) -- the rule of tests/test_factor_hp.py; no
    element is skipped;
  * sum_k A0[k, p] = the one-cell integral over the whole mesh (the edge terms telescope), 1e-13 relative;
  * K0 symmetric positive definite without jitter at m = 7 and 32, ell = 0.2 on [0, 1];
  * the collapsed (Titsias) bound written out densely in numpy -- Kuu = kron, Kuf = Khatri-Rao of the spec's factors,
    log N(y | 0, Qff + sigma^2 I) - tr(Kff - Qff) / (2 sigma^2) -- against oracle.kron.elbo_step through B0KFactor at 1e-10, and the
    step's lengthscale gradient against central differences of that dense function at 1e-6 (the tolerances of the z_grad / mixed-dims
    CPU checks).  oracle/dense.py raises for this basis, hence the dense bound is written here.
"""
import numpy as np
import pytest

import b0_kinds_spec as B
from oracle import dense as D, kron as Kr

KINDS = ("matern32", "matern52")


@pytest.mark.parametrize("c", B.cases(), ids=B.case_ids())
def test_spec_vs_50_digits(c):
    got = B.sample(c, B.spec_outputs(c.kind, c.grid, c.x, c.ell))
    now = {k: B.ratio_to_bound(got[k], c.hp[k], c.S[k]) for k in B.OUTPUTS}
    print(f"{c.id}: err / (eps S) now " + " ".join(f"{k} {now[k]:.2f}" for k in B.OUTPUTS) + f"; stored R_oracle {c.R_oracle:.2f}")
    for k in B.OUTPUTS:
        assert now[k] <= B.tolerance_constant(c), (k, now[k])


def test_fixture_covers_the_edges():
    """both mesh ends, interior knots (the (a, b] convention), outside on both sides, distance 0 (a column on a knot), a distance where
    exp underflows -- in every case; all seven ell / delta for both kernels; delta = 1/32"""
    seen = set()
    for c in B.cases():
        seen.add((c.kind, c.ratio))
        lo, hi = c.grid[0], c.grid[-1]
        assert c.grid[1] - c.grid[0] == 1.0 / 32
        assert lo in c.x and hi in c.x and (c.x < lo).any() and (c.x > hi).any()
        assert np.isin(c.grid[1:-1], c.x).sum() >= 3
        assert np.abs(c.x - lo).max() / c.ell > 760.0
        assert (c.hp["A0"] == 0.0).any() or c.ratio not in ("1/2000", "1/700", "1/100")      # far cells underflow at small ell
        assert {0, 1, 2}.issubset({int(abs(i - j)) for i, j in c.Kidx})
    assert seen == {(k, r) for k in KINDS for r in ("1/2000", "1/700", "1/100", "1", "30", "320", "3.2e4")}


@pytest.mark.parametrize("c", B.cases(), ids=B.case_ids())
def test_float64_scales_equal_the_stored_ones(c):
    got = B.sample(c, B.spec_scales(c.kind, c.grid, c.x, c.ell))
    for k in B.OUTPUTS:
        assert np.allclose(got[k], c.S[k], rtol=1e-12, atol=0.0), k


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ell", [0.004, 0.2, 30.0])
def test_rows_telescope_to_the_whole_mesh(kind, ell):
    rng = np.random.default_rng(3)
    mesh = np.linspace(-0.5, 1.5, 41)
    x = np.concatenate([mesh, rng.uniform(-1.0, 2.0, 60)])
    A, dA = B.b0k_A(kind, mesh, x, ell)
    whole = np.array([mesh[0], mesh[-1]])
    A1, dA1 = B.b0k_A(kind, whole, x, ell)
    # |sum - whole| against the sum of the cells (all non-negative): 1e-13 relative
    assert np.all(np.abs(A.sum(0) - A1[0]) <= 1e-13 * np.abs(A).sum(0))
    S_d = B.S_b0k_A(kind, mesh, x, ell)[1].sum(0)
    assert np.all(np.abs(dA.sum(0) - dA1[0]) <= 1e-13 * S_d)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [7, 32])
def test_K0_is_positive_definite_without_jitter(kind, m):
    K, dK = B.b0k_K(kind, m, 1.0 / m, 0.2)
    assert np.array_equal(K, K.T) and np.array_equal(dK, dK.T)
    lam = np.linalg.eigvalsh(K)
    print(f"{kind} m = {m}: lambda_min {lam[0]:.3e}, cond {lam[-1] / lam[0]:.3e}")
    assert lam[0] > 0.0
    assert Kr.chol_jitter(K)[1] == 0.0


def test_matern12_is_the_oracles_b0():
    mesh, x = np.linspace(0, 1, 10), np.linspace(-0.2, 1.2, 31)
    f, g = B.factor("matern12", mesh, x), Kr.Factor("b0", "matern12", mesh, x)
    for a, b in zip(f.build(0.3), g.build(0.3)):
        assert np.array_equal(a, b)
    assert f.m == 9 and not f.inverse


# ---- the dense bound ---------------------------------------------------------------------------------------------------------
N1, N2, MESH1, MESH2 = 8, 6, np.linspace(0.0, 1.0, 5), np.linspace(0.0, 1.0, 4)      # 8 x 6 grid, 4 x 3 cells


def dense_bound(kind, x1, x2, Y, theta):
    """log N(y | 0, Qff + sigma^2 I) - tr(Kff - Qff) / (2 sigma^2) with every matrix formed (N = 48, M = 12); y[j * n1 + i] = Y[j, i]"""
    l1, l2, s1, s2, sig2 = theta
    K1, _ = B.b0k_K(kind, len(MESH1) - 1, float(MESH1[1] - MESH1[0]), l1)
    K2, _ = B.b0k_K(kind, len(MESH2) - 1, float(MESH2[1] - MESH2[0]), l2)
    A1, _ = B.b0k_A(kind, MESH1, x1, l1)
    A2, _ = B.b0k_A(kind, MESH2, x2, l2)
    Kuu = np.kron(s1 * K1, s2 * K2)                                       # u = i1 * m2 + i2
    X1, X2 = np.tile(np.arange(len(x1)), len(x2)), np.repeat(np.arange(len(x2)), len(x1))      # observation p = j * n1 + i
    Kuf = ((s1 * A1)[:, None, X1] * (s2 * A2)[None, :, X2]).reshape(Kuu.shape[0], -1)           # Khatri-Rao
    Qff = Kuf.T @ np.linalg.solve(Kuu, Kuf)
    y, N = Y.reshape(-1), Y.size
    C = Qff + sig2 * np.eye(N)
    _, logdet = np.linalg.slogdet(C)
    fit = -0.5 * (N * np.log(2 * np.pi) + logdet + y @ np.linalg.solve(C, y))
    return fit - 0.5 * (N * s1 * s2 - np.trace(Qff)) / sig2              # kappa(0) = 1: Kff has the diagonal s1 s2


@pytest.mark.parametrize("kind", KINDS)
def test_step_through_B0KFactor_is_the_dense_titsias_bound(kind):
    X, y, x1, x2 = D.gen_grid(N1, N2)
    Y = np.asarray(y, np.float64).reshape(N2, N1)
    theta = np.array([0.31, 0.47, 1.3, 0.8, 0.05])
    f1, f2 = B.factor(kind, MESH1, x1), B.factor(kind, MESH2, x2)
    st = Kr.elbo_step(Y, f1, f2, theta)
    assert st.d1.jit == 0.0 and st.d2.jit == 0.0
    ref = dense_bound(kind, x1, x2, Y, theta)
    print(f"{kind}: structured {st.elbo:.12f} dense {ref:.12f}")
    assert abs(st.elbo - ref) <= 1e-10 * abs(ref)
    for d in range(2):
        h = 1e-5 * theta[d]
        tp, tm = theta.copy(), theta.copy()
        tp[d] += h
        tm[d] -= h
        fd = (dense_bound(kind, x1, x2, Y, tp) - dense_bound(kind, x1, x2, Y, tm)) / (2 * h)
        print(f"  d / d ell{d + 1}: analytic {st.grad[d]:.10f} central difference {fd:.10f}")
        assert abs(st.grad[d] - fd) <= 1e-6 * max(abs(fd), np.abs(st.grad).max())
