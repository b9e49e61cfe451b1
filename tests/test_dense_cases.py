"""CPU checks of the premises the GPU path tests of the dense blocks rest on (tests/dense_cases.py): the integer families are
integer, bounded and recovered bit for bit by numpy / scipy; the jitter ladder lands where the oracle says; the reference
routines alone stay inside the componentwise limits of DESIGN.md section 5b."""
import numpy as np
import pytest
import scipy.linalg as sla

import dense_cases as dc
from oracle import kron as Kr

CHOL_SIZES = dc.CHOL_SMALL + dc.CHOL_BLOCKED


def is_int(a):
    return np.array_equal(a, np.rint(a))


@pytest.mark.parametrize("m", CHOL_SIZES)
def test_two_level_family_is_integer_and_bounded(m):
    L, Li = dc.two_level_L(m, 0)
    K, Ki = L @ L.T, Li.T @ Li
    assert all(is_int(a) for a in (L, Li, K, Ki))
    assert np.array_equal(np.diag(L), np.ones(m)) and np.array_equal(L, np.tril(L)) and np.array_equal(Li, np.tril(Li))
    assert np.array_equal(L @ Li, np.eye(m)) and np.array_equal(K @ Ki, np.eye(m))
    # sums of m products of such entries stay below 2^53 by ten orders of magnitude
    assert np.abs(L).max() <= 8 and np.abs(Li).max() <= 8 and np.abs(K).max() <= 512 and np.abs(Ki).max() <= 512
    assert m * 512.0 * 512.0 < 2.0 ** 53 * 1e-7
    assert np.array_equal(np.linalg.cholesky(K), L)
    assert np.array_equal(sla.solve_triangular(L, np.eye(m), lower=True), Li)
    if m >= 17:
        assert (K != 0).mean() > 0.5


@pytest.mark.parametrize("m", sorted(set(dc.CHOL_SMALL + dc.TRSM_SIZES)))
def test_dense_unit_family(m):
    L = dc.dense_unit_L(m, 0)
    assert is_int(L) and np.array_equal(np.diag(L), np.ones(m)) and np.abs(L).max() <= 1
    for r in range(0, m, 16):
        Di = np.linalg.inv(L[r:r + 16, r:r + 16])
        assert np.abs(Di).max() < 2 ** 15 and np.array_equal(np.rint(Di) @ L[r:r + 16, r:r + 16], np.eye(Di.shape[0]))
    if m <= 128:
        assert np.array_equal(np.linalg.cholesky(L @ L.T), L)
    for nc in (dc.trsm_ncols(m) if m in dc.TRSM_SIZES else (17,)):
        X = dc.int_rhs((m, nc), m)
        A = L.astype(np.int64)
        for trans in (0, 1):
            R = ((A.T if trans else A) @ X.astype(np.int64)).astype(np.float64)
            assert np.abs(R).max() <= 8 * m
            assert np.array_equal(sla.solve_triangular(L, R, lower=True, trans=trans), X)


def test_trsm_ncols_cover_both_paths():
    small = {c for m in dc.TRSM_SIZES if m <= 128 for c in dc.trsm_ncols(m)}
    large = {c for m in dc.TRSM_SIZES if m > 128 for c in dc.trsm_ncols(m)}
    assert small == set(dc.TRSM_NCOLS) and large == set(dc.TRSM_NCOLS)


@pytest.mark.parametrize("n1,n2", dc.KRON_SMALL + dc.KRON_LARGE)
def test_kron_integer_cases(n1, n2):
    L1, L2, X, Y = dc.kron_int_case(n1, n2, tree=True)
    Li1, Li2 = dc.tree_L_inv(L1), dc.tree_L_inv(L2)
    assert np.abs(Li1).max() <= 1 and np.abs(Li2).max() <= 1 and np.array_equal(L1 @ Li1, np.eye(n1))
    P1, P2 = Li1.T @ Li1, Li2.T @ Li2
    assert np.abs(Y).max() <= 1024 and (np.abs(P1) @ np.abs(Y) @ np.abs(P2)).max() < 2.0 ** 53 * 1e-6
    assert np.array_equal(P1 @ Y @ P2, X) and np.array_equal(Kr.kron_solve(L1, L2, Y), X)
    if max(n1, n2) <= 128:            # all-substitution path: dense unit factors are allowed
        L1, L2, X, Y = dc.kron_int_case(n1, n2, tree=False)
        assert np.abs(Y).max() < 2.0 ** 31
        assert np.array_equal(Kr.kron_solve(L1, L2, Y), X)


@pytest.mark.parametrize("m", dc.LADDER_SIZES)
def test_jitter_ladder_matches_the_oracle(m):
    for lmin, expect in dc.LADDER:
        K = dc.spd_with_lmin(m, lmin, 0)
        assert abs(np.linalg.eigvalsh(K).min() - lmin) < 1e-3 * abs(lmin)
        L, jit = dc.chol_ladder(K)
        if expect is None:
            assert L is None and jit == -1.0
            with pytest.raises(np.linalg.LinAlgError):
                Kr.chol_jitter(K)
        else:
            Lr, jr = Kr.chol_jitter(K)
            assert jit == expect == jr and np.array_equal(L, Lr)


@pytest.mark.parametrize("m", CHOL_SIZES)
def test_reference_cholesky_inside_limits(m):
    K = dc.spd_with_lmin(m, 3e-9, 0)
    L, jit = dc.chol_ladder(K)
    assert jit == 0.0
    Linv = sla.solve_triangular(L, np.eye(m), lower=True)
    lim = dc.kappa_blocks(L, 16 if m <= 128 else 128) * (m + 1) * dc.U
    assert dc.chol_ratio(L, K) <= lim and dc.inv_ratio(L, Linv) <= lim
    # the reference itself needs no block factor (Higham Thm 10.3 / Thm 8.5)
    assert dc.chol_ratio(L, K) <= (m + 1) * dc.U and dc.inv_ratio(L, Linv) <= (m + 1) * dc.U


@pytest.mark.parametrize("m", CHOL_SIZES)
def test_reference_cholesky_well_conditioned(m):
    W = dc.well_conditioned_L(m, 3)
    K = W @ W.T
    K = 0.5 * (K + K.T)
    L, jit = dc.chol_ladder(K)
    assert jit == 0.0 and dc.kappa_blocks(L, 16 if m <= 128 else 128) < 128
    Linv = sla.solve_triangular(L, np.eye(m), lower=True)
    assert dc.chol_ratio(L, K) <= (m + 1) * dc.U and dc.inv_ratio(L, Linv) <= (m + 1) * dc.U


@pytest.mark.parametrize("m", dc.TRSM_SIZES)
def test_reference_trsm_inside_limits(m):
    L = dc.well_conditioned_L(m, 0)
    assert np.linalg.cond(L) < 8 and dc.kappa_blocks(L, 16) < 16
    for nc in dc.trsm_ncols(m):
        R = np.random.default_rng(m).standard_normal((m, nc))
        for trans in (0, 1):
            X = sla.solve_triangular(L, R, lower=True, trans=trans)
            assert dc.trsm_omega(L, X, R, trans) <= m * dc.U


@pytest.mark.parametrize("family", dc.EIG_FAMILIES)
def test_eig_families(family):
    for m in (2, 17, 97):
        G = dc.eig_case(family, m)
        assert np.array_equal(G, G.T) and np.isfinite(G).all()
        w = np.linalg.eigvalsh(G)
        nrm = max(np.abs(w).max(), 1e-300)
        if family == "clusters":
            assert len(np.unique(np.round(w, 9))) == min(3, m)
        if family == "indefinite":
            assert np.abs(np.sort(w) - np.sort(-w)).max() < 1e-14 and w.min() < 0 < w.max()
        if family == "rank_deficient":
            assert (np.abs(w) < 1e-12 * nrm).sum() == m - m // 2
        if family == "diagonal":
            assert np.array_equal(G, np.diag(np.diag(G))) and len(set(np.diag(G))) == m and np.any(np.diff(np.diag(G)) > 0)
        if family in ("scaled_up", "scaled_down"):
            assert nrm > 2.0 ** 190 or nrm < 2.0 ** -190
        if family == "equal_pair":
            assert G[0, 0] == G[m - 1, m - 1] and G[m - 1, 0] != 0
        if family == "zero":
            assert not G.any()
