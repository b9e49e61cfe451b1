"""Inputs and error measures for the dense building blocks (vggp_cholesky_inverse, vggp_trsm, vggp_kron_solve, vggp_eigh): numpy only.

Integer-exact families.  Every intermediate of a Cholesky factorisation, a substitution, an explicit inverse or a product
formed from them is an integer far below 2^53, so fp64 arithmetic is exact in ANY order of summation and the kernels are
compared by equality.  All pivots are exactly 1 (the kernels' rcp / rsq seeds followed by two Newton steps return 1.0 for 1.0).
    tree_L         identity plus one +-1 per row i >= 1 at a random column < i; inverse in {0, +-1}
    two_level_L    (I + N) tree_L, N dense in {-1, 0, 1} on rows >= m // 2, columns < m // 2: L, L^-1, K = L L^T, K^-1 all integer
    dense_unit_L   unit lower triangular, {-1, 0, 1} below the diagonal: 16 x 16 diagonal-block inverses below 2^15, the full
                   inverse NOT representable -- only where nothing larger than a 16 x 16 block is inverted
Floating families.
    spd_with_lmin        Q diag(d) Q^T, d on [0.5, 2] with one entry replaced by lmin (the jitter ladder's handle)
    well_conditioned_L   tril(randn, -1) / sqrt(m) + diag(U[1, 2])
Error measures (numpy.longdouble, u = 2^-53): the componentwise ratios of DESIGN.md section 5b.
"""
import numpy as np

U = 2.0 ** -53
JITTERS = (0.0, 1e-8, 1e-7, 1e-6)

# sizes of the GPU tests (tests/test_dense_cases.py checks the premises at each of them)
CHOL_SMALL = (1, 2, 15, 16, 17, 31, 33, 100, 113, 127, 128)
CHOL_BLOCKED = (129, 130, 255, 256, 257, 300)
LADDER_SIZES = (17, 100, 128, 129, 200, 300)
LADDER = ((-3e-9, 1e-8), (-3e-8, 1e-7), (-3e-7, 1e-6), (-3e-6, None))          # (lambda_min, expected jitter; None = not PD)
TRSM_SIZES = (1, 15, 16, 17, 31, 32, 33, 48, 65, 100, 113, 127, 128, 129, 130, 255, 256, 257, 300)
TRSM_NCOLS = (1, 15, 16, 17, 63, 64, 65, 77)
KRON_SMALL = ((1, 1), (1, 37), (17, 33), (16, 128), (100, 128), (128, 128), (113, 31))
KRON_LARGE = ((129, 96), (96, 129), (257, 130))


def trsm_ncols(m):
    """Two column counts per m, walking TRSM_NCOLS so that every count meets an m <= 128 and an m > 128."""
    k = TRSM_SIZES.index(m)
    return TRSM_NCOLS[(2 * k) % 8], TRSM_NCOLS[(2 * k + 1) % 8]


# ---- integer-exact families ----------------------------------------------------------------------------------------------------
def tree_L(m, seed):
    rng = np.random.default_rng([seed, m, 1])
    L = np.eye(m)
    for i in range(1, m):
        L[i, rng.integers(0, i)] = rng.choice((-1.0, 1.0))
    return L


def tree_L_inv(L):
    """Exact inverse of a tree_L by substitution in int64."""
    m = L.shape[0]
    Li = np.eye(m, dtype=np.int64)
    A = L.astype(np.int64)
    for i in range(1, m):
        Li[i, :i] = -(A[i, :i] @ Li[:i, :i])
    return Li.astype(np.float64)


def two_level_L(m, seed):
    """-> L, Linv (both exact integers in float64)."""
    T = tree_L(m, seed)
    h = m // 2
    N = np.zeros((m, m))
    N[h:, :h] = np.random.default_rng([seed, m, 2]).integers(-1, 2, size=(m - h, h))
    L = (np.eye(m) + N) @ T
    Linv = tree_L_inv(T) @ (np.eye(m) - N)            # N^2 = 0
    return L, Linv


def dense_unit_L(m, seed):
    rng = np.random.default_rng([seed, m, 3])
    return np.tril(rng.integers(-1, 2, size=(m, m)).astype(np.float64), -1) + np.eye(m)


def int_rhs(shape, seed):
    return np.random.default_rng([seed, 4]).integers(-8, 9, size=shape).astype(np.float64)


def kron_int_case(n1, n2, tree):
    """-> L1, L2, X, Y = K1 X K2^T formed in int64, K_d = L_d L_d^T; tree_L factors (integer inverses) or dense_unit_L ones."""
    fam = tree_L if tree else dense_unit_L
    L1, L2 = fam(n1, 1), fam(n2, 2)
    X = int_rhs((n1, n2), n1 * 1000 + n2)
    K1, K2 = (L1 @ L1.T).astype(np.int64), (L2 @ L2.T).astype(np.int64)
    return L1, L2, X, (K1 @ X.astype(np.int64) @ K2.T).astype(np.float64)


# ---- floating families ---------------------------------------------------------------------------------------------------------
def random_orthogonal(m, seed):
    Q, R = np.linalg.qr(np.random.default_rng([seed, m, 5]).standard_normal((m, m)))
    return Q * np.sign(np.diag(R))


def spd_with_lmin(m, lmin, seed):
    rng = np.random.default_rng([seed, m, 6])
    d = rng.uniform(0.5, 2.0, m)
    d[rng.integers(0, m)] = lmin
    Q = random_orthogonal(m, seed)
    K = (Q * d) @ Q.T
    return 0.5 * (K + K.T)


def well_conditioned_L(m, seed):
    rng = np.random.default_rng([seed, m, 7])
    return np.tril(rng.standard_normal((m, m)), -1) / np.sqrt(m) + np.diag(rng.uniform(1.0, 2.0, m))


def chol_ladder(K):
    """psd_safe_cholesky's schedule in numpy: -> (L, jitter) or (None, -1.0) when no level is positive definite."""
    for jit in JITTERS:
        try:
            L = np.linalg.cholesky(K + jit * np.eye(K.shape[0]))
        except np.linalg.LinAlgError:
            continue
        if np.isfinite(L).all():
            return L, jit
    return None, -1.0


# ---- symmetric matrices for the eigensolver ------------------------------------------------------------------------------------
def sym_from_spectrum(d, seed):
    m = len(d)
    Q = random_orthogonal(m, seed)
    G = (Q * np.asarray(d, dtype=np.float64)) @ Q.T
    return 0.5 * (G + G.T)


def eig_case(family, m, seed=0):
    """One symmetric test matrix of family a .. i (module docstring of tests/test_gpu_eigh_paths.py)."""
    rng = np.random.default_rng([seed, m, 8])
    if family == "geometric":
        return sym_from_spectrum(np.logspace(0, -10, m) if m > 1 else np.ones(1), seed)
    if family == "clusters":
        return sym_from_spectrum(np.array([3.0, 1.0, 0.25])[np.arange(m) % 3], seed)
    if family == "indefinite":
        h = np.linspace(0.1, 1.0, m // 2)
        return sym_from_spectrum(np.concatenate([h, -h, np.zeros(m - 2 * (m // 2))]), seed)
    if family == "rank_deficient":
        B = rng.standard_normal((m, max(m // 2, 1)))
        return B @ B.T
    if family == "diagonal":
        return np.diag(rng.permutation(np.arange(1, m + 1) / 8.0))
    if family == "scaled_identity":
        return 3.0 * np.eye(m)
    if family == "scaled_up":
        return eig_case("geometric", m, seed) * 2.0 ** 200
    if family == "scaled_down":
        return eig_case("geometric", m, seed) * 2.0 ** -200
    if family == "equal_pair":
        G = 2.0 * np.eye(m)
        i, j = (m - 1, 0) if m > 1 else (0, 0)
        if m > 1:
            G[i, j] = G[j, i] = 0.5
        return G
    if family == "zero":
        return np.zeros((m, m))
    raise ValueError(family)


EIG_FAMILIES = ("geometric", "clusters", "indefinite", "rank_deficient", "diagonal", "scaled_identity", "scaled_up", "scaled_down",
                "equal_pair", "zero")


# ---- error measures ------------------------------------------------------------------------------------------------------------
def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def kappa_blocks(L, b):
    """Largest infinity-norm condition number of the b x b diagonal blocks of the lower-triangular L."""
    worst = 1.0
    for r in range(0, L.shape[0], b):
        D = np.tril(L[r:r + b, r:r + b])
        worst = max(worst, np.abs(D).sum(1).max() * np.abs(np.linalg.inv(D)).sum(1).max())
    return float(worst)


def _ratio(err, scale):
    """max_ij err / scale with 0 / 0 = 0 (an entry whose scale vanishes must be exact)."""
    err, scale = np.abs(err), np.abs(scale)
    if np.any((scale == 0) & (err != 0)):
        return np.inf
    return float((err[scale > 0] / scale[scale > 0]).max()) if np.any(scale > 0) else 0.0


def trsm_omega(L, X, R, trans=False):
    """Componentwise backward error max |op(L) X - R| / (|op(L)| |X|), op(L) = tril(L) or its transpose."""
    A = _ld(np.tril(L))
    A = A.T if trans else A
    return _ratio(A @ _ld(X) - _ld(R), np.abs(A) @ np.abs(_ld(X)))


def chol_ratio(L, Kj):
    """max |L L^T - Kj| / (|L| |L^T|) over the LOWER triangle (the factorisation's input)."""
    Ld = _ld(np.tril(L))
    E, S = Ld @ Ld.T - _ld(Kj), np.abs(Ld) @ np.abs(Ld).T
    il = np.tril_indices(L.shape[0])
    return _ratio(E[il], S[il])


def inv_ratio(L, Linv):
    """max |L Linv - I| / (|L| |Linv|) over the lower triangle."""
    A, B = _ld(np.tril(L)), _ld(np.tril(Linv))
    E, S = A @ B - np.eye(L.shape[0], dtype=np.longdouble), np.abs(A) @ np.abs(B)
    il = np.tril_indices(L.shape[0])
    return _ratio(E[il], S[il])
