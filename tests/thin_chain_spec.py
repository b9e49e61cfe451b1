"""Plain numpy references of the four single-workgroup kernels of the thin chain (csrc/step.hip chain_thin): the pivoted-Cholesky range
finder, the row orthonormalisation, the Ritz solve of a matrix given as a product, and the thin m-space tail.  numpy only, no GPU.

The tail's reference is the range-only bound and gradient of the header comment of csrc/thin.hip, written once for any float dtype:
called with numpy.longdouble it is the reference, with float64 "the same formula in working precision".  Every quantity is carried as a
pair (value, sum of the absolute values of the terms that formed it): the second member is the forward-bound scale of the first
(abs_f of test_gpu_scattered_iter.py) -- a sum of n terms evaluated in any order is within n u of it.  tests/test_thin_chain_spec.py
pins this formula to oracle/kron.py finish() on Gram matrices of exact rank; tests/test_gpu_thin_chain_paths.py compares the kernels
with it.  The case lists of both files live here."""
import math

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
VG_EIG_RANK_CUT = 1e-14            # csrc/common.h
VG_THIN_MISS = 1e-12
VG_THIN_ELBO_TOL = 1e-10
VG_ESUBMISS = -100
VGGP_ENOCONV = -6
VG_EIG_DIRECT = 1 << 27            # csrc/eigh.hip: the Newton start was taken
VG_EIG_NEWTON_MAX_M = 48
THETA = (0.3, 0.4, 1.7, 0.6, 0.05)


# ---- pivoted Cholesky (csrc/thin.hip vg_pivchol_kernel) -----------------------------------------------------------------------------
def pivchol(G, Omega, r):
    """r steps of diagonally pivoted Cholesky of G in G's dtype: -> V [r][m] (row i = column l_i, or row i of Omega when the pivot is not
    positive), the pivots (-1 for such a step), lead[i] = (largest - runner-up) / largest of the residual diagonal at step i (0 for
    such a step), and scale [r][m]: (|G_pt| + sum_q |l_tq l_pq|) / sqrt(pivot) + |l_t| (G_pp + sum_q l_pq^2) / (2 pivot), the sums of
    the absolute terms of the two recurrences that form an element: its own and the pivot's residual diagonal under the square root.  Pivot = largest residual diagonal, ties to the lowest index, a pivot is used once."""
    dt = G.dtype.type
    m = G.shape[0]
    L = np.zeros((m, r), dtype=dt)
    d = np.diag(G).copy()
    V = np.zeros((r, m), dtype=dt)
    scale = np.zeros((r, m), dtype=dt)
    piv, lead = [], []
    for i in range(r):
        p = int(np.argmax(d))                      # (first occurrence of the maximum: the lowest index)
        best = d[p]
        if best > 0:
            rest = np.delete(d, p)
            lead.append(float((best - rest.max()) / best) if m > 1 else 1.0)
            c = G[p].copy()
            a = np.abs(G[p])
            for q in range(i):
                c = c - L[:, q] * L[p, q]
                a = a + np.abs(L[:, q] * L[p, q])
            sq = np.sqrt(best)
            li = c / sq
            li[p] = sq
            ap = np.abs(G[p, p]) + (L[p, :i] * L[p, :i]).sum()               # the pivot's residual diagonal has a recurrence of its own
            scale[i] = a / sq + np.abs(li) * ap / (2 * best)
            V[i] = li
            piv.append(p)
        else:
            li = Omega[i].astype(dt) * dt(1e-30)
            V[i] = Omega[i]
            piv.append(-1)
            lead.append(0.0)
        L[:, i] = li
        d = d - li * li
        d[p] = dt(-1.0)
    return V, piv, lead, scale


def graded_chol_case(m, r, seed):
    """G = L L^T with a mildly graded lower-triangular L under a hidden permutation: diagonal 0.9^k, strictly lower part at most a tenth of
    its column's diagonal.  The residual diagonal at step k is 0.81^k at the pivot and at most 0.87 of that anywhere else, so every pivot
    leads by more than a tenth (pivchol() reports the margin), and 0.81^64 = 1e-6 leaves the margins far above the rounding of the
    residual update, which is what decides the order in float64."""
    rng = np.random.default_rng(seed)
    L = np.zeros((m, m))
    dg = 0.9 ** np.arange(m, dtype=float)
    for j in range(m):
        L[j, j] = dg[j]
        L[j + 1:, j] = 0.1 * dg[j] * rng.uniform(-1, 1, m - j - 1)
    Lp = L[rng.permutation(m)]
    G = Lp @ Lp.T
    G = 0.5 * (G + G.T)
    Omega = rng.standard_normal((r, m))
    return G, Omega


def exact_chol_case(m, r, rho, seed):
    """Integer L (m x rho) in pivot-echelon form with powers of two on the pivots, G = L L^T (exact in float64), rank rho < r: every
    product, square root and quotient of the factorisation is exact, the residual after rho steps is exactly zero, and the first rho
    rows of V are L^T bit for bit; the others are rows of Omega.  Pivot k sits in row perm[k]; column k is zero at the earlier pivots."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(m)
    L = np.zeros((m, rho))
    for k in range(rho):
        pk = 2.0 ** (rho + 2 - k)                                    # strictly decreasing pivots, all >= 8
        L[perm[k], k] = pk
        rows = perm[k + 1:]
        L[rows, k] = rng.integers(-1, 2, len(rows)).astype(float)    # entries -1, 0, 1: the pivot's residual diagonal leads by far
    G = L @ L.T
    Omega = rng.standard_normal((r, m))
    return G, Omega, L, perm


# ---- row orthonormalisation (csrc/eigh.hip vg_rowqr_kernel_t) -----------------------------------------------------------------------
def rowqr_checks(Z, V1):
    """The four numbers of the row QR, with the rows of Z scaled to unit norm: max |V1 V1^T - I|; max_k |Z_k - (Z V1^T)_k V1| (the span
    is preserved); max |strict upper part of Z V1^T| (the order is preserved); min diag(Z V1^T) (> 0).  Evaluated in long double."""
    Z, V1 = np.asarray(Z, LD), np.asarray(V1, LD)
    r = Z.shape[0]
    Zn = Z / np.sqrt((Z * Z).sum(1))[:, None]
    R = Zn @ V1.T
    orth = float(np.abs(V1 @ V1.T - np.eye(r, dtype=LD)).max())
    res = Zn - R @ V1
    span = float(np.sqrt((res * res).sum(1)).max())
    upper = float(np.abs(np.triu(R, 1)).max()) if r > 1 else 0.0
    return orth, span, upper, float(np.diag(R).min())


def cgs2(Z):
    """float64 classical Gram-Schmidt with an unconditional second pass: the yardstick of the row QR's caps."""
    Z = np.asarray(Z, np.float64)
    V = np.zeros_like(Z)
    for k in range(Z.shape[0]):
        x = Z[k].copy()
        for _ in range(2):
            x = x - (V[:k] @ x) @ V[:k]
        V[k] = x / np.sqrt(x @ x)
    return V


def rowqr_input(kind, r, m, seed):
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((m, m)))[0][:r]
    if kind == "random":
        return rng.standard_normal((r, m)) + 2.0 * Q
    k6 = 6.0 ** -np.minimum(np.arange(r, dtype=float), 15.4)
    if kind == "graded":            # Z = diag(6^-k) (Q + 1e-3 leak): condition up to 1e12
        return k6[:, None] * (Q + 1e-3 * rng.standard_normal((r, m)))
    if kind == "leaky":             # as the chain sees them (Z = V G): row k is 6^-k q_k + 1e-3 sum_j phi_kj 6^-j q_j -- from the fourth row
        return ((np.eye(r) + 1e-3 * rng.standard_normal((r, r))) * k6[None, :]) @ Q      # on the leak onto q_0 dominates: second pass
    if kind == "orthonormal":
        return Q
    if kind == "dependent":         # row r // 2 is a combination of the rows before it (exactly: small integer weights of integer rows)
        Z = rng.integers(-4, 5, (r, m)).astype(float) + 8.0 * np.eye(r, m)
        k = r // 2
        Z[k] = rng.integers(1, 3, k).astype(float) @ Z[:k]
        return Z
    raise ValueError(kind)


# ---- Ritz solve of a product (csrc/eigh.hip vg_eigh_kernel, VgEigJob::Hl / Hr) ------------------------------------------------------
def ritz_matrix(Hl, Hr):
    P = np.tril(np.asarray(Hl, np.float64) @ np.asarray(Hr, np.float64).T)
    return P + np.tril(P, -1).T


def newton_quotient(H):
    """Largest |h_ij / (h_jj - h_ii)| over the off-diagonal elements above the solver's threshold 1e-13 |H|_F / r: the Newton start of
    csrc/eigh.hip vg_newton_diag declines at 0.3."""
    r = H.shape[0]
    thr = 1e-13 * np.linalg.norm(H) / r
    d = np.diag(H)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.abs(H / (d[None, :] - d[:, None]))
    q[(np.abs(H) <= thr) | np.eye(r, dtype=bool)] = 0.0
    return float(np.nan_to_num(q, nan=np.inf).max())


def ritz_ref(Hl, Hr):
    """Eigenvalues, decreasing, of the symmetric matrix whose lower triangle is tril(Hl Hr^T)."""
    return np.linalg.eigvalsh(ritz_matrix(Hl, Hr))[::-1]


RITZ_SPECTRA = ("decay", "cluster", "split", "deficient")


def ritz_spectrum(name, r):
    k = np.arange(r, dtype=float)
    # (6 x per index down to 1e-12 of the largest, then level: every value stays a factor 100 above the rank cut)
    lam = np.maximum(6.0 ** -k, 1e-12 * (1.0 + 0.5 ** k))
    if name == "cluster" and r >= 4:
        lam[1:4] = lam[1]
    if name == "split" and r >= 3:
        lam[2] = lam[1] * (1.0 - 1e-9)
    if name == "deficient":
        lam[max(1, (2 * r) // 3):] = 0.0
    return lam


def ritz_case(r, hk, spectrum, aligned, seed):
    """Hl = V1 G, Hr = V1: G = Q diag(lam, 0) Q^T symmetric hk x hk, V1 r orthonormal rows of length hk -- the leading eigenvectors
    off by 1e-3 and taken through Z = V G and the row QR (aligned: H = V1 G V1^T is nearly diagonal) or turned by a random rotation of the range (H is dense)."""
    rng = np.random.default_rng(seed)
    lam = ritz_spectrum(spectrum, r)
    Q = np.linalg.qr(rng.standard_normal((hk, hk)))[0]
    G = (Q[:, :r] * lam) @ Q[:, :r].T
    G = 0.5 * (G + G.T)
    if aligned:
        # what a warm step hands the solver: the previous eigenvectors, off by 1e-3 in every direction, after one step of subspace
        # iteration and the top-down orthonormalisation, V1 = orth((Q_r^T + 1e-3 noise) G).  Row k is then off by 1e-3 lam_j / lam_k
        # towards the smaller directions only -- a GRADED rotation, and every quotient h_ij / (h_jj - h_ii) the Newton start looks at is
        # about 1e-3.  (A basis that is off by 1e-3 in the absolute sense is NOT nearly diagonal for a graded spectrum: what leaks onto
        # the leading eigenvector couples two small directions by 1e-6 lam_1 against gaps of 1e-9 lam_1, and the start declines.)
        Zc = (Q[:, :r].T + 1e-3 * rng.standard_normal((r, hk))) @ G
        Zc[lam == 0] = Q[:, :r].T[lam == 0]               # (rank < r: null directions fill the basis up)
        V1 = cgs2(Zc)
    else:
        V1 = np.linalg.qr(rng.standard_normal((r, r)))[0] @ Q[:, :r].T
    return V1 @ G, V1, lam


# r -> (hk, spectrum, aligned): every r and every hk of the issue, staged (r <= 48 and hk <= 128) and not, Newton direct and fallback
RITZ_R = (1, 2, 8, 15, 16, 17, 18, 22, 32, 47, 48, 49, 64)
RITZ_HK = ("r", 33, 127, 128, 129, 200, 256)
RITZ_CASES = [
    (1, "r", "decay", True), (1, 33, "decay", False), (2, "r", "decay", True), (2, 129, "decay", False),
    (8, 33, "decay", True), (8, 33, "deficient", False), (8, 200, "cluster", False),
    (15, 127, "decay", True), (15, 256, "split", False), (16, 128, "decay", False), (16, 129, "decay", True),
    (17, "r", "cluster", True), (17, 200, "decay", True), (18, 33, "split", True), (18, 128, "decay", True), (18, 256, "decay", False),
    (22, 127, "decay", False), (22, 129, "decay", True), (22, 33, "deficient", True),
    (32, "r", "decay", False), (32, 128, "decay", True), (32, 256, "decay", True),
    (47, 127, "decay", True), (47, 200, "decay", False), (48, 128, "decay", True), (48, 128, "decay", False), (48, 129, "decay", True),
    (49, 128, "decay", True), (49, "r", "decay", False), (49, 256, "cluster", False),
    (64, "r", "decay", True), (64, 127, "decay", False), (64, 200, "split", False), (64, 256, "deficient", True),
]
RITZ_CASES = [(r, r if hk == "r" else hk, sp, al) for r, hk, sp, al in RITZ_CASES]


# ---- the thin tail (csrc/thin.hip vg_thin_tail_kernel) ------------------------------------------------------------------------------
class AV:
    """A value and the sum of the absolute values of the terms that formed it (arrays or scalars of one dtype)."""
    __array_priority__ = 1000

    def __init__(self, v, a=None):
        self.v = v
        self.a = np.abs(v) if a is None else a

    @staticmethod
    def of(x):
        return x if isinstance(x, AV) else AV(x)

    def __add__(self, o):
        o = AV.of(o)
        return AV(self.v + o.v, self.a + o.a)

    __radd__ = __add__

    def __sub__(self, o):
        o = AV.of(o)
        return AV(self.v - o.v, self.a + o.a)

    def __rsub__(self, o):
        o = AV.of(o)
        return AV(o.v - self.v, self.a + o.a)

    def __neg__(self):
        return AV(-self.v, self.a)

    def __mul__(self, o):
        o = AV.of(o)
        return AV(self.v * o.v, self.a * o.a)

    __rmul__ = __mul__

    def __matmul__(self, o):
        o = AV.of(o)
        return AV(self.v @ o.v, self.a @ o.a)

    @property
    def T(self):
        return AV(self.v.T, self.a.T)

    def sum(self, axis=None):
        return AV(self.v.sum(axis), self.a.sum(axis))

    def diag(self):
        return AV(np.diag(self.v).copy(), np.diag(self.a).copy())


def status_word(chol_status, eig_err, ritz_status, miss):
    """status[k] of the result block: Cholesky status, then the Ritz solve's status, then VGGP_ENOCONV (bit 0 of the eigensolver's error
    word: a replay workgroup gave up), then VG_ESUBMISS (the miss check, or bit 1 of the error word), then 0."""
    if chol_status:
        return chol_status
    if ritz_status:
        return ritz_status
    if eig_err & 1:
        return VGGP_ENOCONV
    if miss or (eig_err & 2):
        return VG_ESUBMISS
    return 0


def miss_thresholds(inp):
    """-> [(absolute threshold of |tr G - sum theta| in scaled units, the same from the first-order ELBO term)] per dimension."""
    s = (inp["theta"][2], inp["theta"][3])
    v = inp["theta"][4]
    tr = (float(np.sum(inp["dG1"])), float(np.sum(inp["dG2"])))
    out = []
    for k in range(2):
        lam, m = inp["lam%d" % (k + 1)], inp["m%d" % (k + 1)]
        t_abs = VG_THIN_MISS * s[k] * lam[0] * (m - len(lam) + 1)
        t_elbo = VG_THIN_ELBO_TOL * inp["N"] * v / (s[1 - k] * tr[1 - k])
        out.append((t_abs, t_elbo))
    return out


def thin_tail(inp, dtype=np.float64):
    """The range-only bound and gradient.  inp: theta [6] (ell1, ell2, s1, s2, v, sequence number), N, yy, m1, m2, W1, W2 [r][r] (row j =
    Ritz vector j), lam1, lam2 [r], AM1, AH1, AM2, AH2 [r][r], AC [3][r1][r2] (unit scale), dG1, dH1, dG2, dH2: the diagonals of G0, H0
    [m]; optional chol_status [2], eig_err [2], rcounters [2][4], jit [2], peer_fail.
    -> dict: out [6] = ELBO and its gradient by (ell1, ell2, s1, s2, v), abs [6] their forward-bound scales, beta, invd [r1][r2] and
    their scales beta_abs, invd_abs, nrank [2], miss [2], status [2], block: the packed 16-double result block (VgHostOut: out[8],
    jitter[2], int32 counters[2][4], int32 status[2], seq)."""
    dt = np.dtype(dtype).type
    A = lambda x: AV(np.asarray(x, dtype=dtype))      # noqa: E731
    th = [dt(t) for t in inp["theta"]]
    s1, s2, v = th[2], th[3], th[4]
    N, yy = dt(inp["N"]), dt(inp["yy"])
    one, two, half = dt(1), dt(2), dt(0.5)
    iv = one / v
    W1, W2 = A(inp["W1"]), A(inp["W2"])
    l1, l2 = A(inp["lam1"]) * AV(s1), A(inp["lam2"]) * AV(s2)
    E1, F1 = W1 @ A(inp["AM1"]) @ W1.T, W1 @ A(inp["AH1"]) @ W1.T
    E2, F2 = W2 @ A(inp["AM2"]) @ W2.T, W2 @ A(inp["AH2"]) @ W2.T
    rs = np.sqrt(s1 * s2)
    AC = np.asarray(inp["AC"], dtype=dtype)
    P, P1, P2 = [(W1 @ A(AC[q]) @ W2.T) * AV(rs) for q in range(3)]
    a = np.outer(l1.v, l2.v) * iv                      # (products of positive numbers: no cancellation to track)
    D = one + a
    iD = one / D
    beta = AV(P.v * iD, P.a * iD)
    w = AV(-a * iD)                                    # 1/D - 1
    L1c, L2r = AV(l1.v[:, None]), AV(l2.v[None, :])
    S0, S1, S2 = AV(np.log1p(a)).sum(), (P * beta).sum(), (beta * beta).sum()
    S3, S4 = AV(a * iD).sum(), (beta * beta * AV(two + a)).sum()
    S5, S6 = (beta * P1).sum(), (beta * P2).sum()
    X1, X1l = beta @ beta.T, (beta * L2r) @ beta.T
    X2, X2l = beta.T @ beta, (beta * L1c).T @ beta
    S7, S8, S9, S10 = (E1 * X1).sum(), (F1 * X1l).sum(), (E2 * X2).sum(), (F2 * X2l).sum()
    rs1, rl1 = w.sum(1), (w * L2r).sum(1)
    rs2, rl2 = w.sum(0), (w * L1c).sum(0)
    e1, f1, e2, f2 = E1.diag(), F1.diag(), E2.diag(), F2.diag()
    S11, S12, S13, S14 = (e1 * rs1).sum(), (f1 * rl1).sum(), (e1 * l1).sum(), l1.sum()
    S15, S16, S17, S18 = (e2 * rs2).sum(), (f2 * rl2).sum(), (e2 * l2).sum(), l2.sum()
    tr = [A(inp[k]).sum() for k in ("dG1", "dH1", "dG2", "dH2")]
    sl1, sl2 = tr[0] * AV(s1), tr[2] * AV(s2)                    # sum of ALL eigenvalues = trace
    tF1, tF2 = tr[1] * AV(two * s1), tr[3] * AV(two * s2)        # tr(Q^T (H + H^T) Q) = 2 tr H
    Nss, sll = AV(N * s1 * s2), sl1 * sl2
    iv2, hiv = iv * iv, half * iv
    pi = dt(4) * np.arctan(dt(1))
    elbo = -(AV(N * np.log(two * pi)) + AV(N * np.log(v)) + S0 + AV(yy * iv) - S1 * AV(iv2)) * AV(half) - (Nss - sll) * AV(hiv)
    quad1 = S5 * AV(two) - S7 - S8 * AV(two * s1 * iv)
    quad2 = S6 * AV(two) - S9 - S10 * AV(two * s2 * iv)
    g_l1 = -(S11 + (S12 * AV(two * s1) + sl2 * tF1) * AV(iv) - quad1 * AV(iv2)) * AV(half) + sl2 * AV(hiv) * (tF1 - S13)
    g_l2 = -(S15 + (S16 * AV(two * s2) + sl1 * tF2) * AV(iv) - quad2 * AV(iv2)) * AV(half) + sl1 * AV(hiv) * (tF2 - S17)
    common = -(S3 - S2 * AV(iv2)) * AV(half)
    g_s1 = common * AV(one / s1) + sll * AV(hiv / s1) - AV(N * s2 * hiv)
    g_s2 = common * AV(one / s2) + sll * AV(hiv / s2) - AV(N * s1 * hiv)
    g_v = -(AV(N * iv) - S3 * AV(iv) - AV(yy * iv2) + S4 * AV(iv2 * iv)) * AV(half) + (Nss - sll) * AV(half * iv2)
    outs = [elbo, g_l1, g_l2, g_s1, g_s2, g_v]
    res = {"out": np.array([o.v for o in outs], dtype=dtype), "abs": np.array([o.a for o in outs], dtype=dtype),
           "beta": beta.v, "beta_abs": beta.a, "invd": one + w.v, "invd_abs": one + w.a, "trG": (sl1.v, sl2.v), "sth": (S14.v, S18.v)}
    # numerical ranks, the subspace-miss check and the packed block
    nrank, miss, status = [], [], []
    cs, ee = inp.get("chol_status", (0, 0)), inp.get("eig_err", (0, 0))
    rc = np.asarray(inp.get("rcounters", np.zeros((2, 4))), dtype=np.int32)
    for k in range(2):
        l, m = (l1.v, l2.v)[k], inp["m%d" % (k + 1)]
        nrank.append(int(np.sum(l > dt(VG_EIG_RANK_CUT) * l[0])))
        trG, sth, slo = (sl1.v, sl2.v)[k], (S14.v, S18.v)[k], (sl2.v, sl1.v)[k]
        gap = np.abs(trG - sth)
        ok = (gap <= dt(VG_THIN_MISS) * l[0] * dt(m - len(l) + 1)) and (gap * slo * iv <= dt(VG_THIN_ELBO_TOL) * N)
        miss.append(not bool(ok))                       # (a NaN fails both comparisons: miss)
        status.append(status_word(int(cs[k]), int(ee[k]), int(rc[k][2]), miss[k]))
    block = np.zeros(16, dtype=np.float64)
    block[:6] = res["out"].astype(np.float64)
    block[6] = inp.get("peer_fail", 0.0)
    block[8:10] = inp.get("jit", (0.0, 0.0))
    words = block[10:15].view(np.int32)
    for k in range(2):
        words[4 * k: 4 * k + 4] = (rc[k][0], (rc[k][1] & 0xff) | (nrank[k] << 8), rc[k][2], 0)
        words[8 + k] = status[k]
    block[15] = inp["theta"][5]
    res.update(nrank=nrank, miss=miss, status=status, block=block)
    return res


# ---- case builders ------------------------------------------------------------------------------------------------------------------
def rbf_like_spectrum(rho, decay=6.0, floor=1e-12):
    """Eigenvalues of G0: decay x per index down to floor (relative), level there: a factor 100 clear of the rank cut on its upper side."""
    k = np.arange(rho, dtype=float)
    return np.maximum(decay ** -k, floor * (1.0 + 0.5 ** k))


def make_dim(m, n, rho, r, seed, spectrum=None, rotate=True):
    """One dimension of a tail case: B0 = U diag(sigma) Wn^T (m x n, rank rho: the trailing eigenvalues of G0 = B0 B0^T are squares of
    B0's rounding, 1e-32 of the largest), random V0 (m x n) and symmetric Mk0; G0, H0 = V0 B0^T; V1: an orthonormal r x m basis that
    contains range(G0) (the columns of U, filled up with null directions when r > rho, then turned by a random rotation
    so that the Ritz vectors W are dense); the Ritz pairs of V1 G0 V1^T sorted decreasing (W: row j = vector j); AM = V1 Mk0 V1^T,
    AH = V1 H0 V1^T."""
    assert rho <= min(m, n) and rho <= r <= m
    rng = np.random.default_rng(seed)
    lam = rbf_like_spectrum(rho) if spectrum is None else np.asarray(spectrum, float)
    Uq = np.linalg.qr(rng.standard_normal((m, m)))[0][:, :rho]
    Wn = np.linalg.qr(rng.standard_normal((n, n)))[0][:, :rho]
    B0 = (Uq * np.sqrt(lam)) @ Wn.T
    V0 = rng.standard_normal((m, n)) / math.sqrt(n)
    Mk0 = rng.standard_normal((m, m)) / math.sqrt(m)
    Mk0 = 0.5 * (Mk0 + Mk0.T)
    G0, H0 = B0 @ B0.T, V0 @ B0.T
    G0 = 0.5 * (G0 + G0.T)
    # (U itself, not eigenvectors computed from G0: those mix a range direction at 1e-12 of the largest with the null space at 1e-4, and
    #  H0 = V0 B0^T sees what such a basis leaves out at the scale of sigma = 1e-6, not of sigma^2)
    V1 = np.linalg.qr(np.hstack([Uq, rng.standard_normal((m, r - rho))]))[0].T
    if rotate and r > 1:
        V1 = np.linalg.qr(rng.standard_normal((r, r)))[0] @ V1
    Hs = V1 @ G0 @ V1.T
    th, Wc = np.linalg.eigh(0.5 * (Hs + Hs.T))
    th, W = th[::-1].copy(), Wc[:, ::-1].T.copy()
    return dict(m=m, n=n, rho=rho, r=r, B0=B0, V0=V0, Mk0=Mk0, G0=G0, H0=H0, V1=V1, lam=th, W=W, AM=V1 @ Mk0 @ V1.T, AH=V1 @ H0 @ V1.T)


def tail_input(d1, d2, seed, theta=THETA, seq=7.0):
    """The tail's inputs of two make_dim() dimensions and white-noise data Y [n2][n1]; also what oracle.kron.finish needs."""
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((d2["n"], d1["n"]))
    C = d1["B0"] @ Y.T @ d2["B0"].T
    C1 = d1["V0"] @ Y.T @ d2["B0"].T
    C2 = d1["B0"] @ Y.T @ d2["V0"].T
    AC = np.stack([d1["V1"] @ Cq @ d2["V1"].T for Cq in (C, C1, C2)])
    return dict(theta=tuple(theta) + (seq,), N=float(Y.size), yy=float((Y * Y).sum()), m1=d1["m"], m2=d2["m"], W1=d1["W"], W2=d2["W"],
                lam1=d1["lam"], lam2=d2["lam"], AM1=d1["AM"], AH1=d1["AH"], AM2=d2["AM"], AH2=d2["AH"], AC=AC,
                dG1=np.diag(d1["G0"]).copy(), dH1=np.diag(d1["H0"]).copy(), dG2=np.diag(d2["G0"]).copy(), dH2=np.diag(d2["H0"]).copy(), Y=Y)


def oracle_finish(d1, d2, inp):
    """oracle.kron.finish on the DimStates of the same construction -> (elbo, grad [5])."""
    from oracle import kron as Kr
    s1, s2 = inp["theta"][2], inp["theta"][3]
    D1 = Kr.DimState(L=None, jit=0.0, B=math.sqrt(s1) * d1["B0"], V=math.sqrt(s1) * d1["V0"], Mk=d1["Mk0"])
    D2 = Kr.DimState(L=None, jit=0.0, B=math.sqrt(s2) * d2["B0"], V=math.sqrt(s2) * d2["V0"], Mk=d2["Mk0"])
    pay = Kr.local_partials(inp["Y"], D1, D2)
    st = Kr.finish(inp["theta"][:5], D1, D2, pay, int(inp["N"]))
    return st.elbo, st.grad


# (r1, r2, m1, m2, rho1, rho2, ac_nslab): every kk = ceil8(r) in {8, 16, 24, 32}, mp in {16, 32}, r1 < r2 and r1 > r2, m_d in
# {r_d, 33, 128, 255, 256}, rho = r (no margin) and rho < r, one slab and three
TAIL_R = ((1, 1), (1, 32), (7, 8), (8, 9), (16, 16), (16, 17), (17, 16), (22, 18), (24, 25), (32, 32), (32, 3))
TAIL_M = ("r", 33, 128, 255, 256)
TAIL_CASES = [
    (1, 1, 1, 33, 1, 1, 1), (1, 32, 128, 32, 1, 30, 3), (7, 8, 7, 255, 7, 6, 1), (8, 9, 256, 33, 5, 9, 3), (16, 16, 16, 128, 14, 16, 1),
    (16, 17, 255, 17, 16, 13, 3), (17, 16, 33, 256, 15, 14, 1), (22, 18, 128, 255, 18, 18, 3), (24, 25, 256, 25, 24, 21, 1),
    (32, 32, 32, 256, 32, 28, 3), (32, 3, 255, 3, 27, 3, 1), (16, 16, 128, 128, 12, 12, 1),
]


def tail_case(case):
    r1, r2, m1, m2, rho1, rho2, nslab = case
    seed = 1000 * r1 + 10 * r2 + nslab
    d1 = make_dim(m1, rho1 + 3, rho1, r1, seed)
    d2 = make_dim(m2, rho2 + 4, rho2, r2, seed + 1)
    return d1, d2, tail_input(d1, d2, seed + 2)


def split_slabs(AC, nslab, seed):
    """AC rounded to multiples of 2^-20 (entries below 2^20 in size) and split into nslab slabs of such multiples whose fixed-order
    float64 sum is the rounded AC bit for bit: -> (AC rounded, slabs [nslab][3][r1][r2])."""
    rng = np.random.default_rng(seed)
    q = 2.0 ** -20
    ACr = np.round(np.asarray(AC, np.float64) / q) * q
    assert np.abs(ACr).max() < 2.0 ** 20
    slabs = np.round(rng.uniform(-4, 4, (nslab,) + ACr.shape) / q) * q
    slabs[-1] = ACr - slabs[:-1].sum(0)
    tot = np.zeros_like(ACr)
    for s in slabs:
        tot = tot + s
    assert np.array_equal(tot, ACr)
    return ACr, slabs


# ---- sizes of the range finder and of the row QR ------------------------------------------------------------------------------------
PIV_M = (1, 2, 63, 64, 65, 96, 128, 255, 256)
PIV_R = (1, 2, 31, 32, 33, 64)
PIV_CASES = [(1, 1), (2, 1), (2, 2), (63, 31), (63, 33), (64, 64), (65, 2), (65, 33), (96, 32), (128, 64), (255, 31), (256, 64), (256, 33)]
ROWQR_THIN = tuple((r, m) for r in (1, 2, 3, 4, 5, 8, 16, 17, 18, 20, 22, 30, 32) for m in (r, 33, 128, 129, 256))
ROWQR_SUB = tuple((r, m) for r in (48, 62, 64) for m in (64, 127, 128))
ROWQR_CASES = ROWQR_THIN + ROWQR_SUB
ROWQR_KINDS = ("random", "graded", "leaky", "orthonormal")
ROWQR_CP = (0, 1, 16 * 1024 - 1, 16 * 1024, "rest")              # "rest" = (m - r) m, the complement rows of the subspace chain

# Worst |float64 - long double| / (u scale) of this file's own formulas over their cases (tests/test_thin_chain_spec.py measures them and
# holds them to these figures); the kernels get eight times as much.
RHO_SPEC = (1.6, 1.9, 1.7, 0.45, 0.45, 1.3)        # ELBO, d/d ell1, ell2, s1, s2, v
RHO_PIV = 0.75


def tie_chol_case():
    """Equal largest diagonals within a wave (rows 5 and 9) and in three different waves of the range finder (rows 5, 70, 200 of 256):
    the lowest index goes first, in the wave's butterfly and in the exchange between the waves."""
    G = np.diag(np.ones(256))
    for i in (5, 9, 70, 200):
        G[i, i] = 4.0
    return G, np.random.default_rng(11).standard_normal((4, 256))


def miss_input(inp, k, which, factor):
    """inp with diag G of dimension k set so that tr G - sum theta (scaled) sits at factor x threshold `which` (0: VG_THIN_MISS lam_max
    (m - r + 1), 1: the first-order ELBO term against VG_THIN_ELBO_TOL N), and N -- an input of its own -- moved so that the other
    threshold is a factor 100 further out."""
    out = dict(inp)
    t_abs, t_elbo = miss_thresholds(inp)[k]
    out["N"] = inp["N"] * (1e2 * t_abs / t_elbo if which == 0 else 1e-2 * t_abs / t_elbo)
    for d in range(2):              # both diagonals hold the Ritz values themselves: the traces differ from their sums by summation order only
        lam, m = inp["lam%d" % (d + 1)], inp["m%d" % (d + 1)]
        dG = np.zeros(m)
        dG[:len(lam)] = lam
        out["dG%d" % (d + 1)] = dG
    thr = miss_thresholds(out)[k][which]
    out["dG%d" % (k + 1)][0] += factor * thr / inp["theta"][2 + k]
    return out
