"""CPU tests of tests/thin_chain_spec.py: the references of the thin chain's four kernels are pinned to oracle/kron.py and to long double,
so that tests/test_gpu_thin_chain_paths.py rests on the oracle and not on a transcription of the kernels.

Measured here (x86-64, numpy long double = 80 bit):
  tail, float64 spec against oracle.kron.finish on the twelve exact-rank cases: ELBO <= 2.1e-16 relative, gradient <= 5.5e-13 (d/d ell),
      3.7e-16 (d/d s, d/d v); caps 1e-13 / 1e-11.
  rho_spec = worst |float64 - long double| / (u abs-scale) of the tail over those cases, per component (ELBO, d/d ell1, ell2, s1, s2, v):
      1.50  1.81  1.69  0.42  0.43  1.24  -- recorded rounded up as thin_chain_spec.RHO_SPEC.
  pivchol, graded cases: same pivots in both precisions, smallest lead of a pivot 0.18; worst |float64 - long double| /
      ((i + 1) u scale) = 0.71 (RHO_PIV = 0.75); the exact-arithmetic cases are identical in both precisions bit for bit.
  row QR yardstick (float64 classical Gram-Schmidt, two passes, all 74 sizes): orthogonality, span and order all below 0.02 of the
      floor 64 m u on every family of inputs -- the floor is the cap everywhere."""
import itertools

import numpy as np
import pytest

import thin_chain_spec as S

TAIL_IDS = ["r%dx%d-m%dx%d-rho%dx%d-slab%d" % c for c in S.TAIL_CASES]


@pytest.fixture(scope="module")
def tails():
    out = {}
    for c in S.TAIL_CASES:
        d1, d2, inp = S.tail_case(c)
        out[c] = (d1, d2, inp, S.thin_tail(inp, np.float64), S.thin_tail(inp, np.longdouble))
    return out


def test_every_size_is_used():
    assert {(c[0], c[1]) for c in S.TAIL_CASES} == set(S.TAIL_R)
    for c in S.TAIL_CASES:
        assert c[4] <= c[0] <= min(c[2], 32) and c[5] <= c[1] <= min(c[3], 32)
    ms = {("r" if m == r else m) for c in S.TAIL_CASES for r, m in ((c[0], c[2]), (c[1], c[3]))}
    assert ms == set(S.TAIL_M)
    assert {c[6] for c in S.TAIL_CASES} == {1, 3}
    assert {((max(c[0], c[1]) + 7) // 8) * 8 for c in S.TAIL_CASES} == {8, 16, 24, 32}
    assert {((max(c[0], c[1]) + 15) // 16) * 16 for c in S.TAIL_CASES} == {16, 32}
    assert any(c[4] == c[0] and c[5] == c[1] for c in S.TAIL_CASES) and any(c[4] < c[0] for c in S.TAIL_CASES)   # no margin / a margin
    assert {m for m, r in S.PIV_CASES} == set(S.PIV_M) and {r for m, r in S.PIV_CASES} == set(S.PIV_R)
    assert all(r <= m for m, r in S.PIV_CASES)
    assert {r for r, m in S.ROWQR_CASES} == {1, 2, 3, 4, 5, 8, 16, 17, 18, 20, 22, 30, 32, 48, 62, 64}
    assert all(r <= m <= 256 for r, m in S.ROWQR_CASES) and any(r % 4 for r, m in S.ROWQR_CASES)
    assert {r for r, hk, sp, al in S.RITZ_CASES} == set(S.RITZ_R)
    assert {("r" if hk == r else hk) for r, hk, sp, al in S.RITZ_CASES} | {33} == set(S.RITZ_HK)
    assert {hk for r, hk, sp, al in S.RITZ_CASES} >= {33, 127, 128, 129, 200, 256}
    assert {sp for r, hk, sp, al in S.RITZ_CASES} == set(S.RITZ_SPECTRA)
    # staged (r <= 48 and hk <= 128) or not, nearly diagonal (Newton start) or dense (fallback): all four; r > 48: neither
    combos = {(r <= 48 and hk <= 128, al) for r, hk, sp, al in S.RITZ_CASES if r <= 48}
    assert combos == set(itertools.product((True, False), (True, False)))
    assert any(r > 48 for r, hk, sp, al in S.RITZ_CASES)


@pytest.mark.parametrize("case", S.TAIL_CASES, ids=TAIL_IDS)
def test_tail_spec_reproduces_the_oracle(tails, case):
    """The float64 spec against oracle.kron.finish of the same DimStates: ELBO 1e-13, every gradient component 1e-11, relative; the miss
    check is silent, the ranks are the constructed ones."""
    d1, d2, inp, f64, ld = tails[case]
    elbo, grad = S.oracle_finish(d1, d2, inp)
    print("ELBO", abs(f64["out"][0] - elbo) / abs(elbo), "grad", np.abs(f64["out"][1:] - grad) / np.abs(grad))
    assert abs(f64["out"][0] - elbo) <= 1e-13 * abs(elbo)
    assert np.all(np.abs(f64["out"][1:] - grad) <= 1e-11 * np.abs(grad))
    assert f64["miss"] == [False, False] and f64["status"] == [0, 0]
    assert f64["nrank"] == [case[4], case[5]] == ld["nrank"]
    for k in range(2):
        assert abs(f64["trG"][k] - f64["sth"][k]) <= 9e-16 * max(1.0, f64["trG"][k])
    # spectra a factor 10 clear of the rank cut
    for lam in (inp["lam1"], inp["lam2"]):
        rel = np.abs(lam) / lam[0]
        assert not np.any((rel > 0.1 * S.VG_EIG_RANK_CUT) & (rel < 10 * S.VG_EIG_RANK_CUT))


def test_float64_spec_against_long_double(tails):
    worst = np.zeros(6)
    for c in S.TAIL_CASES:
        f64, ld = tails[c][3], tails[c][4]
        worst = np.maximum(worst, np.array(np.abs(f64["out"].astype(S.LD) - ld["out"]) / (S.U * ld["abs"]), dtype=float))
        for key in ("beta", "invd"):
            err = np.abs(f64[key].astype(S.LD) - ld[key]) / (S.U * ld[key + "_abs"])
            assert float(err.max()) <= 64 * max(c[0], c[1])
        assert np.array_equal(f64["block"][6:], ld["block"][6:])          # the packed words do not depend on the precision
    print("rho_spec", worst)
    assert np.all(worst <= np.array(S.RHO_SPEC)), worst
    assert np.all(worst >= 0.5 * np.array(S.RHO_SPEC)), worst             # (the recorded figures are the measured ones, not slack)


def test_status_precedence_table():
    """status[k]: Cholesky status, then the Ritz solve's status, then VGGP_ENOCONV, then VG_ESUBMISS, then 0 -- through the spec's block."""
    d1, d2, inp = S.tail_case(S.TAIL_CASES[2])
    for chol, rstat, err, k in itertools.product((0, -2), (0, -6), (0, 1, 2, 3), (0, 1)):
        for miss in (False, True):
            i2 = dict(inp)
            cs, ee, rc = [0, 0], [0, 0], np.zeros((2, 4), dtype=np.int32)
            cs[k], ee[k], rc[k][2] = chol, err, rstat
            rc[k][0], rc[k][1] = 17, 5 | (9 << 8)
            i2.update(chol_status=cs, eig_err=ee, rcounters=rc, jit=(1e-8, 0.0), peer_fail=3.0)
            if miss:
                i2["lam%d" % (k + 1)] = inp["lam%d" % (k + 1)] * 0.5
            res = S.thin_tail(i2)
            want = chol if chol else rstat if rstat else S.VGGP_ENOCONV if err & 1 else S.VG_ESUBMISS if (miss or err & 2) else 0
            words = res["block"][10:15].view(np.int32)
            assert res["miss"][k] == miss and res["status"][k] == want == words[8 + k]
            assert res["status"][1 - k] == 0 == words[9 - k]
            assert list(words[4 * k: 4 * k + 4]) == [17, 5 | (res["nrank"][k] << 8), rstat, 0]
            assert res["block"][6] == 3.0 and res["block"][7] == 0.0 and res["block"][8] == 1e-8 and res["block"][15] == inp["theta"][5]


def test_miss_thresholds():
    """tr G - sum theta at 0.1 x and 10 x each of the two thresholds, the other one far away: silent below, a miss above; NaN is a miss."""
    d1, d2, inp = S.tail_case(S.TAIL_CASES[4])
    for k, which in itertools.product((0, 1), (0, 1)):
        for factor, want in ((0.1, False), (10.0, True)):
            i2 = S.miss_input(inp, k, which, factor)
            res = S.thin_tail(i2)
            assert res["miss"][k] == want and res["miss"][1 - k] is False, (k, which, factor)
            assert res["status"][k] == (S.VG_ESUBMISS if want else 0)
    for k in (0, 1):
        i2 = dict(inp)
        lam = inp["lam%d" % (k + 1)].copy()
        lam[-1] = np.nan
        i2["lam%d" % (k + 1)] = lam
        assert S.thin_tail(i2)["miss"][k] is True


@pytest.mark.parametrize("m,r", S.PIV_CASES)
def test_pivchol_spec(m, r):
    G, Om = S.graded_chol_case(m, r, 100 * m + r)
    V, piv, lead, scale = S.pivchol(G, Om, r)
    Vl, pivl, leadl, scalel = S.pivchol(G.astype(S.LD), Om.astype(S.LD), r)
    assert piv == pivl and min(piv) >= 0 and len(set(piv)) == r
    assert min(lead) >= 1e-3 and min(leadl) >= 1e-3                        # determinate pivots
    steps = np.arange(1, r + 1)[:, None]
    rho = float((np.abs(V.astype(S.LD) - Vl) / (steps * S.U * scalel)).max())
    print("rho_piv", rho)
    assert rho <= S.RHO_PIV
    # exact arithmetic: identical in both precisions, L^T then rows of Omega
    rank = min(r - 1, 20)
    G, Om, L, perm = S.exact_chol_case(m, r, rank, m + r)
    V, piv, _, _ = S.pivchol(G, Om, r)
    Vl = S.pivchol(G.astype(S.LD), Om.astype(S.LD), r)[0]
    assert np.array_equal(V, Vl.astype(np.float64)) and np.array_equal(Vl, V.astype(S.LD))
    assert np.array_equal(V[:rank], L.T) and np.array_equal(V[rank:], Om[rank:])
    assert piv == list(perm[:rank]) + [-1] * (r - rank)


def test_pivchol_tie_goes_to_the_lowest_index():
    G, Om = S.tie_chol_case()
    V, piv, _, _ = S.pivchol(G, Om, 4)
    assert piv == [5, 9, 70, 200] and np.array_equal(V[0], 2.0 * np.eye(256)[5])


@pytest.mark.parametrize("kind", S.ROWQR_KINDS)
def test_rowqr_yardstick(kind):
    """The float64 two-pass Gram-Schmidt stays below the floor 64 m u on every size: the floor is the kernel's cap everywhere."""
    worst = np.zeros(3)
    for r, m in S.ROWQR_CASES:
        Z = S.rowqr_input(kind, r, m, 1000 * r + m)
        orth, span, upper, mind = S.rowqr_checks(Z, S.cgs2(Z))
        worst = np.maximum(worst, np.array([orth, span, upper]) / (64 * m * S.U))
        assert mind > 0
    print(kind, worst)
    assert np.all(8 * worst <= 1.0)


def test_leaky_rows_force_the_second_pass():
    """From the fourth row on, projecting a row of the 'leaky' input off the rows before it removes more than half of its squared norm."""
    Z = S.rowqr_input("leaky", 32, 128, 32128)
    V = S.cgs2(Z)
    for k in range(4, 32):
        c = V[:k] @ Z[k]
        assert (c @ c) > 0.5 * (Z[k] @ Z[k])
    Z = S.rowqr_input("orthonormal", 32, 128, 32128)
    assert np.abs(Z @ Z.T - np.eye(32)).max() < 1e-14


@pytest.mark.parametrize("r,hk,spectrum,aligned", S.RITZ_CASES)
def test_ritz_cases_stay_clear_of_the_rank_cut(r, hk, spectrum, aligned):
    Hl, Hr, lam = S.ritz_case(r, hk, spectrum, aligned, 1000 * r + hk)
    th = S.ritz_ref(Hl, Hr)
    rel = np.abs(th) / th[0]
    assert np.all(np.diff(th) <= 0)
    assert not np.any((rel > 0.1 * S.VG_EIG_RANK_CUT) & (rel < 10 * S.VG_EIG_RANK_CUT))
    assert int(np.sum(rel > S.VG_EIG_RANK_CUT)) == int(np.sum(lam > 0))
    H = S.ritz_matrix(Hl, Hr)
    off = np.abs(H - np.diag(np.diag(H))).max()
    assert (off < 5e-3 * th[0]) if aligned else (r < 3 or off > 5e-2 * th[0])
    # the premise of "the Newton start must be taken" / "must decline" (it declines at a quotient of 0.3)
    nq = S.newton_quotient(H)
    print("newton quotient", r, hk, spectrum, aligned, nq)
    if aligned and spectrum == "decay":
        assert nq < 0.03
    if not aligned and r >= 8:
        assert nq > 3.0


def test_split_slabs_sum_bitwise():
    AC = np.random.default_rng(3).standard_normal((3, 7, 8)) * 30
    ACr, slabs = S.split_slabs(AC, 3, 5)
    assert np.abs(ACr - AC).max() <= 2.0 ** -21 and slabs.shape == (3, 3, 7, 8)
    assert np.array_equal((slabs[0] + slabs[1]) + slabs[2], ACr)
