"""vggp_cholesky_inverse on every path and edge: the single-workgroup MFMA kernel (m <= 128, four jitter levels racing) and the
blocked path (m > 128, host jitter loop), at sizes around every 16-block and 128-panel boundary.

Integer-exact inputs (tests/dense_cases.py) are compared by equality; floating inputs against the componentwise limits of DESIGN.md
section 5b; the jitter ladder against the oracle at factor-3 margins; plus the lower-triangle-only contract, buffer placement, the
state left behind by VGGP_ENOTPD and the VGGP_EINVAL contract.  Every call goes through `chol`, which places K in a NaN-filled
parent and L, Linv in sentinel-filled parents and checks that nothing outside the windows changed."""
import ctypes as C

import numpy as np
import pytest
import torch

import dense_cases as dc
from variational_gridded_gaussian_processes_amd._lib import VGGP_EINVAL, VGGP_ENOTPD, VGGP_OK

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 67                 # odd: the windows are 8-byte but not 16-byte aligned
SENT = -777.25
ALL_SIZES = dc.CHOL_SMALL + dc.CHOL_BLOCKED


def bits(t):
    return t.contiguous().view(torch.int64)


def window(m, fill):
    parent = torch.full((2 * GUARD + m * m,), fill, dtype=torch.float64, device=DEV)
    return parent, parent[GUARD:GUARD + m * m].view(m, m)


def chol(engine, K):
    """-> rc, L, Linv, jitter (numpy); K numpy [m][m]."""
    m = K.shape[0]
    pk, wk = window(m, float("nan"))
    pl, wl = window(m, SENT)
    pi, wi = window(m, SENT)
    wk.copy_(torch.tensor(K, device=DEV))
    pk0 = bits(pk).clone()
    jit = C.c_double(123.0)
    rc = engine.lib.vggp_cholesky_inverse(engine._h, wk.data_ptr(), m, wl.data_ptr(), wi.data_ptr(), C.byref(jit),
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(bits(pk), pk0), "K or its surroundings were written"
    for p in (pl, pi):
        assert bool((p[:GUARD] == SENT).all()) and bool((p[GUARD + m * m:] == SENT).all()), "write outside the output window"
    return rc, wl.cpu().numpy(), wi.cpu().numpy(), jit.value


def nan_upper(K):
    Kn = K.copy()
    Kn[np.triu_indices(K.shape[0], 1)] = np.nan
    return Kn


def same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


def check_limits(tag, m, L, Li, Kj, Lref):
    """Componentwise limits kappa_b (m + 1) u of DESIGN.md 5b; prints the measured ratios (in units of (m + 1) u) and the reference's."""
    import scipy.linalg as sla
    kb = dc.kappa_blocks(Lref, 16 if m <= 128 else 128)
    unit = (m + 1) * dc.U
    r_f, r_i = dc.chol_ratio(L, Kj), dc.inv_ratio(L, Li)
    ref_f, ref_i = dc.chol_ratio(Lref, Kj), dc.inv_ratio(Lref, sla.solve_triangular(Lref, np.eye(m), lower=True))
    print(f"RATIO chol {tag} m={m} kappa_b={kb:.3g} LLt gpu={r_f / unit:.3g} ref={ref_f / unit:.3g} "
          f"LLinv gpu={r_i / unit:.3g} ref={ref_i / unit:.3g} [(m+1)u]")
    assert np.abs(np.triu(L, 1)).max(initial=0.0) == 0.0 and np.abs(np.triu(Li, 1)).max(initial=0.0) == 0.0
    assert r_f <= kb * unit and r_i <= kb * unit


@pytest.mark.parametrize("m", ALL_SIZES)
def test_integer_exact_two_level(engine, m):
    """L, Linv and K are integer: every path must return them exactly, at jitter 0 -- and read the lower triangle only."""
    Lx, Lix = dc.two_level_L(m, 0)
    K = Lx @ Lx.T
    rc, L, Li, jit = chol(engine, K)
    assert rc == VGGP_OK and jit == 0.0
    assert np.array_equal(L, Lx)
    assert np.array_equal(Li, Lix)
    rc2, L2, Li2, jit2 = chol(engine, nan_upper(K))
    assert rc2 == VGGP_OK and jit2 == 0.0 and same_bits(L2, L) and same_bits(Li2, Li)


@pytest.mark.parametrize("m", dc.CHOL_SMALL)
def test_integer_exact_dense_unit(engine, m):
    """Dense unit factor: the 16 x 16 diagonal-block inverses are integers below 2^15, the full inverse is not representable --
    L alone is compared."""
    Lx = dc.dense_unit_L(m, 0)
    rc, L, Li, jit = chol(engine, Lx @ Lx.T)
    assert rc == VGGP_OK and jit == 0.0 and np.array_equal(L, Lx)


@pytest.mark.parametrize("m", ALL_SIZES)
def test_floating_limits(engine, m):
    K = dc.spd_with_lmin(m, 3e-9, 0)
    Lref, jref = dc.chol_ladder(K)
    rc, L, Li, jit = chol(engine, K)
    assert rc == VGGP_OK and jit == jref == 0.0
    check_limits("lmin=+3e-9", m, L, Li, K, Lref)
    rc2, L2, Li2, jit2 = chol(engine, nan_upper(K))
    assert rc2 == VGGP_OK and jit2 == 0.0 and same_bits(L2, L) and same_bits(Li2, Li)


@pytest.mark.parametrize("m", ALL_SIZES)
def test_floating_limits_well_conditioned(engine, m):
    """K = fl(W W^T) of a well-conditioned W: kappa_b is 5 .. 15 for the 16-blocks and 40 .. 80 for the 128-blocks (against
    1e3 .. 1e6 with lambda_min = 3e-9), so the same limits sit two to three orders of magnitude above the kernels' measured error
    and not seven."""
    W = dc.well_conditioned_L(m, 3)
    K = W @ W.T
    K = 0.5 * (K + K.T)
    Lref, jref = dc.chol_ladder(K)
    rc, L, Li, jit = chol(engine, K)
    assert rc == VGGP_OK and jit == jref == 0.0
    check_limits("well-conditioned", m, L, Li, K, Lref)


@pytest.mark.parametrize("lmin,expect", dc.LADDER[:3])
@pytest.mark.parametrize("m", dc.LADDER_SIZES)
def test_jitter_ladder(engine, m, lmin, expect):
    """lambda_min = -3e-9 / -3e-8 / -3e-7: the first level that clears it wins, on the racing path and in the host loop."""
    K = dc.spd_with_lmin(m, lmin, 0)
    Lref, jref = dc.chol_ladder(K)
    rc, L, Li, jit = chol(engine, K)
    assert jref == expect
    assert rc == VGGP_OK and jit == jref
    check_limits(f"lmin={lmin:g}", m, L, Li, K + jit * np.eye(m), Lref)


@pytest.mark.parametrize("bad", ["lmin=-3e-6", "nan"])
@pytest.mark.parametrize("m", dc.LADDER_SIZES)
def test_not_pd_and_the_call_after(engine, m, bad):
    """Fall-through of the ladder (and an all-NaN K, where every level fails its first pivot): VGGP_ENOTPD, jitter -1, NaN outputs
    for m <= 128; the shared scratch flags are cleared -- the next valid call returns the bits of the same call made before."""
    Kgood = dc.spd_with_lmin(m, -3e-8, 1)
    Kbad = dc.spd_with_lmin(m, -3e-6, 0) if bad != "nan" else np.full((m, m), np.nan)
    if bad != "nan":
        assert dc.chol_ladder(Kbad)[1] == -1.0
    before = chol(engine, Kgood)
    rc, L, Li, jit = chol(engine, Kbad)
    assert rc == VGGP_ENOTPD and jit == -1.0
    assert b"not positive definite" in engine.lib.vggp_last_error()
    if m <= 128:
        assert np.isnan(L).all() and np.isnan(Li).all()
    after = chol(engine, Kgood)
    assert before[0] == after[0] == VGGP_OK and before[3] == after[3] == 1e-7
    assert same_bits(before[1], after[1]) and same_bits(before[2], after[2])


@pytest.mark.parametrize("m", [17, 128])
def test_level_flags_do_not_survive_a_call(engine, m):
    """The four racing workgroups of the m <= 128 path talk through four flag words in the shared scratch.  An all-NaN K leaves
    all four at `failed`; in the next call every level succeeds and finishes at the same moment, so a level that still sees its
    lower sibling's stale `failed` also declares itself the winner: jitter 1e-8 .. 1e-6 and a factor of K + jitter I.  Whether
    a stale word is seen is a matter of timing, hence the alternation: eight chances instead of one."""
    Lx, Lix = dc.two_level_L(m, 4)
    K = Lx @ Lx.T
    nan = np.full((m, m), np.nan)
    for _ in range(8):
        assert chol(engine, nan)[0] == VGGP_ENOTPD
        rc, L, Li, jit = chol(engine, K)
        assert rc == VGGP_OK and jit == 0.0 and np.array_equal(L, Lx) and np.array_equal(Li, Lix)


@pytest.mark.parametrize("m", [113, 257])
def test_bitwise_repeatable(engine, m):
    K = dc.spd_with_lmin(m, -3e-9, 2)
    first = chol(engine, K)
    assert first[0] == VGGP_OK and first[3] == 1e-8
    for _ in range(3):
        again = chol(engine, K)
        assert again[3] == first[3] and same_bits(again[1], first[1]) and same_bits(again[2], first[2])


def test_einval_contract(engine):
    """m outside [1, 8192] and NULL pointers are refused before any memory is touched (the buffers hold ONE element)."""
    buf = torch.full((3,), SENT, dtype=torch.float64, device=DEV)
    k, l, li = (buf[i:i + 1].data_ptr() for i in range(3))
    st = torch.cuda.current_stream().cuda_stream
    for args in ((k, 0, l, li), (k, -1, l, li), (k, 8193, l, li), (None, 4, l, li), (k, 4, None, li), (k, 4, l, None)):
        jit = C.c_double(123.0)
        assert engine.lib.vggp_cholesky_inverse(engine._h, args[0], args[1], args[2], args[3], C.byref(jit), st) == VGGP_EINVAL
        assert jit.value == 123.0
    assert engine.lib.vggp_cholesky_inverse(None, k, 1, l, li, None, st) == VGGP_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
    # jitter_out may be NULL
    buf[0] = 4.0
    assert engine.lib.vggp_cholesky_inverse(engine._h, k, 1, l, li, None, st) == VGGP_OK
    torch.cuda.synchronize()
    assert buf.tolist() == [4.0, 2.0, 0.5]
