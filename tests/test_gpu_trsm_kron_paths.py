"""vggp_trsm and vggp_kron_solve on every path and edge.

trsm: every template instance of the strip kernel (NB = 1, 2, 4, 8 for m <= 16, 32, 64, 128), sizes that leave identity-extension
rows inside an instance, the blocked path beyond 128 (GEMM update + strip kernel per 128-block row), column counts around the
16-column strip and the 64-column workgroup, both orientations.  kron_solve: the all-substitution path (both factors <= 128: four
in-place solves, two of them on the transposed view), the inverse-forming path (block doubling, 1-row blocks at n = 129), and the
two A/B switches, each in a fresh child process.

Integer-exact inputs (tests/dense_cases.py) are compared by equality, floating ones against the componentwise backward-error limit
of DESIGN.md section 5b (trsm) and the oracle (kron_solve).  Factors sit in NaN-filled parents with NaN above the diagonal, right-hand
sides in NaN-filled parents, results in sentinel-filled parents; nothing outside the windows may change."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dense_cases as dc
from oracle import kron as Kr
from variational_gridded_gaussian_processes_amd._lib import VGGP_EINVAL, VGGP_ENOTPD, VGGP_OK

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -777.25
HERE = os.path.dirname(os.path.abspath(__file__))


def bits(t):
    return t.contiguous().view(torch.int64)


def place(A, fill, guard):
    """A (numpy, 2-D) as a contiguous window of a `fill`-filled parent -> parent, window."""
    n = A.size
    parent = torch.full((2 * guard + n,), fill, dtype=torch.float64, device=DEV)
    w = parent[guard:guard + n].view(*A.shape)
    w.copy_(torch.tensor(A, device=DEV))
    return parent, w


def guards_hold(parent, guard, n, fill):
    g = torch.cat([parent[:guard], parent[guard + n:]])
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def nan_upper(L):
    Ln = L.copy()
    Ln[np.triu_indices(L.shape[0], 1)] = np.nan
    return Ln


def trsm(engine, L, R, trans, guard, alias=False):
    """X = op(L)^-1 R through the C ABI with guarded buffers -> numpy X."""
    m, ncols = R.shape
    nan = float("nan")
    pl, wl = place(L, nan, guard)
    pr, wr = place(R, nan, guard)
    px, wx = (pr, wr) if alias else place(np.zeros_like(R), SENT, guard)
    if not alias:
        wx.fill_(SENT)
    pl0, pr0 = bits(pl).clone(), bits(pr).clone()
    rc = engine.lib.vggp_trsm(engine._h, wl.data_ptr(), m, wr.data_ptr(), ncols, wx.data_ptr(), 1 if trans else 0,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == VGGP_OK, engine.lib.vggp_last_error()
    assert torch.equal(bits(pl), pl0), "L or its surroundings were written"
    if alias:
        assert guards_hold(pr, guard, R.size, nan)
    else:
        assert torch.equal(bits(pr), pr0), "R or its surroundings were written"
        assert guards_hold(px, guard, R.size, SENT), "write outside X"
    return wx.cpu().numpy()


def kron(engine, L1, L2, Y, guard=64, alias=False):
    n1, n2 = Y.shape
    nan = float("nan")
    p1, w1 = place(L1, nan, guard)
    p2, w2 = place(L2, nan, guard)
    py, wy = place(Y, nan, guard)
    px, wx = (py, wy) if alias else place(np.zeros_like(Y), SENT, guard)
    if not alias:
        wx.fill_(SENT)
    b1, b2, by = bits(p1).clone(), bits(p2).clone(), bits(py).clone()
    rc = engine.lib.vggp_kron_solve(engine._h, w1.data_ptr(), n1, w2.data_ptr(), n2, wy.data_ptr(), wx.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == VGGP_OK, engine.lib.vggp_last_error()
    assert torch.equal(bits(p1), b1) and torch.equal(bits(p2), b2), "a factor or its surroundings were written"
    if alias:
        assert guards_hold(py, guard, Y.size, nan)
    else:
        assert torch.equal(bits(py), by), "Y or its surroundings were written"
        assert guards_hold(px, guard, Y.size, SENT), "write outside X"
    return wx.cpu().numpy()


# ---- trsm ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [False, True], ids=["L", "Lt"])
@pytest.mark.parametrize("m", dc.TRSM_SIZES)
def test_trsm_integer_exact(engine, m, trans):
    """dense_unit_L, X integer in [-8, 8], R = op(L) X in int64: the solve returns X exactly.  The factor carries NaN above its
    diagonal (the header: the upper part is not read).  16-byte aligned windows: the vector staging loads of even m."""
    L = dc.dense_unit_L(m, 0)
    A = L.astype(np.int64)
    for ncols in dc.trsm_ncols(m):
        X = dc.int_rhs((m, ncols), m)
        R = ((A.T if trans else A) @ X.astype(np.int64)).astype(np.float64)
        got = trsm(engine, nan_upper(L), R, trans, guard=64)
        assert np.array_equal(got, X), (m, ncols)


@pytest.mark.parametrize("trans", [False, True], ids=["L", "Lt"])
@pytest.mark.parametrize("m", dc.TRSM_SIZES)
def test_trsm_backward_error(engine, m, trans):
    """well_conditioned_L: componentwise backward error omega <= kappa16 m u.  Windows at an odd offset (8-byte
    alignment only: the scalar staging loads)."""
    import scipy.linalg as sla
    L = dc.well_conditioned_L(m, 0)
    k16 = dc.kappa_blocks(L, 16)
    for ncols in dc.trsm_ncols(m):
        R = np.random.default_rng(m).standard_normal((m, ncols))
        X = trsm(engine, nan_upper(L), R, trans, guard=67)
        om = dc.trsm_omega(L, X, R, trans)
        ref = dc.trsm_omega(L, sla.solve_triangular(L, R, lower=True, trans=1 if trans else 0), R, trans)
        print(f"RATIO trsm m={m} ncols={ncols} trans={int(trans)} kappa16={k16:.3g} gpu={om / (m * dc.U):.3g} ref={ref / (m * dc.U):.3g} [m u]")
        assert om <= k16 * m * dc.U, (m, ncols)


@pytest.mark.parametrize("trans", [False, True], ids=["L", "Lt"])
@pytest.mark.parametrize("m,ncols", [(100, 65), (257, 63)])
def test_trsm_in_place(engine, m, ncols, trans):
    L = dc.dense_unit_L(m, 1)
    A = L.astype(np.int64)
    X = dc.int_rhs((m, ncols), m + 7)
    R = ((A.T if trans else A) @ X.astype(np.int64)).astype(np.float64)
    assert np.array_equal(trsm(engine, nan_upper(L), R, trans, guard=64, alias=True), X)


def test_trsm_einval_contract(engine):
    buf = torch.full((3,), SENT, dtype=torch.float64, device=DEV)
    l, r, x = (buf[i:i + 1].data_ptr() for i in range(3))
    st = torch.cuda.current_stream().cuda_stream
    for args in ((l, 0, r, 1, x), (l, 1, r, 0, x), (l, 16385, r, 1, x), (l, -3, r, 1, x), (None, 1, r, 1, x), (l, 1, None, 1, x),
                 (l, 1, r, 1, None)):
        assert engine.lib.vggp_trsm(engine._h, *args, 0, st) == VGGP_EINVAL
    assert engine.lib.vggp_trsm(None, l, 1, r, 1, x, 0, st) == VGGP_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


# ---- kron_solve ----------------------------------------------------------------------------------------------------------------
kron_int_case = dc.kron_int_case


@pytest.mark.parametrize("n1,n2", dc.KRON_SMALL + dc.KRON_LARGE)
def test_kron_integer_exact(engine, n1, n2):
    """Y = K1 X K2^T in int64 with integer factors whose inverses are integer too (tree_L): X comes back exactly on either path;
    dense unit factors as well where all four solves are substitutions."""
    L1, L2, X, Y = kron_int_case(n1, n2, tree=True)
    assert np.array_equal(kron(engine, nan_upper(L1), nan_upper(L2), Y), X)
    if max(n1, n2) <= 128:
        L1, L2, X, Y = kron_int_case(n1, n2, tree=False)
        assert np.array_equal(kron(engine, nan_upper(L1), nan_upper(L2), Y, guard=67), X)


@pytest.mark.parametrize("n1,n2", dc.KRON_SMALL + dc.KRON_LARGE)
def test_kron_vs_oracle(engine, n1, n2):
    """well_conditioned_L factors, asymmetric data, n1 != n2: relative error against the oracle below 1e-9 and the residual
    K1 X K2^T - Y within 20 x the oracle's own (floored at 1e-12) -- the criteria of test_gpu_blocks.test_kron_solve."""
    L1, L2 = dc.well_conditioned_L(n1, 1), dc.well_conditioned_L(n2, 2)
    Y = np.random.default_rng(n1 * 1000 + n2).standard_normal((n1, n2))
    X = kron(engine, nan_upper(L1), nan_upper(L2), Y)
    ref = Kr.kron_solve(L1, L2, Y)
    K1, K2 = L1 @ L1.T, L2 @ L2.T
    err = np.abs(X - ref).max() / np.abs(ref).max()
    r_gpu, r_ref = np.abs(K1 @ X @ K2.T - Y).max(), np.abs(K1 @ ref @ K2.T - Y).max()
    print(f"RATIO kron n1={n1} n2={n2} rel_err={err:.3g} resid gpu={r_gpu:.3g} ref={r_ref:.3g}")
    assert err < 1e-9
    assert r_gpu < 1e-9 * np.abs(X).max() and r_gpu < 20 * max(r_ref, 1e-12)


@pytest.mark.parametrize("n1,n2", [(100, 128), (113, 31), (129, 96), (257, 130)])
def test_kron_in_place(engine, n1, n2):
    L1, L2, X, Y = kron_int_case(n1, n2, tree=True)
    assert np.array_equal(kron(engine, nan_upper(L1), nan_upper(L2), Y, alias=True), X)


def poison_workspace(engine, m=300):
    """An all-NaN K on the blocked Cholesky path fails at every level and leaves NaN all over the context's shared scratch (its
    working copy of K, the diagonal-block inverses, the panel products): what the next call finds where it never writes."""
    K = torch.full((m, m), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.empty(2, m, m, dtype=torch.float64, device=DEV)
    rc = engine.lib.vggp_cholesky_inverse(engine._h, K.data_ptr(), m, out[0].data_ptr(), out[1].data_ptr(), None,
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == VGGP_ENOTPD


@pytest.mark.parametrize("n1,n2", [(17, 33), (129, 96), (96, 129), (257, 130)])
def test_kron_ignores_stale_scratch(engine, n1, n2):
    """The inverse-forming path never clears its scratch: the 128-blocks of the explicit inverses above the diagonal are neither
    written nor read (a 128 x 1 block at n = 129).  With NaN left there by an earlier call the result must not change."""
    L1, L2, X, Y = kron_int_case(n1, n2, tree=True)
    before = kron(engine, L1, L2, Y)
    poison_workspace(engine)
    after = kron(engine, L1, L2, Y)
    assert np.array_equal(before, X) and np.array_equal(after, X)
    Lw1, Lw2 = dc.well_conditioned_L(n1, 1), dc.well_conditioned_L(n2, 2)
    poison_workspace(engine)
    a = kron(engine, Lw1, Lw2, Y)
    b = kron(engine, Lw1, Lw2, Y)                   # (the scratch now holds the previous solve's own leftovers)
    assert np.isfinite(a).all() and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_kron_einval_contract(engine):
    buf = torch.full((4,), SENT, dtype=torch.float64, device=DEV)
    l1, l2, y, x = (buf[i:i + 1].data_ptr() for i in range(4))
    st = torch.cuda.current_stream().cuda_stream
    for args in ((l1, 0, l2, 1, y, x), (l1, 1, l2, 0, y, x), (l1, 16385, l2, 1, y, x), (l1, 1, l2, 16385, y, x),
                 (None, 1, l2, 1, y, x), (l1, 1, None, 1, y, x), (l1, 1, l2, 1, None, x), (l1, 1, l2, 1, y, None)):
        assert engine.lib.vggp_kron_solve(engine._h, *args, st) == VGGP_EINVAL
    assert engine.lib.vggp_kron_solve(None, l1, 1, l2, 1, y, x, st) == VGGP_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


# ---- A/B switches: read once per process, so each gets one fresh child ----------------------------------------------------------
def child_main():
    """Runs in the child: the integer-exact Kronecker cases at the two large shapes, on whatever path the environment selects."""
    from variational_gridded_gaussian_processes_amd import Engine
    engine = Engine(0)
    poison_workspace(engine)
    for n1, n2 in ((129, 96), (257, 130)):
        L1, L2, X, Y = kron_int_case(n1, n2, tree=True)
        for alias in (False, True):
            got = kron(engine, nan_upper(L1), nan_upper(L2), Y, alias=alias)
            assert np.array_equal(got, X), (n1, n2, alias, float(np.abs(got - X).max()))
    print("child ok")


@pytest.mark.parametrize("switch", ["VGGP_KRON_SUBST", "VGGP_KRON_FOUR"])
def test_kron_ab_switches_compute_the_same(switch):
    """A baseline switch that computes something else misleads every A/B timing made with it."""
    env = dict(os.environ)
    env[switch] = "1"
    driver = (f"import sys; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; "
              "import test_gpu_trsm_kron_paths as T; T.child_main()")
    flags = ["-s"] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable, *flags, "-c", driver], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, (p.returncode, p.stdout[-400:], p.stderr[-1500:])
