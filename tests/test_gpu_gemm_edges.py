"""vggp_gemm at the edges of its three kernels (csrc/gemm.hip vg_gemm_launch): the 32 x 32 small tile (< 128 tiles of 64 x 64
and K <= 512), the 64 x 64 x 32 deep-stage tile (>= 128 whole tiles, K % 32 == 0, each operand unit-stride along one axis with
an even leading dimension and a 16-byte aligned base) and the generic 64 x 64 x 16 tile (everything else).

Every case runs on two kinds of data:
  * integers in [-8, 8]: every product and partial sum is an integer below 2^53, so the fp64 result is exact and is compared with
    an int64 product by equality -- a dropped, duplicated or misrouted k-tile or fragment cannot hide behind a tolerance;
  * asymmetric random data against the ELEMENTWISE forward bound |err_ij| <= K 2^-52 (|A| |B|)_ij (2^-52 = 2u: one u K (|A||B|)
    for the kernel's sum in any order, one for the float64 reference's), never a max-norm.
Operands that are views live in parents filled with NaN, C windows in parents filled with a sentinel."""
import numpy as np
import pytest
import torch

from variational_gridded_gaussian_processes_amd._lib import VGGP_EINVAL, VGGP_OK

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -52
SENTINEL = -777.25


def values(M, N, K, integer, seed=0):
    g = torch.Generator(device="cpu").manual_seed(1000 * M + 10 * N + K + seed)
    if integer:
        return (torch.randint(-8, 9, (M, K), generator=g).double(), torch.randint(-8, 9, (K, N), generator=g).double())
    return torch.randn(M, K, generator=g, dtype=torch.float64), torch.randn(K, N, generator=g, dtype=torch.float64)


def place(X, order="r", pad=0, off=0):
    """A GPU view holding the values of the CPU matrix X: row-major ("r") or column-major ("c") storage with leading dimension
    extent + pad, starting `off` doubles into its parent allocation; the parent is NaN wherever the view does not reach."""
    S = X if order == "r" else X.t()
    rows, cols = S.shape
    ld = cols + pad
    parent = torch.full((off + rows * ld,), float("nan"), dtype=torch.float64, device=DEV)
    view = parent[off:off + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(S)
    return view if order == "r" else view.t()


def check(engine, a, b, A, B, integer, what=""):
    """engine.gemm(a, b) for the device views a, b of the CPU values A, B"""
    out = engine.gemm(a, b).cpu()
    assert out.shape == (A.shape[0], B.shape[1])
    assert bool(torch.isfinite(out).all()), what
    if integer:
        ref = (A.long() @ B.long()).double()
        assert torch.equal(out, ref), (what, int((out != ref).sum()))
    else:
        ref, bound = A @ B, A.shape[1] * U * (A.abs() @ B.abs())
        worst = float(((out - ref).abs() / bound).max())
        assert worst <= 1.0, (what, worst)
    return out


ORDERS = [("r", "r"), ("r", "c"), ("c", "r"), ("c", "c")]
# name: (M, N, K, kwargs of place() for A, for B)
DISPATCH = {
    "deep_128_tiles": (512, 1024, 64, {}, {}),
    "deep_broken_base_A": (512, 1024, 64, dict(off=1), {}),
    "deep_broken_base_B": (512, 1024, 64, {}, dict(off=1)),
    "deep_broken_odd_ld_A": (512, 1024, 64, dict(pad=1), {}),        # parents of row length 65 / 513
    "deep_broken_odd_ld_B": (512, 1024, 64, {}, dict(pad=1)),        # parents of row length 1025 / 65
    "deep_broken_K48": (512, 1024, 48, {}, {}),
    "deep_broken_M513": (513, 1024, 64, {}, {}),
    "deep_broken_N1000": (512, 1000, 64, {}, {}),
    "deep_ld_larger_than_extent": (512, 1024, 64, dict(pad=8), dict(pad=6)),      # still qualifies: sub-matrix views on the deep tile
    "generic_ragged_128_tiles": (513, 1000, 50, {}, {}),
    "generic_ragged_views": (513, 1000, 50, dict(pad=7, off=3), dict(pad=5, off=1)),
    "small_tile": (33, 31, 511, {}, {}),
    "small_tile_views": (33, 31, 511, dict(pad=7, off=1), dict(pad=3, off=5)),
    "boundary_K512_small": (64, 64, 512, {}, {}),
    "boundary_K513_generic": (64, 64, 513, {}, {}),
    "K1_generic": (1024, 1024, 1, {}, {}),
    "one_by_one": (1, 1, 1, {}, {}),
}


@pytest.mark.parametrize("integer", [True, False], ids=["int", "rand"])
@pytest.mark.parametrize("name", list(DISPATCH))
def test_gemm_dispatch_edges(engine, name, integer):
    """One shape per dispatch decision, all four operand orientations."""
    M, N, K, ka, kb = DISPATCH[name]
    A, B = values(M, N, K, integer)
    for oa, ob in ORDERS:
        check(engine, place(A, oa, **ka), place(B, ob, **kb), A, B, integer, (name, oa, ob))


@pytest.mark.parametrize("integer", [True, False], ids=["int", "rand"])
@pytest.mark.parametrize("M,N,K", [(70, 45, 37), (513, 1000, 50)], ids=["small", "generic"])
def test_gemm_both_strides_non_unit(engine, M, N, K, integer):
    """P[::2, ::3] views (and their transposes): neither stride of an operand is 1; the skipped elements are NaN."""
    A, B = values(M, N, K, integer)

    def strided(X):
        P = torch.full((2 * X.shape[0], 3 * X.shape[1]), float("nan"), dtype=torch.float64, device=DEV)
        P[::2, ::3] = X.to(DEV)
        return P[::2, ::3]

    a, b = strided(A), strided(B)
    assert a.stride() == (6 * K, 3) and b.stride() == (6 * N, 3)
    check(engine, a, b, A, B, integer, "rows")
    check(engine, strided(A.t()).t(), strided(B.t()).t(), A, B, integer, "columns")


@pytest.mark.parametrize("integer", [True, False], ids=["int", "rand"])
@pytest.mark.parametrize("which", ["A_rows", "A_cols", "B_rows", "B_cols"])
@pytest.mark.parametrize("M,N,K", [(33, 31, 40), (512, 1024, 64), (513, 1000, 50)], ids=["small", "deep", "generic"])
def test_gemm_stride_zero(engine, M, N, K, which, integer):
    """torch.expand views (stride 0) on each operand in turn.  (An expanded row of a K-contiguous operand has leading dimension
    0 -- even -- so the 512 x 1024 x 64 product still qualifies for the deep tile.)"""
    A, B = values(M, N, K, integer, seed=3)
    a, b = A.to(DEV), B.to(DEV)
    op, mode = which.split("_")

    def ex(X):
        return X[:1].expand_as(X) if mode == "rows" else X[:, :1].expand_as(X)

    if op == "A":
        A, a = ex(A), ex(a)
    else:
        B, b = ex(B), ex(b)
    assert 0 in (a.stride() + b.stride())
    check(engine, a, b, A.contiguous(), B.contiguous(), integer, which)


@pytest.mark.parametrize("M,N,K", [(33, 31, 511), (512, 1024, 64), (513, 1000, 50)], ids=["small", "deep", "generic"])
def test_gemm_ldc_window_keeps_its_surroundings(engine, M, N, K):
    """C is an interior M x N window of a sentinel-filled [M + 2][N + 3] parent (ldc = N + 3 > N, base an odd number of doubles
    into the parent, hence not 16-byte aligned): the window holds the exact product and every other element keeps the sentinel."""
    A, B = values(M, N, K, True, seed=5)
    a, b = A.to(DEV), B.to(DEV)
    parent = torch.full((M + 2, N + 3), SENTINEL, dtype=torch.float64, device=DEV)
    c0 = 1 if N % 2 else 2                               # (N + 3) + c0 odd
    win = parent[1:M + 1, c0:c0 + N]
    assert (win.data_ptr() - parent.data_ptr()) // 8 % 2 == 1 and win.data_ptr() % 16 == 8
    rc = engine.lib.vggp_gemm(engine._h, a.data_ptr(), a.stride(0), a.stride(1), b.data_ptr(), b.stride(0), b.stride(1),
                              win.data_ptr(), N + 3, M, N, K, torch.cuda.current_stream().cuda_stream)
    assert rc == VGGP_OK
    torch.cuda.synchronize()
    expect = torch.full((M + 2, N + 3), SENTINEL, dtype=torch.float64)
    expect[1:M + 1, c0:c0 + N] = (A.long() @ B.long()).double()
    assert torch.equal(parent.cpu(), expect)


def test_gemm_contract(engine):
    """VGGP_EINVAL for ldc < N, an empty dimension and a NULL operand; nothing is launched (C keeps its sentinel)."""
    M, N, K = 8, 12, 5
    a = torch.ones(M, K, dtype=torch.float64, device=DEV)
    b = torch.ones(K, N, dtype=torch.float64, device=DEV)
    c = torch.full((M, N), SENTINEL, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(A=a.data_ptr(), B=b.data_ptr(), Cp=c.data_ptr(), ldc=N, m=M, n=N, k=K):
        return engine.lib.vggp_gemm(engine._h, A, K, 1, B, N, 1, Cp, ldc, m, n, k, st)

    assert call(ldc=N - 1) == VGGP_EINVAL
    assert call(m=0) == VGGP_EINVAL and call(n=0) == VGGP_EINVAL and call(k=0) == VGGP_EINVAL
    assert call(A=None) == VGGP_EINVAL and call(B=None) == VGGP_EINVAL and call(Cp=None) == VGGP_EINVAL
    torch.cuda.synchronize()
    assert bool((c == SENTINEL).all())
    assert call() == VGGP_OK
    torch.cuda.synchronize()
    assert bool((c == float(K)).all())


@pytest.mark.parametrize("M,N,K", [(33, 31, 511), (512, 1024, 64), (513, 1000, 50)], ids=["small", "deep", "generic"])
def test_gemm_bitwise_repeatable(engine, M, N, K):
    A, B = values(M, N, K, False, seed=7)
    a, b = A.to(DEV), B.to(DEV)
    first = engine.gemm(a, b)
    for _ in range(3):
        assert torch.equal(engine.gemm(a, b), first)
