"""vggp_factor_build on every path of its kernel (csrc/factor_build.hip): WIDE (ncols >= 512: tmw rows x 512 columns) and TALL
(4 tmw rows x 128 columns) tiles, 16-byte and scalar stores (ncols even and both outputs 16-byte aligned, or not), 16-byte and
scalar coordinate loads, and tmw = 2, 4, 8, 16 rows per wave (launches of < 2^18, >= 2^18, >= 2^21, >= 2^24 elements).

Two references:
  * tests/golden/factor_hp.npz -- 50-digit values at sampled elements, every basis, ell from 1/2000 to 3.2e4 mesh spacings --
    with |got - hp| <= c eps S, c = 4 max(R_oracle, 1) (factor_hp_cases.py; R_oracle is the numpy oracle's measured constant, the
    4 allows the device's exp / expm1 / cos a couple of ulp more than libm);
  * the numpy oracle (itself pinned on that file by tests/test_factor_hp.py) for whole matrices, same rule with S evaluated in
    float64 and c doubled (both sides round): c = 8 max(R, 1), R the worst R_oracle of the basis / kernel family.
No element is skipped or filtered.  The B0 cases at ell = delta/2000 and delta/700 returned NaN / inf before K0 moved from
e^{-kt} 4 sinh^2(t/2) to the expm1 form (csrc/factor_elem.h vg_b0_K)."""
import itertools

import numpy as np
import pytest
import torch

import factor_hp_cases as H
from variational_gridded_gaussian_processes_amd._lib import BASIS, KIND, VGGP_EINVAL, VGGP_OK

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.25


def dev(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def raw(engine, kind, basis, x, n, grid, m, ell, flags, outs):
    """the C-ABI call on raw device addresses (None = NULL); outs = (A0, dA0, K0, dK0) addresses"""
    return engine.lib.vggp_factor_build(engine._h, KIND[kind], BASIS[basis], x, n, grid, m, float(ell), int(flags),
                                        outs[0], outs[1], outs[2], outs[3], torch.cuda.current_stream().cuda_stream)


# ---- against the 50-digit fixture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", H.cases(), ids=H.case_ids())
def test_kernel_vs_50_digits(engine, c):
    outs = engine.factor_build(c.kind, c.basis, dev(c.x), dev(c.grid), c.ell, flags=c.flags)
    mats = [o.cpu().numpy() for o in outs]
    got = H.sample(c, mats)
    q = {k: H.ratio_to_bound(got[k], c.hp[k], c.S[k]) for k in H.OUTPUTS}
    with np.errstate(divide="ignore", invalid="ignore"):
        relerr = {k: float(np.nanmax(np.where(np.abs(c.hp[k]) > 1e-290, np.abs(got[k] - c.hp[k]) / np.abs(c.hp[k]), 0.0))) for k in H.OUTPUTS}
    print(f"{c.id}: err / (eps S) " + " ".join(f"{k} {q[k]:.2f}" for k in H.OUTPUTS) + f" (bound {H.tolerance_constant(c):.1f}); worst relative error "
          + " ".join(f"{k} {relerr[k]:.1e}" for k in H.OUTPUTS))
    for k, mat in zip(H.OUTPUTS, mats):
        assert np.isfinite(mat).all(), f"{k} is not finite"
    for k in H.OUTPUTS:
        assert q[k] <= H.tolerance_constant(c), (k, q[k])


# ---- every tile path, whole matrices against the numpy oracle -----------------------------------------------------------------
# (m, n): A-part path / K-part path
#   40 x 301, 300            tmw 2  TALL, scalar then 16-byte stores
#   40 x 511, 512, 513       tmw 2  the TALL / WIDE switch; 513: the last WIDE tile holds one column
#   65 x 4099                tmw 4  WIDE, odd ncols, ragged rows / K 65 x 65 TALL scalar stores
#   130 x 16390              tmw 8  WIDE, even ncols, 16-byte stores / K 130 x 130
#   250 x 67110              tmw 16 WIDE / K 250 x 250 TALL with 64-row tiles (VG_FB_MAXROWS, the LDS staging limit)
SHAPES = [(40, 301), (40, 300), (40, 511), (40, 512), (40, 513), (65, 4099), (130, 16390)]
PATH_CASES = [(m, n, fam) for (m, n) in SHAPES for fam in ("matern32", "rbf", "b0")] + [(250, 67110, "matern32"), (250, 67110, "b0")]


def expected_tmw(m, n):
    total = m * n + m * m
    return 16 if total >= 1 << 24 else 8 if total >= 1 << 21 else 4 if total >= 1 << 18 else 2


def path_inputs(m, n, fam):
    """B0: every mesh knot is a column (so are the knots that start a wave's and a tile's row group, where the rolling-edge
    recurrence restarts), then points inside and outside the mesh; pairwise: the inducing coordinates themselves, then the same"""
    rng = np.random.default_rng(1000 * m + n)
    grid = np.linspace(0.0, 1.0, m + 1 if fam == "b0" else m)
    x = np.concatenate([grid, rng.uniform(-0.1, 1.1, n - len(grid))])
    ell = 3.3 / m
    return grid, x, ell


@pytest.mark.parametrize("m,n,fam", PATH_CASES, ids=[f"{m}x{n}-{fam}" for m, n, fam in PATH_CASES])
def test_every_tile_path_vs_oracle(engine, m, n, fam):
    assert expected_tmw(m, n) == {40: 2, 65: 4, 130: 8, 250: 16}[m]
    grid, x, ell = path_inputs(m, n, fam)
    kind, basis = ("matern12", "b0") if fam == "b0" else (fam, "points")
    xd, gd = dev(x), dev(grid)
    outs = engine.factor_build(kind, basis, xd, gd, ell)
    again = engine.factor_build(kind, basis, xd, gd, ell)
    for o, o2 in zip(outs, again):
        assert torch.equal(o, o2)                       # bitwise repeatable on every path
    del again
    ref = H.oracle_outputs(kind, basis, grid, x, ell)
    if fam == "b0":
        SA, SK = H.S_b0_A(grid, x, ell), H.S_b0_K(m, float(grid[1] - grid[0]), ell)
    else:
        SA, SK = H.S_points(kind, grid, x, ell), H.S_points(kind, grid, grid, ell)
    c = H.family_constant(basis, kind)
    worst = {}
    for k, o, r, S in zip(H.OUTPUTS, outs, ref, (SA[0], SA[1], SK[0], SK[1])):
        got = o.cpu().numpy()
        assert got.shape == r.shape
        worst[k] = H.ratio_to_bound(got, r, S)
    print(f"{m} x {n} {fam}: err / (eps S) " + " ".join(f"{k} {worst[k]:.2f}" for k in H.OUTPUTS) + f" (bound {c:.1f})")
    for k in H.OUTPUTS:
        assert worst[k] <= c, (k, worst[k])


# ---- alignment and aliasing ---------------------------------------------------------------------------------------------------
def carve(parent, cursor, count, parity):
    """the next `count` doubles of `parent` at an offset of the given parity (0: 16-byte aligned, 1: 8-byte only), 16 doubles
    after the previous region; -> (view, offset, new cursor)"""
    off = cursor + 16
    off += (off + parity) % 2
    return parent[off:off + count], off, off + count


@pytest.mark.parametrize("fam", ["matern32", "b0"])
@pytest.mark.parametrize("m,n", [(40, 300), (40, 512), (40, 513), (65, 4099)])
def test_placement_does_not_change_a_bit(engine, m, n, fam):
    """x, the grid and all four outputs carved out of ONE device buffer, at 16-byte aligned offsets and at offsets that are only
    8-byte aligned (scalar coordinate loads, scalar stores): the same bits in both placements and in separate allocations, NaN
    around x and the grid never reaches an output, and the sentinel around the outputs is untouched."""
    grid, x, ell = path_inputs(m, n, fam)
    kind, basis = ("matern12", "b0") if fam == "b0" else (fam, "points")
    plain = [o.cpu() for o in engine.factor_build(kind, basis, dev(x), dev(grid), ell)]
    sizes = [len(x), len(grid), m * n, m * n, m * m, m * m]
    for parity in (0, 1):
        parent = torch.full((sum(sizes) + 32 * len(sizes) + 64,), SENTINEL, dtype=torch.float64, device=DEV)
        assert parent.data_ptr() % 16 == 0
        cursor, regions = 0, []
        for s in sizes:
            view, off, cursor = carve(parent, cursor, s, parity)
            assert view.data_ptr() % 16 == 8 * parity
            regions.append((view, off))
        for (view, off), src in zip(regions[:2], (x, grid)):
            parent[off - 8:off + len(src) + 8] = float("nan")
            view.copy_(dev(src))
        expect = parent.cpu().clone()
        rc = raw(engine, kind, basis, regions[0][0].data_ptr(), n, regions[1][0].data_ptr(), m, ell, 0, [v.data_ptr() for v, _ in regions[2:]])
        assert rc == VGGP_OK
        torch.cuda.synchronize()
        after = parent.cpu()
        for (view, off), want in zip(regions[2:], plain):
            got = after[off:off + want.numel()].view(want.shape)
            assert bool(torch.isfinite(got).all())
            assert torch.equal(got, want), parity
            expect[off:off + want.numel()] = want.reshape(-1)
        # everything else (sentinels, NaN borders, inputs) is bit-for-bit what it was
        assert torch.equal(after.view(torch.int64), expect.view(torch.int64))


# ---- output selection ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["matern32", "b0"])
def test_every_subset_of_outputs(engine, fam):
    """Each of the 16 subsets of {A0, dA0, K0, dK0} (the others NULL): requested outputs equal the all-outputs call to the bit,
    unrequested memory keeps its sentinel.  65 x 4099: all outputs run at tmw = 4, the K-only subsets at tmw = 2."""
    m, n = 65, 4099
    grid, x, ell = path_inputs(m, n, fam)
    kind, basis = ("matern12", "b0") if fam == "b0" else (fam, "points")
    xd, gd = dev(x), dev(grid)
    full = engine.factor_build(kind, basis, xd, gd, ell)
    for mask in itertools.product([False, True], repeat=4):
        bufs = [torch.full_like(f, SENTINEL) for f in full]
        rc = raw(engine, kind, basis, xd.data_ptr(), n, gd.data_ptr(), m, ell, 0, [b.data_ptr() if w else None for b, w in zip(bufs, mask)])
        assert rc == VGGP_OK, mask
        torch.cuda.synchronize()
        for b, f, w in zip(bufs, full, mask):
            assert torch.equal(b, f) if w else bool((b == SENTINEL).all()), mask


@pytest.mark.parametrize("fam", ["matern32", "b0"])
def test_no_observations(engine, fam):
    """n = 0, with and without an x pointer: the K part equals the ordinary call's, memory offered for the (empty) A part is
    not written."""
    m = 40
    grid, x, ell = path_inputs(m, 300, fam)
    kind, basis = ("matern12", "b0") if fam == "b0" else (fam, "points")
    xd, gd = dev(x), dev(grid)
    full = engine.factor_build(kind, basis, xd, gd, ell)
    for xptr, with_a in ((None, False), (xd.data_ptr(), True), (xd.data_ptr(), False)):
        a, da = torch.full((m, 8), SENTINEL, dtype=torch.float64, device=DEV), torch.full((m, 8), SENTINEL, dtype=torch.float64, device=DEV)
        k, dk = torch.full_like(full[2], SENTINEL), torch.full_like(full[3], SENTINEL)
        rc = raw(engine, kind, basis, xptr, 0, gd.data_ptr(), m, ell, 0,
                 [a.data_ptr() if with_a else None, da.data_ptr() if with_a else None, k.data_ptr(), dk.data_ptr()])
        assert rc == VGGP_OK
        torch.cuda.synchronize()
        assert torch.equal(k, full[2]) and torch.equal(dk, full[3])
        assert bool((a == SENTINEL).all()) and bool((da == SENTINEL).all())


# ---- contract -----------------------------------------------------------------------------------------------------------------
def test_factor_build_contract(engine):
    """VGGP_EINVAL for ell <= 0, B0 / VFF / B1 with a kernel that is not Matern-1/2, a NULL grid, NULL x with A outputs
    requested; nothing is written."""
    m, n = 9, 21
    x, mesh = dev(np.linspace(0, 1, n)), dev(np.linspace(0, 1, m + 1))
    vff_grid = dev(np.concatenate([[0.0, 1.0], np.pi * np.arange(5)]))        # m = 2 * 4 + 1 = 9
    bufs = [torch.full((m, n), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(2)] + \
           [torch.full((m, m), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(2)]
    ptrs = [b.data_ptr() for b in bufs]

    def call(kind="matern12", basis="b0", xp=x.data_ptr(), gp=mesh.data_ptr(), ell=0.3, outs=ptrs):
        return raw(engine, kind, basis, xp, n, gp, m, ell, 0, outs)

    assert call(ell=0.0) == VGGP_EINVAL and call(ell=-0.5) == VGGP_EINVAL
    assert call(basis="points", ell=0.0) == VGGP_EINVAL
    for kind in ("matern32", "matern52", "rbf"):
        assert call(kind=kind, basis="b0") == VGGP_EINVAL
        assert call(kind=kind, basis="vff", gp=vff_grid.data_ptr()) == VGGP_EINVAL
        assert call(kind=kind, basis="b1") == VGGP_EINVAL
    assert call(gp=None) == VGGP_EINVAL and call(basis="points", gp=None) == VGGP_EINVAL
    assert call(xp=None) == VGGP_EINVAL
    assert call(xp=None, outs=[ptrs[0], None, None, None]) == VGGP_EINVAL
    assert call(xp=None, outs=[None, ptrs[1], ptrs[2], ptrs[3]]) == VGGP_EINVAL
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in bufs)
    assert call(xp=None, outs=[None, None, ptrs[2], ptrs[3]]) == VGGP_OK       # NULL x is fine when no A output is asked for
    assert call(basis="vff", gp=vff_grid.data_ptr()) == VGGP_OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.stack([b.sum() for b in bufs])).all())
