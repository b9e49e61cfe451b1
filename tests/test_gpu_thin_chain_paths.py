"""The four single-workgroup kernels of the thin chain, one at a time through their test exports (vggp_pivchol, vggp_rowqr, vggp_ritz,
vggp_thin_tail), against the plain references of tests/thin_chain_spec.py -- which tests/test_thin_chain_spec.py pins to oracle/kron.py --
and composed into the chain on synthetic Gram matrices.  Inputs sit in NaN-filled parents, outputs in sentinel-filled parents with guard
zones; every run asserts that the inputs and the guards are untouched.

a. vg_pivchol_kernel   graded G = L L^T with determinate pivots (every pivot leads the runner-up by 0.18 of the residual diagonal): the
   pivot sequence and, element by element, V against the long-double spec within 8 RHO_PIV (i + 1) u scale (scale: the absolute terms of
   the element's recurrence and of its pivot's).  Integer L in pivot-echelon form, rank < r: V bit for bit (L^T, then rows of Omega) --
   tie-break, "a pivot is used once", the `best > 0` branch, the cross-wave argmax.  Equal diagonals in three waves: lowest index first.
   The two-job launch is not exposed by the export and is not covered here (the step tests reach it).
b. vg_rowqr_kernel_t   all three instantiations at 74 sizes, r = 1 .. 64 (18, 22, 30, 62 and the other r that are no multiple of 4 are
   the ones whose last block used to run past the r x m allocation), inputs random / graded diag(6^-k)(Q + 1e-3 leak) / leaky (rows
   dominated by what leaks onto the leading directions: the second pass) / orthonormal.  Orthogonality, span, order within
   max(8 x float64 two-pass Gram-Schmidt on the same input, 64 m u), positive diagonal.  A row that is an exact combination of earlier rows:
   the output is finite and the rows BEFORE it hold the caps -- the kernel normalises rounding noise there, which is the chain's documented
   behaviour (the miss check is what protects the step).  Pass-through copy: bit for bit, cp_n = 0, 1, 16 K - 1, 16 K, (m - r) m.
c. vg_eigh_kernel, product form with Newton start   H = (V1 G) V1^T for r = 1 .. 64, hk = r .. 256: factors staged in LDS or read from
   global memory, Newton start taken (nearly diagonal H; counters[3] bit 27) or declined (dense H: Jacobi sweeps), spectra with 6 x decay,
   a triple cluster, a pair split by 1e-9, rank < r.  Criteria of test_eigh.
d. vg_thin_tail_kernel   eleven (r1, r2) on exact-rank inputs of make_dim(): the six outputs within 8 RHO_SPEC u abs-scale of the long-double
   spec, beta and 1/D within 64 r u abs-scale, out == hout[0:6] bit for bit, optional pointers, three slabs == one slab bit for bit, the
   packed words, the two miss thresholds at 0.1 x and 10 x for each dimension, NaN, the status precedence table, and oracle.kron.finish
   (ELBO 1e-12, gradient 1e-10).
e. the chain composed from the exports (pivchol, rowqr, Z = V G, rowqr, Ritz, sandwiches, tail; products through vggp_gemm) on synthetic
   Gram matrices of exact rank with a 6 x spectrum against oracle.kron.finish at the caps of d; the same with rank = r + 2 and with a 1.3 x
   spectrum that runs through the cut: VG_ESUBMISS, every word of the block finite.

Measured on one MI355X (all 174 tests: 4.5 s), the reference's own figure beside each:
  a. pivots equal on all 13 sizes; worst |V - long double| / ((i + 1) u scale) 0.57 (float64 numpy spec 0.71, RHO_PIV 0.75, cap 6);
     exact-arithmetic and tie cases equal bit for bit.
  b. worst over the 74 sizes, kernel / float64 two-pass Gram-Schmidt: orthogonality 5.9e-16 / 7.4e-16, span 5.8e-16 / 7.2e-16, order
     3.9e-16 / 1.3e-16; nowhere above 0.026 of its cap (the floor 64 m u everywhere); rows before an exactly dependent row 3.9e-16; with
     the pass-through copy 3.8e-16.  Against a build of the parent commit with the same exports: all 180 outputs with r = 0 mod 4
     identical bit for bit; 24 of the 235 with r != 0 mod 4 differ in the last bit (the parent's extra rows were whatever the LDS held,
     and a NaN or a large value there asked for a second pass over the whole block).
  c. worst over the 34 cases: theta 8.9e-16 max|theta| (cap 1e-12), |W W^T - I| 2.3e-14 (1e-11), residual 5.7e-14 |H|_F (1e-11); Newton
     start taken in all 13 nearly diagonal cases with r <= 48 and 6 x decay (0 - 2 iterations, no rotation round), on the aligned split
     pair and the aligned rank-deficient case, and in the dense cases with r = 1, 2; declined in every dense case with r >= 8 (7 - 12
     sweeps, 35 - 519 rounds), at r > 48, and on the aligned triple cluster (zero gaps).
  d. worst |kernel - long double| / (u abs-scale) per component (ELBO, d/d ell1, ell2, s1, s2, v): 0.76 1.81 1.69 0.67 0.43 0.91, the
     float64 numpy spec's own rho_spec 1.50 1.81 1.69 0.42 0.43 1.24 (caps 8 RHO_SPEC); beta 2.5, 1/D 1.0 (caps 64 r); against
     oracle.kron.finish ELBO 2.1e-16, gradient 5.2e-13 (d/d ell), 3.7e-16 (others).
  e. chain from the exports against the oracle: ELBO equal to the last bit, gradient <= 2.5e-13 (d/d ell), 3.8e-16 (others), ranks 6 and 9
     found; rank = r + 2 and the 1.3 x spectrum: VG_ESUBMISS in both dimensions on all three shapes, blocks finite.
Mutations tried against this file (each made the named tests fail, then reverted): a tk[] entry of the tail pointing at the wrong buffer
(test_tail_against_spec_and_oracle, all cases, and test_chain_from_the_exports); kk rounded DOWN to 8 (test_tail_against_spec_and_oracle);
dg[q][l + 192] dropped (the same, m = 255 / 256); the tie-break of the cross-wave exchange flipped (test_pivchol_tie_goes_to_the_lowest_index;
the in-wave flip went unnoticed until rows 5 and 9 tied too); the block's second pass disabled (test_rowqr_sizes, 50 sizes); the two
miss thresholds swapped for dimension 2 (test_tail_miss_thresholds).  kk rounded up to 16 instead of 8 changes no bit and no test fails:
kk only stops the reduction early over operands that are zero there.  The `staged` condition moved by one was not run: the launcher
sizes the LDS from its own copy of the condition, so that mutant stores past its allocation; the boundary itself (r = 48 / 49,
hk = 128 / 129) is in the case list."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import thin_chain_spec as S
from variational_gridded_gaussian_processes_amd._lib import VGGP_EINVAL, VGGP_OK, ThinTailArgs

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENT = -777.25
ISENT = 0x5A5A5A5A


class Win:
    """Device windows: inputs in NaN-filled parents (snapshotted), outputs in sentinel-filled parents with guard zones."""

    def __init__(self):
        self.ins, self.outs = [], []

    def inp(self, a):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.copy())
        fill = float("nan") if t.dtype == torch.float64 else ISENT
        parent = torch.full((2 * GUARD + t.numel(),), fill, dtype=t.dtype, device=DEV)
        w = parent[GUARD:GUARD + t.numel()].view(t.shape)
        w.copy_(t)
        self.ins.append((parent, parent.clone()))
        return w

    def out(self, *shape):
        n = int(np.prod(shape))
        parent = torch.full((2 * GUARD + n,), SENT, dtype=torch.float64, device=DEV)
        self.outs.append((parent, n))
        return parent[GUARD:GUARD + n].view(shape)

    def check(self):
        torch.cuda.synchronize()
        for p, p0 in self.ins:
            same = torch.equal(p.view(torch.int64), p0.view(torch.int64)) if p.dtype == torch.float64 else torch.equal(p, p0)
            assert same, "an input or its surroundings were written"
        for p, n in self.outs:
            assert bool((p[:GUARD] == SENT).all()) and bool((p[GUARD + n:] == SENT).all()), "write outside an output window"


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return (np.asarray(a, np.float64) + 0.0).view(np.int64)         # (+ 0.0: -0 and +0 are the same result)


# ---- a. pivchol ------------------------------------------------------------------------------------------------------------------------
def run_pivchol(engine, G, Om):
    r, m = Om.shape
    w = Win()
    g, o, v = w.inp(G), w.inp(Om), w.out(r, m)
    rc = engine.lib.vggp_pivchol(engine._h, g.data_ptr(), o.data_ptr(), m, r, v.data_ptr(), stream())
    w.check()
    assert rc == VGGP_OK, engine.lib.vggp_last_error()
    V = v.cpu().numpy()
    assert not (V == SENT).any()
    return V


@pytest.mark.parametrize("m,r", S.PIV_CASES)
def test_pivchol_determinate_pivots(engine, m, r):
    G, Om = S.graded_chol_case(m, r, 100 * m + r)
    Vl, piv, lead, scale = S.pivchol(G.astype(S.LD), Om.astype(S.LD), r)
    assert min(lead) >= 1e-3
    V = run_pivchol(engine, G, Om)
    assert list(np.abs(V).argmax(1)) == piv
    steps = np.arange(1, r + 1)[:, None]
    ratio = float((np.abs(V.astype(S.LD) - Vl) / (steps * S.U * scale)).max())
    print("pivchol ratio", m, r, ratio)
    assert ratio <= 8 * S.RHO_PIV


@pytest.mark.parametrize("m,r", S.PIV_CASES)
def test_pivchol_exact_arithmetic_bitwise(engine, m, r):
    rank = min(r - 1, 20)
    G, Om, L, perm = S.exact_chol_case(m, r, rank, m + r)
    want = S.pivchol(G, Om, r)[0]
    V = run_pivchol(engine, G, Om)
    assert np.array_equal(bits(V), bits(want))
    assert np.array_equal(V[:rank], L.T) and np.array_equal(bits(V[rank:]), bits(Om[rank:]))


def test_pivchol_tie_goes_to_the_lowest_index(engine):
    G, Om = S.tie_chol_case()
    V = run_pivchol(engine, G, Om)
    assert np.array_equal(bits(V), bits(S.pivchol(G, Om, 4)[0]))
    assert list(np.abs(V).argmax(1)) == [5, 9, 70, 200]


# ---- b. rowqr --------------------------------------------------------------------------------------------------------------------------
def run_rowqr(engine, Z, cp=None):
    r, m = Z.shape
    w = Win()
    z, v = w.inp(Z), w.out(r, m)
    src = dst = None
    if cp is not None and cp.size:
        src, dst = w.inp(cp), w.out(cp.size)
    rc = engine.lib.vggp_rowqr(engine._h, z.data_ptr(), r, m, v.data_ptr(), src.data_ptr() if src is not None else None,
                               dst.data_ptr() if dst is not None else None, cp.size if cp is not None else 0, stream())
    w.check()
    assert rc == VGGP_OK, engine.lib.vggp_last_error()
    V1 = v.cpu().numpy()
    assert not (V1 == SENT).any()
    return (V1, dst.cpu().numpy()) if dst is not None else V1


def rowqr_caps(Z):
    ref = S.rowqr_checks(Z, S.cgs2(Z))
    floor = 64 * Z.shape[1] * S.U
    return [max(8 * x, floor) for x in ref[:3]], ref


def assert_rowqr(Z, V1, tag):
    caps, ref = rowqr_caps(Z)
    got = S.rowqr_checks(Z, V1)
    print("rowqr", tag, "got", got, "two-pass float64", ref, "caps", caps)
    assert np.isfinite(V1).all()
    assert got[0] <= caps[0] and got[1] <= caps[1] and got[2] <= caps[2] and got[3] > 0.0, (tag, got, caps)
    return got


@pytest.mark.parametrize("r,m", S.ROWQR_CASES, ids=["r%d-m%d" % c for c in S.ROWQR_CASES])
def test_rowqr_sizes(engine, r, m):
    for kind in S.ROWQR_KINDS:
        Z = S.rowqr_input(kind, r, m, 1000 * r + m)
        assert_rowqr(Z, run_rowqr(engine, Z), (kind, r, m))


@pytest.mark.parametrize("r,m", [(8, 33), (17, 128), (30, 129), (62, 127), (20, 256)])
def test_rowqr_exactly_dependent_row(engine, r, m):
    Z = S.rowqr_input("dependent", r, m, 1000 * r + m)
    V1 = run_rowqr(engine, Z)
    assert np.isfinite(V1).all()
    k = r // 2
    assert_rowqr(Z[:k], V1[:k], ("dependent", r, m))


@pytest.mark.parametrize("r,m", [(4, 64), (18, 33), (16, 128), (62, 127), (64, 128), (22, 256)])
def test_rowqr_pass_through_copy(engine, r, m):
    """cp_n > 0 selects the instantiation with the copy in registers (m <= 128; the wide one copies in a loop): the copy is bit for bit, and
    the orthonormalisation holds the same caps."""
    Z = S.rowqr_input("leaky", r, m, 1000 * r + m)
    rng = np.random.default_rng(r + m)
    for cp_n in S.ROWQR_CP:
        n = (m - r) * m if cp_n == "rest" else cp_n
        cp = rng.standard_normal(n)
        res = run_rowqr(engine, Z, cp)
        V1, dst = res if n else (res, cp)
        assert np.array_equal(dst.view(np.int64), cp.view(np.int64))
        assert_rowqr(Z, V1, ("copy", r, m, n))


# ---- c. ritz ---------------------------------------------------------------------------------------------------------------------------
def run_ritz(engine, Hl, Hr):
    r, hk = Hl.shape
    w = Win()
    hl, hr, lam, W = w.inp(Hl), w.inp(Hr), w.out(r), w.out(r, r)
    cnt, err = (C.c_int32 * 4)(-1, -1, -1, -1), C.c_int32(-1)
    rc = engine.lib.vggp_ritz(engine._h, hl.data_ptr(), hr.data_ptr(), r, hk, lam.data_ptr(), W.data_ptr(), cnt, C.byref(err), stream())
    w.check()
    return rc, lam.cpu().numpy(), W.cpu().numpy(), list(cnt), err.value


@pytest.mark.parametrize("r,hk,spectrum,aligned", S.RITZ_CASES,
                         ids=["r%d-hk%d-%s-%s" % (r, hk, sp, "aligned" if al else "dense") for r, hk, sp, al in S.RITZ_CASES])
def test_ritz_product_form(engine, r, hk, spectrum, aligned):
    Hl, Hr, _ = S.ritz_case(r, hk, spectrum, aligned, 1000 * r + hk)
    ref = S.ritz_ref(Hl, Hr)
    H = S.ritz_matrix(Hl, Hr)
    rc, lam, W, cnt, err = run_ritz(engine, Hl, Hr)
    direct = bool(cnt[3] & S.VG_EIG_DIRECT)
    resid = np.linalg.norm(W @ H @ W.T - np.diag(lam)) / np.linalg.norm(H)
    print("ritz", r, hk, spectrum, aligned, "direct", direct, "rounds", cnt[0], "iterations", cnt[1] & 0xff, "theta",
          np.abs(lam - ref).max() / np.abs(ref).max(), "orth", np.abs(W @ W.T - np.eye(r)).max(), "resid", resid)
    assert rc == VGGP_OK, engine.lib.vggp_last_error()
    assert err == 0 and cnt[2] == 0
    assert np.isfinite(lam).all() and np.isfinite(W).all()
    assert np.all(np.diff(lam) <= 0)
    assert np.abs(lam - ref).max() < 1e-12 * np.abs(ref).max()
    assert np.abs(W @ W.T - np.eye(r)).max() < 1e-11
    assert resid < 1e-11
    assert cnt[1] >> 8 == int(np.sum(ref > S.VG_EIG_RANK_CUT * ref[0]))
    if r > S.VG_EIG_NEWTON_MAX_M:
        assert not direct
    elif aligned and spectrum == "decay":
        assert direct and cnt[0] == 0                       # the Newton start must be taken: no rotation rounds at all
    elif not aligned and r >= 8:
        assert not direct and cnt[0] > 0                    # dense H: the start declines, the sweeps converge


# ---- d. thin_tail ----------------------------------------------------------------------------------------------------------------------
def run_tail(engine, inp, slabs=None, slab_pad=0, want=("out", "beta", "hout"), words=False):
    """-> dict of numpy outputs (out [8], beta, invd, hout [16]); words: the optional status / counter / jitter / peer_fail words of inp."""
    r1, r2, m1, m2 = len(inp["lam1"]), len(inp["lam2"]), inp["m1"], inp["m2"]
    w = Win()
    a = ThinTailArgs()
    keep = []

    def put(x):
        t = w.inp(x)
        keep.append(t)
        return t.data_ptr()

    def diag_only(d, m):
        M = np.full((m, m), np.nan)
        M[np.arange(m), np.arange(m)] = d
        return M

    a.theta = put(np.array(inp["theta"], dtype=np.float64))
    a.n_total, a.yy = float(inp["N"]), float(inp["yy"])
    a.r1, a.r2, a.m1, a.m2 = r1, r2, m1, m2
    for k in ("W1", "W2", "lam1", "lam2", "AM1", "AH1", "AM2", "AH2"):
        setattr(a, k, put(inp[k]))
    if slabs is None:
        a.AC, a.ac_nslab, a.ac_slab = put(inp["AC"]), 1, 3 * r1 * r2
    else:
        S3 = np.full((len(slabs), 3 * r1 * r2 + slab_pad), np.nan)
        S3[:, :3 * r1 * r2] = slabs.reshape(len(slabs), -1)
        a.AC, a.ac_nslab, a.ac_slab = put(S3), len(slabs), 3 * r1 * r2 + slab_pad
    a.G1, a.H1 = put(diag_only(inp["dG1"], m1)), put(diag_only(inp["dH1"], m1))
    a.G2, a.H2 = put(diag_only(inp["dG2"], m2)), put(diag_only(inp["dH2"], m2))
    outs = {}
    if "out" in want:
        outs["out"] = w.out(8)
        a.out = outs["out"].data_ptr()
    if "beta" in want:
        outs["beta"], outs["invd"] = w.out(r1, r2), w.out(r1, r2)
        a.beta_out, a.invd_out = outs["beta"].data_ptr(), outs["invd"].data_ptr()
    if "hout" in want:
        outs["hout"] = w.out(16)
        a.hout = outs["hout"].data_ptr()
    if words:
        cs, ee = inp.get("chol_status", (0, 0)), inp.get("eig_err", (0, 0))
        rc = np.asarray(inp.get("rcounters", np.zeros((2, 4))), dtype=np.int32)
        for k in range(2):
            a.status[k] = put(np.array([cs[k], ee[k]], dtype=np.int32))
            a.rcounters[k] = put(rc[k].copy())
            a.jit[k] = put(np.array([inp.get("jit", (0.0, 0.0))[k]]))
        a.peer_fail = put(np.array([inp.get("peer_fail", 0.0)]))
    rc = engine.lib.vggp_thin_tail(engine._h, C.byref(a), stream())
    w.check()
    assert rc == VGGP_OK, engine.lib.vggp_last_error()
    return {k: v.cpu().numpy() for k, v in outs.items()}


@pytest.fixture(scope="module")
def tails():
    out = {}
    for c in S.TAIL_CASES:
        d1, d2, inp = S.tail_case(c)
        out[c] = (d1, d2, inp, S.thin_tail(inp, np.longdouble))
    return out


TAIL_IDS = ["r%dx%d-m%dx%d-rho%dx%d-slab%d" % c for c in S.TAIL_CASES]


@pytest.mark.parametrize("case", S.TAIL_CASES, ids=TAIL_IDS)
def test_tail_against_spec_and_oracle(engine, tails, case):
    d1, d2, inp, ld = tails[case]
    r1, r2 = case[0], case[1]
    got = run_tail(engine, inp)
    out = got["out"]
    ratio = np.array(np.abs(out[:6].astype(S.LD) - ld["out"]) / (S.U * ld["abs"]), dtype=float)
    rb = float((np.abs(got["beta"].astype(S.LD) - ld["beta"]) / (S.U * ld["beta_abs"])).max())
    rd = float((np.abs(got["invd"].astype(S.LD) - ld["invd"]) / (S.U * ld["invd_abs"])).max())
    elbo, grad = S.oracle_finish(d1, d2, inp)
    print("tail", case, "ratio", ratio.tolist(), "rho_spec", S.RHO_SPEC, "beta", rb, "invd", rd, "oracle ELBO", abs(out[0] - elbo) / abs(elbo),
          "grad", (np.abs(out[1:6] - grad) / np.abs(grad)).tolist())
    assert np.isfinite(out[:6]).all()
    assert np.all(ratio <= 8 * np.array(S.RHO_SPEC)), ratio
    assert rb <= 64 * max(r1, r2) and rd <= 64 * max(r1, r2)
    assert np.array_equal(out[:6].view(np.int64), got["hout"][:6].view(np.int64))
    assert out[6] == SENT and out[7] == SENT                                       # out[6:8] belong to the caller
    # the packed block with no optional word given: zeros, the ranks, the sequence number
    assert np.array_equal(got["hout"][6:].view(np.int64), ld["block"][6:].view(np.int64))
    # against the oracle
    assert abs(out[0] - elbo) <= 1e-12 * abs(elbo)
    assert np.all(np.abs(out[1:6] - grad) <= 1e-10 * np.abs(grad))


@pytest.mark.parametrize("case", [S.TAIL_CASES[1], S.TAIL_CASES[7], S.TAIL_CASES[9]], ids=[TAIL_IDS[1], TAIL_IDS[7], TAIL_IDS[9]])
def test_tail_optional_pointers_and_slabs(engine, tails, case):
    """Optional outputs left out: the others keep their bits.  AC as three slabs (a stride beyond 3 r1 r2, NaN between the slabs) whose
    fixed-order sum is the unsplit AC bit for bit: every output keeps its bits."""
    inp = dict(tails[case][2])
    ACr, slabs = S.split_slabs(inp["AC"], 3, 17)
    inp["AC"] = ACr
    full = run_tail(engine, inp)
    for want in (("hout",), ("out",), ("out", "hout"), ("beta", "hout")):
        part = run_tail(engine, inp, want=want)
        for k, v in part.items():
            assert np.array_equal(v.view(np.int64), full[k].view(np.int64)), (want, k)
        if "beta" in want:
            assert np.array_equal(part["invd"].view(np.int64), full["invd"].view(np.int64))
    for pad in (0, 5):
        split = run_tail(engine, inp, slabs=slabs, slab_pad=pad)
        for k in ("out", "beta", "invd", "hout"):
            assert np.array_equal(split[k].view(np.int64), full[k].view(np.int64)), (pad, k)


def test_tail_packed_words(engine, tails):
    inp = dict(tails[S.TAIL_CASES[5]][2])
    rc = np.array([[23, 4 | (31 << 8), 0, 99], [0, 3 | (2 << 8), 0, -5]], dtype=np.int32)
    inp.update(rcounters=rc, jit=(1e-8, 1e-6), peer_fail=2.0, chol_status=(0, 0), eig_err=(0, 0))
    want = S.thin_tail(inp, np.longdouble)
    got = run_tail(engine, inp, words=True)
    assert np.array_equal(got["hout"][6:].view(np.int64), want["block"][6:].view(np.int64))
    words = got["hout"][10:15].view(np.int32)
    assert list(words[:4]) == [23, 4 | (16 << 8), 0, 0] and list(words[4:8]) == [0, 3 | (13 << 8), 0, 0] and list(words[8:10]) == [0, 0]
    assert got["hout"][15] == inp["theta"][5] and got["hout"][6] == 2.0 and list(got["hout"][8:10]) == [1e-8, 1e-6]


def test_tail_miss_thresholds(engine, tails):
    """tr G - sum theta at 0.1 x and 10 x each threshold, each dimension: 0 below, VG_ESUBMISS above; the other dimension stays 0."""
    inp = tails[S.TAIL_CASES[4]][2]
    for k, which in itertools.product((0, 1), (0, 1)):
        for factor, want in ((0.1, 0), (10.0, S.VG_ESUBMISS)):
            i2 = S.miss_input(inp, k, which, factor)
            assert S.thin_tail(i2)["status"][k] == want
            st = run_tail(engine, i2, want=("hout",))["hout"][14:15].view(np.int32)
            assert st[k] == want and st[1 - k] == 0, (k, which, factor, list(st))
    for k in (0, 1):
        i2 = dict(inp)
        lam = inp["lam%d" % (k + 1)].copy()
        lam[-1] = np.nan
        i2["lam%d" % (k + 1)] = lam
        st = run_tail(engine, i2, want=("hout",))["hout"][14:15].view(np.int32)
        assert st[k] == S.VG_ESUBMISS


def test_tail_status_precedence(engine, tails):
    inp = tails[S.TAIL_CASES[2]][2]
    for chol, rstat, err, k, miss in itertools.product((0, -2), (0, -6), (0, 1, 2, 3), (0, 1), (False, True)):
        i2 = dict(inp)
        cs, ee, rc = [0, 0], [0, 0], np.zeros((2, 4), dtype=np.int32)
        cs[k], ee[k], rc[k][2] = chol, err, rstat
        i2.update(chol_status=cs, eig_err=ee, rcounters=rc)
        if miss:
            i2["lam%d" % (k + 1)] = inp["lam%d" % (k + 1)] * 0.5
        want = S.thin_tail(i2)["status"]
        assert want[k] == (chol if chol else rstat if rstat else S.VGGP_ENOCONV if err & 1 else S.VG_ESUBMISS if (miss or err & 2) else 0)
        st = run_tail(engine, i2, want=("hout",), words=True)["hout"][14:15].view(np.int32)
        assert list(st) == want, (chol, rstat, err, k, miss)


# ---- e. the chain composed from the exports -------------------------------------------------------------------------------------------
def chain_dim(m, rank, seed, decay=6.0):
    lam = decay ** -np.arange(rank, dtype=float)
    return S.make_dim(m, rank + 3, rank, rank, seed, spectrum=lam)


def run_chain(engine, d1, d2, r1, r2, seed):
    """pivchol, rowqr, Z = V G, rowqr, Ritz, the sandwiches, thin_tail -- every product through vggp_gemm -> (hout [16], inp)."""
    inp = S.tail_input(d1, d2, seed)
    rng = np.random.default_rng(seed)
    T = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)      # noqa: E731
    V1s, lams, Ws, AMs, AHs = [], [], [], [], []
    for d, r in ((d1, r1), (d2, r2)):
        m = d["m"]
        G, H0, Mk = T(d["G0"]), T(d["H0"]), T(d["Mk0"])
        V = engine.pivchol(G, T(rng.standard_normal((r, m))))
        Z = engine.gemm(engine.rowqr(V), G)
        V1 = engine.rowqr(Z)
        lam, W, cnt, err = engine.ritz(engine.gemm(V1, G), V1)
        V1s.append(V1); lams.append(lam); Ws.append(W)
        AMs.append(engine.gemm(engine.gemm(V1, Mk), V1.T))
        AHs.append(engine.gemm(engine.gemm(V1, H0), V1.T))
    C3 = [d1["B0"] @ inp["Y"].T @ d2["B0"].T, d1["V0"] @ inp["Y"].T @ d2["B0"].T, d1["B0"] @ inp["Y"].T @ d2["V0"].T]
    AC = torch.stack([engine.gemm(engine.gemm(V1s[0], T(Cq)), V1s[1].T) for Cq in C3])
    torch.cuda.synchronize()
    i2 = dict(inp)
    i2.update(W1=Ws[0].cpu().numpy(), W2=Ws[1].cpu().numpy(), lam1=lams[0].cpu().numpy(), lam2=lams[1].cpu().numpy(),
              AM1=AMs[0].cpu().numpy(), AH1=AHs[0].cpu().numpy(), AM2=AMs[1].cpu().numpy(), AH2=AHs[1].cpu().numpy(), AC=AC.cpu().numpy())
    return run_tail(engine, i2, want=("hout",))["hout"], i2


CHAIN_M = ((96, 128), (200, 256), (130, 100))


@pytest.mark.parametrize("m1,m2", CHAIN_M)
def test_chain_from_the_exports(engine, m1, m2):
    """Exact rank 6 and 9, r by the step's rule (rank + 3, rounded up to even): against oracle.kron.finish at the caps of the tail."""
    d1, d2 = chain_dim(m1, 6, m1), chain_dim(m2, 9, m2 + 1)
    hout, inp = run_chain(engine, d1, d2, 10, 12, m1 + m2)
    elbo, grad = S.oracle_finish(d1, d2, inp)
    st = hout[14:15].view(np.int32)
    words = hout[10:14].view(np.int32)
    print("chain", m1, m2, "ELBO", abs(hout[0] - elbo) / abs(elbo), "grad", (np.abs(hout[1:6] - grad) / np.abs(grad)).tolist(), "status", list(st),
          "ranks", words[1] >> 8, words[5] >> 8)
    assert list(st) == [0, 0]
    assert (words[1] >> 8, words[5] >> 8) == (6, 9)
    assert abs(hout[0] - elbo) <= 1e-12 * abs(elbo)
    assert np.all(np.abs(hout[1:6] - grad) <= 1e-10 * np.abs(grad))


@pytest.mark.parametrize("m1,m2", CHAIN_M)
@pytest.mark.parametrize("variant", ["rank_r_plus_2", "decay_1p3"])
def test_chain_miss_is_caught(engine, m1, m2, variant):
    """The range finder cannot hold the range in r rows: the tail must say VG_ESUBMISS for both dimensions, with a finite block."""
    r1, r2 = 8, 10
    if variant == "rank_r_plus_2":
        d1, d2 = chain_dim(m1, r1 + 2, m1), chain_dim(m2, r2 + 2, m2 + 1)
    else:
        d1, d2 = chain_dim(m1, 40, m1, decay=1.3), chain_dim(m2, 40, m2 + 1, decay=1.3)
    hout, _ = run_chain(engine, d1, d2, r1, r2, m1 + m2)
    st = hout[14:15].view(np.int32)
    print("chain", variant, m1, m2, "status", list(st))
    assert list(st) == [S.VG_ESUBMISS, S.VG_ESUBMISS]
    assert np.isfinite(hout[:10]).all() and np.isfinite(hout[15])


# ---- argument checks: VGGP_EINVAL before anything is launched -------------------------------------------------------------------------
def test_einval_contracts(engine):
    """r > m, r beyond the kernel's limit, m > 256, null pointers, a null context: VGGP_EINVAL, nothing written.  (The exports take one
    job each, so the launchers' njobs checks cannot be reached through them.)"""
    lib, h, st = engine.lib, engine._h, stream()
    buf = torch.full((64,), SENT, dtype=torch.float64, device=DEV)
    p = buf.data_ptr()
    for args in ((p, p, 4, 5, p), (p, p, 257, 4, p), (p, p, 128, 65, p), (p, p, 4, 0, p), (None, p, 4, 2, p), (p, None, 4, 2, p), (p, p, 4, 2, None)):
        assert lib.vggp_pivchol(h, *args, st) == VGGP_EINVAL
    assert lib.vggp_pivchol(None, p, p, 4, 2, p, st) == VGGP_EINVAL
    for args in ((p, 5, 4, p, None, None, 0), (p, 65, 128, p, None, None, 0), (p, 4, 257, p, None, None, 0), (p, 0, 4, p, None, None, 0),
                 (None, 2, 4, p, None, None, 0), (p, 2, 4, None, None, None, 0), (p, 2, 4, p, None, p, 3), (p, 2, 4, p, p, None, 3),
                 (p, 2, 4, p, p, p, -1)):
        assert lib.vggp_rowqr(h, *args, st) == VGGP_EINVAL
    assert lib.vggp_rowqr(None, p, 2, 4, p, None, None, 0, st) == VGGP_EINVAL
    cnt, err = (C.c_int32 * 4)(-1, -1, -1, -1), C.c_int32(-1)
    for args in ((p, p, 5, 4, p, p), (p, p, 65, 128, p, p), (p, p, 4, 257, p, p), (p, p, 0, 4, p, p), (None, p, 2, 4, p, p), (p, None, 2, 4, p, p),
                 (p, p, 2, 4, None, p), (p, p, 2, 4, p, None)):
        assert lib.vggp_ritz(h, *args, cnt, C.byref(err), st) == VGGP_EINVAL
    assert lib.vggp_ritz(None, p, p, 2, 4, p, p, cnt, C.byref(err), st) == VGGP_EINVAL
    assert list(cnt) == [-1] * 4 and err.value == -1

    def targs(**kw):
        a = ThinTailArgs()
        for k in ("theta", "W1", "W2", "lam1", "lam2", "AM1", "AH1", "AM2", "AH2", "AC", "G1", "H1", "G2", "H2", "out", "beta_out", "invd_out", "hout"):
            setattr(a, k, p)
        a.r1, a.r2, a.m1, a.m2, a.ac_nslab, a.ac_slab = 2, 2, 4, 4, 1, 12
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = [dict(r1=5), dict(r2=5), dict(r1=33, m1=64), dict(r2=33, m2=64), dict(m1=257), dict(m2=257), dict(r1=0), dict(ac_nslab=0),
           dict(ac_nslab=2, ac_slab=11), dict(beta_out=None), dict(invd_out=None)]
    bad += [{k: None} for k in ("theta", "W1", "W2", "lam1", "lam2", "AM1", "AH1", "AM2", "AH2", "AC", "G1", "H1", "G2", "H2")]
    for kw in bad:
        assert lib.vggp_thin_tail(h, C.byref(targs(**kw)), st) == VGGP_EINVAL, kw
    assert lib.vggp_thin_tail(h, None, st) == VGGP_EINVAL
    assert lib.vggp_thin_tail(None, C.byref(targs()), st) == VGGP_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
