"""vggp_eigh on every path it reaches, with spectra beyond the smooth kernel factors of test_gpu_blocks.test_eigh.

Paths.  Scalar cyclic Jacobi by padded size m2 = m + (m & 1): m2 < 16 (no dense phase), 16 <= m2 <= 128 (fixed-address dense phase,
first-order polish), m <= 184 (LDS), m > 184 (global memory).  Block Jacobi: nb = 2 ceil(m / 32) = 2, 4, 6, 8, whole and ragged
32-blocks.
Spectra (tests/dense_cases.py eig_case), Q diag(d) Q^T with a random orthogonal Q unless stated:
    geometric        1 down to 1e-10                       clusters          three values, each repeated about m / 3 times (the
    indefinite       symmetric about 0                                       polish divides by g_ii - g_jj)
    rank_deficient   B B^T, B of shape m x (m // 2)        diagonal          distinct unsorted entries, no Q
    scaled_identity  3 I                                   scaled_up / _down geometric times 2^200 / 2^-200
    equal_pair       2 I plus one off-diagonal pair: g_ii == g_jj, the 45 degree rotation
    zero             the zero matrix: every threshold is 0, nothing rotates, every loop is bounded by its sweep limit
Each family runs at one size of every path; the sizes of a path rotate through the families, so every size is used.
Criteria are test_eigh's: eigenvalues within 1e-12 max|w| of numpy.linalg.eigvalsh, |Qt Qt^T - I| < 1e-11,
||Qt G Qt^T - diag(lam)||_F < 1e-11 ||G||_F, sweeps < 60, descending lam for the scalar variant.  Eigenvectors are judged through
orthonormality and the residual only: a cluster has no unique basis."""
import ctypes as C

import numpy as np
import pytest
import torch

import dense_cases as dc
from variational_gridded_gaussian_processes_amd._lib import FLAG_BLOCK_JACOBI, VGGP_EINVAL, VGGP_ENOTPD, VGGP_OK

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENT = -777.25

SCALAR_PATHS = {"m2<16": (2, 3, 14), "dense": (15, 16, 17, 47, 48, 49, 127), "lds": (129, 183, 184), "global": (186, 255)}
BLOCK_PATHS = {"nb2": (2, 31, 32), "nb4": (33,), "nb6": (65, 96), "nb8": (97, 127)}
CASES = [(fam, block, path, sizes[f % len(sizes)])
         for f, fam in enumerate(dc.EIG_FAMILIES)
         for block, paths in ((False, SCALAR_PATHS), (True, BLOCK_PATHS))
         for path, sizes in paths.items()]


def test_every_size_is_used():
    for block, paths in ((False, SCALAR_PATHS), (True, BLOCK_PATHS)):
        want = {m for s in paths.values() for m in s}
        assert want == {m for fam, b, path, m in CASES if b == block}


def eigh(engine, G, block):
    """-> rc, lam, Qt (numpy), sweeps; G in a NaN-filled parent, lam and Qt in sentinel-filled parents."""
    m = G.shape[0]
    pg = torch.full((2 * GUARD + m * m,), float("nan"), dtype=torch.float64, device=DEV)
    wg = pg[GUARD:GUARD + m * m].view(m, m)
    wg.copy_(torch.tensor(G, device=DEV))
    pg0 = pg.view(torch.int64).clone()
    pq = torch.full((2 * GUARD + m * m,), SENT, dtype=torch.float64, device=DEV)
    pl = torch.full((2 * GUARD + m,), SENT, dtype=torch.float64, device=DEV)
    wq, wl = pq[GUARD:GUARD + m * m].view(m, m), pl[GUARD:GUARD + m]
    sw = C.c_int32(-1)
    rc = engine.lib.vggp_eigh(engine._h, wg.data_ptr(), m, wl.data_ptr(), wq.data_ptr(), C.byref(sw), FLAG_BLOCK_JACOBI if block else 0,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(pg.view(torch.int64), pg0), "G or its surroundings were written"
    for p, n in ((pq, m * m), (pl, m)):
        assert bool((p[:GUARD] == SENT).all()) and bool((p[GUARD + n:] == SENT).all()), "write outside an output window"
    return rc, wl.cpu().numpy(), wq.cpu().numpy(), sw.value


@pytest.mark.parametrize("family,block,path,m", CASES, ids=[f"{f}-{'block' if b else 'scalar'}-{p}-{m}" for f, b, p, m in CASES])
def test_eigh_spectra(engine, family, block, path, m):
    G = dc.eig_case(family, m)
    rc, lam, Qt, sweeps = eigh(engine, G, block)
    assert rc == VGGP_OK, engine.lib.vggp_last_error()
    assert np.isfinite(lam).all() and np.isfinite(Qt).all()
    w = np.linalg.eigvalsh(G)
    wmax, gn = np.abs(w).max(), np.linalg.norm(G)
    resid = np.linalg.norm(Qt @ G @ Qt.T - np.diag(lam))
    if family == "zero":
        assert wmax == 0.0 and not lam.any() and resid == 0.0
    else:
        assert np.abs(np.sort(lam) - w).max() < 1e-12 * wmax
        assert resid < 1e-11 * gn
    assert np.abs(Qt @ Qt.T - np.eye(m)).max() < 1e-11
    assert 0 <= sweeps < 60
    if not block:
        assert np.all(np.diff(lam) <= 0)
    if family == "diagonal":
        d = np.diag(G)
        if block:
            assert np.array_equal(np.sort(lam), np.sort(d))
        else:
            assert np.array_equal(lam, np.sort(d)[::-1])
        assert np.isin(Qt, (0.0, 1.0, -1.0)).all() and np.array_equal(np.abs(Qt).sum(1), np.ones(m))
        assert np.array_equal(np.abs(Qt) @ d, lam)               # row j is the unit vector of lam[j]'s position


@pytest.mark.parametrize("m,block", [(48, False), (97, True), (184, False)])
def test_eigh_bitwise_repeatable(engine, m, block):
    G = dc.eig_case("clusters", m)
    rc0, lam0, Qt0, sw0 = eigh(engine, G, block)
    assert rc0 == VGGP_OK
    for _ in range(3):
        rc, lam, Qt, sw = eigh(engine, G, block)
        assert rc == VGGP_OK and sw == sw0
        assert np.array_equal(lam.view(np.int64), lam0.view(np.int64)) and np.array_equal(Qt.view(np.int64), Qt0.view(np.int64))


@pytest.mark.parametrize("m,block", [(14, False), (127, False), (184, False), (186, False), (97, True)])
def test_eigh_ignores_stale_scratch(engine, m, block):
    """The work matrix, rotation log and counters live in the context's shared scratch.  An all-NaN K on the blocked Cholesky path
    leaves NaN all over it; the same solve after that returns the same bits as before."""
    G = dc.eig_case("geometric", m)
    before = eigh(engine, G, block)
    K = torch.full((300, 300), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.empty(2, 300, 300, dtype=torch.float64, device=DEV)
    assert engine.lib.vggp_cholesky_inverse(engine._h, K.data_ptr(), 300, out[0].data_ptr(), out[1].data_ptr(), None,
                                            torch.cuda.current_stream().cuda_stream) == VGGP_ENOTPD
    torch.cuda.synchronize()
    after = eigh(engine, G, block)
    assert before[0] == after[0] == VGGP_OK and before[3] == after[3]
    assert np.array_equal(before[1].view(np.int64), after[1].view(np.int64))
    assert np.array_equal(before[2].view(np.int64), after[2].view(np.int64))


def test_eigh_einval_contract(engine):
    buf = torch.full((3,), SENT, dtype=torch.float64, device=DEV)
    g, lam, qt = (buf[i:i + 1].data_ptr() for i in range(3))
    st = torch.cuda.current_stream().cuda_stream
    for args in ((g, 0, lam, qt), (g, -1, lam, qt), (g, 257, lam, qt), (None, 1, lam, qt), (g, 1, None, qt), (g, 1, lam, None)):
        sw = C.c_int32(-1)
        assert engine.lib.vggp_eigh(engine._h, *args, C.byref(sw), 0, st) == VGGP_EINVAL
        assert sw.value == -1
    assert engine.lib.vggp_eigh(None, g, 1, lam, qt, None, 0, st) == VGGP_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
    # sweeps_out may be NULL; m = 1 returns the element itself
    buf[0] = -2.5
    assert engine.lib.vggp_eigh(engine._h, g, 1, lam, qt, None, 0, st) == VGGP_OK
    torch.cuda.synchronize()
    assert buf[1].item() == -2.5 and abs(buf[2].item()) == 1.0
