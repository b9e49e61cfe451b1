"""Shapes, integer operands and the numpy reference of vggp_kron_quadform (csrc/raster_var.hip; TEST HELPER, CPU).

    out[a][b] = scale (kd - n1[a] n2[b] + (u1_a (x) u2_b)^T S (u1_a (x) u2_b)),      S flat index (i m2 + j) M + k m2 + l

Every operand takes integer values in {-2, ..., 2}: a term of the four-index sum is at most 2^5 in magnitude and there are M^2 of them,
so every partial sum, in any order, is an integer below 32 M^2 <= 2^21 2^5 < 2^53 for the shapes here -- fp64 sums are exact and the GPU
result must equal numpy's int64 einsum bit for bit.  tests/test_gpu_raster_var.py runs the shapes on the GPU;
tests/test_raster_var_cases.py checks on the CPU that the staged reference equals the direct diagonal of T^T S T and that each shape
still reaches the tile and chunk edges it was chosen for.
"""
from __future__ import annotations

import functools

import numpy as np

TILE, BK = 64, 16                 # output tile and k-tile of vg_krq_kernel

# (m1, m2, P1, P2)
SHAPES = (
    (5, 7, 6, 9),                 # the identity's first check
    (1, 1, 1, 1),
    (3, 66, 65, 67),              # m2^2 = 4356: 69 row tiles; view tiles straddle j boundaries (66 does not divide 64); tile edges on both
    #                               raster axes; P1 = 65 passes the m1^2 = 9 chunk seven times
    (17, 4, 64, 128),             # K = 289 is no multiple of 4; m2^2 = 16 rows: less than one tile
    (16, 16, 300, 1),             # two chunks of 256 and 44 columns, one raster column
)
# P1 across the chunk edges of m1 = 3 (chunk = 9): 1, chunk - 1, chunk, chunk + 1, 2 chunk + 1
CHUNK_EDGE_M = (3, 5)
CHUNK_EDGE_P2 = 9


def chunk(m1, P1):
    """include/vggp.h: the P1 axis is processed in chunks of min(P1, m1^2) columns."""
    return min(P1, m1 * m1)


def chunk_edge_P1(m1):
    c = m1 * m1
    return (1, c - 1, c, c + 1, 2 * c + 1)


def operands(m1, m2, P1, P2, seed=0):
    """-> S [M, M] (not symmetric), U1 [m1, P1], U2 [m2, P2], n1 [P1], n2 [P2]: int64 in {-2, ..., 2}."""
    rng = np.random.default_rng([seed, m1, m2, P1, P2])
    M = m1 * m2
    S = rng.integers(-2, 3, (M, M))
    if M > 1:
        S[0, 1], S[1, 0] = 2, -1          # not symmetric whatever the draw
    return S, rng.integers(-2, 3, (m1, P1)), rng.integers(-2, 3, (m2, P2)), rng.integers(-2, 3, P1), rng.integers(-2, 3, P2)


def quadform(S, U1, U2):
    """int64 einsum of the bare quadratic form -> [P1, P2] (one axis at a time: the direct four-index einsum is the same integers)."""
    m1, m2 = U1.shape[0], U2.shape[0]
    S4 = np.asarray(S, dtype=np.int64).reshape(m1, m2, m1, m2)
    G = np.einsum("ia,ka,ijkl->jla", U1.astype(np.int64), U1.astype(np.int64), S4, optimize=True)
    return np.einsum("jla,jb,lb->ab", G, U2.astype(np.int64), U2.astype(np.int64), optimize=True)


def quadform_direct(S, U1, U2):
    """diag(T^T S T) with the columns t_ab = u1_a (x) u2_b written out (small shapes only)."""
    T = np.einsum("ia,jb->ijab", U1.astype(np.int64), U2.astype(np.int64)).reshape(U1.shape[0] * U2.shape[0], -1)
    return np.einsum("up,uv,vp->p", T, np.asarray(S, dtype=np.int64), T).reshape(U1.shape[1], U2.shape[1])


@functools.lru_cache(maxsize=None)
def case(m1, m2, P1, P2):
    """-> (operands, int64 reference of the bare form): computed once, shared, read-only."""
    ops = operands(m1, m2, P1, P2)
    return ops, quadform(*ops[:3])
