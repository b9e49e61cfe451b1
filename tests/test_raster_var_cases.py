"""CPU checks of tests/raster_var_cases.py: the staged int64 reference is the direct diagonal of T^T S T, every partial sum stays exact
in fp64, and each shape still reaches the tile and chunk edges it was chosen for."""
import numpy as np

import raster_var_cases as RV


def _cdiv(a, b):
    return (a + b - 1) // b


def test_staged_reference_is_the_direct_quadratic_form():
    for shape in ((5, 7, 6, 9), (1, 1, 1, 1), (3, 4, 11, 2)):
        (S, U1, U2, _, _), ref = RV.case(*shape)
        assert ref.dtype == np.int64 and np.array_equal(ref, RV.quadform_direct(S, U1, U2))
        assert np.array_equal(RV.quadform(S.T, U1, U2), ref)          # a quadratic form does not see the antisymmetric part ...
    S, U1, U2, _, _ = RV.operands(5, 7, 6, 9)
    assert not np.array_equal(S, S.T)                                 # ... which the operands do have


def test_sums_are_exact_in_fp64():
    for m1, m2, P1, P2 in RV.SHAPES:
        assert 32 * (m1 * m2) ** 2 < 2 ** 53
        (S, U1, U2, n1, n2), ref = RV.case(m1, m2, P1, P2)
        assert max(np.abs(a).max() for a in (S, U1, U2, n1, n2)) <= 2 and np.abs(ref).max() <= 32 * (m1 * m2) ** 2


def test_shapes_reach_their_edges():
    s = {sh: sh for sh in RV.SHAPES}
    m1, m2, P1, P2 = s[(3, 66, 65, 67)]
    assert _cdiv(m2 * m2, RV.TILE) == 69 and RV.TILE % m2 != 0 and (m2 * m2) % RV.TILE != 0
    assert P1 % RV.TILE != 0 and P2 % RV.TILE != 0 and P2 > RV.TILE and _cdiv(P1, RV.chunk(m1, P1)) == 8
    m1, m2, P1, P2 = s[(17, 4, 64, 128)]
    assert (m1 * m1) % 4 != 0 and m2 * m2 < RV.TILE and (m2 * m2) % 4 == 0 and RV.chunk(m1, P1) == P1
    m1, m2, P1, P2 = s[(16, 16, 300, 1)]
    assert RV.chunk(m1, P1) == 256 and P1 - 256 == 44 and (m1 * m1) % RV.BK == 0
    assert RV.chunk(1, 1) == 1 and RV.chunk(5, 6) == 6
    m1 = RV.CHUNK_EDGE_M[0]
    assert RV.chunk_edge_P1(m1) == (1, 8, 9, 10, 19) and [_cdiv(p, RV.chunk(m1, p)) for p in RV.chunk_edge_P1(m1)] == [1, 1, 1, 2, 3]
