"""CPU premises of tests/masked_dense_cases.py, the tables behind tests/test_gpu_masked_dense_paths.py: every shape still reaches the
launch edge, slab count, panel count or chunk count it was chosen for, the slab scratch of the dense masked step holds what its users
write (and did not before it was sized for them), the recorded reference floors are reproduced, and the per-component error measure
sees what the max-norm does not."""
import numpy as np
import pytest

import masked_dense_cases as P


def _shape(name):
    """(n1, n2, m1, m2) of a masked case as planned (a twin: transposed)."""
    p = P.case_problem(name)
    return p["n1"], p["n2"], P.factors(p)[0].m, P.factors(p)[1].m


def test_replica_tables():
    # gemm_longk: no split below K = 1024, K // 512 slabs from there, empty splits dropped, 256 at the most
    assert [P.longk_slabs(K) for K in (1, 512, 1023, 1024, 1535, 1536, 2048, 4096)] == [1, 1, 1, 2, 2, 3, 4, 8]
    # 131 072 = 256 x 512: 8192 k-tiles, 32 a slab, all 256 slabs full.  131 584 = 257 x 512 asks for 257, is capped at 256, and its
    # 8224 k-tiles at 33 a slab fill 250 slabs: six empty splits dropped
    assert P.longk_slabs(131072) == 256 and P.longk_slabs(131584) == 250 and -(-8224 // 33) == 250
    # vgm_wcol_part: 64 slabs for m2 = 8
    assert P.wcol_slabs(1, 8) == (64, 1, 63) and P.wcol_slabs(2, 8) == (64, 1, 62)
    assert P.wcol_slabs(63, 8) == (64, 1, 1) and P.wcol_slabs(65, 8) == (64, 2, 31)
    assert P.wcol_slabs(40, 6) == (36, 2, 16) and P.wcol_slabs(3, 4) == (16, 1, 13)
    assert [P.chol_panels(M) for M in (127, 128, 129, 256, 258)] == [1, 1, 2, 2, 3]
    assert [P.readout_chunks(ns, 35) for ns in (1, 34, 35, 36, 70, 71)] == [1, 1, 1, 2, 2, 3]


def test_cases_reach_what_they_were_chosen_for():
    # A: 1-D launch / 256-stride edges in n1 (and, transposed, in n2), both with fewer rows than column slabs
    for n1 in (255, 256, 257):
        assert _shape(f"A_{n1}x3_5x4") == (n1, 3, 5, 4) and _shape(f"A_{n1}x3_5x4_T") == (3, n1, 4, 5)
        assert P.wcol_slabs(3, 4)[2] == 13 and P.wcol_slabs(n1, 5)[0] == 25
    # A: vgm_wcol_part with 64 slabs and 1, 2, 63, 65 rows: 63, 62, 1 empty slabs; 65 rows is the first count with two rows per slab
    assert [P.wcol_slabs(_shape(f"A_40x{n2}_6x8")[1], 8)[1:] for n2 in (1, 2, 63, 65)] == [(1, 63), (1, 62), (1, 1), (2, 31)]
    # A: long-K thresholds of PT1 (PT2 in the twin)
    assert [P.longk_slabs(_shape(f"A_{n1}x8_6x3")[0]) for n1 in (1023, 1024, 1535, 1536)] == [1, 2, 2, 3]
    assert [P.longk_slabs(_shape(f"A_{n1}x8_6x3_T")[1]) for n1 in (1023, 1024, 1535, 1536)] == [1, 2, 2, 3]
    # C: panels of the blocked factor
    assert [P.chol_panels(np.prod(_shape(n)[2:])) for n in ("C_128", "C_129", "C_258", "C_129_pts32")] == [1, 2, 3, 2]
    assert [_shape(n)[2] * _shape(n)[3] for n in ("C_128", "C_129", "C_258")] == [128, 129, 258]
    # D: slab counts of the scattered step's long-K products
    assert [P.longk_slabs(N) for N in P.D_N] == [1, 1, 1, 1, 1, 1, 1, 2, 3, 256, 250]
    assert 131584 // 512 == 257                          # ... the last one past the cap
    assert P.case_problem("D_5")["N"] < 18
    # B / E: observation counts
    assert P.case_problem("B_few")["N"] == 20 < P.M_E and P.case_problem("B_one_cell")["N"] == 1
    assert P.case_problem("B_ones")["N"] == 1440 and 100 < P.case_problem("B_track")["N"] < 720
    W = P.case_problem("B_empty_row")["W"]
    assert (W.sum(1) == 0).sum() == 1 and (W.sum(0) == 0).sum() == 0
    W = P.case_problem("B_empty_col")["W"]
    assert (W.sum(1) == 0).sum() == 0 and (W.sum(0) == 0).sum() == 1
    W = P.case_problem("B_single_row")["W"]
    assert (W.sum(1) > 0).sum() == 1 and W.sum() == 40
    # E: chunk counts of the read-outs at M = 35
    assert [P.readout_chunks(ns, P.M_E) for ns in P.NS_POST] == [1, 1, 1, 2, 3]
    assert [P.readout_chunks(a * b, P.M_E) for a, b in P.MV] == [1, 1, 2, 3] and [a * b for a, b in P.MV] == [1, 35, 36, 72]
    p = P.case_problem("D_dup_outside")
    assert len(np.unique(p["X"], axis=0)) == p["N"] - 40


def test_tables_cover_the_families():
    assert len(P.A_CASES) == 30 and len(P.B_CASES) == 10 and len(P.C_CASES) == 4 and len(P.D_CASES) == 16 and len(P.E_CASES) == 5
    assert set(P.FLOORS) == set(P.CASES)
    for name in P.CASES:
        assert set(P.FLOORS[name]) == set(P.quantities(name)), name


@pytest.mark.parametrize("name", [n for n, c in P.CASES.items() if c["layout"] == "masked"])
def test_slab_scratch_fits(name):
    """Every user of the dense masked step's T buffer fits what vgm_layout gives it."""
    s = _shape(name)
    assert P.scratch_need(*s) <= P.new_capacity(*s)


def test_slab_scratch_cases_overran_the_parent_layout():
    """The four slab-scratch shapes need more than the assembly's n1 m2^2 doubles, which is all the buffer held before.  In the two
    whose PT1 product splits (m1 >> m2) the slabs ran past Tv, UB and UV into Zb -- written just before, read by the RJ_Z1 / RJ_Z2
    reductions just after: silent corruption of the lengthscale gradients.  In the two whose PT2 product splits (n2 >> n1) they ended
    inside Tv / UB, which are dead by then: over the buffer, but harmless."""
    for name in P.SLAB_SCRATCH:
        s = _shape(name)
        assert P.scratch_need(*s) > P.parent_capacity(*s), name
        assert P.new_capacity(*s) == P.scratch_need(*s)
    for name in ("A_1024x32_96x2", "A_1024x16_48x1"):
        s = _shape(name)
        assert P.scratch_users(*s)["PT1"] > P.parent_room_to_Zb(*s), name
    for name in ("A_3x4096_4x16", "A_2x2048_4x32"):
        s = _shape(name)
        assert P.parent_capacity(*s) < P.scratch_users(*s)["PT2"] <= P.parent_room_to_Zb(*s), name
    # the issue's third example, not a GPU case (its assembly is 2 M^2 = 8 MB a matrix): Zb fully overwritten
    assert P.scratch_users(1024, 64, 256, 4)["PT1"] - P.parent_room_to_Zb(1024, 64, 256, 4) >= 1024 * 64
    # the twins do not overrun (PT2 splits there, and n1 m2^2 is large), and neither do the config-5 shapes: no growth
    for name in P.SLAB_SCRATCH[:2]:
        s = _shape(name + "_T")
        assert P.scratch_need(*s) == P.parent_capacity(*s)
    assert P.masked_arena_growth_bytes(2048, 2048, 32, 32) == 0 and P.masked_arena_growth_bytes(1024, 1024, 128, 128) == 0
    assert P.masked_arena_growth_bytes(1024, 32, 96, 2) == 8 * (18432 - 4096)


@pytest.mark.parametrize("name", list(P.CASES))
def test_floors_reproduced(name):
    """The recorded floors are reproduced within a factor 3 and lie 100 times below their ceilings."""
    got, rec = P.measure_floors(name), P.FLOORS[name]
    assert set(got) == set(rec)
    for q in rec:
        # (below 1e-14 a floor does not move the bound max(100 floor, 1e-12): compared from there upwards)
        a, b = max(got[q], 1e-14), max(rec[q], 1e-14)
        assert a <= 3.0 * b and b <= 3.0 * a, (q, got[q], rec[q])
        assert 100.0 * rec[q] <= P.ceil(name, q), (q, rec[q])          # otherwise the case is mis-chosen: change the case, not the ceiling
        assert 1e-12 <= P.bound(name, q) <= P.ceil(name, q)


def test_per_component_measure_sees_a_wrong_lengthscale_gradient():
    """A gradient whose d/dell1 is off by 1e-4 of itself passes the max-norm measure at 1e-7 and fails the per-component one."""
    for name in ("A_1024x32_96x2", "A_1024x16_48x1", "D_1024_96x2"):         # (the anisotropic shapes: d/dell1 is 1200 - 1500 times smaller)
        g = P.reference(name)["grad"]
        assert np.abs(g).max() > 1e3 * abs(g[0])
        bad = g.copy()
        bad[0] *= 1.0 + 1e-4
        assert P.rel(bad, g) < 1e-7
        each = P.rel_each(bad, g)
        assert each[0] > 0.99e-4 > P.bound(name, "g_l1") and (each[1:] == 0).all()
