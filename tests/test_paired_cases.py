"""CPU premises of tests/paired_cases.py, the tables behind tests/test_gpu_paired_paths.py: every shape still reaches the tile / split
path it was chosen for, Kuu takes no jitter and stays below cond 1e8, and the recorded reference floors are reproduced."""
import numpy as np
import pytest
import torch

import general_z_spec as S
import paired_cases as P


def test_scattered_split_table():
    """Family A: (ns1, kchunk, empty slabs, tn_per, runs2) of every shape -- a shape must not silently stop reaching its path."""
    for (M, N), want in P.A_EXPECT.items():
        assert P.split_scattered(M, N) == want, (M, N)
        assert f"A_{M}_{N}" in P.CASES
    # what the table's rows are there for, spelled out
    ns1, kchunk, _, _, _ = P.split_scattered(17, 1030)
    assert ns1 == 2 and 1030 - kchunk == 502 and 502 % P.PZ_BK != 0               # second slab ragged against the k-tile
    assert P.split_scattered(64, 1024)[:3] == (2, 512, 0) and 512 % P.PZ_T == 0    # slabs exact, nothing ragged
    ns1, kchunk, empty, _, _ = P.split_scattered(20, 32769)
    assert 32769 - 62 * kchunk == 33 and 63 * kchunk >= 32769 and empty == 1      # slab 62 holds 33 points, slab 63 none
    assert P.split_scattered(130, 65537)[2] == 3                                   # three empty trailing slabs
    for M, N, tn_per, tiles_last in ((8, 524353, 2, 2), (8, 1048641, 3, 3), (65, 262209, 2, 2)):
        got = P.split_scattered(M, N)
        assert got[3] == tn_per and P.last_run(N, tn_per) == (tiles_last, 1)       # pass-2 runs; the last tile holds one point
    assert P.split_scattered(8, 524353)[4] == 4097 and P.split_scattered(8, 1048641)[4] == 5462
    # ... and the run that is cut short (tn_last clamped to the last tile): one tile of one point
    assert P.split_scattered(8, 524289)[3:] == (2, 4097) and P.last_run(524289, 2) == (1, 1)
    # tile counts in M: triangle tiles of pass 1 and Cholesky panels
    tiles = lambda M: -(-M // P.PZ_T) * (-(-M // P.PZ_T) + 1) // 2
    assert [tiles(M) for M in (63, 64, 65, 128, 129, 257)] == [1, 1, 3, 3, 6, 15]
    assert [-(-M // P.PZ_MB) for M in (127, 128, 129, 257)] == [1, 1, 2, 3]


def test_grid_split_table():
    for (M, shape), want in P.C_EXPECT.items():
        assert P.split_grid(M, *shape) == want, (M, shape)
    assert P.split_grid(65, 70, 45) == (1, 1)


@pytest.mark.parametrize("name", list(P.CASES))
def test_case_premises_and_floors(name):
    """Jitter 0, cond(Kuu) <= 1e8; the recorded floors are reproduced within a factor 10 and lie 100 times below their ceilings."""
    ref = P.reference(name)
    assert ref["step"]["jitter"] == 0.0
    assert P.kuu_cond(ref["p"]) <= 1e8
    got, rec = P.measure_floors(name), P.FLOORS[name]
    assert set(got) == set(rec)
    for q in rec:
        # (below 1e-14 a floor does not move the bound max(100 floor, 1e-12): compared from there upwards)
        a, b = max(got[q], 1e-14), max(rec[q], 1e-14)
        assert a <= 10.0 * b and b <= 10.0 * a, (q, got[q], rec[q])
        ceil = P.CEIL[q[5:] if q.startswith("twin_") else q]
        assert 100.0 * rec[q] <= ceil, (q, rec[q])          # otherwise the case is mis-chosen: change the case, not the ceiling
        assert P.bound(name, q) <= ceil


def test_duplicate_point_case_takes_jitter():
    p = P.duplicate_problem()
    assert P.spec_step(p)["jitter"] > 0


def test_coincide_cases_contain_exact_coincidences():
    p = P.case_problem("B_s_coincide")
    h = p["M"] // 2
    assert np.array_equal(p["Z"][:h], p["X"][:h])                                       # d = 0 in both dimensions at (i, i)
    assert not np.any(np.all(p["Z"][:, None, :] == p["X"][None, h:, :], axis=2))
    p = P.case_problem("B_g_coincide")
    assert np.isin(p["Z"][:h, 0], p["x1"]).all() and np.isin(p["Z"][:h, 1], p["x2"]).all()
    assert len({tuple(z) for z in p["Z"]}) == p["M"]                                    # ... and no two inducing points coincide
    # the specification differentiates |d| to 0 there, as the kernels' sg = 0 does
    d = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(torch.abs(d).sum(), d)
    assert g.item() == 0.0


def test_tables_cover_the_families():
    assert len(P.A_CASES) == 19 and len(P.B_CASES) == 16 and len(P.C_CASES) == 5 and len(P.D_CASES) == 12
    assert {P.CASES[n]["M"] for n in P.READOUT_CASES} == {17, 65, 129}
    assert {P.CASES[n]["kinds"] for n in P.READOUT_CASES if P.CASES[n]["layout"] == "grid"} == set(P.EQUAL + P.MIXED)
    for M in (17, 65, 129):
        assert {P.CASES[n]["kinds"] for n in P.READOUT_CASES if P.CASES[n]["layout"] == "scattered" and P.CASES[n]["M"] == M} == \
            set(P.EQUAL + P.MIXED)
