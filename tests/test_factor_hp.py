"""The numpy oracle's factor builders (oracle/kron.py: points_factor, b0_A, b0_K, b0_K_f32, vff_A, vff_K, b1_A, b1_K) against
50-digit values of the same elements (tests/golden/factor_hp.npz, written by tests/golden/make_factor_hp.py from the definitions:
cell integrals by quadrature, kernel profiles, mp.diff for d/d ell).  "Parity with the oracle" is what pins the HIP kernel
elsewhere; this file is what pins the oracle -- at lengthscales from 1/2000 to 3.2e4 mesh spacings, on knots, mesh ends, points
outside the mesh and distances where exp() underflows.

Bound per element: |oracle - hp| <= c eps S with c = 4 max(R_oracle, 1) (factor_hp_cases.py).  R_oracle is this very oracle's
worst err / (eps S) per case as measured when the fixture was written (libm of that machine); the test prints the value it
measures now beside the stored one.  Stored values over all cases: R_oracle <= 3.8 (pairwise), <= 0.7 (B0, with and without
VGGP_FLAG_B0_F32_KDELTA), <= 1.0 (VFF), <= 1.6 (B1) -- i.e. c = 4 for all but some pairwise Matern-3/2, -5/2 and RBF cases
(c <= 15) and the B1 Kuu on the float32-born mesh at the two largest lengthscales (c <= 6.4).
"""
import numpy as np
import pytest

import factor_hp_cases as H
from oracle import kron as Kr


@pytest.mark.parametrize("c", H.cases(), ids=H.case_ids())
def test_oracle_factors_vs_50_digits(c):
    got = H.sample(c, H.oracle_outputs(c.kind, c.basis, c.grid, c.x, c.ell, c.flags))
    now = {k: H.ratio_to_bound(got[k], c.hp[k], c.S[k]) for k in H.OUTPUTS}
    print(f"{c.id}: err / (eps S) now " + " ".join(f"{k} {now[k]:.2f}" for k in H.OUTPUTS) + f"; stored R_oracle {c.R_oracle:.2f}")
    for k in H.OUTPUTS:
        assert now[k] <= H.tolerance_constant(c), (k, now[k])


def test_fixture_covers_the_edges_the_issue_names():
    """both mesh ends, interior knots, points outside on both sides, distance 0, a distance where exp underflows -- in every case"""
    ratios = set()
    for c in H.cases():
        ratios.add(c.ratio)
        lo, hi = (c.grid[0], c.grid[1]) if c.basis == "vff" else (c.grid[0], c.grid[-1])
        assert lo in c.x and hi in c.x and (c.x < lo).any() and (c.x > hi).any()
        if c.basis != "vff":
            assert np.isin(c.grid[1:-1], c.x).sum() >= 3
        assert (np.abs(c.x - lo).max() / c.ell > 760.0)                      # exp(-760) is below the smallest subnormal
        if c.basis == "points":
            assert (c.hp["K0"] == 1.0).any() and (c.hp["A0"] == 1.0).any()    # distance 0: on the diagonal and at x == z
    assert ratios == {"1/2000", "1/700", "1/100", "1", "30", "320", "3.2e4"}
    assert {(c.basis, c.flags) for c in H.cases()} == {("points", 0), ("b0", 0), ("b0", 1), ("vff", 0), ("b1", 0)}
    assert {c.kind for c in H.cases() if c.basis == "points"} == {"matern12", "matern32", "matern52", "rbf"}


@pytest.mark.parametrize("c", [c for c in H.cases() if c.basis == "points" or (c.basis == "b0" and c.flags == 0)],
                         ids=[c.id for c in H.cases() if c.basis == "points" or (c.basis == "b0" and c.flags == 0)])
def test_float64_summand_scales_equal_the_stored_ones(c):
    """factor_hp_cases.S_points / S_b0_A / S_b0_K (the scales the whole-matrix GPU comparisons use) restate the fixture's S"""
    if c.basis == "points":
        SA, SK = H.S_points(c.kind, c.grid, c.x, c.ell), H.S_points(c.kind, c.grid, c.grid, c.ell)
    else:
        SA, SK = H.S_b0_A(c.grid, c.x, c.ell), H.S_b0_K(len(c.grid) - 1, float(c.grid[1] - c.grid[0]), c.ell)
    got = H.sample(c, (SA[0], SA[1], SK[0], SK[1]))
    for k in H.OUTPUTS:
        assert np.allclose(got[k], c.S[k], rtol=1e-9, atol=0.0), k


def test_b0_K_is_finite_below_the_old_overflow():
    """e^{-kt} 4 sinh^2(t/2) overflowed for t = delta/ell > 710 (OverflowError in numpy, inf * 0 = NaN on the device); the
    expm1 form has no growing factor: the neighbour-cell covariance tends to ell^2, everything further out underflows to 0."""
    delta = 1.0 / 32
    for ell in (2.3e-5, 1e-5, 1e-7):
        K, dK = Kr.b0_K(3, delta, ell)
        assert np.isfinite(K).all() and np.isfinite(dK).all()
        assert K[0, 1] == pytest.approx(ell * ell, rel=1e-15) and K[0, 2] == 0.0
        assert K[0, 0] == pytest.approx(2 * ell * (delta - ell), rel=1e-15)
        Kf, _ = Kr.b0_K_f32(3, delta, ell)
        assert K[0, 1] == pytest.approx(Kf[0, 1], rel=1e-15)
