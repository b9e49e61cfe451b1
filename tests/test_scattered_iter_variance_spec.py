"""CPU: the specification of the variance read-outs of the iterative scattered step (tests/scattered_iter_variance_spec.py) against the
dense scattered oracle, Kr.elbo_step_scattered -> Kr.q_v_masked / Kr.posterior_masked.  Conditions: means 1e-7, variances 1e-6 of the
largest entry (what a PCG tolerance of 1e-10 has to deliver), every column converged in fewer than 30 iterations.

Measured: rand20k m = 8 theta_a -- q(v) mean 5.3e-11, variance 4.2e-15, posterior mean 7.1e-11, variance 1.1e-16, 8 / 8 iterations;
trk400 m = 12 theta_b -- 2.0e-11, 2.6e-15, 1.3e-11, <= 1e-16, 8 / 8 iterations (the means carry the error of a0 at tol 1e-10)."""
import numpy as np
import pytest

from oracle import kron as Kr

import scattered_iter_variance_spec as V

XS = np.random.default_rng(9).uniform(0, 1, (70, 2))
CASES = {"rand20k_m8_a": (V.rand20k, 8, V.THETA_A), "trk400_m12_b": (lambda: V.trk(400, 0.5), 12, V.THETA_B)}


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("case", list(CASES))
def test_spec_vs_dense_scattered_oracle(case):
    gen, m, theta = CASES[case]
    X, y = gen()
    f1, f2 = V.b0_factors(m)
    ref = Kr.elbo_step_scattered(X, y, f1, f2, theta)
    rm, rv = Kr.q_v_masked(ref, f1, f2)
    om, ov = Kr.posterior_masked(ref, f1, f2, XS)
    st = V.prepare(X, y, f1, f2, theta)
    mean, var, info = V.q_v(st, f1, f2)
    pm, pv, pinfo = V.posterior(st, f1, f2, XS)
    errs = (rel(mean, rm), rel(var, rv.reshape(-1)), rel(pm, om), rel(pv, ov))
    print(f"{case}: q(v) mean {errs[0]:.1e} var {errs[1]:.1e}; posterior mean {errs[2]:.1e} var {errs[3]:.1e}; "
          f"iterations {info['rounds']} / {pinfo['rounds']}, solves {info['solves']} / {pinfo['solves']}")
    assert errs[0] <= 1e-7 and errs[2] <= 1e-7
    assert errs[1] <= 1e-6 and errs[3] <= 1e-6
    assert info["converged"] and pinfo["converged"]
    assert 0 < info["rounds"] < 30 and 0 < pinfo["rounds"] < 30
    assert info["solves"] == -(-m * m // 64) and pinfo["solves"] == 2
    # a list of cells is the same columns: a column's numbers do not depend on its neighbours in the block
    cells = np.array([0, m * m - 1, 5, 17, 3])
    _, sub, sinfo = V.q_v(st, f1, f2, cells=cells, block=2)
    assert sinfo["solves"] == 3 and rel(sub, var[cells]) <= 1e-12
