"""CPU check of the specification of the iterative masked step's read-outs (tests/masked_iter_readout_spec.py: block PCG on
rank-one right-hand sides, no M x M matrix) against the dense masked oracle (oracle/kron.py q_v_masked, posterior_masked)."""
import numpy as np
import pytest

import masked_iter_readout_spec as S
from oracle import dense as D
from oracle import kron as Kr
from variational_gridded_gaussian_processes_amd import datagen as G

N = 96
THETA = [0.2, 0.3, 1.0, 0.8, 0.01]
BASES = [("b0", "matern12", np.linspace(0, 1, 13)), ("points", "matern32", np.linspace(0, 1, 10)),
         ("points", "rbf", np.linspace(0, 1, 10))]
MASKS = {"bernoulli": lambda: (np.random.default_rng(1).uniform(size=(N, N)) < 0.7).astype(np.float64),
         "track": lambda: G.track_mask(N, N, 2, 0.5)}


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("case", BASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_spec_readouts_equal_the_dense_masked_oracle(case, mask):
    """mean <= 1e-8, variance <= 1e-9 of the largest entry at tol = 1e-10 (measured: 6.6e-10 / 1.1e-12 at worst, 8-10 iterations)."""
    basis, kind, g = case
    _, y, x1, x2 = D.gen_grid(N, N)
    Wn = MASKS[mask]()
    f1, f2 = Kr.Factor(basis, kind, g, x1), Kr.Factor(basis, kind, g, x2)
    ref = Kr.elbo_step_masked(y.reshape(N, N), Wn, f1, f2, THETA)
    st = S.prepare(y.reshape(N, N), Wn, f1, f2, THETA, tol=1e-10)
    mean, var, info = S.q_v(st, f1, f2, tol=1e-10)
    rm, rv = Kr.q_v_masked(ref, f1, f2)
    print(f"{basis}-{kind}-{mask}: q(v) mean {rel(mean, rm):.1e} var {rel(var, rv.reshape(-1)):.1e} its {info['rounds']}")
    assert rel(mean, rm) <= 1e-8
    assert rel(var, rv.reshape(-1)) <= 1e-9
    xs = np.random.default_rng(9).uniform(0, 1, (70, 2))
    pm, pv, pinfo = S.posterior(st, f1, f2, xs, tol=1e-10)
    om, ov = Kr.posterior_masked(ref, f1, f2, xs)
    print(f"{basis}-{kind}-{mask}: posterior mean {rel(pm, om):.1e} var {rel(pv, ov):.1e} its {pinfo['rounds']}")
    assert rel(pm, om) <= 1e-8
    assert rel(pv, ov) <= 1e-9
    assert pinfo["solves"] == 2                       # 70 points: a full block of 64 and a ragged one of 6


def test_spec_blocks_and_cell_subsets_agree():
    """The block width only groups the columns, and a list of cells gives the same entries as the all-cell call."""
    basis, kind, g = BASES[0]
    _, y, x1, x2 = D.gen_grid(N, N)
    Wn = MASKS["bernoulli"]()
    f1, f2 = Kr.Factor(basis, kind, g, x1), Kr.Factor(basis, kind, g, x2)
    st = S.prepare(y.reshape(N, N), Wn, f1, f2, THETA)
    _, var_all, _ = S.q_v(st, f1, f2)
    cells = np.random.default_rng(4).choice(144, size=37, replace=False)
    _, v16, i16 = S.q_v(st, f1, f2, cells=cells, block=16)
    _, v64, i64 = S.q_v(st, f1, f2, cells=cells, block=64)
    assert (i16["solves"], i64["solves"]) == (3, 1)
    assert rel(v16, v64) <= 1e-12 and rel(v16, var_all[cells]) <= 1e-12
