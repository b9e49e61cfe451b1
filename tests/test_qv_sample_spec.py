"""CPU check of the specification of the joint samples of q(v) (tests/qv_sample_spec.py): the Philox generator against published
known answers, the normal map's moments, and the three samplers against the dense oracles by the unit-noise identity
    sum_s (V_s - mean)(V_s - mean)^T = Cov q(v)     when the noise runs over the unit vectors of (E, F).
Bound of the identity: 1e-8 of the largest entry of the dense covariance, the bound the existing spec tests give a PCG-produced mean
(tests/test_masked_iter_readout_spec.py).  Measured: masked 1.6e-11 .. 2.4e-11, 16 iterations at tol 1e-10."""
import numpy as np
import pytest

import masked_iter_readout_spec as MS
import qv_sample_cases as Cs
import qv_sample_spec as S
import scattered_iter_variance_spec as SS
from oracle import kron as Kr


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    assert _hex(S.philox4x32_10([0, 0, 0, 0], [0, 0])) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert _hex(S.philox4x32_10([f, f, f, f], [f, f])) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(S.philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_element_depends_on_its_index_alone():
    whole = S.normal_fill(7, 1, 0, 1001)
    for first, n in ((0, 1), (1, 1), (3, 500), (503, 498), (999, 2)):
        assert np.array_equal(S.normal_fill(7, 1, first, n), whole[first:first + n])
    assert not np.array_equal(S.normal_fill(7, 0, 0, 64), whole[:64])          # another stream: other numbers
    assert not np.array_equal(S.normal_fill(8, 1, 0, 64), whole[:64])          # another seed likewise
    big = 2**40 + 5                                                            # the high counter word is in use
    assert np.array_equal(S.normal_fill(7, 1, big, 4)[1:], S.normal_fill(7, 1, big + 1, 3))
    assert np.abs(whole).max() <= 8.66


def test_moments():
    n = 2**20
    z = S.normal_fill(2024, 0, 0, n)
    print(f"mean {z.mean():+.5f} var {z.var():.5f} max |z| {np.abs(z).max():.3f}")
    assert abs(z.mean()) <= 5.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    z = S.normal_fill(12345, 0, 0, 20000)
    print(f"seed 12345, 20000 draws: mean {z.mean():+.4f} var {z.var():.4f}")
    assert abs(z.mean()) <= 5.0 / np.sqrt(20000) and abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / 20000)


@pytest.mark.parametrize("case", Cs.KERNEL_BASES + ["b1-matern12"])
def test_masked_unit_noise_identity(case):
    Y, W, x1, x2 = Cs.grid_data()
    f1, f2 = Cs.factors(case, x1, x2)
    ref = Kr.elbo_step_masked(Y, W, f1, f2, Cs.THETA)
    cov = Kr.q_v_cov_masked(ref, f1, f2)
    st = MS.prepare(Y, W, f1, f2, Cs.THETA, tol=1e-10)
    eps_u, eps_obs = Cs.unit_noise(f1.m, f2.m, (Cs.N2, Cs.N1))
    out, info = S.sample_masked(st, f1, f2, eps_u, eps_obs, tol=1e-10)
    mean, _, _ = MS.q_v(st, f1, f2, cells=[0])          # the sampler's own mean (its a0 is a PCG result: 1e-10 off the oracle's)
    err = Cs.rel(Cs.outer_sum(out, mean), cov)
    print(f"{case}: {eps_u.shape[0]} unit samples, identity {err:.1e}, {info['rounds']} iterations, {info['solves']} solves")
    assert info["converged"] and err <= 1e-8
    # the columns whose noise falls on unobserved nodes have a zero right-hand side: they return the mean itself
    M = f1.m * f2.m
    dead = M + np.flatnonzero(W.reshape(-1) == 0)
    assert len(dead) > 0 and all(np.array_equal(out[s], mean) for s in dead)


@pytest.mark.parametrize("case", Cs.KERNEL_BASES)
def test_scattered_unit_noise_identity(case):
    X, y = Cs.scattered_data()
    f1, f2 = Cs.factors(case, X[:, 0], X[:, 1])
    ref = Kr.elbo_step_scattered(X, y, f1, f2, Cs.THETA)
    cov = Kr.q_v_cov_masked(ref, f1, f2)
    st = SS.prepare(X, y, f1, f2, Cs.THETA, tol=1e-10)
    mean, _, _ = SS.q_v(st, f1, f2, cells=[0])          # the sampler's own mean
    eps_u, eps_obs = Cs.unit_noise(f1.m, f2.m, (Cs.NPTS,))
    out, info = S.sample_scattered(st, f1, f2, eps_u, eps_obs, tol=1e-10)
    err = Cs.rel(Cs.outer_sum(out, mean), cov)
    print(f"{case}: {eps_u.shape[0]} unit samples, identity {err:.1e}, {info['rounds']} iterations")
    assert info["converged"] and err <= 1e-8


@pytest.mark.parametrize("case", Cs.KERNEL_BASES + ["b1-matern12"])
def test_full_grid_symmetric_root_identity(case):
    Y, _, x1, x2 = Cs.grid_data()
    f1, f2 = Cs.factors(case, x1, x2)
    st = Kr.elbo_step(Y, f1, f2, Cs.THETA)
    mean, _ = Kr.q_v(st)
    M = f1.m * f2.m
    out = S.sample_full(st, np.eye(M).reshape(M, f1.m, f2.m))
    err = Cs.rel(Cs.outer_sum(out, mean), Kr.q_v_cov(st))
    print(f"{case}: full grid identity {err:.1e}")
    assert err <= 1e-8


def test_zero_noise_returns_the_mean():
    Y, W, x1, x2 = Cs.grid_data()
    f1, f2 = Cs.factors("b0-matern12", x1, x2)
    st = MS.prepare(Y, W, f1, f2, Cs.THETA)
    out, info = S.sample_masked(st, f1, f2, np.zeros((3, f1.m, f2.m)), np.zeros((3, Cs.N2, Cs.N1)))
    mean, _, _ = MS.q_v(st, f1, f2, cells=[0])
    assert all(np.array_equal(o, mean) for o in out) and info["rounds"] == 0
    full = Kr.elbo_step(Y, f1, f2, Cs.THETA)
    assert np.array_equal(S.sample_full(full, np.zeros((2, f1.m, f2.m)))[1], Kr.q_v(full)[0])
    X, y = Cs.scattered_data()
    g1, g2 = Cs.factors("b0-matern12", X[:, 0], X[:, 1])
    sst = SS.prepare(X, y, g1, g2, Cs.THETA)
    outs, _ = S.sample_scattered(sst, g1, g2, np.zeros((1, g1.m, g2.m)), np.zeros((1, Cs.NPTS)))
    assert np.array_equal(outs[0], SS.q_v(sst, g1, g2, cells=[0])[0])


def test_generated_noise_is_the_explicit_noise_and_blocks_only_group():
    """sample(seed, first) is sample(eps = the generator's numbers); block widths and the first sample only group the columns."""
    Y, W, x1, x2 = Cs.grid_data()
    f1, f2 = Cs.factors("b0-matern12", x1, x2)
    st = MS.prepare(Y, W, f1, f2, Cs.THETA)
    m1, m2 = f1.m, f2.m
    eu, eo = S.noise_u(3, 0, 9, m1, m2), S.noise_obs_grid(3, 0, 9, Cs.N1, Cs.N2)
    assert np.array_equal(S.noise_u(3, 5, 1, m1, m2)[0], eu[5]) and np.array_equal(S.noise_obs_grid(3, 5, 1, Cs.N1, Cs.N2)[0], eo[5])
    a, ia = S.sample_masked(st, f1, f2, eu, eo, block=4)
    b, ib = S.sample_masked(st, f1, f2, eu, eo, block=64)
    c, _ = S.sample_masked(st, f1, f2, eu[5:6], eo[5:6])
    assert (ia["solves"], ib["solves"]) == (3, 1)
    assert Cs.rel(a, b) <= 1e-12 and Cs.rel(c[0], b[5]) <= 1e-12
