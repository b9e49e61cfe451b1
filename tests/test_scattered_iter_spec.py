"""CPU: the numpy specification of the iterative scattered step (tests/scattered_iter_spec.py) against the dense M-space oracle
oracle.kron.elbo_step_scattered, in the data-rich regime (N / M >= 60) where the step states a tolerance.

Caps (conditions, not measurements): ELBO 1e-4 of max(|ELBO|, N / 2), gradient 2e-4 of its largest component, a0 1e-7 of its
largest entry, fewer than 30 PCG iterations; bitwise repeatable.
"""
import functools

import numpy as np
import pytest

from oracle import kron as Kr

import scattered_iter_spec as S

CASES = {
    "trk400_m12_a": ("trk400", 12, S.THETA_A),
    "trk400_m12_b": ("trk400", 12, S.THETA_B),
    "trk400_m16_b": ("trk400", 16, S.THETA_B),
    "trk600_m24_b": ("trk600", 24, S.THETA_B),
    "rand20k_m8_a": ("rand20k", 8, S.THETA_A),
}


@functools.lru_cache(maxsize=None)
def data(name):
    return {"trk400": lambda: S.trk(400, 0.5), "trk600": lambda: S.trk(600, 0.25), "rand20k": S.rand20k}[name]()


def test_track_point_counts():
    assert len(data("trk400")[1]) == 16090 and len(data("trk600")[1]) == 46680


def test_probes_are_rademacher_and_fixed():
    Z = S.probes(5, 7, 16)
    assert Z.shape == (16, 5, 7) and set(np.unique(Z)) == {-1.0, 1.0}
    assert np.array_equal(Z, S.probes(5, 7, 16))
    assert abs(Z.mean()) < 0.2 and not np.array_equal(Z[0], Z[1])
    # one value by hand: probe column c = 1, element (a, b) = (0, 0), python integers
    mask = (1 << 64) - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & mask
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & mask
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & mask
        return x ^ (x >> 31)

    for c, a, b in ((1, 0, 0), (16, 4, 6), (3, 2, 5)):
        h = mix(S.PROBE_SEED ^ mix((c << 40) ^ (a * 7 + b)))
        assert Z[c - 1, a, b] == (1.0 if (h >> 17) & 1 else -1.0)


@pytest.mark.parametrize("case", list(CASES))
def test_spec_against_dense_oracle(case):
    name, m, theta = CASES[case]
    X, y = data(name)
    f1, f2 = S.b0_factors(m)
    ref = Kr.elbo_step_scattered(X, y, f1, f2, theta)
    st = S.elbo_step_scattered_iter(X, y, f1, f2, theta)
    e_elbo, e_grad = S.errors(st.elbo, st.grad, ref.elbo, ref.grad, len(y))
    e_a0 = float(np.abs(st.A0 - ref.A0).max() / np.abs(ref.A0).max())
    print(f"{case}: N/M {len(y) / m ** 2:.0f} its {st.iters} ELBO {e_elbo:.2e} grad {e_grad:.2e} a0 {e_a0:.2e}")
    assert st.converged and st.iters < 30
    assert e_elbo <= 1e-4
    assert e_grad <= 2e-4
    assert e_a0 <= 1e-7
    if case == "trk400_m12_a":          # bitwise repeatable (one case: the spec is deterministic numpy)
        st2 = S.elbo_step_scattered_iter(X, y, f1, f2, theta)
        assert st2.elbo == st.elbo and np.array_equal(st2.grad, st.grad) and np.array_equal(st2.A0, st.A0)
