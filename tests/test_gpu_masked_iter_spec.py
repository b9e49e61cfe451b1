"""vggp_elbo_step_masked_iter against its numpy specification (tests/masked_iter_spec.py: the oracle's algorithm on the engine's own probe
block, PCG scalars as the kernel keeps them): two float64 evaluations of the same algorithm, so the bound is the specification's own
round-off floor and not the estimator's noise -- max(100 D_case, 10 D_basis, 1e-12) from the committed table, never above 1e-8 (ELBO) /
1e-6 (gradient).  Cold steps after a fresh plan on 96 x 80, 70 x 45 and 200 x 130 grids (every basis / kernel pair, mask and probe
count of masked_iter_spec.CASES) with equal iteration counts, the probe count as info['sweeps'][0], the q(v) mean at 1e-9 and calls
two and three bitwise equal; six steps of one plan (theta (1 + 0.02 k)) against the specification on the basis of ITS step 0 (Rayleigh
quotients) and, for RBF, cold at every step; jumps in theta that make the engine give its kept basis up (inside the step, or for
the next one); the probe limit.

Measured on one MI355X: iteration counts equal in every case and step (1 .. 34); ELBO 2e-16 .. 7e-13, gradient 4e-16 .. 5e-13
(bounds 1e-12 .. 8e-9), q(v) mean 4e-15 .. 2e-11; all ones against vggp_elbo_step 1e-14 (96 x 80) and 5e-12 / 2e-12 (200 x 130).  Under
two mutations of masked.hip (not committed): V1 and B1 swapped in one control-variate field of the l1 trace -- gradient 1e-8 .. 2e-5,
every case with missing data fails; the probe seed's last digit changed -- ELBO 3e-7 .. 1e-3, gradient 3e-7 .. 9e-4, the same cases
fail; test_iterative_masked_step_vs_dense_small passes under both.
"""
import numpy as np
import pytest
import torch

from variational_gridded_gaussian_processes_amd import _lib
from variational_gridded_gaussian_processes_amd._lib import VggpError

import masked_iter_spec as MS
import mixed_dims_cases as MX

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _plan(engine, d1, d2, x1, x2, Y, Wn):
    """A fresh plan (the next step solves the preconditioner's eigenproblem) and the step's device arguments."""
    engine.plan(*MX.plan_args(d1, x1, d2, x2))
    W = dev(Wn)
    Ym = dev(Y) * W
    return Ym, W, float(Wn.sum()), engine.sumsq(Ym)


@pytest.mark.parametrize("case", list(MS.CASES))
def test_cold_step_vs_spec(engine, case):
    d1, d2, f1, f2, x1, x2, Y, Wn, nprobe, theta = MS.case_problem(case)
    st = MS.case_spec(case)
    Ym, W, nobs, yy = _plan(engine, d1, d2, x1, x2, Y, Wn)
    assert (engine.m1, engine.m2) == st.A0.shape and nobs == st.N
    elbo, grad, info = engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta, n_probes=nprobe)
    e_elbo, e_grad = MS.errors(elbo, grad, st.elbo, st.grad, st.N)
    b_elbo, b_grad = MS.bounds(MS.FLOORS[case])
    mean, var, _ = engine.qv_masked_iter(W, nobs, variance=False)
    e_q = rel(mean.cpu().numpy(), MS.qv_mean(st, f1, f2))
    print(f"{case}: iterations {info['rounds'][0]} (spec {st.iters}); ELBO {e_elbo:.2e} (bound {b_elbo:.2e}) gradient {e_grad:.2e} "
          f"(bound {b_grad:.2e}) q(v) mean {e_q:.2e}")
    assert info["status"] == 0
    assert info["rounds"][0] == st.iters
    assert info["sweeps"][0] == nprobe
    assert e_elbo <= b_elbo
    assert e_grad <= b_grad
    assert var is None and e_q <= 1e-9
    # second and third call (kept basis with Rayleigh quotients; RBF: cold again): the third equals the second bit for bit
    e2, g2, i2 = engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta, n_probes=nprobe)
    e3, g3, i3 = engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta, n_probes=nprobe)
    assert e3 == e2 and np.array_equal(g3, g2) and i3["rounds"] == i2["rounds"]
    if MS.CASES[case][2] == "ones":          # everything observed: the preconditioner is exact, and the step is the Kronecker path's
        Yd = dev(Y)
        ke, kg, _ = engine.elbo_step(Yd, engine.sumsq(Yd), theta)
        print(f"{case}: against vggp_elbo_step: ELBO {abs(elbo - ke) / abs(ke):.2e} gradient {rel(grad, kg):.2e}")
        assert info["rounds"][0] <= 3
        assert abs(elbo - ke) <= 1e-8 * abs(ke) and rel(grad, kg) < 1e-6


@pytest.mark.parametrize("name", list(MS.TRAJ))
def test_trajectory_vs_spec(engine, name):
    """One plan, six steps: the engine solves the eigenproblem on step 0 and keeps that basis (RBF: solves every step)."""
    shape, pair, mkind, mseed, kept, _ = MS.TRAJ[name]
    d1, d2, f1, f2, x1, x2, Y, Wn = MS.problem(shape, pair, mkind, mseed)
    sts = MS.traj_spec(name)
    Ym, W, nobs, yy = _plan(engine, d1, d2, x1, x2, Y, Wn)
    for k, st in enumerate(sts):
        elbo, grad, info = engine.elbo_step_masked_iter(Ym, W, nobs, yy, MS.traj_theta(name, k))
        e_elbo, e_grad = MS.errors(elbo, grad, st.elbo, st.grad, st.N)
        b_elbo, b_grad = MS.bounds(*MS.FLOORS[name][k])
        counted = MS.TRAJ_COUNTS[name][k]
        print(f"{name} step {k} ({'kept' if kept and k else 'cold'}): iterations {info['rounds'][0]} (spec {st.iters}, "
              f"{'compared' if counted else 'margins too small to compare'}); ELBO {e_elbo:.2e} (bound {b_elbo:.2e}) "
              f"gradient {e_grad:.2e} (bound {b_grad:.2e})")
        assert info["status"] == 0 and info["sweeps"][0] == 16
        if counted:
            assert info["rounds"][0] == st.iters
        assert e_elbo <= b_elbo, k
        assert e_grad <= b_grad, k
        e_q = rel(engine.qv_masked_iter(W, nobs, variance=False)[0].cpu().numpy(), MS.qv_mean(st, f1, f2))
        assert e_q <= 1e-9, k


@pytest.mark.parametrize("name", list(MS.JUMPS))
def test_jump_in_theta_vs_spec(engine, name):
    """The two branches of the kept-basis policy that a 2 % drift never reaches (masked_iter_spec.JUMPS).  "x": on step 0's basis the
    new theta would take more than step 0's count + 12 iterations, so step 1 gives the basis up and returns the COLD step; step 2
    keeps the basis of that cold solve, step 3 equals step 2 bit for bit.  "half": step 1 stands on step 0's basis with between 4 and 12
    iterations more than step 0, so step 2 solves cold.  The stopping margins hold on step 0 only: later counts within 1."""
    shape, pair, mkind, mseed, _ = MS.JUMPS[name]
    d1, d2, f1, f2, x1, x2, Y, Wn = MS.problem(shape, pair, mkind, mseed)
    sts, _ = MS.jump_spec(name)
    Ym, W, nobs, yy = _plan(engine, d1, d2, x1, x2, Y, Wn)
    half = name.endswith("_half")
    got = []
    for k, (st, (theta, src)) in enumerate(zip(sts, MS.jump_plan(name))):
        elbo, grad, info = engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta)
        got.append((elbo, grad, info))
        e_elbo, e_grad = MS.errors(elbo, grad, st.elbo, st.grad, st.N)
        b_elbo, b_grad = MS.bounds(*MS.FLOORS[name][k])
        e_q = rel(engine.qv_masked_iter(W, nobs, variance=False)[0].cpu().numpy(), MS.qv_mean(st, f1, f2))
        print(f"{name} step {k} ({'cold' if src is None else f'basis of step {src}'}): iterations {info['rounds'][0]} (spec {st.iters}); "
              f"ELBO {e_elbo:.2e} (bound {b_elbo:.2e}) gradient {e_grad:.2e} (bound {b_grad:.2e}) q(v) mean {e_q:.2e}")
        assert info["status"] == 0 and info["sweeps"][0] == 16
        if k == 0:
            assert info["rounds"][0] == st.iters
        else:
            assert abs(info["rounds"][0] - st.iters) <= 1
        assert e_elbo <= b_elbo, k
        assert e_grad <= b_grad, k
        assert e_q <= 1e-9, k
    if half:
        assert got[1][2]["rounds"][0] > got[0][2]["rounds"][0] + 4          # ... which is why step 2 solved cold
    else:
        assert got[1][2]["rounds"][0] <= got[0][2]["rounds"][0] + 12        # the cold step, not an iteration on the stale basis
        e3, g3, i3 = engine.elbo_step_masked_iter(Ym, W, nobs, yy, MS.jump_theta(name))
        assert e3 == got[2][0] and np.array_equal(g3, got[2][1]) and i3["rounds"] == got[2][2]["rounds"]


def test_probe_limit(engine):
    """n_probes = 63 runs (s96_b0_ones_p63 above); one more is VGGP_EINVAL and ends the iterative state."""
    d1, d2, f1, f2, x1, x2, Y, Wn, _, theta = MS.case_problem("s70_b0_track50_p1")
    Ym, W, nobs, yy = _plan(engine, d1, d2, x1, x2, Y, Wn)
    engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta, n_probes=1)
    with pytest.raises(VggpError) as ei:
        engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta, n_probes=MS.MAX_PROBES + 1)
    assert ei.value.code == _lib.VGGP_EINVAL
    with pytest.raises(VggpError) as ei:
        engine.qv_masked_iter(W, nobs, variance=False)
    assert ei.value.code == _lib.VGGP_ESTATE
