"""CPU: the numpy specification of the iterative masked step (tests/masked_iter_spec.py) -- the file the GPU comparison of
tests/test_gpu_masked_iter_spec.py stands on.

  * handed the oracle's own default_rng(seed) probes it reproduces oracle.kron.elbo_step_masked_iter to 1e-12 (ELBO and gradient, scale
    of scattered_iter_spec.errors) with the same iteration count: the specification is the oracle plus the probe source;
  * with the engine's probes every case stays within the caps of the small shapes against the dense oracle.kron.elbo_step_masked
    (2e-4 / 2e-4, test_iterative_masked_step_vs_dense_small);
  * basis= with the state's own (Q1, Q2) at the same theta reproduces the cold step to 1e-10;
  * the stopping margins hold in every column of every cold case (last ratio <= 0.5, the one before >= 2): only then may the GPU test
    assert equal iteration counts; for the trajectories the table TRAJ_COUNTS says step by step where they do, and the steps stay inside
    the engine's rule for keeping a basis (at most 4 iterations more than right after the cold solve);
  * the jumps (JUMPS): on step 0's basis the new theta takes at least 12 + 4 iterations more than step 0 ("x": the engine gives the
    kept basis up inside the step) or between 4 + 2 and 12 - 2 more ("half": the step stands and the next one solves cold), so that the
    GPU test knows which branch of the engine's policy each step takes;
  * the round-off floors: recomputed, none above twice the committed value, and 100 D_case never above the caps 1e-8 / 1e-6.
"""
import os
import re

import numpy as np
import pytest

from oracle import kron as Kr

import masked_iter_spec as MS

ALL = list(MS.CASES)


@pytest.mark.parametrize("case", ALL)
def test_spec_is_the_oracle_plus_the_probe_source(case):
    _, _, f1, f2, _, _, Y, W, nprobe, theta = MS.case_problem(case)
    m1, m2 = MS.SHAPES[MS.CASES[case][0]][1]
    ref = Kr.elbo_step_masked_iter(Y, W, f1, f2, theta, nprobe=nprobe, seed=0)
    Z0 = np.random.default_rng(0).choice([-1.0, 1.0], size=(nprobe, m1, m2))
    st = MS.elbo_step_masked_iter(Y, W, f1, f2, theta, nprobe=nprobe, Z0=Z0)
    e_elbo, e_grad = MS.errors(st.elbo, st.grad, ref.elbo, ref.grad, ref.N)
    print(f"{case}: its {st.iters} (oracle {ref.iters}) ELBO {e_elbo:.2e} grad {e_grad:.2e}")
    assert st.iters == ref.iters and st.N == ref.N and st.A0.shape == (m1, m2)
    assert e_elbo <= 1e-12
    assert e_grad <= 1e-12


@pytest.mark.parametrize("case", ALL)
def test_spec_with_engine_probes_against_dense_oracle(case):
    _, _, f1, f2, _, _, Y, W, _, theta = MS.case_problem(case)
    ref = Kr.elbo_step_masked(Y, W, f1, f2, theta)
    st = MS.case_spec(case)
    e_elbo, e_grad = MS.errors(st.elbo, st.grad, ref.elbo, ref.grad, ref.N)
    print(f"{case}: N {st.N} its {st.iters} ELBO {e_elbo:.2e} grad {e_grad:.2e}")
    assert st.converged
    assert e_elbo <= 2e-4
    assert e_grad <= 2e-4


@pytest.mark.parametrize("case", ALL)
def test_stopping_margins_in_every_column(case):
    st = MS.case_spec(case)
    nprobe = MS.CASES[case][4]
    print(f"{case}: iterations {st.kcol.min()} .. {st.kcol.max()}, last ratio <= {st.last.max():.3g}, the one before >= {st.prev.min():.3g}")
    assert st.converged and len(st.kcol) == nprobe + 1 and (st.kcol >= 1).all()
    assert (st.last <= 0.5).all()
    assert (st.prev >= 2.0).all()
    if MS.CASES[case][2] == "ones":          # the preconditioner is exact on a full grid
        assert st.iters <= 3


def test_case_lists_cover_the_issue():
    """Every shape with two masks at least, every basis / kernel pair, mask and probe count at least once; both dimensions differ."""
    C = list(MS.CASES.values())
    assert len(C) >= 14
    for shape, ((n1, n2), (m1, m2)) in MS.SHAPES.items():
        assert n1 != n2 and m1 != m2
        assert len({c[2] for c in C if c[0] == shape}) >= 2
    assert {c[1] for c in C} == {"b0_m12", "pts_m32", "pts_rbf", "vff", "b1", "b0_m12-pts_m52"}
    assert {c[2] for c in C} >= {"bern70", "bern05", "holes", "ones"} and any(c[2].startswith("track") for c in C)
    assert {c[4] for c in C} == {1, 16, MS.MAX_PROBES}
    W = MS.mask("holes", 96, 80, 133)
    assert (W.sum(1) == 0).sum() == 3 and (W.sum(0) == 0).sum() == 2
    for c in C:          # VFF: an odd feature count in both dimensions where the shape allows, m = 2 nfreq + 1
        if c[1] == "vff":
            d1, d2 = MS.dims("vff", *MS.SHAPES[c[0]][1])
            assert d1.basis == "vff" and (len(d1.grid) - 2) * 2 - 1 == MS.SHAPES[c[0]][1][0] and MS.SHAPES[c[0]][1][0] % 2 == 1


def test_probe_limit_is_the_entry_s():
    """MAX_PROBES is what the iterative steps accept: VGI_MAX_PROBES of mspace_ws.h, which iter_step.hip checks n_probes against (the
    GPU test runs that count and asserts VGGP_EINVAL one above it)."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "variational_gridded_gaussian_processes_amd", "csrc")
    with open(os.path.join(csrc, "mspace_ws.h")) as fh:
        limits = set(re.findall(r"#define VGI_MAX_PROBES (\d+)", fh.read()))
    assert limits == {str(MS.MAX_PROBES)}
    with open(os.path.join(csrc, "iter_step.hip")) as fh:
        assert "n_probes <= VGI_MAX_PROBES" in fh.read()


@pytest.mark.parametrize("case", ["s96_b0_bern70_p16", "s70_pts32_track30_p1", "s96_b1_holes_p16", "s96_vff_bern05_p1"])
def test_basis_argument_is_consistent(case):
    _, _, f1, f2, _, _, Y, W, nprobe, theta = MS.case_problem(case)
    st = MS.case_spec(case)
    kept = MS.elbo_step_masked_iter(Y, W, f1, f2, theta, nprobe=nprobe, basis=(st.Q1, st.Q2))
    e_elbo, e_grad = MS.errors(kept.elbo, kept.grad, st.elbo, st.grad, st.N)
    print(f"{case}: kept basis at the same theta: ELBO {e_elbo:.2e} grad {e_grad:.2e}, Rayleigh quotients {np.abs(kept.lam1 - st.lam1).max():.1e}")
    assert kept.iters == st.iters and np.array_equal(kept.kcol, st.kcol)
    assert e_elbo <= 1e-10
    assert e_grad <= 1e-10
    assert np.array_equal(kept.Q1, st.Q1) and np.array_equal(kept.Q2, st.Q2)


@pytest.mark.parametrize("name", list(MS.TRAJ))
def test_trajectories(name):
    kept = MS.TRAJ[name][4]
    sts = MS.traj_spec(name)
    its = [s.iters for s in sts]
    ok = tuple(s.margins_ok() for s in sts)
    print(f"{name}: iterations {its}, margins {ok}")
    assert len(sts) == MS.TRAJ_STEPS and all(s.converged for s in sts)
    assert ok == MS.TRAJ_COUNTS[name]          # where the GPU test compares the iteration counts
    if kept:
        # the engine keeps a basis while the last step took at most 4 iterations more than the cold one (and gives a step up beyond
        # 12 more): inside that rule the specification's "step 0's basis from step 1 on" is what the engine does
        assert max(its) <= its[0] + 4
        for s in sts[1:]:
            assert np.array_equal(s.Q1, sts[0].Q1) and np.array_equal(s.Q2, sts[0].Q2)
        assert np.abs(sts[1].lam1 - sts[0].lam1).max() > 1e-6          # Rayleigh quotients of the CURRENT Gram matrices
    else:
        assert not np.array_equal(sts[1].Q1, sts[0].Q1)


@pytest.mark.parametrize("name", list(MS.JUMPS))
def test_jumps_take_the_branch_they_are_named_for(name):
    sts, kept0 = MS.jump_spec(name)
    its = [s.iters for s in sts]
    print(f"{name}: iterations {its}, theta' on step 0's basis {kept0.iters}")
    assert len(sts) == 3 and all(s.converged for s in sts) and kept0.converged
    assert sts[0].margins_ok()                 # step 0: the GPU test asserts the equal count
    assert np.array_equal(sts[0].theta, MS.THETA_T) and np.array_equal(sts[1].theta[:2], MS.THETA_T[:2] * MS.JUMPS[name][4])
    if name.endswith("_half"):                 # kept, no retry (<= reference + 12); the next step solves cold (> reference + 4)
        assert its[0] + 4 + 2 <= kept0.iters <= its[0] + 12 - 2
        assert kept0 is sts[1] and np.array_equal(sts[1].Q1, sts[0].Q1) and not np.array_equal(sts[2].Q1, sts[0].Q1)
    else:                                      # given up inside the step (> reference + 12), and the cold step stays clear of the limit
        assert kept0.iters >= its[0] + 12 + 4
        assert its[1] + 1 <= its[0] + 12
        assert np.array_equal(sts[2].Q1, sts[1].Q1) and np.array_equal(sts[2].Q2, sts[1].Q2) and not np.array_equal(sts[1].Q1, sts[0].Q1)


def test_floors_against_the_committed_table():
    assert set(MS.FLOORS) == set(MS.CASES) | set(MS.TRAJ) | set(MS.JUMPS)
    for name in MS.CASES:
        d = MS.floor_case(name)
        print(f"{name}: D_case {d:.2e} (committed {MS.FLOORS[name]:.2e}) -> bounds {MS.bounds(MS.FLOORS[name])}")
        assert d <= 2.0 * MS.FLOORS[name], name
        assert 100.0 * MS.FLOORS[name] <= MS.CAP_ELBO, name
    for name in MS.TRAJ:
        for k, ((dc, db), (rc, rb)) in enumerate(zip(MS.floor_traj(name), MS.FLOORS[name])):
            print(f"{name} step {k}: D_case {dc:.2e} ({rc:.2e}) D_basis {db:.2e} ({rb:.2e})")
            assert dc <= 2.0 * rc and db <= 2.0 * rb, (name, k)
            assert max(100.0 * rc, 10.0 * rb) <= MS.CAP_ELBO, (name, k)
    for name in MS.JUMPS:          # (100 D_case of a cold step at a doubled lengthscale may reach the ELBO cap: bounds() then gives the cap)
        assert len(MS.FLOORS[name]) == 3
        for k, ((dc, db), (rc, rb)) in enumerate(zip(MS.floor_jump(name), MS.FLOORS[name])):
            print(f"{name} step {k}: D_case {dc:.2e} ({rc:.2e}) D_basis {db:.2e} ({rb:.2e})")
            assert dc <= 2.0 * rc and db <= 2.0 * rb, (name, k)
            assert max(100.0 * rc, 10.0 * rb) <= MS.CAP_GRAD, (name, k)
            assert MS.bounds(rc, rb)[0] <= MS.CAP_ELBO and MS.bounds(rc, rb)[1] <= MS.CAP_GRAD, (name, k)
    assert MS.bounds(0.0) == (1e-12, 1e-12) and MS.bounds(1.0) == (MS.CAP_ELBO, MS.CAP_GRAD) and MS.bounds(1e-13, 1e-11)[0] == pytest.approx(1e-10)
