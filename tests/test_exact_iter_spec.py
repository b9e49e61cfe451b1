"""CPU: the numpy specification of the iterative exact GP (tests/exact_iter_spec.py) -- the file the GPU comparison of
tests/test_gpu_exact_iter.py stands on -- against the dense specification (tests/exact_gp_spec.py).

  * every case converges, takes no jitter in the landmark factor, keeps every eigenvalue clear of the 1e-14 cut, and its iteration
    count does not hinge on round-off (count_robust, and the same count under wide=True);
  * the estimator's error E_case against exact_gp_spec.mll / analytic_grad stays within twice the committed value, and within
    2e-2 (MLL) / 0.1 (gradient) for the 48-probe cases the GPU test compares with the dense step;
  * alpha and y^T alpha agree with the dense solve to 1e-8 (they are not estimates: only the PCG tolerance separates them);
  * rank = N = 200: all points are landmarks, P = Sigma, one PCG iteration, and the MLL is the dense one to 1e-9 (the quadrature of a
    1 x 1 tridiagonal is exact and log|P| is the whole log-determinant);
  * the round-off floors D_case: recomputed, none above twice the committed value, 100 D_case never above 1e-8;
  * `python tests/exact_iter_spec.py` rewrites the table it was started with (round trip on a copy).
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_gp_spec as E
import exact_iter_spec as S

ALL = list(S.CASES)


def test_case_list_covers_the_issue():
    C = list(S.CASES.values())
    assert {c[0] for c in C} == {196, 600, 777, 1500}
    assert {c[1] for c in C} >= {(k, k) for k in ("matern12", "matern32", "matern52", "rbf")}
    assert any(c[1][0] != c[1][1] for c in C)
    assert {c[2] for c in C} == {0, 8, 64} and {c[3] for c in C} == {1, 16, 48}
    assert len(S.DENSE_CASES) >= 2 and set(S.FLOORS) == set(S.CASES)


@pytest.mark.parametrize("case", ALL)
def test_conditions_on_the_cases(case):
    st = S.case_spec(case)
    N, _, rank, nprobe, _, _ = S.CASES[case]
    pc, res = st.pc, st.res
    print(f"{case}: iterations {res.kcol.min()} .. {res.kcol.max()}, kept {len(pc.lam)} of {min(rank, N)}, jitter {pc.jitter}")
    assert res.converged and len(res.kcol) == nprobe + 1 and (res.kcol >= 1).all()
    assert pc.jitter == 0.0 and len(pc.lam) == min(rank, N)
    if rank:
        ratio = pc.lam_all / pc.lam_all.max()
        assert not ((ratio > 1e-15) & (ratio < 1e-13)).any()
        assert pc.kzz_eig.min() > 1e-10 * pc.kzz_eig.max()          # the landmark factor is nowhere near a jitter level
        assert np.abs(pc.Q.T @ pc.Q - np.eye(len(pc.lam))).max() <= 1e-8
    assert res.count_robust()


@pytest.mark.parametrize("case", ALL)
def test_against_the_dense_specification(case):
    st = S.case_spec(case)
    kinds, X, y, _, _, theta = S.case_data(case)
    e_mll, e_grad = S.estimator_error(case)
    _, c_mll, c_grad = S.FLOORS[case]
    print(f"{case}: E_case MLL {e_mll:.2e} (committed {c_mll:.2e}) gradient {e_grad:.2e} ({c_grad:.2e})")
    assert e_mll <= 2.0 * c_mll and e_grad <= 2.0 * c_grad
    if case in S.DENSE_CASES:
        assert c_mll <= 2e-2 and c_grad <= 0.1
    ds = E.state(kinds, torch.tensor(X), torch.tensor(theta), torch.tensor(y))
    alpha = ds["alpha"].numpy()
    ya = float(y @ alpha)
    assert ds["eps"] == 0.0
    assert np.abs(st.alpha - alpha).max() <= 1e-8 * np.abs(alpha).max()
    assert abs(st.yalpha - ya) <= 1e-8 * abs(ya)


def test_rank_n_is_the_dense_step():
    N, kinds, rank, nprobe, seed, theta = S.RANK_N
    X, y = S.track_points(N, seed)
    st = S.step(kinds, X, y, theta, nprobe=nprobe, rank=rank)
    val, eps = E.mll(kinds, torch.tensor(X), torch.tensor(theta), torch.tensor(y))
    print(f"rank = N = {N}: iterations {st.res.kcol}, MLL {st.mll:.12g} (dense {float(val):.12g})")
    assert eps == 0.0 and st.pc.jitter == 0.0 and len(st.pc.lam) == N
    assert st.iters == 1 and (st.res.kcol == 1).all()
    assert abs(st.mll - float(val)) <= 1e-9 * abs(float(val))


def test_floors_against_the_committed_table():
    for name in ALL:
        d, wide_iters = S.floor_case(name)
        print(f"{name}: D_case {d:.2e} (committed {S.FLOORS[name][0]:.2e}) -> bounds {S.bounds(S.FLOORS[name][0])}, iterations "
              f"{S.case_spec(name).iters} (wide {wide_iters})")
        assert d <= 2.0 * S.FLOORS[name][0], name
        assert 100.0 * S.FLOORS[name][0] <= S.CAP_MLL, name
        assert wide_iters == S.case_spec(name).iters, name
    assert S.bounds(0.0) == (1e-12, 1e-12) and S.bounds(1.0) == (S.CAP_MLL, S.CAP_GRAD) and S.bounds(1e-13)[0] == pytest.approx(1e-11)


def test_defaults_and_landmarks():
    assert S.defaults() == (16, 64, 1e-10, 1000) and S.defaults(3, 0, 1e-8, 5) == (3, 0, 1e-8, 5)
    assert list(S.landmarks(10, 3)) == [1, 5, 8] and len(S.landmarks(5, 64)) == 5 and len(S.landmarks(5, 0)) == 0
    idx = S.landmarks(100000, 256)
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < 100000
    Z = S.probes(7, 3)
    assert Z.shape == (7, 3) and set(np.unique(Z)) <= {-1.0, 1.0}


def test_regeneration_round_trips(tmp_path):
    """The `__main__` of a copy rewrites its FLOORS block with the values it holds (two significant digits of round-off apart)."""
    here = os.path.dirname(os.path.abspath(__file__))
    for f in ("exact_iter_spec.py", "exact_gp_spec.py", "scattered_iter_spec.py", "conftest.py"):
        shutil.copy(os.path.join(here, f), tmp_path / f)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), str(tmp_path)]))
    driver = ("import exact_iter_spec as S; "
              "keep = {'n196_rbf_r8_p1', 'n600_rbf_r8_p16'}; "
              "[S.CASES.pop(k) for k in list(S.CASES) if k not in keep]; S._regenerate()")
    out = subprocess.run([sys.executable, "-c", driver], cwd=tmp_path, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    src = open(tmp_path / "exact_iter_spec.py").read()
    block = src.split("# FLOORS-BEGIN", 1)[1].split("# FLOORS-END", 1)[0]
    ns = {}
    exec(block.split("\n", 1)[1], ns)
    assert set(ns["FLOORS"]) == {"n196_rbf_r8_p1", "n600_rbf_r8_p16"}
    for k, (d, em, eg) in ns["FLOORS"].items():
        cd, cm, cg = S.FLOORS[k]
        assert d <= 2.0 * cd + 1e-15 and em == pytest.approx(cm, rel=0.02) and eg == pytest.approx(cg, rel=0.02)
    assert src.split("# FLOORS-BEGIN", 1)[0] == open(os.path.join(here, "exact_iter_spec.py")).read().split("# FLOORS-BEGIN", 1)[0]
