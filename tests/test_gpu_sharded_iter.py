"""The iterative masked and scattered steps and their point-wise read-outs on multi-rank contexts: several ranks on ONE GPU, the
host-callback transport carrying the collectives over gloo (the process pattern of tests/test_gpu_dist.py).  Masked grids are split by
rows (sharded.shard_rows: 45 rows over 2 ranks and 80 rows over 3 give uneven slabs), scattered points into uneven shares.

  1. every rank's ELBO and gradient against the numpy specification evaluated on the WHOLE data, with the bounds of the single-rank
     test of the same case (masked: MS.bounds of the committed FLOORS, capped at 1e-8 / 1e-6; scattered: 1e-8 / 1e-6); the PCG
     iteration count equal on all ranks, equal to the specification's and equal to a single-rank run in the parent process
  2. ELBO and gradient bitwise equal across ranks
  3. three steps of one plan, theta (1 + 0.02 k): the kept-basis branch under sharding (masked: against the specification on the basis
     of its step 0, bounds per step; scattered, whose specification has no kept basis: against the single-rank run, 1e-8 / 1e-6)
  4. q(v) at 8 cells and posterior(x*) at 40 points after the sharded step against the same read-outs after the single-rank step
     (means 1e-7, variances 1e-6: the tolerances of tests/test_gpu_masked_iter_readout.py / test_gpu_scattered_iter_variance.py)
  5. max_iter = 1: VGGP_ENOCONV on every rank from the same call, the workers exit normally
  6. the gridded read-out stays refused (VGGP_EINVAL, and the message says which read-out)
and, in one process, the collective sequence itself: a context with the callback transport and ONE rank (the callback is the
identity) issues [the one-time probe of the transport, packed payload, the block vector once per PCG iteration, 32 scalars] and
returns the single-rank step's bits; a context created for two ranks over a callback that sums nothing is refused by that probe.

Measured on one MI355X (2 and 3 ranks; all ranks of a job bitwise equal): step against the specification -- s70_b0_bern70_p16 (23 + 22
and 15 + 15 + 15 rows, 11 iterations) ELBO 0 .. 2.8e-15, gradient 9e-17 .. 3.6e-15 (bound 2.1e-10); s96_rbf_bern70_p16 (40 + 40 and
27 + 27 + 26 rows, 10 iterations) ELBO 2.4e-14 .. 6.2e-14, gradient 7.1e-14 .. 1.9e-13 (bound 7.8e-9); trk400_m12_a (8082 + 8008 and
5400 + 5326 + 5364 points, 8 iterations) ELBO 2.0e-15 .. 8.0e-15, gradient 5.4e-15 .. 1.3e-14; rand20k_m8_a (10037 + 9963 and
6703 + 6630 + 6667 points, 8 iterations) ELBO 2.4e-15 .. 3.1e-15, gradient 3.1e-15 .. 3.7e-15.  Trajectories: t96_b0 10 / 10 / 10
iterations, ELBO 1.7e-16 .. 5.4e-15, gradient 1.6e-15 .. 5.1e-15 (bounds 6.3e-11 .. 7.9e-11); scattered against the single-rank
run 8 / 8 / 8 and 8 / 8 / 9 iterations, ELBO <= 7.9e-15, gradient <= 9.6e-15.  Iteration counts equal to the specification's and to the
single-rank run in every case and step.  Read-outs against the single-rank ones: means <= 1.0e-14, variances <= 8.0e-16 (7 .. 11
iterations, the single-rank counts).  One-rank callback context: [1, 610, 1428 x 11, 32] (masked) and
[1, 384, 1088 x 8, 32] (scattered) for the probe and the step, the single-rank bits.  Before the iterative entries accepted multi-rank contexts every
job of this file ended at its first step with VGGP_EINVAL "single-rank contexts only".
"""
import datetime
import functools
import os
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"
WORLDS = [2, 3]
MASKED_CASES = ["s70_b0_bern70_p16", "s96_rbf_bern70_p16"]         # B0 / Matern-1/2 with missing data (45 rows); points / RBF (80 rows)
MASKED_TRAJ = "t96_b0"
# (data of tests/scattered_iter_spec.py, basis, kernel, m, theta): the smallest track case and the uniform-random case of
# tests/test_gpu_scattered_iter.py (STEP_CASES trk400_m12_a, rand20k_m8_a), whose bounds are 1e-8 (ELBO) and 1e-6 (gradient)
SCATTERED_CASES = {"trk400_m12_a": ("trk400", 12), "rand20k_m8_a": ("rand20k", 8)}
SC_ELBO, SC_GRAD = 1e-8, 1e-6
MEAN_TOL, VAR_TOL = 1e-7, 1e-6
NCELL, NSTAR, TRAJ_STEPS = 8, 40, 3


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _paths():
    for p in (TESTS, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)


def _xs():
    return np.random.default_rng(9).uniform(0, 1, (NSTAR, 2))


def _cells(M):
    return np.random.default_rng(4).choice(M, size=NCELL, replace=False)


# ---- the problems (whole data; a rank takes its slab / share) ---------------------------------------------------------------------------
def _masked_problem(name):
    """-> d1, d2, x1, x2, Y, W [n2, n1], n_probes, the thetas of the steps (one: a cold case; three: the trajectory)."""
    _paths()
    import masked_iter_spec as MS
    if name in MS.CASES:
        d1, d2, _, _, x1, x2, Y, Wn, nprobe, theta = MS.case_problem(name)
        return d1, d2, x1, x2, Y, Wn, nprobe, [theta]
    shape, pair, mkind, mseed, _, _ = MS.TRAJ[name]
    d1, d2, _, _, x1, x2, Y, Wn = MS.problem(shape, pair, mkind, mseed)
    return d1, d2, x1, x2, Y, Wn, 16, [MS.traj_theta(name, k) for k in range(TRAJ_STEPS)]


@functools.lru_cache(maxsize=None)
def _scattered_problem(name):
    _paths()
    import scattered_iter_spec as S
    dname, m = SCATTERED_CASES[name]
    X, y = {"trk400": lambda: S.trk(400, 0.5), "rand20k": S.rand20k}[dname]()
    return X, y, np.linspace(0.0, 1.0, m + 1), S.THETA_A


def _shares(N, world):
    """Uneven shares of N points (the cuts of tests/test_gpu_dist.py _scattered_worker)."""
    return np.linspace(0, N, world + 1).astype(int) + np.array([0] + [37 * (k % 2) for k in range(1, world)] + [0])


# ---- what a rank (or the single-rank engine of the parent: rank 0 of world 1) runs ------------------------------------------------------
def _code(call):
    from variational_gridded_gaussian_processes_amd._lib import VggpError
    try:
        call()
    except VggpError as e:
        return e.code, str(e)
    return 0, ""


def _npy(t):
    return None if t is None else t.cpu().numpy()


def _run_masked(eng, name, rank, world):
    _paths()
    import mixed_dims_cases as MX
    from variational_gridded_gaussian_processes_amd.sharded import shard_rows
    d1, d2, x1, x2, Y, Wn, nprobe, thetas = _masked_problem(name)
    n2, n1 = Wn.shape
    rows = shard_rows(n2, rank, world)
    assert rows.stop > rows.start
    nobs, yy = float(Wn.sum()), float(((Y * Wn) ** 2).sum())          # global
    W = dev(Wn[rows])
    Ym = dev(Y[rows]) * W
    out = {"rows": rows.stop - rows.start, "steps": []}
    eng.plan(*MX.plan_args(d1, x1, d2, x2[rows]), n_total=n1 * n2)
    for th in thetas:
        e, g, info = eng.elbo_step_masked_iter(Ym, W, nobs, yy, th, n_probes=nprobe)
        out["steps"].append((e, g, info["rounds"][0], info["sweeps"][0], info["status"]))
    M = eng.m1 * eng.m2
    qm, qv, qi = eng.qv_masked_iter(W, nobs, cells=_cells(M))
    pm, pv, pi = eng.posterior_masked_iter(dev(_xs()), W, nobs)
    out["readouts"] = (_npy(qm), _npy(qv), _npy(pm), _npy(pv), qi["rounds"][0], pi["rounds"][0])
    if len(thetas) == 1:
        # the gridded read-out of the finished step: refused on a multi-rank context
        C1, C2 = dev(np.ones((3, eng.m1))), dev(np.ones((2, eng.m2)))
        out["gridded"] = _code(lambda: eng.readout_masked_iter(C1, C2, dev(np.ones(3)), dev(np.ones(2)), W, nobs))
        out["noconv"] = _code(lambda: eng.elbo_step_masked_iter(Ym, W, nobs, yy, thetas[0], n_probes=nprobe, max_iter=1))
        out["after_noconv"] = _code(lambda: eng.qv_masked_iter(W, nobs, variance=False))
    return out


def _run_scattered(eng, name, rank, world):
    X, y, g, theta = _scattered_problem(name)
    cuts = _shares(len(y), world)
    mine = slice(cuts[rank], cuts[rank + 1])
    yy = float(y @ y)                                                  # global
    yd = dev(y[mine])
    out = {"rows": mine.stop - mine.start, "steps": []}

    def plan():
        eng.plan("matern12", "b0", g, X[mine, 0].copy(), "matern12", "b0", g, X[mine, 1].copy(), scattered=True, n_total=len(y))
    plan()
    e, gr, info = eng.elbo_step_scattered_iter(yd, yy, theta)
    out["steps"].append((e, gr, info["rounds"][0], info["sweeps"][0], info["status"]))
    M = eng.m1 * eng.m2
    qm, qv, qi = eng.qv_var_scattered_iter(cells=_cells(M))
    pm, pv, pi = eng.posterior_var_scattered_iter(dev(_xs()))
    out["readouts"] = (_npy(qm), _npy(qv), _npy(pm), _npy(pv), qi["rounds"][0], pi["rounds"][0])
    out["means"] = (_npy(eng.qv_scattered_iter()), _npy(eng.posterior_scattered_iter(dev(_xs()))))
    out["noconv"] = _code(lambda: eng.elbo_step_scattered_iter(yd, yy, theta, max_iter=1))
    out["after_noconv"] = _code(eng.qv_scattered_iter)
    plan()                                                             # a fresh plan: cold, then two steps on the kept basis
    out["traj"] = []
    for k in range(TRAJ_STEPS):
        e, gr, info = eng.elbo_step_scattered_iter(yd, yy, theta * (1.0 + 0.02 * k))
        out["traj"].append((e, gr, info["rounds"][0], info["sweeps"][0], info["status"]))
    return out


def _worker(rank, world, port, q, kind, name):
    _paths()
    import torch.distributed as dist
    from variational_gridded_gaussian_processes_amd.sharded import make_engine
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        try:
            eng = make_engine(0, transport="gloo")
            assert eng.n_ranks == world and eng.transport == "callback"
            res = (_run_masked if kind == "masked" else _run_scattered)(eng, name, rank, world)
            q.put((rank, "ok", res))
            dist.barrier()
        except Exception as e:          # noqa: BLE001 -- the parent hears about it instead of waiting for its time limit
            q.put((rank, "error", f"{e!r}\n{traceback.format_exc()}"))
    finally:
        dist.destroy_process_group()


_JOBS = [("masked", n) for n in MASKED_CASES + [MASKED_TRAJ]] + [("scattered", n) for n in SCATTERED_CASES]


_SHARDED = {}


def sharded(kind, name, world):
    """The results of all ranks of one job (rank order), computed once and shared by the tests -- a failed job fails them all at once."""
    key = (kind, name, world)
    if key not in _SHARDED:
        try:
            _SHARDED[key] = ("ok", _launch(kind, name, world))
        except BaseException as e:          # noqa: BLE001
            _SHARDED[key] = ("error", e)
            raise
    status, val = _SHARDED[key]
    if status == "error":
        raise AssertionError(f"the {world}-rank job {kind} / {name} failed in an earlier test: {val!r}")
    return val


def _launch(kind, name, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31200 + (os.getpid() % 1000) + 10 * _JOBS.index((kind, name)) + world
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, kind, name)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=240) for _ in procs], key=lambda r: r[0])
        for p in procs:
            p.join(120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    for rank, status, payload in res:
        assert status == "ok", f"rank {rank}: {payload}"
    return tuple(r[2] for r in res)


_SINGLE = {}


def single(engine, kind, name):
    """The same entries on the single-rank engine of the parent process (the whole data)."""
    if (kind, name) not in _SINGLE:
        _SINGLE[(kind, name)] = (_run_masked if kind == "masked" else _run_scattered)(engine, name, 0, 1)
    return _SINGLE[(kind, name)]


@functools.lru_cache(maxsize=None)
def scattered_spec(name):
    _paths()
    import scattered_iter_spec as S
    X, y, _, theta = _scattered_problem(name)
    f1, f2 = S.b0_factors(SCATTERED_CASES[name][1])
    return S.elbo_step_scattered_iter(X, y, f1, f2, theta)


def _ranks_agree(steps_of_rank):
    for k in range(len(steps_of_rank[0])):
        e0, g0, it0 = steps_of_rank[0][k][:3]
        for st in steps_of_rank[1:]:
            assert st[k][0] == e0 and np.array_equal(st[k][1], g0) and st[k][2] == it0, k


# ---- 1, 2: the step ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("case", MASKED_CASES)
def test_masked_step_vs_spec(engine, case, world):
    import masked_iter_spec as MS
    st = MS.case_spec(case)
    b_elbo, b_grad = MS.bounds(MS.FLOORS[case])
    res, one = sharded("masked", case, world), single(engine, "masked", case)
    assert sum(r["rows"] for r in res) == MS.SHAPES[case[:case.index("_")]][0][1]
    for rank, r in enumerate(res):
        e, g, its, sweeps, status = r["steps"][0]
        e_elbo, e_grad = MS.errors(e, g, st.elbo, st.grad, st.N)
        print(f"{case} world {world} rank {rank} ({r['rows']} rows): iterations {its} (spec {st.iters}, single rank {one['steps'][0][2]}); "
              f"ELBO {e_elbo:.2e} (bound {b_elbo:.2e}) gradient {e_grad:.2e} (bound {b_grad:.2e})")
        assert status == 0 and sweeps == MS.CASES[case][4]
        assert its == st.iters == one["steps"][0][2]
        assert e_elbo <= b_elbo
        assert e_grad <= b_grad
    _ranks_agree([r["steps"] for r in res])


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("case", list(SCATTERED_CASES))
def test_scattered_step_vs_spec(engine, case, world):
    import scattered_iter_spec as S
    st = scattered_spec(case)
    res, one = sharded("scattered", case, world), single(engine, "scattered", case)
    assert sum(r["rows"] for r in res) == st.N and len({r["rows"] for r in res}) > 1
    for rank, r in enumerate(res):
        e, g, its, sweeps, status = r["steps"][0]
        e_elbo, e_grad = S.errors(e, g, st.elbo, st.grad, st.N)
        print(f"{case} world {world} rank {rank} ({r['rows']} points): iterations {its} (spec {st.iters}, single rank {one['steps'][0][2]}); "
              f"ELBO {e_elbo:.2e} gradient {e_grad:.2e}")
        assert status == 0 and sweeps == 16
        assert its == st.iters == one["steps"][0][2]
        assert e_elbo <= SC_ELBO
        assert e_grad <= SC_GRAD
    _ranks_agree([r["steps"] for r in res])


# ---- 3: trajectories (kept basis) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_masked_trajectory_vs_spec(engine, world):
    import masked_iter_spec as MS
    name = MASKED_TRAJ
    sts = MS.traj_spec(name)[:TRAJ_STEPS]
    res, one = sharded("masked", name, world), single(engine, "masked", name)
    for k, st in enumerate(sts):
        b_elbo, b_grad = MS.bounds(*MS.FLOORS[name][k])
        for rank, r in enumerate(res):
            e, g, its, sweeps, status = r["steps"][k]
            e_elbo, e_grad = MS.errors(e, g, st.elbo, st.grad, st.N)
            print(f"{name} world {world} rank {rank} step {k} ({'kept' if k else 'cold'}): iterations {its} (spec {st.iters}, single rank "
                  f"{one['steps'][k][2]}); ELBO {e_elbo:.2e} (bound {b_elbo:.2e}) gradient {e_grad:.2e} (bound {b_grad:.2e})")
            assert status == 0 and sweeps == 16
            assert MS.TRAJ_COUNTS[name][k] and its == st.iters == one["steps"][k][2]
            assert e_elbo <= b_elbo, k
            assert e_grad <= b_grad, k
    _ranks_agree([r["steps"] for r in res])


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("case", list(SCATTERED_CASES))
def test_scattered_trajectory_vs_single_rank(engine, case, world):
    import scattered_iter_spec as S
    N = scattered_spec(case).N
    res, one = sharded("scattered", case, world), single(engine, "scattered", case)
    for k in range(TRAJ_STEPS):
        e1, g1, its1 = one["traj"][k][:3]
        for rank, r in enumerate(res):
            e, g, its, sweeps, status = r["traj"][k]
            e_elbo, e_grad = S.errors(e, g, e1, g1, N)
            print(f"{case} world {world} rank {rank} step {k}: iterations {its} (single rank {its1}); ELBO {e_elbo:.2e} gradient {e_grad:.2e}")
            assert status == 0 and sweeps == 16 and its == its1
            assert e_elbo <= SC_ELBO, k
            assert e_grad <= SC_GRAD, k
    _ranks_agree([r["traj"] for r in res])


# ---- 4: read-outs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("kind,case", [("masked", c) for c in MASKED_CASES] + [("scattered", c) for c in SCATTERED_CASES])
def test_readouts_vs_single_rank(engine, kind, case, world):
    res, one = sharded(kind, case, world), single(engine, kind, case)
    ref = one["readouts"]
    for rank, r in enumerate(res):
        got = r["readouts"]
        errs = [rel(got[i], ref[i]) for i in range(4)]
        print(f"{case} world {world} rank {rank}: q(v) mean {errs[0]:.1e} var {errs[1]:.1e}; posterior mean {errs[2]:.1e} var {errs[3]:.1e}; "
              f"iterations {got[4]} / {got[5]} (single rank {ref[4]} / {ref[5]})")
        assert got[1].shape == (NCELL,) and got[2].shape == (NSTAR,) and got[3].shape == (NSTAR,)
        assert errs[0] <= MEAN_TOL and errs[2] <= MEAN_TOL
        assert errs[1] <= VAR_TOL and errs[3] <= VAR_TOL
        assert (got[1] > 0).all() and 0 < got[4] < 100 and 0 < got[5] < 100
        for i in range(4):
            assert np.array_equal(got[i], res[0]["readouts"][i])          # replicated: the same bits on every rank
        if kind == "scattered":
            assert rel(r["means"][0], one["means"][0]) <= MEAN_TOL and rel(r["means"][1], one["means"][1]) <= MEAN_TOL
            assert np.array_equal(r["means"][0], got[0])


# ---- 5, 6: failure behaviour ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("kind,case", [("masked", MASKED_CASES[0]), ("scattered", "rand20k_m8_a")])
def test_no_hang_on_non_convergence(kind, case, world):
    from variational_gridded_gaussian_processes_amd import _lib
    for r in sharded(kind, case, world):          # (sharded() has asserted that the workers exited normally)
        assert r["noconv"][0] == _lib.VGGP_ENOCONV and "1 iterations" in r["noconv"][1]
        assert r["after_noconv"][0] == _lib.VGGP_ESTATE          # ... and the failed step left nothing to read


@pytest.mark.parametrize("world", WORLDS)
def test_gridded_readout_still_refused(world):
    from variational_gridded_gaussian_processes_amd import _lib
    for r in sharded("masked", MASKED_CASES[0], world):
        code, msg = r["gridded"]
        assert code == _lib.VGGP_EINVAL and "gridded read-out" in msg and "single-rank" in msg


def test_transport_that_does_not_span_the_ranks_is_refused():
    """A context created for two ranks whose all-reduce sums nothing: every rank would count its own PCG iterations on half of the
    data.  The iterative entries find out with one all-reduce of 1.0 and return VGGP_EINVAL; the verdict is kept (one probe)."""
    from variational_gridded_gaussian_processes_amd import Engine, _lib
    import masked_iter_spec as MS
    import mixed_dims_cases as MX
    d1, d2, _, _, x1, x2, Y, Wn, nprobe, theta = MS.case_problem(MASKED_CASES[0])
    calls = []
    eng = Engine(0, n_ranks=2, rank=0, allreduce=lambda buf: calls.append(buf.size))
    try:
        eng.plan(*MX.plan_args(d1, x1, d2, x2[:23]), n_total=Wn.size)
        W = dev(Wn[:23])
        for call in (lambda: eng.elbo_step_masked_iter(dev(Y[:23]) * W, W, float(Wn.sum()), 1.0, theta, n_probes=nprobe),
                     lambda: eng.qv_masked_iter(W, float(Wn.sum()), variance=False),
                     lambda: eng.posterior_masked_iter(dev(_xs()), W, float(Wn.sum()))):
            code, msg = _code(call)
            assert code == _lib.VGGP_EINVAL and "does not sum over its n_ranks = 2 ranks" in msg
    finally:
        eng.close()
    assert calls == [1]


# ---- the collective sequence, in one process --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,case", [("masked", MASKED_CASES[0]), ("scattered", "rand20k_m8_a")])
def test_collective_sequence_one_rank_callback(engine, kind, case):
    """A context with the callback transport and one rank runs the multi-rank sequence with an identity collective: the calls are
    the packed payload, the block vector once per PCG iteration and the 32 packed scalars, in this order, and the step returns the
    bits of the plain single-rank context (the packing moves numbers, it does not change them)."""
    from variational_gridded_gaussian_processes_amd import Engine
    calls = []
    eng = Engine(0, n_ranks=1, rank=0, allreduce=lambda buf: calls.append(buf.size))
    try:
        assert eng.transport == "callback"
        got = (_run_masked if kind == "masked" else _run_scattered)(eng, case, 0, 1)
    finally:
        eng.close()
    one = single(engine, kind, case)
    e, g, its = got["steps"][0][:3]
    assert e == one["steps"][0][0] and np.array_equal(g, one["steps"][0][1]) and its == one["steps"][0][2]
    m1, m2 = got["readouts"][0].shape
    M, nbc = m1 * m2, 17
    if kind == "masked":
        import masked_iter_spec as MS
        n1 = MS.SHAPES[case[:case.index("_")]][0][0]
        pre = 2 * m2 * m2 + 3 * M + n1
    else:
        pre = (2 * m2 * m2 + 3 * M + 31) // 32 * 32 + m1 * m1
    print(f"{case}: {len(calls)} collectives; the probe and the step's: {calls[:its + 3]}")
    assert calls[0] == 1          # the first iterative entry on the context asks once whether the transport spans its ranks
    calls = calls[1:]
    assert calls[:its + 2] == [pre] + [M * nbc] * its + [32]
    q_its, p_its = got["readouts"][4], got["readouts"][5]
    assert calls[its + 2:its + 2 + q_its + p_its] == [M * NCELL] * q_its + [M * NSTAR] * p_its          # the read-outs: the operator's alone
    for i in range(4):
        assert np.array_equal(got["readouts"][i], one["readouts"][i])
