"""Several ranks on ONE GPU: the in-library multi-rank step (vggp_elbo_step on an n_ranks > 1 context = partials ->
the context's all-reduce -> finish, csrc/comm.hip) with the host-callback transport carrying the payload over gloo
(RCCL refuses several ranks on one device; the RCCL transport itself is exercised with a communicator of size one in
test_rccl_transport_size_one).  Every rank equals the single-rank step and the oracle."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N1, N2, M1, M2 = 96, 70, 12, 9            # 70 rows over 2 ranks: 35 + 35; over 3 (shard_rows): 24 + 24 + 22
THETA = [0.2, 0.3, 1.0, 0.8, 0.01]


NSTEP = 6


def _worker(rank, world, port, q, kind="matern32", m1=M1, m2=M2):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from oracle import dense as D
    from variational_gridded_gaussian_processes_amd import Engine
    from variational_gridded_gaussian_processes_amd.sharded import ShardedStep, make_engine, shard_rows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X, y, x1, x2 = D.gen_grid(N1, N2)
        rows = shard_rows(N2, rank, world)
        eng = make_engine(0, transport="gloo")
        assert eng.n_ranks == world and eng.transport == "callback"
        eng.plan(kind, "points", np.linspace(0, 1, m1), x1, kind, "points", np.linspace(0, 1, m2), x2[rows],
                 n_total=N1 * N2, warm_start=True)
        Y = torch.tensor(y.reshape(N2, N1)[rows], device="cuda:0")
        sh = ShardedStep(eng)
        yy = sh.sumsq_total(Y)
        out = []
        for k in range(NSTEP):                   # cold, warm, extrapolated, then refined + polished starts (finish graph variants)
            th = np.array(THETA) * (1.0 + 0.01 * k)
            e, g, info = sh.step(Y, yy, th)
            out.append((e, g, sum(info["rounds"])))
        mean, var = eng.qv()
        q.put((rank, out, mean.cpu().numpy(), var.cpu().numpy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_step_equals_single_rank_and_oracle(engine, world):
    from oracle import dense as D, kron as Kr
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + (os.getpid() % 1000) + world
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    X, y, x1, x2 = D.gen_grid(N1, N2)
    g1, g2 = np.linspace(0, 1, M1), np.linspace(0, 1, M2)
    f1, f2 = Kr.Factor("points", "matern32", g1, x1), Kr.Factor("points", "matern32", g2, x2)
    engine.plan("matern32", "points", g1, x1, "matern32", "points", g2, x2, warm_start=True)
    Y = torch.tensor(y.reshape(N2, N1), device="cuda")
    for k in range(NSTEP):
        th = np.array(THETA) * (1.0 + 0.01 * k)
        ref = Kr.elbo_step(y.reshape(N2, N1), f1, f2, th)
        e1, g1_, _ = engine.elbo_step(Y, engine.sumsq(Y), th)
        for rank, out, _, _ in res:
            e, g = out[k][:2]
            assert abs(e - ref.elbo) <= 1e-9 * abs(ref.elbo)
            assert np.abs(g - ref.grad).max() <= 1e-7 * np.abs(ref.grad).max()
            assert abs(e - e1) <= 1e-10 * abs(e1)
        assert all(r[1][k][0] == res[0][1][k][0] for r in res)         # every rank holds the identical value
    rm, rv = Kr.q_v(ref)
    for _, _, mean, var in res:
        assert np.abs(mean - rm).max() <= 1e-7 * np.abs(rm).max()
        assert np.abs(var - rv).max() <= 1e-7 * np.abs(rv).max()


def test_sharded_rbf_runs_the_subspace_start(engine):
    """RBF factors (numerically rank-deficient Gram matrices): the split partials -> all-reduce -> finish path takes the
    subspace start once the ranks are known (few rotation rounds) and still equals the oracle."""
    from oracle import dense as D, kron as Kr
    world, kind, m1, m2 = 2, "rbf", 88, 80
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 1000)
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, kind, m1, m2)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    X, y, x1, x2 = D.gen_grid(N1, N2)
    f1 = Kr.Factor("points", kind, np.linspace(0, 1, m1), x1)
    f2 = Kr.Factor("points", kind, np.linspace(0, 1, m2), x2)
    for k in range(NSTEP):
        th = np.array(THETA) * (1.0 + 0.01 * k)
        ref = Kr.elbo_step(y.reshape(N2, N1), f1, f2, th)
        for rank, out, _, _ in res:
            e, g, rounds = out[k]
            assert abs(e - ref.elbo) <= 1e-8 * abs(ref.elbo)
            assert np.abs(g - ref.grad).max() <= 1e-6 * np.abs(ref.grad).max()
    assert all(r[1][NSTEP - 1][2] < 60 for r in res), [r[1][NSTEP - 1][2] for r in res]


# ---- BASELINE configs[3]: 4096 x 4096 RBF grid, sharded 4-way along the slow storage axis, m_d = 128 -----------------
C4_N, C4_M, C4_WORLD = 4096, 128, 4
C4_THETA = [0.2, 0.2, 1.0, 1.0, 0.0025]
C4_STEPS = 3


def _config4_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from oracle import dense as D
    from variational_gridded_gaussian_processes_amd import Engine
    from variational_gridded_gaussian_processes_amd.sharded import ShardedStep, make_engine, shard_rows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X, y, x1, x2 = D.gen_grid(C4_N, C4_N)
        del X
        rows = shard_rows(C4_N, rank, world)
        assert rows.stop - rows.start == C4_N // world           # the 1024-row x 4096 slab of the config
        g = np.linspace(0, 1, C4_M)
        eng = make_engine(0, transport="gloo")
        eng.plan("rbf", "points", g, x1, "rbf", "points", g, x2[rows], n_total=C4_N * C4_N, warm_start=True)
        Y = torch.tensor(y.reshape(C4_N, C4_N)[rows], device="cuda:0")
        sh = ShardedStep(eng)
        yy = sh.sumsq_total(Y)
        out = []
        for k in range(C4_STEPS):
            th = np.array(C4_THETA) * (1.0 + 0.01 * k)
            e, gr, info = sh.step(Y, yy, th)
            out.append((e, gr, info["jitter"]))
        mean, var = eng.qv()
        q.put((rank, out, mean.cpu().numpy(), var.cpu().numpy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_config4_four_ranks_1024x4096_slabs_vs_structured_oracle(engine):
    """BASELINE configs[3] as specified: 4096 x 4096 RBF grid, m_d = 128, four ranks each owning a 1024-row x 4096 slab,
    ONE all-reduce per step (gloo carries it here: four processes share the one GPU of the test box; RCCL on the node).
    Every rank's value / gradient / q(v) against oracle/kron.py on the FULL grid: value 1e-8, gradient 3e-6."""
    from oracle import dense as D, kron as Kr
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29800 + (os.getpid() % 1000)
    procs = [ctx.Process(target=_config4_worker, args=(r, C4_WORLD, port, q)) for r in range(C4_WORLD)]
    for p in procs:
        p.start()
    X, y, x1, x2 = D.gen_grid(C4_N, C4_N)          # the oracle runs while the ranks do
    del X
    g = np.linspace(0, 1, C4_M)
    f1, f2 = Kr.Factor("points", "rbf", g, x1), Kr.Factor("points", "rbf", g, x2)
    refs = [Kr.elbo_step(y.reshape(C4_N, C4_N), f1, f2, np.array(C4_THETA) * (1.0 + 0.01 * k)) for k in range(C4_STEPS)]
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for k, ref in enumerate(refs):
        for rank, out, _, _ in res:
            e, gr, jit = out[k]
            assert tuple(jit) == (ref.d1.jit, ref.d2.jit)
            assert abs(e - ref.elbo) <= 1e-8 * abs(ref.elbo), (k, rank, e, ref.elbo)
            # (3e-6: 16.8 M observations, cond(K + 1e-8 I) ~ 1e10 -- the gradient sits on the rounding of the Cholesky factor: 0.8e-6
            #  with the two-pivot elimination order of its diagonal blocks, 1.3e-6 with the four-pivot order; north star 1e-5)
            assert np.abs(gr - ref.grad).max() <= 3e-6 * np.abs(ref.grad).max(), (k, rank)
        assert all(r[1][k][0] == res[0][1][k][0] for r in res)         # identical on every rank (no broadcast needed)
    rm, rv = Kr.q_v(refs[-1])
    for _, _, mean, var in res:
        assert np.abs(mean - rm).max() <= 1e-6 * np.abs(rm).max()
        # (the posterior variance is 1e-6 of the prior variance here -- 16.8 M observations -- and still matches to 1e-6
        # relative: the read-out after warm-started steps re-runs the eigensolve cold, step.hip vg_accurate_state)
        assert np.abs(var - rv).max() <= 1e-6 * np.abs(rv).max()


def test_rccl_transport_size_one(engine):
    """The RCCL transport on the one GPU of the test box: a communicator of size one (unique id from vggp_unique_id,
    ncclCommInitRank inside vggp_create).  The step then runs the multi-rank sequence -- partials graph, ncclAllReduce of the
    packed payload ON THE STEP'S STREAM, finish graph, one host synchronisation -- and must equal the fused single-rank step
    bit for bit along a warm-started trajectory; vggp_allreduce / vggp_sumsq go through the same communicator."""
    from oracle import dense as D, kron as Kr
    from variational_gridded_gaussian_processes_amd import Engine
    n1, n2, m = 96, 70, 24
    X, y, x1, x2 = D.gen_grid(n1, n2)
    g = np.linspace(0, 1, m)
    eng = Engine(0, 1, 0, Engine.unique_id())
    assert eng.transport == "rccl"
    Y = torch.tensor(y.reshape(n2, n1), device="cuda")
    t = torch.arange(5, dtype=torch.float64, device="cuda")
    assert torch.equal(eng.allreduce(t.clone()), t)
    f1, f2 = Kr.Factor("points", "rbf", g, x1), Kr.Factor("points", "rbf", g, x2)
    for e in (eng, engine):
        e.plan("rbf", "points", g, x1, "rbf", "points", g, x2, warm_start=True)
    yy = eng.sumsq(Y)
    assert yy == engine.sumsq(Y)
    for k in range(6):
        th = np.array(THETA) * (1.0 + 0.01 * k)
        e_r, g_r, i_r = eng.elbo_step(Y, yy, th)
        e_s, g_s, i_s = engine.elbo_step(Y, yy, th)
        ref = Kr.elbo_step(y.reshape(n2, n1), f1, f2, th)
        assert abs(e_r - ref.elbo) <= 1e-8 * abs(ref.elbo) and np.abs(g_r - ref.grad).max() <= 1e-6 * np.abs(ref.grad).max()
        assert abs(e_r - e_s) <= 1e-12 * abs(e_s)
    eng.close()


# ---- masked grids across ranks (BASELINE configs[4] names 8 GPUs) ------------------------------------------------------------
MK_N1, MK_N2, MK_NK = 72, 60, 9          # B0 mesh with 8 x 8 cells: M = 64


def _masked_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from oracle import dense as D
    from variational_gridded_gaussian_processes_amd.sharded import make_engine, shard_rows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X, y, x1, x2 = D.gen_grid(MK_N1, MK_N2)
        Wn = (np.random.default_rng(1).uniform(size=(MK_N2, MK_N1)) < 0.7).astype(np.float64)
        rows = shard_rows(MK_N2, rank, world)
        mesh = np.linspace(0, 1, MK_NK)
        eng = make_engine(0, transport="gloo")
        eng.plan("matern12", "b0", mesh, x1, "matern12", "b0", mesh, x2[rows], n_total=MK_N1 * MK_N2)
        W = torch.tensor(Wn[rows], device="cuda:0")
        Ym = torch.tensor(y.reshape(MK_N2, MK_N1)[rows], device="cuda:0") * W
        yy = eng.sumsq(Ym)                       # summed over the ranks by the library
        out = []
        for k in range(3):
            th = np.array(THETA) * (1.0 + 0.02 * k)
            out.append(eng.elbo_step_masked(Ym, W, float(Wn.sum()), yy, th)[:2])
        mean, var = eng.qv_masked()
        xs = np.random.default_rng(3).uniform(0, 1, (40, 2))
        pm, pv = eng.posterior_masked(torch.tensor(xs, device="cuda:0"))
        q.put((rank, out, mean.cpu().numpy(), var.cpu().numpy(), pm.cpu().numpy(), pv.cpu().numpy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_masked_step_sharded_over_ranks(engine, world):
    """Config 5's split: every rank assembles the partial Phi_r of its grid rows, ONE all-reduce (3 M^2 + 3 M + n1 doubles),
    replicated dense factorisation, a second all-reduce of the row-sum scalars; equals the masked oracle on the full grid."""
    from oracle import dense as D, kron as Kr
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29900 + (os.getpid() % 1000) + world
    procs = [ctx.Process(target=_masked_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    X, y, x1, x2 = D.gen_grid(MK_N1, MK_N2)
    Wn = (np.random.default_rng(1).uniform(size=(MK_N2, MK_N1)) < 0.7).astype(np.float64)
    mesh = np.linspace(0, 1, MK_NK)
    f1, f2 = Kr.Factor("b0", "matern12", mesh, x1), Kr.Factor("b0", "matern12", mesh, x2)
    for k in range(3):
        ref = Kr.elbo_step_masked(y.reshape(MK_N2, MK_N1), Wn, f1, f2, np.array(THETA) * (1.0 + 0.02 * k))
        for rank, out, *_ in res:
            e, g = out[k]
            assert abs(e - ref.elbo) <= 1e-9 * abs(ref.elbo), (k, rank)
            assert np.abs(g - ref.grad).max() <= 1e-7 * np.abs(ref.grad).max(), (k, rank)
        assert all(r[1][k][0] == res[0][1][k][0] for r in res)
    rm, rv = Kr.q_v_masked(ref)
    xs = np.random.default_rng(3).uniform(0, 1, (40, 2))
    om, ov = Kr.posterior_masked(ref, f1, f2, xs)
    for _, _, mean, var, pm, pv in res:
        assert np.abs(mean - rm).max() <= 1e-7 * np.abs(rm).max() and np.abs(var - rv).max() <= 1e-7 * np.abs(rv).max()
        assert np.abs(pm - om).max() <= 1e-7 * np.abs(om).max() and np.abs(pv - ov).max() <= 1e-6 * np.abs(ov).max()


# ---- scattered points across ranks -------------------------------------------------------------------------------------------
SC_N, SC_M1, SC_M2 = 3000, 10, 8


def _scattered_points():
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (SC_N, 2))
    y = np.sin(5 * X[:, 0]) * np.cos(4 * X[:, 1]) + 0.05 * rng.normal(size=SC_N)
    return X, y


def _scattered_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from variational_gridded_gaussian_processes_amd.sharded import make_engine
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X, y = _scattered_points()
        cuts = np.linspace(0, SC_N, world + 1).astype(int) + np.array([0] + [37 * (k % 2) for k in range(1, world)] + [0])   # uneven shares
        mine = slice(cuts[rank], cuts[rank + 1])
        eng = make_engine(0, transport="gloo")
        eng.plan("matern32", "points", np.linspace(0, 1, SC_M1), X[mine, 0].copy(), "matern32", "points", np.linspace(0, 1, SC_M2),
                 X[mine, 1].copy(), scattered=True, n_total=SC_N)
        yd = torch.tensor(y[mine], device="cuda:0")
        out = []
        for k in range(2):
            th = np.array(THETA) * (1.0 + 0.02 * k)
            out.append(eng.elbo_step_scattered(yd, float(y @ y), th)[:2])
        mean, var = eng.qv_masked()
        gz1, gz2 = eng.zgrad_scattered(yd)
        q.put((rank, out, mean.cpu().numpy(), var.cpu().numpy(), gz1.cpu().numpy(), gz2.cpu().numpy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_scattered_step_sharded_over_points(engine, world):
    """Scattered observations split over ranks by POINTS (uneven shares): every rank assembles the partial sums of its points, ONE
    all-reduce (3 M^2 + 3 M doubles), replicated dense factorisation, a second all-reduce of the point-sum scalars; every rank
    equals the scattered oracle on all the points."""
    from oracle import kron as Kr
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29950 + (os.getpid() % 1000) + world
    procs = [ctx.Process(target=_scattered_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    X, y = _scattered_points()
    f1 = Kr.Factor("points", "matern32", np.linspace(0, 1, SC_M1), X[:, 0])
    f2 = Kr.Factor("points", "matern32", np.linspace(0, 1, SC_M2), X[:, 1])
    for k in range(2):
        ref = Kr.elbo_step_scattered(X, y, f1, f2, np.array(THETA) * (1.0 + 0.02 * k))
        for rank, out, *_ in res:
            e, g = out[k]
            assert abs(e - ref.elbo) <= 1e-9 * abs(ref.elbo), (k, rank)
            assert np.abs(g - ref.grad).max() <= 1e-7 * np.abs(ref.grad).max(), (k, rank)
        assert all(r[1][k][0] == res[0][1][k][0] for r in res)
    rm, rv = Kr.q_v_masked(ref)
    z1, z2 = Kr.z_grad_scattered(ref, X, y, f1, f2)          # Z-gradient: local parts + one all-reduce of m1 + m2 doubles
    for _, _, mean, var, gz1, gz2 in res:
        assert np.abs(mean - rm).max() <= 1e-7 * np.abs(rm).max() and np.abs(var - rv).max() <= 1e-7 * np.abs(rv).max()
        assert np.abs(gz1 - z1).max() <= 1e-6 * np.abs(z1).max() and np.abs(gz2 - z2).max() <= 1e-6 * np.abs(z2).max()


# ---- Z-gradient of a row-sharded full-grid job ---------------------------------------------------------------------------------
def _zgrad_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from oracle import dense as D
    from variational_gridded_gaussian_processes_amd.sharded import ShardedStep, make_engine, shard_rows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X, y, x1, x2 = D.gen_grid(N1, N2)
        rows = shard_rows(N2, rank, world)
        rng = np.random.default_rng(3)
        z1 = np.linspace(0.03, 0.97, M1) + rng.uniform(-0.02, 0.02, M1)
        z2 = np.linspace(0.03, 0.97, M2) + rng.uniform(-0.02, 0.02, M2)
        eng = make_engine(0, transport="gloo")
        eng.plan("matern32", "points", z1, x1, "matern32", "points", z2, x2[rows], n_total=N1 * N2)
        Y = torch.tensor(y.reshape(N2, N1)[rows], device="cuda:0")
        sh = ShardedStep(eng)
        e, g, info = sh.step(Y, sh.sumsq_total(Y), np.array(THETA))
        gz1, gz2 = eng.zgrad(Y)
        q.put((rank, e, gz1.cpu().numpy(), gz2.cpu().numpy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_zgrad_of_a_row_sharded_job(engine, world):
    """vggp_zgrad on an n_ranks > 1 context: each rank contracts the observations of its rows, the terms that only involve
    replicated state are added by rank 0, ONE all-reduce of m1 + m2 doubles; every rank equals oracle z_grad on the full grid."""
    from oracle import dense as D, kron as Kr
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29850 + (os.getpid() % 1000) + world
    procs = [ctx.Process(target=_zgrad_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    X, y, x1, x2 = D.gen_grid(N1, N2)
    rng = np.random.default_rng(3)
    z1 = np.linspace(0.03, 0.97, M1) + rng.uniform(-0.02, 0.02, M1)
    z2 = np.linspace(0.03, 0.97, M2) + rng.uniform(-0.02, 0.02, M2)
    f1, f2 = Kr.Factor("points", "matern32", z1, x1), Kr.Factor("points", "matern32", z2, x2)
    Y = y.reshape(N2, N1)
    ref = Kr.elbo_step(Y, f1, f2, np.array(THETA))
    r1, r2 = Kr.z_grad(ref, f1, f2, Y)
    for rank, e, gz1, gz2 in res:
        assert abs(e - ref.elbo) <= 1e-9 * abs(ref.elbo)
        assert np.abs(gz1 - r1).max() <= 1e-6 * np.abs(r1).max() and np.abs(gz2 - r2).max() <= 1e-6 * np.abs(r2).max(), rank


# ---- failure of one rank: every rank gets an error, nobody hangs -----------------------------------------------------------------
FAULT_STEP = 3          # (the step counter of a context starts at 1)


def _fault_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    if rank == 1:
        os.environ["VGGP_FAULT_PARTIALS_AT"] = str(FAULT_STEP)      # this rank's partials "fail" at its 3rd step (csrc/step.hip)
    import torch.distributed as dist
    from oracle import dense as D
    from variational_gridded_gaussian_processes_amd import VggpError
    from variational_gridded_gaussian_processes_amd.sharded import make_engine, shard_rows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X, y, x1, x2 = D.gen_grid(N1, N2)
        rows = shard_rows(N2, rank, world)
        eng = make_engine(0, transport="gloo")
        eng.plan("matern32", "points", np.linspace(0, 1, M1), x1, "matern32", "points", np.linspace(0, 1, M2), x2[rows],
                 n_total=N1 * N2, warm_start=True)
        Y = torch.tensor(y.reshape(N2, N1)[rows], device="cuda:0")
        yy = eng.sumsq(Y)
        out = []
        for k in range(5):
            th = np.array(THETA) * (1.0 + 0.01 * k)
            try:
                e, g, info = eng.elbo_step(Y, yy, th)
                out.append(("ok", e))
            except VggpError as ex:
                out.append(("err", ex.code, str(ex)))
        q.put((rank, out))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_a_failing_rank_is_an_error_on_every_rank_not_a_hang(engine):
    """a rank whose half of the step fails must not leave its peers inside the all-reduce.  Rank 1's partials fail at
    step 3 (fault injection): it still joins the collective, with a zero payload and the failure word set, so BOTH ranks return
    an error for that step (the failing rank its own, the peer VGGP_ERCCL) and both continue with the next step, which again
    equals the single-rank result."""
    from oracle import dense as D
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29900 + (os.getpid() % 1000)
    procs = [ctx.Process(target=_fault_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    X, y, x1, x2 = D.gen_grid(N1, N2)
    engine.plan("matern32", "points", np.linspace(0, 1, M1), x1, "matern32", "points", np.linspace(0, 1, M2), x2, warm_start=True)
    Y = torch.tensor(y.reshape(N2, N1), device="cuda")
    for k in range(5):
        e1, _, _ = engine.elbo_step(Y, engine.sumsq(Y), np.array(THETA) * (1.0 + 0.01 * k))
        for rank, out in res:
            if k == FAULT_STEP - 1:
                assert out[k][0] == "err", (rank, out[k])
                assert out[k][1] == (-3 if rank == 1 else -7), (rank, out[k])          # VGGP_EHIP (injected) / VGGP_ERCCL (peer)
                assert ("injected fault" in out[k][2]) if rank == 1 else ("rank(s) of the job failed" in out[k][2])
            else:
                assert out[k][0] == "ok" and abs(out[k][1] - e1) <= 1e-9 * abs(e1), (rank, k, out[k], e1)


# ---- RCCL between devices: runs only where more than one GPU is visible ----------------------------------------------------------
def _rccl_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from oracle import dense as D
    from variational_gridded_gaussian_processes_amd.sharded import make_engine, shard_rows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)       # bootstrap of the unique id only
    try:
        X, y, x1, x2 = D.gen_grid(N1, N2)
        rows = shard_rows(N2, rank, world)
        dev = f"cuda:{rank}"
        eng = make_engine(rank, transport="rccl")                      # one device per rank, the context owns the communicator
        assert eng.n_ranks == world and eng.transport == "rccl"
        eng.plan("matern32", "points", np.linspace(0, 1, M1), x1, "matern32", "points", np.linspace(0, 1, M2), x2[rows],
                 n_total=N1 * N2, warm_start=True)
        Y = torch.tensor(y.reshape(N2, N1)[rows], device=dev)
        yy = eng.sumsq(Y)
        out = []
        for k in range(NSTEP):
            e, g, info = eng.elbo_step(Y, yy, np.array(THETA) * (1.0 + 0.01 * k))
            out.append((e, g))
        q.put((rank, out))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: RCCL refuses two ranks on one device")
def test_rccl_all_reduce_between_two_devices():
    """The transport bench.py --gpus N uses -- one process per GPU, RCCL communicator inside the context, partials graph ->
    ncclAllReduce on the step's stream -> finish graph -- on two real devices: every rank equals the oracle on the full grid."""
    from oracle import dense as D, kron as Kr
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29800 + (os.getpid() % 1000)
    procs = [ctx.Process(target=_rccl_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    X, y, x1, x2 = D.gen_grid(N1, N2)
    f1 = Kr.Factor("points", "matern32", np.linspace(0, 1, M1), x1)
    f2 = Kr.Factor("points", "matern32", np.linspace(0, 1, M2), x2)
    for k in range(NSTEP):
        ref = Kr.elbo_step(y.reshape(N2, N1), f1, f2, np.array(THETA) * (1.0 + 0.01 * k))
        for rank, out in res:
            e, g = out[k]
            assert abs(e - ref.elbo) <= 1e-9 * abs(ref.elbo) and np.abs(g - ref.grad).max() <= 1e-7 * np.abs(ref.grad).max()
        assert res[0][1][k][0] == res[1][1][k][0]
