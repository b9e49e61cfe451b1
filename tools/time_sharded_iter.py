"""ms per step of the iterative masked step (2048 x 2048 grid, 30 % missing: the shapes of tools/time_masked_iter.py / bench_masked.py)
and of the iterative scattered step (100 000 uniform points: tools/time_scattered_iter.py) on 1 rank and on 2 ranks that SHARE ONE GPU,
the collectives carried by the host-callback transport over gloo.  This is a one-GPU rehearsal through a host-staged collective: the
two ranks take turns on the same device and every all-reduce goes device -> pinned host -> gloo -> device, so the numbers show what
the multi-rank sequence costs (one block-vector all-reduce per PCG iteration, two packed ones per step), NOT how the step scales.  No
multi-GPU curve has been measured.  Writes profiles/sharded_iter_times.json, which says the same in its own text.

    python tools/time_sharded_iter.py [--sizes 128] [--n 2048] [--points 100000] [--steps 3] [--out profiles/sharded_iter_times.json]
"""
import argparse
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.multiprocessing as mp

THETA_M = [0.2, 0.2, 1.0, 1.0, 0.0025]          # bench.py THETA0 (masked_iter_bench)
THETA_S = [0.1, 0.12, 0.7, 0.9, 0.01]           # tools/time_scattered_iter.py
NOTE = ("One-GPU rehearsal through a host-staged collective: the ranks of a multi-rank row share ONE MI355X and every all-reduce is "
        "staged through pinned host memory and gloo.  The rows show the overhead of the multi-rank sequence, not scaling; no "
        "multi-GPU curve has been measured.")


def _worker(rank, world, port, q, what, m, n, points, steps):
    import torch.distributed as dist
    from oracle import dense as D
    from variational_gridded_gaussian_processes_amd import Engine, datagen
    from variational_gridded_gaussian_processes_amd.sharded import make_engine, shard_rows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    try:
        torch.cuda.set_device(0)
        eng = make_engine(0, transport="gloo") if world > 1 else Engine(0)
        g = np.linspace(0.0, 1.0, m + 1)
        if what == "masked":
            _, y, x1, x2 = D.gen_grid(n, n)
            Wn = (np.random.default_rng(1).uniform(size=(n, n)) < 0.7).astype(np.float64)
            rows = shard_rows(n, rank, world)
            eng.plan("matern12", "b0", g, x1, "matern12", "b0", g, x2[rows], n_total=n * n)
            W = torch.tensor(Wn[rows], device="cuda")
            Ym = torch.tensor(y.reshape(n, n)[rows], device="cuda") * W
            nobs, yy = float(Wn.sum()), float(((y.reshape(n, n) * Wn) ** 2).sum())

            def step(k):
                return eng.elbo_step_masked_iter(Ym, W, nobs, yy, [t * (1 + 0.01 * k) for t in THETA_M])
        else:
            rng = np.random.default_rng(0)
            X = rng.random((points, 2))
            y = datagen.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(points)
            cuts = np.linspace(0, points, world + 1).astype(int)
            mine = slice(cuts[rank], cuts[rank + 1])
            eng.plan("matern12", "b0", g, X[mine, 0].copy(), "matern12", "b0", g, X[mine, 1].copy(), scattered=True, n_total=points)
            yd, yy = torch.tensor(y[mine], device="cuda"), float(y @ y)

            def step(k):
                return eng.elbo_step_scattered_iter(yd, yy, THETA_S)
        step(0)                                      # cold: solves the preconditioner's eigenproblem
        ms = []
        for k in range(1, steps + 1):
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            e, _, info = step(k)
            ms.append((time.perf_counter() - t0) * 1e3)
        if rank == 0:
            q.put({"step": what, "ranks": world, "m_d": m, "M": m * m, "ms_per_step": float(np.median(ms)), "ms": ms,
                   "pcg_iterations": info["rounds"][0], "elbo_last": e})
        dist.barrier()
    except Exception as e:          # noqa: BLE001 -- main() hears about it instead of waiting for its time limit
        q.put({"error": repr(e), "rank": rank})
        raise
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128")
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_iter_times.json"))
    a = ap.parse_args()
    ctx = mp.get_context("spawn")
    res = {"note": NOTE, "transport": "host callback over gloo, all ranks on one GPU", "grid": [a.n, a.n], "points": a.points,
           "n_probes": 16, "rows": []}
    job = 0
    for m in [int(s) for s in a.sizes.split(",")]:
        for what in ("masked", "scattered"):
            for world in (1, 2):
                q = ctx.Queue()
                port = 32300 + (os.getpid() % 400) + job
                job += 1
                procs = [ctx.Process(target=_worker, args=(r, world, port, q, what, m, a.n, a.points, a.steps)) for r in range(world)]
                for p in procs:
                    p.start()
                try:
                    row = q.get(timeout=900)
                    for p in procs:
                        p.join(120)
                finally:
                    for p in procs:
                        if p.is_alive():
                            p.terminate()
                print(json.dumps(row), flush=True)
                if "error" in row:
                    sys.exit(1)
                res["rows"].append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
