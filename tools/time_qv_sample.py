"""ms of joint samples of q(v) (vggp_qv_sample, vggp_qv_sample_masked_iter, vggp_qv_sample_scattered_iter; generated noise) at 64 and
1024 samples, B0 Matern-1/2 features, bench.py's THETA0, tol 1e-10:
    full       1024 x 1024 grid, m_d = 128
    masked     2048 x 2048 grid with 30 % of the nodes missing, m_d = 256
    scattered  100 000 uniform points, m_d = 128
Beside each figure, from the same run: ONE 64-column variance block solve at the same shape (q(v) variance of 64 cells:
vggp_qv_masked_iter / vggp_qv_var_scattered_iter; on the full grid, where no solve exists, vggp_qv of all cells) with its PCG iteration
count.  A 64-sample block runs the same solve at the same width; its right-hand sides are not rank one, so the iteration counts
differ and both are recorded.  A record, not a gate.

Method: each call is host-synchronous (it returns after its last kernel); wall clock around the call between device synchronisations,
median of `reps` after `warm` warm-up calls (the first call also allocates the workspace).  Writes profiles/qv_sample_times.json.

    python tools/time_qv_sample.py [--only full,masked,scattered] [--out profiles/qv_sample_times.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import bench
from variational_gridded_gaussian_processes_amd import Engine, datagen as D

SAMPLES = (64, 1024)


def timed(fn, reps, warm):
    out = None
    for _ in range(warm):
        out = fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), [float(t) for t in ms], out


def sample_rows(row, sample, reps64, reps1024):
    for S in SAMPLES:
        reps, warm = (reps64, 2) if S == 64 else (reps1024, 1)
        ms, all_ms, res = timed(lambda: sample(S), reps, warm)
        row[f"sample_{S}_ms"] = ms
        row[f"sample_{S}_ms_all"] = all_ms
        row[f"sample_{S}_reps_after_warmups"] = [reps, warm]
        if isinstance(res, tuple):
            row[f"sample_{S}_pcg_iterations"] = res[1]["rounds"][0]
            row[f"sample_{S}_block_solves"] = res[1]["sweeps"][0]
        row[f"sample_{S}_ms_per_sample"] = ms / S


def full(e, reps64, reps1024):
    n, m = 1024, 128
    _, y, x1, x2 = D.gen_grid(n, n)
    mesh = np.linspace(0, 1, m + 1)
    e.plan("matern12", "b0", mesh, x1, "matern12", "b0", mesh, x2)
    Y = torch.tensor(y.reshape(n, n), device=e.device)
    e.elbo_step(Y, e.sumsq(Y), bench.THETA0)
    row = {"shape": "full 1024 x 1024", "m_d": m, "M": m * m}
    sample_rows(row, lambda S: e.qv_sample(S, seed=1), reps64, reps1024)
    row["qv_all_cells_ms"], row["qv_all_cells_ms_all"], _ = timed(e.qv, reps64, 2)
    return row


def masked(e, reps64, reps1024):
    n, m = 2048, 256
    _, y, x1, x2 = D.gen_grid(n, n)
    mesh = np.linspace(0, 1, m + 1)
    W = torch.tensor((np.random.default_rng(1).uniform(size=(n, n)) < 0.7).astype(np.float64), device=e.device)
    Ym = torch.tensor(y.reshape(n, n), device=e.device) * W
    nobs = float(W.sum().item())
    e.plan("matern12", "b0", mesh, x1, "matern12", "b0", mesh, x2)
    step = e.elbo_step_masked_iter(Ym, W, nobs, e.sumsq(Ym), bench.THETA0)[2]
    cells = np.random.default_rng(7).choice(m * m, size=64, replace=False)
    row = {"shape": "masked 2048 x 2048, 30 % missing", "m_d": m, "M": m * m, "step_pcg_iterations": step["rounds"][0]}
    sample_rows(row, lambda S: e.qv_sample_masked_iter(W, nobs, S, seed=1), reps64, reps1024)
    ms, all_ms, res = timed(lambda: e.qv_masked_iter(W, nobs, cells=cells), reps64, 2)
    row.update(variance_64_cells_ms=ms, variance_64_cells_ms_all=all_ms, variance_64_cells_pcg_iterations=res[2]["rounds"][0])
    return row


def scattered(e, reps64, reps1024):
    N, m = 100000, 128
    rng = np.random.default_rng(0)
    X = rng.random((N, 2))
    y = D.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(N)
    mesh = np.linspace(0, 1, m + 1)
    e.plan("matern12", "b0", mesh, X[:, 0], "matern12", "b0", mesh, X[:, 1], scattered=True)
    yd = torch.tensor(y, dtype=torch.float64, device=e.device)
    step = e.elbo_step_scattered_iter(yd, float(y @ y), bench.THETA0)[2]
    cells = rng.choice(m * m, size=64, replace=False)
    row = {"shape": "100 000 scattered points", "m_d": m, "M": m * m, "step_pcg_iterations": step["rounds"][0]}
    sample_rows(row, lambda S: e.qv_sample_scattered_iter(S, seed=1), reps64, reps1024)
    ms, all_ms, res = timed(lambda: e.qv_var_scattered_iter(cells=cells), reps64, 2)
    row.update(variance_64_cells_ms=ms, variance_64_cells_ms_all=all_ms, variance_64_cells_pcg_iterations=res[2]["rounds"][0])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="full,masked,scattered")
    ap.add_argument("--reps64", type=int, default=7)
    ap.add_argument("--reps1024", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qv_sample_times.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    e = Engine(0)
    res = {"theta": list(bench.THETA0), "tol": 1e-10, "block": 64, "noise": "generated on the device (seed 1)", "measured": True,
           "device": torch.cuda.get_device_name(0),
           "method": "wall clock around the host-synchronous call between device synchronisations; median of reps after warm-ups "
                     "(sample_S_reps_after_warmups); every repeat is in *_ms_all",
           "rows": []}
    for name in a.only.split(","):
        row = {"full": full, "masked": masked, "scattered": scattered}[name](e, a.reps64, a.reps1024)
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
