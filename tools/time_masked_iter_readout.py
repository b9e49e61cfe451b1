"""ms of the iterative masked step's read-outs (vggp_qv_masked_iter, vggp_posterior_masked_iter) on the 2048 x 2048 grid with 30 %
missing of bench.py masked_iter, m_d = 128 and 256, beside the step's own time from the same run.
    python tools/time_masked_iter_readout.py [--out profiles/masked_iter_readout_times.json]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from variational_gridded_gaussian_processes_amd import Engine, datagen as D

torch.cuda.set_device(0)
eng = Engine(0)
n, n_probes, steps = 2048, 16, 3
X, y, x1, x2 = D.gen_grid(n, n)
del X
W = torch.tensor((np.random.default_rng(1).uniform(size=(n, n)) < 0.7).astype(np.float64), device=eng.device)
Ym = torch.tensor(y.reshape(n, n), device=eng.device) * W
nobs = float(W.sum().item())
rng = np.random.default_rng(7)
xs = torch.tensor(rng.uniform(0, 1, (4096, 2)), device=eng.device)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


out = {"n": n, "missing": 0.3, "n_probes": n_probes, "block": 64}
for m in (128, 256):
    mesh = np.linspace(0, 1, m + 1)
    eng.plan("matern12", "b0", mesh, x1, "matern12", "b0", mesh, x2)
    yy = eng.sumsq(Ym)
    eng.elbo_step_masked_iter(Ym, W, nobs, yy, bench.THETA0, n_probes=n_probes)
    ms_step, info = timed(lambda: [eng.elbo_step_masked_iter(Ym, W, nobs, yy, [t * (1 + 0.01 * (k + 1)) for t in bench.THETA0],
                                                             n_probes=n_probes)[2] for k in range(steps)][-1])
    cells = rng.choice(m * m, size=256, replace=False)
    eng.qv_masked_iter(W, nobs, cells=cells[:64])                     # first call: allocates the read-out workspace
    eng.posterior_masked_iter(xs[:64], W, nobs)
    ms_mean, _ = timed(lambda: eng.qv_masked_iter(W, nobs, variance=False))
    ms_one, one = timed(lambda: eng.qv_masked_iter(W, nobs, cells=cells[:64]))
    ms_var, qv = timed(lambda: eng.qv_masked_iter(W, nobs, cells=cells))
    ms_post, post = timed(lambda: eng.posterior_masked_iter(xs, W, nobs))
    r = {"M": m * m, "ms_step": ms_step / steps, "step_pcg_iterations": info["rounds"][0], "step_columns": n_probes + 1,
         "ms_qv_mean": ms_mean,
         "ms_one_block_solve_64_cells": ms_one, "one_block_pcg_iterations": one[2]["rounds"][0],
         "ms_qv_var_256_cells": ms_var, "qv_block_solves": qv[2]["sweeps"][0], "qv_pcg_iterations": qv[2]["rounds"][0],
         "ms_posterior_4096_points": ms_post, "posterior_block_solves": post[2]["sweeps"][0],
         "posterior_pcg_iterations": post[2]["rounds"][0],
         "var_min": float(qv[1].min().item()), "posterior_var_min": float(post[1].min().item())}
    r["ms_per_block_solve_posterior"] = ms_post / r["posterior_block_solves"]
    # what a 64-column solve would cost if it were the step's 17-column PCG widened: (step time) * 64 / 17 is an upper bound on that
    # figure, the step also pays for factors, traces and quadrature
    r["ms_step_scaled_64_over_17"] = r["ms_step"] * 64.0 / (n_probes + 1)
    out[f"m_d_{m}"] = r
txt = json.dumps(out, indent=1)
print(txt)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(txt + "\n")
