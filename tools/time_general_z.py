"""Timing of the paired (general) inducing points: one JSON line per shape with ms per training step (value, theta-gradient and
Z-gradient) and ms per q_v() read-out (10 x 10 B0 cells), device-synchronised, after warm-up.  Not imported by any test.

    python tools/time_general_z.py [--reps 5] [--shapes nb5,cv500,grid1024,pts4096]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from variational_gridded_gaussian_processes_amd import Engine  # noqa: E402
from variational_gridded_gaussian_processes_amd.datagen import gen_grid  # noqa: E402
from variational_gridded_gaussian_processes_amd.models import _b0_cross_points, _b0_kvv_diag_unit  # noqa: E402

SHAPES = {"nb5": ("grid", 25, 100), "cv500": ("points", 100_000, 500), "grid1024": ("grid", 1024, 1024), "pts4096": ("points", 100_000, 4096)}


def run(eng, name, layout, n, M, reps):
    rng = np.random.default_rng(0)
    theta = [0.3, 0.25, 0.8, 1.2, 0.01]
    Z = rng.random((M, 2))
    if layout == "grid":
        X, y, x1, x2 = gen_grid(n, n)
        Y = torch.tensor(y, device=eng.device).reshape(n, n).contiguous()
        eng.plan_paired("matern12", Z, x1, x2)
        yy = float((Y * Y).sum())
        step = lambda: (eng.elbo_step(Y, yy, theta), eng.zgrad(Y))
        N = n * n
    else:
        X = rng.random((n, 2))
        yt = torch.tensor(np.sin(5 * X[:, 0]) + np.cos(7 * X[:, 1]), device=eng.device)
        eng.plan_paired("matern12", Z, X[:, 0], X[:, 1], scattered=True)
        yy = float((yt * yt).sum())
        step = lambda: (eng.elbo_step_scattered(yt, yy, theta), eng.zgrad_scattered(yt))
        N = n
    mesh = torch.linspace(0, 1, 11).double()
    C1, C2 = _b0_cross_points(mesh, torch.tensor(Z[:, 0]), theta[0]), _b0_cross_points(mesh, torch.tensor(Z[:, 1]), theta[1])
    kd1 = torch.full((10,), _b0_kvv_diag_unit(0.1, theta[0]), dtype=torch.float64)
    kd2 = torch.full((10,), _b0_kvv_diag_unit(0.1, theta[1]), dtype=torch.float64)
    readout = lambda: eng.readout(C1, C2, kd1, kd2, literal=True, masked=True)

    def timed(fn):
        fn()
        torch.cuda.synchronize(eng.device)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(eng.device)
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))
    ms_step = timed(step)
    ms_qv = timed(readout)
    print(json.dumps(dict(shape=name, layout=layout, N=N, M=M, ms_step=round(ms_step, 3), ms_qv=round(ms_qv, 3), reps=reps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    eng = Engine(0)
    for name in a.shapes.split(","):
        run(eng, name, *SHAPES[name], a.reps)


if __name__ == "__main__":
    main()
