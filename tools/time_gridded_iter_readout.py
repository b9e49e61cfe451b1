"""ms of the gridded read-out after the iterative scattered step (vggp_readout_scattered_iter) at N = 100 000 uniform points, inducing
points on a grid of m_d = 128 and 256 per dimension (Matern-1/2), output grids of 256^2 and 1024^2 B0 cells: the literal all-cells
read-out (one Gram product over the points, no solve) and ONE 64-column conditional block solve, beside the iterative step's own time
from the same run.  Also vg_kr_sqgram against its yardstick -- vggp_kr_back with nb = 1, F = 1 on pre-squared operands, the same
FLOP count -- at mv1 = mv2 = 256, N = 100 000: the two alternate within each of `--rounds` rounds and every round's median is kept,
so the spread between rounds is in the file.  HIP events, median of 10 after 3 warm-ups.  Writes profiles/gridded_iter_readout_times.json.

    python tools/time_gridded_iter_readout.py [--n 100000] [--sizes 128,256] [--grids 256,1024] [--out profiles/gridded_iter_readout_times.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from variational_gridded_gaussian_processes_amd import Engine, datagen
from variational_gridded_gaussian_processes_amd.models import _b0_cross_points, _b0_kvv_diag_unit

THETA = [0.1, 0.12, 0.7, 0.9, 0.01]


def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--grids", default="256,1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gridded_iter_readout_times.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    e = Engine(0)
    rng = np.random.default_rng(0)
    X = rng.random((a.n, 2))
    y = datagen.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(a.n)
    yd = torch.tensor(y, dtype=torch.float64, device="cuda")
    yy = float(y @ y)
    res = {"N": a.n, "theta": THETA, "n_probes": 16, "block": 64, "method": "HIP events, median of 10 after 3 warm-ups",
           "measured": True, "device": torch.cuda.get_device_name(0), "readouts": []}
    # the kernel against its yardstick, alternating
    mv = 256
    P1 = torch.randn(mv, a.n, dtype=torch.float64, device="cuda")
    P2 = torch.randn(mv, a.n, dtype=torch.float64, device="cuda")
    Q1, Q2 = P1 * P1, P2 * P2
    F1 = torch.ones(1, a.n, dtype=torch.float64, device="cuda")
    err = float(((e.kr_sqgram(P1, P2) - e.kr_back(Q1, Q2, F1)[:, 0, :]).abs().max() / e.kr_sqgram(P1, P2).abs().max()).item())
    sq, back = [], []
    for _ in range(a.rounds):
        sq.append(timed(lambda: e.kr_sqgram(P1, P2)))
        back.append(timed(lambda: e.kr_back(Q1, Q2, F1)))
    fl = 2.0 * mv * mv * a.n
    res["kr_sqgram_vs_kr_back"] = {
        "mv1": mv, "mv2": mv, "N": a.n, "flop": fl, "rounds": a.rounds, "sqgram_ms_per_round": sq, "kr_back_nb1_presquared_ms_per_round": back,
        "sqgram_ms": float(np.median(sq)), "kr_back_ms": float(np.median(back)), "sqgram_spread_ms": [min(sq), max(sq)],
        "kr_back_spread_ms": [min(back), max(back)], "sqgram_tflops": fl / (float(np.median(sq)) * 1e-3) / 1e12,
        "operand_bytes": 2.0 * mv * a.n * 8, "max_rel_difference": err,
        "note": "both timings include the host call and its final stream synchronise (the exported entry points)"}
    print(json.dumps(res["kr_sqgram_vs_kr_back"]), flush=True)
    del P1, P2, Q1, Q2, F1
    for m in [int(s) for s in a.sizes.split(",")]:
        z = np.linspace(0.0, 1.0, m)
        e.plan("matern12", "points", z, X[:, 0], "matern12", "points", z, X[:, 1], scattered=True)
        info = {}

        def step():
            info.update(e.elbo_step_scattered_iter(yd, yy, THETA)[2])
        step_ms = timed(step)
        zt = torch.tensor(z)
        for ns in [int(s) for s in a.grids.split(",")]:
            mesh = torch.linspace(0.0, 1.0, ns + 1, dtype=torch.float64)
            C1, C2 = _b0_cross_points(mesh, zt, THETA[0]), _b0_cross_points(mesh, zt, THETA[1])
            kd1 = torch.full((ns,), _b0_kvv_diag_unit(1.0 / ns, THETA[0]), dtype=torch.float64)
            kd2 = torch.full((ns,), _b0_kvv_diag_unit(1.0 / ns, THETA[1]), dtype=torch.float64)
            ops = [t.cuda() for t in (C1, C2, kd1, kd2)]
            cells = rng.choice(ns * ns, size=64, replace=False)
            row = {"m_d": m, "M": m * m, "cells": ns * ns, "step_ms": step_ms, "step_pcg_iterations": info["rounds"][0]}
            row["mean_only_ms"] = timed(lambda: e.readout_scattered_iter(*ops, variance=False))
            row["literal_all_cells_ms"] = timed(lambda: e.readout_scattered_iter(*ops, literal=True))
            out = {}

            def solve():
                out["info"] = e.readout_scattered_iter(*ops, literal=False, cells=cells)[2]
            row["conditional_one_block_64_cells_ms"] = timed(solve)
            row["block_pcg_iterations"] = out["info"]["rounds"][0]
            row["literal_over_step"] = row["literal_all_cells_ms"] / step_ms
            print(json.dumps(row), flush=True)
            res["readouts"].append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
