"""Times of the iterative exact GP (vggp_exact_step_iter, vggp_exact_kmv) on along-track points (datagen.generate_track on a 2000 x 2000
field scaled to the unit box, every point moved inside its cell by default_rng(0)) at N = 16384, 32768 and 100 000 with Matern-1/2 and
Matern-3/2, theta of tests/test_gpu_exact_gp.py, the entry's defaults (16 probes, rank 64, tol 1e-10, at most 1000 iterations):
ms per step (one step, wall clock around the call after a warm-up step at N = 2048), its PCG iterations, ms per value-only kernel
product at the step's block width (17 columns: two accumulators; HIP events, median of 5 after 1 warm-up) and generated kernel
elements per second (N^2 per product).  A step that does not converge within max_iter is recorded as such with the time it took.
Next to the N = 16384 rows the dense step's time from profiles/exact_gp_times.json (uniform points, same N and theta) is repeated.
These are records, not thresholds.  Writes profiles/exact_gp_iter_times.json.

    python tools/bench_exact_iter.py [--sizes 16384,32768,100000] [--kinds matern12,matern32] [--out profiles/exact_gp_iter_times.json]
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

from variational_gridded_gaussian_processes_amd import Engine, VggpError, datagen

THETA = [0.3, 0.25, 1.3, 0.8, 0.05]
N_PROBES = 16


def track_points(n, field=2000):
    lon, lat = datagen.generate_track(field, field, 2, 0.5)
    pts = np.unique(np.stack([lon, lat], 1), axis=0)
    pts = pts[np.lexsort((pts[:, 1], pts[:, 0]))]
    pick = pts[(np.arange(n, dtype=np.int64) * len(pts)) // n]
    rng = np.random.default_rng(0)
    X = (pick + rng.random((n, 2))) / field
    return X, datagen.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(n)


def product_ms(e, kind, Xd, nb, reps=5):
    V = torch.ones(Xd.shape[0], nb, dtype=torch.float64, device="cuda")
    ms = []
    for k in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        e.exact_kmv(kind, kind, THETA[0], THETA[1], Xd, Xd, V)
        b.record()
        b.synchronize()
        if k:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def row_for(e, kind, n, dense_ms):
    X, y = track_points(n)
    yd = torch.tensor(y, dtype=torch.float64, device="cuda")
    Xd = torch.tensor(X, dtype=torch.float64, device="cuda")
    row = {"kind": kind, "N": n, "n_probes": N_PROBES, "rank": 64, "tol": 1e-10}
    row["product_ms_17_columns"] = product_ms(e, kind, Xd, 1 + N_PROBES)
    row["generated_elements_per_s"] = float(n) * n / (row["product_ms_17_columns"] * 1e-3)
    e.exact_iter_plan(kind, kind, X[:, 0], X[:, 1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        mll, _, info = e.exact_step_iter(yd, THETA, n_probes=N_PROBES)
        row.update(converged=True, mll=mll, pcg_iterations=info["rounds"][0], jitter=info["jitter"][0])
    except VggpError as err:
        row.update(converged=False, error=str(err))
    torch.cuda.synchronize()
    row["step_ms"] = (time.perf_counter() - t0) * 1e3
    if dense_ms is not None:
        row["dense_step_ms_same_N_uniform_points"] = dense_ms
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16384,32768,100000")
    ap.add_argument("--kinds", default="matern12,matern32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_gp_iter_times.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    e = Engine(0)
    dense = {}
    try:
        with open(os.path.join(ROOT, "profiles", "exact_gp_times.json")) as f:
            dense = {(r["kind"], r["N"]): r["step_ms"] for r in json.load(f)["rows"]}
    except OSError:
        pass
    Xw, yw = track_points(2048)          # warm-up: code objects, workspaces of the building blocks
    e.exact_iter_plan("matern32", "matern32", Xw[:, 0], Xw[:, 1])
    e.exact_step_iter(torch.tensor(yw, device="cuda"), THETA, n_probes=N_PROBES)
    res = {"theta": THETA, "measured": True, "device": torch.cuda.get_device_name(0),
           "method": "step: wall clock around one call; product: HIP events, median of 5 after 1 warm-up", "rows": []}
    for n in [int(s) for s in a.sizes.split(",")]:
        for kind in a.kinds.split(","):
            res["rows"].append(row_for(e, kind, n, dense.get(("matern12", n))))
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as f:          # (after every row: a long run that is cut short keeps what it measured)
                json.dump(res, f, indent=1)
                f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
