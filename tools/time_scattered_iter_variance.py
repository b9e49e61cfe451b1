"""ms of the point-wise variance read-outs of the iterative scattered step (vggp_qv_var_scattered_iter,
vggp_posterior_var_scattered_iter) at N = 100 000 uniform points, inducing points on a grid of m_d = 128 and 256 per dimension
(Matern-1/2, theta_b of tests/scattered_iter_spec.py, tol 1e-10): ONE 64-point posterior block solve and ONE 64-cell q(v) block solve,
with their PCG iteration counts and the time per iteration.  Their yardstick is the conditional 64-cell solve of
vggp_readout_scattered_iter in profiles/gridded_iter_readout_times.json (the same solver on other right-hand sides).

Also the field kernel with two columns per workgroup (vggp_kr_field2) against the four-column one (vggp_kr_field) at nb = 64 and
nb = 16: the two alternate within each of `--rounds` rounds and every round's median is kept, so the spread between rounds is in the
file, with the verdict of the rule "faster in every round by more than the largest round-to-round difference of either kernel".
HIP events, median of 10 after 3 warm-ups.  Writes profiles/scattered_iter_variance_times.json.

    python tools/time_scattered_iter_variance.py [--n 100000] [--sizes 128,256] [--kernels-only] [--out profiles/scattered_iter_variance_times.json]
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


def kernel_rows(e, n, sizes, rounds):
    rows = []
    for m in sizes:
        L = torch.randn(m, n, dtype=torch.float64, device="cuda")
        R = torch.randn(m, n, dtype=torch.float64, device="cuda")
        for nb in (64, 16):
            V = torch.randn(m, nb, m, dtype=torch.float64, device="cuda")
            same = bool(torch.equal(e.kr_field(L, R, V, cols_per_wg=2), e.kr_field(L, R, V)))
            two, four = [], []
            for _ in range(rounds):
                two.append(timed(lambda: e.kr_field(L, R, V, cols_per_wg=2)))
                four.append(timed(lambda: e.kr_field(L, R, V)))
            wobble = max(max(abs(a - b) for a, b in zip(t[1:], t[:-1])) for t in (two, four))
            fl = 2.0 * m * m * nb * n
            row = {"m_d": m, "N": n, "nb": nb, "flop": fl, "rounds": rounds, "two_column_ms_per_round": two, "four_column_ms_per_round": four,
                   "two_column_ms": float(np.median(two)), "four_column_ms": float(np.median(four)),
                   "two_column_tflops": fl / (float(np.median(two)) * 1e-3) / 1e12, "four_column_tflops": fl / (float(np.median(four)) * 1e-3) / 1e12,
                   "largest_round_to_round_difference_ms": wobble,
                   "faster_in_every_round_by_more_than_that": all(f - t > wobble for t, f in zip(two, four)),
                   "not_slower": float(np.median(two)) <= float(np.median(four)), "bitwise_equal": same}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def add_yardstick(res):
    """Beside each block solve: the conditional 64-cell solve of vggp_readout_scattered_iter that profiles/gridded_iter_readout_times.json
    recorded on the four-column field kernel (the same solver on other right-hand sides), per iteration."""
    path = os.path.join(ROOT, "profiles", "gridded_iter_readout_times.json")
    if not os.path.exists(path):
        return
    with open(path) as f:
        rows = json.load(f)["readouts"]
    for row in res["block_solves"]:
        ref = [r for r in rows if r["m_d"] == row["m_d"]]
        if ref:
            ms, its = ref[0]["conditional_one_block_64_cells_ms"], ref[0]["block_pcg_iterations"]
            row["yardstick_conditional_64_cells"] = {"ms": ms, "pcg_iterations": its, "ms_per_iteration": ms / its,
                                                     "source": "profiles/gridded_iter_readout_times.json (four-column field kernel)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scattered_iter_variance_times.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    e = Engine(0)
    sizes = [int(s) for s in a.sizes.split(",")]
    rng = np.random.default_rng(0)
    X = rng.random((a.n, 2))
    y = datagen.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(a.n)
    res = {"N": a.n, "theta": THETA, "n_probes": 16, "block": 64, "tol": 1e-10, "method": "HIP events, median of 10 after 3 warm-ups",
           "measured": True, "device": torch.cuda.get_device_name(0),
           "kr_field2_vs_kr_field": {"note": "both timings include the host call and its final stream synchronise (the exported entry points)",
                                     "rows": kernel_rows(e, a.n, sizes, a.rounds)},
           "block_solves": []}
    if not a.kernels_only:
        yd = torch.tensor(y, dtype=torch.float64, device="cuda")
        yy = float(y @ y)
        xs = torch.tensor(rng.random((64, 2)), dtype=torch.float64, device="cuda")
        for m in sizes:
            z = np.linspace(0.0, 1.0, m)
            e.plan("matern12", "points", z, X[:, 0], "matern12", "points", z, X[:, 1], scattered=True)
            step = e.elbo_step_scattered_iter(yd, yy, THETA)[2]
            cells = rng.choice(m * m, size=64, replace=False)
            out = {}

            def post():
                out["p"] = e.posterior_var_scattered_iter(xs)[2]

            def qv():
                out["q"] = e.qv_var_scattered_iter(cells=cells)[2]
            row = {"m_d": m, "M": m * m, "step_pcg_iterations": step["rounds"][0]}
            row["posterior_64_points_ms"] = timed(post)
            row["posterior_pcg_iterations"] = out["p"]["rounds"][0]
            row["posterior_ms_per_iteration"] = row["posterior_64_points_ms"] / max(row["posterior_pcg_iterations"], 1)
            row["qv_64_cells_ms"] = timed(qv)
            row["qv_pcg_iterations"] = out["q"]["rounds"][0]
            row["qv_ms_per_iteration"] = row["qv_64_cells_ms"] / max(row["qv_pcg_iterations"], 1)
            print(json.dumps(row), flush=True)
            res["block_solves"].append(row)
    add_yardstick(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
