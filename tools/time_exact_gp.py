"""ms of the exact GP (vggp_exact_step and its read-outs) at N = 1024, 4096, 16384 uniform points with Matern-1/2 and at N = 4096 with
Matern-3/2, Matern-5/2 and RBF (theta of tests/test_gpu_exact_gp.py): the step, its split into Sigma build / Cholesky + inverse / alpha /
gradient pass (the engine's per-stage events, vggp_profile, in runs of their own), the gradient pass's GB/s over the nominal 8 N^2
bytes of Sigma^-1 and over the bytes of the upper tiles it actually reads, posterior(x*) at 1000 points, and q(v) on 32 x 32 B0 cells
with both variances.  In the same run, as the yardstick, the existing paired scattered step with Z = X at the same N
(Engine.plan_paired + elbo_step_scattered): the exact step does one factorisation where that one does two and has none of its
M x M x N passes, so it should be no slower at any N; both numbers and their ratio are recorded.
HIP events, median of 10 after 3 warm-ups.  Writes profiles/exact_gp_times.json.

    python tools/time_exact_gp.py [--sizes 1024,4096,16384] [--kinds-n 4096] [--no-yardstick] [--out profiles/exact_gp_times.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from variational_gridded_gaussian_processes_amd import Engine, VggpError, datagen
from variational_gridded_gaussian_processes_amd.models import _b0_kvv_diag_unit

THETA = [0.3, 0.25, 1.3, 0.8, 0.05]
HBM_PEAK_GBS = 6290.0          # measured float4 copy on the MI355X (8.0 TB/s spec)
STAGES = {"factor_build": "sigma_build_ms", "cholesky_inverse": "cholesky_inverse_ms", "gemm_C(B1*S)": "alpha_ms",
          "final_reduce": "gradient_pass_ms"}


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


def row_for(e, kind, n, yardstick):
    rng = np.random.default_rng(0)
    X = rng.random((n, 2))
    y = datagen.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(n)
    yd = torch.tensor(y, dtype=torch.float64, device="cuda")
    e.exact_plan(kind, kind, X[:, 0], X[:, 1])
    out = {}

    def step():
        out["s"] = e.exact_step(yd, THETA)
    row = {"kind": kind, "N": n, "step_ms": timed(step), "mll": out["s"][0], "jitter": out["s"][2]["jitter"][0]}
    # the split: per-stage events inside the step, a run of its own
    e.profile(True)
    e.profile_read(reset=True)
    for _ in range(13):
        step()
    ms, steps = e.profile_read(reset=True)
    e.profile(False)
    for stage, key in STAGES.items():
        row[key] = ms[stage] / max(steps, 1)
    tiles = (n + 63) // 64
    read = 8.0 * 64 * 64 * tiles * (tiles + 1) / 2
    g = row["gradient_pass_ms"] * 1e-3
    row["gradient_pass_gbs_over_8N2"] = 8.0 * n * n / g / 1e9
    row["gradient_pass_gbs_over_bytes_read"] = read / g / 1e9
    row["gradient_pass_share_of_hbm_peak_over_bytes_read"] = read / g / 1e9 / HBM_PEAK_GBS
    xs = torch.tensor(rng.random((1000, 2)), dtype=torch.float64, device="cuda")
    row["posterior_1000_points_ms"] = timed(lambda: e.exact_posterior(xs))
    if kind == "matern12":
        mesh = torch.linspace(0, 1, 33).double().cuda()
        x1, x2 = torch.tensor(X[:, 0], device="cuda").contiguous(), torch.tensor(X[:, 1], device="cuda").contiguous()
        C1 = e.factor_build("matern12", "b0", x1, mesh, THETA[0])[0]
        C2 = e.factor_build("matern12", "b0", x2, mesh, THETA[1])[0]
        kd1 = torch.full((32,), _b0_kvv_diag_unit(1.0 / 32, THETA[0]), dtype=torch.float64, device="cuda")
        kd2 = torch.full((32,), _b0_kvv_diag_unit(1.0 / 32, THETA[1]), dtype=torch.float64, device="cuda")
        row["q_v_32x32_literal_ms"] = timed(lambda: e.exact_readout(C1, C2, kd1, kd2, literal=True))
        row["q_v_32x32_conditional_ms"] = timed(lambda: e.exact_readout(C1, C2, kd1, kd2, literal=False))
    if yardstick:
        try:
            e.plan_paired(kind, X, X[:, 0], X[:, 1], scattered=True)
            yy = float(y @ y)

            def pstep():
                out["p"] = e.elbo_step_scattered(yd, yy, THETA)
            row["paired_z_equal_x_step_ms"] = timed(pstep)
            row["paired_z_equal_x_jitter"] = out["p"][2]["jitter"][0]
            row["paired_z_equal_x_elbo"] = out["p"][0]
            row["exact_over_paired"] = row["step_ms"] / row["paired_z_equal_x_step_ms"]
            row["exact_not_slower"] = row["step_ms"] <= row["paired_z_equal_x_step_ms"]
        except VggpError as err:          # (Kuu = K(X, X) carries no noise: it may not factor at every N)
            row["paired_z_equal_x_error"] = str(err)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--kinds-n", type=int, default=4096)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_gp_times.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    e = Engine(0)
    res = {"theta": THETA, "method": "HIP events, median of 10 after 3 warm-ups; the split: the engine's per-stage events, mean of 13 steps",
           "measured": True, "device": torch.cuda.get_device_name(0), "hbm_peak_gbs_measured_copy": HBM_PEAK_GBS, "rows": []}
    for n in [int(s) for s in a.sizes.split(",")]:
        res["rows"].append(row_for(e, "matern12", n, not a.no_yardstick))
    for kind in ("matern32", "matern52", "rbf"):
        res["rows"].append(row_for(e, kind, a.kinds_n, not a.no_yardstick))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
