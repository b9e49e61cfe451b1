"""ms of mean AND variance of posterior(x*) on a raster after the dense masked / scattered steps: Engine.posterior_raster_var_masked
(vggp_posterior_raster_var_masked: the raster mean, then the two-stage separable contraction against the state's dense Sinv) against
the route there was before, Engine.posterior_masked (vggp_posterior_masked) at the cartesian points, in the same process.

    scattered   100 000 uniform points, B0 Matern-1/2 cells, m_d = 32 (M = 1024), one vggp_elbo_step_scattered; maps 256^2 and 1024^2
    masked64    2048 x 2048 grid with 30 % missing, m_d = 64 (M = 4096), one vggp_elbo_step_masked; maps 256^2 and 1024^2
    masked128   the same grid, m_d = 128 (M = 16384); the new entry at 256^2 and 1024^2, the point-wise route at 256^2 ONLY (its 1024^2
                figure is recorded as not measured: 5.4e14 flops per call)
    stage1      vggp_kron_quadform at M = 16384, P1 = 1024, P2 = 1 on a random matrix: the second stage is then 2 P1 m2^2 flops, so the
                call is stage 1 -- 2 P1 M^2 flops against the fp64-MFMA peak (78.6 TFLOP/s), and the least HBM traffic 8 M^2 bytes
                against 6.29 TB/s achievable.  A host-clock figure of the whole call, not a kernel time.
Both routes' variances are compared at every timed size (largest difference relative to the largest variance).  A record, not a gate;
the condition read from it is raster_var_ms < pointwise_ms at every measured size.

Method: host clock around a window of calls between device synchronisations; a window holds as many calls as last 250 ms or more
(counted from the last warm-up round) and is divided by that count; the two routes alternate inside one loop, warm-up rounds first (the
first call allocates the workspace), median of the timed windows.  Writes profiles/posterior_raster_var_times.json.

    python tools/bench_posterior_raster_var.py [--only scattered,masked64,masked128,stage1] [--out FILE]
    python tools/bench_posterior_raster_var.py --stage1-calls 3        # nothing but that many stage-1 calls: the target of a counter run
    python tools/bench_posterior_raster_var.py --merge-fetch BYTES     # add the counter run's bytes per stage-1 launch to the file

The HBM traffic of stage 1 comes from a counter run of its own (rocprofv3 --pmc FETCH_SIZE around --stage1-calls: one counter per pass, no
tracing beside it); FETCH_SIZE counts a wide streaming read at half its bytes on this chip and is uncalibrated for 8-byte-per-lane loads, so the
file records the raw counter next to the algorithmic bytes and says so.
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

WINDOW_MS = 250.0
PEAK_FP64_MFMA = 78.6e12          # DESIGN.md section 2 (tools/ubench/mfma64.hip)
HBM_ACHIEVABLE = 6.29e12
OUT = os.path.join(ROOT, "profiles", "posterior_raster_var_times.json")


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def axes(P, device):
    rng = np.random.default_rng(P)
    g1, g2 = np.sort(rng.uniform(0, 1, P)), np.sort(rng.uniform(0, 1, P))
    return torch.tensor(g1, device=device), torch.tensor(g2, device=device)


def windows(fns, reps, warm):
    """fns: {name: call} -> {name: (median ms, all ms, calls per window)}, last results; the routes alternate inside one loop."""
    ms = {k: [] for k in fns}
    inner = {k: 1 for k in fns}
    out = {}
    for it in range(warm + reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner[name] if it >= warm else 1):
                out[name] = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if it >= warm:
                ms[name].append(dt / inner[name])
            elif it == warm - 1:
                inner[name] = int(min(20000, max(1, np.ceil(WINDOW_MS / dt))))
    return {k: (float(np.median(v)), [float(t) for t in v], inner[k]) for k, v in ms.items()}, out


def time_sizes(e, M, m2, sizes, pointwise_sizes, reps=5, warm=2):
    rows = []
    for P in sizes:
        g1, g2 = axes(P, e.device)
        fns = {"raster_var": lambda: e.posterior_raster_var_masked(g1, g2)}
        if P in pointwise_sizes:
            xs = torch.cartesian_prod(g1, g2)                # point a * P + b = (g1[a], g2[b])
            fns["pointwise"] = lambda: e.posterior_masked(xs)
        t, out = windows(fns, reps, warm)
        row = {"raster": f"{P} x {P}", "points": P * P, "reps_after_warmups": [reps, warm],
               "flops_raster_var": 2.0 * P * M * M + 2.0 * P * P * m2 * m2, "flops_pointwise": 2.0 * P * P * M * M,
               "raster_var_ms": t["raster_var"][0], "raster_var_ms_all": t["raster_var"][1], "raster_var_calls_per_window": t["raster_var"][2]}
        if "pointwise" in t:
            row.update({"pointwise_ms": t["pointwise"][0], "pointwise_ms_all": t["pointwise"][1],
                        "pointwise_calls_per_window": t["pointwise"][2], "pointwise_over_raster_var": t["pointwise"][0] / t["raster_var"][0],
                        "mean_raster_vs_pointwise": rel(out["raster_var"][0].reshape(-1), out["pointwise"][0]),
                        "var_raster_vs_pointwise": rel(out["raster_var"][1].reshape(-1), out["pointwise"][1])})
        else:
            row["pointwise_ms"] = "not measured"
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
        out.clear()
        torch.cuda.empty_cache()
    return rows


def scattered_state(e):
    N, m = 100_000, 32
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (N, 2))
    y = D.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(N)
    mesh = np.linspace(0, 1, m + 1)
    e.plan("matern12", "b0", mesh, X[:, 0].copy(), "matern12", "b0", mesh, X[:, 1].copy(), scattered=True)
    elbo, grad, info = e.elbo_step_scattered(torch.tensor(y, device=e.device), float(y @ y), bench.THETA0)
    assert info["status"] == 0
    return {"state": f"{N} uniform points, matern12, b0, m_d = {m} (M = {m * m}), one vggp_elbo_step_scattered at bench.py's THETA0",
            "sizes": time_sizes(e, m * m, m, (256, 1024), (256, 1024))}


def masked_state(e, m, pointwise_sizes):
    n = 2048
    _, y, x1, x2 = D.gen_grid(n, n)
    W = (np.random.default_rng(1).uniform(size=(n, n)) > 0.3).astype(np.float64)
    mesh = np.linspace(0, 1, m + 1)
    e.plan("matern12", "b0", mesh, x1, "matern12", "b0", mesh, x2)
    Wd = torch.tensor(W, device=e.device)
    Ym = torch.tensor(y.reshape(n, n), device=e.device) * Wd
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    elbo, grad, info = e.elbo_step_masked(Ym, Wd, float(W.sum()), e.sumsq(Ym), bench.THETA0)
    torch.cuda.synchronize()
    assert info["status"] == 0
    return {"state": f"{n} x {n} grid, 30 % missing, matern12, b0, m_d = {m} (M = {m * m}), one vggp_elbo_step_masked at bench.py's THETA0",
            "step_s_first_call": time.perf_counter() - t0, "sizes": time_sizes(e, m * m, m, (256, 1024), pointwise_sizes)}


def stage1_operands(e, m=128, P1=1024):
    gen = torch.Generator(device=e.device).manual_seed(0)
    S = torch.randn(m * m, m * m, dtype=torch.float64, device=e.device, generator=gen)
    U1 = torch.randn(m, P1, dtype=torch.float64, device=e.device, generator=gen)
    U2 = torch.randn(m, 1, dtype=torch.float64, device=e.device, generator=gen)
    return S, U1, U2


def stage1(e):
    m, P1 = 128, 1024
    S, U1, U2 = stage1_operands(e, m, P1)
    out = torch.empty(P1, 1, dtype=torch.float64, device=e.device)
    t, _ = windows({"stage1": lambda: e.kron_quadform(S, U1, U2, out=out)}, 5, 2)
    ms, M = t["stage1"][0], m * m
    flops, byts = 2.0 * P1 * M * M, 8.0 * M * M
    return {"shape": f"M = {M} (m_d = {m}), P1 = {P1}, P2 = 1, random operands: vggp_kron_quadform, whole call on the host clock",
            "ms": ms, "ms_all": t["stage1"][1], "calls_per_window": t["stage1"][2], "flops": flops, "tflops": flops / ms / 1e9,
            "fraction_of_fp64_mfma_peak_78.6": flops / (ms * 1e-3) / PEAK_FP64_MFMA,
            "algorithmic_bytes_8M2": byts, "ms_at_achievable_hbm_6.29TBs": byts / HBM_ACHIEVABLE * 1e3,
            "bound": "fp64 MFMA (flops / peak = %.2f ms against %.2f ms of HBM time)" % (flops / PEAK_FP64_MFMA * 1e3, byts / HBM_ACHIEVABLE * 1e3),
            "hbm_fetch_bytes_per_stage1_launch": "not measured"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="scattered,masked64,masked128,stage1")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--stage1-calls", type=int, default=0)
    ap.add_argument("--merge-fetch", type=float, default=None)
    args = ap.parse_args()
    if args.merge_fetch is not None:
        with open(args.out) as f:
            res = json.load(f)
        s = res["stage1"]
        s["hbm_fetch_bytes_per_stage1_launch"] = args.merge_fetch
        s["hbm_fetch_over_algorithmic_8M2"] = args.merge_fetch / s["algorithmic_bytes_8M2"]
        s["hbm_fetch_note"] = ("FETCH_SIZE of the stage-1 launch from a counter run of its own, raw: the counter tallies wide streaming reads "
                               "at half their bytes on this chip and is uncalibrated for this kernel's 8-byte-per-lane loads")
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_posterior_raster_var needs the GPU: nothing is timed without one")
    e = Engine(0)
    if args.stage1_calls:
        S, U1, U2 = stage1_operands(e)
        for _ in range(args.stage1_calls):
            e.kron_quadform(S, U1, U2)
        torch.cuda.synchronize()
        return
    res = {}
    if os.path.exists(args.out):          # a run of some of the cases (--only) keeps the others' records
        with open(args.out) as f:
            res = json.load(f)
    res.update({"device": torch.cuda.get_device_name(0),
           "method": "host clock around windows of >= 250 ms of calls between device synchronisations, routes alternating, median of the "
                     "timed windows after warm-ups; ms per whole call (factor build, GEMMs, every launch)"})
    only = args.only.split(",")
    if "scattered" in only:
        res["scattered"] = scattered_state(e)
    if "masked64" in only:
        res["masked64"] = masked_state(e, 64, (256, 1024))
    if "masked128" in only:
        res["masked128"] = masked_state(e, 128, (256,))
        res["masked128"]["note"] = "point-wise route at 1024 x 1024 not measured (5.4e14 flops per call); no extrapolation recorded"
    if "stage1" in only:
        res["stage1"] = stage1(e)
    rows = [r for k in ("scattered", "masked64", "masked128") if k in res for r in res[k]["sizes"] if r["pointwise_ms"] != "not measured"]
    res["raster_var_faster_at_every_measured_size"] = all(r["raster_var_ms"] < r["pointwise_ms"] for r in rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
