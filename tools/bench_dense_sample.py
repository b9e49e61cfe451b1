"""ms of the joint samplers of the dense masked / scattered states: the triangular product X = Xg^T E on its own (vggp_tri_t_apply,
csrc/dense_sample.hip) beside the same product through the batch GEMM with VG_TRI_B_LOWER, and Engine.qv_sample_masked /
posterior_raster_sample_masked end to end, 64 samples per call.

    kernel      M in {1024, 4096, 16384}, 64 sample columns, a random lower-triangular Xl (true zeros above the diagonal) and E in the layout
                [1][64][M] (m1 = 1: the one layout both routes take); the dedicated kernel and the GEMM route alternate inside one loop,
                in one process, on the same operands.  Per route: ms, the read rate 4 M^2 bytes / time, its fraction of the 5.1 TB/s the
                factor builder reaches (README) and of the 6.29 TB/s achievable, and the share of the fp64-MFMA bound 64 M^2 flops at
                78.6 TFLOP/s.  The kernel alone also in the square layout m1 = m2 = sqrt(M).  Both results are compared.
    q_v         per call of 64 samples on the README's two dense states (100 000 scattered points, M = 1024; 2048^2 grid with 30 %
                missing, M = 4096) and at M = 16384 (the same grid, m_d = 128); beside it the route of dense_samples=False
                (models._dense_sampler: vggp_qv_cov_masked, the symmetric root on the host, one product), which stops at M = 4096.
    maps        a 256^2 and a 1024^2 map from the first two states, the three per-axis roots timed on their own (roots_ms, as in
                profiles/posterior_sample_times.json).
A record, not a gate; the condition read from it: kernel_ms <= gemm_ms at M = 16384.

Method: the product: HIP events around a window of back-to-back asynchronous calls on one stream, a window holds as many calls as last
20 ms or more and is divided by that count, `warm` untimed windows first, median of `reps` windows, every window kept in *_ms_all.
The entries: host clock around one host-synchronous call between device synchronisations, one warm-up call (it allocates the
workspace), median of `reps` calls, every repeat kept.  Writes profiles/dense_sample_times.json.

    python tools/bench_dense_sample.py [--only kernel,scattered,masked64,masked128] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bench
from bench_posterior_sample import axes, roots_ms, timed
from variational_gridded_gaussian_processes_amd import Engine, datagen as D
from variational_gridded_gaussian_processes_amd.models import _symmetric_root

S = 64
WINDOW_MS = 20.0
PEAK_FP64_MFMA = 78.6e12
FACTOR_BUILDER_RATE = 5.1e12      # README: the factor builder reaches 4.9-5.3 TB/s
HBM_ACHIEVABLE = 6.29e12
SWITCH = "VGGP_TRI_T_GEMM"


def event_windows(fns, reps, warm):
    """fns: {name: asynchronous call} -> {name: (median ms per call, all, calls per window)}; the routes alternate inside one loop."""
    ms = {k: [] for k in fns}
    inner = {k: 1 for k in fns}
    for it in range(warm + reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(inner[name]):
                fn()
            b.record()
            torch.cuda.synchronize()
            dt = a.elapsed_time(b)
            if it >= warm:
                ms[name].append(dt / inner[name])
            elif it == 0:
                inner[name] = int(min(2000, max(1, np.ceil(WINDOW_MS / max(dt, 1e-3)))))
    return {k: (float(np.median(v)), [float(t) for t in v], inner[k]) for k, v in ms.items()}


def kernel_rows(e, sizes, reps, warm):
    rows = []
    for M in sizes:
        gen = torch.Generator(device=e.device).manual_seed(M)
        Xl = torch.randn(M, M, dtype=torch.float64, device=e.device, generator=gen).tril_()
        E = torch.randn(1, S, M, dtype=torch.float64, device=e.device, generator=gen)
        out_k, out_g = torch.empty_like(E), torch.empty_like(E)
        r = int(round(M ** 0.5))
        Esq, out_sq = E.reshape(S, r, r).transpose(0, 1).contiguous(), torch.empty(r, S, r, dtype=torch.float64, device=e.device)

        def gemm():
            os.environ[SWITCH] = "1"
            try:
                e.tri_t_apply(Xl, E, out=out_g)
            finally:
                os.environ.pop(SWITCH, None)
        t = event_windows({"kernel": lambda: e.tri_t_apply(Xl, E, out=out_k), "gemm": gemm,
                           "kernel_square_layout": lambda: e.tri_t_apply(Xl, Esq, out=out_sq)}, reps, warm)
        nbytes, flops = 4.0 * M * M, float(S) * M * M
        row = {"M": M, "samples": S, "bytes_lower_triangle": nbytes, "flops": flops, "reps_after_warmups": [reps, warm],
               "kernel_vs_gemm_result": float((out_k - out_g).abs().max() / out_g.abs().max()),
               "square_layout_vs_flat_result": float((out_sq.transpose(0, 1).reshape(S, M) - out_k[0]).abs().max() / out_k.abs().max())}
        for name, (med, all_ms, inner) in t.items():
            row.update({f"{name}_ms": med, f"{name}_ms_all": all_ms, f"{name}_calls_per_window": inner,
                        f"{name}_read_TBps": nbytes / (med * 1e-3) / 1e12,
                        f"{name}_fraction_of_factor_builder_rate": nbytes / (med * 1e-3) / FACTOR_BUILDER_RATE,
                        f"{name}_fraction_of_hbm_achievable": nbytes / (med * 1e-3) / HBM_ACHIEVABLE,
                        f"{name}_share_of_mfma_bound": flops / PEAK_FP64_MFMA / (med * 1e-3)})
        row["gemm_over_kernel"] = t["gemm"][0] / t["kernel"][0]
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
        del Xl, E, out_k, out_g, Esq, out_sq
        torch.cuda.empty_cache()
    return rows


def qv_row(e, M, reps, parent):
    ms, all_ms, res = timed(lambda: e.qv_sample_masked(S, seed=1), reps, 1)
    row = {"qv_sample_masked_ms": ms, "qv_sample_masked_ms_all": all_ms, "ms_per_sample": ms / S, "finite": bool(torch.isfinite(res[0]).all().item())}
    if parent:
        def dense_route():
            mean = e.qv_masked()[0].reshape(-1).cpu()
            cov = e.qv_cov_masked().cpu()
            eps = e.normal_fill(1, 0, 0, S * M).reshape(S, M).cpu()
            return mean[None, :] + eps @ _symmetric_root(cov)
        p_ms, p_all, _ = timed(dense_route, 1 if M > 2048 else reps, 0)          # (a 4096 x 4096 eigh on the host: seconds)
        row.update(dense_covariance_route="qv_masked + qv_cov_masked (device) -> host, symmetric root by eigh, one [64, M] x [M, M] product "
                                          "(models._dense_sampler, the route of dense_samples=False)",
                   dense_covariance_route_ms=p_ms, dense_covariance_route_ms_all=p_all, dense_route_over_qv_sample_masked=p_ms / ms)
    else:
        row["dense_covariance_route_ms"] = "refuses: models._dense_sampler stops at M = 4096"
    print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
    return row


def map_rows(e, sizes, reps):
    rows = []
    for P in sizes:
        g1, g2 = axes(P, e.device)
        ms, all_ms, res = timed(lambda: e.posterior_raster_sample_masked(g1, g2, S, seed=1), reps, 1)
        r_ms, r_all, _ = roots_ms(e, "matern12", g1, g2, bench.THETA0[:2], reps)
        row = {"raster": f"{P} x {P}", "samples": S, "ms_per_call": ms, "ms_per_call_all": all_ms, "ms_per_sample": ms / S, "roots_ms": r_ms,
               "roots_ms_all": r_all, "root_jitter_levels": list(res[1]["jitter"]), "finite": bool(torch.isfinite(res[0]).all().item())}
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
        del res
        torch.cuda.empty_cache()
    return rows


def scattered_state(e, reps):
    N, m = 100_000, 32
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (N, 2))
    y = D.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(N)
    mesh = np.linspace(0, 1, m + 1)
    e.plan("matern12", "b0", mesh, X[:, 0].copy(), "matern12", "b0", mesh, X[:, 1].copy(), scattered=True)
    _, _, info = e.elbo_step_scattered(torch.tensor(y, device=e.device), float(y @ y), bench.THETA0)
    assert info["status"] == 0
    return {"state": f"{N} uniform points, matern12, b0, m_d = {m} (M = {m * m}), one vggp_elbo_step_scattered at bench.py's THETA0",
            "q_v": qv_row(e, m * m, reps, True), "maps": map_rows(e, (256, 1024), reps)}


def masked_state(e, m, reps, parent, maps):
    n = 2048
    _, y, x1, x2 = D.gen_grid(n, n)
    W = (np.random.default_rng(1).uniform(size=(n, n)) > 0.3).astype(np.float64)
    mesh = np.linspace(0, 1, m + 1)
    e.plan("matern12", "b0", mesh, x1, "matern12", "b0", mesh, x2)
    Wd = torch.tensor(W, device=e.device)
    Ym = torch.tensor(y.reshape(n, n), device=e.device) * Wd
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, _, info = e.elbo_step_masked(Ym, Wd, float(W.sum()), e.sumsq(Ym), bench.THETA0)
    torch.cuda.synchronize()
    assert info["status"] == 0
    row = {"state": f"{n} x {n} grid, 30 % missing, matern12, b0, m_d = {m} (M = {m * m}), one vggp_elbo_step_masked at bench.py's THETA0",
           "step_s_first_call": time.perf_counter() - t0, "q_v": qv_row(e, m * m, reps, parent)}
    if maps:
        row["maps"] = map_rows(e, (256, 1024), reps)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="kernel,scattered,masked64,masked128")
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_sample_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dense_sample needs the GPU: nothing is timed without one")
    torch.cuda.set_device(0)
    e = Engine(0)
    res = {"device": torch.cuda.get_device_name(0), "theta": list(bench.THETA0), "samples_per_call": S, "noise": "generated on the device (seed 1)",
           "fp64_mfma_peak_tflops": PEAK_FP64_MFMA / 1e12, "factor_builder_rate_TBps": FACTOR_BUILDER_RATE / 1e12,
           "hbm_achievable_TBps": HBM_ACHIEVABLE / 1e12, "measured": True,
           "method": "kernel rows: HIP events around a window of back-to-back asynchronous calls (>= 20 ms or 1 call) divided by the count, "
                     "the routes alternating inside one loop in one process on the same operands, median of reps windows after warm windows; "
                     "entries: host clock around one host-synchronous call between device synchronisations, median of reps calls after one "
                     "warm-up; every repeat is in *_ms_all; roots_ms: the three Cholesky roots of a call timed on their own"}
    only = a.only.split(",")
    if "kernel" in only:
        res["kernel"] = kernel_rows(e, [int(s) for s in a.sizes.split(",")], a.reps, a.warm)
    if "scattered" in only:
        res["scattered_M1024"] = scattered_state(e, min(a.reps, 5))
    if "masked64" in only:
        res["masked_M4096"] = masked_state(e, 64, min(a.reps, 5), True, True)
    if "masked128" in only:
        res["masked_M16384"] = masked_state(e, 128, min(a.reps, 5), False, False)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
