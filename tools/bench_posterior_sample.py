"""ms of joint samples of posterior(x*) on a raster: Engine.posterior_raster_sample* (vggp_posterior_raster_sample*, generated noise),
64 samples of a 256^2 and a 1024^2 raster.

    headline   1024 x 1024 grid, RBF, m_d = 128 inducing points (bench.py's flagship plan, THETA0), one cold vggp_elbo_step
    masked     2048 x 2048 grid with 30 % of the nodes missing, B0 Matern-1/2 cells, m_d = 128, one vggp_elbo_step_masked_iter
Per state and raster: ms per call and per sample; the time of the three per-axis roots measured separately (the same machinery on
matrices of the same size and kind: vggp_factor_build's point kernel on the axis plus the nugget, vggp_cholesky_inverse three times);
the share of the fp64-MFMA bound, per-sample flops 2 m1 m2 p2 + 2 m1 p2^2 + p1 p2^2 + 2 m1 p1 p2 + p1^2 p2 against 78.6 TFLOP/s.
Beside them, at a 90 x 90 raster (8100 points, under the 8192 of vggp_posterior_cov), the only route there was before:
posterior(cartesian_prod).covariance_matrix plus a symmetric root on the host and one matrix product for the 64 samples.
A record, not a gate: no threshold is set.

Method: host clock around one host-synchronous call between device synchronisations; `warm` untimed calls first (the first call
allocates the workspace), median of `reps` calls; every repeat is kept in *_ms_all.  Writes profiles/posterior_sample_times.json.

    python tools/bench_posterior_sample.py [--only headline,masked,dense90] [--sizes 256,1024] [--out FILE]
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

PEAK_TFLOPS = 78.6          # fp64 MFMA
S = 64
ETA = 1e-8


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


def axes(P, device):
    """Two different irregular axes of P coordinates inside the data range."""
    rng = np.random.default_rng(P)
    g1, g2 = np.sort(rng.uniform(0, 1, P)), np.sort(rng.uniform(0, 1, P))
    return torch.tensor(g1, device=device), torch.tensor(g2, device=device)


def flops_per_sample(m1, m2, p1, p2):
    return 2 * m1 * m2 * p2 + 2 * m1 * p2 ** 2 + p1 * p2 ** 2 + 2 * m1 * p1 * p2 + p1 ** 2 * p2


def roots_ms(e, kind, g1, g2, ell, reps):
    """The three roots of a call on their own: k_d + eta I by the factor build, vggp_cholesky_inverse on k_1, k_2, k_2."""
    x0 = torch.zeros(1, dtype=torch.float64, device=e.device)
    K1 = e.factor_build(kind, "points", x0, g1, ell[0])[2]
    K2 = e.factor_build(kind, "points", x0, g2, ell[1])[2]
    K1.diagonal().add_(ETA)
    K2.diagonal().add_(ETA)

    def run():
        return [e.cholesky_inverse(K)[2] for K in (K1, K2, K2)]
    ms, all_ms, levels = timed(run, reps, 1)
    return ms, all_ms, levels


def sample_rows(e, kind, m, sizes, call, reps):
    rows = []
    for P in sizes:
        g1, g2 = axes(P, e.device)
        row = {"raster": f"{P} x {P}", "samples": S}
        try:
            ms, all_ms, res = timed(lambda: call(g1, g2), reps, 1)
        except Exception as err:                 # (recorded, not hidden: e.g. VGGP_ENOTPD of a root)
            row["error"] = str(err)
            rows.append(row)
            print(json.dumps(row), flush=True)
            continue
        out, info = res
        fl = flops_per_sample(m, m, P, P)
        r_ms, r_all, _ = roots_ms(e, kind, g1, g2, bench.THETA0[:2], reps)
        row.update(ms_per_call=ms, ms_per_call_all=all_ms, ms_per_sample=ms / S, roots_ms=r_ms, roots_ms_all=r_all,
                   root_jitter_levels=list(info["jitter"]), flops_per_sample=fl,
                   mfma_bound_ms_per_call=S * fl / (PEAK_TFLOPS * 1e9),
                   share_of_mfma_bound=S * fl / (PEAK_TFLOPS * 1e9) / ms,
                   share_of_mfma_bound_without_roots=S * fl / (PEAK_TFLOPS * 1e9) / max(ms - r_ms, 1e-9),
                   finite=bool(torch.isfinite(out).all().item()))
        if info["sweeps"][0]:
            row.update(pcg_iterations=info["rounds"][0], block_solves=info["sweeps"][0])
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
        del out, res
        torch.cuda.empty_cache()
    return rows


def headline(e, sizes, reps):
    n, m = 1024, 128
    _, y, x1, x2 = D.gen_grid(n, n)
    g = np.linspace(0, 1, m)
    e.plan("rbf", "points", g, x1, "rbf", "points", g, x2)
    Y = torch.tensor(y.reshape(n, n), device=e.device)
    _, _, info = e.elbo_step(Y, e.sumsq(Y), bench.THETA0)
    row = {"state": f"{n} x {n} grid, rbf, points, m_d = {m}, one cold vggp_elbo_step at bench.py's THETA0", "step_rounds": list(info["rounds"])}
    row["sizes"] = sample_rows(e, "rbf", m, sizes, lambda g1, g2: e.posterior_raster_sample(g1, g2, S, seed=1), reps)
    return row


def masked(e, sizes, reps):
    n, m = 2048, 128
    _, y, x1, x2 = D.gen_grid(n, n)
    mesh = np.linspace(0, 1, m + 1)
    W = torch.tensor((np.random.default_rng(1).uniform(size=(n, n)) < 0.7).astype(np.float64), device=e.device)
    Ym = torch.tensor(y.reshape(n, n), device=e.device) * W
    nobs = float(W.sum().item())
    e.plan("matern12", "b0", mesh, x1, "matern12", "b0", mesh, x2)
    step = e.elbo_step_masked_iter(Ym, W, nobs, e.sumsq(Ym), bench.THETA0)[2]
    row = {"state": f"masked {n} x {n} grid, 30 % missing, matern12, b0, m_d = {m}, one vggp_elbo_step_masked_iter at bench.py's THETA0",
           "step_pcg_iterations": step["rounds"][0]}
    row["sizes"] = sample_rows(e, "matern12", m, sizes, lambda g1, g2: e.posterior_raster_sample_masked_iter(g1, g2, W, nobs, S, seed=1), reps)
    return row


def dense90(e, reps):
    """The 90 x 90 raster both ways, on a state the dense route can serve (M ns <= 2^27: m_d = 64), Matern-3/2 points."""
    n, m, P = 256, 64, 90
    _, y, x1, x2 = D.gen_grid(n, n)
    g = np.linspace(0, 1, m)
    e.plan("matern32", "points", g, x1, "matern32", "points", g, x2)
    Y = torch.tensor(y.reshape(n, n), device=e.device)
    e.elbo_step(Y, e.sumsq(Y), bench.THETA0)
    g1, g2 = axes(P, e.device)
    xs = torch.cartesian_prod(g1, g2)

    def dense():
        cov = e.posterior_cov(xs).cpu()
        mean = e.posterior(xs)[0].cpu()
        w, V = torch.linalg.eigh(0.5 * (cov + cov.T))
        root = (V * w.clamp_min(0).sqrt()[None, :]) @ V.T
        return mean[None] + torch.randn(S, P * P, dtype=torch.float64) @ root
    d_ms, d_all, _ = timed(dense, 1, 0)              # (one 8100 x 8100 eigh on the host: tens of seconds)
    r_ms, r_all, res = timed(lambda: e.posterior_raster_sample(g1, g2, S, seed=1), reps, 1)
    return {"state": f"{n} x {n} grid, matern32, points, m_d = {m}, one cold vggp_elbo_step", "raster": f"{P} x {P}", "samples": S,
            "dense_route": "posterior_cov (device) -> host, symmetric root by eigh, one [64, 8100] x [8100, 8100] product",
            "dense_route_ms": d_ms, "dense_route_ms_all": d_all, "raster_sample_ms": r_ms, "raster_sample_ms_all": r_all,
            "dense_over_raster_sample": d_ms / r_ms, "root_jitter_levels": list(res[1]["jitter"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="headline,masked,dense90")
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_sample_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_posterior_sample needs the GPU: nothing is timed without one")
    torch.cuda.set_device(0)
    sizes = [int(s) for s in a.sizes.split(",")]
    e = Engine(0)
    res = {"device": torch.cuda.get_device_name(0), "theta": list(bench.THETA0), "samples_per_call": S, "noise": "generated on the device (seed 1)",
           "nugget": ETA, "fp64_mfma_peak_tflops": PEAK_TFLOPS, "measured": True,
           "method": "host clock around one host-synchronous call between device synchronisations; median of reps calls after one warm-up; "
                     "every repeat is in *_ms_all; roots_ms: the three Cholesky roots of a call timed on their own"}
    only = a.only.split(",")
    if "headline" in only:
        res["headline"] = headline(e, sizes, a.reps)
    if "masked" in only:
        res["masked"] = masked(e, sizes, a.reps)
    if "dense90" in only:
        res["dense_90x90"] = dense90(e, a.reps)
        print(json.dumps({k: v for k, v in res["dense_90x90"].items() if not k.endswith("_all")}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
