"""ms of posterior(x*) on a raster: Engine.posterior_raster (vggp_posterior_raster, one factor column per AXIS coordinate and one
two-sided fp64-MFMA product) against the unchanged point-wise entry at the same cartesian points, rasters 256^2, 1024^2 and 4096^2.

    headline   1024 x 1024 grid, RBF, m_d = 128 inducing points (bench.py's flagship plan, THETA0), one cold step: mean and variance
               against vggp_posterior.  A cold RBF step at this size ends in the thin chain, so both read-outs contract its range
               directions only (q_d ~ 20, not 128).
    full_rank  the same grid and m_d with Matern-3/2 kernels: every direction kept, q_d = 128 -- the case the operation counts
               O(P1 P2 q1) against O(P1 P2 q1 q2) are about
    scattered  100 000 uniform points, B0 Matern-1/2 cells, m_d = 128, one vggp_elbo_step_scattered_iter: the mean-only route against
               vggp_posterior_scattered_iter
Beside the times of the headline and full-rank states: the error of both routes against oracle/kron.py's posterior() at the 256^2
raster (the pair tests/test_gpu_posterior_raster.py asserts on small problems), and the largest difference between the two routes at
every size.  A record, not a gate; the acceptance condition read from it is raster_ms <= pointwise_ms at every size.

Method: host clock around a window of calls between device synchronisations (a call includes the entry's own launches, factor build
and GEMMs, not only the last kernel); a window holds as many calls as last 250 ms or more (counted from the last warm-up round, at most
20000) and is divided by that count; the two routes alternate inside one loop, `warm` untimed rounds first (the first call allocates the
workspace), median of `reps` windows.  Writes profiles/posterior_raster_times.json.

    python tools/bench_posterior_raster.py [--only headline,full_rank,scattered] [--sizes 256,1024,4096] [--out FILE]
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
from oracle import kron as Kr
from variational_gridded_gaussian_processes_amd import Engine, datagen as D

REPS = {256: (7, 3), 1024: (7, 2), 4096: (5, 1)}            # raster side -> (timed windows, warm-up rounds)
WINDOW_MS = 250.0


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def axes(P, device):
    """Two different irregular axes of P coordinates inside the data range."""
    rng = np.random.default_rng(P)
    g1, g2 = np.sort(rng.uniform(0, 1, P)), np.sort(rng.uniform(0, 1, P))
    return torch.tensor(g1, device=device), torch.tensor(g2, device=device)


def alternate(raster, pointwise, reps, warm):
    """-> (median ms, all ms) of each route, the routes alternating inside one loop, and their last results"""
    ms = {"raster": [], "pointwise": []}
    inner = {"raster": 1, "pointwise": 1}       # calls per timed window, set from the last warm-up round so that a window lasts >= WINDOW_MS
    out = {}
    for it in range(warm + reps):
        for name, fn in (("raster", raster), ("pointwise", pointwise)):
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


def time_sizes(e, sizes, want_var, pointwise_entry):
    rows = []
    for P in sizes:
        g1, g2 = axes(P, e.device)
        xs = torch.cartesian_prod(g1, g2)                    # point a * P + b = (g1[a], g2[b])
        reps, warm = REPS.get(P, (5, 1))
        t, out = alternate(lambda: e.posterior_raster(g1, g2, want_var=want_var), lambda: pointwise_entry(xs), reps, warm)
        rm, rv = out["raster"]
        pw = out["pointwise"]
        pm, pv = pw if isinstance(pw, tuple) else (pw, None)
        row = {"raster": f"{P} x {P}", "points": P * P, "reps_after_warmups": [reps, warm],
               "calls_per_timed_window": {"raster": t["raster"][2], "pointwise": t["pointwise"][2]},
               "raster_ms": t["raster"][0], "raster_ms_min_max": [min(t["raster"][1]), max(t["raster"][1])], "raster_ms_all": t["raster"][1],
               "pointwise_ms": t["pointwise"][0], "pointwise_ms_min_max": [min(t["pointwise"][1]), max(t["pointwise"][1])],
               "pointwise_ms_all": t["pointwise"][1],
               "pointwise_over_raster": t["pointwise"][0] / t["raster"][0],
               "mean_raster_vs_pointwise": rel(rm.reshape(-1), pm)}
        if want_var:
            row["var_raster_vs_pointwise"] = rel(rv.reshape(-1), pv)
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
        del xs, out, rm, rv, pm, pv, pw
        torch.cuda.empty_cache()
    return rows


def grid_state(e, kind, sizes):
    n, m = 1024, 128
    _, y, x1, x2 = D.gen_grid(n, n)
    g = np.linspace(0, 1, m)
    e.plan(kind, "points", g, x1, kind, "points", g, x2)
    Y = torch.tensor(y.reshape(n, n), device=e.device)
    elbo, grad, info = e.elbo_step(Y, e.sumsq(Y), bench.THETA0)
    row = {"state": f"{n} x {n} grid, {kind}, points, m_d = {m}, one cold vggp_elbo_step at bench.py's THETA0",
           "pointwise_entry": "vggp_posterior", "outputs": "mean and variance", "step_rounds": list(info["rounds"])}
    if 256 in sizes:                                         # the error pair against the oracle, at the smallest raster
        g1, g2 = axes(256, e.device)
        xs = torch.cartesian_prod(g1, g2)
        f1, f2 = Kr.Factor("points", kind, g, x1), Kr.Factor("points", kind, g, x2)
        st = Kr.elbo_step(y.reshape(n, n), f1, f2, bench.THETA0)
        om, ov = (torch.tensor(a) for a in Kr.posterior(st, f1, f2, xs.cpu().numpy()))
        rm, rv = (t.reshape(-1).cpu() for t in e.posterior_raster(g1, g2))
        pm, pv = (t.cpu() for t in e.posterior(xs))
        row["errors_vs_oracle_at_256x256"] = {"raster_mean": rel(rm, om), "pointwise_mean": rel(pm, om),
                                              "raster_var": rel(rv, ov), "pointwise_var": rel(pv, ov)}
        print(json.dumps(row["errors_vs_oracle_at_256x256"]), flush=True)
    row["sizes"] = time_sizes(e, sizes, True, e.posterior)
    return row


def scattered_state(e, sizes):
    N, m = 100_000, 128
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (N, 2))
    y = D.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(N)
    mesh = np.linspace(0, 1, m + 1)
    e.plan("matern12", "b0", mesh, X[:, 0].copy(), "matern12", "b0", mesh, X[:, 1].copy(), scattered=True)
    yd = torch.tensor(y, device=e.device)
    elbo, grad, info = e.elbo_step_scattered_iter(yd, float(y @ y), bench.THETA0)
    row = {"state": f"{N} uniform points, matern12, b0, m_d = {m}, one vggp_elbo_step_scattered_iter at bench.py's THETA0",
           "pointwise_entry": "vggp_posterior_scattered_iter", "outputs": "mean only", "step_pcg_iterations": info["rounds"][0]}
    row["sizes"] = time_sizes(e, sizes, False, e.posterior_scattered_iter)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="headline,full_rank,scattered")
    ap.add_argument("--sizes", default="256,1024,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_raster_times.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_posterior_raster needs the GPU: nothing is timed without one")
    sizes = [int(s) for s in args.sizes.split(",")]
    e = Engine(0)
    res = {"device": torch.cuda.get_device_name(0),
           "method": "host clock around windows of >= 250 ms of calls between device synchronisations, routes alternating, median of reps "
                     "windows after warm-ups; ms per whole call (factor build, GEMMs and the last kernel)"}
    only = args.only.split(",")
    if "headline" in only:
        res["headline"] = grid_state(e, "rbf", sizes)
    if "full_rank" in only:
        res["full_rank"] = grid_state(e, "matern32", sizes)
    if "scattered" in only:
        res["scattered"] = scattered_state(e, sizes)
    rows = [r for k in ("headline", "full_rank", "scattered") if k in res for r in res[k]["sizes"]]
    res["raster_not_slower_at_every_size"] = all(r["raster_ms"] <= r["pointwise_ms"] for r in rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
