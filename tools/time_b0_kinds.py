"""Cost of the B0K families (profiles/b0_kinds_times.json): the factor launch at 8192^2 (device events around the launch into preallocated outputs) and the warm / cold
step of the 1024^2 flagship shape at 128 cells per dimension, Matern-1/2 (b0), -3/2 and -5/2 (b0k) in one session; then
Matern-5/2 and -3/2 at 256 x 256, 128 cells against the structured oracle.   python tools/time_b0_kinds.py [out.json]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
from oracle import dense as D
from variational_gridded_gaussian_processes_amd import Engine
from variational_gridded_gaussian_processes_amd._lib import BASIS, KIND
import bench
out = {"factor_8192": {}, "step_1024_m128": {}}
eng = Engine(0)
m = n = 8192
x = torch.linspace(-0.05, 1.05, n, dtype=torch.float64, device="cuda")
g = torch.linspace(0, 1, m + 1, dtype=torch.float64, device="cuda")
bufs = [torch.empty(m, n, dtype=torch.float64, device="cuda") for _ in range(4)]
st = torch.cuda.current_stream().cuda_stream
for kind, basis in (("matern12", "b0"), ("matern32", "b0k"), ("matern52", "b0k"), ("matern32", "points")):
    gg = g if basis != "points" else g[:m].contiguous()
    def go():
        rc = eng.lib.vggp_factor_build(eng._h, KIND[kind], BASIS[basis], x.data_ptr(), n, gg.data_ptr(), m, 0.2, 0, *[b.data_ptr() for b in bufs], st)
        assert rc == 0
    for _ in range(3): go()
    ts = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); go(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b) * 1e-3)
    byt = 32.0 * m * n
    out["factor_8192"][f"{kind}-{basis}"] = {"us_median": float(np.median(ts) * 1e6), "us_min": float(min(ts) * 1e6), "TB_per_s_median": byt / float(np.median(ts)) / 1e12}
    print(kind, basis, out["factor_8192"][f"{kind}-{basis}"], flush=True)
del bufs
n, cells = 1024, 128
X, y, x1, x2 = D.gen_grid(n, n); del X
Y = torch.tensor(y.reshape(n, n), device="cuda"); yy = eng.sumsq(Y)
mesh = np.linspace(0, 1, cells + 1)
for kind, basis in (("matern12", "b0"), ("matern32", "b0k"), ("matern52", "b0k")):
    for warm in (True, False):
        eng.plan(kind, basis, mesh, x1, kind, basis, mesh, x2, warm_start=warm)
        opt = bench.FitLoop5(bench.raw_start(), lr=0.01)
        def one():
            e, gr, info = eng.elbo_step(Y, yy, opt.theta()); opt.update(gr); return e, info
        for _ in range(30): e, info = one()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        steps = 200 if warm else 60
        infos = []
        for _ in range(steps):
            e, info = one(); infos.append(info)
        torch.cuda.synchronize(); ms = (time.perf_counter() - t0) / steps * 1e3
        r = {"ms_per_step": ms, "last_sweeps": infos[-1]["sweeps"], "last_rounds": infos[-1]["rounds"], "polished_last": infos[-1]["polished"],
             "max_sweeps": [max(i["sweeps"][0] for i in infos), max(i["sweeps"][1] for i in infos)], "jitter": infos[-1]["jitter"],
             "status_all_ok": all(i["status"] == 0 for i in infos), "elbo_last": e}
        out["step_1024_m128"][f"{kind}-{basis}-{'warm' if warm else 'cold'}"] = r
        print(kind, basis, "warm" if warm else "cold", r, flush=True)
# Matern-5/2 at 256 x 256, 128 cells: jitter level and agreement with the structured oracle (by hand, not asserted)
import b0_kinds_spec as B
from oracle import kron as Kr
n = 256
X, y, x1, x2 = D.gen_grid(n, n)
theta = [0.2, 0.2, 1.0, 1.0, 0.0025]
res = {}
for kind in ("matern52", "matern32"):
    f1, f2 = B.factor(kind, mesh, x1), B.factor(kind, mesh, x2)
    ref = Kr.elbo_step(y.reshape(n, n), f1, f2, theta)
    eng.plan(kind, "b0k", mesh, x1, kind, "b0k", mesh, x2)
    Yd = torch.tensor(y.reshape(n, n), device="cuda")
    elbo, grad, info = eng.elbo_step(Yd, eng.sumsq(Yd), theta)
    mean, var = eng.qv(); rm, rv = Kr.q_v(ref)
    rel = lambda a, b: float(np.abs(np.asarray(a) - b).max() / np.abs(b).max())
    res[kind] = {"jitter_gpu": info["jitter"], "jitter_oracle": [ref.d1.jit, ref.d2.jit], "status": info["status"], "sweeps": info["sweeps"],
                 "elbo_rel": abs(elbo - ref.elbo) / abs(ref.elbo), "grad_rel": rel(grad, ref.grad), "qv_mean_rel": rel(mean.cpu().numpy(), rm),
                 "qv_var_rel": rel(var.cpu().numpy(), rv)}
    print(kind, "256x256 m128", res[kind], flush=True)
out["size_256_m128"] = res
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1, default=lambda o: list(o) if isinstance(o, tuple) else str(o))
