"""ms per step of the dense scattered step (vggp_elbo_step_scattered) and the iterative one (vggp_elbo_step_scattered_iter) at
N = 100 000 uniform points, B0 / Matern-1/2; HIP events, median of 10 after 3 warm-ups.  Also the achieved TF/s of the two Khatri-Rao
kernels beside vggp_gemm on a product of the same dimensions ((m1 nb) x N x m2 for field, (m1) x (nb m2) x N for back; 2 m1 m2 N nb
FLOP each).  Writes profiles/scattered_iter_times.json.

    python tools/time_scattered_iter.py [--n 100000] [--sizes 32,64,128,192,256] [--out profiles/scattered_iter_times.json]
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
from variational_gridded_gaussian_processes_amd._lib import VggpError

THETA = [0.1, 0.12, 0.7, 0.9, 0.01]
NB = 17


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
    ap.add_argument("--sizes", default="32,64,128,192,256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scattered_iter_times.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    e = Engine(0)
    rng = np.random.default_rng(0)
    X = rng.random((a.n, 2))
    y = datagen.latent_2d(X[:, 0], X[:, 1]) + 0.05 * rng.standard_normal(a.n)
    yd = torch.tensor(y, dtype=torch.float64, device="cuda")
    yy = float(y @ y)
    res = {"N": a.n, "theta": THETA, "n_probes": 16, "steps": [], "kernels": []}
    for m in [int(s) for s in a.sizes.split(",")]:
        g = np.linspace(0.0, 1.0, m + 1)
        e.plan("matern12", "b0", g, X[:, 0], "matern12", "b0", g, X[:, 1], scattered=True)
        row = {"m_d": m, "M": m * m}
        info = {}

        def it_step():
            info.update(e.elbo_step_scattered_iter(yd, yy, THETA)[2])
        row["iter_ms"] = timed(it_step)
        row["pcg_iterations"] = info["rounds"][0]
        row["dense_ms"] = None
        if m <= 128:
            need = 8.0 * (10.0 * m ** 4 + 4.0 * m * m * a.n)
            if need < 0.8 * torch.cuda.mem_get_info()[0] and m * m * a.n < 2 ** 31:
                try:
                    row["dense_ms"] = timed(lambda: e.elbo_step_scattered(yd, yy, THETA), reps=10 if m <= 64 else 3, warm=1)
                except VggpError as ex:
                    row["dense_error"] = str(ex)
            else:
                row["dense_error"] = f"workspace of about {need / 2 ** 30:.0f} GiB (or m^2 N >= 2^31) does not fit"
        print(json.dumps(row), flush=True)
        res["steps"].append(row)
        # the two kernels alone, beside vggp_gemm on a product of the same dimensions
        L = torch.randn(m, a.n, dtype=torch.float64, device="cuda")
        R = torch.randn(m, a.n, dtype=torch.float64, device="cuda")
        V = torch.randn(m, NB, m, dtype=torch.float64, device="cuda")
        F = torch.randn(NB, a.n, dtype=torch.float64, device="cuda")
        fl = 2.0 * m * m * a.n * NB
        k = {"m_d": m, "nb": NB, "flop": fl}
        k["field_tfs"] = fl / (timed(lambda: e.kr_field(L, R, V)) * 1e-3) / 1e12
        k["back_tfs"] = fl / (timed(lambda: e.kr_back(L, R, F)) * 1e-3) / 1e12
        Vm = V.reshape(m * NB, m)
        k["gemm_field_shape_tfs"] = fl / (timed(lambda: e.gemm(Vm, R)) * 1e-3) / 1e12                    # (m1 nb) x N x m2
        Bt = torch.randn(a.n, NB * m, dtype=torch.float64, device="cuda")
        k["gemm_back_shape_tfs"] = fl / (timed(lambda: e.gemm(L, Bt)) * 1e-3) / 1e12                     # m1 x (nb m2) x N
        del Bt
        print(json.dumps(k), flush=True)
        res["kernels"].append(k)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
