"""Bitwise fingerprint of the M-space solvers: the dense and the iterative masked / scattered steps with every read-out.

One line per entry of include/vggp.h that lives in csrc/masked.hip, masked_readout.hip, iter_step.hip, iter_readout.hip (and the
vggp_kr_* building blocks of kr.hip, and vggp_readout of api.hip, which shares vg_whitened_cross with them): a SHA-256 over the raw
outputs, the return code and everything vggp_info carries.  The problems are the small ones of tests/masked_iter_spec.py (shape s70:
n = 70 x 45, m = 7 x 12), as a masked grid and as the scattered points of its masks; steps run three times with theta (1 + 0.01 k), so
that the iterative steps reach their kept-basis path.  No call is expected to fail: the first error ends the process with a non-zero
status and nothing more is started on the GPU.  Two builds that print the same lines compute the same bits
(profiles/mspace_digest.txt is the committed baseline).

    python tools/mspace_digest.py --out profiles/mspace_digest.txt
    python tools/mspace_digest.py --lib other/libvggp_hip.so ...      # fingerprint another build of the library
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from step_digest import _sha  # noqa: E402

STEPS = 3
DENSE_PAIRS = ("b0_m12", "vff", "pts_m32")
ITER_CASES = ("s70_b0_bern70_p16", "s70_pts32_track30_p1")
CELLS = (40, 3, 77, 12, 83, 5)          # six cells of the 7 x 12 q(v), unordered: with block = 4 the second block is ragged
GRID_CELLS = (17, 2, 29, 11, 0, 8)      # ... and of the 5 x 6 gridded read-out
_OUT = None


def _parts(out):
    """Flatten a call's result into arrays: tensors, numbers, None (skipped) and info dicts (every field)."""
    import torch
    if out is None:
        return []
    if isinstance(out, dict):
        return [[*out["jitter"], *out["sweeps"], *out["rounds"], out["status"], *[float(b) for b in out["polished"]]]]
    if isinstance(out, torch.Tensor):
        return [out.cpu().numpy()]
    if isinstance(out, (tuple, list)):
        return [p for o in out for p in _parts(o)]
    return [out]


def _line(tag, name, call):
    from variational_gridded_gaussian_processes_amd import VggpError
    try:
        out = call()
    except VggpError as e:
        _emit(f"{tag} {name} rc {e.code} -")
        raise
    _emit(f"{tag} {name} rc 0 {_sha(*_parts(out))}")


def _emit(line):
    print(line, flush=True)
    if _OUT:
        _OUT.write(line + "\n")
        _OUT.flush()


def _operands(dev, m1, m2):
    import numpy as np
    rng = np.random.default_rng(21)
    return dev(rng.standard_normal((5, m1))), dev(rng.standard_normal((6, m2))), dev(rng.uniform(0.5, 1.5, 5)), dev(rng.uniform(0.5, 1.5, 6))


def _points(x1, x2, Y, W):
    """The observed nodes of a mask as scattered points: X [N, 2], y [N]."""
    import numpy as np
    j, i = np.nonzero(W)
    return np.stack([x1[i], x2[j]], axis=1), Y[j, i]


def run(tag: str) -> int:
    import numpy as np
    import torch
    import masked_iter_spec as MS
    import mixed_dims_cases as MX
    from variational_gridded_gaussian_processes_amd import Engine

    def dev(a):
        return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")

    engine = Engine(0)
    xs = dev(np.random.default_rng(9).uniform(0, 1, (6, 2)))
    theta_k = lambda theta, k: np.asarray(theta) * (1 + 0.01 * k)

    def dense_readouts(t, ops):
        _line(tag, f"{t} qv_masked", engine.qv_masked)
        _line(tag, f"{t} posterior_masked", lambda: engine.posterior_masked(xs))
        _line(tag, f"{t} posterior_cov_masked", lambda: engine.posterior_cov(xs, masked=True))
        _line(tag, f"{t} qv_cov_masked", engine.qv_cov_masked)
        _line(tag, f"{t} readout_masked literal", lambda: engine.readout(*ops, literal=True, masked=True))
        _line(tag, f"{t} readout_masked conditional", lambda: engine.readout(*ops, literal=False, masked=True))

    # ---- dense masked and dense scattered ------------------------------------------------------------------------------------
    for pair in DENSE_PAIRS:
        d1, d2, _, _, x1, x2, Y, Wn = MS.problem("s70", pair, "bern70", 30)
        engine.plan(*MX.plan_args(d1, x1, d2, x2))
        ops = _operands(dev, engine.m1, engine.m2)
        W = dev(Wn)
        Ym = dev(Y) * W
        nobs, yy = float(Wn.sum()), engine.sumsq(Ym)
        t = f"dense_masked {pair}"
        for k in range(STEPS):
            _line(tag, f"{t} elbo_step_masked {k}", lambda: engine.elbo_step_masked(Ym, W, nobs, yy, theta_k(MS.THETA, k)))
        dense_readouts(t, ops)

        X, yn = _points(x1, x2, Y, MS.mask("track30", 70, 45, 1))
        X, yn = X[::6], yn[::6]                                        # a few hundred points
        engine.plan(*MX.plan_args(d1, X[:, 0], d2, X[:, 1]), scattered=True)
        y = dev(yn)
        yy = float(yn @ yn)
        t = f"dense_scattered {pair} N={len(yn)}"
        for k in range(STEPS):
            _line(tag, f"{t} elbo_step_scattered {k}", lambda: engine.elbo_step_scattered(y, yy, theta_k(MS.THETA, k)))
        _line(tag, f"{t} zgrad_scattered", lambda: engine.zgrad_scattered(y))
        dense_readouts(t, ops)

    # ---- iterative masked and iterative scattered ----------------------------------------------------------------------------
    for case in ITER_CASES:
        d1, d2, _, _, x1, x2, Y, Wn, nprobe, theta = MS.case_problem(case)
        engine.plan(*MX.plan_args(d1, x1, d2, x2))
        ops = _operands(dev, engine.m1, engine.m2)
        W = dev(Wn)
        Ym = dev(Y) * W
        nobs, yy = float(Wn.sum()), engine.sumsq(Ym)
        t = f"iter_masked {case}"
        for k in range(STEPS):
            _line(tag, f"{t} elbo_step_masked_iter {k}",
                  lambda: engine.elbo_step_masked_iter(Ym, W, nobs, yy, theta_k(theta, k), n_probes=nprobe))
        _line(tag, f"{t} qv_masked_iter all", lambda: engine.qv_masked_iter(W, nobs))
        _line(tag, f"{t} qv_masked_iter cells", lambda: engine.qv_masked_iter(W, nobs, cells=CELLS, block=4))
        _line(tag, f"{t} posterior_masked_iter", lambda: engine.posterior_masked_iter(xs, W, nobs, block=4))
        for literal in (True, False):
            _line(tag, f"{t} readout_masked_iter {'literal' if literal else 'conditional'}",
                  lambda: engine.readout_masked_iter(*ops, W, nobs, literal=literal, cells=GRID_CELLS, block=4))
        _line(tag, f"{t} qv_sample_masked_iter", lambda: engine.qv_sample_masked_iter(W, nobs, 5, seed=1, block=4))

        X, yn = _points(x1, x2, Y, Wn)
        engine.plan(*MX.plan_args(d1, X[:, 0], d2, X[:, 1]), scattered=True)
        y = dev(yn)
        yy = float(yn @ yn)
        t = f"iter_scattered {case} N={len(yn)}"
        for k in range(STEPS):
            _line(tag, f"{t} elbo_step_scattered_iter {k}",
                  lambda: engine.elbo_step_scattered_iter(y, yy, theta_k(theta, k), n_probes=nprobe))
        _line(tag, f"{t} qv_scattered_iter", engine.qv_scattered_iter)
        _line(tag, f"{t} posterior_scattered_iter", lambda: engine.posterior_scattered_iter(xs))
        _line(tag, f"{t} qv_var_scattered_iter all", engine.qv_var_scattered_iter)
        _line(tag, f"{t} qv_var_scattered_iter cells", lambda: engine.qv_var_scattered_iter(cells=CELLS, block=4))
        _line(tag, f"{t} posterior_var_scattered_iter", lambda: engine.posterior_var_scattered_iter(xs, block=4))
        for literal in (True, False):
            _line(tag, f"{t} readout_scattered_iter {'literal' if literal else 'conditional'}",
                  lambda: engine.readout_scattered_iter(*ops, literal=literal, cells=GRID_CELLS, block=4))
        _line(tag, f"{t} qv_sample_scattered_iter", lambda: engine.qv_sample_scattered_iter(5, seed=1, block=4))

    # ---- building blocks: m = 7 x 12, N = 300, nb = 5 ------------------------------------------------------------------------
    rng = np.random.default_rng(5)
    L, R, V, F = dev(rng.standard_normal((7, 300))), dev(rng.standard_normal((12, 300))), dev(rng.standard_normal((7, 5, 12))), \
        dev(rng.standard_normal((5, 300)))
    _line(tag, "blocks kr_field", lambda: engine.kr_field(L, R, V))
    _line(tag, "blocks kr_field2", lambda: engine.kr_field(L, R, V, cols_per_wg=2))
    _line(tag, "blocks kr_back", lambda: engine.kr_back(L, R, F))
    _line(tag, "blocks kr_sqgram", lambda: engine.kr_sqgram(L, R))

    # ---- the full-grid read-out (vg_whitened_cross in api.hip) ------------------------------------------------------------------
    d1, d2, _, _, x1, x2, Y, _ = MS.problem("s70", "b0_m12", "ones", 1)
    engine.plan(*MX.plan_args(d1, x1, d2, x2))
    ops = _operands(dev, engine.m1, engine.m2)
    Yd = dev(Y)
    yy = engine.sumsq(Yd)
    for k in range(STEPS):
        _line(tag, f"full_grid b0_m12 elbo_step {k}", lambda: engine.elbo_step(Yd, yy, theta_k(MS.THETA, k)))
    _line(tag, "full_grid b0_m12 readout literal", lambda: engine.readout(*ops, literal=True))
    _line(tag, "full_grid b0_m12 readout conditional", lambda: engine.readout(*ops, literal=False))
    engine.close()
    return 0


def main() -> int:
    global _OUT
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=None, help="fingerprint this build of libvggp_hip.so instead of the in-tree one")
    ap.add_argument("--tag", default="mspace", help="first word of every line")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if args.lib:
        from variational_gridded_gaussian_processes_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    if args.out:
        _OUT = open(args.out, "w")
    from variational_gridded_gaussian_processes_amd import VggpError
    try:
        return run(args.tag)
    except VggpError as e:      # any library error: nothing more on the GPU, not even the context's teardown
        print(f"{args.tag}: {e}; stopping", file=sys.stderr, flush=True)
        os._exit(1)


if __name__ == "__main__":
    sys.exit(main())
