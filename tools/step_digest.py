"""Bitwise fingerprint of the full-grid ELBO step: every chain of the step's state machine, step by step.

Drives each trajectory of tests/test_gpu_readout_states.py (STATES: cold, polish / refine, extrapolated with rounds, thin, jump ->
cold retry, cold-thin, Newton at m = 192, Newton on B1, split-API subspace, split-API polish) and one mixed-kernel case of
tests/mixed_dims_cases.py to its last step and prints, per step, a SHA-256 over the ELBO, the gradient, the step's diagnostics
(everything vggp_info carries: jitter, sweeps, rounds, status, polished -- it has no numerical ranks, so none are hashed) and the
return code; after the last step of a trajectory a SHA-256 over the outputs of vggp_qv, vggp_posterior and vggp_zgrad.  No step of
these trajectories is expected to fail: the first error ends the process with a non-zero status, and nothing more is started on
the GPU (with --all: no further configuration either).  With --profile the steps run with vggp_profile on, and each trajectory also lists the
stages of vggp_profile_read that were charged time.  Two builds that print the same lines compute the same bits.  --brief folds
the step lines of a trajectory into one line (their count and a SHA-256 over them): the form kept in profiles/step_digest.txt,
which is a tenth of the size.  A mismatch against that file names the trajectory; the run without --brief then names the step.

    python tools/step_digest.py                      # one configuration: the environment as it is
    python tools/step_digest.py --all                # every configuration of CONFIGS, a fresh child process each
    python tools/step_digest.py --all --brief --out profiles/step_digest.txt
    python tools/step_digest.py --lib other/libvggp_hip.so ...      # fingerprint another build of the library
"""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

# name -> (environment, extra arguments): the switches that select another launch sequence for the same numbers
CONFIGS = {
    "default": ({}, []),
    "no_graph": ({"VGGP_NO_GRAPH": "1"}, []),
    "no_ride": ({"VGGP_NO_RIDE": "1"}, []),
    "no_early": ({"VGGP_NO_EARLY": "1"}, []),
    "no_early_reg": ({"VGGP_NO_EARLY_REG": "1"}, []),
    "no_thin": ({"VGGP_NO_THIN": "1"}, []),
    "no_newton_chain": ({"VGGP_NO_NEWTON_CHAIN": "1"}, []),
    "no_refine": ({"VGGP_NO_REFINE": "1"}, []),
    "sub_extrap": ({"VGGP_SUB_EXTRAP": "1"}, []),
    "chol_legacy": ({"VGGP_CHOL_LEGACY": "1"}, []),
    "profile": ({}, ["--profile"]),
}
CHILD_TIMEOUT_S = 240
MIXED = "rbf_pts11-m12_vff9"
MIXED_STEPS = 8


def _sha(*parts) -> str:
    import numpy as np
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(np.asarray(p, dtype=np.float64)).tobytes())
    return h.hexdigest()


def _step_line(tag, k, call):
    """One step -> its digest line; a failed step prints its return code and raises (main ends the process)."""
    from variational_gridded_gaussian_processes_amd import VggpError
    try:
        elbo, grad, info = call()
    except VggpError as e:
        print(f"{tag} step {k} rc {e.code} -", flush=True)
        raise
    diag = [*info["jitter"], *info["sweeps"], *info["rounds"], info["status"], *[float(b) for b in info["polished"]]]
    return f"{tag} step {k} rc 0 {_sha([elbo], grad, diag)} elbo {elbo!r} rounds {info['rounds']} polished {info['polished']}"


def _readouts_line(tag, engine, Y, xs):
    mean, var = engine.qv()
    pm, pv = engine.posterior(xs)
    g1, g2 = engine.zgrad(Y)
    return f"{tag} readouts {_sha(*[t.cpu().numpy() for t in (mean, var, pm, pv, g1, g2)])}"


def _stages_line(tag, engine):
    ms, steps = engine.profile_read(reset=True)
    return f"{tag} stages {[i for i, v in enumerate(ms.values()) if v != 0.0]} steps {steps}"


def run(tag: str, profile: bool, only) -> int:
    import numpy as np
    import torch
    import mixed_dims_cases as MC
    from test_gpu_readout_states import STATES, XS, _Plan
    from variational_gridded_gaussian_processes_amd import Engine

    engine = Engine(0)
    if profile:
        engine.profile(True)
    xs = torch.tensor(XS, device="cuda")
    for name, S in STATES.items():
        if only and name not in only:
            continue
        t = f"{tag} {name}"
        p = _Plan(engine, S)
        if profile:
            engine.profile_read(reset=True)
        for k in range(S["last"] + 1):
            print(_step_line(t, k, lambda: p.step(S["path"](k))), flush=True)
        if profile:
            print(_stages_line(t, engine), flush=True)
        print(_readouts_line(t, engine, p.Y, xs), flush=True)
    if not only or MIXED in only:
        t = f"{tag} {MIXED}"
        d1, d2, n, theta = MC.FULL[MIXED]
        d1, d2, x1, x2, Yn, _, _, theta = MC.grid_problem(d1, d2, n, theta)
        engine.plan(*MC.plan_args(d1, x1, d2, x2), warm_start=True)
        Y = torch.tensor(Yn, device="cuda")
        yy = engine.sumsq(Y)
        if profile:
            engine.profile_read(reset=True)
        for k in range(MIXED_STEPS):
            print(_step_line(t, k, lambda: engine.elbo_step(Y, yy, np.asarray(theta) * (1 + 0.01 * k))), flush=True)
        if profile:
            print(_stages_line(t, engine), flush=True)
        print(_readouts_line(t, engine, Y, xs), flush=True)
    engine.close()
    return 0


def _brief(text: str) -> str:
    """The step lines of each trajectory folded into one: '<config> <trajectory> steps <count> <SHA-256 over those lines>'."""
    out, run, key = [], [], None

    def close():
        if run:
            out.append(f"{key} steps {len(run)} {hashlib.sha256(chr(10).join(run).encode()).hexdigest()}")
            run.clear()
    for line in text.splitlines():
        w = line.split()
        if len(w) > 3 and w[2] == "step":
            if key != f"{w[0]} {w[1]}":
                close()
                key = f"{w[0]} {w[1]}"
            run.append(line)
        else:
            close()
            out.append(line)
    close()
    return "".join(l + "\n" for l in out)


def run_all(args) -> int:
    """Every configuration in a fresh child process, one after another; the first failure stops the rest."""
    out = open(args.out, "w") if args.out else None
    if out and args.brief:
        out.write("# tools/step_digest.py --all --brief: per trajectory, the number of step lines and a SHA-256 over them "
                  "(the per-step lines: the same command without --brief)\n")
    for name, (env, extra) in CONFIGS.items():
        if args.configs and name not in args.configs:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--tag", name, *extra]
        if args.lib:
            cmd += ["--lib", args.lib]
        if args.only:
            cmd += ["--only", *args.only]
        try:
            r = subprocess.run(cmd, env={**os.environ, **env}, stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result after {CHILD_TIMEOUT_S} s; stopping", file=sys.stderr)
            return 124
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if out:
            out.write(_brief(r.stdout) if args.brief else r.stdout)
            out.flush()
        if r.returncode:
            print(f"{name}: exit status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--all", action="store_true", help="run every configuration of CONFIGS, each in a child process of its own")
    ap.add_argument("--configs", nargs="*", default=None, help="with --all: only these configurations")
    ap.add_argument("--out", default=None, help="with --all: also write the lines to this file")
    ap.add_argument("--brief", action="store_true", help="with --out: one line per trajectory instead of one per step")
    ap.add_argument("--lib", default=None, help="fingerprint this build of libvggp_hip.so instead of the in-tree one")
    ap.add_argument("--tag", default="env", help="first word of every line")
    ap.add_argument("--profile", action="store_true", help="run with vggp_profile on and list the stages that were charged time")
    ap.add_argument("--only", nargs="*", default=None, help="only these trajectories")
    args = ap.parse_args()
    if args.all:
        return run_all(args)
    if args.lib:
        from variational_gridded_gaussian_processes_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from variational_gridded_gaussian_processes_amd import VggpError
    try:
        return run(args.tag, args.profile, args.only)
    except VggpError as e:      # any library error: nothing more on the GPU, not even the context's teardown
        print(f"{args.tag}: {e}; stopping", file=sys.stderr, flush=True)
        os._exit(1)


if __name__ == "__main__":
    sys.exit(main())
