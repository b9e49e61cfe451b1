"""Host-side pieces of bench.py that run without a GPU: the plain-float fit loop of the headline equals the numpy Adam it replaced,
the self-launch refuses a world-size mismatch before anything touches a device, and the argument parser keeps the driver's contract."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_fitloop5_equals_numpy_adam():
    rng = np.random.default_rng(0)
    a = bench.Adam(bench.raw_start(), lr=0.01)
    b = bench.FitLoop5(bench.raw_start(), lr=0.01)
    for _ in range(50):
        raw = a.x
        th_a = bench.theta_from_raw(raw.copy())
        th_b = np.array(b.theta())
        assert np.allclose(th_a, th_b, rtol=1e-14, atol=0)
        g = rng.standard_normal(5) * np.array([1e4, 1e4, 1e3, 1e3, 1e6])          # d ELBO / d theta
        a.step(-(g / (1.0 + np.exp(-raw))))                                      # minimise -ELBO through the softplus
        b.update(g)
    assert np.allclose(a.x, np.array(b.x), rtol=1e-12, atol=0)


def test_world_size_mismatch_is_exit_code_2():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2, (p.returncode, p.stderr[-400:])


def test_algorithmic_flops_of_the_headline_shape():
    f = bench.algorithmic_flops(1024, 1024, 128, 128)
    total = sum(v for v in f.values() if isinstance(v, (int, float)))
    assert 0.8e9 < total < 1.1e9          # DESIGN / VERDICT: 0.927 GFLOP per step at 1024 x 1024, m_d = 128


def test_plain_run_is_the_default_and_steps_must_be_positive():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        try:
            bench.parse_args(bad)
        except SystemExit as e:
            assert e.code == 2
        else:
            raise AssertionError(f"{bad} was accepted")


def test_dump_outputs_writes_float64_npy(tmp_path):
    d = tmp_path / "outs"
    bench.dump_outputs(str(d), {"elbo": -891.5, "grad": np.arange(5.0), "theta": [0.2, 0.2, 1.0, 1.0, 0.0026]})
    assert sorted(p.name for p in d.iterdir()) == ["elbo.npy", "grad.npy", "theta.npy"]
    e = np.load(d / "elbo.npy")
    assert e.dtype == np.float64 and e.shape == (1,) and e[0] == -891.5
    assert np.array_equal(np.load(d / "grad.npy"), np.arange(5.0))
    assert np.load(d / "theta.npy").dtype == np.float64
