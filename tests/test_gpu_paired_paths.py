"""The paired inducing-point path (VGGP_FLAG_PAIRED_Z: csrc/paired.hip, csrc/gen_gemm.h) on every tile edge, kernel kind and read-out,
against the float64 specification tests/general_z_spec.py.  Cases, split replica, reference and bounds: tests/paired_cases.py (their
premises are checked on the CPU by tests/test_paired_cases.py).

Every case plans through Engine.plan_paired, steps, takes the Z-gradient, compares the data-dependent part of the ELBO (ELBO - C0),
the theta-gradient and the Z-gradient under bound(case, quantity) = max(100 x the reference's own floor, 1e-12) (never above the
path's ceilings 1e-7 / 1e-6 / 1e-6, read-outs 1e-7), then repeats the step and asserts the same bits and the specification's jitter.
    A  scattered step: MFMA fragment, tile, tile-pair / Cholesky-panel edges in M; ragged, exact and empty pass-1 slabs; pass-2 runs
    B  all four kinds and three mixed pairs, scattered and full grid, and z coincident with x (d = 0 in vg_kappa_z)
    C  full-grid shapes (split and unsplit Grams in one step, one grid row, n1 < n2) and the grid against the scattered route
    D  every read-out with NaN guard bands: q(u), posterior at the COL1 column-tile edges, posterior covariance, gridded read-out
    E  state and argument contracts of include/vggp.h (return codes through the C entries; a refused call changes nothing)
Each figure is printed before it is asserted (`pytest -s`): "PAIRED family case quantity error bound".

Measured on the MI355X, worst error / bound per family:
    A  0.76   ELBO part at M = 8, N = 1 048 641: 7.6e-13 against 1e-12 (Z-gradient 0.63 there, theta-gradient 0.44 at M = 130, N = 65 537)
    B  0.049  Z-gradient, scattered (Matern-3/2, RBF): 1.5e-12 against 3.1e-11
    C  0.050  Z-gradient between the grid and the scattered route: 1.1e-12 against 2.2e-11
    D  0.25   gridded read-out mean at M = 17, Matern-3/2: 3.3e-13 against 1.3e-12; every other read-out quantity <= 0.064
"""
import ctypes as C

import numpy as np
import pytest
import torch

import paired_cases as P

pytestmark = pytest.mark.gpu

GUARD = 64


def _lib():
    from variational_gridded_gaussian_processes_amd import _lib as L
    return L


def _call(engine, fn, *args):
    """A C entry on the engine's context and torch's current stream -> return code (nothing raised)."""
    return getattr(engine.lib, fn)(engine._h, *args, torch.cuda.current_stream(engine.device).cuda_stream)


def _dev(engine, a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(engine.device).contiguous()


def _guarded(engine, n):
    """-> (buffer of NaN sentinels, its interior view of n doubles)."""
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device=engine.device)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


def _report(name, q, got, want, bound=None):
    err = P.rel(got, want)
    b = P.bound(name, q) if bound is None else bound
    print(f"PAIRED {name[0]} {name} {q} {err:.3e} {b:.3e}")
    return err, b


def _plan(engine, p, as_points=False):
    """Plan the problem -> (y on the device, step(), zgrad())."""
    if p["layout"] == "scattered" or as_points:
        X = p["X"] if p["layout"] == "scattered" else P.grid_points(p)
        engine.plan_paired(p["kinds"], p["Z"], X[:, 0], X[:, 1], scattered=True)
        y = _dev(engine, p["y"])
        return y, (lambda th=p["theta"]: engine.elbo_step_scattered(y, p["yy"], th)), (lambda: engine.zgrad_scattered(y))
    engine.plan_paired(p["kinds"], p["Z"], p["x1"], p["x2"])
    Y = _dev(engine, p["y"].reshape(p["n2"], p["n1"]))
    return Y, (lambda th=p["theta"]: engine.elbo_step(Y, p["yy"], th)), (lambda: engine.zgrad(Y))


def _step_bits(step, zgrad):
    e, g, info = step()
    gz = torch.stack(zgrad(), 1).cpu().numpy()
    return e, g, gz, info["jitter"][0]


def _same_bits(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def _check_step(engine, name, as_points=False):
    ref = P.reference(name)
    p, want = ref["p"], ref["step"]
    _, step, zgrad = _plan(engine, p, as_points)
    first = _step_bits(step, zgrad)
    e, g, gz, jit = first
    res = [_report(name, "elbo", e - P.c0(p["N"], p["yy"], p["theta"][4]), want["elbo"]),
           _report(name, "grad_theta", g, want["grad_theta"]), _report(name, "grad_z", gz, want["grad_z"])]
    assert jit == want["jitter"] == 0.0
    for err, b in res:
        assert err <= b
    assert _same_bits(_step_bits(step, zgrad), first)          # bitwise repeatable
    return first


# ---- D: read-outs with guard bands ---------------------------------------------------------------------------------------------
def _qu(engine, M):
    bm, mean = _guarded(engine, M)
    bv, var = _guarded(engine, M)
    bc, cov = _guarded(engine, M * M)
    assert _call(engine, "vggp_qv_masked", mean.data_ptr(), var.data_ptr()) == 0
    assert _call(engine, "vggp_qv_cov_masked", cov.data_ptr()) == 0
    assert _intact(bm, M) and _intact(bv, M) and _intact(bc, M * M)
    return mean.cpu().numpy(), var.cpu().numpy(), cov.cpu().numpy().reshape(M, M)


def _posterior(engine, xs, ns):
    xs1, xs2 = _dev(engine, xs[:ns, 0]), _dev(engine, xs[:ns, 1])
    bm, mean = _guarded(engine, ns)
    bv, var = _guarded(engine, ns)
    assert _call(engine, "vggp_posterior_masked", xs1.data_ptr(), xs2.data_ptr(), ns, mean.data_ptr(), var.data_ptr()) == 0
    assert _intact(bm, ns) and _intact(bv, ns)
    return mean.cpu().numpy(), var.cpu().numpy()


def _posterior_cov(engine, xs, ns):
    xs1, xs2 = _dev(engine, xs[:ns, 0]), _dev(engine, xs[:ns, 1])
    bc, cov = _guarded(engine, ns * ns)
    assert _call(engine, "vggp_posterior_cov_masked", xs1.data_ptr(), xs2.data_ptr(), ns, cov.data_ptr()) == 0
    assert _intact(bc, ns * ns)
    return cov.cpu().numpy().reshape(ns, ns)


def _readout(engine, C1, C2, kd1, kd2, literal):
    mv1, mv2 = C1.shape[0], C2.shape[0]
    d = [_dev(engine, a) for a in (C1, C2, kd1, kd2)]
    bm, mean = _guarded(engine, mv1 * mv2)
    bv, var = _guarded(engine, mv1 * mv2)
    assert _call(engine, "vggp_readout_masked", d[0].data_ptr(), mv1, d[1].data_ptr(), mv2, d[2].data_ptr(), d[3].data_ptr(),
                 mean.data_ptr(), var.data_ptr(), 1 if literal else 0) == 0
    assert _intact(bm, mv1 * mv2) and _intact(bv, mv1 * mv2)
    return mean.cpu().numpy(), var.cpu().numpy()


def _check_readouts(engine, name):
    """Every read-out of the planned and stepped case against the specification; -> the worst (error, bound) pairs are asserted."""
    ref = P.reference(name)
    p, want = ref["p"], ref["read"]
    M = p["M"]
    res = []
    mean, var, cov = _qu(engine, M)
    res += [_report(name, "qu_mean", mean, want["qu_mean"]), _report(name, "qu_var", var, want["qu_var"]),
            _report(name, "qu_cov", cov, want["qu_cov"])]
    xs, mats = P.readout_inputs(M)
    pvar = {}
    for ns in P.NS_POST:
        m, v = _posterior(engine, xs, ns)
        pvar[ns] = v
        res += [_report(name, "post_mean", m, want["post_mean"][:ns]), _report(name, "post_var", v, want["post_var"][:ns])]
    for ns in P.NS_COV:
        cv = _posterior_cov(engine, xs, ns)
        res.append(_report(name, "post_cov", cv, want["post_cov"][:ns, :ns]))
        res.append(_report(name, "post_var", np.diagonal(cv), pvar[ns]))          # its diagonal == posterior_masked's variance
    for (mv1, mv2), (C1, C2, kd1, kd2) in mats.items():
        for literal in (True, False):
            tag = "lit" if literal else "cond"
            m, v = _readout(engine, C1, C2, kd1, kd2, literal)
            res += [_report(name, f"qv_mean_{tag}", m, want[f"qv_mean_{tag}_{mv1}x{mv2}"]),
                    _report(name, f"qv_var_{tag}", v, want[f"qv_var_{tag}_{mv1}x{mv2}"])]
    for err, b in res:
        assert err <= b


@pytest.mark.parametrize("name", list(P.CASES))
def test_case(engine, name):
    """Families A - D: the step of every case, and every read-out of the cases that carry them."""
    _check_step(engine, name)
    if P.CASES[name]["readouts"]:
        _check_readouts(engine, name)


def test_grid_route_against_scattered_route(engine):
    """C, last row: the same model through the Grams and Hadamard products (grid plan) and through the generated GEMM (scattered plan
    on the 3150 grid nodes).  Bound between the routes: 100 x the discrepancy of the specification's grid= and X= forms."""
    name = P.C_TWIN
    grid = _check_step(engine, name)
    pts = _check_step(engine, name, as_points=True)
    p = P.reference(name)["p"]
    k = P.c0(p["N"], p["yy"], p["theta"][4])
    res = [_report(name, "twin_elbo", pts[0] - k, grid[0] - k), _report(name, "twin_grad_theta", pts[1], grid[1]),
           _report(name, "twin_grad_z", pts[2], grid[2])]
    for err, b in res:
        assert err <= b


def test_posterior_no_points_writes_nothing(engine):
    p = P.reference("A_17_1030")["p"]
    _, step, _ = _plan(engine, p)
    step()
    xs = _dev(engine, np.zeros(4))
    bm, mean = _guarded(engine, 4)
    bv, var = _guarded(engine, 4)
    assert _call(engine, "vggp_posterior_masked", xs.data_ptr(), xs.data_ptr(), 0, mean.data_ptr(), var.data_ptr()) == 0
    assert bool(torch.isnan(bm).all()) and bool(torch.isnan(bv).all())


def test_duplicate_point_jitter(engine):
    """Two identical inducing points: the jitter the specification's psd_safe_cholesky takes, and the same bits on a repeat."""
    p = P.duplicate_problem()
    _, step, zgrad = _plan(engine, p)
    first = _step_bits(step, zgrad)
    want = P.spec_step(p)
    assert first[3] == want["jitter"] > 0
    assert _same_bits(_step_bits(step, zgrad), first)


# ---- E: state and arguments ----------------------------------------------------------------------------------------------------
E_SCATTERED, E_GRID = "A_17_1030", "B_g_1212"


def _read_bits(engine, p):
    """Bits of the read-outs that scale by the stored theta: q(u), posterior(x*) at five points, the gridded read-out (2 x 3 cells,
    both literal settings)."""
    M = p["M"]
    rng = np.random.default_rng([M, 31])
    xs = rng.random((5, 2))
    C1, C2, kd1, kd2 = rng.random((2, M)), rng.random((3, M)), 0.5 + rng.random(2), 0.5 + rng.random(3)
    mean, var = engine.qv_masked()
    out = [mean.cpu().numpy(), var.cpu().numpy()]
    out += list(_posterior(engine, xs, 5))
    for literal in (True, False):
        out += list(_readout(engine, C1, C2, kd1, kd2, literal))
    return tuple(out)


def _all_bits(engine, p, step, zgrad):
    """Step, Z-gradient and read-outs of the planned problem as one tuple of bits."""
    return _step_bits(step, zgrad) + _read_bits(engine, p)


def _eq(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def fresh(engine):
    """Bits of the two E problems on a context that has seen nothing else."""
    from variational_gridded_gaussian_processes_amd import Engine
    out = {}
    for name in (E_SCATTERED, E_GRID):
        e2 = Engine(engine.device_index)
        p = P.reference(name)["p"]
        _, step, zgrad = _plan(e2, p)
        out[name] = _all_bits(e2, p, step, zgrad)
        e2.close()
    return out


def _readout_codes(engine, p, y):
    """Return codes of every read-out and of the matching zgrad entry (outputs sized for ns = 2, mv = 2 x 2)."""
    M = p["M"]
    o = torch.zeros(max(M * M, 16), dtype=torch.float64, device=engine.device)
    o2 = torch.zeros_like(o)
    xs = _dev(engine, [0.3, 0.6])
    Cm = _dev(engine, np.ones((2, M)))
    zg = "vggp_zgrad_scattered" if p["layout"] == "scattered" else "vggp_zgrad"
    return dict(
        qv=_call(engine, "vggp_qv_masked", o.data_ptr(), o2.data_ptr()),
        qv_cov=_call(engine, "vggp_qv_cov_masked", o.data_ptr()),
        posterior=_call(engine, "vggp_posterior_masked", xs.data_ptr(), xs.data_ptr(), 2, o.data_ptr(), o2.data_ptr()),
        posterior_cov=_call(engine, "vggp_posterior_cov_masked", xs.data_ptr(), xs.data_ptr(), 2, o.data_ptr()),
        readout=_call(engine, "vggp_readout_masked", Cm.data_ptr(), 2, Cm.data_ptr(), 2, xs.data_ptr(), xs.data_ptr(), o.data_ptr(),
                      o2.data_ptr(), 1),
        zgrad=_call(engine, zg, y.data_ptr(), o.data_ptr(), o2.data_ptr()))


@pytest.mark.parametrize("name", [E_SCATTERED, E_GRID])
def test_state_before_step_and_after_set_inducing(engine, fresh, name):
    L = _lib()
    ref = P.reference(name)
    p = ref["p"]
    # planned at another Z: no step yet -> VGGP_ESTATE everywhere
    p0 = dict(p, Z=np.random.default_rng(21).random(p["Z"].shape))
    y, step, zgrad = _plan(engine, p0)
    assert set(_readout_codes(engine, p, y).values()) == {L.VGGP_ESTATE}
    step()
    assert set(_readout_codes(engine, p, y).values()) == {L.VGGP_OK}
    # moved to the case's Z: the state is gone until the next step, which then equals a fresh plan at that Z and the specification
    engine.set_inducing(0, p["Z"][:, 0])
    engine.set_inducing(1, p["Z"][:, 1])
    assert set(_readout_codes(engine, p, y).values()) == {L.VGGP_ESTATE}
    got = _all_bits(engine, p, step, zgrad)
    assert _eq(got, fresh[name])
    want = ref["step"]
    for q, val in (("elbo", got[0] - P.c0(p["N"], p["yy"], p["theta"][4])), ("grad_theta", got[1]), ("grad_z", got[2])):
        err, b = _report(name, q, val, want[q])
        assert err <= b
    err, b = _report(name, "qu_mean", got[4], ref["read"]["qu_mean"])
    assert err <= b
    assert set(_readout_codes(engine, p, y).values()) == {L.VGGP_OK}


@pytest.mark.parametrize("name", [E_SCATTERED, E_GRID])
def test_refused_arguments_change_nothing(engine, fresh, name):
    """Every refused call leaves the state of the last step as it was: after each group of refusals the read-outs and the Z-gradient
    give the bits of a context that has seen nothing else, and so does the next step."""
    L = _lib()
    p = P.reference(name)["p"]
    M = p["M"]
    scattered = p["layout"] == "scattered"
    y, step, zgrad = _plan(engine, p)
    assert _eq(_all_bits(engine, p, step, zgrad), fresh[name])

    def unchanged(after):
        gz = torch.stack(zgrad(), 1).cpu().numpy()
        assert _eq((gz,) + _read_bits(engine, p), (fresh[name][2],) + fresh[name][4:]), after

    g1, g2 = torch.zeros(M, dtype=torch.float64, device=engine.device), torch.zeros(M, dtype=torch.float64, device=engine.device)
    th = (C.c_double * 5)(*p["theta"])
    e_out, g_out = C.c_double(), (C.c_double * 5)()
    right_step = "vggp_elbo_step_scattered" if scattered else "vggp_elbo_step"
    # the Z-gradient belongs to the step's array
    other = y.clone()
    assert _call(engine, "vggp_zgrad_scattered" if scattered else "vggp_zgrad", other.data_ptr(), g1.data_ptr(), g2.data_ptr()) == L.VGGP_EINVAL
    unchanged("zgrad with another array")
    # the entry that does not match the plan (step and Z-gradient)
    wrong_step, wrong_zg = ("vggp_elbo_step", "vggp_zgrad") if scattered else ("vggp_elbo_step_scattered", "vggp_zgrad_scattered")
    assert _call(engine, wrong_step, y.data_ptr(), p["yy"], th, C.byref(e_out), g_out, None) == L.VGGP_EINVAL
    assert _call(engine, wrong_zg, y.data_ptr(), g1.data_ptr(), g2.data_ptr()) == L.VGGP_EINVAL
    unchanged("the wrong entry")
    # covariance of more than 8192 points: refused before memory is touched (a 16-double output would not survive otherwise).
    # (M ns > 2^27 cannot be reached on its own: M <= 16384 and ns <= 8192 give at most 2^27.)
    xs = torch.zeros(8193, dtype=torch.float64, device=engine.device)
    bc, cov = _guarded(engine, 16)
    assert _call(engine, "vggp_posterior_cov_masked", xs.data_ptr(), xs.data_ptr(), 8193, cov.data_ptr()) == L.VGGP_EINVAL
    assert _call(engine, "vggp_posterior_cov_masked", xs.data_ptr(), xs.data_ptr(), 0, cov.data_ptr()) == L.VGGP_EINVAL
    assert bool(torch.isnan(bc).all())
    unchanged("posterior_cov with 8193 and 0 points")
    # set_inducing: wrong length, a NaN, a third dimension -- the old Z stays
    bad = p["Z"][:, 0].copy()
    bad[M // 2] = np.nan
    for dim, z in ((0, p["Z"][:-1, 0]), (1, bad), (2, p["Z"][:, 0])):
        with pytest.raises(L.VggpError) as ei:
            engine.set_inducing(dim, z)
        assert ei.value.code == L.VGGP_EINVAL
    unchanged("refused set_inducing")
    # theta with one zero, negative, infinite or NaN component
    for i, v in ((0, 0.0), (1, -0.2), (2, float("inf")), (3, float("nan")), (4, 0.0)):
        t = list(p["theta"])
        t[i] = v
        assert _call(engine, right_step, y.data_ptr(), p["yy"], (C.c_double * 5)(*t), C.byref(e_out), g_out, None) == L.VGGP_EINVAL
    unchanged("theta with one bad component")
    # theta whose components BEFORE the bad one are valid but different: nothing of it may be stored (the read-outs scale by the
    # stored s1, s2, sigma2 and use the stored lengthscales)
    t = [2.0 * v for v in p["theta"]]
    t[4] = 0.0
    assert _call(engine, right_step, y.data_ptr(), p["yy"], (C.c_double * 5)(*t), C.byref(e_out), g_out, None) == L.VGGP_EINVAL
    unchanged("2 theta with sigma2 = 0")
    t = list(p["theta"])
    t[0], t[1], t[2] = 0.7 * t[0], 1.3 * t[1], float("inf")
    assert _call(engine, right_step, y.data_ptr(), p["yy"], (C.c_double * 5)(*t), C.byref(e_out), g_out, None) == L.VGGP_EINVAL
    unchanged("other lengthscales with s1 = inf")
    # a non-finite observation coordinate: the plan is refused and the previous one stays
    for which in (0, 1):
        x = [p["X"][:, 0].copy(), p["X"][:, 1].copy()] if scattered else [p["x1"].copy(), p["x2"].copy()]
        x[which][len(x[which]) // 2] = np.nan if which == 0 else np.inf
        with pytest.raises(L.VggpError) as ei:
            engine.plan_paired(p["kinds"], p["Z"], x[0], x[1], scattered=scattered)
        assert ei.value.code == L.VGGP_EINVAL and "observation coordinate" in str(ei.value)
    unchanged("refused plan")
    # ... and the next step gives the fresh context's bits again
    assert _eq(_all_bits(engine, p, step, zgrad), fresh[name])
