"""The dense masked and scattered steps (csrc/masked.hip) and their read-outs (csrc/masked_readout.hip) on every shape, mask and chunk
edge, against oracle/kron.py.  Cases, replica of the host decisions, reference and bounds: tests/masked_dense_cases.py (their premises
are checked on the CPU by tests/test_masked_dense_cases.py).

Every case plans through Engine.plan, steps, compares the data-dependent part of the ELBO (ELBO - C0) and EACH gradient component
relative to its own reference magnitude under bound(case, quantity) = max(100 x the reference's own floor, 1e-12) (never above the
path's ceilings), then repeats the step and asserts the same bits.
    A  grid shape of the masked step and its transposed twin: 1-D launch and 256-stride edges, fewer grid rows than column slabs,
       the long-K thresholds, and the shapes whose slab scratch exceeds the assembly's buffer
    B  masks: all ones (== vggp_elbo_step), one cell, an empty row / column, one row, checkerboard, half plane, a track, n_obs < M
    C  the blocked factor as the step wires it (M = 128, 129, 258): log-det, Sinv and both partial traces through ELBO, gradient, q(v)
    D  scattered step: N = 1 ... 131 584 (slab thresholds and the 256-slab cap), thin m, duplicates, points off the mesh, e_d = -1
    E  every read-out at its chunk edges (ns = 1, M - 1, M, M + 1, 2 M + 1) with NaN guard bands; the Z-gradient
    F  state: read-outs repeated and reordered, step after read-outs, dense -> iterative -> dense, re-plan, a refused theta
Each figure is printed before it is asserted (`pytest -s`): "MASKED_DENSE family case quantity error bound".

Measured on the MI355X, worst error / bound per family:
    A  0.16   d/dell1 at (32, 1024 | 2, 96): 1.6e-13 against 1e-12; the slab-scratch shapes <= 0.15
    B  0.21   d/dell1, one observed row: 4.0e-13 against 1.9e-12
    C  0.10   d/dell1 at M = 129: 1.6e-13 against 1.5e-12
    D  0.31   d/dell1, (points, B1): 5.6e-13 against 1.8e-12; every B0 case <= 0.04
    E  0.063  Z-gradient, N = 1023 Matern-3/2: 7.6e-13 against 1.2e-11
"""
import ctypes as C

import numpy as np
import pytest
import torch

import masked_dense_cases as P
import mixed_dims_cases as MX

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
    """The guard bands still hold their sentinels, and every one of the n outputs was written (with a finite number): a read-out that
    skips an entry fails here, not through a NaN in a comparison."""
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()) and bool(torch.isfinite(buf[GUARD:GUARD + n]).all())


def _report(name, q, err, bound=None):
    b = P.bound(name, q) if bound is None else bound
    print(f"MASKED_DENSE {name[0]} {name} {q} {err:.3e} {b:.3e}")
    return err, b


def _plan(engine, name):
    """Plan the case -> (problem, step(theta=case's), the step's data tensor: y (scattered) or Ym (masked), W or None)."""
    p = P.case_problem(name)
    d1, d2 = p["d1"], p["d2"]
    if p["layout"] == "masked":
        engine.plan(*MX.plan_args(d1, p["x1"], d2, p["x2"]))
        W = _dev(engine, p["W"])
        Ym = _dev(engine, p["Y"] * p["W"])
        return p, (lambda th=p["theta"]: engine.elbo_step_masked(Ym, W, float(p["N"]), p["yy"], th)), Ym, W
    engine.plan(*MX.plan_args(d1, p["X"][:, 0].copy(), d2, p["X"][:, 1].copy()), scattered=True)
    y = _dev(engine, p["y"])
    return p, (lambda th=p["theta"]: engine.elbo_step_scattered(y, p["yy"], th)), y, None


def _check_step(engine, name):
    """Step of the planned case against the reference, and bitwise repeatable -> (problem, step, data, W, (elbo, grad))."""
    p, step, data, W = _plan(engine, name)
    want = P.reference(name)
    e, g, info = step()
    assert info["status"] == 0
    assert np.isfinite(e) and np.isfinite(g).all()
    res = [_report(name, "elbo", float(P.rel_each(e - P.c0(p["N"], p["yy"], p["theta"][4]), want["elbo"])))]
    each = P.rel_each(g, want["grad"])
    res += [_report(name, q, float(each[i])) for i, q in enumerate(P.GRAD)]
    for err, b in res:
        assert err <= b
    e2, g2, _ = step()
    assert e2 == e and np.array_equal(g2, g)                       # bitwise repeatable
    return p, step, data, W, (e, g)


# ---- read-outs with guard bands ------------------------------------------------------------------------------------------------
def _qv(engine, M):
    bm, mean = _guarded(engine, M)
    bv, var = _guarded(engine, M)
    assert _call(engine, "vggp_qv_masked", mean.data_ptr(), var.data_ptr()) == 0
    assert _intact(bm, M) and _intact(bv, M)
    return mean.cpu().numpy(), var.cpu().numpy()


def _qv_cov(engine, M):
    bc, cov = _guarded(engine, M * M)
    assert _call(engine, "vggp_qv_cov_masked", cov.data_ptr()) == 0
    assert _intact(bc, M * M)
    return cov.cpu().numpy().reshape(M, M)


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
    return mean.cpu().numpy().reshape(mv1, mv2), var.cpu().numpy().reshape(mv1, mv2)


def _check_qv(engine, name, cov):
    want = P.reference(name)
    M = want["qv_mean"].size
    mean, var = _qv(engine, M)
    res = [_report(name, "qv_mean", P.rel(mean, want["qv_mean"].reshape(-1))), _report(name, "qv_var", P.rel(var, want["qv_var"].reshape(-1)))]
    if cov:
        cv = _qv_cov(engine, M)
        res.append(_report(name, "qv_cov", P.rel(cv, want["qv_cov"])))
        res.append(_report(name, "qv_var", P.rel(np.diagonal(cv), var)))                  # its diagonal == vggp_qv_masked's variance
        assert np.abs(cv - cv.T).max() <= 1e-13 * np.abs(cv).max()
    for err, b in res:
        assert err <= b


# ---- A - D: the step of every case ---------------------------------------------------------------------------------------------
STEP_CASES = [n for n, c in P.CASES.items() if c["read"] in (None, "qv", "qvcov")]


@pytest.mark.parametrize("name", STEP_CASES)
def test_step(engine, name):
    """Families A - D: ELBO part and every gradient component of the case; q(v) (and its covariance) where the case carries it."""
    p, step, data, W, (e, g) = _check_step(engine, name)
    read = P.CASES[name]["read"]
    if read:
        _check_qv(engine, name, cov=read == "qvcov")
    if name == "B_ones":                  # a full mask: the dense solver must agree with the Kronecker (eigen) path, as today
        e2, g2, _ = engine.elbo_step(data, p["yy"], p["theta"])
        assert abs(e2 - e) <= 1e-9 * abs(e) and P.rel(g, g2) < 1e-7


# ---- E: read-outs --------------------------------------------------------------------------------------------------------------
E_STATES = [P.E_MASKED, P.E_SCATTERED]


def _state(engine, name):
    p, step, data, W = _plan(engine, name)
    e, g, info = step()
    assert info["status"] == 0
    return p, step, data, W, (e, g)


@pytest.mark.parametrize("name", E_STATES)
def test_state_step(engine, name):
    _check_step(engine, name)


@pytest.mark.parametrize("ns", P.NS_POST)
@pytest.mark.parametrize("name", E_STATES)
def test_posterior(engine, name, ns):
    """vggp_posterior_masked at the chunk edges: one point, one short of a chunk, one chunk, one over, two chunks and one point."""
    _state(engine, name)
    want = P.reference(name)
    xs, _ = P.readout_inputs()
    assert P.readout_chunks(ns, P.M_E) == {1: 1, 34: 1, 35: 1, 36: 2, 71: 3}[ns]
    m, v = _posterior(engine, xs, ns)
    for err, b in (_report(name, "post_mean", P.rel(m, want["post_mean"][:ns])), _report(name, "post_var", P.rel(v, want["post_var"][:ns]))):
        assert err <= b


@pytest.mark.parametrize("ns", P.NS_COV)
@pytest.mark.parametrize("name", E_STATES)
def test_posterior_cov(engine, name, ns):
    _state(engine, name)
    want = P.reference(name)
    xs, _ = P.readout_inputs()
    cv = _posterior_cov(engine, xs, ns)
    _, v = _posterior(engine, xs, ns)
    res = [_report(name, "post_cov", P.rel(cv, want["post_cov"][:ns, :ns])), _report(name, "post_var", P.rel(np.diagonal(cv), v))]
    for err, b in res:
        assert err <= b
    assert np.abs(cv - cv.T).max() <= 1e-13 * np.abs(cv).max()


@pytest.mark.parametrize("name", E_STATES)
def test_posterior_cov_refuses_more_than_M_points(engine, name):
    """ns = M + 1: VGGP_EINVAL, nothing written, and the state stays readable (the next read-out gives the bits of the one before)."""
    L = _lib()
    _state(engine, name)
    xs, _ = P.readout_inputs()
    before = _posterior(engine, xs, 5)
    ns = P.M_E + 1
    xs1, xs2 = _dev(engine, xs[:ns, 0]), _dev(engine, xs[:ns, 1])
    bc, cov = _guarded(engine, ns * ns)
    assert _call(engine, "vggp_posterior_cov_masked", xs1.data_ptr(), xs2.data_ptr(), ns, cov.data_ptr()) == L.VGGP_EINVAL
    assert bool(torch.isnan(bc).all())
    after = _posterior(engine, xs, 5)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


@pytest.mark.parametrize("name", E_STATES)
def test_qv_and_cov(engine, name):
    _state(engine, name)
    _check_qv(engine, name, cov=True)


@pytest.mark.parametrize("mv", P.MV, ids=lambda mv: f"{mv[0]}x{mv[1]}")
@pytest.mark.parametrize("name", E_STATES)
def test_gridded_readout(engine, name, mv):
    """vggp_readout_masked, literal and conditional, at ns = mv1 mv2 = 1, M, M + 1 and above 2 M cells."""
    _state(engine, name)
    want = P.reference(name)
    _, mats = P.readout_inputs()
    C1, C2, kd1, kd2 = mats[mv]
    res = []
    for literal in (True, False):
        tag = "lit" if literal else "cond"
        m, v = _readout(engine, C1, C2, kd1, kd2, literal)
        res += [_report(name, f"ro_mean_{tag}", P.rel(m, want[f"ro_mean_{tag}_{mv[0]}x{mv[1]}"])),
                _report(name, f"ro_var_{tag}", P.rel(v, want[f"ro_var_{tag}_{mv[0]}x{mv[1]}"]))]
    for err, b in res:
        assert err <= b


@pytest.mark.parametrize("name", [n for n, c in P.CASES.items() if c["read"] == "zgrad"])
def test_zgrad_scattered(engine, name):
    p, step, y, _, _ = _check_step(engine, name)
    want = P.reference(name)
    g1, g2 = engine.zgrad_scattered(y)
    res = [_report(name, "zg1", P.rel(g1.cpu().numpy(), want["zg1"])), _report(name, "zg2", P.rel(g2.cpu().numpy(), want["zg2"]))]
    for err, b in res:
        assert err <= b
    h1, h2 = engine.zgrad_scattered(y)
    assert torch.equal(g1, h1) and torch.equal(g2, h2)


# ---- F: state ------------------------------------------------------------------------------------------------------------------
def _readers(engine):
    """name -> callable of every read-out of E (each returns a tuple of numpy arrays)."""
    xs, mats = P.readout_inputs()
    r = {"qv": lambda: _qv(engine, P.M_E), "qv_cov": lambda: (_qv_cov(engine, P.M_E),)}
    for ns in P.NS_POST:
        r[f"post_{ns}"] = lambda ns=ns: _posterior(engine, xs, ns)
    for ns in P.NS_COV:
        r[f"post_cov_{ns}"] = lambda ns=ns: (_posterior_cov(engine, xs, ns),)
    for mv, a in mats.items():
        for literal in (True, False):
            r[f"ro_{mv[0]}x{mv[1]}_{int(literal)}"] = lambda a=a, literal=literal: _readout(engine, *a, literal)
    return r


def _read_all(engine, order=None):
    r = _readers(engine)
    return {k: r[k]() for k in (order or list(r))}


def _same(a, b):
    return set(a) == set(b) and all(len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) for k in a)


@pytest.fixture(scope="module")
def fresh(engine):
    """Step and read-out bits of the two E states on a context that has seen nothing else."""
    from variational_gridded_gaussian_processes_amd import Engine
    out = {}
    for name in E_STATES:
        e2 = Engine(engine.device_index)
        _, _, _, _, eg = _state(e2, name)
        out[name] = (eg, _read_all(e2))
        e2.close()
    return out


def _step_same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", E_STATES)
def test_readouts_repeat_and_reorder(engine, fresh, name):
    """Every read-out twice and in two different orders gives the same bits (they share the M x M scratch matrices and the
    grow-only misc buffer), and the step after all of them equals the step before."""
    _, step, _, _, eg = _state(engine, name)
    assert _step_same(eg, fresh[name][0])
    first = _read_all(engine)
    assert _same(first, fresh[name][1])
    assert _same(_read_all(engine), first)
    keys = list(first)
    assert _same(_read_all(engine, keys[::-1]), first)
    rot = keys[len(keys) // 2:] + keys[:len(keys) // 2]
    assert _same(_read_all(engine, rot[::2] + rot[1::2]), first)
    e, g, _ = step()
    assert _step_same((e, g), eg)
    assert _same(_read_all(engine), first)


def test_dense_iterative_dense_on_one_context(engine, fresh):
    """masked -> masked_iter -> masked: vgm_prepare lays the workspace out again each time `iter` flips; the dense step and its
    read-outs after the round trip equal a fresh context's."""
    name = P.E_MASKED
    p, step, Ym, W, eg = _state(engine, name)
    assert _step_same(eg, fresh[name][0])
    _, gi, info = engine.elbo_step_masked_iter(Ym, W, float(p["N"]), p["yy"], p["theta"])
    assert np.isfinite(gi).all()
    e, g, _ = step()
    assert _step_same((e, g), fresh[name][0])
    assert _same(_read_all(engine), fresh[name][1])


@pytest.mark.parametrize("name", E_STATES)
def test_replan_and_back(engine, fresh, name):
    _state(engine, name)
    for other in ("A_257x3_5x4", "D_257", "A_3x4096_4x16"):
        _, ostep, _, _ = _plan(engine, other)
        ostep()
    _, _, _, _, eg = _state(engine, name)
    assert _step_same(eg, fresh[name][0])
    assert _same(_read_all(engine), fresh[name][1])


@pytest.mark.parametrize("name", E_STATES)
def test_refused_theta_leaves_no_state(engine, fresh, name):
    """A step refused for a non-finite theta leaves VGGP_ESTATE on every dense read-out (nothing of an earlier step stays readable),
    and the next good step gives a fresh context's bits."""
    L = _lib()
    p, step, data, W, _ = _state(engine, name)
    M = P.M_E
    e_out, g_out = C.c_double(), (C.c_double * 5)()
    for i, v in ((1, float("nan")), (4, float("inf"))):
        t = list(p["theta"])
        t[i] = v
        th = (C.c_double * 5)(*t)
        if p["layout"] == "masked":
            rc = _call(engine, "vggp_elbo_step_masked", data.data_ptr(), W.data_ptr(), float(p["N"]), p["yy"], th, C.byref(e_out), g_out, None)
        else:
            rc = _call(engine, "vggp_elbo_step_scattered", data.data_ptr(), p["yy"], th, C.byref(e_out), g_out, None)
        assert rc == L.VGGP_EINVAL
        o = torch.zeros(M * M, dtype=torch.float64, device=engine.device)
        o2 = torch.zeros_like(o)
        xs = _dev(engine, [0.3, 0.6])
        Cm1, Cm2 = _dev(engine, np.ones((2, 7))), _dev(engine, np.ones((2, 5)))
        codes = dict(
            qv=_call(engine, "vggp_qv_masked", o.data_ptr(), o2.data_ptr()),
            qv_cov=_call(engine, "vggp_qv_cov_masked", o.data_ptr()),
            posterior=_call(engine, "vggp_posterior_masked", xs.data_ptr(), xs.data_ptr(), 2, o.data_ptr(), o2.data_ptr()),
            posterior_cov=_call(engine, "vggp_posterior_cov_masked", xs.data_ptr(), xs.data_ptr(), 2, o.data_ptr()),
            readout=_call(engine, "vggp_readout_masked", Cm1.data_ptr(), 2, Cm2.data_ptr(), 2, xs.data_ptr(), xs.data_ptr(), o.data_ptr(),
                          o2.data_ptr(), 1))
        if p["layout"] == "scattered":
            codes["zgrad"] = _call(engine, "vggp_zgrad_scattered", data.data_ptr(), o.data_ptr(), o2.data_ptr())
        assert set(codes.values()) == {L.VGGP_ESTATE}, codes
        assert not bool(o.any()) and not bool(o2.any())                  # ... and nothing was written
        e, g, _ = step()
        assert _step_same((e, g), fresh[name][0])
    assert _same(_read_all(engine), fresh[name][1])
