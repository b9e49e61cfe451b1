"""The six read-outs of the full-grid step (vggp_qv, vggp_qv_cov, vggp_posterior, vggp_posterior_cov, vggp_readout, vggp_zgrad) after
every chain of the step's state machine, against the CPU oracle.

vggp_elbo_step (csrc/step.hip) leaves a different m-space state behind depending on the chain it ran -- a full basis, the range
rows of a thin step, split-K slabs, a payload the context does not own -- and the read-outs of csrc/api.hip reach it through three
branches (the thin read-out, the cold rebuild vg_accurate_state of csrc/step.hip, or straight through).  Each test drives a plan along a trajectory to a
named state, asserts through the step's diagnostics that the intended chain ran, reads everything out, and then takes three more
steps on the same plan: a read-out that rebuilds the state replaces the basis the next step starts from.

Which chain runs where the diagnostics cannot tell: a warm RBF step without rotation rounds is either the thin chain or the full
subspace chain.  vg_thin_ok selects the thin chain for every vggp_elbo_step whose range estimate (numerical rank + margin) is at
most 32 rows in both dimensions -- at 192 x 192, m = 64 / 48 and m = 48 that is about 20 rows (numerical rank 17 / 16) -- and never
for the partials / finish pair, whose payload the context does not own: the split-API RBF state is the full subspace chain at the
same grid.  Both are covered, by shape and by entry point.  At m = 24 the same lengthscales leave rank 17 of 24: no subspace start,
the warm steps there are the extrapolated start followed by rotation rounds (less than half of the cold step's).

Bounds (all relative to the largest entry of the reference, rel()): the ELBO / gradient figures of the existing trajectory test of
each chain (1e-8 / 1e-6; 5e-8 / 3e-7 on the thin chain with the early projection, m <= 48); q(v) 1e-6; posterior 1e-6 / 1e-5; zgrad
1e-6 (Matern) / 1e-5 (RBF); qv_cov and posterior_cov share their diagonals with qv / posterior and readout shares qv's algebra: 1e-6
for means and qv_cov, 1e-5 for posterior_cov and readout's variance.  A cold step on a fresh plan at the same theta must meet the same
bounds (checked in the same run): the inputs are not too ill-conditioned for the bound.  Noise variance sigma^2 = 0.01 on the RBF
trajectories (the path of _rbf_trajectory in test_gpu_elbo.py), 0.02 on the Matern-3/2 ones: there the q(v) variance read from
the warm basis of a partials / finish step (what every read-out of that entry point used before vggp_elbo_finish kept the payload)
is off by 2.6e-5 at 192 x 192, m = 48 -- 26 times its bound -- while the posterior variance at x* stays at 6e-9.

The zgrad bound of the RBF chains is asserted in a test of its own (test_zgrad_after_rbf_chains_vs_oracle), on inducing points
for which the reference determines that gradient; see there."""
import numpy as np
import pytest
import torch

from oracle import dense as D
from oracle import kron as Kr

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_QV, TOL_PM, TOL_PV = 1e-6, 1e-6, 1e-5


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _np(t):
    return t.cpu().numpy()


# ---- the states -----------------------------------------------------------------------------------------------------------
def _quiet(info, k, first):
    return sum(info["rounds"]) == 0


def _b1_grid(m=96, pad=6):
    d = 1.0 / (m - 1 - 2 * pad)
    return np.linspace(-pad * d, 1 + pad * d, m)


_RBF0 = np.array([0.2, 0.22, 1.0, 1.1, 0.01])


def _rbf_path(k):
    return _RBF0 * (1 + 0.01 * k) * (1.3 if k >= 15 else 1.0)


def _m32_path(k):
    return np.array([0.3 * 1.01 ** k, 0.25 * 1.01 ** k, 0.9, 1.2, 0.02])


# name -> kind, basis, (n1, n2), (g1, g2), path(k) -> theta, warm plan, entry point, first step that may be the state, last step tried,
#         reached(info, k, info of step 0) -> the intended chain ran, (ELBO, gradient) bound
STATES = {
    # one cold step: the full Jacobi solve (rotation rounds)
    "cold": dict(kind="matern52", basis="points", n=(40, 33), g=(np.linspace(0, 1, 17), np.linspace(0, 1, 12)),
                 path=lambda k: np.array([0.25, 0.2, 1.3, 0.7, 0.01]) * (1 + 0.01 * k), warm=False, api="step", first=0, last=0,
                 reached=lambda i, k, i0: sum(i["rounds"]) > 0, tol=(1e-8, 1e-6)),
    # warm start (extrapolation, refinement) ending in the first-order polish
    "matern32_polished": dict(kind="matern32", basis="points", n=(96, 96), g=(np.linspace(0, 1, 64), np.linspace(0, 1, 48)),
                              path=_m32_path, warm=True, api="step", first=6, last=14,
                              reached=lambda i, k, i0: all(i["polished"]), tol=(1e-8, 1e-6)),
    # warm RBF steps: extrapolated start + rotation rounds at m = 24, no rotation round (the thin chain) at m = 64 / 48
    "rbf24_warm": dict(kind="rbf", basis="points", n=(192, 192), g=(np.linspace(0, 1, 24),) * 2, path=_rbf_path, warm=True, api="step",
                       first=6, last=14, reached=lambda i, k, i0: 0 < 2 * sum(i["rounds"]) < sum(i0["rounds"]), tol=(5e-8, 3e-7)),
    "rbf64x48_quiet": dict(kind="rbf", basis="points", n=(192, 192), g=(np.linspace(0, 1, 64), np.linspace(0, 1, 48)), path=_rbf_path,
                           warm=True, api="step", first=6, last=14, reached=_quiet, tol=(1e-8, 1e-6)),
    # the step right after the 30 % jump: the warm start is dropped and the step runs the full solve again, like step 0
    "rbf24_jump": dict(kind="rbf", basis="points", n=(192, 192), g=(np.linspace(0, 1, 24),) * 2, path=_rbf_path, warm=True, api="step",
                       first=15, last=15, reached=lambda i, k, i0: 2 * sum(i["rounds"]) >= sum(i0["rounds"]) > 0, tol=(5e-8, 3e-7)),
    "rbf64x48_jump": dict(kind="rbf", basis="points", n=(192, 192), g=(np.linspace(0, 1, 64), np.linspace(0, 1, 48)), path=_rbf_path,
                          warm=True, api="step", first=15, last=15,
                          reached=lambda i, k, i0: 2 * sum(i["rounds"]) >= sum(i0["rounds"]) > 0, tol=(1e-8, 1e-6)),
    # cold range finder + thin chain (the rounds bound of test_cold_rbf_steps_take_the_range_finder)
    "rbf96_cold_thin": dict(kind="rbf", basis="points", n=(256, 256), g=(np.linspace(0, 1, 96),) * 2,
                            path=lambda k: np.array([0.2, 0.22, 1.0, 0.9, 0.01]) * (1 + 0.01 * k), warm=False, api="step", first=0, last=0,
                            reached=lambda i, k, i0: sum(i["rounds"]) < 400, tol=(1e-8, 1e-6)),
    # Newton chain: no rotation round and no polish
    "matern12_newton": dict(kind="matern12", basis="points", n=(384, 384), g=(np.linspace(0, 1, 192),) * 2,
                            path=lambda k: np.array([0.2, 0.25, 1.0, 0.9, 0.01]) * (1 + 0.005 * k), warm=True, api="step", first=5, last=12,
                            reached=lambda i, k, i0: sum(i["rounds"]) == 0 and not any(i["polished"]), tol=(1e-8, 1e-6)),
    # Newton chain on an inverse-scaled basis (Kuu ~ 1 / s): B1 hats on a padded mesh
    "b1_newton": dict(kind="matern12", basis="b1", n=(512, 512), g=(_b1_grid(),) * 2,
                      path=lambda k: np.array([0.2, 0.25, 1.0, 0.9, 0.01]) * (1 + 0.004 * k), warm=True, api="step", first=6, last=15,
                      reached=_quiet, tol=(1e-8, 1e-6)),
    # partials into a caller's tensor + finish on a warm plan: the payload is not the context's (full subspace chain / polish)
    "split_rbf48": dict(kind="rbf", basis="points", n=(192, 192), g=(np.linspace(0, 1, 48),) * 2, path=_rbf_path, warm=True, api="split",
                        first=8, last=14, reached=_quiet, tol=(1e-8, 1e-6)),
    "split_matern32": dict(kind="matern32", basis="points", n=(96, 96), g=(np.linspace(0, 1, 64), np.linspace(0, 1, 48)), path=_m32_path,
                           warm=True, api="split", first=8, last=14, reached=lambda i, k, i0: all(i["polished"]), tol=(1e-8, 1e-6)),
}

_DATA = {}


def _data(n):
    """Grid data of one size, generated once."""
    if n not in _DATA:
        X, y, x1, x2 = D.gen_grid(*n)
        _DATA[n] = (y.reshape(n[1], n[0]), x1, x2)
    return _DATA[n]


class _Plan:
    """One planned engine context driven through either entry point."""

    def __init__(self, engine, S, warm=None):
        self.e, self.S = engine, S
        self.Yn, x1, x2 = _data(S["n"])
        self.f1 = Kr.Factor(S["basis"], S["kind"], np.asarray(S["g"][0], float), x1)
        self.f2 = Kr.Factor(S["basis"], S["kind"], np.asarray(S["g"][1], float), x2)
        engine.plan(S["kind"], S["basis"], S["g"][0], x1, S["kind"], S["basis"], S["g"][1], x2,
                    warm_start=S["warm"] if warm is None else warm)
        self.Y = torch.tensor(self.Yn, device=DEV)
        self.yy = engine.sumsq(self.Y)
        self.pay = torch.empty(engine.payload_len, dtype=torch.float64, device=DEV)      # the caller's payload tensor

    def step(self, th, api=None):
        if (api or self.S["api"]) == "split":
            self.e.elbo_partials(self.Y, th, self.pay)
            return self.e.elbo_finish(self.pay, self.yy, th)
        return self.e.elbo_step(self.Y, self.yy, th)

    def oracle(self, th):
        return Kr.elbo_step(self.Yn, self.f1, self.f2, th)


def _drive(engine, S):
    """Run the state's trajectory up to the first step (from S['first'] on) whose diagnostics show the intended chain."""
    p = _Plan(engine, S)
    infos = []
    for k in range(S["last"] + 1):
        elbo, grad, info = p.step(S["path"](k))
        assert info["status"] == 0, (k, info)
        infos.append(info)
        if k >= S["first"] and S["reached"](info, k, infos[0]):
            return p, k, elbo, grad, infos
    raise AssertionError(f"the intended chain did not run: {[(i['rounds'], i['polished']) for i in infos]}")


# ---- references -----------------------------------------------------------------------------------------------------------------
def _cells(f, mesh, ell):
    """Unit-outputscale Cov(v, u) (mv x m) of B0 cells on `mesh` with the inducing features of f, and the unit diagonal of Kvv:
    the oracle's closed forms where it has them (Matern-1/2 points, B1 hats), 8-point Gauss-Legendre cell integrals of the kernel
    otherwise (the read-out is linear algebra in these inputs; GPU and oracle receive the same arrays)."""
    if f.kind == "matern12":
        return Kr.cross_b0(f, mesh, ell)
    xg, wg = np.polynomial.legendre.leggauss(8)
    mid, half = 0.5 * (mesh[1:] + mesh[:-1]), 0.5 * (mesh[1:] - mesh[:-1])
    t = mid[:, None] + half[:, None] * xg[None, :]                                       # (mv, 8) nodes of every cell
    z = np.asarray(f.grid, float)
    C = (Kr.kappa_and_dell(f.kind, np.abs(t[:, :, None] - z[None, None, :]), ell)[0] * (half[:, None] * wg[None, :])[:, :, None]).sum(1)
    w2 = (half[:, None] * wg[None, :])
    kd = np.array([(Kr.kappa_and_dell(f.kind, np.abs(t[a][:, None] - t[a][None, :]), ell)[0] * np.outer(w2[a], w2[a])).sum()
                   for a in range(len(mid))])
    return C, kd


def _meshes(S):
    """B0 output meshes of different sizes in the two dimensions (B1: cells between the hats' knots, as the reference pads them)."""
    if S["basis"] == "b1":
        g = np.asarray(S["g"][0], float)
        return g[6:len(g) - 6], g[10:len(g) - 10]
    return np.linspace(0, 1, 8), np.linspace(0.1, 0.9, 6)


XS = np.random.default_rng(2).uniform(-0.05, 1.05, (64, 2))          # a few points outside the data range
_REF = {}


def _reference(engine, name, k):
    """Oracle step and read-outs at the theta of step k of a state, computed once and shared by the tests of that state; the cold
    step on a fresh plan at that theta is checked against the same bounds here."""
    key = (name, k)
    if key in _REF:
        return _REF[key]
    S = STATES[name]
    th = S["path"](k)
    Yn, x1, x2 = _data(S["n"])
    f1 = Kr.Factor(S["basis"], S["kind"], np.asarray(S["g"][0], float), x1)
    f2 = Kr.Factor(S["basis"], S["kind"], np.asarray(S["g"][1], float), x2)
    st = Kr.elbo_step(Yn, f1, f2, th)
    M = f1.m * f2.m
    mesh1, mesh2 = _meshes(S)
    C1, kd1 = _cells(f1, mesh1, th[0])
    C2, kd2 = _cells(f2, mesh2, th[1])
    assert C1.shape[0] != C2.shape[0]
    R = dict(th=th, st=st, M=M, C=(C1, C2, kd1, kd2), qv=Kr.q_v(st), qv_cov=Kr.q_v_cov(st) if M <= 8192 else None,
             post=Kr.posterior(st, f1, f2, XS), post_cov=Kr.posterior_cov(st, f1, f2, XS),
             ro_lit=Kr.readout(st, f1, f2, C1, C2, kd1, kd2, literal=True), ro_cond=Kr.readout(st, f1, f2, C1, C2, kd1, kd2, literal=False),
             zg=Kr.z_grad(st, f1, f2, Yn) if S["basis"] == "points" else None, zg_tol=1e-5 if S["kind"] == "rbf" else 1e-6)
    _REF[key] = R
    p = _Plan(engine, S, warm=False)
    elbo, grad, info = p.step(th, api="step")
    figs = [("cold elbo", abs(elbo - st.elbo) / abs(st.elbo), S["tol"][0]), ("cold grad", rel(grad, st.grad), S["tol"][1])]
    figs, _ = _without_rbf_zgrad(figs + _read(engine, p, R, FORWARD, "cold "), S)
    _check(figs, f"{name}: cold step on a fresh plan at theta of step {k}")
    return R


# ---- read-outs ------------------------------------------------------------------------------------------------------------------
FORWARD = ("qv", "posterior", "qv_cov", "posterior_cov", "readout_literal", "readout_conditional", "zgrad")
REVERSE = ("zgrad", "readout_literal", "posterior_cov", "readout_conditional", "qv_cov", "posterior", "qv")


def _read(engine, p, R, order, tag=""):
    """Every read-out in the given order -> [(label, measured relative error, bound)]."""
    from variational_gridded_gaussian_processes_amd import VggpError
    xs = torch.tensor(XS, device=DEV)
    C1, C2, kd1, kd2 = [torch.tensor(a) for a in R["C"]]
    figs = []
    for what in order:
        if what == "qv":
            mean, var = engine.qv()
            figs += [(tag + "qv mean", rel(_np(mean), R["qv"][0]), TOL_QV), (tag + "qv var", rel(_np(var), R["qv"][1]), TOL_QV)]
        elif what == "posterior":
            pm, pv = engine.posterior(xs)
            figs += [(tag + "posterior mean", rel(_np(pm), R["post"][0]), TOL_PM), (tag + "posterior var", rel(_np(pv), R["post"][1]), TOL_PV)]
        elif what == "qv_cov":
            if R["M"] <= 8192:
                figs.append((tag + "qv_cov", rel(_np(engine.qv_cov()), R["qv_cov"]), TOL_QV))
            else:                                   # the header's limit: a dense M x M covariance is refused, the state stays
                with pytest.raises(VggpError):
                    _qv_cov_beyond_limit(engine)
        elif what == "posterior_cov":
            figs.append((tag + "posterior_cov", rel(_np(engine.posterior_cov(xs)), R["post_cov"]), TOL_PV))
        elif what in ("readout_literal", "readout_conditional"):
            lit = what == "readout_literal"
            mean, var = engine.readout(C1, C2, kd1, kd2, literal=lit)
            rm, rv = R["ro_lit" if lit else "ro_cond"]
            assert mean.shape == rm.shape
            figs += [(tag + what + " mean", rel(_np(mean), rm), TOL_QV), (tag + what + " var", rel(_np(var), rv), TOL_PV)]
        elif what == "zgrad" and R["zg"] is not None:
            g1, g2 = engine.zgrad(p.Y)
            figs += [(tag + "zgrad 1", rel(_np(g1), R["zg"][0]), R["zg_tol"]), (tag + "zgrad 2", rel(_np(g2), R["zg"][1]), R["zg_tol"])]
    return figs


def _qv_cov_beyond_limit(engine):
    """vggp_qv_cov beyond M = 8192 with a one-element output: the size check comes before anything is written."""
    from variational_gridded_gaussian_processes_amd._lib import check
    out = torch.empty(1, dtype=torch.float64, device=DEV)
    check(engine.lib.vggp_qv_cov(engine._h, out.data_ptr(), torch.cuda.current_stream(engine.device).cuda_stream))


def _without_rbf_zgrad(figs, S):
    """-> (the figures asserted here, the zgrad figures of an RBF state on evenly spread inducing points: printed only -- the reference
    does not determine them to the bound there; the bound is asserted in test_zgrad_after_rbf_chains_vs_oracle on moved inputs)."""
    held = [f for f in figs if S["kind"] == "rbf" and "zgrad" in f[0]]
    for label, err, bound in held:
        print(f"(bound asserted in test_zgrad_after_rbf_chains_vs_oracle) {label}: {err:.3e} (bound {bound:.0e})")
    return [f for f in figs if f not in held], held


def _state(engine, name):
    """Drive the plan to the named state; the first visit also computes the reference and checks the cold step at its theta."""
    S = STATES[name]
    p, k, elbo, grad, infos = _drive(engine, S)
    if (name, k) not in _REF:
        _reference(engine, name, k)                          # (its cold check re-plans the context: drive again)
        p, k2, elbo, grad, infos = _drive(engine, S)
        assert k2 == k
    return p, k, elbo, grad, infos, _REF[(name, k)]


def _check(figs, what):
    for label, err, bound in figs:
        print(f"{what}: {label}: {err:.3e} (bound {bound:.0e})")
    bad = [(label, float(f"{err:.3e}"), bound) for label, err, bound in figs if not err < bound]
    assert not bad, (what, bad)


# ---- the tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name", list(STATES))
def test_readouts_after_each_chain_vs_oracle(engine, name, order):
    """Step value, gradient and every read-out after the named chain, then three more steps from whatever basis the read-outs left.
    forward: the q(v) / posterior pair first (after a thin step: the thin read-outs), the rebuilding read-outs after them;
    reverse: zgrad, readout and posterior_cov first, q(v) last (the rebuild is the first consumer of the step's state).
    Beyond M = 8192 (m = 96 / 96, 192, B1 96) vggp_qv_cov must refuse; the other five are tested."""
    S = STATES[name]
    p, k, elbo, grad, infos, R = _state(engine, name)
    st = R["st"]
    figs = [("elbo", abs(elbo - st.elbo) / abs(st.elbo), S["tol"][0]), ("grad", rel(grad, st.grad), S["tol"][1])]
    figs, _ = _without_rbf_zgrad(figs + _read(engine, p, R, FORWARD if order == "forward" else REVERSE), S)
    for j in range(1, 4):
        th = S["path"](k + j)
        e2, g2, info = p.step(th)
        assert info["status"] == 0, (j, info)
        ref = p.oracle(th)
        figs += [(f"step +{j} elbo", abs(e2 - ref.elbo) / abs(ref.elbo), S["tol"][0]), (f"step +{j} grad", rel(g2, ref.grad), S["tol"][1])]
        print(f"{name}/{order}: step +{j}: rounds {info['rounds']}, polished {info['polished']}")
    print(f"{name}/{order}: state at step {k}: rounds {infos[k]['rounds']}, polished {infos[k]['polished']}, "
          f"rounds of the trajectory {[sum(i['rounds']) for i in infos]}")
    _check(figs, f"{name}/{order}")


# Inducing points of the RBF states' zgrad test, as (first, last) of an even spread: part of the data range is left without inducing
# points (m = 24 warm: only its upper tenth, so that the numerical rank stays at 15 - 16 of 24 and the subspace start stays off;
# the partials / finish pair: [0, 0.7], where its full subspace chain runs without rotation rounds from step 10 on)
ZGRAD_SPAN = {"rbf24_warm": (0.0, 0.9), "rbf24_jump": (0.4, 0.6), "rbf64x48_quiet": (0.4, 0.6), "rbf64x48_jump": (0.4, 0.6),
              "rbf96_cold_thin": (0.0, 0.5), "split_rbf48": (0.0, 0.7)}


@pytest.mark.parametrize("name", list(ZGRAD_SPAN))
def test_zgrad_after_rbf_chains_vs_oracle(engine, name):
    """vggp_zgrad as the first read-out after each RBF chain, and after the cold step on a fresh plan at the same theta, at the 1e-5
    of test_zgrad_vs_oracle -- on inducing points that do NOT cover the data range evenly.

    With m points spread evenly over [0, 1] (the plans of the test above) the ELBO is nearly stationary in Z: its largest gradient
    component is 0.04 - 0.08, the residue of terms of size 1e6 that cancel, and cond(Kuu + 1e-8 I) ~ 1e10 sits in front of their
    rounding.  The REFERENCE's own z_grad then moves by 2e-5 ... 2e-3 when Z changes by one unit in the last place, and the engine's
    cold step differs from it by as much (measured, dimension 1 / 2: m = 24 1.7e-3 / 2.7e-4; m = 64 / 48 4.2e-3 / 7.7e-4, after the
    jump 7.4e-5 / 1.0e-4; m = 96 4.9e-3 / 3.9e-3; m = 48 1.2e-3 / 1.6e-4): those inputs are too ill-conditioned for THIS read-out,
    whatever the chain -- the test above still calls it there, in sequence, for what it does to the state.  Moved inputs: the same
    grids, kernels, trajectories and chains (asserted by the same diagnostics), inducing points on part of the range only.  The
    gradient is then 3e2 - 2e6 and the reference moves by 4e-8 ... 2e-6 under the same perturbation."""
    a, b = ZGRAD_SPAN[name]
    S = dict(STATES[name], g=tuple(np.linspace(a, b, len(g)) for g in STATES[name]["g"]))
    p, k, elbo, grad, infos = _drive(engine, S)
    th = S["path"](k)
    st = p.oracle(th)
    r1, r2 = Kr.z_grad(st, p.f1, p.f2, p.Yn)
    g1, g2 = engine.zgrad(p.Y)
    figs = [("zgrad 1", rel(_np(g1), r1), 1e-5), ("zgrad 2", rel(_np(g2), r2), 1e-5)]
    print(f"{name}: zgrad state at step {k}: rounds {infos[k]['rounds']}, trajectory {[sum(i['rounds']) for i in infos]}, "
          f"elbo {abs(elbo - st.elbo) / abs(st.elbo):.2e}, grad {rel(grad, st.grad):.2e}, largest |dELBO/dz| {np.abs(r1).max():.2e}")
    pc = _Plan(engine, S, warm=False)
    pc.step(th, api="step")
    g1, g2 = engine.zgrad(pc.Y)
    figs += [("cold zgrad 1", rel(_np(g1), r1), 1e-5), ("cold zgrad 2", rel(_np(g2), r2), 1e-5)]
    _check(figs, f"{name}: zgrad")


def test_mixed_entry_points_on_one_warm_plan(engine):
    """vggp_elbo_step x 6 (into the thin chain), partials / finish x 2 (which cannot run thin: vg_warm restarts cold), vggp_elbo_step x 3
    on ONE warm RBF context: every step against the oracle, q(v) and posterior after the last step of each group."""
    S = dict(STATES["split_rbf48"])
    p = _Plan(engine, S)
    xs = torch.tensor(XS, device=DEV)
    figs, k = [], 0
    for api, count, tol in (("step", 6, (5e-8, 3e-7)), ("split", 2, (1e-8, 1e-6)), ("step", 3, (5e-8, 3e-7))):
        for _ in range(count):
            th = _rbf_path(k)
            elbo, grad, info = p.step(th, api=api)
            assert info["status"] == 0, (k, info)
            ref = p.oracle(th)
            figs += [(f"step {k} ({api}) elbo", abs(elbo - ref.elbo) / abs(ref.elbo), tol[0]), (f"step {k} ({api}) grad", rel(grad, ref.grad), tol[1])]
            print(f"mixed: step {k} ({api}): rounds {info['rounds']}")
            k += 1
        mean, var = engine.qv()
        pm, pv = engine.posterior(xs)
        rm, rv = Kr.q_v(ref)
        om, ov = Kr.posterior(ref, p.f1, p.f2, XS)
        figs += [(f"after step {k - 1} qv mean", rel(_np(mean), rm), TOL_QV), (f"after step {k - 1} qv var", rel(_np(var), rv), TOL_QV),
                 (f"after step {k - 1} posterior mean", rel(_np(pm), om), TOL_PM), (f"after step {k - 1} posterior var", rel(_np(pv), ov), TOL_PV)]
    _check(figs, "mixed entry points")


@pytest.mark.parametrize("name", ["cold_points", "thin_rbf"])
def test_posterior_beyond_one_chunk(engine, name):
    """vggp_posterior walks x* in chunks of 65536 points: 65536 + 37 points after a cold step (Matern-1/2 points, m = 9 / 7, 16 x 12) and
    after a thin RBF step (192 x 192, m = 48), against the oracle over all points and over the last 37 -- the second chunk -- alone."""
    if name == "cold_points":
        S = dict(kind="matern12", basis="points", n=(16, 12), g=(np.linspace(0, 1, 9), np.linspace(0, 1, 7)),
                 path=lambda k: np.array([0.2, 0.3, 1.0, 0.8, 0.01]), warm=False, api="step", first=0, last=0,
                 reached=lambda i, k, i0: sum(i["rounds"]) > 0)
    else:
        S = dict(STATES["split_rbf48"], api="step", first=6)
    p, k, elbo, grad, infos = _drive(engine, S)
    st = p.oracle(S["path"](k))
    ns = 65536 + 37
    xs = np.random.default_rng(4).uniform(0, 1, (ns, 2))
    pm, pv = engine.posterior(torch.tensor(xs, device=DEV))
    assert pm.shape == (ns,) and pv.shape == (ns,)
    om, ov = Kr.posterior(st, p.f1, p.f2, xs)
    pm, pv = _np(pm), _np(pv)
    _check([("mean, all points", rel(pm, om), TOL_PM), ("var, all points", rel(pv, ov), TOL_PV),
            ("mean, last 37", rel(pm[-37:], om[-37:]), TOL_PM), ("var, last 37", rel(pv[-37:], ov[-37:]), TOL_PV),
            ("mean, first chunk", rel(pm[:65536], om[:65536]), TOL_PM), ("var, first chunk", rel(pv[:65536], ov[:65536]), TOL_PV)],
           f"posterior chunks / {name}")
