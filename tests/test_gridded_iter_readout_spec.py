"""CPU check of the specification of the gridded read-out after an iterative step (tests/gridded_iter_readout_spec.py: mean by two
products, literal variance by one Gram product over the data, conditional variance by block PCG) against the literal dense formulas
(oracle/dense.py DenseKron.q_v_gridded) on a small problem, and against the dense Sigma~ on along-track points.

Measured: small problems, of the largest reference entry: mean <= 5.3e-11 (the PCG tolerance of a0), literal variance <= 1.1e-14,
conditional variance <= 6.0e-14, 10-11 iterations; track points: conditional variance against Sigma~^-1 <= 9.7e-15, literal closed form
against t^T Sigma~ t <= 1.8e-15, 10-11 iterations."""
import functools

import numpy as np
import pytest
import torch

import gridded_iter_readout_spec as G
import scattered_iter_spec as S
from oracle import dense as D
from oracle import kron as Kr

LIMS = (-0.1, 1.1)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def vff_grid(nf):
    return np.concatenate([[LIMS[0], LIMS[1]], D.vff_omegas(nf, *LIMS).double().numpy()])


def small(data):
    """The points of test_gpu_models.test_gridded_vff_model_readout_on_incomplete_data_vs_dense: a 24 x 20 grid with 30 % missing,
    as it is ("masked") or jittered off the grid ("scattered")."""
    n1, n2 = 24, 20
    X, y, x1, x2 = D.gen_grid(n1, n2)
    rng = np.random.default_rng(5)
    keep = rng.random(len(y)) > 0.3
    Xk, yk = X[keep], y[keep]
    if data == "scattered":
        Xk = np.clip(Xk + rng.normal(scale=4e-3, size=Xk.shape), 0.0, 1.0)
    return Xk, yk, x1, x2, keep.reshape(n2, n1).astype(np.float64), (y * keep).reshape(n2, n1)


@pytest.mark.parametrize("basis", ["points", "vff"])
@pytest.mark.parametrize("data", ["scattered", "masked"])
def test_spec_equals_the_dense_gridded_readout(data, basis):
    ns = 7
    X, y, x1, x2, W, Ym = small(data)
    theta = Kr.theta_from_raw(np.zeros(5))
    if basis == "points":
        z = np.linspace(0, 1, 6)
        g, dm = z, D.DenseKron(X, y, "points", "matern12", torch.tensor(z), torch.tensor(z))
    else:
        g, dm = vff_grid(5), D.DenseKron(X, y, "vff", "matern12", (LIMS[0], LIMS[1], 5), (LIMS[0], LIMS[1], 5))
    f1, f2 = Kr.Factor(basis, "matern12", g, x1), Kr.Factor(basis, "matern12", g, x2)
    st = G.prepare_scattered(X, y, f1, f2, theta) if data == "scattered" else G.prepare_masked(Ym, W, f1, f2, theta)
    mesh = np.linspace(0, 1, ns + 1)
    (C1, kd1), (C2, kd2) = Kr.cross_b0(f1, mesh, theta[0]), Kr.cross_b0(f2, mesh, theta[1])
    tm = torch.tensor(mesh)
    for literal in (True, False):
        qd = dm.q_v_gridded(tm, tm, literal=literal)
        mean, var, info = G.readout(st, C1, C2, kd1, kd2, literal=literal)
        e_m, e_v = rel(mean.reshape(-1), qd.mean.detach().numpy()), rel(var, qd.variance.detach().numpy())
        print(f"{data}-{basis} literal={literal}: N = {len(y)}, mean {e_m:.1e} var {e_v:.1e} solves {info['solves']} its {info['rounds']}")
        assert e_m <= 1e-9
        assert e_v <= 1e-9
        assert info["solves"] == (0 if literal else 1)


@functools.lru_cache(maxsize=None)
def track_state(basis):
    X, y = S.trk(400, 0.5)
    g = vff_grid(6) if basis == "vff" else np.linspace(0.0, 1.0, 16)
    e = np.empty(0)
    f1, f2 = Kr.Factor(basis, "matern12", g, e), Kr.Factor(basis, "matern12", g, e)
    st = G.prepare_scattered(X, y, f1, f2, S.THETA_B)
    (C1, kd1), (C2, kd2) = Kr.cross_b0(f1, np.linspace(0, 1, 10), S.THETA_B[0]), Kr.cross_b0(f2, np.linspace(0, 1, 9), S.THETA_B[1])
    ops = (C1, C2, kd1, kd2)
    return st, ops, G.readout_dense(st, *ops, literal=False), G.readout_dense(st, *ops, literal=True)


@pytest.mark.parametrize("basis", ["vff", "points"])
def test_spec_on_track_points(basis):
    """trk(400, 0.5), 9 x 8 = 72 cells: a full block of 64 and a ragged one (block 64), five blocks (block 16)."""
    st, ops, ref_cond, ref_lit = track_state(basis)
    assert st.d1.B.shape[0] == (13 if basis == "vff" else 16) and st.iters < 30
    _, lit, info = G.readout(st, *ops, literal=True)
    print(f"{basis}: a0 iterations {st.iters}; literal closed form against t^T Sigma~ t {rel(lit, ref_lit):.1e}")
    assert info["solves"] == 0 and rel(lit, ref_lit) <= 1e-8
    for block, solves in ((64, 2), (16, 5)):
        _, var, info = G.readout(st, *ops, literal=False, block=block)
        print(f"{basis} block {block}: conditional variance against Sigma~^-1 {rel(var, ref_cond):.1e}, most iterations {info['rounds']}")
        assert info["solves"] == solves and info["rounds"] < 30
        assert rel(var, ref_cond) <= 1e-8
    cells = np.array([0, 71, 17, 40, 63])
    _, vc, info = G.readout(st, *ops, literal=False, cells=cells)
    assert info["solves"] == 1 and rel(vc, ref_cond[cells]) <= 1e-8
