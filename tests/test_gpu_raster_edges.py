"""vggp_raster_contract (csrc/raster.hip vg_raster_kernel) at every edge of its 64 x 64 x 16 tile, on its own:

    mean[a][b] = sum_i T1[i][a] U[i][b],      var[a][b] = c0 + c1 sum_i T1[i][a]^2 Uv[i][b]

Small-integer-valued doubles (the idiom of tests/test_gpu_gemm_edges.py): every product, square and partial sum is an integer far
below 2^53 and c0, c1 are integers too, so the fp64 result is exact in any summation order, fused or not, and is compared with an
int64 numpy product by EQUALITY -- a dropped, duplicated or misrouted k-slice, fragment or edge element cannot hide behind a
tolerance.  Operands sit in parents filled with NaN on both sides (a read past an edge that reached a product would poison it), the
outputs in parents filled with a sentinel whose bands around the output must come back untouched."""
import numpy as np
import pytest
import torch

from variational_gridded_gaussian_processes_amd import VggpError
from variational_gridded_gaussian_processes_amd._lib import VGGP_EINVAL

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.25
BAND = 193                                    # doubles of guard band on either side of an output (no multiple of anything)
QS = [1, 3, 4, 5, 18, 33, 130]                # k not a multiple of 4 / of the k-tile, one k-tile, several
PS = [1, 15, 16, 17, 63, 65, 130]             # below / at / above one MFMA block, one tile minus / plus one, three tiles
C0, C1 = 3.0, -2.0


def guarded_in(X):
    """A contiguous GPU view holding X inside a parent that is NaN on both sides."""
    parent = torch.full((X.numel() + 2 * 37,), float("nan"), dtype=torch.float64, device=DEV)
    view = parent[37:37 + X.numel()].view(*X.shape)
    view.copy_(X)
    return view


def guarded_out(P1, P2):
    parent = torch.full((P1 * P2 + 2 * BAND,), SENTINEL, dtype=torch.float64, device=DEV)
    return parent, parent[BAND:BAND + P1 * P2].view(P1, P2)


def bands_untouched(parent):
    return bool((parent[:BAND] == SENTINEL).all()) and bool((parent[-BAND:] == SENTINEL).all())


def operands(q, P1, P2):
    g = torch.Generator(device="cpu").manual_seed(10000 * q + 100 * P1 + P2)
    T1 = torch.randint(-4, 5, (q, P1), generator=g)
    U = torch.randint(-4, 5, (q, P2), generator=g)
    Uv = torch.randint(0, 5, (q, P2), generator=g)
    return T1, U, Uv


@pytest.mark.parametrize("with_var", [True, False], ids=["mean_var", "mean_only"])
@pytest.mark.parametrize("q", QS)
def test_raster_contract_is_exact_on_every_edge(engine, q, with_var):
    for P1 in PS:
        for P2 in PS:
            T1, U, Uv = operands(q, P1, P2)
            ref_m = (T1.t() @ U).double()
            ref_v = C0 + C1 * ((T1 * T1).t() @ Uv).double()
            pm, om = guarded_out(P1, P2)
            pv, ov = guarded_out(P1, P2)
            t1, u = guarded_in(T1.double()), guarded_in(U.double())
            uv = guarded_in(Uv.double()) if with_var else None
            engine.raster_contract(t1, u, uv, C0, C1, out=(om, ov if with_var else None))
            what = (q, P1, P2, with_var)
            assert torch.equal(om.cpu(), ref_m), (what, int((om.cpu() != ref_m).sum()))
            assert bands_untouched(pm), what
            if with_var:
                assert torch.equal(ov.cpu(), ref_v), (what, int((ov.cpu() != ref_v).sum()))
            else:                             # var = NULL: the second output is never written
                assert bool((pv == SENTINEL).all()), what
            assert bands_untouched(pv), what


def test_raster_contract_ignores_uv_without_var(engine):
    """Uv given, var NULL: the mean only, the same bits."""
    T1, U, Uv = operands(33, 65, 17)
    a, _ = engine.raster_contract(T1.double().to(DEV), U.double().to(DEV), None)
    pm, om = guarded_out(65, 17)
    engine.raster_contract(T1.double().to(DEV), U.double().to(DEV), Uv.double().to(DEV), out=(om, None))
    assert torch.equal(a, om) and bands_untouched(pm)


def test_raster_contract_refuses_bad_arguments(engine):
    from variational_gridded_gaussian_processes_amd._lib import check
    t = torch.zeros(4, 4, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def code(*args):
        try:
            check(engine.lib.vggp_raster_contract(engine._h, *args, st))
        except VggpError as e:
            return e.code
        return 0
    p = t.data_ptr()
    assert code(p, p, p, 4, 4, 4, 0.0, 1.0, p, p) == 0
    assert code(p, p, None, 4, 4, 4, 0.0, 1.0, p, p) == VGGP_EINVAL          # var without Uv
    assert code(None, p, p, 4, 4, 4, 0.0, 1.0, p, p) == VGGP_EINVAL
    assert code(p, p, p, 0, 4, 4, 0.0, 1.0, p, p) == VGGP_EINVAL
    assert code(p, p, p, 4, 0, 4, 0.0, 1.0, p, p) == VGGP_EINVAL
    assert code(p, p, p, 4, 4, (1 << 20) + 1, 0.0, 1.0, p, p) == VGGP_EINVAL
    # Engine.raster_contract hands pointers on: anything but contiguous float64 GPU tensors is refused before the call (engine._ptr)
    wide = torch.zeros(4, 8, dtype=torch.float64, device=DEV)
    for bad in (t.float(), t.cpu(), wide[:, ::2]):
        for args in ((bad, t, t), (t, bad, t), (t, t, bad)):
            with pytest.raises(TypeError):
                engine.raster_contract(*args)
        with pytest.raises(TypeError):
            engine.raster_contract(t, t, t, out=(bad, t))
        with pytest.raises(TypeError):
            engine.raster_contract(t, t, t, out=(t.clone(), bad))
