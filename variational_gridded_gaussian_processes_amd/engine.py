"""Thin host wrapper over the C-ABI: one `Engine` = one vggp_ctx on one GPU.

PyTorch is used only as the array container (device memory, streams); every number comes out
of libvggp_hip.so.  All tensors handed to the engine must be CUDA(ROCm) float64 and contiguous.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import BASIS, KIND, Desc, Info, check


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise TypeError("engine tensors must be contiguous float64 on the GPU")
    return t.data_ptr()


def _stream(device=None) -> int:
    """torch's current stream ON THE ENGINE'S DEVICE (not on torch's current device)."""
    return torch.cuda.current_stream(device).cuda_stream


def _dvec(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))


def _basis_m(basis: str, g: np.ndarray) -> int:
    """Number of inducing features of a dimension from its grid array."""
    if basis == "one":
        return 1
    if basis in ("b0", "b0k"):
        return len(g) - 1
    if basis == "vff":
        return 2 * (len(g) - 3) + 1
    return len(g)


class Engine:
    """Owns a vggp_ctx.  See include/vggp.h for the contract of every call."""

    def __init__(self, device: Optional[int] = None, n_ranks: int = 1, rank: int = 0, unique_id: Optional[bytes] = None,
                 allreduce=None):
        """n_ranks > 1: this process is rank `rank` of a row-sharded job (one Engine per GPU).  `unique_id` (bytes from
        Engine.unique_id() on rank 0, distributed by the host program) gives the context its RCCL communicator; or
        `allreduce(numpy_view)` -- a Python function summing a float64 array over the ranks in place -- installs the host
        callback transport (the multi-rank rehearsal on one GPU, where RCCL refuses duplicate devices)."""
        if not torch.cuda.is_available():
            raise RuntimeError("variational_gridded_gaussian_processes_amd needs a gfx950 GPU: "
                               "torch.cuda.is_available() is False and there is no CPU path")
        self.lib = _lib.load()
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.n_ranks, self.rank = int(n_ranks), int(rank)
        if unique_id is not None and len(unique_id) != _lib.UNIQUE_ID_BYTES:
            raise ValueError(f"unique_id must be {_lib.UNIQUE_ID_BYTES} bytes")
        h = C.c_void_p()
        uid = C.create_string_buffer(bytes(unique_id), _lib.UNIQUE_ID_BYTES) if unique_id is not None else None
        check(self.lib.vggp_create(C.byref(h), self.device_index, self.n_ranks, self.rank, C.cast(uid, C.c_void_p) if uid else None))
        self._h = h
        self._cb = None
        if allreduce is not None:
            def _trampoline(_user, buf, count, fn=allreduce):
                try:
                    fn(np.ctypeslib.as_array(buf, shape=(int(count),)))
                    return 0
                except Exception:          # never let a Python exception cross the C boundary
                    import traceback
                    traceback.print_exc()
                    return 1
            self._cb = _lib.ALLREDUCE_FN(_trampoline)          # keep the thunk alive as long as the context
            check(self.lib.vggp_set_allreduce(self._h, self._cb, None))
        self.m1 = self.m2 = self.n1 = self.n2 = 0
        self.planned = False
        self._step_bufs = None
        self.paired = False          # the current plan is a paired one (plan_paired)
        self.plan_token = 0          # bumped by every plan(): a model sharing this engine re-plans when it is not the last planner
        self.exact_n = 0             # points of the current exact plan (exact_plan)
        self.exact_token = 0         # ... and its counter, for the exact models that share this engine
        self.exact_iter_n = 0        # the same for the iterative exact plan (exact_iter_plan)
        self.exact_iter_token = 0

    @staticmethod
    def unique_id() -> bytes:
        """RCCL unique id for Engine(..., n_ranks, rank, unique_id): call on rank 0, ship the bytes to the other ranks."""
        buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        check(_lib.load().vggp_unique_id(C.cast(buf, C.c_void_p)))
        return buf.raw

    @property
    def transport(self) -> str:
        t = C.c_int()
        check(self.lib.vggp_comm_info(self._h, None, None, C.byref(t)))
        return {0: "none", 1: "rccl", 2: "callback"}[t.value]

    def comm_info(self) -> dict:
        """What the CONTEXT reports about its collective (vggp_comm_info): communicator size, this rank, transport."""
        n, r, t = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.vggp_comm_info(self._h, C.byref(n), C.byref(r), C.byref(t)))
        return {"n_ranks": n.value, "rank": r.value, "transport": {0: "none", 1: "rccl", 2: "callback"}[t.value]}

    def allreduce(self, t: torch.Tensor) -> torch.Tensor:
        """The context's sum all-reduce on a contiguous float64 GPU tensor, in place."""
        check(self.lib.vggp_allreduce(self._h, _ptr(t), t.numel(), _stream(self.device)))
        return t

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vggp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- planning -------------------------------------------------------------------------------
    def plan(self, kind1: str, basis1: str, grid1, x1, kind2: str, basis2: str, grid2, x2,
             n_total: Optional[int] = None, warm_start: bool = False, b0_f32_kdelta: bool = False,
             block_jacobi: bool = False, scattered: bool = False) -> None:
        """grid_d: mesh (m+1 knots, basis 'b0' or 'b0k'), inducing coordinates (m, 'points'), knot mesh (m, 'b1') or
        [a, b, omega_0 .. omega_M] (m = 2M + 1, 'vff'); x_d: the n_d unique (local) observation coordinates along d."""
        x1, x2 = _dvec(x1), _dvec(x2)
        g1 = _dvec(grid1) if basis1 != "one" else np.ones(1)
        g2 = _dvec(grid2) if basis2 != "one" else np.ones(1)
        m1, m2 = _basis_m(basis1, g1), _basis_m(basis2, g2)
        d = Desc()
        d.kind1, d.basis1, d.kind2, d.basis2 = KIND[kind1], BASIS[basis1], KIND[kind2], BASIS[basis2]
        d.n1, d.n2, d.m1, d.m2 = len(x1), len(x2), m1, m2
        d.n_total = int(n_total) if n_total is not None else len(x1) * len(x2)
        d.x1, d.x2 = x1.ctypes.data, x2.ctypes.data
        d.grid1, d.grid2 = g1.ctypes.data, g2.ctypes.data
        d.warm_start = 1 if warm_start else 0
        d.flags = (_lib.FLAG_B0_F32_KDELTA if b0_f32_kdelta else 0) | (_lib.FLAG_BLOCK_JACOBI if block_jacobi else 0) | \
                  (_lib.FLAG_SCATTERED if scattered else 0)
        if scattered:          # x1[k], x2[k]: the coordinates of point k (no grid)
            if len(x1) != len(x2):
                raise ValueError("scattered plan: x1 and x2 must hold one coordinate pair per point")
            d.n_total = int(n_total) if n_total is not None else len(x1)      # (point-sharded job: points over all ranks)
        self.scattered = bool(scattered)
        with torch.cuda.device(self.device):
            check(self.lib.vggp_plan(self._h, C.byref(d)))
        self.paired = False
        self.m1, self.m2, self.n1, self.n2 = m1, m2, len(x1), len(x2)
        self.payload_len = int(self.lib.vggp_payload_len(self._h))
        self.planned = True
        self.plan_token += 1

    def plan_paired(self, kind, Z, x1, x2, scattered: bool = False) -> None:
        """Paired (general) inducing points (VGGP_FLAG_PAIRED_Z): Z (M, 2) any set of points, Kuu = s (K1 o K2).  kind: one kernel
        name for both dimensions, or a pair (kind1, kind2).  x1, x2: the grid axes of Y [n2, n1], or (scattered=True) the
        coordinates of the N points.  The steps, zgrad*, set_inducing, qv_masked, qv_cov_masked, readout(masked=True) and
        posterior_masked / posterior_cov(masked=True) then mean the paired model."""
        kind1, kind2 = (kind, kind) if isinstance(kind, str) else kind
        Zn = np.ascontiguousarray(np.asarray(Z, dtype=np.float64).reshape(-1, 2))
        z1, z2 = np.ascontiguousarray(Zn[:, 0]), np.ascontiguousarray(Zn[:, 1])
        x1, x2 = _dvec(x1), _dvec(x2)
        if scattered and len(x1) != len(x2):
            raise ValueError("scattered plan: x1 and x2 must hold one coordinate pair per point")
        M = Zn.shape[0]
        d = Desc()
        d.kind1, d.kind2 = KIND[kind1], KIND[kind2]
        d.basis1 = d.basis2 = BASIS["points"]
        d.n1, d.n2, d.m1, d.m2 = len(x1), len(x2), M, M
        d.n_total = len(x1) if scattered else len(x1) * len(x2)
        d.x1, d.x2, d.grid1, d.grid2 = x1.ctypes.data, x2.ctypes.data, z1.ctypes.data, z2.ctypes.data
        d.warm_start = 0
        d.flags = _lib.FLAG_PAIRED_Z | (_lib.FLAG_SCATTERED if scattered else 0)
        with torch.cuda.device(self.device):
            check(self.lib.vggp_plan(self._h, C.byref(d)))
        self.scattered = bool(scattered)
        self.paired = True
        self.m1, self.m2, self.n1, self.n2 = M, M, len(x1), len(x2)
        self.payload_len = 0
        self.planned = True
        self.plan_token += 1

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.vggp_workspace_bytes(self._h))

    # -- hot path ---------------------------------------------------------------------------------
    def _check_Y(self, Y: torch.Tensor):
        if tuple(Y.shape) != (self.n2, self.n1):
            raise ValueError(f"Y must be [n2={self.n2}, n1={self.n1}] (x1 fastest), got {tuple(Y.shape)}")

    def elbo_step(self, Y: torch.Tensor, yy_total: float, theta: Sequence[float]):
        """-> (elbo, grad[5] wrt (ell1, ell2, s1, s2, sigma2), info dict)."""
        self._check_Y(Y)
        b = self._step_bufs           # (host argument blocks of the fit loop's call, allocated once: the call is made ~4000 times a second)
        if b is None:
            th, elbo, grad, info = (C.c_double * 5)(), C.c_double(), (C.c_double * 5)(), Info()
            b = self._step_bufs = (th, elbo, grad, info, C.byref(elbo), C.byref(info), np.frombuffer(grad, dtype=np.float64))
        th = b[0]
        th[0], th[1], th[2], th[3], th[4] = theta
        check(self.lib.vggp_elbo_step(self._h, _ptr(Y), float(yy_total), th, b[4], b[2], b[5], _stream(self.device)))
        return b[1].value, b[6].copy(), self._info(b[3])

    def elbo_step_masked(self, Ym: torch.Tensor, W: torch.Tensor, n_obs: float, yy_obs: float, theta: Sequence[float]):
        """Masked grid: Ym = W*Y and W (0/1 float64) are [n2, n1]; -> (elbo, grad[5], info)."""
        self._check_Y(Ym)
        self._check_Y(W)
        th = (C.c_double * 5)(*[float(t) for t in theta])
        elbo = C.c_double()
        grad = (C.c_double * 5)()
        info = Info()
        check(self.lib.vggp_elbo_step_masked(self._h, _ptr(Ym), _ptr(W), float(n_obs), float(yy_obs), th, C.byref(elbo),
                                             grad, C.byref(info), _stream(self.device)))
        return elbo.value, np.array(list(grad)), self._info(info)

    def elbo_step_masked_iter(self, Ym: torch.Tensor, W: torch.Tensor, n_obs: float, yy_obs: float, theta: Sequence[float],
                              n_probes: int = 16, tol: float = 1e-10, max_iter: int = 100):
        """The masked step without any M x M matrix (PCG + Lanczos quadrature + control-variate trace estimators, fixed probes;
        include/vggp.h): -> (elbo, grad[5], info) with info['rounds'][0] = PCG iterations.  On a multi-rank engine
        (sharded.make_engine): Ym, W are this rank's row slab, n_obs and yy_obs the global values; every rank returns the same bits."""
        self._check_Y(Ym)
        self._check_Y(W)
        th = (C.c_double * 5)(*[float(t) for t in theta])
        elbo = C.c_double()
        grad = (C.c_double * 5)()
        info = Info()
        check(self.lib.vggp_elbo_step_masked_iter(self._h, _ptr(Ym), _ptr(W), float(n_obs), float(yy_obs), th, int(n_probes), float(tol),
                                                  int(max_iter), C.byref(elbo), grad, C.byref(info), _stream(self.device)))
        return elbo.value, np.array(list(grad)), self._info(info)

    def qv_masked_iter(self, W: torch.Tensor, n_obs: float, cells=None, variance: bool = True, tol: float = 1e-10,
                       max_iter: int = 100, block: int = 0):
        """q(v) after elbo_step_masked_iter (W, n_obs: the step's): -> (mean [m1, m2], var [n_cells] or None, info).  cells: flat
        indices i1*m2 + i2 of the cells whose variance is wanted (None: every cell -- ceil(M / block) block PCG solves);
        variance=False: the mean only (no solve).  info['rounds'][0] = most PCG iterations of a block solve, info['sweeps'][0] =
        block solves."""
        self._check_Y(W)
        mean = torch.empty(self.m1, self.m2, dtype=torch.float64, device=self.device)
        info = Info()
        if not variance:
            cp, nc, var = None, 0, None
        elif cells is None:
            cp, nc = None, self.m1 * self.m2
            var = torch.empty(nc, dtype=torch.float64, device=self.device)
        else:
            ca = np.ascontiguousarray(torch.as_tensor(cells).detach().cpu().numpy().reshape(-1), dtype=np.int64)
            cp, nc = ca.ctypes.data_as(C.POINTER(C.c_int64)), len(ca)
            var = torch.empty(nc, dtype=torch.float64, device=self.device) if nc else None
        check(self.lib.vggp_qv_masked_iter(self._h, _ptr(W), float(n_obs), cp, nc, float(tol), int(max_iter), int(block), _ptr(mean),
                                           _ptr(var), C.byref(info), _stream(self.device)))
        return mean, var, self._info(info)

    def posterior_masked_iter(self, x_star: torch.Tensor, W: torch.Tensor, n_obs: float, tol: float = 1e-10, max_iter: int = 100,
                              block: int = 0):
        """posterior(x*) after elbo_step_masked_iter; x_star [ns, 2] -> (mean [ns], var [ns], info)."""
        self._check_Y(W)
        xs = x_star.to(self.device, torch.float64)
        xs1, xs2 = xs[:, 0].contiguous(), xs[:, 1].contiguous()
        ns = xs1.shape[0]
        mean = torch.empty(ns, dtype=torch.float64, device=self.device)
        var = torch.empty_like(mean)
        info = Info()
        check(self.lib.vggp_posterior_masked_iter(self._h, _ptr(W), float(n_obs), _ptr(xs1), _ptr(xs2), ns, float(tol), int(max_iter),
                                                  int(block), _ptr(mean), _ptr(var), C.byref(info), _stream(self.device)))
        return mean, var, self._info(info)

    def elbo_step_scattered(self, y: torch.Tensor, yy: float, theta: Sequence[float]):
        """N scattered points (plan(..., scattered=True) with their coordinate pairs): y [N] float64 GPU tensor, yy = sum y^2;
        -> (elbo, grad[5], info).  qv_masked / posterior_masked / the *_cov_masked read-outs apply afterwards."""
        if not (y.is_cuda and y.dtype == torch.float64 and y.is_contiguous() and y.numel() == self.n1):
            raise TypeError("y must be a contiguous float64 GPU tensor with one value per planned point")
        th = (C.c_double * 5)(*[float(t) for t in theta])
        elbo = C.c_double()
        grad = (C.c_double * 5)()
        info = Info()
        check(self.lib.vggp_elbo_step_scattered(self._h, _ptr(y), float(yy), th, C.byref(elbo), grad, C.byref(info),
                                                _stream(self.device)))
        return elbo.value, np.array(list(grad)), self._info(info)

    def elbo_step_scattered_iter(self, y: torch.Tensor, yy: float, theta: Sequence[float], n_probes: int = 16, tol: float = 1e-10,
                                 max_iter: int = 100):
        """The scattered step without any M x M matrix or m_d^2 x N buffer (PCG on the Khatri-Rao operator, Lanczos quadrature,
        control-variate traces, fixed probes; include/vggp.h): any M with m_d <= 256.  -> (elbo, grad[5], info) with
        info['rounds'][0] = PCG iterations.  Read-outs: qv_scattered_iter, posterior_scattered_iter (means only), their
        *_var_scattered_iter forms (with point-wise variances), readout_scattered_iter (the gridded q(v): mean and variance).
        On a multi-rank engine (sharded.make_engine): y holds this rank's points (plan(..., n_total=N over all ranks)), yy is global."""
        if not (y.is_cuda and y.dtype == torch.float64 and y.is_contiguous() and y.numel() == self.n1):
            raise TypeError("y must be a contiguous float64 GPU tensor with one value per planned point")
        th = (C.c_double * 5)(*[float(t) for t in theta])
        elbo = C.c_double()
        grad = (C.c_double * 5)()
        info = Info()
        check(self.lib.vggp_elbo_step_scattered_iter(self._h, _ptr(y), float(yy), th, int(n_probes), float(tol), int(max_iter),
                                                     C.byref(elbo), grad, C.byref(info), _stream(self.device)))
        return elbo.value, np.array(list(grad)), self._info(info)

    def qv_scattered_iter(self) -> torch.Tensor:
        """q(v) mean [m1, m2] after elbo_step_scattered_iter (no solve; qv_var_scattered_iter adds the variances)."""
        mean = torch.empty(self.m1, self.m2, dtype=torch.float64, device=self.device)
        check(self.lib.vggp_qv_scattered_iter(self._h, _ptr(mean), _stream(self.device)))
        return mean

    def posterior_scattered_iter(self, x_star: torch.Tensor) -> torch.Tensor:
        """posterior(x*) mean after elbo_step_scattered_iter; x_star [ns, 2] -> mean [ns]."""
        xs = x_star.to(self.device, torch.float64)
        xs1, xs2 = xs[:, 0].contiguous(), xs[:, 1].contiguous()
        ns = xs1.shape[0]
        mean = torch.empty(ns, dtype=torch.float64, device=self.device)
        check(self.lib.vggp_posterior_scattered_iter(self._h, _ptr(xs1), _ptr(xs2), ns, _ptr(mean), _stream(self.device)))
        return mean

    def qv_var_scattered_iter(self, cells=None, variance: bool = True, tol: float = 1e-10, max_iter: int = 100, block: int = 0):
        """q(v) after elbo_step_scattered_iter: -> (mean [m1, m2], var [n_cells] or None, info).  cells, variance, info as
        qv_masked_iter: None means every cell (ceil(M / block) block PCG solves), variance=False the mean only (no solve)."""
        mean = torch.empty(self.m1, self.m2, dtype=torch.float64, device=self.device)
        info = Info()
        if not variance:
            cp, nc, var = None, 0, None
        elif cells is None:
            cp, nc = None, self.m1 * self.m2
            var = torch.empty(nc, dtype=torch.float64, device=self.device)
        else:
            ca = np.ascontiguousarray(torch.as_tensor(cells).detach().cpu().numpy().reshape(-1), dtype=np.int64)
            cp, nc = ca.ctypes.data_as(C.POINTER(C.c_int64)), len(ca)
            var = torch.empty(nc, dtype=torch.float64, device=self.device) if nc else None
        check(self.lib.vggp_qv_var_scattered_iter(self._h, cp, nc, float(tol), int(max_iter), int(block), _ptr(mean), _ptr(var),
                                                  C.byref(info), _stream(self.device)))
        return mean, var, self._info(info)

    def posterior_var_scattered_iter(self, x_star: torch.Tensor, tol: float = 1e-10, max_iter: int = 100, block: int = 0):
        """posterior(x*) after elbo_step_scattered_iter; x_star [ns, 2] -> (mean [ns], var [ns], info): ceil(ns / block) solves."""
        xs = x_star.to(self.device, torch.float64)
        xs1, xs2 = xs[:, 0].contiguous(), xs[:, 1].contiguous()
        ns = xs1.shape[0]
        mean = torch.empty(ns, dtype=torch.float64, device=self.device)
        var = torch.empty_like(mean)
        info = Info()
        check(self.lib.vggp_posterior_var_scattered_iter(self._h, _ptr(xs1), _ptr(xs2), ns, float(tol), int(max_iter), int(block),
                                                         _ptr(mean), _ptr(var), C.byref(info), _stream(self.device)))
        return mean, var, self._info(info)

    def kr_field(self, L: torch.Tensor, R: torch.Tensor, V: torch.Tensor, cols_per_wg: int = 4) -> torch.Tensor:
        """Khatri-Rao field kernel: L [m1, N], R [m2, N], V [m1, nb, m2] -> F [nb, N], F[c, k] = l_k^T V_c r_k.  cols_per_wg: 4 (the
        step's kernel) or 2 (the read-outs' instantiation; the same bits)."""
        m1, N = L.shape
        m2, nb = R.shape[0], V.shape[1]
        if R.shape[1] != N or tuple(V.shape) != (m1, nb, m2):
            raise ValueError("kr_field: L [m1, N], R [m2, N], V [m1, nb, m2]")
        if cols_per_wg not in (2, 4):
            raise ValueError("kr_field: cols_per_wg is 2 or 4")
        fn = self.lib.vggp_kr_field2 if cols_per_wg == 2 else self.lib.vggp_kr_field
        F = torch.empty(nb, N, dtype=torch.float64, device=self.device)
        check(fn(self._h, _ptr(L), _ptr(R), _ptr(V), m1, m2, N, nb, _ptr(F), _stream(self.device)))
        return F

    def kr_back(self, L: torch.Tensor, R: torch.Tensor, F: torch.Tensor) -> torch.Tensor:
        """Khatri-Rao back kernel: L [m1, N], R [m2, N], F [nb, N] -> out [m1, nb, m2] = sum_k F[c, k] l_k r_k^T."""
        m1, N = L.shape
        m2, nb = R.shape[0], F.shape[0]
        if R.shape[1] != N or F.shape[1] != N:
            raise ValueError("kr_back: L [m1, N], R [m2, N], F [nb, N]")
        out = torch.empty(m1, nb, m2, dtype=torch.float64, device=self.device)
        check(self.lib.vggp_kr_back(self._h, _ptr(L), _ptr(R), _ptr(F), m1, m2, N, nb, _ptr(out), _stream(self.device)))
        return out

    def kr_sqgram(self, P1: torch.Tensor, P2: torch.Tensor) -> torch.Tensor:
        """Squared Gram kernel of the literal gridded read-out: P1 [mv1, N], P2 [mv2, N] -> out [mv1, mv2] = (P1 o P1)(P2 o P2)^T."""
        mv1, N = P1.shape
        mv2 = P2.shape[0]
        if P2.shape[1] != N:
            raise ValueError("kr_sqgram: P1 [mv1, N], P2 [mv2, N]")
        for t in (P1, P2):
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
                raise TypeError("kr_sqgram operands must be contiguous float64 GPU tensors")
        out = torch.empty(mv1, mv2, dtype=torch.float64, device=self.device)
        check(self.lib.vggp_kr_sqgram(self._h, _ptr(P1), _ptr(P2), mv1, mv2, N, _ptr(out), _stream(self.device)))
        return out

    def _readout_iter(self, fn, lead, C1, C2, kd1, kd2, literal, cells, variance, tol, max_iter, block):
        C1, C2 = C1.to(self.device, torch.float64).contiguous(), C2.to(self.device, torch.float64).contiguous()
        kd1, kd2 = kd1.to(self.device, torch.float64).contiguous(), kd2.to(self.device, torch.float64).contiguous()
        if C1.shape[1] != self.m1 or C2.shape[1] != self.m2 or kd1.numel() != C1.shape[0] or kd2.numel() != C2.shape[0]:
            raise ValueError("C_d must be [mv_d, m_d] and kd_d [mv_d]")
        mv1, mv2 = C1.shape[0], C2.shape[0]
        mean = torch.empty(mv1, mv2, dtype=torch.float64, device=self.device)
        info = Info()
        if not variance:
            cp, nc, var = None, 0, None
        elif cells is None:
            cp, nc = None, mv1 * mv2
            var = torch.empty(nc, dtype=torch.float64, device=self.device)
        else:
            ca = np.ascontiguousarray(torch.as_tensor(cells).detach().cpu().numpy().reshape(-1), dtype=np.int64)
            cp, nc = ca.ctypes.data_as(C.POINTER(C.c_int64)), len(ca)
            var = torch.empty(nc, dtype=torch.float64, device=self.device) if nc else None
        check(fn(self._h, *lead, _ptr(C1), mv1, _ptr(C2), mv2, _ptr(kd1), _ptr(kd2), cp, nc, float(tol), int(max_iter), int(block),
                 _ptr(mean), _ptr(var), 1 if literal else 0, C.byref(info), _stream(self.device)))
        return mean, var, self._info(info)

    def readout_masked_iter(self, C1: torch.Tensor, C2: torch.Tensor, kd1: torch.Tensor, kd2: torch.Tensor, W: torch.Tensor,
                            n_obs: float, literal: bool = True, cells=None, variance: bool = True, tol: float = 1e-10,
                            max_iter: int = 100, block: int = 0):
        """Gridded read-out q(v) after elbo_step_masked_iter (W, n_obs: the step's; C_d, kd_d as readout): -> (mean [mv1, mv2],
        var [n_cells] or None, info).  cells: flat indices a*mv2 + b (None: every cell); variance=False: the mean only.
        literal=True: the reference's variance, a Gram product over the data (no solve, info['sweeps'][0] == 0); literal=False: the
        conditional variance, ceil(n_cells / block) block PCG solves."""
        self._check_Y(W)
        return self._readout_iter(self.lib.vggp_readout_masked_iter, (_ptr(W), float(n_obs)), C1, C2, kd1, kd2, literal, cells, variance,
                                  tol, max_iter, block)

    def readout_scattered_iter(self, C1: torch.Tensor, C2: torch.Tensor, kd1: torch.Tensor, kd2: torch.Tensor, literal: bool = True,
                               cells=None, variance: bool = True, tol: float = 1e-10, max_iter: int = 100, block: int = 0):
        """Gridded read-out q(v) after elbo_step_scattered_iter; arguments and result as readout_masked_iter."""
        return self._readout_iter(self.lib.vggp_readout_scattered_iter, (), C1, C2, kd1, kd2, literal, cells, variance, tol, max_iter,
                                  block)

    def qv_masked(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> mean, var [m1, m2]; on a paired plan q(u) over the M inducing points, [M] each."""
        shape = (self.m1,) if self.paired else (self.m1, self.m2)
        mean = torch.empty(*shape, dtype=torch.float64, device=self.device)
        var = torch.empty_like(mean)
        check(self.lib.vggp_qv_masked(self._h, _ptr(mean), _ptr(var), _stream(self.device)))
        return mean, var

    def elbo_partials(self, Y: torch.Tensor, theta: Sequence[float], payload: Optional[torch.Tensor] = None):
        self._check_Y(Y)
        if payload is None:
            payload = torch.empty(self.payload_len, dtype=torch.float64, device=self.device)
        th = (C.c_double * 5)(*[float(t) for t in theta])
        check(self.lib.vggp_elbo_partials(self._h, _ptr(Y), th, _ptr(payload), _stream(self.device)))
        return payload

    def elbo_finish(self, payload: torch.Tensor, yy_total: float, theta: Sequence[float]):
        th = (C.c_double * 5)(*[float(t) for t in theta])
        elbo = C.c_double()
        grad = (C.c_double * 5)()
        info = Info()
        check(self.lib.vggp_elbo_finish(self._h, _ptr(payload), float(yy_total), th, C.byref(elbo), grad,
                                        C.byref(info), _stream(self.device)))
        return elbo.value, np.array(list(grad)), self._info(info)

    @staticmethod
    def _info(i: Info) -> dict:
        return dict(jitter=(i.jitter1, i.jitter2), sweeps=(i.sweeps1, i.sweeps2), rounds=(i.rounds1, i.rounds2),
                    status=i.status, polished=(bool(i.polished & 1), bool(i.polished & 2)))

    def qv(self) -> Tuple[torch.Tensor, torch.Tensor]:
        mean = torch.empty(self.m1, self.m2, dtype=torch.float64, device=self.device)
        var = torch.empty_like(mean)
        check(self.lib.vggp_qv(self._h, _ptr(mean), _ptr(var), _stream(self.device)))
        return mean, var

    def qv_cov(self) -> torch.Tensor:
        M = self.m1 * self.m2
        cov = torch.empty(M, M, dtype=torch.float64, device=self.device)
        check(self.lib.vggp_qv_cov(self._h, _ptr(cov), _stream(self.device)))
        return cov

    # -- joint samples of q(v) (include/vggp.h: vggp_qv_sample*; no M x M matrix anywhere) ------------------------------
    def normal_fill(self, seed: int, stream_id: int, first_idx: int, n: int) -> torch.Tensor:
        """Elements first_idx .. first_idx + n of the counter-based normal sequence (seed, stream_id) (vggp_normal_fill) -> [n]."""
        out = torch.empty(int(n), dtype=torch.float64, device=self.device)
        check(self.lib.vggp_normal_fill(self._h, int(seed) & (2**64 - 1), int(stream_id), int(first_idx), int(n), _ptr(out) if n else None,
                                        _stream(self.device)))
        return out

    def _sample_noise(self, n_samples, eps_u, eps_obs, obs_shape):
        S = int(n_samples)
        if eps_u is not None and tuple(eps_u.shape) != (S, self.m1, self.m2):
            raise ValueError(f"eps_u must be [n_samples={S}, m1={self.m1}, m2={self.m2}], got {tuple(eps_u.shape)}")
        if eps_obs is not None and tuple(eps_obs.shape) != (S,) + obs_shape:
            raise ValueError(f"eps_obs must be {(S,) + obs_shape}, got {tuple(eps_obs.shape)}")
        return S, torch.empty(max(S, 0), self.m1, self.m2, dtype=torch.float64, device=self.device)

    def qv_sample(self, n_samples: int, seed: int = 0, first: int = 0, eps_u: Optional[torch.Tensor] = None) -> torch.Tensor:
        """n_samples joint samples of q(v) after elbo_step (full grid) -> [n_samples, m1, m2].  eps_u [n_samples, m1, m2]: the
        caller's standard normals; None: generated on the device, sample s = first + local of `seed` (the same numbers in any call)."""
        S, out = self._sample_noise(n_samples, eps_u, None, ())
        check(self.lib.vggp_qv_sample(self._h, S, int(seed) & (2**64 - 1), int(first), _ptr(eps_u), _ptr(out) if S > 0 else None,
                                      _stream(self.device)))
        return out

    def qv_sample_masked_iter(self, W: torch.Tensor, n_obs: float, n_samples: int, seed: int = 0, first: int = 0,
                              eps_u: Optional[torch.Tensor] = None, eps_obs: Optional[torch.Tensor] = None, tol: float = 1e-10,
                              max_iter: int = 100, block: int = 0):
        """Joint samples of q(v) after elbo_step_masked_iter (W, n_obs: the step's) -> ([n_samples, m1, m2], info): one block PCG
        solve per `block` <= 64 samples.  eps_u [n_samples, m1, m2] and eps_obs [n_samples, n2, n1]: both given or both None
        (generated from seed / first as qv_sample).  info['rounds'][0] = most PCG iterations, info['sweeps'][0] = block solves."""
        self._check_Y(W)
        S, out = self._sample_noise(n_samples, eps_u, eps_obs, (self.n2, self.n1))
        info = Info()
        check(self.lib.vggp_qv_sample_masked_iter(self._h, _ptr(W), float(n_obs), S, int(seed) & (2**64 - 1), int(first), _ptr(eps_u),
                                                  _ptr(eps_obs), float(tol), int(max_iter), int(block), _ptr(out) if S > 0 else None,
                                                  C.byref(info), _stream(self.device)))
        return out, self._info(info)

    def qv_sample_scattered_iter(self, n_samples: int, seed: int = 0, first: int = 0, eps_u: Optional[torch.Tensor] = None,
                                 eps_obs: Optional[torch.Tensor] = None, tol: float = 1e-10, max_iter: int = 100, block: int = 0):
        """Joint samples of q(v) after elbo_step_scattered_iter -> ([n_samples, m1, m2], info); eps_obs [n_samples, N]; otherwise as
        qv_sample_masked_iter."""
        S, out = self._sample_noise(n_samples, eps_u, eps_obs, (self.n1,))
        info = Info()
        check(self.lib.vggp_qv_sample_scattered_iter(self._h, S, int(seed) & (2**64 - 1), int(first), _ptr(eps_u), _ptr(eps_obs), float(tol),
                                                     int(max_iter), int(block), _ptr(out) if S > 0 else None, C.byref(info),
                                                     _stream(self.device)))
        return out, self._info(info)

    def qv_sample_masked(self, n_samples: int, seed: int = 0, first: int = 0, eps_u: Optional[torch.Tensor] = None, block: int = 0):
        """Joint samples of q(v) after elbo_step_masked / elbo_step_scattered (the dense states) -> ([n_samples, m1, m2], info): the
        coefficient draw X = Xg^T E from the inverse factor the step keeps, one launch per `block` <= 64 samples, nothing solved
        (info['rounds'] and info['sweeps'] are 0).  eps_u [n_samples, m1, m2] or None (generated from seed / first as qv_sample)."""
        S, out = self._sample_noise(n_samples, eps_u, None, ())
        info = Info()
        check(self.lib.vggp_qv_sample_masked(self._h, S, int(seed) & (2**64 - 1), int(first), _ptr(eps_u), int(block),
                                             _ptr(out) if S > 0 else None, C.byref(info), _stream(self.device)))
        return out, self._info(info)

    def tri_t_apply(self, Xl: torch.Tensor, E: torch.Tensor, cn: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The dense samplers' product on its own (vggp_tri_t_apply): Xl [M, M] lower triangular (nothing above its diagonal is read),
        E [m1, nbc, m2] with M = m1 m2 -> out [m1, nbc, m2], out(u, c) = sum_{k >= u} Xl[k, u] E(k, c) for c < cn (None: nbc), zeros
        for c >= cn.  Asynchronous on torch's current stream."""
        m1, nbc, m2 = E.shape
        if tuple(Xl.shape) != (m1 * m2, m1 * m2):
            raise ValueError("tri_t_apply: Xl [m1 m2, m1 m2], E [m1, nbc, m2]")
        if out is None:
            out = torch.empty_like(E)
        elif tuple(out.shape) != tuple(E.shape):
            raise ValueError("tri_t_apply: out must be [m1, nbc, m2]")
        check(self.lib.vggp_tri_t_apply(self._h, _ptr(Xl), m1, m2, _ptr(E), nbc, nbc if cn is None else int(cn), _ptr(out),
                                        _stream(self.device)))
        return out

    def readout(self, C1: torch.Tensor, C2: torch.Tensor, kd1: torch.Tensor, kd2: torch.Tensor, literal: bool = True,
                masked: bool = False):
        """Gridded read-out q(v) of B0 cell features from the inducing posterior of the last step (include/vggp.h):
        C_d [mv_d, m_d] unit-outputscale cross-covariances, kd_d [mv_d] unit diagonals of Kvv_d -> mean, var [mv1, mv2]."""
        C1, C2 = C1.to(self.device, torch.float64).contiguous(), C2.to(self.device, torch.float64).contiguous()
        kd1, kd2 = kd1.to(self.device, torch.float64).contiguous(), kd2.to(self.device, torch.float64).contiguous()
        if C1.shape[1] != self.m1 or C2.shape[1] != self.m2:
            raise ValueError("C_d must be [mv_d, m_d]")
        mean = torch.empty(C1.shape[0], C2.shape[0], dtype=torch.float64, device=self.device)
        var = torch.empty_like(mean)
        fn = self.lib.vggp_readout_masked if masked else self.lib.vggp_readout      # masked: state of a masked / scattered step
        check(fn(self._h, _ptr(C1), C1.shape[0], _ptr(C2), C2.shape[0], _ptr(kd1), _ptr(kd2), _ptr(mean),
                 _ptr(var), 1 if literal else 0, _stream(self.device)))
        return mean, var

    def posterior_cov(self, x_star: torch.Tensor, masked: bool = False) -> torch.Tensor:
        """Dense covariance of posterior(x*) (kronecker_structure.py:223-229), x_star [ns, 2] -> [ns, ns]."""
        xs = x_star.to(self.device, torch.float64)
        if xs.dim() == 1:
            xs = torch.stack([xs, torch.zeros_like(xs)], dim=1)
        xs1, xs2 = xs[:, 0].contiguous(), xs[:, 1].contiguous()
        ns = xs1.shape[0]
        cov = torch.empty(ns, ns, dtype=torch.float64, device=self.device)
        fn = self.lib.vggp_posterior_cov_masked if masked else self.lib.vggp_posterior_cov
        check(fn(self._h, _ptr(xs1), _ptr(xs2), ns, _ptr(cov), _stream(self.device)))
        return cov

    def set_inducing(self, dim: int, z) -> None:
        """Move the inducing points of a 'points' basis (dimension 0 or 1) without re-planning: graphs and warm start stay."""
        zz = _dvec(z)
        with torch.cuda.device(self.device):
            check(self.lib.vggp_set_inducing(self._h, int(dim), zz.ctypes.data, len(zz)))

    def zgrad(self, Y: torch.Tensor):
        """d ELBO / d z of the last elbo_step(Y, ...) for the inducing coordinates of both dimensions ("points" bases; zeros
        otherwise) -> (g1 [m1], g2 [m2]) device tensors."""
        g1 = torch.empty(self.m1, dtype=torch.float64, device=self.device)
        g2 = torch.empty(self.m2, dtype=torch.float64, device=self.device)
        check(self.lib.vggp_zgrad(self._h, _ptr(Y), _ptr(g1), _ptr(g2), _stream(self.device)))
        return g1, g2

    def zgrad_scattered(self, y: torch.Tensor):
        """d ELBO / d z of the last elbo_step_scattered(y, ...) -> (g1 [m1], g2 [m2]) device tensors."""
        g1 = torch.empty(self.m1, dtype=torch.float64, device=self.device)
        g2 = torch.empty(self.m2, dtype=torch.float64, device=self.device)
        check(self.lib.vggp_zgrad_scattered(self._h, _ptr(y), _ptr(g1), _ptr(g2), _stream(self.device)))
        return g1, g2

    def qv_cov_masked(self) -> torch.Tensor:
        M = self.m1 if self.paired else self.m1 * self.m2
        cov = torch.empty(M, M, dtype=torch.float64, device=self.device)
        check(self.lib.vggp_qv_cov_masked(self._h, _ptr(cov), _stream(self.device)))
        return cov

    def posterior_masked(self, x_star: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """posterior(x*) of the last masked step; x_star [ns, 2] -> mean[ns], var[ns]."""
        return self.posterior(x_star, _fn="vggp_posterior_masked")

    def posterior(self, x_star: torch.Tensor, _fn: str = "vggp_posterior") -> Tuple[torch.Tensor, torch.Tensor]:
        """x_star [ns, 2] (or [ns] with a trivial second dimension) -> mean[ns], var[ns]."""
        xs = x_star.to(self.device, torch.float64)
        if xs.dim() == 1:
            xs = torch.stack([xs, torch.zeros_like(xs)], dim=1)
        xs1, xs2 = xs[:, 0].contiguous(), xs[:, 1].contiguous()
        ns = xs1.shape[0]
        mean = torch.empty(ns, dtype=torch.float64, device=self.device)
        var = torch.empty_like(mean)
        check(getattr(self.lib, _fn)(self._h, _ptr(xs1), _ptr(xs2), ns, _ptr(mean), _ptr(var), _stream(self.device)))
        return mean, var

    def posterior_raster(self, g1: torch.Tensor, g2: torch.Tensor, want_var: bool = True):
        """posterior(x*) on the cartesian grid of two coordinate axes (vggp_posterior_raster): g1 [p1], g2 [p2] -> (mean [p1, p2],
        var [p1, p2] or None), element (a, b) at the point (g1[a], g2[b]).  Reads the last finished step, whichever kind; the masked,
        scattered and iterative states give the mean only (want_var=True raises there: use their point-wise read-outs, or
        posterior_raster_var_masked after the dense masked / scattered steps)."""
        a1 = torch.as_tensor(g1).to(self.device, torch.float64).reshape(-1).contiguous()
        a2 = torch.as_tensor(g2).to(self.device, torch.float64).reshape(-1).contiguous()
        p1, p2 = a1.numel(), a2.numel()
        mean = torch.empty(p1, p2, dtype=torch.float64, device=self.device)
        var = torch.empty_like(mean) if want_var else None
        check(self.lib.vggp_posterior_raster(self._h, _ptr(a1), p1, _ptr(a2), p2, _ptr(mean), _ptr(var), _stream(self.device)))
        return mean, var

    def raster_contract(self, T1: torch.Tensor, U: torch.Tensor, Uv: Optional[torch.Tensor] = None, c0: float = 0.0, c1: float = 1.0,
                        out: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]] = None):
        """The raster kernel on its own (vggp_raster_contract): T1 [q, P1], U [q, P2], Uv [q, P2] or None -> (mean [P1, P2] = T1^T U,
        var [P1, P2] = c0 + c1 (T1 o T1)^T Uv or None).  out: (mean, var) views to write into instead of fresh tensors.  Operands and
        outputs must be contiguous float64 GPU tensors (TypeError otherwise: the kernel receives their pointers)."""
        q, P1 = T1.shape
        P2 = U.shape[1]
        if U.shape[0] != q or (Uv is not None and tuple(Uv.shape) != (q, P2)):
            raise ValueError("raster_contract: T1 [q, P1], U [q, P2], Uv [q, P2]")
        if out is None:
            mean = torch.empty(P1, P2, dtype=torch.float64, device=self.device)
            var = torch.empty_like(mean) if Uv is not None else None
        else:
            mean, var = out
            if tuple(mean.shape) != (P1, P2) or (var is not None and tuple(var.shape) != (P1, P2)):
                raise ValueError("raster_contract: out tensors must be [P1, P2]")
        check(self.lib.vggp_raster_contract(self._h, _ptr(T1), _ptr(U), _ptr(Uv), q, P1, P2, float(c0), float(c1), _ptr(mean), _ptr(var),
                                            _stream(self.device)))
        return mean, var

    def posterior_raster_var_masked(self, g1: torch.Tensor, g2: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Mean and variance of posterior(x*) on the raster g1 x g2 after elbo_step_masked / elbo_step_scattered
        (vggp_posterior_raster_var_masked) -> (mean [p1, p2], var [p1, p2]).  The mean is posterior_raster's, bit for bit; the variance
        is the separable contraction against the state's dense Sinv (kron_quadform), not the point-wise route."""
        a1 = torch.as_tensor(g1).to(self.device, torch.float64).reshape(-1).contiguous()
        a2 = torch.as_tensor(g2).to(self.device, torch.float64).reshape(-1).contiguous()
        p1, p2 = a1.numel(), a2.numel()
        mean = torch.empty(p1, p2, dtype=torch.float64, device=self.device)
        var = torch.empty_like(mean)
        check(self.lib.vggp_posterior_raster_var_masked(self._h, _ptr(a1), p1, _ptr(a2), p2, _ptr(mean), _ptr(var), _stream(self.device)))
        return mean, var

    def kron_quadform(self, S: torch.Tensor, U1: torch.Tensor, U2: torch.Tensor, n1: Optional[torch.Tensor] = None,
                      n2: Optional[torch.Tensor] = None, kd: float = 0.0, scale: float = 1.0,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The raster variance's contraction on its own (vggp_kron_quadform): S [M, M] (M = m1 m2, any matrix), U1 [m1, P1], U2 [m2, P2],
        n1 [P1], n2 [P2] (both or neither) -> out [P1, P2] = scale (kd - n1[a] n2[b] + (u1_a (x) u2_b)^T S (u1_a (x) u2_b)).  Operands
        and `out` must be contiguous float64 GPU tensors (TypeError otherwise: the kernel receives their pointers)."""
        m1, P1 = U1.shape
        m2, P2 = U2.shape
        if tuple(S.shape) != (m1 * m2, m1 * m2) or (n1 is None) != (n2 is None) or \
                (n1 is not None and (tuple(n1.shape) != (P1,) or tuple(n2.shape) != (P2,))):
            raise ValueError("kron_quadform: S [m1 m2, m1 m2], U1 [m1, P1], U2 [m2, P2], n1 [P1] and n2 [P2] (both or neither)")
        if out is None:
            out = torch.empty(P1, P2, dtype=torch.float64, device=self.device)
        elif tuple(out.shape) != (P1, P2):
            raise ValueError("kron_quadform: out must be [P1, P2]")
        check(self.lib.vggp_kron_quadform(self._h, _ptr(S), m1, m2, _ptr(U1), P1, _ptr(U2), P2, _ptr(n1), _ptr(n2), float(kd), float(scale),
                                          _ptr(out), _stream(self.device)))
        return out

    # -- joint samples of posterior(x*) on a raster (include/vggp.h: vggp_posterior_raster_sample*; no p1 p2 x p1 p2 matrix) ------
    def _raster_sample_args(self, g1, g2, n_samples, eps_u, eps_obs, obs_shape, eps_g, eps_h):
        a1 = torch.as_tensor(g1).to(self.device, torch.float64).reshape(-1).contiguous()
        a2 = torch.as_tensor(g2).to(self.device, torch.float64).reshape(-1).contiguous()
        p1, p2, S = a1.numel(), a2.numel(), int(n_samples)
        if eps_u is not None and tuple(eps_u.shape) != (S, self.m1, self.m2):
            raise ValueError(f"eps_u must be [n_samples={S}, m1={self.m1}, m2={self.m2}], got {tuple(eps_u.shape)}")
        if eps_obs is not None and tuple(eps_obs.shape) != (S,) + obs_shape:
            raise ValueError(f"eps_obs must be {(S,) + obs_shape}, got {tuple(eps_obs.shape)}")
        if eps_g is not None and tuple(eps_g.shape) != (S, p1, p2):
            raise ValueError(f"eps_g must be [n_samples={S}, p1={p1}, p2={p2}], got {tuple(eps_g.shape)}")
        if eps_h is not None and tuple(eps_h.shape) != (S, self.m1, p2):
            raise ValueError(f"eps_h must be [n_samples={S}, m1={self.m1}, p2={p2}], got {tuple(eps_h.shape)}")
        return a1, a2, p1, p2, S, torch.empty(max(S, 0), p1, p2, dtype=torch.float64, device=self.device)

    def posterior_raster_sample(self, g1, g2, n_samples: int, seed: int = 0, first: int = 0, eps_u: Optional[torch.Tensor] = None,
                                eps_g: Optional[torch.Tensor] = None, eps_h: Optional[torch.Tensor] = None):
        """n_samples joint samples of posterior(x*) on the raster g1 x g2 after elbo_step (full grid) -> ([n_samples, p1, p2], info).
        eps_u [n_samples, m1, m2], eps_g [n_samples, p1, p2], eps_h [n_samples, m1, p2]: the caller's standard normals, all or none;
        none: generated on the device, sample s = first + local of `seed` (sharing E_s with qv_sample).  info['jitter']: the levels
        the roots took on top of the 1e-8 nugget."""
        a1, a2, p1, p2, S, out = self._raster_sample_args(g1, g2, n_samples, eps_u, None, (), eps_g, eps_h)
        info = Info()
        check(self.lib.vggp_posterior_raster_sample(self._h, _ptr(a1), p1, _ptr(a2), p2, S, int(seed) & (2**64 - 1), int(first), _ptr(eps_u),
                                                    _ptr(eps_g), _ptr(eps_h), _ptr(out) if S > 0 else None, C.byref(info),
                                                    _stream(self.device)))
        return out, self._info(info)

    def posterior_raster_sample_masked_iter(self, g1, g2, W: torch.Tensor, n_obs: float, n_samples: int, seed: int = 0, first: int = 0,
                                            eps_u: Optional[torch.Tensor] = None, eps_obs: Optional[torch.Tensor] = None,
                                            eps_g: Optional[torch.Tensor] = None, eps_h: Optional[torch.Tensor] = None, tol: float = 1e-10,
                                            max_iter: int = 100, block: int = 0):
        """As posterior_raster_sample after elbo_step_masked_iter (W, n_obs: the step's); eps_obs [n_samples, n2, n1]; one block PCG
        solve per block of samples (info['rounds'][0] = most PCG iterations, info['sweeps'][0] = block solves)."""
        self._check_Y(W)
        a1, a2, p1, p2, S, out = self._raster_sample_args(g1, g2, n_samples, eps_u, eps_obs, (self.n2, self.n1), eps_g, eps_h)
        info = Info()
        check(self.lib.vggp_posterior_raster_sample_masked_iter(self._h, _ptr(a1), p1, _ptr(a2), p2, _ptr(W), float(n_obs), S,
                                                                int(seed) & (2**64 - 1), int(first), _ptr(eps_u), _ptr(eps_obs), _ptr(eps_g),
                                                                _ptr(eps_h), float(tol), int(max_iter), int(block),
                                                                _ptr(out) if S > 0 else None, C.byref(info), _stream(self.device)))
        return out, self._info(info)

    def posterior_raster_sample_scattered_iter(self, g1, g2, n_samples: int, seed: int = 0, first: int = 0,
                                               eps_u: Optional[torch.Tensor] = None, eps_obs: Optional[torch.Tensor] = None,
                                               eps_g: Optional[torch.Tensor] = None, eps_h: Optional[torch.Tensor] = None,
                                               tol: float = 1e-10, max_iter: int = 100, block: int = 0):
        """As posterior_raster_sample_masked_iter after elbo_step_scattered_iter; eps_obs [n_samples, N]."""
        a1, a2, p1, p2, S, out = self._raster_sample_args(g1, g2, n_samples, eps_u, eps_obs, (self.n1,), eps_g, eps_h)
        info = Info()
        check(self.lib.vggp_posterior_raster_sample_scattered_iter(self._h, _ptr(a1), p1, _ptr(a2), p2, S, int(seed) & (2**64 - 1), int(first),
                                                                   _ptr(eps_u), _ptr(eps_obs), _ptr(eps_g), _ptr(eps_h), float(tol),
                                                                   int(max_iter), int(block), _ptr(out) if S > 0 else None,
                                                                   C.byref(info), _stream(self.device)))
        return out, self._info(info)

    def posterior_raster_sample_masked(self, g1, g2, n_samples: int, seed: int = 0, first: int = 0, eps_u: Optional[torch.Tensor] = None,
                                       eps_g: Optional[torch.Tensor] = None, eps_h: Optional[torch.Tensor] = None, block: int = 0):
        """As posterior_raster_sample after elbo_step_masked / elbo_step_scattered (the dense states): the coefficient draw of
        qv_sample_masked (sample s of a seed shares its E_s), nothing solved."""
        a1, a2, p1, p2, S, out = self._raster_sample_args(g1, g2, n_samples, eps_u, None, (), eps_g, eps_h)
        info = Info()
        check(self.lib.vggp_posterior_raster_sample_masked(self._h, _ptr(a1), p1, _ptr(a2), p2, S, int(seed) & (2**64 - 1), int(first),
                                                           _ptr(eps_u), _ptr(eps_g), _ptr(eps_h), int(block),
                                                           _ptr(out) if S > 0 else None, C.byref(info), _stream(self.device)))
        return out, self._info(info)

    def raster_sample_contract(self, B1: torch.Tensor, Wt: torch.Tensor, C1: torch.Tensor, Tt: torch.Tensor, c: float = 1.0,
                               mean: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The raster samplers' kernel on its own (vggp_raster_sample_contract): B1 [q, P1], Wt [S, q, P2], C1 [P1, P1] lower triangular
        (nothing above its diagonal is read), Tt [S, P1, P2], mean [P1, P2] or None -> out [S, P1, P2] = mean + B1^T Wt[s] + c C1 Tt[s]."""
        q, P1 = B1.shape
        S, P2 = Wt.shape[0], Wt.shape[2]
        if tuple(Wt.shape) != (S, q, P2) or tuple(C1.shape) != (P1, P1) or tuple(Tt.shape) != (S, P1, P2) or \
                (mean is not None and tuple(mean.shape) != (P1, P2)):
            raise ValueError("raster_sample_contract: B1 [q, P1], Wt [S, q, P2], C1 [P1, P1], Tt [S, P1, P2], mean [P1, P2]")
        if out is None:
            out = torch.empty(S, P1, P2, dtype=torch.float64, device=self.device)
        elif tuple(out.shape) != (S, P1, P2):
            raise ValueError("raster_sample_contract: out must be [S, P1, P2]")
        check(self.lib.vggp_raster_sample_contract(self._h, _ptr(B1), _ptr(Wt), _ptr(C1), _ptr(Tt), S, q, P1, P2, float(c), _ptr(mean),
                                                   _ptr(out), _stream(self.device)))
        return out

    # -- exact GP (dense N x N, N <= 16384; a workspace of its own beside the planned model) --------------
    def exact_plan(self, kind1: str, kind2: str, x1, x2) -> None:
        """Exact GP on the N points (x1[k], x2[k]) with kernel_1 * kernel_2 of the given kinds (vggp_exact_plan).  Independent of
        plan() / plan_paired(): neither disturbs the other's state."""
        x1, x2 = _dvec(x1), _dvec(x2)
        if len(x1) != len(x2):
            raise ValueError("exact plan: x1 and x2 must hold one coordinate pair per point")
        with torch.cuda.device(self.device):
            check(self.lib.vggp_exact_plan(self._h, KIND[kind1], KIND[kind2], x1.ctypes.data, x2.ctypes.data, len(x1)))
        self.exact_n = len(x1)
        self.exact_token += 1

    def exact_step(self, y: torch.Tensor, theta: Sequence[float]):
        """-> (marginal log likelihood, grad[5] wrt (ell1, ell2, s1, s2, sigma2), info dict); y [N] float64 GPU tensor."""
        if not (y.is_cuda and y.dtype == torch.float64 and y.is_contiguous() and y.numel() == self.exact_n):
            raise TypeError("y must be a contiguous float64 GPU tensor with one value per planned point")
        th = (C.c_double * 5)(*[float(t) for t in theta])
        mll = C.c_double()
        grad = (C.c_double * 5)()
        info = Info()
        check(self.lib.vggp_exact_step(self._h, _ptr(y), th, C.byref(mll), grad, C.byref(info), _stream(self.device)))
        return mll.value, np.array(list(grad)), self._info(info)

    def exact_posterior(self, x_star: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """posterior(x*) of the last exact step; x_star [ns, 2] -> mean[ns], var[ns]."""
        return self.posterior(x_star, _fn="vggp_exact_posterior")

    def exact_posterior_cov(self, x_star: torch.Tensor) -> torch.Tensor:
        """Dense covariance of the exact posterior(x*), x_star [ns, 2] (ns <= 8192) -> [ns, ns]."""
        xs = x_star.to(self.device, torch.float64)
        xs1, xs2 = xs[:, 0].contiguous(), xs[:, 1].contiguous()
        ns = xs1.shape[0]
        cov = torch.empty(ns, ns, dtype=torch.float64, device=self.device)
        check(self.lib.vggp_exact_posterior_cov(self._h, _ptr(xs1), _ptr(xs2), ns, _ptr(cov), _stream(self.device)))
        return cov

    def exact_readout(self, C1: torch.Tensor, C2: torch.Tensor, kd1: torch.Tensor, kd2: torch.Tensor, literal: bool = True):
        """Gridded read-out q(v) of B0 cell features from the last exact step (Matern-1/2 plans): C_d [mv_d, N] unit-outputscale
        Cov(v, f(x_i)) along d, kd_d [mv_d] unit diagonals of Kvv_d -> mean, var [mv1, mv2]."""
        C1, C2 = C1.to(self.device, torch.float64).contiguous(), C2.to(self.device, torch.float64).contiguous()
        kd1, kd2 = kd1.to(self.device, torch.float64).contiguous(), kd2.to(self.device, torch.float64).contiguous()
        if C1.shape[1] != self.exact_n or C2.shape[1] != self.exact_n or kd1.numel() != C1.shape[0] or kd2.numel() != C2.shape[0]:
            raise ValueError("C_d must be [mv_d, N] and kd_d [mv_d]")
        mean = torch.empty(C1.shape[0], C2.shape[0], dtype=torch.float64, device=self.device)
        var = torch.empty_like(mean)
        check(self.lib.vggp_exact_readout(self._h, _ptr(C1), C1.shape[0], _ptr(C2), C2.shape[0], _ptr(kd1), _ptr(kd2), _ptr(mean),
                                          _ptr(var), 1 if literal else 0, _stream(self.device)))
        return mean, var

    # -- iterative exact GP (matrix-free PCG; any N with N * 64 < 2^31; a workspace of its own) --------------
    def exact_iter_plan(self, kind1: str, kind2: str, x1, x2) -> None:
        """Iterative exact GP on the N points (x1[k], x2[k]) (vggp_exact_iter_plan).  Independent of plan() and of exact_plan()."""
        x1, x2 = _dvec(x1), _dvec(x2)
        if len(x1) != len(x2):
            raise ValueError("exact plan: x1 and x2 must hold one coordinate pair per point")
        with torch.cuda.device(self.device):
            check(self.lib.vggp_exact_iter_plan(self._h, KIND[kind1], KIND[kind2], x1.ctypes.data, x2.ctypes.data, len(x1)))
        self.exact_iter_n = len(x1)
        self.exact_iter_token += 1

    def exact_step_iter(self, y: torch.Tensor, theta: Sequence[float], n_probes: int = 0, rank: int = -1, tol: float = 0.0,
                        max_iter: int = 0):
        """-> (marginal log likelihood, grad[5], info dict): PCG + stochastic Lanczos quadrature estimates (vggp_exact_step_iter);
        the defaults (16 probes, rank 64, tol 1e-10, 1000 iterations) are the entry's.  info["rounds"][0] = PCG iterations."""
        if not (y.is_cuda and y.dtype == torch.float64 and y.is_contiguous() and y.numel() == self.exact_iter_n):
            raise TypeError("y must be a contiguous float64 GPU tensor with one value per planned point")
        th = (C.c_double * 5)(*[float(t) for t in theta])
        mll = C.c_double()
        grad = (C.c_double * 5)()
        info = Info()
        check(self.lib.vggp_exact_step_iter(self._h, _ptr(y), th, int(n_probes), int(rank), float(tol), int(max_iter), C.byref(mll), grad,
                                            C.byref(info), _stream(self.device)))
        return mll.value, np.array(list(grad)), self._info(info)

    def exact_posterior_iter(self, x_star: torch.Tensor, variance: bool = True, tol: float = 0.0, max_iter: int = 0):
        """posterior(x*) of the last iterative exact step; x_star [ns, 2] -> mean[ns], var[ns] (None without variance), info."""
        xs = x_star.to(self.device, torch.float64)
        xs1, xs2 = xs[:, 0].contiguous(), xs[:, 1].contiguous()
        ns = xs1.shape[0]
        mean = torch.empty(ns, dtype=torch.float64, device=self.device)
        var = torch.empty_like(mean) if variance else None
        info = Info()
        check(self.lib.vggp_exact_posterior_iter(self._h, _ptr(xs1), _ptr(xs2), ns, float(tol), int(max_iter), _ptr(mean), _ptr(var),
                                                 C.byref(info), _stream(self.device)))
        return mean, var, self._info(info)

    def exact_readout_iter(self, C1: torch.Tensor, C2: torch.Tensor, kd1: torch.Tensor, kd2: torch.Tensor, literal: bool = True, cells=None,
                           variance: bool = True, tol: float = 0.0, max_iter: int = 0):
        """Gridded read-out q(v) from the last iterative exact step (Matern-1/2 plans), operands as exact_readout -> mean [mv1, mv2],
        var, info: literal=True gives var [mv1, mv2] without a solve; literal=False the conditional variance at `cells` [n_cells]."""
        C1, C2 = C1.to(self.device, torch.float64).contiguous(), C2.to(self.device, torch.float64).contiguous()
        kd1, kd2 = kd1.to(self.device, torch.float64).contiguous(), kd2.to(self.device, torch.float64).contiguous()
        n = self.exact_iter_n
        if C1.shape[1] != n or C2.shape[1] != n or kd1.numel() != C1.shape[0] or kd2.numel() != C2.shape[0]:
            raise ValueError("C_d must be [mv_d, N] and kd_d [mv_d]")
        mean = torch.empty(C1.shape[0], C2.shape[0], dtype=torch.float64, device=self.device)
        cl, ncell = None, 0
        if cells is not None:
            idx = np.ascontiguousarray(np.asarray(cells, dtype=np.int64).reshape(-1))
            cl, ncell = idx.ctypes.data_as(C.POINTER(C.c_int64)), len(idx)
        var = None
        if variance:
            # (never an empty tensor: its null pointer would read as "mean only" and hide a missing cell list from the entry)
            var = torch.empty_like(mean) if literal else torch.empty(max(ncell, 1), dtype=torch.float64, device=self.device)
        info = Info()
        check(self.lib.vggp_exact_readout_iter(self._h, _ptr(C1), C1.shape[0], _ptr(C2), C2.shape[0], _ptr(kd1), _ptr(kd2), cl, ncell,
                                               float(tol), int(max_iter), _ptr(mean), _ptr(var), 1 if literal else 0, C.byref(info),
                                               _stream(self.device)))
        return mean, (var if (var is None or literal) else var[:ncell]), self._info(info)

    def exact_iter_alpha(self, theta: Sequence[float], chunk: int = 2048) -> torch.Tensor:
        """alpha = Sigma^-1 y of the last iterative exact step [N], read back exactly (diagnostics and tests; Matern-1/2 plans): the
        gridded read-out's mean s C1 diag(alpha) C2^T with C1 = 1^T and one-hot rows in C2 is s alpha_i, one term per output."""
        n, s = self.exact_iter_n, float(theta[2]) * float(theta[3])
        one = torch.ones(1, n, dtype=torch.float64, device=self.device)
        out = torch.empty(n, dtype=torch.float64, device=self.device)
        for i0 in range(0, n, chunk):
            k = min(chunk, n - i0)
            C2 = torch.zeros(k, n, dtype=torch.float64, device=self.device)
            C2[torch.arange(k), i0 + torch.arange(k)] = 1.0
            mean, _, _ = self.exact_readout_iter(one, C2, torch.ones(1), torch.ones(k), variance=False)
            out[i0:i0 + k] = mean[0] / s
        return out

    def exact_kmv(self, kind1: str, kind2: str, ell1: float, ell2: float, xr: torch.Tensor, xc: torch.Tensor, V: torch.Tensor,
                  derivatives: bool = False):
        """Matrix-free K0(xr, xc) @ V at unit outputscale (vggp_exact_kmv): xr [Nr, 2], xc [Nc, 2], V [Nc, nb] (nb <= 64) float64
        -> out0 [Nr, nb]; derivatives=True -> (out0, out1, out2) with dK0/d ell1 and dK0/d ell2 in the same pass."""
        xr, xc = xr.to(self.device, torch.float64), xc.to(self.device, torch.float64)
        if xr.dim() != 2 or xr.shape[1] != 2 or xc.dim() != 2 or xc.shape[1] != 2:
            raise ValueError("xr and xc must be (N, 2)")
        if not (V.is_cuda and V.dtype == torch.float64 and V.is_contiguous() and V.dim() == 2 and V.shape[0] == xc.shape[0]):
            raise TypeError("V must be a contiguous float64 GPU tensor [Nc, nb]")
        xr1, xr2, xc1, xc2 = xr[:, 0].contiguous(), xr[:, 1].contiguous(), xc[:, 0].contiguous(), xc[:, 1].contiguous()
        Nr, Nc, nb = xr.shape[0], xc.shape[0], V.shape[1]
        outs = [torch.empty(Nr, nb, dtype=torch.float64, device=self.device) for _ in range(3 if derivatives else 1)]
        check(self.lib.vggp_exact_kmv(self._h, KIND[kind1], KIND[kind2], float(ell1), float(ell2), _ptr(xr1), _ptr(xr2), Nr, _ptr(xc1),
                                      _ptr(xc2), Nc, _ptr(V), nb, _ptr(outs[0]), _ptr(outs[1]) if derivatives else None,
                                      _ptr(outs[2]) if derivatives else None, _stream(self.device)))
        return tuple(outs) if derivatives else outs[0]

    # -- building blocks ------------------------------------------------------------------------------
    def factor_build(self, kind: str, basis: str, x: torch.Tensor, grid: torch.Tensor, ell: float, flags: int = 0):
        """-> A0[m,n], dA0[m,n], K0[m,m], dK0[m,m] at unit outputscale."""
        n = x.shape[0]
        m = _basis_m(basis, np.empty(grid.shape[0]))
        o = dict(dtype=torch.float64, device=self.device)
        A, dA, K, dK = torch.empty(m, n, **o), torch.empty(m, n, **o), torch.empty(m, m, **o), torch.empty(m, m, **o)
        check(self.lib.vggp_factor_build(self._h, KIND[kind], BASIS[basis], _ptr(x), n, _ptr(grid), m, float(ell), int(flags),
                                         _ptr(A), _ptr(dA), _ptr(K), _ptr(dK), _stream(self.device)))
        return A, dA, K, dK

    def cholesky_inverse(self, K: torch.Tensor):
        m = K.shape[0]
        L, Li = torch.empty_like(K), torch.empty_like(K)
        jit = C.c_double()
        check(self.lib.vggp_cholesky_inverse(self._h, _ptr(K), m, _ptr(L), _ptr(Li), C.byref(jit), _stream(self.device)))
        return L, Li, jit.value

    def eigh(self, G: torch.Tensor, block: bool = False):
        """-> lam[m], Qt[m,m] (row j = eigenvector j), sweeps."""
        m = G.shape[0]
        lam = torch.empty(m, dtype=torch.float64, device=self.device)
        Qt = torch.empty_like(G)
        sw = C.c_int32()
        check(self.lib.vggp_eigh(self._h, _ptr(G), m, _ptr(lam), _ptr(Qt), C.byref(sw),
                                 _lib.FLAG_BLOCK_JACOBI if block else 0, _stream(self.device)))
        return lam, Qt, sw.value

    # the thin chain's kernels, one job each (include/vggp.h; tests/test_gpu_thin_chain_paths.py)
    def pivchol(self, G: torch.Tensor, Omega: torch.Tensor) -> torch.Tensor:
        """-> V[r,m]: r = Omega.shape[0] steps of diagonally pivoted Cholesky of G[m,m], the columns as rows."""
        r, m = Omega.shape
        V = torch.empty(r, m, dtype=torch.float64, device=self.device)
        check(self.lib.vggp_pivchol(self._h, _ptr(G), _ptr(Omega), m, r, _ptr(V), _stream(self.device)))
        return V

    def rowqr(self, Z: torch.Tensor, cp_src: torch.Tensor = None) -> torch.Tensor:
        """-> V1[r,m], the rows of Z orthonormalised in their order (and the pass-through copy of cp_src, when given)."""
        r, m = Z.shape
        V1 = torch.empty_like(Z)
        cp_dst = torch.empty_like(cp_src) if cp_src is not None else None
        check(self.lib.vggp_rowqr(self._h, _ptr(Z), r, m, _ptr(V1), _ptr(cp_src) if cp_src is not None else None,
                                  _ptr(cp_dst) if cp_src is not None else None, cp_src.numel() if cp_src is not None else 0,
                                  _stream(self.device)))
        return V1 if cp_src is None else (V1, cp_dst)

    def ritz(self, Hl: torch.Tensor, Hr: torch.Tensor):
        """-> lam[r] (decreasing), W[r,r] (row j = Ritz vector j), counters[4], err of the matrix whose lower triangle is tril(Hl Hr^T)."""
        r, hk = Hl.shape
        lam = torch.empty(r, dtype=torch.float64, device=self.device)
        W = torch.empty(r, r, dtype=torch.float64, device=self.device)
        cnt, err = (C.c_int32 * 4)(), C.c_int32()
        check(self.lib.vggp_ritz(self._h, _ptr(Hl), _ptr(Hr), r, hk, _ptr(lam), _ptr(W), cnt, C.byref(err), _stream(self.device)))
        return lam, W, list(cnt), err.value

    def thin_tail(self, args: "_lib.ThinTailArgs") -> None:
        """The thin m-space stage on the device arrays named by `args` (see vggp_thin_tail_args)."""
        check(self.lib.vggp_thin_tail(self._h, C.byref(args), _stream(self.device)))

    def gemm(self, A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
        """C = A @ B for 2-D float64 GPU tensors with arbitrary strides (no copies are made)."""
        M, K = A.shape
        K2, N = B.shape
        assert K == K2
        Cm = torch.empty(M, N, dtype=torch.float64, device=self.device)
        for t in (A, B):
            if not (t.is_cuda and t.dtype == torch.float64):
                raise TypeError("gemm operands must be float64 GPU tensors")
        check(self.lib.vggp_gemm(self._h, A.data_ptr(), A.stride(0), A.stride(1), B.data_ptr(), B.stride(0),
                                 B.stride(1), Cm.data_ptr(), N, M, N, K, _stream(self.device)))
        return Cm

    def kron_solve(self, L1: torch.Tensor, L2: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
        """X = K1^{-1} Y K2^{-T} with K_d = L_d L_d^T from the Cholesky factors (four triangular solves by substitution)."""
        n1, n2 = Y.shape
        X = torch.empty_like(Y)
        check(self.lib.vggp_kron_solve(self._h, _ptr(L1), n1, _ptr(L2), n2, _ptr(Y), _ptr(X), _stream(self.device)))
        return X

    def trsm(self, L: torch.Tensor, R: torch.Tensor, trans: bool = False) -> torch.Tensor:
        """Solve L X = R (or L^T X = R) for lower-triangular L [m, m] and R [m, ncols] by substitution."""
        m, ncols = R.shape
        X = torch.empty_like(R)
        check(self.lib.vggp_trsm(self._h, _ptr(L), m, _ptr(R), ncols, _ptr(X), 1 if trans else 0, _stream(self.device)))
        return X

    def profile(self, enable: bool = True) -> None:
        check(self.lib.vggp_profile(self._h, 1 if enable else 0))

    def profile_read(self, reset: bool = True):
        """-> ({stage name: accumulated ms}, steps) measured with HIP events on the launch stream."""
        ms = (C.c_double * _lib.NSTAGE)()
        steps = C.c_int32()
        check(self.lib.vggp_profile_read(self._h, ms, C.byref(steps), 1 if reset else 0))
        names = [self.lib.vggp_stage_name(i).decode() for i in range(_lib.NSTAGE)]
        return dict(zip(names, list(ms))), steps.value

    def project_kernel_name(self) -> str:
        return self.lib.vggp_project_kernel_name().decode()

    def sumsq(self, y: torch.Tensor) -> float:
        out = C.c_double()
        check(self.lib.vggp_sumsq(self._h, _ptr(y), y.numel(), C.byref(out), _stream(self.device)))
        return out.value
