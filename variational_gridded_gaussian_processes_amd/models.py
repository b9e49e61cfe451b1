"""Drop-in host-side mirror of the reference's model API for the Kronecker ELBO hot path.

Same class names, constructor arguments, method names and attribute reads as the reference's
notebooks use:

    reference                                                    here
    src/models/sparse/gridded_kronecker_structure.py:1255-1433   Matern12GriddedGP
    src/models/sparse/kronecker_structure.py:671-849             Matern12B0SplineGriddedGP
    src/models/sparse/kronecker_structure.py:287-338             Matern12SVGP (+ Matern32/52/RBF variants, new)
    src/models/sparse/kronecker_structure.py:15-278              KroneckerStructure (base: _elbo, q_v, posterior, ...)
    src/models/sparse/univariate_structure.py:721-825, :325-354  univariate.Matern12B0SplineGriddedGP, univariate.*SVGP

`model._elbo()` returns a differentiable 0-d tensor, so the notebooks' loop
`optimizer.zero_grad(); loss = -model._elbo(); loss.backward(); optimizer.step()` with
`torch.optim.Adam(model.parameters(), lr)` runs unchanged -- but value and gradient come from ONE
call into libvggp_hip.so (analytic gradient), not from autograd over dense N x N algebra.
The gpytorch pieces the reference leans on (GaussianLikelihood, ScaleKernel, MaternKernel,
MultivariateNormal) are mirrored here only as far as the path reads them: parameter transforms
(softplus, noise >= 1e-4, raw init 0) and accessor names.  There is no CPU fallback.
"""
from __future__ import annotations

import math
import warnings
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import VggpError
from .basis import B0SplineBasis, B1SplineBasis, FourierBasisMatern12
from .engine import Engine, _basis_m

NOISE_LOWER = 1e-4


def _inv_softplus(y: torch.Tensor) -> torch.Tensor:
    return y + torch.log(-torch.expm1(-y))


# ---------------------------------------------------------------------------------------------
# minimal mirrors of the gpytorch modules whose attributes the notebooks read
# ---------------------------------------------------------------------------------------------
class _BaseKernel(torch.nn.Module):
    """MaternKernel(nu) / RBFKernel: only the lengthscale parameter lives here."""

    def __init__(self, kind: str):
        super().__init__()
        self.kind = kind
        self.nu = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5, "rbf": math.inf}[kind]
        self.raw_lengthscale = torch.nn.Parameter(torch.zeros(1, 1))

    @property
    def lengthscale(self) -> torch.Tensor:
        # a fresh tensor, like gpytorch's property: `kernel.lengthscale[0] = v` therefore does NOT
        # update the raw parameter (the reference's non_informative_initialise quirk)
        return torch.nn.functional.softplus(self.raw_lengthscale)

    @lengthscale.setter
    def lengthscale(self, value):
        v = torch.as_tensor(value, dtype=self.raw_lengthscale.dtype).reshape(1, 1)
        with torch.no_grad():
            self.raw_lengthscale.copy_(_inv_softplus(v))


class ScaleKernel(torch.nn.Module):
    def __init__(self, base_kernel: _BaseKernel):
        super().__init__()
        self.base_kernel = base_kernel
        self.raw_outputscale = torch.nn.Parameter(torch.zeros(()))

    @property
    def outputscale(self) -> torch.Tensor:
        return torch.nn.functional.softplus(self.raw_outputscale)

    @outputscale.setter
    def outputscale(self, value):
        v = torch.as_tensor(value, dtype=self.raw_outputscale.dtype).reshape(())
        with torch.no_grad():
            self.raw_outputscale.copy_(_inv_softplus(v))


class GaussianLikelihood(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.raw_noise = torch.nn.Parameter(torch.zeros(1))

    @property
    def noise(self) -> torch.Tensor:
        return torch.nn.functional.softplus(self.raw_noise) + NOISE_LOWER

    @noise.setter
    def noise(self, value):
        v = torch.as_tensor(value, dtype=self.raw_noise.dtype).reshape(1)
        with torch.no_grad():
            self.raw_noise.copy_(_inv_softplus(v - NOISE_LOWER))


class MultivariateNormal:
    """What q_v()/posterior() return: `.mean`, `.variance`, `.stddev`, `.confidence_region()` and a lazily
    materialised `.covariance_matrix` (dense, small problems only).  `variance` may be a callable: it is then evaluated once, on
    the first use of `.variance`, `.stddev` or `.confidence_region()` (the all-cell variance of the iterative masked solver costs
    M / 64 block solves, the mean none).
    `.sample(sample_shape, seed)` draws JOINT samples where a sampler is attached: the q_v() of KroneckerStructure on full grids and on
    both iterative solvers (engine side, no M x M matrix) and on the dense masked / scattered states up to M = 4096 (from
    `.covariance_matrix`); this is also the q_u() of the Gridded* classes, the same distribution.  Not attached (sample raises
    NotImplementedError): the gridded q_v() of the Gridded* classes (v != u: a joint residual Kvv - Kvu Kuu^-1 Kuv is needed),
    the point-wise posterior(x*), paired inducing points, the 1-D classes, the exact GP, multi-rank contexts.  posterior_grid() and
    posterior_predictive_grid() carry a sampler of the whole map on full grids and on both iterative solvers (not on the dense masked /
    scattered states, not for B1 hats).  A model built with dense_samples=True draws both on the engine on the dense states as well,
    at any M the dense solver takes (KroneckerStructure.__init__)."""

    def __init__(self, mean: torch.Tensor, variance, cov_fn=None, sample_fn=None):
        self.mean = mean
        self._variance = variance
        self._cov_fn = cov_fn
        self._cov = None
        self._sample_fn = sample_fn      # (n, seed, first) -> [n, *mean.shape]
        self._next = 0                   # the next sample number of the unseeded sequence
        self._seed0 = None

    def sample(self, sample_shape=torch.Size(), seed: Optional[int] = None) -> torch.Tensor:
        """Joint samples, sample_shape + mean.shape.  Not differentiable (there is no rsample).  With a seed the call is reproducible:
        it returns samples 0 .. n - 1 of that seed.  Without one, successive calls on this object continue one sequence (the object
        draws a seed once and keeps the number of the next sample)."""
        if self._sample_fn is None:
            raise NotImplementedError("joint samples are not available for this distribution: q_v() of the KroneckerStructure models "
                                      "(full grid, solver='iterative', scattered_solver='iterative', dense states up to M = 4096) "
                                      "and posterior_grid() on full grids and the iterative solvers carry a sampler; the gridded q_v() "
                                      "of the Gridded* classes, the point-wise posterior(x*), paired inducing points, the 1-D classes "
                                      "and the exact GP do not")
        shape = torch.Size(sample_shape)
        n = int(np.prod(shape)) if len(shape) else 1
        if n < 1:
            return torch.empty(shape + self.mean.shape, dtype=self.mean.dtype)
        if seed is None:
            if self._seed0 is None:
                self._seed0 = int(torch.randint(0, 2**62, (1,)).item())
            out = self._sample_fn(n, self._seed0, self._next)
            self._next += n
        else:
            out = self._sample_fn(n, int(seed), 0)
        return out.reshape(shape + self.mean.shape)

    @property
    def variance(self) -> torch.Tensor:
        if callable(self._variance):
            self._variance = self._variance()
        return self._variance

    @property
    def stddev(self) -> torch.Tensor:
        return self.variance.clamp_min(0).sqrt()

    @property
    def covariance_matrix(self) -> torch.Tensor:
        if self._cov is None:
            if self._cov_fn is None:
                raise NotImplementedError("dense covariance is not available for this distribution; use .variance")
            self._cov = self._cov_fn()
        return self._cov

    def confidence_region(self) -> Tuple[torch.Tensor, torch.Tensor]:
        s2 = 2.0 * self.stddev
        return self.mean - s2, self.mean + s2


def _symmetric_root(cov: torch.Tensor) -> torch.Tensor:
    """The symmetric square root of a covariance matrix by eigh, eigenvalues clamped at 0."""
    w, V = torch.linalg.eigh(0.5 * (cov + cov.T))
    return (V * w.clamp_min(0).sqrt()[None, :]) @ V.T


class _ElboFunction(torch.autograd.Function):
    """value + analytic gradient from one vggp_elbo_step; backward only scales the cached gradient."""

    @staticmethod
    def forward(ctx, theta: torch.Tensor, model: "KroneckerStructure", Z: Optional[torch.Tensor] = None):
        try:
            elbo, grad, info = model._engine_step([float(t) for t in theta.detach().cpu()])
        except VggpError as e:
            if e.code == _lib.VGGP_ENOTPD:       # what the reference's notebooks catch (61_envisat... cell 39)
                raise torch.linalg.LinAlgError(str(e)) from e
            raise
        model.last_info = info
        gz = None
        if Z is not None and Z.requires_grad:
            # trainable inducing points (the reference registers Z as a Parameter, kronecker_structure.py:303-304, and autograd
            # reaches it through kernel(Z)): analytic gradient from the engine's resident state (vggp_zgrad)
            g1, g2 = model._engine.zgrad_scattered(model._Y) if getattr(model, "_scattered", False) else model._engine.zgrad(model._Y)
            cols = [g1] if Z.shape[1] == 1 else [g1, g2]
            gz = torch.stack(cols, dim=1).to(dtype=Z.dtype, device=Z.device)
        ctx.save_for_backward(torch.as_tensor(grad, dtype=theta.dtype, device=theta.device), gz)
        return torch.as_tensor(elbo, dtype=theta.dtype, device=theta.device)

    @staticmethod
    def backward(ctx, grad_out):
        g, gz = ctx.saved_tensors
        return grad_out * g, None, (grad_out * gz if gz is not None else None)


def _detect_grid(X: torch.Tensor):
    """X (N,2) -> (x1, x2, W, flat).  Full grid in gen_2d layout (utils/datagenerators.py:70-72: x1 fastest): W and flat
    are None.  Otherwise X must be a subset of the cartesian grid of its own unique coordinates (a masked grid,
    BASELINE config 5): W[j, i] = 1 on observed points and flat[k] = j*n1 + i places y[k] on the grid."""
    Xn = X.detach().cpu().numpy().astype(np.float64)
    if Xn.ndim != 2 or Xn.shape[1] != 2:
        raise ValueError("X must be (N, 2)")
    N = Xn.shape[0]
    x2_first = Xn[0, 1]
    n1 = int(np.argmax(Xn[:, 1] != x2_first)) if np.any(Xn[:, 1] != x2_first) else N
    if n1 > 0 and N % n1 == 0:
        n2 = N // n1
        G = Xn.reshape(n2, n1, 2)
        x1, x2 = G[0, :, 0].copy(), G[:, 0, 1].copy()
        if (np.array_equal(G[:, :, 0], np.broadcast_to(x1, (n2, n1)))
                and np.array_equal(G[:, :, 1], np.broadcast_to(x2[:, None], (n2, n1)))):
            return x1, x2, None, None
    x1, i = np.unique(Xn[:, 0], return_inverse=True)
    x2, j = np.unique(Xn[:, 1], return_inverse=True)
    if len(x1) * len(x2) > 16 * N:
        # general scattered points (along-track data): no grid at all -- the per-point coordinates go to the engine as they are
        # (vggp_elbo_step_scattered: Khatri-Rao assembly in M-space)
        return Xn[:, 0].copy(), Xn[:, 1].copy(), "scattered", None
    flat = j.astype(np.int64) * len(x1) + i.astype(np.int64)
    W = np.zeros(len(x1) * len(x2))
    W[flat] = 1.0
    if int(W.sum()) != N:
        raise ValueError("X holds duplicated points")
    return x1, x2, W.reshape(len(x2), len(x1)), flat


class KroneckerStructure(torch.nn.Module):
    """kronecker_structure.py:15-278 -- the 2-D sparse-GP base class, structured engine inside."""

    kind = "matern12"

    def __init__(self, X: torch.Tensor, y: torch.Tensor, engine: Optional[Engine] = None, warm_start: bool = True,
                 solver: str = "auto", scattered_solver: str = "auto", scattered_variances: bool = False,
                 dense_samples: bool = False):
        """solver: how a grid with holes is solved.  "dense": the M x M solver (M = m1 m2 <= 16384); "iterative": PCG without any
        M x M matrix (Engine.elbo_step_masked_iter and its read-outs; also accepted on a full grid, which it treats as a mask of
        ones); "auto": iterative only for a grid with holes whose M exceeds the dense solver's limit, dense everywhere else.
        `solver` does not apply to scattered points or paired inducing points: "iterative" raises ValueError there.
        scattered_solver: how scattered points (along-track data) are solved.  "dense": the M x M solver (M <= 16384, four
        m_d^2 x N buffers); "iterative": PCG on the Khatri-Rao operator without any of them (Engine.elbo_step_scattered_iter; q_v()
        and posterior() of the inducing features then carry means only unless scattered_variances is set, the gridded q_v() of the
        Gridded* classes mean and variance);
        "auto": iterative only when M exceeds the dense solver's limit ("iterative" on a grid with holes, which `solver` governs
        otherwise, treats it as its observed points).  A model whose
        inducing points are trained (SVGP, train_z=True) keeps the dense path: its Z-gradient reads dense state.
        scattered_variances: on the iterative scattered solver, give q_v(), q_u(), posterior() and posterior_predictive() their
        point-wise variances (Engine.qv_var_scattered_iter / posterior_var_scattered_iter: ceil(columns / 64) block PCG solves; the
        all-cell variance of q_v() is computed on first use).  False keeps the means-only distributions, whose .variance raises;
        q_v_at(cells) gives the variance of a few cells either way.  No effect on the other solvers.
        dense_samples: on the dense masked / scattered states (without paired inducing points), draw joint samples on the engine
        from the inverse factor the step keeps (Engine.qv_sample_masked / posterior_raster_sample_masked: X = Xg^T E, one launch per
        64 samples, nothing solved and no M x M temporary): q_v().sample works at every M <= 16384, posterior_grid().sample and
        posterior_predictive_grid().sample draw maps, and sample s of a seed is one joint draw across q_v() and the map, as on the
        other solvers.  False (the default) keeps q_v().sample on the symmetric root of covariance_matrix (M <= 4096; other numbers,
        the same distribution) and the raster samplers refusing.  No effect on full grids and on the iterative solvers."""
        super().__init__()
        if solver not in ("auto", "dense", "iterative"):
            raise ValueError(f"solver must be 'auto', 'dense' or 'iterative', got {solver!r}")
        if scattered_solver not in ("auto", "dense", "iterative"):
            raise ValueError(f"scattered_solver must be 'auto', 'dense' or 'iterative', got {scattered_solver!r}")
        self.solver = solver
        self.scattered_solver = scattered_solver
        self.scattered_variances = bool(scattered_variances)
        self.dense_samples = bool(dense_samples)
        self.last_readout_info = None    # PCG counts of the last variance read-out on an iterative solver
        self._siter = False              # the iterative scattered step applies (decided at plan time)
        self.n_probes, self.tol, self.max_iter = 16, 1e-10, 100      # of the iterative solver (the engine's defaults)
        self._iter = False
        self.train_inputs = (X,)
        self.train_targets = y
        self.likelihood = GaussianLikelihood()
        self.kernel_1 = ScaleKernel(_BaseKernel(self.kind))
        self.kernel_2 = ScaleKernel(_BaseKernel(self.kind))
        self._engine = engine if engine is not None else Engine()
        self._warm = warm_start
        self._planned = False
        self._plan_token, self._plan_key = -1, None
        self.last_info = None
        self._x1, self._x2, W, flat = _detect_grid(X)
        n2, n1 = len(self._x2), len(self._x1)
        yd = torch.as_tensor(y, dtype=torch.float64).reshape(-1).to(self._engine.device)
        self._scattered = isinstance(W, str)
        self._masked = W is not None     # (read-outs of the scattered mode are the masked ones: dense M-space state)
        if self._scattered:              # scattered points: y stays a vector, one coordinate pair per point
            self._Y = yd.contiguous()
            self._nobs = float(yd.numel())
        elif self._masked:               # masked grid: scatter the observations onto the grid (zeros elsewhere)
            self._W = torch.as_tensor(W, device=self._engine.device)
            self._Y = torch.zeros(n2 * n1, dtype=torch.float64, device=self._engine.device)
            self._Y[torch.as_tensor(flat, device=self._engine.device)] = yd
            self._Y = self._Y.reshape(n2, n1)
            self._nobs = float(W.sum())
        else:
            self._Y = yd.reshape(n2, n1).contiguous()
            if solver == "iterative":    # a full grid through the iterative solver: a mask of ones
                self._masked, self._nobs = True, float(n1 * n2)
                self._W = torch.ones(n2, n1, dtype=torch.float64, device=self._engine.device)
        if self._scattered:
            self._no_iterative("scattered points")
        self._yy = float((yd * yd).sum().item()) if self._scattered else self._engine.sumsq(self._Y)
        if scattered_solver == "iterative" and W is not None and not self._scattered:
            self._as_scattered()         # forced on a grid with holes: it is then treated as its observed points

    def _no_iterative(self, what: str):
        if self.solver == "iterative":
            raise ValueError(f"{type(self).__name__}: solver='iterative' needs observations on a grid (with or without holes); "
                             f"{what} take the dense M-space solver")

    def _use_iterative(self, basis, g1, g2) -> bool:
        """The iterative masked solver applies (see __init__)."""
        if self.solver == "dense" or self._scattered or not self._masked or basis == "paired":
            return False
        return self.solver == "iterative" or _basis_m(basis, np.asarray(g1)) * _basis_m(basis, np.asarray(g2)) > 16384

    def _use_scattered_iterative(self, basis, g1, g2) -> bool:
        """The iterative scattered solver applies (see __init__)."""
        if not self._scattered or self.scattered_solver == "dense" or basis == "paired":
            return False
        want = self.scattered_solver == "iterative" or _basis_m(basis, np.asarray(g1)) * _basis_m(basis, np.asarray(g2)) > 16384
        Z = getattr(self, "Z", None)
        if want and isinstance(Z, torch.Tensor) and Z.requires_grad:
            # vggp_zgrad_scattered reads the dense step's Sigma~^-1: trained inducing points stay on the dense path
            if self.scattered_solver == "iterative" and not getattr(self, "_warned_siter", False):
                warnings.warn(f"{type(self).__name__}: scattered_solver='iterative' does not apply while the inducing points are trained "
                              f"(the Z-gradient reads the dense solver's state); the dense scattered solver is used")
                self._warned_siter = True
            return False
        return want

    def _scattered_iter_variance(self):
        raise NotImplementedError(f"{type(self).__name__}: the iterative scattered solver provides means only unless the model is built "
                                  f"with scattered_variances=True (block PCG solves, the follow-up to vggp_qv_scattered_iter / "
                                  f"vggp_posterior_scattered_iter; q_v_at(cells) gives a few variances without it); dense covariances "
                                  f"need scattered_solver='dense' (M <= 16384)")

    def _as_scattered(self):
        """Switch a masked-grid model to the scattered representation of the same observations (one coordinate pair per point):
        the step with a Z-gradient on incomplete data is vggp_zgrad_scattered."""
        if self._scattered or not self._masked:
            return
        self._no_iterative("a grid with holes whose inducing points are trained (it is treated as its observed points)")
        Xn = self.train_inputs[0].detach().cpu().numpy().astype(np.float64)
        yd = torch.as_tensor(self.train_targets, dtype=torch.float64).reshape(-1).to(self._engine.device)
        self._x1, self._x2 = Xn[:, 0].copy(), Xn[:, 1].copy()
        self._scattered, self._Y, self._nobs = True, yd.contiguous(), float(yd.numel())
        self._yy = float((yd * yd).sum().item())
        self._W = None
        self._planned = False

    # subclasses provide (basis, grid_1, grid_2)
    def _basis(self) -> Tuple[str, np.ndarray, np.ndarray]:
        raise NotImplementedError

    def _f32_mesh(self) -> bool:
        """True when the B0 mesh is a float32 tensor (the reference's default): reproduce its float32 k*delta."""
        mesh = getattr(self, "mesh_1", getattr(self, "mesh", None))
        return mesh is not None and mesh.dtype == torch.float32

    def _plan(self):
        """(Re)plan the engine when this model is not its last planner (an Engine may be shared between models: the plan --
        factors, basis, meshes -- lives in the engine) or when its inducing description changed since the last plan."""
        basis, g1, g2 = self._basis()
        self._iter = self._use_iterative(basis, g1, g2)
        self._siter = self._use_scattered_iterative(basis, g1, g2)
        key = (basis, np.asarray(g1).tobytes(), np.asarray(g2).tobytes())
        if self._planned and self._plan_token == self._engine.plan_token and key != self._plan_key and basis == "points" \
                and self._plan_key is not None and len(self._plan_key[1]) == len(key[1]) and len(self._plan_key[2]) == len(key[2]):
            # only the inducing points moved (an optimiser training Z): new coordinates in place, plan / graphs / warm start stay
            if key[1] != self._plan_key[1]:
                self._engine.set_inducing(0, g1)
            if key[2] != self._plan_key[2]:
                self._engine.set_inducing(1, g2)
            self._plan_key = key
        elif not self._planned or self._plan_token != self._engine.plan_token or key != self._plan_key:
            if (self._scattered or self._masked) and not self._iter and not self._siter:
                self._check_dense_workspace(basis, g1, g2)
            self._engine.plan(self.kind, basis, g1, self._x1, self.kind, basis, g2, self._x2, warm_start=self._warm,
                              b0_f32_kdelta=self._f32_mesh(), scattered=self._scattered)
            self._planned = True
            self._plan_token, self._plan_key = self._engine.plan_token, key

    def _check_dense_workspace(self, basis, g1, g2):
        """The masked / scattered steps work on dense M x M matrices (M = m1 m2 <= 16384; ~10 M^2 doubles) and, for scattered points,
        on four m_d^2 x N pair-product buffers that are not chunked over N: say so here, with the numbers, instead of failing in
        hipMalloc at the first step."""
        m1 = len(g1) - 1 if basis in ("b0", "b0k") else (2 * (len(g1) - 3) + 1 if basis == "vff" else len(g1))
        m2 = len(g2) - 1 if basis in ("b0", "b0k") else (2 * (len(g2) - 3) + 1 if basis == "vff" else len(g2))
        M, N = m1 * m2, int(self._nobs)
        if M > 16384:
            raise ValueError(f"{type(self).__name__}: X is {'scattered' if self._scattered else 'a grid with holes'}, which takes the dense "
                             f"M-space solver, and M = m1 * m2 = {m1} * {m2} = {M} exceeds its limit of 16384 "
                             f"(solver='auto' or 'iterative' handles larger M on grids with holes, scattered_solver='auto' or "
                             f"'iterative' on scattered points whose inducing points are not trained)")
        n_pair = N if self._scattered else max(len(self._x1), len(self._x2))
        need = 8.0 * (10.0 * M * M + 2.0 * (m1 * m1 + m2 * m2) * n_pair)
        free = torch.cuda.mem_get_info(self._engine.device)[0] if torch.cuda.is_available() else None
        if free is not None and need > free:
            raise ValueError(f"{type(self).__name__}: the dense M-space workspace needs about {need / 2**30:.1f} GiB (M = {M}, N = {N}, "
                             f"m_d = {m1}, {m2}: ~10 M^2 + 2 (m1^2 + m2^2) N doubles) but {free / 2**30:.1f} GiB of device memory are free")

    def _theta(self) -> torch.Tensor:
        return torch.stack([self.kernel_1.base_kernel.lengthscale.reshape(()),
                            self.kernel_2.base_kernel.lengthscale.reshape(()),
                            self.kernel_1.outputscale.reshape(()), self.kernel_2.outputscale.reshape(()),
                            self.likelihood.noise.reshape(())]).to(torch.float64)

    def _engine_step(self, theta):
        self._plan()
        if self._siter:
            return self._engine.elbo_step_scattered_iter(self._Y, self._yy, theta, n_probes=self.n_probes, tol=self.tol,
                                                         max_iter=self.max_iter)
        if self._scattered:
            return self._engine.elbo_step_scattered(self._Y, self._yy, theta)
        if self._iter:
            return self._engine.elbo_step_masked_iter(self._Y, self._W, self._nobs, self._yy, theta, n_probes=self.n_probes,
                                                      tol=self.tol, max_iter=self.max_iter)
        if self._masked:
            return self._engine.elbo_step_masked(self._Y, self._W, self._nobs, self._yy, theta)
        return self._engine.elbo_step(self._Y, self._yy, theta)

    # -- reference API ---------------------------------------------------------------------------
    def _elbo(self) -> torch.Tensor:
        """kronecker_structure.py:249-278 (collapsed Titsias bound at the optimal q(u))."""
        return _ElboFunction.apply(self._theta(), self)

    def _refresh(self):
        """q_v()/posterior() read the engine state of the CURRENT hyper-parameters."""
        with torch.no_grad():
            _ElboFunction.apply(self._theta(), self)

    def q_v(self) -> MultivariateNormal:
        """gridded_kronecker_structure.py:1409-1433 == kronecker_structure.py:825-849.
        mean is flat (M,) with u = i1*m2 + i2 (callers do `.mean.reshape(m, m).T`).
        `.sample(torch.Size([S]), seed=None)` draws joint samples [S, M]: on a full grid from the step's Kronecker eigenbasis
        (Engine.qv_sample), on the iterative solvers by one block PCG solve per 64 samples (Engine.qv_sample_masked_iter /
        qv_sample_scattered_iter; no solve runs before sample() is called, last_readout_info holds its PCG counts), on the dense masked /
        scattered states from covariance_matrix up to M = 4096 -- or, with dense_samples=True, from the step's inverse factor at any M
        (Engine.qv_sample_masked).  Out of scope (sample raises NotImplementedError): the gridded q_v() of
        the Gridded* classes (v != u), the point-wise posterior(x*) (posterior_grid() samples maps), paired inducing points, the 1-D
        classes, the exact GP; multi-rank engines refuse."""
        self._refresh()
        if self._siter and self.scattered_variances:         # the mean now, the variance of all M cells on first use (as below)
            def svar():
                self._refresh()          # the engine may have been re-planned by another model since
                _, v, self.last_readout_info = self._engine.qv_var_scattered_iter(tol=self.tol, max_iter=self.max_iter)
                return v.cpu()
            return MultivariateNormal(self._engine.qv_scattered_iter().reshape(-1).cpu(), svar, sample_fn=self._engine_sampler())
        if self._siter:                  # iterative scattered solver: the mean only (no solve); joint samples cost one solve per 64
            return MultivariateNormal(self._engine.qv_scattered_iter().reshape(-1).cpu(), self._scattered_iter_variance,
                                      cov_fn=self._scattered_iter_variance, sample_fn=self._engine_sampler())
        if self._iter:
            # iterative solver: the mean needs no solve and comes now; the variance of all M cells costs ceil(M / 64) block PCG
            # solves and is computed on first use (q_v_at gives it for a few cells); there is no dense covariance
            mean, _, _ = self._engine.qv_masked_iter(self._W, self._nobs, variance=False)

            def var():
                self._refresh()          # the engine may have been re-planned by another model since
                return self._engine.qv_masked_iter(self._W, self._nobs, tol=self.tol, max_iter=self.max_iter)[1].cpu()
            return MultivariateNormal(mean.reshape(-1).cpu(), var, sample_fn=self._engine_sampler())
        if self._masked:
            mean, var = self._engine.qv_masked()
            qv = MultivariateNormal(mean.reshape(-1).cpu(), var.reshape(-1).cpu(),
                                    cov_fn=lambda: self._engine.qv_cov_masked().cpu())
            if not self._engine.paired:  # (paired inducing points: no sampler)
                qv._sample_fn = self._dense_engine_sampler() if self.dense_samples else self._dense_sampler(qv)
            return qv
        mean, var = self._engine.qv()
        return MultivariateNormal(mean.reshape(-1).cpu(), var.reshape(-1).cpu(),
                                  cov_fn=lambda: self._engine.qv_cov().cpu(), sample_fn=self._engine_sampler())

    def _engine_sampler(self):
        """q_v().sample on a full grid and on the iterative solvers: Engine.qv_sample* (n, seed, first) -> [n, M] on the host.  No
        solve happens before sample() is called; the iterative solvers leave their PCG counts in last_readout_info."""
        def fn(n, seed, first):
            self._refresh()              # the engine may have been re-planned by another model since
            eng = self._engine
            if self._siter:
                out, self.last_readout_info = eng.qv_sample_scattered_iter(n, seed, first, tol=self.tol, max_iter=self.max_iter)
            elif self._iter:
                out, self.last_readout_info = eng.qv_sample_masked_iter(self._W, self._nobs, n, seed, first, tol=self.tol,
                                                                        max_iter=self.max_iter)
            else:
                out = eng.qv_sample(n, seed, first)
            return out.reshape(n, -1).cpu()
        return fn

    def _dense_sampler(self, qv: MultivariateNormal):
        """q_v().sample on the dense masked / scattered states: in torch from the dense covariance (no new kernel), M <= 4096; the
        standard normals are the engine's counter-based ones (stream 0, idx = s M + u), so a seed means the same noise everywhere."""
        M = qv.mean.numel()

        def fn(n, seed, first):
            if M > 4096:
                which = "scattered_solver='iterative'" if self._scattered else "solver='iterative'"
                raise NotImplementedError(f"{type(self).__name__}: joint samples from the dense covariance stop at M = 4096 (M = {M}); "
                                          f"build the model with {which}, whose sampler needs no M x M matrix")
            eps = self._engine.normal_fill(seed, 0, first * M, n * M).reshape(n, M).cpu()
            return qv.mean[None, :] + eps @ _symmetric_root(qv.covariance_matrix)
        return fn

    def _dense_engine_sampler(self):
        """q_v().sample on the dense masked / scattered states with dense_samples=True: Engine.qv_sample_masked (n, seed, first) ->
        [n, M] on the host, any M the dense solver takes; nothing is solved (last_readout_info: zero counts)."""
        def fn(n, seed, first):
            self._refresh()              # the engine may have been re-planned by another model since
            out, self.last_readout_info = self._engine.qv_sample_masked(n, seed, first)
            return out.reshape(n, -1).cpu()
        return fn

    def q_v_at(self, cells) -> MultivariateNormal:
        """q(v) at a subset of the cells (flat indices u = i1*m2 + i2): mean and variance.  On the iterative solver this costs
        ceil(len(cells) / 64) block solves instead of the ceil(M / 64) of q_v().variance; elsewhere it indexes q_v()."""
        idx = torch.as_tensor(cells, dtype=torch.int64).reshape(-1)
        self._plan()
        if not (self._iter or self._siter):
            qv = self.q_v()
            return MultivariateNormal(qv.mean[idx], qv.variance[idx])
        self._refresh()
        if self._siter:                  # (an explicit request: whatever scattered_variances says)
            mean, var, self.last_readout_info = self._engine.qv_var_scattered_iter(cells=idx, tol=self.tol, max_iter=self.max_iter)
        else:
            mean, var, _ = self._engine.qv_masked_iter(self._W, self._nobs, cells=idx, tol=self.tol, max_iter=self.max_iter)
        return MultivariateNormal(mean.reshape(-1).cpu()[idx], var.cpu())

    def posterior(self, x_star: torch.Tensor) -> MultivariateNormal:
        """kronecker_structure.py:199-230: mean and variance at x_star (N*, 2); `.covariance_matrix` (the reference's dense
        N* x N* matrix, :223-229) is materialised on first access (vggp_posterior_cov: N* <= 8192, M N* <= 2^27)."""
        self._refresh()
        xs = torch.as_tensor(x_star, dtype=torch.float64)
        if self._siter and self.scattered_variances:          # (no dense covariance, as on the iterative masked solver)
            mean, var, self.last_readout_info = self._engine.posterior_var_scattered_iter(xs, tol=self.tol, max_iter=self.max_iter)
            return MultivariateNormal(mean.cpu(), var.cpu())
        if self._siter:
            return MultivariateNormal(self._engine.posterior_scattered_iter(xs).cpu(), self._scattered_iter_variance,
                                      cov_fn=self._scattered_iter_variance)
        if self._iter:                   # (no dense covariance on the iterative solver: .covariance_matrix raises)
            mean, var, _ = self._engine.posterior_masked_iter(xs, self._W, self._nobs, tol=self.tol, max_iter=self.max_iter)
            return MultivariateNormal(mean.cpu(), var.cpu())
        post = self._engine.posterior_masked if self._masked else self._engine.posterior
        mean, var = post(xs)

        def cov():
            self._refresh()          # the engine may have been re-planned by another model since
            return self._engine.posterior_cov(xs, masked=self._masked).cpu()
        return MultivariateNormal(mean.cpu(), var.cpu(), cov_fn=cov)

    def posterior_predictive(self, x_star: torch.Tensor) -> MultivariateNormal:
        """kronecker_structure.py:232-247: the likelihood adds the noise variance."""
        p = self.posterior(x_star)
        noise = self.likelihood.noise.detach().to(p.variance.dtype)
        return MultivariateNormal(p.mean, p.variance + noise,
                                  cov_fn=lambda: p.covariance_matrix + noise * torch.eye(p.mean.shape[0], dtype=p.variance.dtype))

    def posterior_grid(self, x1_star: torch.Tensor, x2_star: torch.Tensor, raster_variance: bool = False) -> MultivariateNormal:
        """posterior(torch.cartesian_prod(x1_star, x2_star)) for a map: the raster of two coordinate axes (the meshgrid cells of the
        reference's notebooks), flat index a * P2 + b.  Mean and variance come from Engine.posterior_raster, O(P1 P2 m) instead of
        O(P1 P2 m^2); there is no dense covariance (`.covariance_matrix` raises).  On a grid with holes, on scattered points and on the
        iterative solvers the raster entry gives the mean; the variance then comes from that state's point-wise route (posterior()), on
        the first use of `.variance`.  raster_variance=True on a dense masked / scattered state takes `.variance` from
        Engine.posterior_raster_var_masked instead (the separable contraction against the state's Sinv: O(P1 M^2 + P1 P2 m2^2), not
        O(P1 P2 M^2); equal to the point-wise route to rounding, not bit for bit), lazily as well; it changes nothing on a full grid
        (the raster variance is what is returned there) and raises NotImplementedError on the iterative solvers, which keep no Sinv.
        `.sample(torch.Size([S]), seed=None)` draws JOINT samples [S, P1 P2] of the map on full grids and on both iterative solvers
        (Engine.posterior_raster_sample*: per-axis Cholesky roots of the prior residual, P_d <= 8192, no P1 P2 x P1 P2 matrix; a fixed
        nugget of 1e-8 at unit outputscale).  It raises NotImplementedError on the dense masked / scattered states (build the model with
        solver='iterative' resp. scattered_solver='iterative', or with dense_samples=True: Engine.posterior_raster_sample_masked) and
        for B1 hat features (indefinite residual)."""
        self._refresh()
        a1 = torch.as_tensor(x1_star, dtype=torch.float64).reshape(-1)
        a2 = torch.as_tensor(x2_star, dtype=torch.float64).reshape(-1)
        if self._engine.paired:
            raise NotImplementedError(f"{type(self).__name__}: posterior_grid needs Kronecker inducing features; paired inducing points "
                                      f"have none -- use posterior(torch.cartesian_prod(x1_star, x2_star))")

        def no_cov():
            raise NotImplementedError("posterior_grid has no dense covariance (a raster of P1 P2 points); use .variance, or posterior() "
                                      "on a few points for its .covariance_matrix")
        sampler = self._raster_sampler(a1, a2)
        if not (self._masked or self._scattered):
            mean, var = self._engine.posterior_raster(a1, a2)
            return MultivariateNormal(mean.reshape(-1).cpu(), var.reshape(-1).cpu(), cov_fn=no_cov, sample_fn=sampler)
        if raster_variance and (self._iter or self._siter):
            raise NotImplementedError(f"{type(self).__name__}: raster_variance=True needs the dense Sinv of the masked / scattered step; "
                                      f"the iterative solvers keep none -- use posterior(torch.cartesian_prod(x1_star, x2_star)).variance")
        mean, _ = self._engine.posterior_raster(a1, a2, want_var=False)

        def var():                       # (posterior() refreshes the state itself; means-only scattered models raise here as there)
            if raster_variance:
                self._refresh()          # the engine may have been re-planned by another model since
                return self._engine.posterior_raster_var_masked(a1, a2)[1].reshape(-1).cpu()
            return self.posterior(torch.cartesian_prod(a1, a2)).variance
        return MultivariateNormal(mean.reshape(-1).cpu(), var, cov_fn=no_cov, sample_fn=sampler)

    def _raster_sampler(self, a1: torch.Tensor, a2: torch.Tensor, predictive: bool = False):
        """posterior_grid().sample on a full grid and on the iterative solvers: Engine.posterior_raster_sample* (n, seed, first) ->
        [n, P1 P2] on the host, flat index a P2 + b; sample s of a seed shares its coefficient noise with sample s of q_v().  No root and
        no solve happens before sample() is called; the iterative solvers leave their PCG counts in last_readout_info (the dense states
        with dense_samples=True: Engine.posterior_raster_sample_masked, zero counts).  predictive: plus sqrt(noise) times the engine's stream 4 (idx = s P1 P2 + a P2 + b).  The states that have no raster sampler get a function
        that raises NotImplementedError with the way out."""
        name = type(self).__name__
        if self._basis()[0] == "b1":
            def refuse(n, seed, first):
                raise NotImplementedError(f"{name}: joint samples of posterior_grid are not available for B1 hat features: the prior "
                                          "residual k - q of that basis is indefinite, so the raster covariance has no Kronecker root")
            return refuse
        dense = (self._masked or self._scattered) and not (self._iter or self._siter)      # the dense M-space states
        if dense and not self.dense_samples:
            which = "scattered_solver='iterative'" if self._scattered else "solver='iterative'"

            def refuse(n, seed, first):
                raise NotImplementedError(f"{name}: joint samples of posterior_grid need the whitened coefficient draw of the iterative "
                                          f"state; build the model with {which}")
            return refuse
        P = a1.numel() * a2.numel()

        def fn(n, seed, first):
            self._refresh()              # the engine may have been re-planned by another model since
            eng = self._engine
            if dense:
                out, self.last_readout_info = eng.posterior_raster_sample_masked(a1, a2, n, seed, first)
            elif self._siter:
                out, self.last_readout_info = eng.posterior_raster_sample_scattered_iter(a1, a2, n, seed, first, tol=self.tol,
                                                                                         max_iter=self.max_iter)
            elif self._iter:
                out, self.last_readout_info = eng.posterior_raster_sample_masked_iter(a1, a2, self._W, self._nobs, n, seed, first,
                                                                                      tol=self.tol, max_iter=self.max_iter)
            else:
                out, _ = eng.posterior_raster_sample(a1, a2, n, seed, first)
            out = out.reshape(n, P)
            if predictive:
                noise = self.likelihood.noise.detach().to(torch.float64).reshape(()).item()
                out = out + noise ** 0.5 * eng.normal_fill(seed, 4, first * P, n * P).reshape(n, P)
            return out.cpu()
        return fn

    def posterior_predictive_grid(self, x1_star: torch.Tensor, x2_star: torch.Tensor, raster_variance: bool = False) -> MultivariateNormal:
        """posterior_grid with the likelihood's noise variance added (kronecker_structure.py:232-247 on a raster).  `.sample()` draws
        the samples posterior_grid().sample() draws for the seed, plus independent observation noise.  raster_variance: as posterior_grid."""
        p = self.posterior_grid(x1_star, x2_star, raster_variance=raster_variance)
        noise = self.likelihood.noise.detach().to(torch.float64)
        variance = p._variance
        a1 = torch.as_tensor(x1_star, dtype=torch.float64).reshape(-1)
        a2 = torch.as_tensor(x2_star, dtype=torch.float64).reshape(-1)
        return MultivariateNormal(p.mean, (lambda: p.variance + noise) if callable(variance) else variance + noise, cov_fn=p._cov_fn,
                                  sample_fn=self._raster_sampler(a1, a2, predictive=True))

    # -- dense views kept for small sizes / debugging (the hot path never forms them) ------------------------------
    def _factor(self, d: int, x: torch.Tensor):
        """Unit-outputscale per-dimension factors from the engine: A0 (m x n at coordinates x), K0 (m x m)."""
        basis, g1, g2 = self._basis()
        ell = (self.kernel_1 if d == 0 else self.kernel_2).base_kernel.lengthscale.reshape(()).item()
        grid = torch.as_tensor(g1 if d == 0 else g2, dtype=torch.float64, device=self._engine.device)
        xs = torch.as_tensor(x, dtype=torch.float64, device=self._engine.device).contiguous()
        flags = 1 if (basis == "b0" and self._f32_mesh()) else 0          # ("b0k" never carries the float32 flag)
        A, _, K, _ = self._engine.factor_build(self.kind, basis, xs, grid, ell, flags)
        return A, K

    def _Kuu_along_dim(self, d: int) -> torch.Tensor:
        """kronecker_structure.py:702-739 (B0) / :318-319 (points): m_d x m_d, outputscale applied (no jitter)."""
        s = (self.kernel_1 if d == 0 else self.kernel_2).outputscale.detach().to(torch.float64)
        _, K = self._factor(d, torch.zeros(1, dtype=torch.float64))
        if self._basis()[0] in ("vff", "b1"):          # inter-domain features: Kuu_d = K0 / s_d
            return (K / s.to(K.device)).cpu()
        return (s.to(K.device) * K).cpu()

    def _Kuf_along_dim(self, d: int, x: torch.Tensor) -> torch.Tensor:
        """kronecker_structure.py:741-790 (B0) / :336-337 (points): m_d x len(x)."""
        s = (self.kernel_1 if d == 0 else self.kernel_2).outputscale.detach().to(torch.float64)
        A, _ = self._factor(d, x)
        if self._basis()[0] in ("vff", "b1"):          # ... and Kuf_d carries no outputscale
            return A.cpu()
        return (s.to(A.device) * A).cpu()

    def _Kuu(self) -> torch.Tensor:
        """kronecker_structure.py:792-806: torch.kron(Kuu_1, Kuu_2), M x M dense -- small M only."""
        K1, K2 = self._Kuu_along_dim(0), self._Kuu_along_dim(1)
        if K1.shape[0] * K2.shape[0] > 8192:
            raise ValueError("_Kuu(): M = m1*m2 > 8192; the dense matrix is for small sizes / debugging only")
        return torch.kron(K1, K2)

    def _Kuf(self, x: torch.Tensor) -> torch.Tensor:
        """kronecker_structure.py:808-823: row-wise Khatri-Rao of the per-dimension factors, M x N, u = i1*m2 + i2."""
        x = torch.as_tensor(x, dtype=torch.float64)
        A1, A2 = self._Kuf_along_dim(0, x[:, 0]), self._Kuf_along_dim(1, x[:, 1])
        if A1.shape[0] * A2.shape[0] * x.shape[0] > (1 << 27):
            raise ValueError("_Kuf(): M*N too large for the dense matrix (small sizes / debugging only)")
        return (A1[:, None, :] * A2[None, :, :]).reshape(-1, x.shape[0])

    def _sigma(self) -> torch.Tensor:
        """kronecker_structure.py:134-150: Kuu + Kuf Kuf^T / sigma^2 (dense; debugging only)."""
        Kuf = self._Kuf(self.train_inputs[0])
        return self._Kuu() + Kuf @ Kuf.T / self.likelihood.noise.detach().to(torch.float64).cpu()

    def prior(self, x: torch.Tensor) -> MultivariateNormal:
        """kronecker_structure.py:90-103: zero mean, product kernel k1(x1,x1') k2(x2,x2') -- dense N x N, small N only."""
        x = torch.as_tensor(x, dtype=torch.float64)
        if x.shape[0] > 8192:
            raise ValueError("prior(): dense N x N covariance, N <= 8192")
        cov = torch.ones(x.shape[0], x.shape[0], dtype=torch.float64)
        for d, k in ((0, self.kernel_1), (1, self.kernel_2)):
            r = (x[:, d, None] - x[None, :, d]).abs() / k.base_kernel.lengthscale.reshape(()).item()
            kind = k.base_kernel.kind
            if kind == "matern12":
                kd = torch.exp(-r)
            elif kind == "matern32":
                kd = (1 + math.sqrt(3) * r) * torch.exp(-math.sqrt(3) * r)
            elif kind == "matern52":
                kd = (1 + math.sqrt(5) * r + 5 * r * r / 3) * torch.exp(-math.sqrt(5) * r)
            else:
                kd = torch.exp(-0.5 * r * r)
            cov = cov * k.outputscale.detach().to(torch.float64) * kd
        return MultivariateNormal(torch.zeros(x.shape[0], dtype=torch.float64), torch.diagonal(cov).clone(), cov_fn=lambda: cov)

    def non_informative_initialise(self, lmbda: float, kappa: float) -> None:
        """kronecker_structure.py:34-61.  As in the reference, the `lengthscale[0] = ...` assignments go
        through the property getter and leave the raw lengthscale untouched (documented quirk)."""
        X, y = self.train_inputs[0], self.train_targets
        self.kernel_1.outputscale = y.var()
        self.kernel_1.base_kernel.lengthscale[0] = (X[:, 0].std() / lmbda)
        self.kernel_2.outputscale = y.var()
        self.kernel_2.base_kernel.lengthscale[0] = (X[:, 1].std() / lmbda)
        self.likelihood.noise = ((self.kernel_1.outputscale + self.kernel_2.outputscale) / 2) / (kappa ** 2)

    def informative_initialise(self, prior_amplitude: float, lmbda: float) -> None:
        """kronecker_structure.py:63-88."""
        X, y = self.train_inputs[0], self.train_targets
        self.kernel_1.outputscale = (torch.tensor(prior_amplitude) / 2) ** 2
        self.kernel_1.base_kernel.lengthscale[0] = (X[:, 0].std() / lmbda)
        self.kernel_2.outputscale = (torch.tensor(prior_amplitude) / 2) ** 2
        self.kernel_2.base_kernel.lengthscale[0] = (X[:, 1].std() / lmbda)
        self.likelihood.noise = y.var() - ((self.kernel_1.outputscale + self.kernel_2.outputscale) / 2)

    # convenience: the notebooks' fit loop / grid prediction
    def fit(self, n_iter: int = 100, lr: float = 0.01):
        opt = torch.optim.Adam(self.parameters(), lr=lr)
        history = torch.empty(n_iter)
        for i in range(n_iter):
            opt.zero_grad()
            loss = -self._elbo()
            history[i] = loss.item()
            loss.backward()
            opt.step()
        return history

    def predict(self) -> MultivariateNormal:
        return self.q_v()


class _B0Gridded(KroneckerStructure):
    def __init__(self, X, y, nknots: int, dim1lims: Tuple[float, float], dim2lims: Tuple[float, float], **kw):
        super().__init__(X, y, **kw)
        self.nknots = nknots
        self.dim1lims, self.dim2lims = dim1lims, dim2lims
        self.mesh_1 = torch.linspace(dim1lims[0], dim1lims[1], nknots)   # default dtype, as the reference
        self.mesh_2 = torch.linspace(dim2lims[0], dim2lims[1], nknots)
        self.delta_1 = self.mesh_1[1] - self.mesh_1[0]
        self.delta_2 = self.mesh_2[1] - self.mesh_2[0]
        self.b0_mesh_1, self.b0_mesh_2 = self.mesh_1, self.mesh_2
        # gridded_kronecker_structure.py:1283-1284 / kronecker_structure.py:698-699 (bspline.py:81-103)
        self.basis_1 = B0SplineBasis(self.mesh_1, self._engine, kind=self.kind)
        self.basis_2 = B0SplineBasis(self.mesh_2, self._engine, kind=self.kind)

    def _basis(self):
        return "b0", self.mesh_1.double().numpy(), self.mesh_2.double().numpy()


class Matern12GriddedGP(_B0Gridded):
    """gridded_kronecker_structure.py:1255-1433 (the flagship model)."""


class Matern12B0SplineGriddedGP(_B0Gridded):
    """kronecker_structure.py:671-849 (identical maths)."""


class _B0KGridded(_B0Gridded):
    """The gridded model on the cells of VGGP_BASIS_B0K: the inducing features are the integrals of a Matern-3/2 or -5/2 process over
    the B0 cells, so q_v() is the gridded product of a once- or twice-differentiable field.  The reference has no such model: there is
    no float32 mesh arithmetic to reproduce, and the mesh enters as mesh.double()."""

    def _basis(self):
        return "b0k", self.mesh_1.double().numpy(), self.mesh_2.double().numpy()

    def _f32_mesh(self) -> bool:
        return False


class Matern32GriddedGP(_B0KGridded):
    kind = "matern32"


class Matern52GriddedGP(_B0KGridded):
    kind = "matern52"


Matern32B0SplineGriddedGP = Matern32GriddedGP
Matern52B0SplineGriddedGP = Matern52GriddedGP


class Matern12VFFGP(KroneckerStructure):
    """kronecker_structure.py:346-515: variational Fourier features, Matern-1/2.  Kuu_d = diag(alpha) + beta beta^T (:400-462,
    scales with 1/s_d), Kuf_d = Fourier basis (fourier.py:14-88, no s_d): only the per-dimension factors differ."""

    def __init__(self, X, y, nfrequencies: int, dim1lims: Tuple[float, float], dim2lims: Tuple[float, float], **kw):
        super().__init__(X, y, **kw)
        self.nfrequencies = nfrequencies
        self.dim1lims, self.dim2lims = dim1lims, dim2lims
        # fourier.py:13, float32 like the reference (python float * int64 arange / python float)
        self.omegas_1 = (2 * torch.pi) * torch.arange(nfrequencies + 1) / (dim1lims[1] - dim1lims[0])
        self.omegas_2 = (2 * torch.pi) * torch.arange(nfrequencies + 1) / (dim2lims[1] - dim2lims[0])

    @property
    def basis_1(self) -> FourierBasisMatern12:
        """kronecker_structure.py:464-470: the Fourier basis at the CURRENT lengthscale (the reference rebuilds it per call)."""
        return FourierBasisMatern12(self.nfrequencies, self.dim1lims[0], self.dim1lims[1],
                                    self.kernel_1.base_kernel.lengthscale.reshape(()).item(), self._engine)

    @property
    def basis_2(self) -> FourierBasisMatern12:
        return FourierBasisMatern12(self.nfrequencies, self.dim2lims[0], self.dim2lims[1],
                                    self.kernel_2.base_kernel.lengthscale.reshape(()).item(), self._engine)

    def _basis(self):
        g1 = np.concatenate([[self.dim1lims[0], self.dim1lims[1]], self.omegas_1.double().numpy()])
        g2 = np.concatenate([[self.dim2lims[0], self.dim2lims[1]], self.omegas_2.double().numpy()])
        return "vff", g1, g2


def _gridded_q_v(model, literal: bool, cells=None) -> MultivariateNormal:
    """q(v) of the B0 cell features on the output grid of a Gridded* model, from the engine state of the current hyper-parameters
    (flat index a * nsplines + b; `cells`: only those).  Dense solvers: vggp_readout / vggp_readout_masked.  Iterative solvers
    (solver= / scattered_solver=): vggp_readout_masked_iter / vggp_readout_scattered_iter -- literal=True is a Gram product over the
    data and comes at once; literal=False costs ceil(cells / 64) block PCG solves, so without `cells` the mean comes now and the
    variance on first use, and there is no dense covariance."""
    model._refresh()
    C1, C2, kd1, kd2 = model._readout_operands()
    idx = None if cells is None else torch.as_tensor(cells, dtype=torch.int64).reshape(-1)
    if not (model._siter or model._iter):
        mean, var = model._engine.readout(C1, C2, kd1, kd2, literal=literal, masked=model._masked)
        mean, var = mean.reshape(-1).cpu(), var.reshape(-1).cpu()
        return MultivariateNormal(mean, var) if idx is None else MultivariateNormal(mean[idx], var[idx])

    def run(variance: bool):
        kw = dict(literal=literal, cells=idx, variance=variance, tol=model.tol, max_iter=model.max_iter)
        if model._siter:
            return model._engine.readout_scattered_iter(C1, C2, kd1, kd2, **kw)
        return model._engine.readout_masked_iter(C1, C2, kd1, kd2, model._W, model._nobs, **kw)
    if literal or idx is not None:
        mean, var, model.last_readout_info = run(True)
        mean = mean.reshape(-1).cpu()
        return MultivariateNormal(mean if idx is None else mean[idx], var.cpu())
    mean = run(False)[0]

    def var():
        model._refresh()                 # the engine may have been re-planned by another model since
        _, v, model.last_readout_info = run(True)
        return v.cpu()
    return MultivariateNormal(mean.reshape(-1).cpu(), var)


def _b0_kvv_diag_unit(delta: float, ell: float) -> float:
    """diag of the unit-outputscale B0 Gram matrix (gridded_kronecker_structure.py:341-394): ell^2 * 2 (e^{-d/l} + d/l - 1)."""
    r = delta / ell
    return ell * ell * 2.0 * (math.exp(-r) + r - 1.0)


class GriddedMatern12VFFGP(Matern12VFFGP):
    """gridded_kronecker_structure.py:470-654: the VFF model with a gridded read-out -- q_v() is the distribution of the
    B0 cell features v on an nsplines x nsplines grid, obtained from the inducing posterior q(u) through p(v | u).
    Mean and variance come from `vggp_readout` (Kronecker in the per-dimension cross-covariances :499-555); the variance is
    the reference's own expression (:431, literal=True) unless literal=False is asked for."""

    def __init__(self, X, y, nfrequencies: int, vffdim1lims, vffdim2lims, nsplines: int, griddim1lims, griddim2lims, **kw):
        super().__init__(X, y, nfrequencies, vffdim1lims, vffdim2lims, **kw)
        self.nsplines = nsplines
        self.nknots = nsplines + 1
        self.griddim1lims, self.griddim2lims = griddim1lims, griddim2lims
        self.mesh_1 = torch.linspace(griddim1lims[0], griddim1lims[1], self.nknots)
        self.mesh_2 = torch.linspace(griddim2lims[0], griddim2lims[1], self.nknots)
        self.delta_1 = self.mesh_1[1] - self.mesh_1[0]
        self.delta_2 = self.mesh_2[1] - self.mesh_2[0]

    @staticmethod
    def _Kvu_along_dim(mesh: torch.Tensor, a: float, omegas: torch.Tensor) -> torch.Tensor:
        """:499-541: cell integrals of 1, cos(w (t - a)), sin(w (t - a)); (nsplines, 2M + 1), no hyper-parameter."""
        me, om = mesh.double(), omegas.double()
        k0 = torch.ones(me.shape[0] - 1, 1, dtype=torch.float64) * (me[1] - me[0])
        kc = (torch.sin(om[1:] * (me[1:] - a)[:, None]) - torch.sin(om[1:] * (me[:-1] - a)[:, None])) / om[1:]
        ks = -(torch.cos(om[1:] * (me[1:] - a)[:, None]) - torch.cos(om[1:] * (me[:-1] - a)[:, None])) / om[1:]
        return torch.cat([k0, kc, ks], dim=1)

    def q_u(self) -> MultivariateNormal:
        """:613-624 -- the posterior over the Fourier features (what the parent class calls q_v)."""
        return super().q_v()

    def _readout_operands(self):
        """C_d (nsplines x m_d) and the unit diagonals of Kvv_d at the current lengthscales."""
        C1 = self._Kvu_along_dim(self.mesh_1, self.dim1lims[0], self.omegas_1)
        C2 = self._Kvu_along_dim(self.mesh_2, self.dim2lims[0], self.omegas_2)
        l1 = self.kernel_1.base_kernel.lengthscale.reshape(()).item()
        l2 = self.kernel_2.base_kernel.lengthscale.reshape(()).item()
        kd1 = torch.full((self.nsplines,), _b0_kvv_diag_unit(float(self.delta_1.double()), l1), dtype=torch.float64)
        kd2 = torch.full((self.nsplines,), _b0_kvv_diag_unit(float(self.delta_2.double()), l2), dtype=torch.float64)
        return C1, C2, kd1, kd2

    def q_v(self, psd: bool = True, literal: bool = True) -> MultivariateNormal:
        """:634-654 (mean and the diagonal of the covariance; flat index a * nsplines + b).  On the iterative solvers see
        _gridded_q_v: literal=False computes the variance on first use."""
        return _gridded_q_v(self, literal)

    def q_v_cells(self, cells, literal: bool = False) -> MultivariateNormal:
        """q_v() at a list of output cells (flat indices a * nsplines + b): on the iterative solvers ceil(len(cells) / 64) block
        solves for literal=False; elsewhere it indexes q_v().  (q_v_at is the parent's: cells of the inducing features.)"""
        return _gridded_q_v(self, literal, cells)


def _b0_cross_points(mesh: torch.Tensor, z: torch.Tensor, ell: float) -> torch.Tensor:
    """Unit-outputscale Cov(v_k, f(z)) for B0 cells on `mesh` (gridded_kronecker_structure.py:281-321): (nsplines, len(z)).
    Host-side set-up of the read-out (a few hundred numbers); cell k = (mesh[k], mesh[k+1]] like searchsorted(right=False)."""
    me, zz = mesh.double(), z.double()
    a, b = me[:-1, None], me[1:, None]
    E1, E2 = ell * torch.exp(-(zz[None, :] - a).abs() / ell), ell * torch.exp(-(zz[None, :] - b).abs() / ell)
    inside = (zz[None, :] > a) & (zz[None, :] <= b)
    sign = torch.where(zz[None, :] <= a, 1.0, -1.0)
    return torch.where(inside, 2 * ell - (E1 + E2), sign * (E1 - E2))


class _GriddedReadout:
    """q_u -> p(v | u) -> q_v on an nsplines x nsplines B0 grid through vggp_readout (mixin of the Gridded* classes)."""

    def _grid_init(self, nsplines: int, griddim1lims, griddim2lims):
        self.n_b0_splines = self.nsplines = nsplines
        self.dim1_grid_lims, self.dim2_grid_lims = griddim1lims, griddim2lims
        self.b0_mesh_1 = torch.linspace(griddim1lims[0], griddim1lims[1], nsplines + 1)
        self.b0_mesh_2 = torch.linspace(griddim2lims[0], griddim2lims[1], nsplines + 1)
        self.b0_delta_1 = self.b0_mesh_1[1] - self.b0_mesh_1[0]
        self.b0_delta_2 = self.b0_mesh_2[1] - self.b0_mesh_2[0]
        self.b0_basis_1 = B0SplineBasis(self.b0_mesh_1, self._engine)
        self.b0_basis_2 = B0SplineBasis(self.b0_mesh_2, self._engine)

    def _cross(self, d: int, ell: float) -> torch.Tensor:        # C_d (nsplines x m_d) at unit outputscale
        raise NotImplementedError

    def q_u(self) -> MultivariateNormal:
        """The posterior over the inducing features (what the Kronecker base class calls q_v)."""
        return KroneckerStructure.q_v(self)

    def _readout_operands(self):
        l1 = self.kernel_1.base_kernel.lengthscale.reshape(()).item()
        l2 = self.kernel_2.base_kernel.lengthscale.reshape(()).item()
        kd1 = torch.full((self.nsplines,), _b0_kvv_diag_unit(float(self.b0_delta_1.double()), l1), dtype=torch.float64)
        kd2 = torch.full((self.nsplines,), _b0_kvv_diag_unit(float(self.b0_delta_2.double()), l2), dtype=torch.float64)
        return self._cross(0, l1), self._cross(1, l2), kd1, kd2

    def q_v(self, psd: bool = True, literal: bool = True) -> MultivariateNormal:
        """mean and the diagonal of the covariance of the B0 cell features (flat index a * nsplines + b); the variance is the
        reference's own expression (literal=True) unless literal=False asks for the conditional variance under q(u) -- on the
        iterative solvers that one is computed on first use (see _gridded_q_v)."""
        return _gridded_q_v(self, literal)

    def q_v_cells(self, cells, literal: bool = False) -> MultivariateNormal:
        """q_v() at a list of output cells (flat indices a * nsplines + b): on the iterative solvers ceil(len(cells) / 64) block
        solves for literal=False; elsewhere it indexes q_v().  (q_v_at is the base class's: cells of the inducing features.)"""
        return _gridded_q_v(self, literal, cells)


class Matern12B1SplineASVGP(KroneckerStructure):
    """kronecker_structure.py:524-660: B1-spline (hat function) inducing features, Matern-1/2.
    Kuu_d = (A ell + B / ell + BC) / (2 s_d) (:560-614, tridiagonal), Kuf_d = hats(x) (:616-628)."""

    def __init__(self, X, y, nknots: int, dim1lims: Tuple[float, float], dim2lims: Tuple[float, float], **kw):
        super().__init__(X, y, **kw)
        self.nknots = nknots
        self.dim1lims, self.dim2lims = dim1lims, dim2lims
        self.mesh_1 = torch.linspace(dim1lims[0], dim1lims[1], nknots)
        self.mesh_2 = torch.linspace(dim2lims[0], dim2lims[1], nknots)
        self.delta_1 = self.mesh_1[1] - self.mesh_1[0]
        self.delta_2 = self.mesh_2[1] - self.mesh_2[0]
        self.delta = self.delta_1
        self.basis_1 = B1SplineBasis(self.mesh_1, self._engine)      # kronecker_structure.py:548-549
        self.basis_2 = B1SplineBasis(self.mesh_2, self._engine)

    def _basis(self):
        return "b1", self.mesh_1.double().numpy(), self.mesh_2.double().numpy()

    def _f32_mesh(self) -> bool:
        return False                 # the float32 (k*delta) quirk belongs to the B0 closed forms only


class Matern12SVGP(KroneckerStructure):
    """kronecker_structure.py:287-338: Z (m, 2) holds the per-dimension inducing coordinates; the inducing set
    is cartesian_prod(Z[:,0], Z[:,1]) (:336), so Kuu = kron(K1(Z[:,0]), K2(Z[:,1])) (:318-321).
    Z is a trainable Parameter as in the reference (:303-304): `_elbo()` carries its analytic gradient (vggp_zgrad) unless
    `train_z=False`.  Moved inducing points reach the engine through vggp_set_inducing (no re-plan: graphs and warm start stay).  On
    incomplete data (scattered points, or a grid with holes, which is then treated as its observed points) the gradient is
    vggp_zgrad_scattered's."""

    def __init__(self, X, y, Z: torch.Tensor, train_z: bool = True, **kw):
        super().__init__(X, y, **kw)
        self.Z = torch.nn.Parameter(torch.as_tensor(Z, dtype=torch.float64).clone(), requires_grad=bool(train_z))
        if train_z:
            self._as_scattered()

    def _elbo(self) -> torch.Tensor:
        return _ElboFunction.apply(self._theta(), self, self.Z)

    def _basis(self):
        Z = self.Z.detach().cpu().numpy()
        return "points", Z[:, 0].copy(), Z[:, 1].copy()


class Matern32SVGP(Matern12SVGP):
    kind = "matern32"


class Matern52SVGP(Matern12SVGP):
    kind = "matern52"


class RBFSVGP(Matern12SVGP):
    kind = "rbf"


# ---------------------------------------------------------------------------------------------
# 1-D models: the same engine with a trivial second factor (VGGP_BASIS_ONE)
# ---------------------------------------------------------------------------------------------
class _SparseGP1D(torch.nn.Module):
    """univariate_structure.py:15-263 (SparseGP): one factor; kernel = ScaleKernel(Matern)."""

    kind = "matern12"

    def __init__(self, X: torch.Tensor, y: torch.Tensor, engine: Optional[Engine] = None, warm_start: bool = True):
        super().__init__()
        self.train_inputs = (X,)
        self.train_targets = y
        self.likelihood = GaussianLikelihood()
        self.kernel = ScaleKernel(_BaseKernel(self.kind))
        self._engine = engine if engine is not None else Engine()
        self._warm = warm_start
        self._planned = False
        self._plan_token, self._plan_key = -1, None
        self._masked = False
        self.last_info = None
        self._x = torch.as_tensor(X, dtype=torch.float64).reshape(-1).numpy().copy()
        self._Y = torch.as_tensor(y, dtype=torch.float64).reshape(1, -1).contiguous().to(self._engine.device)
        self._yy = self._engine.sumsq(self._Y)

    def _basis(self):
        raise NotImplementedError

    def _plan(self):
        basis, g = self._basis()
        key = (basis, np.asarray(g).tobytes())
        if self._planned and self._plan_token == self._engine.plan_token and key != self._plan_key and basis == "points" \
                and self._plan_key is not None and len(self._plan_key[1]) == len(key[1]):
            self._engine.set_inducing(0, g)          # only Z moved
            self._plan_key = key
        elif not self._planned or self._plan_token != self._engine.plan_token or key != self._plan_key:
            mesh = getattr(self, "mesh", None)
            self._engine.plan(self.kind, basis, g, self._x, "matern12", "one", None, np.zeros(1), warm_start=self._warm,
                              b0_f32_kdelta=basis != "b0k" and mesh is not None and mesh.dtype == torch.float32)
            self._planned = True
            self._plan_token, self._plan_key = self._engine.plan_token, key

    def _theta(self):
        one = torch.ones((), dtype=torch.float64)
        return torch.stack([self.kernel.base_kernel.lengthscale.reshape(()).double(), one,
                            self.kernel.outputscale.reshape(()).double(), one,
                            self.likelihood.noise.reshape(()).double()])

    def _engine_step(self, theta):
        self._plan()
        if self._masked:
            return self._engine.elbo_step_masked(self._Y, self._W, self._nobs, self._yy, theta)
        return self._engine.elbo_step(self._Y, self._yy, theta)

    def _elbo(self):
        """univariate_structure.py:234-263."""
        return _ElboFunction.apply(self._theta(), self)

    def _refresh(self):
        with torch.no_grad():
            _ElboFunction.apply(self._theta(), self)

    def q_v(self) -> MultivariateNormal:
        """univariate_structure.py:693-717."""
        self._refresh()
        if self._masked:
            mean, var = self._engine.qv_masked()
            return MultivariateNormal(mean.reshape(-1).cpu(), var.reshape(-1).cpu())
        mean, var = self._engine.qv()
        return MultivariateNormal(mean.reshape(-1).cpu(), var.reshape(-1).cpu(),
                                  cov_fn=lambda: self._engine.qv_cov().cpu())

    def posterior(self, x_star) -> MultivariateNormal:
        """univariate_structure.py:184-215 (mean and diagonal)."""
        self._refresh()
        mean, var = self._engine.posterior(torch.as_tensor(x_star, dtype=torch.float64).reshape(-1))
        return MultivariateNormal(mean.cpu(), var.cpu())

    def posterior_predictive(self, x_star) -> MultivariateNormal:
        p = self.posterior(x_star)
        return MultivariateNormal(p.mean, p.variance + self.likelihood.noise.detach().to(p.variance.dtype))

    def non_informative_initialise(self, lmbda: float, kappa: float) -> None:
        """univariate_structure.py:45-66 (same lengthscale-getter quirk)."""
        X, y = self.train_inputs[0], self.train_targets
        self.kernel.outputscale = y.var()
        self.likelihood.noise = self.kernel.outputscale / (kappa ** 2)
        self.kernel.base_kernel.lengthscale[0] = (X.std() / lmbda)

    def informative_initialise(self, prior_amplitude: float, lmbda: float) -> None:
        """univariate_structure.py:68-87."""
        X, y = self.train_inputs[0], self.train_targets
        self.kernel.outputscale = (torch.tensor(prior_amplitude) / 2) ** 2
        self.likelihood.noise = y.var() - self.kernel.outputscale
        self.kernel.base_kernel.lengthscale[0] = (X.std() / lmbda)


class univariate:
    """Namespace for the 1-D classes (they share names with the 2-D ones in the reference's other module)."""

    class Matern12B0SplineGriddedGP(_SparseGP1D):
        """univariate_structure.py:721-825."""

        def __init__(self, X, y, nknots: int, dim1lims: Tuple[float, float], **kw):
            super().__init__(X, y, **kw)
            self.nknots = nknots
            self.alim, self.blim = dim1lims
            self.mesh = torch.linspace(self.alim, self.blim, nknots)
            self.delta = self.mesh[1] - self.mesh[0]
            self.n_splines = nknots - 1
            self.basis = B0SplineBasis(self.mesh, self._engine, kind=self.kind)       # univariate_structure.py:738

        def _basis(self):
            return ("b0" if self.kind == "matern12" else "b0k"), self.mesh.double().numpy()

    class Matern32B0SplineGriddedGP(Matern12B0SplineGriddedGP):
        """the 1-D twin of Matern32GriddedGP (cells of VGGP_BASIS_B0K)"""
        kind = "matern32"

    class Matern52B0SplineGriddedGP(Matern12B0SplineGriddedGP):
        kind = "matern52"

    class Matern12SVGP(_SparseGP1D):
        """univariate_structure.py:273-332."""

        def __init__(self, X, y, Z, train_z: bool = True, **kw):
            super().__init__(X, y, **kw)
            self.Z = torch.nn.Parameter(torch.as_tensor(Z, dtype=torch.float64).reshape(-1, 1).clone(),
                                        requires_grad=bool(train_z))

        def _elbo(self):
            return _ElboFunction.apply(self._theta(), self, self.Z)

        def _basis(self):
            return "points", self.Z.detach().cpu().numpy().reshape(-1).copy()

    class Matern32SVGP(Matern12SVGP):
        kind = "matern32"

    class Matern52SVGP(Matern12SVGP):
        kind = "matern52"


class GriddedMatern12SVGP(_GriddedReadout, KroneckerStructure):
    """gridded_kronecker_structure.py:222-460: inducing POINTS Z (M, 2) with a gridded read-out on B0 cells.  The reference
    evaluates the product kernel on the rows of Z (Kuu = k(Z, Z), :252-264), a Hadamard product K1 o K2.

    inducing="grid": Z lists cartesian_prod(z1, z2) (either coordinate fastest), k(Z, Z) = kron(K1, K2) and the Kronecker engine
    runs; Z stays frozen.  inducing="general": any Z (notebooks 5, 6, 61, 7 draw it at random) through the paired inducing points of
    the engine (VGGP_FLAG_PAIRED_Z, dense M-space, M <= 16384); Z is a trainable Parameter as in the reference (:236) unless
    train_z=False, and `_elbo()` carries its analytic gradient.  inducing="auto" picks "grid" for a cartesian Z, "general" when no
    coordinate column repeats a value, and raises otherwise (select_inducing_mode)."""

    def __init__(self, X, y, Z: torch.Tensor, n_b0_splines: int, dim1_grid_lims, dim2_grid_lims, inducing: str = "auto",
                 train_z: bool = True, **kw):
        KroneckerStructure.__init__(self, X, y, **kw)
        Zt = torch.as_tensor(Z, dtype=torch.float64)
        self.inducing = select_inducing_mode(Zt, inducing)
        if self.inducing == "grid":
            self.Z = torch.nn.Parameter(Zt.clone(), requires_grad=False)
            self._z1, self._z2, self._u_of_row = _detect_cartesian(Zt)
        else:
            self.Z = torch.nn.Parameter(Zt.clone(), requires_grad=bool(train_z))
            self._no_iterative("paired inducing points (inducing='general')")
            if self._masked:                                    # a grid with holes is its observed points
                self._as_scattered()
            self._masked = True                                 # read-outs: the dense M-space ones (vggp_*_masked)
        self._grid_init(n_b0_splines, dim1_grid_lims, dim2_grid_lims)

    def _basis(self):
        if self.inducing == "general":
            Z = self.Z.detach().cpu().numpy()
            return "paired", Z[:, 0].copy(), Z[:, 1].copy()
        return "points", self._z1.copy(), self._z2.copy()

    def _plan(self):
        if self.inducing == "grid":
            return KroneckerStructure._plan(self)
        _, g1, g2 = self._basis()
        key = ("paired", g1.tobytes(), g2.tobytes())
        if self._planned and self._plan_token == self._engine.plan_token and self._plan_key is not None:
            if key != self._plan_key:              # only Z moved (an optimiser step): new coordinates in place, no re-plan
                if key[1] != self._plan_key[1]:
                    self._engine.set_inducing(0, g1)
                if key[2] != self._plan_key[2]:
                    self._engine.set_inducing(1, g2)
                self._plan_key = key
            return
        self._engine.plan_paired(self.kind, np.stack([g1, g2], axis=1), self._x1, self._x2, scattered=self._scattered)
        self._planned = True
        self._plan_token, self._plan_key = self._engine.plan_token, key

    def _engine_step(self, theta):
        if self.inducing == "grid":
            return KroneckerStructure._engine_step(self, theta)
        self._plan()
        if self._scattered:
            return self._engine.elbo_step_scattered(self._Y, self._yy, theta)
        return self._engine.elbo_step(self._Y, self._yy, theta)

    def _elbo(self) -> torch.Tensor:
        if self.inducing == "general":
            return _ElboFunction.apply(self._theta(), self, self.Z)
        return KroneckerStructure._elbo(self)

    def _cross(self, d: int, ell: float) -> torch.Tensor:
        mesh = self.b0_mesh_1 if d == 0 else self.b0_mesh_2
        if self.inducing == "general":
            return _b0_cross_points(mesh, self.Z.detach()[:, d].cpu(), ell)
        return _b0_cross_points(mesh, torch.as_tensor(self._z1 if d == 0 else self._z2), ell)

    def q_u(self) -> MultivariateNormal:
        """:396-405, in the row order of the caller's Z."""
        qu = KroneckerStructure.q_v(self)
        if self.inducing == "general":
            return qu
        idx = torch.as_tensor(self._u_of_row)
        sample = (lambda n, seed, first: qu._sample_fn(n, seed, first)[:, idx]) if qu._sample_fn is not None else None
        if callable(qu._variance):       # iterative solvers: the variance stays lazy (block solves, or not provided: scattered)
            return MultivariateNormal(qu.mean[idx], lambda: qu.variance[idx], sample_fn=sample)
        return MultivariateNormal(qu.mean[idx], qu.variance[idx], sample_fn=sample)


def select_inducing_mode(Z, inducing: str = "auto", rtol: float = 1e-6) -> str:
    """How GriddedMatern12SVGP treats Z (M, 2): "grid" (a full cartesian grid, Kronecker engine) or "general" (paired inducing
    points).  "auto": "grid" when Z is cartesian, "general" when neither coordinate column repeats a value (up to rtol of its span,
    as _cluster_coordinates judges it), otherwise ValueError -- a cartesian grid with a dropped row is almost certainly a mistake."""
    if inducing not in ("auto", "grid", "general"):
        raise ValueError(f"inducing must be 'auto', 'grid' or 'general', got {inducing!r}")
    Zt = torch.as_tensor(Z, dtype=torch.float64)
    if Zt.dim() != 2 or Zt.shape[1] != 2:
        raise ValueError("Z must be (M, 2)")
    if inducing == "general":
        return "general"
    try:
        _detect_cartesian(Zt, rtol)
        return "grid"
    except ValueError:
        if inducing == "grid":
            raise
    Zn = Zt.detach().cpu().numpy()
    z1, _ = _cluster_coordinates(Zn[:, 0], rtol)
    z2, _ = _cluster_coordinates(Zn[:, 1], rtol)
    if len(z1) == Zn.shape[0] and len(z2) == Zn.shape[0]:
        return "general"
    _detect_cartesian(Zt, rtol, hint=True)
    raise AssertionError("unreachable")


def _cluster_coordinates(v: np.ndarray, rtol: float):
    """Distinct values of v up to rtol * span(v) (coordinates that went through a float32 round trip or a scaler differ in the
    last bits): (centres, index of each entry's centre); a centre is the mean of its cluster."""
    order = np.argsort(v, kind="stable")
    vs = v[order]
    tol = rtol * max(float(vs[-1] - vs[0]), np.finfo(np.float64).tiny) if len(vs) else 0.0
    new = np.concatenate([[True], np.diff(vs) > tol]) if len(vs) else np.zeros(0, bool)
    gid = np.cumsum(new) - 1
    centres = np.bincount(gid, weights=vs) / np.bincount(gid)
    inv = np.empty(len(v), dtype=np.int64)
    inv[order] = gid
    return centres, inv


def _detect_cartesian(Z: torch.Tensor, rtol: float = 1e-6, hint: bool = False):
    """Z (M, 2) listing every pair of cartesian_prod(z1, z2) exactly once, in any row order -> (z1, z2, u_of_row) with
    u_of_row[r] = i1 * m2 + i2, the engine's inducing index of row r; raises when Z is not such a grid.  Coordinates are
    matched up to rtol of their span, so a grid that passed through float32 or a scaler is still recognised."""
    Zn = Z.detach().cpu().numpy().astype(np.float64)
    if Zn.ndim != 2 or Zn.shape[1] != 2:
        raise ValueError("Z must be (M, 2)")
    z1, i1 = _cluster_coordinates(Zn[:, 0], rtol)
    z2, i2 = _cluster_coordinates(Zn[:, 1], rtol)
    u = i1 * len(z2) + i2
    if len(z1) * len(z2) != Zn.shape[0] or len(np.unique(u)) != Zn.shape[0]:
        raise ValueError("GriddedMatern12SVGP: Z must be a full cartesian grid cartesian_prod(z1, z2): only then is "
                         "k(Z, Z) = kron(K1, K2)" + ("; a Z whose coordinates repeat but that is no full grid is refused by "
                         "inducing='auto' -- pass inducing=\"general\" to use arbitrary inducing points" if hint else
                         " (inducing=\"general\" takes arbitrary inducing points)"))
    return z1, z2, u


class GriddedMatern12ASVGP(_GriddedReadout, Matern12B1SplineASVGP):
    """gridded_kronecker_structure.py:685-969: B1-spline inducing features on the B0 mesh padded by `padding_factor` knots on
    either side (:699-724), gridded read-out with the reference's own Cov(v, u) -- delta at the two knots of each cell
    (:831-845; the reference's value, not the exact RKHS cross-covariance)."""

    def __init__(self, X, y, n_b0_splines: int, padding_factor: int, dim1_grid_lims, dim2_grid_lims, **kw):
        KroneckerStructure.__init__(self, X, y, **kw)
        self._grid_init(n_b0_splines, dim1_grid_lims, dim2_grid_lims)
        self.padding_factor = padding_factor

        def padded(mesh, delta):
            left = torch.tensor([(mesh[0] - i * delta).item() for i in range(padding_factor, 0, -1)])
            right = torch.tensor([(mesh[-1] + i * delta).item() for i in range(1, padding_factor + 1)])
            return torch.cat((left, mesh, right))
        self.b0_mesh_padded_1 = padded(self.b0_mesh_1, self.b0_delta_1)
        self.b0_mesh_padded_2 = padded(self.b0_mesh_2, self.b0_delta_2)
        self.mesh_1, self.mesh_2 = self.b0_mesh_padded_1, self.b0_mesh_padded_2          # the B1 knots of the parent class
        self.nknots = self.mesh_1.shape[0]
        self.delta_1, self.delta_2 = self.mesh_1[1] - self.mesh_1[0], self.mesh_2[1] - self.mesh_2[0]
        self.delta = self.delta_1
        self.b1_basis_1 = self.basis_1 = B1SplineBasis(self.mesh_1, self._engine)
        self.b1_basis_2 = self.basis_2 = B1SplineBasis(self.mesh_2, self._engine)

    def _cross(self, d: int, ell: float) -> torch.Tensor:
        mesh = self.mesh_1 if d == 0 else self.mesh_2
        K, ns, pad = mesh.shape[0], self.nsplines, self.padding_factor
        C = torch.zeros(ns, K, dtype=torch.float64)
        delta = float((mesh[1] - mesh[0]).double())
        idx = torch.arange(ns)
        C[idx, pad + idx] = delta
        C[idx, pad + idx + 1] = delta
        return C
