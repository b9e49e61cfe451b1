"""Exact GPs on scattered 2-D points: the dense baseline the reference's notebooks fit beside every sparse model.

    reference                                                   here
    src/models/exact/bivariate_structure.py:9-173               Matern12GP, Matern32GP, Matern52GP (+ RBFGP, new)
    src/models/sparse/gridded_kronecker_structure.py:21-211     GriddedMatern12ExactGP

kernel = kernel_1 * kernel_2 on active dims 0 and 1, Sigma = K + noise I.  Two solvers (`solver=`):
    "dense"      Sigma is an N x N matrix (N <= 16384) that the engine builds from the coordinates and factors on the GPU
                 (include/vggp.h, vggp_exact_*)
    "iterative"  Sigma is never stored: a matrix-free kernel-matrix product, preconditioned block conjugate gradients and stochastic
                 Lanczos quadrature on fixed probes (vggp_exact_*_iter) -- what gpytorch does above max_cholesky_size, at any N the
                 along-track data has (N ~ 100 000).  The marginal likelihood and its gradient are then estimates (`n_probes`,
                 `precond_rank`, `cg_tol`, `max_cg_iter`); alpha and the read-outs are exact to the CG tolerance.  posterior() gives the
                 mean at once and the variance on first access (ceil(N* / 64) block solves); there is no dense covariance.
    "auto"       dense up to N = 16384 (bit for bit what it always was), iterative above.
`log_marginal_likelihood()` returns a differentiable 0-d tensor whose value and analytic gradient come from one vggp_exact_step
(or vggp_exact_step_iter); `mll()` is the same per point, what gpytorch's ExactMarginalLogLikelihood returns and the notebooks
negate.  Raw parameters, transforms and attribute names are those of the sparse classes (models.py).  The reference's non_informative_initialise / informative_initialise of these classes read
`self.mean.outputscale` and `self.kernel.outputscale`, which do not exist (they raise there), and are not ported.  There is no CPU
fallback.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import VggpError
from .basis import B0SplineBasis
from .engine import Engine
from .models import GaussianLikelihood, KroneckerStructure, MultivariateNormal, ScaleKernel, _b0_kvv_diag_unit, _BaseKernel


class _MllFunction(torch.autograd.Function):
    """value + analytic gradient from one vggp_exact_step; backward only scales the cached gradient."""

    @staticmethod
    def forward(ctx, theta: torch.Tensor, model: "GP"):
        try:
            mll, grad, info = model._engine_step([float(t) for t in theta.detach().cpu()])
        except VggpError as e:
            if e.code == _lib.VGGP_ENOTPD:
                raise torch.linalg.LinAlgError(str(e)) from e
            raise
        model.last_info = info
        ctx.save_for_backward(torch.as_tensor(grad, dtype=theta.dtype, device=theta.device))
        return torch.as_tensor(mll, dtype=theta.dtype, device=theta.device)

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return grad_out * g, None


class GP(torch.nn.Module):
    """bivariate_structure.py:9-134 -- exact GP regression with a product kernel, zero mean."""

    kind = "matern12"

    DENSE_MAX_N = 16384

    def __init__(self, train_x: torch.Tensor, train_y: torch.Tensor, likelihood: Optional[GaussianLikelihood] = None,
                 engine: Optional[Engine] = None, solver: str = "auto", n_probes: int = 16, precond_rank: int = 64, cg_tol: float = 1e-10,
                 max_cg_iter: int = 1000):
        super().__init__()
        X = torch.as_tensor(train_x)
        if X.dim() != 2 or X.shape[1] != 2:
            raise ValueError("train_x must be (N, 2)")
        if solver not in ("auto", "dense", "iterative"):
            raise ValueError("solver must be 'auto', 'dense' or 'iterative'")
        self.solver = solver
        self._iterative = solver == "iterative" or (solver == "auto" and X.shape[0] > self.DENSE_MAX_N)
        self.n_probes, self.precond_rank, self.cg_tol, self.max_cg_iter = int(n_probes), int(precond_rank), float(cg_tol), int(max_cg_iter)
        self.last_readout_info = None
        self.train_x, self.train_y = train_x, train_y
        self.train_inputs = (train_x,)
        self.train_targets = train_y
        self.likelihood = likelihood if likelihood is not None else GaussianLikelihood()
        self.kernel_1 = ScaleKernel(_BaseKernel(self.kind))
        self.kernel_2 = ScaleKernel(_BaseKernel(self.kind))
        self._engine = engine if engine is not None else Engine()
        Xn = X.detach().cpu().numpy().astype(np.float64)
        self._x1, self._x2 = Xn[:, 0].copy(), Xn[:, 1].copy()
        self._y = torch.as_tensor(train_y, dtype=torch.float64).reshape(-1).to(self._engine.device).contiguous()
        if self._y.numel() != Xn.shape[0]:
            raise ValueError("train_y must hold one value per row of train_x")
        self._plan_token = -1
        self.last_info = None

    def _plan(self):
        if self._iterative:
            if self._plan_token != self._engine.exact_iter_token:
                self._engine.exact_iter_plan(self.kind, self.kind, self._x1, self._x2)
                self._plan_token = self._engine.exact_iter_token
            return
        if self._plan_token == self._engine.exact_token:
            return
        self._engine.exact_plan(self.kind, self.kind, self._x1, self._x2)
        self._plan_token = self._engine.exact_token

    _theta = KroneckerStructure._theta

    def _engine_step(self, theta):
        self._plan()
        if self._iterative:
            return self._engine.exact_step_iter(self._y, theta, n_probes=self.n_probes, rank=self.precond_rank, tol=self.cg_tol,
                                                max_iter=self.max_cg_iter)
        return self._engine.exact_step(self._y, theta)

    def _refresh(self):
        """The read-outs use the engine state of the CURRENT hyper-parameters."""
        with torch.no_grad():
            _MllFunction.apply(self._theta(), self)

    def log_marginal_likelihood(self) -> torch.Tensor:
        """log p(y | X, theta), differentiable in the raw parameters."""
        return _MllFunction.apply(self._theta(), self)

    def mll(self) -> torch.Tensor:
        """log p(y) / N: gpytorch's ExactMarginalLogLikelihood(likelihood, model)(model(train_x), train_y)."""
        return self.log_marginal_likelihood() / self._y.numel()

    def fit(self, n_iter: int = 100, lr: float = 0.01):
        """The notebooks' loop: Adam on -mll()."""
        opt = torch.optim.Adam(self.parameters(), lr=lr)
        history = torch.empty(n_iter)
        for i in range(n_iter):
            opt.zero_grad()
            loss = -self.mll()
            history[i] = loss.item()
            loss.backward()
            opt.step()
        return history

    prior = KroneckerStructure.prior                    # bivariate_structure.py:85-96 (dense, N* <= 8192)

    def posterior(self, x_star: torch.Tensor) -> MultivariateNormal:
        """bivariate_structure.py:98-115, without the fast_pred_var approximation: mean and variance at x_star (N*, 2);
        `.covariance_matrix` is materialised on first access (vggp_exact_posterior_cov, N* <= 8192)."""
        self._refresh()
        xs = torch.as_tensor(x_star, dtype=torch.float64)
        if self._iterative:              # the mean now (one product); the variance on first access; no dense covariance
            mean, _, _ = self._engine.exact_posterior_iter(xs, variance=False)

            def var():
                self._refresh()          # another exact model may have planned the engine since
                _, v, self.last_readout_info = self._engine.exact_posterior_iter(xs, tol=self.cg_tol, max_iter=self.max_cg_iter)
                return v.cpu()
            return MultivariateNormal(mean.cpu(), var)
        mean, var = self._engine.exact_posterior(xs)

        def cov():
            self._refresh()          # another exact model may have planned the engine since
            return self._engine.exact_posterior_cov(xs).cpu()
        return MultivariateNormal(mean.cpu(), var.cpu(), cov_fn=cov)

    posterior_predictive = KroneckerStructure.posterior_predictive      # bivariate_structure.py:117-134: + noise


class Matern12GP(GP):
    """bivariate_structure.py:137-147."""
    kind = "matern12"


class Matern32GP(GP):
    """bivariate_structure.py:150-160."""
    kind = "matern32"


class Matern52GP(GP):
    """bivariate_structure.py:163-173."""
    kind = "matern52"


class RBFGP(GP):
    """The same model with an RBF product kernel (no reference counterpart, like RBFSVGP)."""
    kind = "rbf"


class GriddedMatern12ExactGP(Matern12GP):
    """gridded_kronecker_structure.py:21-211: the exact GP with a gridded read-out -- q_v() is the distribution of the B0 cell
    features v on an n_b0_splines x n_b0_splines grid given the data (flat index a * nsplines + b)."""

    def __init__(self, train_x, train_y, n_b0_splines: int, dim1_grid_lims: Tuple[float, float], dim2_grid_lims: Tuple[float, float],
                 likelihood: Optional[GaussianLikelihood] = None, engine: Optional[Engine] = None, **solver_options):
        super().__init__(train_x, train_y, likelihood, engine, **solver_options)
        self.n_b0_splines = self.nsplines = n_b0_splines
        self.dim1_grid_lims, self.dim2_grid_lims = dim1_grid_lims, dim2_grid_lims
        self.b0_mesh_1 = torch.linspace(dim1_grid_lims[0], dim1_grid_lims[1], n_b0_splines + 1)
        self.b0_mesh_2 = torch.linspace(dim2_grid_lims[0], dim2_grid_lims[1], n_b0_splines + 1)
        self.b0_delta_1 = self.b0_mesh_1[1] - self.b0_mesh_1[0]
        self.b0_delta_2 = self.b0_mesh_2[1] - self.b0_mesh_2[0]
        self.b0_basis_1 = B0SplineBasis(self.b0_mesh_1, self._engine)
        self.b0_basis_2 = B0SplineBasis(self.b0_mesh_2, self._engine)

    def _readout_operands(self):
        """C_d (nsplines x N, :52-101 at unit outputscale, built on the device) and the unit diagonals of Kvv_d (:111-149)."""
        dev = self._engine.device
        out = []
        for x, mesh, k in ((self._x1, self.b0_mesh_1, self.kernel_1), (self._x2, self.b0_mesh_2, self.kernel_2)):
            ell = k.base_kernel.lengthscale.reshape(()).item()
            xs = torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous()
            out.append(self._engine.factor_build("matern12", "b0", xs, mesh.double().to(dev).contiguous(), ell)[0])
        l1 = self.kernel_1.base_kernel.lengthscale.reshape(()).item()
        l2 = self.kernel_2.base_kernel.lengthscale.reshape(()).item()
        kd1 = torch.full((self.nsplines,), _b0_kvv_diag_unit(float(self.b0_delta_1.double()), l1), dtype=torch.float64)
        kd2 = torch.full((self.nsplines,), _b0_kvv_diag_unit(float(self.b0_delta_2.double()), l2), dtype=torch.float64)
        return out[0], out[1], kd1, kd2

    def q_v(self, psd: bool = True, literal: bool = True) -> MultivariateNormal:
        """:177-191, mean and the diagonal of the covariance.  literal=True: the reference's own expression, in the form
        Kvv + Kvx Kxv / noise it reduces to (vggp.h); literal=False: the conditional variance of v given the data."""
        self._refresh()
        if self._iterative:
            if not literal:
                raise NotImplementedError("the iterative solver has no conditional variance of all cells at once: q_v_cells(cells)")
            mean, var, self.last_readout_info = self._engine.exact_readout_iter(*self._readout_operands(), literal=True)
            return MultivariateNormal(mean.reshape(-1).cpu(), var.reshape(-1).cpu())
        mean, var = self._engine.exact_readout(*self._readout_operands(), literal=literal)
        return MultivariateNormal(mean.reshape(-1).cpu(), var.reshape(-1).cpu())

    def q_v_cells(self, cells, literal: bool = False) -> MultivariateNormal:
        """q_v() at a list of output cells (flat indices a * nsplines + b); on the iterative solver the conditional variance costs
        ceil(len(cells) / 64) block solves."""
        idx = torch.as_tensor(cells, dtype=torch.int64).reshape(-1)
        if self._iterative and not literal:
            self._refresh()
            mean, var, self.last_readout_info = self._engine.exact_readout_iter(*self._readout_operands(), literal=False, cells=idx,
                                                                                 tol=self.cg_tol, max_iter=self.max_cg_iter)
            return MultivariateNormal(mean.reshape(-1).cpu()[idx], var.cpu())
        qv = self.q_v(literal=literal)
        return MultivariateNormal(qv.mean[idx], qv.variance[idx])
