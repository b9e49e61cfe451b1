/*
 * vggp.h -- C-ABI of libvggp_hip.so: the MI355X (gfx950) engine for the
 * Kronecker-structured collapsed-ELBO hot path of
 * maxnorman569/Variational-Gridded-Gaussian-Processes.
 *
 * The reference has NO FFI / plugin boundary (it is plain Python classes on
 * gpytorch); this boundary is defined by the build.  Each entry
 * point cites the reference code it replaces (paths relative to the reference
 * checkout).  Host code (Python/ctypes) owns every data
 * buffer; pointers marked DEVICE are hipMalloc'ed (e.g. torch tensor.data_ptr()),
 * contiguous float64.  The library owns only the opaque context (workspace arena,
 * HIP-graph cache).  Every function returns 0 on success or a negative VGGP_E*
 * code; the message is available from vggp_last_error() (thread-local).  Nothing
 * throws across the boundary.  One context per (process, device); not re-entrant.
 * All work is enqueued on the hipStream_t passed as `stream` (void*, 0 = default).
 *
 * Conventions
 *   theta[5] = { ell_1, ell_2, s_1, s_2, sigma2 }  (constrained values:
 *              lengthscales, outputscales, likelihood.noise -- a variance,
 *              kronecker_structure.py:263)
 *   Y        : observations on the local grid shard, [n2][n1] row-major,
 *              Y[j][i] = y(x1[i], x2[j])  (x1 fastest: utils/datagenerators.py:70-72)
 *   inducing index u = i1*m2 + i2 (kronecker_structure.py:805, :822)
 *   multi-GPU: one process (one context) per GPU; the grid is sharded along the slow storage axis (rows j of Y,
 *              i.e. dimension 2); dimension 1 and all m-space algebra are replicated.  The context OWNS the collective
 *              (an RCCL communicator created in vggp_create, or a host callback): vggp_elbo_step on an n_ranks > 1
 *              context is  partials -> ONE sum all-reduce of the packed payload -> finish  on one stream with one host
 *              synchronisation, and every rank returns the identical value and gradient.
 */
#ifndef VGGP_H
#define VGGP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGGP_VERSION 200          /* 0.2.0 */

/* error codes */
#define VGGP_OK        0
#define VGGP_EINVAL   -1          /* bad argument / shape                          */
#define VGGP_ENOTPD   -2          /* a factor is not PD after the jitter schedule  */
#define VGGP_EHIP     -3          /* HIP runtime error                             */
#define VGGP_ENOMEM   -4
#define VGGP_ESTATE   -5          /* call order (e.g. finish before partials)      */
#define VGGP_ENOCONV  -6          /* Jacobi eigensolver hit its sweep limit        */
#define VGGP_ERCCL    -7          /* the collective failed (RCCL error, RCCL not loadable, callback error) */

/* kernel family of one dimension (gpytorch MaternKernel(nu) / the build's RBF) */
#define VGGP_KIND_MATERN12 0
#define VGGP_KIND_MATERN32 1
#define VGGP_KIND_MATERN52 2
#define VGGP_KIND_RBF      3

/* inducing-feature basis of one dimension */
#define VGGP_BASIS_POINTS 0       /* pairwise k(z, x): Matern12SVGP, kronecker_structure.py:306-338 */
#define VGGP_BASIS_B0     1       /* B0-spline cell integrals (Matern-1/2 only; the other kernels' cells are VGGP_BASIS_B0K):
                                     kronecker_structure.py:702-790 == gridded_kronecker_structure.py:1286-1374 */
#define VGGP_BASIS_ONE    2       /* trivial factor K=[1], A=1: turns the engine into the 1-D model,
                                     univariate_structure.py:234-263, :693-717 */
#define VGGP_BASIS_VFF    3       /* variational Fourier features (Matern-1/2 only): Matern12VFFGP,
                                     kronecker_structure.py:346-515.  grid = [a, b, omega_0 .. omega_M], m = 2M + 1.
                                     Kuu_d = K0(ell) / s_d, Kuf_d = features(x) (no s_d). */
#define VGGP_BASIS_B1     4       /* B1-spline (hat function) features (Matern-1/2 only): Matern12B1SplineASVGP,
                                     kronecker_structure.py:524-660.  grid = knot mesh (m knots).
                                     Kuu_d = (A ell + B / ell + BC) / (2 s_d), Kuf_d = hats(x). */
#define VGGP_BASIS_B0K    5       /* B0 cells under the dimension's own kernel: the features of VGGP_BASIS_B0 (grid = mesh of m + 1
                                     equispaced knots, cell k = (g_k, g_k+1], x <= g_0 counts as below; Kuu_d = s_d K0, Kuf_d = s_d A0)
                                     with K0 = double cell integral and A0 = cell integral of the Matern-1/2, -3/2 or -5/2 profile.
                                     Matern-1/2 runs the code of VGGP_BASIS_B0 (bit-equal outputs); RBF is refused, and so is
                                     VGGP_FLAG_B0_F32_KDELTA (the reference has no such model whose rounding could be reproduced). */

/* The reference keeps the B0 mesh and delta as float32 attributes (torch.linspace default
 * dtype; Module.to(float64) does not touch them), so `(k - 1) * delta` in _Kuu_along_dim
 * (kronecker_structure.py:731-733) is rounded to float32 before the float64 division by the
 * lengthscale.  With this flag the B0 Kuu builder reproduces that rounding (and the literal
 * three-exponential form) so results match the reference bit-for-bit in the inputs. */
#define VGGP_FLAG_B0_F32_KDELTA 1
/* Use the block-Jacobi eigensolver (16-wide index blocks, MFMA super-block updates) instead of the scalar cyclic
 * Jacobi for m <= 128.  Same results to rounding; measured slower on RBF factors and ~10 % faster on Matern factors
 * at m = 128, hence off by default. */
#define VGGP_FLAG_BLOCK_JACOBI 2
#define VGGP_FLAG_SCATTERED 4      /* x1[k], x2[k] are the coordinates of N = n1 = n2 scattered POINTS (not grid axes): only        */
                                   /* vggp_elbo_step_scattered and the *_masked read-outs apply                                      */
/* Paired (general) inducing points -- GriddedMatern12SVGP / Matern12SVGP with a Z that is no cartesian grid
 * (gridded_kronecker_structure.py:235-264, :396-438; bound kronecker_structure.py:249-278).  grid1[i], grid2[i] are the two
 * coordinates of inducing point i; m1 = m2 = M, 1 <= M <= 16384; both bases VGGP_BASIS_POINTS (the per-dimension m <= 256 cap does
 * not apply); combines with VGGP_FLAG_SCATTERED.  kernel = kernel_1 * kernel_2 on active dims 0 / 1, so
 *     Kuu = s (K1 o K2) (Hadamard),  Kuf[i, k] = s k1(z_i1, x_k1) k2(z_i2, x_k2),  s = s1 s2,
 * factored densely in M-space; the jitter follows psd_safe_cholesky on Kuu itself (0, 1e-8, 1e-7, 1e-6 added to its diagonal;
 * reported in vggp_info.jitter1).  The plan allocates O(M^2 + M n_d) (full grid) / O(M^2 + N) (scattered) doubles once.
 * On a paired context:
 *   vggp_elbo_step (full grid Y [n2][n1]) / vggp_elbo_step_scattered (y [N])   value + theta-gradient; one host synchronisation
 *                                                            (a Kuu that needs jitter is refactored at the next level)
 *   vggp_zgrad / vggp_zgrad_scattered     gz1 = dE/dZ[:, 0], gz2 = dE/dZ[:, 1], each [M] (same Y / y as the step)
 *   vggp_set_inducing(dim, z, M)          moves one coordinate column of Z without re-planning
 *   vggp_qv_masked                        q(u) mean and variance, [M] each
 *   vggp_qv_cov_masked                    q(u) covariance Kuu Sigma^-1 Kuu, [M][M]
 *   vggp_readout_masked                   C_d is [mv_d][M]; Kvu[(a, b), i] = s C1[a][i] C2[b][i] (face-split, flat a mv2 + b)
 *   vggp_posterior_masked, vggp_posterior_cov_masked   posterior(x*) from k(x*, Z)
 * Every other step or read-out (vggp_qv, vggp_qv_cov, vggp_readout, vggp_posterior, vggp_posterior_cov, the masked steps, the
 * partials / finish pair) returns VGGP_EINVAL, and so does a paired step on an n_ranks > 1 context.
 * State and arguments (a refused call changes nothing: the next valid call gives the bits it would give on a fresh context):
 *   vggp_plan              VGGP_EINVAL for a non-finite inducing coordinate or observation coordinate x1[i] / x2[i], a bad kind or
 *                          basis, M outside [1, 16384], and the size limits (scattered N < 2^30; grid n_d < 2^24, M n_d < 2^34): all
 *                          checked before anything is allocated or released, so the previous plan (paired or not) and the state of its
 *                          last step stay usable.  VGGP_ENOMEM ends the previous plan.
 *   steps                  vggp_elbo_step on a plan with VGGP_FLAG_SCATTERED and vggp_elbo_step_scattered on one without it return
 *                          VGGP_EINVAL.  All five theta components must be positive and finite (VGGP_EINVAL otherwise); they are
 *                          checked before any is stored, so the read-outs of the earlier step go on working and keep its bits.  A step
 *                          that ends in VGGP_ENOTPD or a HIP error leaves no state: read-outs return VGGP_ESTATE until the next step.
 *   read-outs, vggp_zgrad* VGGP_ESTATE until a step has succeeded on the current plan AND the current inducing points: vggp_plan and
 *                          a successful vggp_set_inducing end the state.  The read-outs test the state before their other arguments; vggp_zgrad*
 *                          tests null outputs and the grid / scattered entry first, so the wrong entry returns VGGP_EINVAL with or
 *                          without a step.
 *   vggp_zgrad*            VGGP_EINVAL for the entry that does not match the plan (grid / scattered) and for a Y / y that is not the
 *                          pointer the last step was given (the gradient belongs to that array).
 *   vggp_set_inducing      VGGP_EINVAL for dim outside {0, 1}, m != M, a null or non-finite z: Z and the state of the last step stay.
 *   vggp_posterior_masked  n_star = 0 succeeds and writes nothing; n_star < 0 or >= 2^30, null pointers: VGGP_EINVAL.
 *   vggp_posterior_cov_masked   1 <= n_star <= 8192 (with M <= 16384 this implies M n_star <= 2^27), VGGP_EINVAL otherwise, before any
 *                          memory is touched (there is no n_star <= M condition on a paired context).
 *   vggp_readout_masked    mv_d >= 1, mv1 mv2 < 2^30, no null pointer: VGGP_EINVAL otherwise. */
#define VGGP_FLAG_PAIRED_Z 8

typedef struct vggp_ctx vggp_ctx;

/* Problem description (host struct; the small coordinate arrays are HOST pointers and
 * are copied into the context by vggp_plan). */
typedef struct vggp_desc {
    int32_t kind1, basis1;        /* dimension 1 (x1, fast axis of Y)                 */
    int32_t kind2, basis2;        /* dimension 2 (x2, slow axis of Y; sharded axis)   */
    int64_t n1, n2;               /* LOCAL grid: Y is [n2][n1]                        */
    int64_t m1, m2;               /* inducing features per dimension                  */
    int64_t n_total;              /* number of observations over ALL ranks (N)        */
    const double* x1;             /* HOST [n1]  unique coordinates along dim 1        */
    const double* x2;             /* HOST [n2]  local coordinates along dim 2         */
    const double* grid1;          /* HOST: mesh [m1+1] (B0, B0K) or inducing coords [m1] */
    const double* grid2;          /* HOST: mesh [m2+1] (B0, B0K) or inducing coords [m2] */
    int32_t warm_start;           /* 1: reuse the previous step's eigenvectors        */
    int32_t flags;                /* VGGP_FLAG_* bit mask                             */
} vggp_desc;

/* per-step diagnostics (host struct filled by vggp_elbo_finish / vggp_elbo_step) */
typedef struct vggp_info {
    double jitter1, jitter2;      /* jitter actually added to the unit-scale factors  */
    int32_t sweeps1, sweeps2;     /* Jacobi sweeps used                               */
    int32_t rounds1, rounds2;     /* Jacobi rotation rounds applied                   */
    int32_t status;               /* 0 or a VGGP_E* code detected on the device       */
    int32_t polished;             /* bit d-1: dimension d's eigensolver ended in a first-order polish */
} vggp_info;

int         vggp_version(void);
const char* vggp_last_error(void);

/* lifecycle ---------------------------------------------------------------- */
/* One context per (process, GPU).  n_ranks = 1: single GPU (rank, unique_id ignored).  n_ranks > 1: this process is rank
 * `rank` of a row-sharded job; `unique_id` (VGGP_UNIQUE_ID_BYTES bytes, generated on rank 0 by vggp_unique_id and
 * distributed to the other ranks by the host program) creates the context's RCCL communicator (collective call: every
 * rank must be inside vggp_create).  unique_id = NULL with n_ranks > 1 creates no communicator: the caller installs a host
 * transport with vggp_set_allreduce before the first step.  (A unique id with n_ranks = 1 creates a communicator of size
 * one and the step runs the multi-rank sequence through it: the RCCL path on a one-GPU box.) */
#define VGGP_UNIQUE_ID_BYTES 128
int vggp_create(vggp_ctx** out, int device, int n_ranks, int rank, const void* unique_id);
int vggp_destroy(vggp_ctx* ctx);
int vggp_unique_id(void* out /* VGGP_UNIQUE_ID_BYTES */);
/* Host-callback transport: fn sums `count` doubles at the HOST address `buf` over all ranks, in place, and returns 0.
 * The library stages the payload through pinned memory around the call.  Used by the multi-rank rehearsal on one GPU
 * (gloo; RCCL refuses several ranks on one device) and as the seam for other transports. */
typedef int (*vggp_allreduce_fn)(void* user, double* buf, int64_t count);
int vggp_set_allreduce(vggp_ctx* ctx, vggp_allreduce_fn fn, void* user);
/* The context's sum all-reduce on a DEVICE buffer (in place; returns after the result is complete). */
int vggp_allreduce(vggp_ctx* ctx, double* buf, int64_t count, void* stream);
/* n_ranks, rank and the transport in use (0 none, 1 RCCL, 2 host callback); any output may be NULL. */
int vggp_comm_info(const vggp_ctx* ctx, int* n_ranks, int* rank, int* transport);
/* (Re)plan the context for a problem: allocates the workspace arena (no allocation
 * happens per step afterwards) and uploads coordinates / meshes.
 * Replaces: KroneckerStructure.__init__ + Matern12GriddedGP.__init__ bookkeeping
 * (kronecker_structure.py:19-32, gridded_kronecker_structure.py:1259-1284). */
int vggp_plan(vggp_ctx* ctx, const vggp_desc* desc);
/* Number of doubles in the all-reduce payload {G2,H2,C,C1,C2} of the planned problem. */
int64_t vggp_payload_len(const vggp_ctx* ctx);
int64_t vggp_workspace_bytes(const vggp_ctx* ctx);

/* the hot path ------------------------------------------------------------- */
/* One ELBO step = value + gradient w.r.t. theta.  Replaces KroneckerStructure._elbo
 * (kronecker_structure.py:249-278) AND the autograd backward of the notebook loop
 * (5_gridded_kronecker_structure_models.ipynb cell 26).
 *   Y        DEVICE [n2][n1]  (this rank's row slab)
 *   yy_total sum of y^2 over ALL ranks (constant of the data; vggp_sumsq returns it)
 *   elbo_out, grad_out[5]  HOST outputs (the only host sync of the step)
 * Single-rank convenience = vggp_elbo_partials + vggp_elbo_finish. */
int vggp_elbo_step(vggp_ctx* ctx, const double* Y, double yy_total, const double theta[5],
                   double* elbo_out, double grad_out[5], vggp_info* info, void* stream);

/* The two halves of the step, for callers that carry the all-reduce themselves (vggp_elbo_step on a multi-rank context
 * does all three): partials fills `payload` (DEVICE, vggp_payload_len doubles) with this rank's contribution; the caller
 * sums it over ranks with ONE all-reduce and passes the reduced buffer to finish.  The buffer is the caller's again when finish
 * returns: after a warm-started step finish keeps its own copy of the reduced payload (one device-to-device copy of
 * vggp_payload_len doubles on the step's stream, about 10 us), so the read-outs that follow (vggp_qv, vggp_qv_cov, vggp_posterior,
 * vggp_posterior_cov, vggp_readout) have the accuracy they have after vggp_elbo_step. */
int vggp_elbo_partials(vggp_ctx* ctx, const double* Y, const double theta[5],
                       double* payload, void* stream);
int vggp_elbo_finish(vggp_ctx* ctx, const double* payload, double yy_total, const double theta[5],
                     double* elbo_out, double grad_out[5], vggp_info* info, void* stream);

/* Masked / partially observed grid (BASELINE config 5).  Ym = W o Y and W (0/1 as float64) are DEVICE [n2][n1] (this rank's
 * row slab); n_obs = sum(W), yy_obs = sum(Ym^2) over ALL ranks.  Phi = Kuf W Kuf^T is assembled in M-space (M = m1 m2 <= 16384)
 * and factored densely; value + analytic gradient as for vggp_elbo_step.  Replaces KroneckerStructure._elbo
 * (kronecker_structure.py:249-278) called with the observed subset of the grid as X, y.
 * Multi-rank context: every rank assembles the partial Phi_r (and its two lengthscale derivatives, the projections and a
 * column statistic) of its rows, ONE all-reduce (3 M^2 + 3 M + n1 doubles) makes Sigma~ and its factorisation replicated,
 * and a second all-reduce of 21 scalars closes the gradient terms that are sums over grid rows. */
int vggp_elbo_step_masked(vggp_ctx* ctx, const double* Ym, const double* W, double n_obs, double yy_obs,
                          const double theta[5], double* elbo_out, double grad_out[5], vggp_info* info, void* stream);
/* The masked step WITHOUT the M x M matrices -- for M = m1 m2 beyond the dense solver (M > 16384) or when O(M^3) is too slow:
 * what gpytorch does for the reference above max_cholesky_size = 800 (`inv_matmul` by CG, `log_prob` by stochastic Lanczos
 * quadrature, kronecker_structure.py:269, :273), here with matricised Kronecker MVMs  Sigma~ V = V + rho B1 (W^T o (B1^T V B2)) B2^T,
 * the Kronecker-eigenbasis preconditioner P = I + rho p G1 (x) G2 (p = observed fraction), log|Sigma~| = log|P| + Lanczos
 * quadrature of the PCG coefficients of n_probes FIXED Rademacher probes, and derivative traces as closed form + control-variate
 * probe estimator.  Bitwise reproducible.  Stated tolerance against vggp_elbo_step_masked: ELBO 1e-5 relative, gradient 1e-4 of
 * its largest component (n_probes = 16).  n_probes <= 0: 16; tol <= 0: 1e-10 (PCG residual, relative); max_iter <= 0: 100.
 * Arguments otherwise as vggp_elbo_step_masked; info->rounds1 = PCG iterations, info->sweeps1 = probes.
 * Multi-rank context (the split of vggp_elbo_step_masked): LOCAL are the row slab Ym[rows], W[rows] and the plan's x2[rows];
 * GLOBAL are n_obs, yy_obs and desc.n_total = n1 n2 over all ranks (the preconditioner's observed fraction is n_obs / n_total);
 * REPLICATED are the block vectors, probes, preconditioner, its kept basis and every PCG scalar.  Collectives, on the step's
 * stream and in the same order on every rank: one packed all-reduce before the solve (G2, H2 | C, C1, C2 | a column statistic:
 * 2 m2^2 + 3 M + n1 doubles), one all-reduce of the partial operator product per PCG iteration (M (n_probes + 1) doubles), one
 * packed all-reduce of 32 scalars after the solve (the sums over grid rows: reduction jobs, control-variate field sums, exact-trace
 * products).  Every host decision (iteration count, kept or cold basis, VGGP_ENOCONV, status) is taken from replicated data, so
 * all ranks return the same code from the same call with bitwise equal results; host waits poll the communicator.
 * That holds only over a transport that really sums over the n_ranks ranks of vggp_create: the first iterative entry (step or
 * read-out) called on a multi-rank context all-reduces the single value 1.0, once per context and transport, and every iterative
 * entry returns VGGP_EINVAL when it does not come back as n_ranks (a callback that sums nothing, a communicator of another size).
 * Its read-outs are vggp_qv_masked_iter and vggp_posterior_masked_iter below (the dense ones, vggp_qv_masked, ..., return
 * VGGP_ESTATE after this step: there is no Sigma~^-1 to read). */
int vggp_elbo_step_masked_iter(vggp_ctx* ctx, const double* Ym, const double* W, double n_obs, double yy_obs,
                               const double theta[5], int n_probes, double tol, int max_iter, double* elbo_out, double grad_out[5],
                               vggp_info* info, void* stream);
/* Read-outs of the iterative step, again without any M x M matrix.  Every read-out quantity belongs to a rank-one whitened
 * column t = u1 (x) u2:  mean = (s1 s2 / sigma^2) t^T a0,  var = s1 s2 (kappa - |t|^2 + t^T Sigma~^-1 t), with a0 = Sigma~^-1 c0
 * from the step and t^T Sigma~^-1 t from a block PCG solve Sigma~ X = T over `block` columns at a time: the step's operator, its
 * preconditioner (in the eigenbasis the step left behind) and its per-column stopping rule |r| <= tol |r0|.  No probes: the
 * results are deterministic.  Cost: ceil(columns / block) block solves, each about the step's PCG at the same width.
 *   W, n_obs   the mask and observation count the step was given (DEVICE [n2][n1])
 *   tol <= 0: 1e-10;  max_iter <= 0: 100;  block <= 0: the largest of 64, 32, 16, ... the step's index limits allow; block <= 64
 *   info       (may be NULL) rounds1 = largest PCG iteration count over the block solves, sweeps1 = number of block solves
 * Both return VGGP_ESTATE unless the LAST finished step on the context was a successful vggp_elbo_step_masked_iter (vggp_plan,
 * vggp_set_inducing, any other step and a failed iterative step end that state); VGGP_ENOCONV when a column does not converge;
 * VGGP_EINVAL on paired or scattered contexts, a cell index outside [0, M), block > 64.  Multi-rank context: W is the rank's
 * row slab, n_obs global; right-hand sides and results are replicated, and the only collective is the operator's all-reduce of each
 * PCG iteration (every rank must make the same call).  The workspace (block
 * vectors and one n1 x block x n2 field) is allocated on first use and apart from the step's: a read-out leaves the step's kept
 * preconditioner basis valid and the next step's results unchanged.
 *
 * q(v): u_d = row i_d of L0_d, kappa = |t|^2, so var = s1^e1 s2^e2 t^T Sigma~^-1 t (e_d = -1 for VFF / B1 features, else 1); the
 * mean needs no solve (L0_1 A0 L0_2^T, scaled as vggp_qv_masked scales it).
 *   mean   DEVICE [m1][m2], all cells (NULL to skip)
 *   cells  HOST int64 [n_cells] flat indices i1*m2 + i2, or NULL with n_cells = M for every cell
 *   var    DEVICE [n_cells] (NULL with n_cells = 0: mean only) */
int vggp_qv_masked_iter(vggp_ctx* ctx, const double* W, double n_obs, const int64_t* cells, int64_t n_cells, double tol,
                        int max_iter, int block, double* mean, double* var, vggp_info* info, void* stream);
/* posterior(x*) (kronecker_structure.py:199-230 on the observed subset): u_d = L0_d^-1 a_d(x*_d), kappa = 1.
 *   xs1, xs2 DEVICE [n_star];  mean, var DEVICE [n_star] */
int vggp_posterior_masked_iter(vggp_ctx* ctx, const double* W, double n_obs, const double* xs1, const double* xs2,
                               int64_t n_star, double tol, int max_iter, int block, double* mean, double* var, vggp_info* info,
                               void* stream);
/* The scattered step WITHOUT the M x M matrices and without any m_d^2 x N or m_d x columns x N buffer -- along-track data beyond
 * the dense solver of vggp_elbo_step_scattered (M = m1 m2 > 16384, or m_d^2 N >= 2^31) or where its O(M^2 N + M^3) is too slow.
 * The iterative masked step with the sum over observed grid nodes replaced by a sum over the points (a Khatri-Rao operator),
 *     Sigma~ V = V + rho sum_k b1_k (b1_k^T V b2_k) b2_k^T,     B_d = L0_d^-1 A0_d(x_d)  (m_d x N, one column per point),
 * applied by two fused fp64-MFMA kernels (vggp_kr_field, vggp_kr_back below); preconditioner P = I + (rho / N) G1 (x) G2 with
 * G_d = B_d B_d^T, diagonal in the Kronecker eigenbasis (the independence approximation E[Phi] = G1 (x) G2 / N: exact when the
 * points form a full grid); PCG, Lanczos quadrature on FIXED probes and control-variate traces as vggp_elbo_step_masked_iter.
 * Bitwise reproducible (no floating-point atomics).  Workspace O(M cols + (m1 + m2) N + cols N), cols = n_probes + 1.
 *   y DEVICE [N], yy = sum y^2, theta as vggp_elbo_step_scattered; n_probes <= 0: 16 (at most 63); tol <= 0: 1e-10; max_iter <= 0: 100
 *   info->rounds1 = PCG iterations, info->sweeps1 = probes.  Any m_d <= 256.
 * Accuracy: a0 = Sigma~^-1 c0, and with it both mean read-outs below, is exact to the PCG tolerance wherever the PCG converges.
 * The stochastic ELBO and gradient match the iterative masked step's quality (ELBO 1e-5 relative, gradient 1e-4 of its largest
 * component against vggp_elbo_step_scattered, 16 probes) when the points outnumber the inducing features by about 60 or more;
 * they degrade to 1e-3 .. 1e-2 when N is about M, where few tracks also cost PCG iterations.  No tolerance is stated there.
 * Needs a context planned with VGGP_FLAG_SCATTERED (VGGP_EINVAL otherwise, and on paired contexts); VGGP_ENOCONV when
 * the PCG does not converge.  Multi-rank context (the split of vggp_elbo_step_scattered): LOCAL are the rank's own points x, y (any
 * share); GLOBAL are yy and desc.n_total = N over all ranks (p = 1 / n_total); REPLICATED is everything in M-space.  Collectives as
 * vggp_elbo_step_masked_iter: before the solve G2 | C, C1, C2 | G1 in one call, per PCG iteration the partial operator product,
 * after the solve 32 scalars (the sums over points, PT1 and PT2 through their scalars <Mk_d, PT_d>); the same host decisions on
 * every rank.  The kept-basis rules are the masked iterative step's (VGGP_ITER_COLD_BASIS honoured).  The dense
 * read-outs (vggp_qv_masked, ...) and vggp_zgrad_scattered return VGGP_ESTATE after this step. */
int vggp_elbo_step_scattered_iter(vggp_ctx* ctx, const double* y, double yy, const double theta[5], int n_probes, double tol,
                                  int max_iter, double* elbo_out, double grad_out[5], vggp_info* info, void* stream);
/* Mean read-outs of the iterative scattered step; both need only a0: mean = (s1 s2 / sigma^2) t^T a0.  VGGP_ESTATE unless the LAST
 * finished step on the context was a successful vggp_elbo_step_scattered_iter.  The POINT-WISE VARIANCES of these two come from the
 * vggp_*_var_scattered_iter entries below.  Multi-rank context: a0 is replicated, no collective.
 *   vggp_qv_scattered_iter         mean DEVICE [m1][m2] = L0_1 A0 L0_2^T scaled as vggp_qv_masked_iter scales it (e_d = -1 for VFF / B1)
 *   vggp_posterior_scattered_iter  xs1, xs2 DEVICE [n_star]; mean DEVICE [n_star] */
int vggp_qv_scattered_iter(vggp_ctx* ctx, double* mean, void* stream);
int vggp_posterior_scattered_iter(vggp_ctx* ctx, const double* xs1, const double* xs2, int64_t n_star, double* mean, void* stream);
/* The same two read-outs WITH their point-wise variances: vggp_qv_masked_iter / vggp_posterior_masked_iter without W, n_obs, on the
 * Khatri-Rao operator with p = 1 / N.  Every column is rank one, t = u1 (x) u2, and t^T Sigma~^-1 t comes from block PCG solves over
 * `block` <= 64 columns at a time (the solve vggp_readout_scattered_iter runs: the step's operator, kept preconditioner basis and
 * per-column stopping rule; no probes, deterministic; a column's numbers do not depend on its neighbours or on `block`).
 *   q(v)       t = L0_1[i1,:] (x) L0_2[i2,:];  var = s1^e1 s2^e2 t^T Sigma~^-1 t, e_d = -1 for VFF / B1 and 1 otherwise
 *              cells  HOST int64 [n_cells] flat indices i1*m2 + i2, or NULL with n_cells = M for every cell (ceil(M / block) solves)
 *              mean   DEVICE [m1][m2], every cell, as vggp_qv_scattered_iter (NULL to skip);  var DEVICE [n_cells] (NULL with
 *              n_cells = 0: the mean only, no solve)
 *   posterior  u_d = L0_d^-1 a_d(x*_d);  mean = (s1 s2 / sigma^2) t^T a0,  var = s1 s2 (1 - |t|^2 + t^T Sigma~^-1 t)
 *              xs1, xs2, mean, var DEVICE [n_star]
 *   tol <= 0: 1e-10; max_iter <= 0: 100; block <= 0: the largest of 64, 32, ... with N block < 2^31 and M block < 2^31
 *   info->rounds1 = largest PCG count, info->sweeps1 = number of block solves
 * VGGP_ESTATE unless the LAST finished step on the context was a successful vggp_elbo_step_scattered_iter; VGGP_ENOCONV when a column
 * does not converge; VGGP_EINVAL on a grid plan, on paired contexts, for a cell outside [0, M), block > 64, null arguments.
 * Multi-rank context: right-hand sides and results are replicated; the operator's all-reduce of each PCG iteration is the only
 * collective (every rank must make the same call).  The workspace is the iterative read-outs' own: a read-out between two steps leaves the second step's bits unchanged. */
int vggp_qv_var_scattered_iter(vggp_ctx* ctx, const int64_t* cells, int64_t n_cells, double tol, int max_iter, int block, double* mean,
                               double* var, vggp_info* info, void* stream);
int vggp_posterior_var_scattered_iter(vggp_ctx* ctx, const double* xs1, const double* xs2, int64_t n_star, double tol, int max_iter,
                                      int block, double* mean, double* var, vggp_info* info, void* stream);
/* Building blocks of that step, exported for tests: the two kernels on caller-supplied DEVICE arrays.  L [m1][N], R [m2][N] (one
 * column per point), block vectors [m1][nb][m2], fields [nb][N]; 1 <= m_d <= 256, 1 <= nb <= 64.  The context need not be planned.
 *   field  F[c][k]      = sum_a L[a][k] sum_b V[a][c][b] R[b][k]
 *   back   out[a][c][b] = sum_k L[a][k] F[c][k] R[b][k]      (reduction split over workgroups, slabs summed in fixed order) */
int vggp_kr_field(vggp_ctx* ctx, const double* L, const double* R, const double* V, int64_t m1, int64_t m2, int64_t N, int64_t nb,
                  double* F, void* stream);
int vggp_kr_back(vggp_ctx* ctx, const double* L, const double* R, const double* F, int64_t m1, int64_t m2, int64_t N, int64_t nb,
                 double* out, void* stream);
/* The field kernel with two columns per workgroup instead of four (half the registers, several waves per SIMD): arguments and limits
 * of vggp_kr_field, and the same bits -- a column's accumulators, k order and reductions do not depend on the column group. */
int vggp_kr_field2(vggp_ctx* ctx, const double* L, const double* R, const double* V, int64_t m1, int64_t m2, int64_t N, int64_t nb,
                   double* F, void* stream);
/* Gridded read-out q(v) of B0 cell features after an ITERATIVE step: vggp_readout_masked's algebra and scaling (C_d DEVICE [mv_d][m_d],
 * kd_d DEVICE [mv_d], flags = VGGP_READOUT_LITERAL as there) with Sigma~^-1 applied instead of stored, so M = m1 m2 is not limited.
 * U_d = L0_d^-1 C_d^T; cell (a, b) owns t = U1[:, a] (x) U2[:, b]; rho = s1 s2 / sigma^2; P_d = U_d^T B_d (mv_d x n_d).
 *   mean      rho U1^T A0 U2, all cells, two GEMMs, no solve
 *   literal   var[a][b] = s1 s2 (kd1[a] kd2[b] + rho S[a][b]): the reference's expression (X = S_u^-1), where |t|^2 cancels and
 *             t^T Sigma~ t is a Gram product over the data -- S = (P1 o P1)(P2 o P2)^T over the points (vggp_kr_sqgram on chunks of
 *             points, workspace O((mv1 + mv2) chunk + mv1 mv2) whatever N) or (P1 o P1) W^T (P2 o P2)^T on a grid with holes.  No solve:
 *             all cells for about one application of the operator; info->sweeps1 = 0
 *   otherwise var = s1 s2 (kd1[a] kd2[b] - |t|^2 + t^T Sigma~^-1 t), the conditional variance under q(u): block PCG solves over `block`
 *             cells at a time as vggp_qv_masked_iter runs them (operator, kept preconditioner basis, per-column stopping rule; no
 *             probes); info->rounds1 = largest PCG count, info->sweeps1 = number of block solves
 *   mean   DEVICE [mv1][mv2], every cell (NULL to skip)
 *   cells  HOST int64 [n_cells] flat indices a*mv2 + b, or NULL with n_cells = mv1*mv2 for every cell
 *   var    DEVICE [n_cells] (NULL with n_cells = 0: the mean only)
 *   W, n_obs (masked), tol, max_iter, block: as vggp_qv_masked_iter
 * VGGP_ESTATE unless the LAST finished step on the context was the matching successful iterative step; VGGP_ENOCONV when a column does
 * not converge; VGGP_EINVAL on paired contexts and -- the GRIDDED read-outs alone among the iterative entries -- on multi-rank contexts
 * (the message says so; vggp_qv_*_iter and vggp_posterior_*_iter run there), the wrong plan kind (a grid against VGGP_FLAG_SCATTERED), a cell index
 * outside [0, mv1*mv2), block > 64.  The block solve's workspace is the iterative read-outs' (allocated on first use, apart from the
 * step's): a read-out leaves the kept preconditioner basis valid and the next step's results unchanged. */
int vggp_readout_masked_iter(vggp_ctx* ctx, const double* W, double n_obs, const double* C1, int64_t mv1, const double* C2, int64_t mv2,
                             const double* kd1, const double* kd2, const int64_t* cells, int64_t n_cells, double tol, int max_iter,
                             int block, double* mean, double* var, int flags, vggp_info* info, void* stream);
int vggp_readout_scattered_iter(vggp_ctx* ctx, const double* C1, int64_t mv1, const double* C2, int64_t mv2, const double* kd1,
                                const double* kd2, const int64_t* cells, int64_t n_cells, double tol, int max_iter, int block,
                                double* mean, double* var, int flags, vggp_info* info, void* stream);
/* Building block of the literal read-out, exported for tests: out[a][b] = sum_k P1[a][k]^2 P2[b][k]^2 on DEVICE arrays P1 [mv1][N],
 * P2 [mv2][N], out [mv1][mv2]; any mv_d >= 1 (mv1 mv2 < 2^28).  An fp64-MFMA GEMM whose operands are squared as its fragments are
 * formed; reduction split over workgroups, slabs summed in fixed order: bitwise reproducible.  The context need not be planned. */
int vggp_kr_sqgram(vggp_ctx* ctx, const double* P1, const double* P2, int64_t mv1, int64_t mv2, int64_t N, double* out, void* stream);
/* q(v) of the last masked step: mean and covariance diagonal, DEVICE [m1][m2]. */
int vggp_qv_masked(vggp_ctx* ctx, double* mean, double* var, void* stream);
/* posterior(x*) of the last masked step (kronecker_structure.py:199-230); arguments as vggp_posterior. */
int vggp_posterior_masked(vggp_ctx* ctx, const double* xs1, const double* xs2, int64_t n_star, double* mean, double* var,
                          void* stream);

/* Gridded read-out q(v) of B0 cell features v from the posterior over the inducing features u of the last finished step
 * (q_u -> p(v|u) -> q_v; gridded_kronecker_structure.py:396-438 SVGP, :613-654 VFF, :903-947 ASVGP), Kronecker in the
 * per-dimension cross-covariances: C_d DEVICE [mv_d][m_d] = Cov(v, u) along dimension d at UNIT outputscale (Kvu_d / s_d
 * for kernel-evaluated features, Kvu_d itself for VFF / B1 features), kd_d DEVICE [mv_d] = diag(Kvv_d) / s_d.
 * mean, var DEVICE [mv1][mv2]:  mean = Kvu Kuu^-1 mu_u;  var = diag(Kvv - Kvu Kuu^-1 Kuv + Kvu X Kuv) with
 * X = S_u^-1 when flags & VGGP_READOUT_LITERAL (what the reference's q_v computes, :431) and X = Kuu^-1 S_u Kuu^-1
 * (the conditional variance of v under q(u)) otherwise. */
#define VGGP_READOUT_LITERAL 1
int vggp_readout(vggp_ctx* ctx, const double* C1, int64_t mv1, const double* C2, int64_t mv2, const double* kd1, const double* kd2,
                 double* mean, double* var, int flags, void* stream);

/* The same read-out from the M-space state of the last MASKED or SCATTERED step (the Gridded* models on data that is no full
 * grid: along-track observations, notebook 61); arguments as vggp_readout. */
int vggp_readout_masked(vggp_ctx* ctx, const double* C1, int64_t mv1, const double* C2, int64_t mv2, const double* kd1, const double* kd2,
                        double* mean, double* var, int flags, void* stream);

/* q(v) of the last finished step: mean and diagonal of the covariance, both DEVICE
 * [m1][m2] (flat index u = i1*m2+i2).  Replaces Matern12GriddedGP.q_v
 * (gridded_kronecker_structure.py:1409-1433 == kronecker_structure.py:825-849). */
int vggp_qv(vggp_ctx* ctx, double* mean, double* var, void* stream);
/* Dense M x M covariance Kuu Sigma^{-1} Kuu of q(v) (DEVICE, M = m1*m2; small M only). */
int vggp_qv_cov(vggp_ctx* ctx, double* cov, void* stream);

/* Joint (correlated) samples of q(v) without any M x M matrix -- what `.sample(torch.Size([S]))` gives on the MultivariateNormal the
 * reference's q_v() returns (kronecker_structure.py:825-849).  All read-outs share one whitened form,
 *     Cov q(v) = s1^e1 s2^e2 (L0_1 (x) L0_2) Sigma~^-1 (L0_1 (x) L0_2)^T,  Sigma~ = I + rho Phi,  rho = s1 s2 / sigma^2,  e_d as vggp_qv_masked_iter,
 * so sample s is  V_s = mean + sqrt(s1^e1 s2^e2) L0_1 X_s L0_2^T  with Cov(vec X_s) = Sigma~^-1, and the mean is the one vggp_qv* returns.
 *   full grid (vggp_qv_sample, state of vggp_elbo_step / vggp_elbo_finish; the route of vggp_qv_cov: the accurate state, then the kept
 *       Q_d, 1/D, L0_d):  X_s = Sigma~^-1/2 E_s = Q1 ((Q1^T E_s Q2) o D^-1/2) Q2^T,  D = 1 + rho lam1 lam2^T,  E_s m1 x m2 standard normals.
 *       The SYMMETRIC root: independent of the signs, order and cluster bases of the eigenvectors.  No solve, no tolerance.
 *   iterative masked / scattered (pathwise):  Z_s = E_s + sqrt(rho) K F_s,  X_s = Sigma~^-1 Z_s, with F_s standard normals over the n1 x n2
 *       nodes resp. the N points and K the second half of the step's operator (K F = B1 (W^T o F) B2^T resp. sum_k F_k b1_k b2_k^T), so
 *       that Cov(vec Z_s) = Sigma~ exactly.  ONE block PCG solve per `block` <= 64 samples: the solve of vggp_qv_masked_iter /
 *       vggp_qv_var_scattered_iter (operator, kept preconditioner basis, per-column stopping rule, the read-outs' own workspace).
 *       tol, max_iter, block, info, W, n_obs exactly as there: info->rounds1 = largest PCG count, info->sweeps1 = number of block solves.
 * Noise.  eps_u DEVICE [n_samples][m1][m2] is E, eps_obs DEVICE [n_samples][n2][n1] (grid; the layout of Y and W) resp. [n_samples][N]
 * (points) is F; on the iterative entries either both are given and used as they are (values on unobserved nodes are not read into the
 * result), or both are NULL and the noise is generated on the device by vggp_normal_fill's generator from (seed, first):
 *       E  stream 0, idx = s M + i1 m2 + i2;     F  stream 1, idx = s n1 n2 + j n1 + i (grid), s N + k (points);     s = first + local sample.
 * Sample s of a seed is therefore the same numbers whatever n_samples, block, or the call that asks for it: out(first = 5, n = 1) is row 5
 * of out(first = 0, n = 70), bit for bit on the iterative entries, to rounding (1e-12) on the full grid.  A column of zero noise returns
 * the mean bit for bit.
 *   out   DEVICE [n_samples][m1][m2], flat cell index of vggp_qv
 * VGGP_ESTATE unless the last finished step on the context was the matching successful step (the rules of vggp_qv_cov, vggp_qv_masked_iter,
 * vggp_qv_var_scattered_iter); VGGP_ENOCONV when a column does not converge; VGGP_EINVAL on paired contexts, the wrong plan kind,
 * n_samples < 1, first < 0, a NULL out, only one of eps_u / eps_obs, block > 64, and on multi-rank contexts (the message says so: the
 * counter-based noise is what a multi-rank version will need, it is not built).  A sampling call between two steps leaves the next
 * step's bits unchanged. */
int vggp_qv_sample(vggp_ctx* ctx, int64_t n_samples, uint64_t seed, int64_t first, const double* eps_u, double* out, void* stream);
int vggp_qv_sample_masked_iter(vggp_ctx* ctx, const double* W, double n_obs, int64_t n_samples, uint64_t seed, int64_t first,
                               const double* eps_u, const double* eps_obs, double tol, int max_iter, int block, double* out,
                               vggp_info* info, void* stream);
int vggp_qv_sample_scattered_iter(vggp_ctx* ctx, int64_t n_samples, uint64_t seed, int64_t first, const double* eps_u,
                                  const double* eps_obs, double tol, int max_iter, int block, double* out, vggp_info* info, void* stream);
/* The same samples from the DENSE M-space state of the last successful vggp_elbo_step_masked or vggp_elbo_step_scattered (one entry for
 * both data kinds, as vggp_qv_masked).  The step keeps Xg = L^-1, the inverse of the Cholesky factor of Sigma~ = L L^T, lower triangular,
 * and the coefficient draw is
 *     X_s = Xg^T E_s,     Cov(vec X_s) = Xg^T Xg = Sigma~^-1,
 * one launch of vggp_tri_t_apply's kernel per block of min(64, block, n_samples) samples: no factorisation, no solve, no tolerance and no
 * M x M temporary, at every M <= 16384.  (A root of Sigma~^-1 other than the symmetric one: the samples have the distribution of
 * vggp_qv_cov_masked, they are not the numbers a symmetric root gives.)  The mean is vggp_qv_masked's, bit for bit; the tail -- L0_1 X
 * L0_2^T, the scale, the mean -- is the iterative entries'.  eps_u DEVICE [n_samples][m1][m2] or NULL (stream 0 from (seed, first), the
 * E_s of every other sampler); there is no eps_obs, W, tol or max_iter; info->rounds* and info->sweeps* are 0 (info may be NULL).  Sample
 * s of a seed is the same numbers whatever n_samples, block or call asks for it, bit for bit; zero noise returns the mean bit for bit.
 * Workspace: 4 M nbc + M doubles of the samplers' own scratch (the raster samplers'); the step's state -- Xg, the factor, Sigma~^-1,
 * a0 -- is only read: the point-wise read-outs return the same bits before and after, and a call between two steps changes no bit of
 * the second step.  VGGP_ESTATE unless the LAST finished step on the context is a successful dense masked / scattered one (not after
 * vggp_plan alone, a full-grid step or an iterative step); VGGP_EINVAL before anything is launched or written on paired contexts,
 * multi-rank contexts, n_samples < 1, first < 0, a NULL out, block > 64. */
int vggp_qv_sample_masked(vggp_ctx* ctx, int64_t n_samples, uint64_t seed, int64_t first, const double* eps_u, int block, double* out,
                          vggp_info* info, void* stream);
/* Its product as a building block, exported for tests, on caller-supplied DEVICE arrays: Xl [M][M] row-major, M = m1 m2 <= 16384, lower
 * triangular -- NOTHING above its diagonal is read (NaN included); E and out block vectors in the samplers' interleaved layout
 * [m1][nbc][m2], element (cell u = i1 m2 + i2, column c) at (i1 nbc + c) m2 + i2; 1 <= cn <= nbc <= 64:
 *     out(u, c) = sum_{k >= u} Xl[k][u] E(k, c)  for c < cn,     out(u, c) = 0  for cn <= c < nbc.
 * ONE fp64-MFMA kernel: the sample columns are one operand, a 32-column tile of Xl the other (row k of Xl is contiguous along u: the
 * triangle streams once, in 256-byte runs).  Workgroup b takes column tile b and its mirror nt - 1 - b, so every workgroup streams the
 * same number of rows (static balance, no work queue); M = 16384 gives 256 workgroups.  Each output element is summed by one wave in
 * ascending k from the first row of its tile: no split-K, no atomics, bitwise repeatable, and the bits of a column depend neither on
 * its position in the block nor on cn or nbc.  Edges (M no multiple of 4, 16, 32 or 64, a tile that straddles an i1 boundary of the
 * layout, cn < nbc < 64, M < nbc, M = 1) are handled in the kernel: nothing is padded or copied.  Indices are 64-bit.  The launch is
 * asynchronous on `stream`.  VGGP_EINVAL: a NULL argument, sizes outside the ranges above, out == E (the product cannot run in place).
 * The context need not be planned.  (VGGP_TRI_T_GEMM=1 in the environment routes a call with m1 = 1 through the batch GEMM and its
 * 128-granular triangular skip instead: the yardstick of tools/bench_dense_sample.py, not a route any sampler takes.) */
int vggp_tri_t_apply(vggp_ctx* ctx, const double* Xl, int64_t m1, int64_t m2, const double* E, int nbc, int cn, double* out, void* stream);

/* Gradient of the ELBO of the LAST vggp_elbo_step with respect to the inducing-point coordinates of the "points" basis
 * (Matern12SVGP and friends register Z as a trainable Parameter, kronecker_structure.py:303-304, and let autograd differentiate
 * through kernel(Z) :318-319 and kernel(cartesian_prod(Z), x) :336-337).  Y: the same device array the step was given.
 * gz1 [m1], gz2 [m2] (device): d ELBO / d z_d[i]; zeros for a dimension whose basis is not VGGP_BASIS_POINTS.
 * Analytic (no autograd): the sensitivities Kbar = L^-T W_M L^-1, Abar = L^-T W_V follow from the linearity of the lengthscale
 * gradient in (dK, dA), and d kappa(z, x)/dz = -(d kappa/d ell) ell / (z - x) for the stationary kernels.
 * Row-sharded contexts: Y is the rank's slab; the parts of the ranks' rows are summed by one all-reduce of m1 + m2 doubles. */
int vggp_zgrad(vggp_ctx* ctx, const double* Y, double* gz1, double* gz2, void* stream);

/* Collapsed ELBO and gradient for N SCATTERED observations (along-track points: the reference's _elbo(), kronecker_structure.py
 * :249-278, receives arbitrary (x1, x2) pairs in notebooks 6 / 61 / 7 and evaluates Kuf densely, :808-823).  The context must have
 * been planned with VGGP_FLAG_SCATTERED (x1[k], x2[k] = the coordinates of point k, n1 = n2 = N).  y [N] device, yy = sum y^2.
 * Kuf[:, k] = a1(x1_k) (x) a2(x2_k) is a Khatri-Rao product: Sigma~ = I + rho sum_k (b1_k (x) b2_k)(b1_k (x) b2_k)^T is assembled
 * in M-space (M = m1 m2 <= 16384) by one GEMM over the points and factored densely, as in the masked step; cost O(M^2 N + M^3).
 * vggp_qv_masked / vggp_posterior_masked / the *_cov_masked entries read the result. */
int vggp_elbo_step_scattered(vggp_ctx* ctx, const double* y, double yy, const double theta[5], double* elbo_out,
                             double grad_out[5], vggp_info* info, void* stream);

/* Gradient of the scattered ELBO w.r.t. the inducing coordinates (what the reference obtains from autograd through _elbo()
 * into the Z Parameter of its SVGP classes, kronecker_structure.py:303-304, when X holds scattered points), after
 * vggp_elbo_step_scattered on the same y: gz1 [m1], gz2 [m2] (DEVICE; zeros for a dimension that does not use the points
 * basis).  One more M x M x N product; workspace 2 M N doubles (M N < 2^31).  Point-sharded contexts: the parts of the ranks'
 * points are summed by one all-reduce of m1 + m2 doubles. */
int vggp_zgrad_scattered(vggp_ctx* ctx, const double* y, double* gz1, double* gz2, void* stream);

/* New inducing coordinates z[0..m) (host array) for dimension dim (0 or 1) of a planned context whose basis there is
 * VGGP_BASIS_POINTS, without re-planning: arena, captured graphs and the eigensolver's warm start are kept.  What an optimiser
 * that trains Z (kronecker_structure.py:303-304 registers it as a Parameter) calls between steps.  Read-outs need a new step. */
int vggp_set_inducing(vggp_ctx* ctx, int dim, const double* z, int64_t m);

/* Point-wise posterior at ns scattered test points (xs1[p], xs2[p]) (DEVICE inputs):
 * mean[ns], var[ns] (DEVICE).  Replaces KroneckerStructure.posterior mean and the
 * diagonal of its covariance (kronecker_structure.py:199-230). */
int vggp_posterior(vggp_ctx* ctx, const double* xs1, const double* xs2, int64_t ns,
                   double* mean, double* var, void* stream);

/* posterior(x*) on a RASTER: the p1 x p2 cartesian grid of two coordinate axes, what every map of the reference evaluates
 * (kronecker_structure.py:199-230 with X* built from a meshgrid).  g1 DEVICE [p1], g2 DEVICE [p2]; mean, var DEVICE [p1][p2], flat
 * index a p2 + b; by definition the values the point-wise entry of the state gives at the points (g1[a], g2[b]).  On a raster the
 * whitened factors are needed at the axis coordinates only, T_d = Q_d^T L0_d^-1 A_d(g_d) (q_d x p_d), and
 *     mean = T1^T (Wm T2),      var = s1 s2 (1 + (T1 o T1)^T (Wv (T2 o T2)))
 * with the compact weights of vggp_posterior: O(p1 p2 q1) in one fp64-MFMA launch (vggp_raster_contract below) instead of the
 * O(p1 p2 q1 q2) of the point-wise contraction.  Reads the LAST finished step on the context, whichever kind it was:
 *   vggp_elbo_step / vggp_elbo_finish   mean and variance; vggp_posterior's preamble (accurate recompute after a warm step, thin read-out)
 *   vggp_elbo_step_masked / _scattered, vggp_elbo_step_masked_iter, vggp_elbo_step_scattered_iter
 *                                       mean = (s1 s2 / sigma^2) U1^T A0 U2 from the state's m1 x m2 coefficients, U_d = L0_d^-1 A_d(g_d);
 *                                       var must be NULL (VGGP_EINVAL before anything is launched: those variances t^T Sigma~^-1 t are no
 *                                       Kronecker sums -- vggp_posterior_masked, vggp_posterior_masked_iter,
 *                                       vggp_posterior_var_scattered_iter give them point by point; after the two DENSE steps
 *                                       vggp_posterior_raster_var_masked below gives mean and variance on the raster)
 * var = NULL: the mean only, on every state.  1 <= p_d <= 2^20; output indices are 64-bit.  Workspace (the context's lazy scratch):
 * 2 m1 p1 + (2 m2 + 2 m1) p2 + m1^2 + m2^2 doubles after a full-grid step (the last two: W_d = Q_d^T L0_d^-1), 2 m1 p1 + (2 m2 + m1) p2
 * after the other steps; nothing of size p1 p2.  VGGP_ESTATE without a finished step (the rules of the state's point-wise
 * entry); VGGP_EINVAL on paired contexts.  Multi-rank contexts: as the state's point-wise entry (the state is replicated; after an
 * iterative step the transport is verified and polled, no collective).  A raster call between two steps leaves the second step's bits
 * unchanged wherever vggp_posterior does: after a cold or thin full-grid step and after the masked, scattered and iterative steps.  After a
 * WARM full-grid step the first read-out of either kind runs the accurate recompute, which replaces the basis the next step starts from;
 * the next step then returns the bits it returns after a vggp_posterior call in the raster call's place (both tested). */
int vggp_posterior_raster(vggp_ctx* ctx, const double* g1, int64_t p1, const double* g2, int64_t p2, double* mean, double* var,
                          void* stream);
/* Its kernel as a building block, exported for tests, on caller-supplied DEVICE arrays: T1 [q][P1], U, Uv [q][P2], outputs [P1][P2],
 *     mean[a][b] = sum_i T1[i][a] U[i][b],      var[a][b] = c0 + c1 sum_i T1[i][a]^2 Uv[i][b]
 * One fp64-MFMA launch, 64 x 64 output tiles; the variance product's A fragment is the square of the mean product's, taken in
 * registers; edges (P_d no multiple of 64, q no multiple of 4) are handled in the kernel, nothing is padded or copied.  var = NULL (Uv
 * may then be NULL) skips the second product.  1 <= q, P1, P2 <= 2^20.  The context need not be planned. */
int vggp_raster_contract(vggp_ctx* ctx, const double* T1, const double* U, const double* Uv, int64_t q, int64_t P1, int64_t P2,
                         double c0, double c1, double* mean, double* var, void* stream);

/* Mean AND variance on the raster after a successful vggp_elbo_step_masked or vggp_elbo_step_scattered -- the dense M-space states,
 * where vggp_posterior_raster gives the mean only.  Arguments as vggp_posterior_raster (g1 DEVICE [p1], g2 DEVICE [p2]; mean, var
 * DEVICE [p1][p2], flat index a p2 + b, both required).  The mean is vggp_posterior_raster's (the same launches, the same bits).  The
 * variance var = s1 s2 (1 - |t|^2 + t^T Sinv t) is no Kronecker sum -- Sinv = Sigma~^-1 is a dense M x M matrix -- but every raster
 * column is rank one, t_ab = u1_a (x) u2_b with u_d = L0_d^-1 a_d(g_d), so the quadratic form separates one axis at a time
 * (vggp_kron_quadform below, n_d = squared column norms of U_d, kd = 1, scale = s1 s2 read from theta on the device):
 * 2 p1 M^2 + 2 p1 p2 m2^2 flops instead of the 2 p1 p2 M^2 of vggp_posterior_masked at the p1 p2 points, to which it agrees to rounding
 * (the same form summed in another order; tested at 1e-6 relative, measured: DESIGN.md).  The chunk's intermediate sits in the step's
 * M x M scratch where vggp_posterior_masked keeps its T; Sinv, a0 and everything a later read-out or step reads is left untouched: the
 * point-wise read-outs return the same bits before and after, and a call between two steps changes no bit of the second step (tested).
 * Workspace otherwise: vggp_posterior_raster's 2 m1 p1 + (2 m2 + m1) p2 doubles of the context's lazy scratch.
 * VGGP_ESTATE unless the LAST finished step on the context is a dense masked / scattered one (not after vggp_plan alone, a full-grid
 * step or an iterative step: those have no Sinv).  VGGP_EINVAL before anything is launched on paired contexts, multi-rank contexts,
 * NULL arguments, p_d outside [1, 2^20]. */
int vggp_posterior_raster_var_masked(vggp_ctx* ctx, const double* g1, int64_t p1, const double* g2, int64_t p2, double* mean, double* var,
                                     void* stream);
/* Its contraction as a building block, exported for tests, on caller-supplied DEVICE arrays: S [M][M] (M = m1 m2 <= 16384, flat index
 * (i m2 + j) M + k m2 + l; it need NOT be symmetric), U1 [m1][P1], U2 [m2][P2], n1 [P1], n2 [P2] (both or neither), out [P1][P2]:
 *     out[a][b] = scale (kd - n1[a] n2[b] + sum_{i,j,k,l} U1[i][a] U2[j][b] S[(i m2 + j) M + k m2 + l] U1[k][a] U2[l][b])
 * n1 = n2 = NULL and kd = 0, scale = 1 give the bare quadratic form (u1_a (x) u2_b)^T S (u1_a (x) u2_b).  Two launches of ONE fp64-MFMA
 * kernel (64 x 64 output tiles) per chunk of the P1 axis,
 *     Gt[(j,l)][a] = sum_{(i,k)} S((i,k), (j,l)) U1[i][a] U1[k][a]           (m2^2 x chunk, K = m1^2; S read through the index view, no copy)
 *     out[a][b]    = scale (kd - n1[a] n2[b] + sum_{(j,l)} Gt[(j,l)][a] U2[j][b] U2[l][b])                      (chunk x P2, K = m2^2)
 * whose second operand, the Khatri-Rao self-product V[p][c] V[q][c], is formed from two coalesced loads and one multiply while the
 * fragments are staged and never stored.  Edges (K no multiple of 4 or 16, rows / columns no multiple of 64, view tiles that straddle
 * a j boundary) are handled in the kernel: nothing is padded or copied.  No split-K and no atomics: one wave sums each element in
 * ascending k, so results are bitwise repeatable.
 * Chunk rule: the P1 axis is processed in chunks of chunk = min(P1, m1^2) columns (the last one may be shorter), so that Gt -- m2^2 x
 * chunk doubles of the context's lazy scratch -- never passes M^2 doubles.  1 <= P1, P2 <= 2^20.  The context need not be planned. */
int vggp_kron_quadform(vggp_ctx* ctx, const double* S, int64_t m1, int64_t m2, const double* U1, int64_t P1, const double* U2, int64_t P2,
                       const double* n1, const double* n2, double kd, double scale, double* out, void* stream);

/* Joint (correlated) samples of posterior(x*) on a raster: n_samples realisations of f on the p1 x p2 cartesian grid of the axes g1, g2
 * (DEVICE [p1], [p2]), what `.sample()` gives on the MultivariateNormal the reference's posterior() returns for X* = cartesian_prod(g1, g2)
 * (kronecker_structure.py:199-230), without any p1 p2 x p1 p2 matrix.  With the state of the last finished step -- L0_d, theta, and X_s the
 * whitened coefficient draw of the vggp_qv_sample* entries above, Cov(vec X_s) = Sigma~^-1, produced by the very same stage --
 *     U_d = L0_d^-1 A0_d(g_d),  B_d = sqrt(s_d) U_d  (m_d x p_d),     k_d = the unit POINT kernel of dimension d on its axis (p_d x p_d),
 *     r_d = k_d - U_d^T U_d,     C_d = chol(r_d + eta I),     Kc2 = chol(k_2 + eta I),     eta = 1e-8 (a fixed nugget at unit outputscale),
 *     F_s = mu + B1^T W_s + sqrt(s1 s2) C1 T_s,     W_s = X_s B2 + sqrt(s2) H_s C2^T  (m1 x p2),     T_s = G_s Kc2^T  (p1 x p2),
 * mu = the mean vggp_posterior_raster returns in the same state, G_s [p1][p2] and H_s [m1][p2] standard normals, so that
 *     Cov(vec F_s) = (B1 (x) B2)^T Sigma~^-1 (B1 (x) B2) + s1 s2 (r1 + eta I) (x) (k2 + eta I) + (B1^T B1) (x) s2 (r2 + eta I)
 * = K** + Kuf*^T Sigma^-1 Kuf* - Kuf*^T Kuu^-1 Kuf* (:223-229) plus the nugget terms (about 2 eta s1 s2 of extra variance): the prior
 * residual k1 (x) k2 - q1 (x) q2 = (k1 - q1) (x) k2 + q1 (x) (k2 - q2) is a sum of two PSD Kronecker products.  Cost per sample
 * 2 m1 m2 p2 + 2 m1 p2^2 + p1 p2^2 + 2 m1 p1 p2 + p1^2 p2 flops; the roots (per call, nothing is cached) are three p_d x p_d Cholesky
 * factorisations by vggp_cholesky_inverse, its jitter schedule on top of the nugget: info->jitter1 = the level C1 took, info->jitter2 =
 * the larger of C2's and Kc2's (0 on every tested problem); VGGP_ENOTPD when a root fails every level.
 * Noise.  eps_u [n_samples][m1][m2] (E) and, on the iterative entries, eps_obs (F) as the vggp_qv_sample* entries; eps_g DEVICE
 * [n_samples][p1][p2] is G, eps_h DEVICE [n_samples][m1][p2] is H.  Either ALL of an entry's noise arrays are given, or all are NULL and
 * the noise is generated on the device from (seed, first): streams 0 and 1 as above and
 *       G  stream 2, idx = s p1 p2 + a p2 + b;     H  stream 3, idx = s m1 p2 + i p2 + b;     s = first + local sample.
 * Sample s of a seed is the same numbers whatever n_samples, block or call asks for it (to 1e-12), and it uses the E_s of sample s of
 * vggp_qv_sample* with that seed: the two are one joint draw.  Zero noise returns mu bit for bit.
 *   out   DEVICE [n_samples][p1][p2], flat index a p2 + b
 * Samples are processed in blocks of min(64, block, n_samples) samples, fewer when the block's p1 x p2 scratch would pass 1 GiB (one
 * sample if a single map is larger); G is generated into `out`.  The number of launches of a block does not depend on the samples in
 * it.  Iterative entries: W, n_obs, tol, max_iter, block, info->rounds1 / sweeps1 as vggp_qv_sample_*_iter (one block solve per block
 * of samples).  Workspace (the context's own, kept): p1 p2 + 2 m1 p1 + 2 m2 p2 + 2 p1^2 + 3 p2^2 + max(p1, p2)^2 + nbc (2 m1 p2 + p1 p2)
 * doubles, plus 2 nbc m1 m2 on a full grid.
 * State rules: those of the matching vggp_qv_sample* entry (the full-grid entry: after vggp_elbo_step / vggp_elbo_finish; it takes mu
 * first, then the accurate state as vggp_qv_sample does); a call between two steps leaves the next step's bits unchanged wherever
 * that entry does.  VGGP_EINVAL before anything is launched or written: paired contexts; a dimension with VGGP_BASIS_B1 (its residual
 * k_d - q_d is indefinite: that covariance is no Schur complement); multi-rank contexts; p_d < 1 or p_d > 8192 (the Cholesky's limit);
 * n_samples < 1; first < 0; NULL out or axes; only some of the noise arrays; block > 64. */
int vggp_posterior_raster_sample(vggp_ctx* ctx, const double* g1, int64_t p1, const double* g2, int64_t p2, int64_t n_samples, uint64_t seed,
                                 int64_t first, const double* eps_u, const double* eps_g, const double* eps_h, double* out, vggp_info* info,
                                 void* stream);
int vggp_posterior_raster_sample_masked_iter(vggp_ctx* ctx, const double* g1, int64_t p1, const double* g2, int64_t p2, const double* W,
                                             double n_obs, int64_t n_samples, uint64_t seed, int64_t first, const double* eps_u,
                                             const double* eps_obs, const double* eps_g, const double* eps_h, double tol, int max_iter,
                                             int block, double* out, vggp_info* info, void* stream);
int vggp_posterior_raster_sample_scattered_iter(vggp_ctx* ctx, const double* g1, int64_t p1, const double* g2, int64_t p2, int64_t n_samples,
                                                uint64_t seed, int64_t first, const double* eps_u, const double* eps_obs, const double* eps_g,
                                                const double* eps_h, double tol, int max_iter, int block, double* out, vggp_info* info,
                                                void* stream);
/* The same map samples from the dense M-space state of the last successful vggp_elbo_step_masked or vggp_elbo_step_scattered: X_s =
 * Xg^T E_s as vggp_qv_sample_masked draws it (the same launch on the same E_s: sample s of a seed is one joint draw across the two
 * entries), mu = the mean vggp_posterior_raster returns in this state, then the roots, the nugget, info->jitter1 / jitter2, the block
 * rule and the kernels of the entries above, unchanged.  No eps_obs, W, tol or max_iter: nothing is solved, info->rounds* and
 * info->sweeps* are 0.  Workspace: the list above plus 2 nbc m1 m2 doubles (E and X); the step's state is only read (the rules of
 * vggp_qv_sample_masked).  VGGP_ESTATE unless the LAST finished step is a successful dense masked / scattered one; VGGP_EINVAL before
 * anything is launched or written: the list of the entries above. */
int vggp_posterior_raster_sample_masked(vggp_ctx* ctx, const double* g1, int64_t p1, const double* g2, int64_t p2, int64_t n_samples,
                                        uint64_t seed, int64_t first, const double* eps_u, const double* eps_g, const double* eps_h, int block,
                                        double* out, vggp_info* info, void* stream);
/* Their last kernel as a building block, exported for tests, on caller-supplied DEVICE arrays: B1 [q][P1], Wt [S][q][P2], C1 [P1][P1]
 * lower triangular, Tt [S][P1][P2], mean [P1][P2] or NULL, out [S][P1][P2]:
 *     out[s][a][b] = mean[a][b] + sum_i B1[i][a] Wt[s][i][b] + c sum_{a' <= a} C1[a][a'] Tt[s][a'][b]
 * One fp64-MFMA launch for all samples, 64 x 64 output tiles; both products accumulate in the same registers; the triangular product's
 * k-range ends at the tile's last row, and nothing above the diagonal of C1 is read (NaN included); c = 0 skips that product; edges are
 * handled in the kernel, nothing is padded or copied; output indices are 64-bit.  1 <= q, P1, P2 <= 2^20, 1 <= S <= 65535.  The
 * context need not be planned. */
int vggp_raster_sample_contract(vggp_ctx* ctx, const double* B1, const double* Wt, const double* C1, const double* Tt, int64_t S, int64_t q,
                                int64_t P1, int64_t P2, double c, const double* mean, double* out, void* stream);

/* Dense ns x ns covariance of posterior(x*) (DEVICE [ns][ns]; ns <= 8192 and M ns <= 2^27): K** + Kuf*^T Sigma^-1 Kuf* -
 * Kuf*^T Kuu^-1 Kuf*, kronecker_structure.py:223-229, from the step's eigenbasis (never forming Sigma); the masked variant
 * from the dense Sigma~^-1 of the last masked / scattered step.  Callers that only need the diagonal use vggp_posterior.
 * vggp_posterior_cov_masked takes 1 <= ns <= M = m1 m2 points per call (T and Sigma~^-1 T live in the step's two M x M scratch
 * matrices and, unlike vggp_posterior_masked, a covariance cannot be chunked over the points): ns > M returns VGGP_EINVAL before
 * anything is launched or written, and the state of the step stays readable.  (A paired context has no ns <= M condition: above.) */
int vggp_posterior_cov(vggp_ctx* ctx, const double* xs1, const double* xs2, int64_t ns, double* cov, void* stream);
int vggp_posterior_cov_masked(vggp_ctx* ctx, const double* xs1, const double* xs2, int64_t ns, double* cov, void* stream);
/* Dense M x M covariance of q(v) of the last masked step (Kuu Sigma^-1 Kuu on the observed subset). */
int vggp_qv_cov_masked(vggp_ctx* ctx, double* cov, void* stream);

/* Exact GP on N scattered points, 1 <= N <= 16384 -- the dense baseline of the reference's notebooks: Matern12GP / Matern32GP /
 * Matern52GP (src/models/exact/bivariate_structure.py) and GriddedMatern12ExactGP (gridded_kronecker_structure.py:21-211).
 * kernel = kernel_1 * kernel_2 on active dims 0 and 1, s = s1 s2:
 *     K0[i, j] = k1(|x_i1 - x_j1| / ell1) k2(|x_i2 - x_j2| / ell2),  Sigma = s K0 + sigma2 I (+ eps I),  alpha = Sigma^-1 y,
 *     MLL = -1/2 [y^T alpha + log|Sigma| + N log 2 pi]   (what ExactMarginalLogLikelihood returns, times N).
 * eps follows the psd_safe_cholesky schedule on Sigma itself (0, 1e-8, 1e-7, 1e-6, then VGGP_ENOTPD), reported in vggp_info.jitter1.
 * The exact state is a workspace of its own on the context (about 4 N^2 doubles, allocated by vggp_exact_plan; VGGP_ENOMEM when the
 * device cannot hold it): it is independent of vggp_plan -- a planned sparse model keeps its state across exact calls and the exact
 * state survives a later vggp_plan -- and is replaced by the next vggp_exact_plan.  Single-rank contexts only.
 *
 * vggp_exact_plan: x1, x2 HOST [N] coordinates (finite), kind_d one of VGGP_KIND_*. */
int vggp_exact_plan(vggp_ctx* ctx, int kind1, int kind2, const double* x1, const double* x2, int64_t N);
/* MLL and its gradient with respect to the constrained theta (as vggp_elbo_step); y DEVICE [N].  Sigma is built from the coordinates,
 * factored by the blocked MFMA Cholesky + inverse, and W = alpha alpha^T - Sigma^-1 is contracted against K0 and dK0/d ell_d in one pass
 * over the upper tiles of Sigma^-1 (kernel derivatives evaluated on chip; fixed-order sums: bitwise repeatable).  One host
 * synchronisation.  Under vggp_profile the step charges the Sigma build to stage 0, Cholesky + inverse to stage 1, alpha to stage 5
 * and the gradient pass to stage 18. */
int vggp_exact_step(vggp_ctx* ctx, const double* y, const double theta[5], double* mll_out, double grad_out[5], vggp_info* info,
                    void* stream);
/* posterior(x*) of the last exact step at ns test points (DEVICE inputs and outputs): mean = s B*^T alpha,
 * var = s - s^2 diag(B*^T Sigma^-1 B*), B*[i, p] = k1(x_i1, x*_p1) k2(x_i2, x*_p2) (gpytorch's ExactGP prediction without
 * fast_pred_var); the predictive distribution adds sigma2.  vggp_exact_posterior_cov: the dense [ns][ns] covariance, ns <= 8192. */
int vggp_exact_posterior(vggp_ctx* ctx, const double* xs1, const double* xs2, int64_t ns, double* mean, double* var, void* stream);
int vggp_exact_posterior_cov(vggp_ctx* ctx, const double* xs1, const double* xs2, int64_t ns, double* cov, void* stream);
/* Gridded read-out q(v) of B0 cell features from the last exact step (GriddedMatern12ExactGP.q_v, gridded_kronecker_structure.py
 * :177-191; Matern-1/2 plans only: the cell integrals are Matern-1/2 closed forms).  C_d DEVICE [mv_d][N] = Cov(v, f(x_i)) along d at
 * unit outputscale (:52-101), kd_d DEVICE [mv_d] = diag(Kvv_d) / s_d; Kvx[(a, b), i] = s C1[a][i] C2[b][i], cells flat a mv2 + b.
 * mean, var DEVICE [mv1][mv2]: mean = Kvx alpha; var = s kd1 kd2 + diag(Kvx Kxv) / sigma2 with VGGP_READOUT_LITERAL -- the reference's
 * Kvv - Kvx Kxx^-1 Kxv + Kvx P^-1 Kxv, P = Kxx - Kxx Sigma^-1 Kxx, in the form P^-1 = Kxx^-1 + I / sigma2 that never inverts Kxx (a
 * Gram product over the points, no solve) -- and the conditional variance s kd1 kd2 - diag(Kvx Sigma^-1 Kxv) otherwise. */
int vggp_exact_readout(vggp_ctx* ctx, const double* C1, int64_t mv1, const double* C2, int64_t mv2, const double* kd1, const double* kd2,
                       double* mean, double* var, int flags, void* stream);
/* Errors of the exact entries: VGGP_EINVAL for a null context, N outside [1, 16384], a bad kind, non-finite coordinates, a theta
 * component <= 0, an n_ranks > 1 context, ns > 8192 (covariance), a read-out of cells on a plan that is not Matern-1/2; VGGP_ESTATE for a
 * step without a plan or a read-out before a successful step on the current plan. */

/* Iterative exact GP: the same model as vggp_exact_* at any N >= 1 with N * 64 < 2^31 (along-track data at N ~ 100 000), float64,
 * single-rank, bitwise repeatable (no floating-point atomics; every reduction in a fixed order).  Sigma = s K0 + sigma2 I is never
 * stored and takes no jitter: it is applied through vggp_exact_kmv's matrix-free product.  The reference reaches this size through
 * gpytorch's conjugate gradients and stochastic Lanczos quadrature above max_cholesky_size; this is that recipe with fixed probes.
 *     preconditioner  Nystroem on r = min(rank, N) strided landmarks idx_j = ((2 j + 1) N) / (2 r) (deterministic: no pivot search):
 *                     Lz Lz^T = s K0[idx, idx] (psd_safe jitter schedule, vggp_info.jitter1), L = s K0[:, idx] Lz^-T, P = sigma2 I +
 *                     L L^T, L^T L = V diag(lam) V^T (lam_i <= 1e-14 lam_max dropped), Q = L V lam^-1/2,
 *                     P^w = sigma2^w (I + Q diag((1 + lam / sigma2)^w - 1) Q^T), log|P| = N log sigma2 + sum log1p(lam / sigma2);
 *                     rank = 0: P = sigma2 I
 *     block           column 0: y; columns c >= 1: z_c = P^1/2 z0_c, z0_c Rademacher from the counter hash of the other iterative
 *                     steps (same seed constant), keyed on (c, i): the same probes on every device, every run
 *     PCG on Sigma, preconditioner P^-1, per-column stop |r| <= tol |r0|, columns go inactive individually; alpha = x_0
 *     log|Sigma| ~ log|P| + mean_c N e1^T log(T_c) e1 (T_c: Lanczos tridiagonal of the PCG coefficients of column c)
 *     tr(Sigma^-1 D) ~ mean_c u_c^T D w_c, u_c = x_c, w_c = P^-1 z_c: ONE derivative-mode product on [alpha, w_1 .. w_p]
 *     MLL = -1/2 [y^T alpha + log|Sigma| + N log 2 pi], dMLL/d ell_d = (s / 2) [alpha^T d_d K0 alpha - tr_d],
 *     dMLL/d s1 = (s2 / 2) [alpha^T K0 alpha - tr_K] (s2 symmetric), dMLL/d sigma2 = 1/2 [alpha^T alpha - tr_I]
 * The MLL and its gradient are ESTIMATES (alpha and y^T alpha are exact to the PCG tolerance): tests/exact_iter_spec.py holds the
 * same-probe numpy specification and the measured errors.  The workspace is O(N (64 + rank)) doubles, independent of vggp_plan and of
 * the dense exact workspace, and is replaced by the next vggp_exact_iter_plan.
 *
 * vggp_exact_iter_plan: x1, x2 HOST [N] coordinates (finite), kind_d one of VGGP_KIND_*. */
int vggp_exact_iter_plan(vggp_ctx* ctx, int kind1, int kind2, const double* x1, const double* x2, int64_t N);
/* y DEVICE [N]; theta as vggp_exact_step.  n_probes <= 0: 16 (at most 63); rank < 0: 64 (at most 256); tol <= 0: 1e-10; max_iter <= 0:
 * 1000 (gpytorch's max_cg_iterations).  info: jitter1 = the landmark factor's jitter, rounds1 = PCG iterations, sweeps1 = probes.
 * One value-only product per iteration for the whole block (one host synchronisation per iteration: the count of active columns). */
int vggp_exact_step_iter(vggp_ctx* ctx, const double* y, const double theta[5], int n_probes, int rank, double tol, int max_iter,
                         double* mll_out, double grad_out[5], vggp_info* info, void* stream);
/* posterior(x*) from the state of the last successful iterative step (alpha, theta, Q, lam): xs1, xs2 DEVICE [ns], mean, var DEVICE [ns]
 * (var NULL: mean only).  mean = s K0(x*, X) alpha, one rectangular product; var = s - s^2 b*^T Sigma^-1 b*, b*_p = K0(X, x*_p) as
 * explicit [N][64] blocks: ceil(ns / 64) block PCG solves (info: sweeps1 = solves, rounds1 = the largest iteration count).  A column's
 * numbers do not depend on its neighbours.  There is no dense covariance on this solver. */
int vggp_exact_posterior_iter(vggp_ctx* ctx, const double* xs1, const double* xs2, int64_t ns, double tol, int max_iter, double* mean,
                              double* var, vggp_info* info, void* stream);
/* Gridded read-out q(v) as vggp_exact_readout (Matern-1/2 plans; C_d DEVICE [mv_d][N], kd_d DEVICE [mv_d], cells flat a mv2 + b):
 * mean DEVICE [mv1][mv2] = s C1 diag(alpha) C2^T, one GEMM.  var (may be NULL): with VGGP_READOUT_LITERAL DEVICE [mv1][mv2] =
 * s kd1 kd2 + s^2 (C1 o C1)(C2 o C2)^T / sigma2, a Gram product without a solve; otherwise the conditional variance at the n_cells
 * cells of the HOST list `cells`, DEVICE [n_cells], from the block PCG with columns s C1[a] o C2[b]. */
int vggp_exact_readout_iter(vggp_ctx* ctx, const double* C1, int64_t mv1, const double* C2, int64_t mv2, const double* kd1,
                            const double* kd2, const int64_t* cells, int64_t n_cells, double tol, int max_iter, double* mean, double* var,
                            int flags, vggp_info* info, void* stream);
/* Errors of the iterative exact entries: VGGP_EINVAL for a bad kind, non-finite coordinates, a theta component <= 0, n_probes > 63,
 * rank > 256, a cell out of range, a conditional variance without cells, cells on a plan that is not Matern-1/2, an n_ranks > 1
 * context; VGGP_ESTATE without a plan, or for a read-out without a successful step on the current plan; VGGP_ENOCONV when a column
 * does not converge within max_iter (this ends the state); VGGP_ENOTPD when the landmark factor fails after jitter 1e-6; VGGP_ENOMEM. */

/* building blocks (exported for tests, benchmarks and re-use) ---------------- */
/* Matrix-free kernel-matrix product of the exact GP's K0 (the building block of an iterative exact solver beyond N = 16384; no plan
 * needed, single-rank contexts only):
 *     out0[i][c] = sum_j K0(xr_i, xc_j) V[j][c],  K0(a, b) = k1(|a1 - b1| / ell1) k2(|a2 - b2| / ell2) at unit outputscale,
 *     out1, out2 = the same with dK0/d ell1 and dK0/d ell2 in the same pass (both NULL: value only; out0 is the same bits either way).
 * Row points xr1, xr2 DEVICE [Nr], column points xc1, xc2 DEVICE [Nc] (the square case passes the same arrays twice; the rectangular
 * case is a posterior mean), V DEVICE [Nc][nb] row-major, out* DEVICE [Nr][nb], 1 <= nb <= 64, Nr, Nc in [1, 2^25), kind_d any of
 * VGGP_KIND_* (mixed pairs included).  K0 is never stored: each lane generates its fragment of v_mfma_f64_16x16x4_f64 from the
 * coordinates with one exp per element, shared by the value and both derivatives (csrc/exact_iter.hip).  A row's sum over j is taken by
 * one workgroup in ascending j without atomics: bitwise repeatable.  VGGP_EINVAL for a null context or argument, a bad kind, a
 * lengthscale <= 0, sizes out of range, only one of out1 / out2, an n_ranks > 1 context. */
int vggp_exact_kmv(vggp_ctx* ctx, int kind1, int kind2, double ell1, double ell2, const double* xr1, const double* xr2, int64_t Nr,
                   const double* xc1, const double* xc2, int64_t Nc, const double* V, int64_t nb, double* out0, double* out1, double* out2,
                   void* stream);

/* Counter-based standard normals, the noise of the vggp_qv_sample* entries (csrc/sample.hip): out[k] = element first_idx + k of the
 * sequence (seed, stream_id), DEVICE [n].  Philox4x32-10 with the published constants (multipliers 0xD2511F53, 0xCD9E8D57; Weyl
 * increments 0x9E3779B9, 0xBB67AE85), key = (seed & 0xffffffff, seed >> 32), counter = (c & 0xffffffff, c >> 32, stream_id, 0),
 * c = idx >> 1; from the output words w0..w3: a = (w0 << 21) | (w1 >> 11), u1 = (a + 0.5) 2^-53, b = (w2 << 21) | (w3 >> 11),
 * u2 = (b + 0.5) 2^-53, r = sqrt(-2 ln u1); element idx = r cos(2 pi u2) for even idx, r sin(2 pi u2) for odd idx.  u1 > 0, so
 * |z| <= 8.66.  An element depends on (seed, stream_id, idx) alone: any split of a range gives the same bits.  The context need not
 * be planned.  VGGP_EINVAL: a NULL ctx, stream_id < 0, first_idx < 0, n < 0, a NULL out with n > 0; n = 0 writes nothing. */
int vggp_normal_fill(vggp_ctx* ctx, uint64_t seed, int stream_id, int64_t first_idx, int64_t n, double* out, void* stream);

/* Unit-outputscale factor build for one dimension: A0[m][n], dA0/d ell [m][n],
 * K0[m][m], dK0/d ell [m][m] (any output pointer may be NULL).  x DEVICE [n];
 * grid DEVICE ([m+1] mesh for B0 and B0K, [m] coords for POINTS).
 * Replaces _Kuu_along_dim/_Kuf_along_dim (kronecker_structure.py:702-790) and the
 * pairwise kernel_d(Z), kernel(Z, x) evaluations (:318-319, :336-337).
 * Range: every ell > 0 gives finite outputs.  The B0 Kuu is evaluated as ell^2 e^{-(k-1)t} expm1(-t)^2 with
 * t = delta / ell (delta = grid[1] - grid[0]), which neither overflows nor cancels for any t > 0 (for t -> inf the
 * neighbour-cell covariance tends to ell^2, cells further apart underflow to 0).  At LARGE ell / delta the B0 closed forms
 * cancel: relative error about eps * ell/delta in A0 and K0 and eps * (ell/delta)^2 in dA0 and dK0 (5e-11 at
 * ell = 320 delta, 7e-7 at ell = 3.2e4 delta; table in DESIGN.md section 5a); with VGGP_FLAG_B0_F32_KDELTA the
 * reference-literal three-exponential Kuu loses a further factor ell/delta.  The B0K forms of Matern-3/2 and -5/2 (edge-term
 * differences for A0, E (a0 + k a1 + k^2 a2) with expm1-built mesh constants for K0) are finite for every ell > 0 as well and cancel
 * more steeply at large ell / delta (their derivatives fall off like (delta/ell)^3): table in DESIGN.md section 5a.
 * VGGP_EINVAL: ell <= 0, B0 / VFF / B1 with a kind other than Matern-1/2, B0K with RBF or with VGGP_FLAG_B0_F32_KDELTA, a NULL grid,
 * a NULL x with A0 or dA0 requested.
 * n = 0 is allowed (only K0 / dK0 are written). */
int vggp_factor_build(vggp_ctx* ctx, int kind, int basis, const double* x, int64_t n,
                      const double* grid, int64_t m, double ell, int flags,
                      double* A0, double* dA0, double* K0, double* dK0, void* stream);

/* Cholesky K + jitter*I = L L^T with the psd_safe_cholesky jitter schedule (0, 1e-8,
 * 1e-7, 1e-6) and the explicit inverse of L.  K, L, Linv DEVICE [m][m] row-major.
 * Replaces the Cholesky hidden inside lazify(Kuu).inv_matmul (kronecker_structure.py:269).
 * jitter_out HOST (may be NULL).
 * Only the LOWER triangle of K is read (i >= j), as numpy / LAPACK do: anything above the diagonal, NaN included, changes no bit
 * of the result.  L and Linv are written as whole m x m matrices, exact zeros above the diagonal; nothing outside them is written.
 * The lowest level that succeeds is the one returned, and it is the oracle's (oracle/kron.py chol_jitter).
 *   m <= 128   one launch, the four levels race in four workgroups;  m > 128   blocked (128-wide panels), one attempt per level.
 * VGGP_ENOTPD (no level is positive definite; also a K with NaN on or below the diagonal): *jitter_out = -1.0;
 *   m <= 128: L and Linv are NaN throughout;  m > 128: L and Linv are unspecified (partly NaN).  The next call is unaffected.
 * VGGP_EINVAL: a NULL ctx, K, L or Linv, m < 1, m > 8192 -- checked before any memory is touched (*jitter_out keeps its value). */
int vggp_cholesky_inverse(vggp_ctx* ctx, const double* K, int64_t m, double* L, double* Linv,
                          double* jitter_out, void* stream);

/* Symmetric eigendecomposition G = Q diag(lam) Q^T by parallel cyclic Jacobi.
 * G DEVICE [m][m]; lam DEVICE [m]; Qt DEVICE [m][m] with ROW j = eigenvector j.
 * Any finite symmetric G is accepted: indefinite, exactly rank deficient, repeated eigenvalues (within a cluster Qt is AN orthonormal
 * basis, not a particular one), already diagonal (lam is then the diagonal bit for bit and Qt has entries 0 and +-1 only), any overall
 * scale whose squares stay finite (2^-200 .. 2^200 tested), and the zero matrix (lam = 0, Qt orthonormal, *sweeps_out may be 0).
 * Order of lam: flags = 0 (scalar cyclic Jacobi) returns the pairs sorted, lam[0] >= lam[1] >= ...; VGGP_FLAG_BLOCK_JACOBI (m <= 128;
 * larger m runs the scalar solver) returns them in no particular order.  sweeps_out HOST (may be NULL).  Bitwise repeatable.
 * VGGP_EINVAL: a NULL ctx, G, lam or Qt, m < 1, m > 256 -- before any memory is touched;  VGGP_ENOCONV: sweep limit (60 / 30) reached.
 * NaN or inf in G is outside the contract (the pipeline's Cholesky fails first). */
int vggp_eigh(vggp_ctx* ctx, const double* G, int64_t m, double* lam, double* Qt,
              int32_t* sweeps_out, int flags, void* stream);

/* The four single-workgroup kernels of the thin chain (csrc/step.hip chain_thin: the step of numerically rank-deficient Gram matrices,
 * RBF factors), one job each on caller-supplied DEVICE arrays, exported for tests.  Each entry validates what its launcher validates
 * (plus NULL pointers) before any memory is touched -- VGGP_EINVAL otherwise --, launches exactly the kernel a step launches for such a
 * job (no rider), and synchronises the stream before it returns.  None of them changes what a step launches.
 *
 * vggp_pivchol   cold range finder (csrc/thin.hip vg_pivchol_kernel): r steps of diagonally pivoted Cholesky of the symmetric G [m][m];
 *                row i of V [r][m] is the i-th column l_i.  Pivot = largest residual diagonal, ties to the lowest index, a pivot is used
 *                once; a step whose pivot is not positive writes row i of Omega [r][m] instead.  1 <= r <= min(m, 64), m <= 256.
 * vggp_rowqr     row orthonormalisation (csrc/eigh.hip vg_rowqr_kernel_t): V1 [r][m] = the rows of Z [r][m] orthonormalised in the given
 *                order (classical Gram-Schmidt, re-orthogonalised where a pass removed more than half of a row); also copies cp_n doubles
 *                cp_src -> cp_dst (cp_n = 0: both may be NULL).  1 <= r <= min(m, 64), m <= 256.  m > 128 selects the wide instantiation
 *                (four elements per lane), cp_n > 0 at m <= 128 the one with the pass-through copy in registers.
 * vggp_ritz      Rayleigh-Ritz solve of the symmetric matrix whose lower triangle is tril(Hl Hr^T) (Hl, Hr [r][hk] row-major; the
 *                product is formed by the eigensolver's producer workgroup, csrc/eigh.hip vg_eigh_kernel, factors staged in LDS when
 *                r <= 48 and hk <= 128), Newton start first (r <= 48) and Jacobi sweeps when it declines.  lam [r] decreasing, row j
 *                of W [r][r] = Ritz vector j.  counters_out HOST [4] (may be NULL): [0] logged rotation rounds, [1] iterations or sweeps
 *                | numerical rank << 8 (Ritz values above 1e-14 of the largest), [2] solver status, [3] the producer's final word: bit 27
 *                set = the Newton start was taken.  err_out HOST (may be NULL): the eigensolver's error bits.  1 <= r <= 64,
 *                r <= hk <= 256: the envelope of the two chains (the product form exists in the solver's LDS variant only, so the
 *                launcher's own bound r <= 256 does not hold for it).  VGGP_ENOCONV when [2] or the error bits are set.
 * vggp_thin_tail the thin m-space stage (csrc/thin.hip vg_thin_tail_kernel): from the Ritz pairs and the r x r sandwiches to the bound, its
 *                gradient, beta and 1/D on range x range, the subspace-miss check and the packed 128-byte result block.  All arrays
 *                DEVICE; out [8], beta_out / invd_out [r1][r2] (both or neither), peer_fail, jit[d], status[d] ([2]: Cholesky status,
 *                eigensolver error bits) and rcounters[d] ([4]) may be NULL; hout [16] doubles (the result block: out[8], jitter[2],
 *                int32 counters[2][4], int32 status[2], sequence number = theta[5]) may be NULL too.  1 <= r_d <= min(m_d, 32),
 *                m_d <= 256, ac_nslab >= 1. */
typedef struct vggp_thin_tail_args {
    const double* theta;              /* [6]: ell1, ell2, s1, s2, v, sequence number */
    double n_total, yy;
    int32_t r1, r2, m1, m2;
    const double *W1, *W2;            /* [r][r], row j = Ritz vector j */
    const double *lam1, *lam2;        /* [r] Ritz values, unit scale, decreasing */
    const double *AM1, *AH1, *AM2, *AH2;   /* [r][r]: V1 Mk0 V1^T, V1 H0 V1^T */
    const double* AC;                 /* [3][r1][r2]: V1_1 {C, C1, C2} V1_2^T, as the fixed-order sum of ac_nslab slabs ac_slab doubles apart */
    int32_t ac_nslab;
    int64_t ac_slab;
    const double *G1, *H1, *G2, *H2;  /* [m][m]: only the diagonals are read */
    double* out;
    double *beta_out, *invd_out;
    double* hout;
    const double* peer_fail;
    const double* jit[2];
    const int32_t* status[2];
    const int32_t* rcounters[2];
} vggp_thin_tail_args;
int vggp_pivchol(vggp_ctx* ctx, const double* G, const double* Omega, int64_t m, int64_t r, double* V, void* stream);
int vggp_rowqr(vggp_ctx* ctx, const double* Z, int64_t r, int64_t m, double* V1, const double* cp_src, double* cp_dst, int64_t cp_n,
               void* stream);
int vggp_ritz(vggp_ctx* ctx, const double* Hl, const double* Hr, int64_t r, int64_t hk, double* lam, double* W, int32_t* counters_out,
              int32_t* err_out, void* stream);
int vggp_thin_tail(vggp_ctx* ctx, const vggp_thin_tail_args* args, void* stream);

/* Strided fp64 MFMA GEMM  C[M][N] = op(A) op(B)  with element (i,k) of op(A) at
 * A[i*sa_m + k*sa_k] and (k,j) of op(B) at B[k*sb_k + j*sb_n]; C row-major, ld = ldc. */
int vggp_gemm(vggp_ctx* ctx, const double* A, int64_t sa_m, int64_t sa_k,
              const double* B, int64_t sb_k, int64_t sb_n,
              double* C, int64_t ldc, int64_t M, int64_t N, int64_t K, void* stream);

/* Triangular solve by substitution on the matrix cores: L X = R (trans = 0) or L^T X = R (trans = 1), L DEVICE [m][m]
 * lower-triangular (row-major, the upper part is not read), R, X DEVICE [m][ncols] row-major (X may alias R).
 * Blocked: 16 x 16 diagonal blocks inverted in a wave, 128 x 128 diagonal blocks solved from LDS, the rest by MFMA GEMM
 * updates (csrc/trsm.hip).  Replaces the triangular solves inside lazify(Kuu).inv_matmul (kronecker_structure.py:269).
 * "Not read" means: no value above the diagonal of L, NaN included, reaches the result.  Componentwise backward error
 * |op(L) X - R| <= kappa16 m u |op(L)| |X|, kappa16 = largest infinity-norm condition number of the 16 x 16 diagonal blocks (measured:
 * below m u).  VGGP_EINVAL: a NULL ctx, L, R or X, m < 1, m > 16384, ncols < 1, m ncols >= 2^31 -- before any
 * memory is touched. */
int vggp_trsm(vggp_ctx* ctx, const double* L, int64_t m, const double* R, int64_t ncols, double* X, int trans, void* stream);

/* Kronecker solve  X = K1^{-1} Y K2^{-T},  K_d = L_d L_d^T,  from the CHOLESKY FACTORS (BASELINE metric ii; nothing is
 * pre-inverted by the caller, the whole solve is inside this call), X = L1^{-T} (L1^{-1} Y L2^{-T}) L2^{-1}, never
 * materialising K1 (x) K2.  n1, n2 <= 128: four triangular solves by substitution (vggp_trsm's strip kernel).  Larger
 * factors: their 128 x 128 diagonal blocks are inverted by substitution on the identity, the rest of L^{-1} follows by
 * block doubling (two MFMA GEMM launches per level), and the four applications are triangular-aware MFMA GEMMs that skip
 * the zero half -- a substitution sweep over n / 128 block rows is a chain of 2 n / 128 dependent launches per solve
 * (1.3 ms at n = 1024 against 0.3 ms; VGGP_KRON_SUBST=1 selects it).  L1 [n1][n1], L2 [n2][n2] lower-triangular
 * (e.g. from vggp_cholesky_inverse), Y, X DEVICE [n1][n2] (X may alias Y).
 * Replaces Kuu.inv_matmul(.) with Kuu = torch.kron(Kuu_1, Kuu_2) (kronecker_structure.py:269, :805).
 * Only the lower triangles of L1 and L2 are used.  The three forms (default, VGGP_KRON_SUBST=1, VGGP_KRON_FOUR=1; the switches are
 * read once per process) compute the same X: bit for bit on exactly representable data.  The result does not depend on what earlier
 * calls left in the context's scratch.  VGGP_EINVAL: a NULL ctx, L1, L2, Y or X, n_d < 1, n_d > 16384, n1 n2 >= 2^31 -- before any
 * memory is touched. */
int vggp_kron_solve(vggp_ctx* ctx, const double* L1, int64_t n1, const double* L2, int64_t n2,
                    const double* Y, double* X, void* stream);

/* Per-stage timing with HIP events on the stream the kernels are launched on (bench.py's
 * live roofline measurement).  When enabled, every ELBO step records one event after each
 * launch group; vggp_profile_read returns the accumulated milliseconds per stage. */
#define VGGP_NSTAGE 20
int         vggp_profile(vggp_ctx* ctx, int enable);
int         vggp_profile_read(vggp_ctx* ctx, double ms_out[VGGP_NSTAGE], int32_t* steps_out, int reset);
const char* vggp_stage_name(int stage);
/* Name of the kernel the last projection launch (S = [B2;V2] Y, the only pass over Y) dispatched: the roofline kernel. */
const char* vggp_project_kernel_name(void);

/* sum of squares of a DEVICE array, summed over all ranks of the context (yy_total); result to HOST. */
int vggp_sumsq(vggp_ctx* ctx, const double* y, int64_t n, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VGGP_H */
