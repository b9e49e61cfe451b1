// ================================================================================================================================
// Read-outs of the iterative step: q(v) and posterior(x*) without Sigma~^-1 as a matrix (vggp_qv_masked_iter,
// vggp_posterior_masked_iter).  The algebra is vggp_qv_masked's / vggp_posterior_masked's; every quantity belongs to a rank-one
// whitened column t = u1 (x) u2:
//     mean = (s1 s2 / v) t^T a0,      var = s1 s2 (kappa - |t|^2 + t^T Sigma~^-1 t)
//   posterior(x*)   u_d = L0_d^-1 a_d(x*_d), kappa = 1
//   q(v) at (i1,i2) u_d = row i_d of L0_d,  kappa = |t|^2  ->  var = s1^e1 s2^e2 t^T Sigma~^-1 t;  the mean of ALL cells is
//                   L0_1 A0 L0_2^T (two GEMMs, no solve)
// t^T Sigma~^-1 t comes from a block PCG solve Sigma~ X = T over `block` <= 64 columns at a time in the step's interleaved layout
// [m1][nbc][m2], with the step's operator, its preconditioner (the basis and Rayleigh quotients it left in d.Qt, d.lam0) and its
// per-column stopping rule.  No probes: deterministic.  Workspace of its own (w.rmem): the step's arena, with the kept
// preconditioner basis Qk1/Qk2 in it, is not touched.  Specification: tests/masked_iter_readout_spec.py.
// ================================================================================================================================
#include "mspace_ws.h"

// The rank-one right-hand sides of a block: T[i][c][j] = U1(i, a_c) U2(j, b_c) for the cn columns of this block; the unused columns of a
// ragged block are zero.  A factor is addressed as base[i sf + a sc] (i: feature, a: the column's own index in this dimension):
//   posterior(x*)   U_d [m_d][cn]: sf = cn, sc = 1, a_c = b_c = c (div = 0)
//   q(v)            rows of L0_d: sf = 1, sc = m_d; column c belongs to cell u = cells[c] (or p0 + c) = a m2 + b (div = m2)
//   gridded         U_d [m_d][mv_d]: sf = mv_d, sc = 1; cell p = cells[c] (or p0 + c) = a mv2 + b (div = mv2)
struct VgRank1Factor { const double* base; long sf, sc; };
// which cell a column stands for: cells[c], or p0 + c when the list is null
struct VgCellRule { const long long* cells; long p0, div; };
__device__ static inline long vgi_cell(const VgCellRule& r, int c) { return r.cells ? (long)r.cells[c] : r.p0 + c; }
__global__ void vgi_rank1_kernel(const VgRank1Factor F1, const VgRank1Factor F2, const VgCellRule rule, int m1, int nbc, int m2, int cn, double* T) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)m1 * nbc * m2) return;
    const int j = (int)(idx % m2), c = (int)((idx / m2) % nbc), i = (int)(idx / ((long)m2 * nbc));
    if (c >= cn) { T[idx] = 0.0; return; }
    long a = c, b = c;
    if (rule.div) { const long p = vgi_cell(rule, c); a = p / rule.div; b = p - a * rule.div; }
    T[idx] = F1.base[i * F1.sf + a * F1.sc] * F2.base[j * F2.sf + b * F2.sc];
}
// one workgroup per column: lin = <T, a0>, nrm = <T, T>, quad = <T, X> in one pass, then the epilogue writes the scaled outputs of the column
//   posterior   mean = (s1 s2 / v) lin, var = s1 s2 (1 - nrm + quad)
//   q(v)        var = s1^e1 s2^e2 quad
//   gridded     var = s1 s2 (kd1_a kd2_b - nrm + quad) at the column's cell (a, b)
struct VgiPostEpilogue {
    double *mean, *var;
    __device__ void operator()(int c, double lin, double nrm, double quad, const double* theta) const {
        const double ss = theta[2] * theta[3];
        mean[c] = (ss / theta[4]) * lin;
        var[c] = ss * (1.0 - nrm + quad);
    }
};
struct VgiQvEpilogue {
    int e1, e2;
    double* var;
    __device__ void operator()(int c, double, double, double quad, const double* theta) const {
        var[c] = (e1 > 0 ? theta[2] : 1.0 / theta[2]) * (e2 > 0 ? theta[3] : 1.0 / theta[3]) * quad;
    }
};
struct VgiGridEpilogue {
    const double *kd1, *kd2;
    VgCellRule rule;
    double* var;
    __device__ void operator()(int c, double, double nrm, double quad, const double* theta) const {
        const long p = vgi_cell(rule, c);
        const long a = p / rule.div, b = p - a * rule.div;
        var[c] = theta[2] * theta[3] * (kd1[a] * kd2[b] - nrm + quad);
    }
};
template <class Epilogue>
__global__ __launch_bounds__(256) void vgi_readout_reduce_kernel(const double* T, const double* X, const double* a0, int m1, int nbc, int m2,
                                                                 const double* theta, const Epilogue epi) {
    __shared__ double red[12];
    const int c = blockIdx.x;
    double lin = 0.0, nrm = 0.0, quad = 0.0;
    for (long e = threadIdx.x; e < (long)m1 * m2; e += 256) {
        const long a = e / m2, b = e - a * m2, o = (a * nbc + c) * m2 + b;
        const double t = T[o];
        lin += t * a0[e];
        nrm += t * t;
        quad += t * X[o];
    }
    for (int off = 32; off > 0; off >>= 1) { lin += __shfl_xor(lin, off); nrm += __shfl_xor(nrm, off); quad += __shfl_xor(quad, off); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = lin; red[4 + (threadIdx.x >> 6)] = nrm; red[8 + (threadIdx.x >> 6)] = quad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lin = (red[0] + red[1]) + (red[2] + red[3]);
        nrm = (red[4] + red[5]) + (red[6] + red[7]);
        quad = (red[8] + red[9]) + (red[10] + red[11]);
        epi(c, lin, nrm, quad, theta);
    }
}
// x *= s1 s2 / sigma^2: the scale of a posterior / gridded mean (no basis exponents: the columns are whitened)
__global__ void vgs_scale_mean_kernel(double* x, long n, const double* theta) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= theta[2] * theta[3] / theta[4];
}

// What every read-out entry checks first: the context, the data kind of its plan (not_scattered / not_grid: the entry's own words for
// a plan of the other kind), W and n_obs of a masked step (bad_W: likewise) and the width of a block solve
// gridded: the gridded read-outs keep to single-rank contexts (their Gram products over the data have no collective); the point-wise
// ones run on a multi-rank context too: right-hand sides and results are replicated, the operator's all-reduce is vgi_apply's
static int vgi_readout_enter(vggp_ctx* c, const char* fn, bool scattered, bool gridded, const char* not_scattered, const char* not_grid,
                             const char* bad_W, const double* W, double n_obs, int block) {
    if (!c || !c->planned) { vg_set_error("%s: context not planned", fn); return VGGP_ESTATE; }
    VG_NOT_PAIRED(c, fn);
    if (scattered) VG_REQUIRE(c->desc.flags & VGGP_FLAG_SCATTERED, "%s: %s", fn, not_scattered);
    else VG_REQUIRE(!(c->desc.flags & VGGP_FLAG_SCATTERED), "%s: %s", fn, not_grid);
    if (gridded)
        VG_REQUIRE(!vgi_multi(c), "%s: the gridded read-out of an iterative step runs on single-rank contexts only (multi-rank contexts: "
                   "vggp_qv_*_iter / vggp_posterior_*_iter)", fn);
    else { const int vrc_ = vg_comm_verify(c, fn); if (vrc_) return vrc_; }
    if (!scattered) VG_REQUIRE(W && std::isfinite(n_obs) && n_obs > 0.0, "%s: %s", fn, bad_W);
    VG_REQUIRE(block <= 64, "%s: block = %d exceeds 64 columns per block solve", fn, block);
    return VGGP_OK;
}
// ... and, once its own arguments are checked: the block width (0: the widest that fits), a finished iterative step, the defaults of
// tol and max_iter, a zeroed info
static int vgi_readout_defaults(vggp_ctx* c, const char* fn, bool scattered, int* block, double* tol, int* max_iter, vggp_info* info) {
    const long n1 = c->desc.n1, n2 = c->desc.n2, M = (long)c->desc.m1 * c->desc.m2;
    auto fits = [&](long b) {
        return scattered ? (n1 * b < (1L << 31) && M * b < (1L << 31)) : (n1 * b * n2 < (1L << 31) * 4 && n1 * b < (1L << 31) && M * b < (1L << 31));
    };
    if (*block <= 0) { *block = 64; while (*block > 1 && !fits(*block)) *block >>= 1; }
    VG_REQUIRE(fits(*block), "%s: problem too large for block = %d", fn, *block);
    if (!c->have_iter || !c->masked) {
        vg_set_error("%s: no finished %s on this context", fn, scattered ? "vggp_elbo_step_scattered_iter" : "vggp_elbo_step_masked_iter");
        return VGGP_ESTATE;
    }
    if (*max_iter <= 0) *max_iter = 100;
    if (!(*tol > 0.0)) *tol = 1e-10;
    if (info) { info->jitter1 = info->jitter2 = 0.0; info->sweeps1 = info->sweeps2 = info->rounds1 = info->rounds2 = 0; info->status = 0; info->polished = 0; }
    return VGGP_OK;
}

// The read-outs' arena (w.rmem) for blocks of nbc columns, the transposed mask of a masked step in it, and the step's p.
// post: posterior(x*) needs the factor columns; sample: the joint samples need room for the mean.  Scattered points (n1 = N): no mask
// and no grid-sized buffers, fields [nbc][N]
static int vgi_readout_prepare(const vggp_ctx* c, VgMasked& w, VgReadout& r, int nbc, bool post, const double* W, double n_obs, hipStream_t st,
                               bool sample = false) {
    const size_t m1 = w.m1, m2 = w.m2, n1 = w.n1, n2 = w.n2, M = w.M, mx = std::max(m1, m2);
    VgIter& it = r.it;
    const bool sc = w.scattered;
    char oom[256];
    snprintf(oom, sizeof(oom), "the read-out workspace of the iterative step needs %%.1f GiB at block = %d but only %%.1f GiB of device "
             "memory are free (a smaller block needs less)", nbc);
    bool grew = false;
    const int rc = vg_arena_carve(&w.rmem, &w.rbytes, oom, &grew, [&](VgArena& a) {
        it.Wt = a.take(sc ? 0 : n1 * n2);
        it.X = a.take(M * nbc); it.R = a.take(M * nbc); it.Zp = a.take(M * nbc); it.Pd = a.take(M * nbc); it.AP = a.take(M * nbc);
        it.Tm = a.take(M * nbc); it.Tm2 = a.take(M * nbc); r.T = a.take(M * nbc);
        it.T1 = a.take(sc ? 0 : n1 * nbc * mx);
        it.F0 = a.take(sc ? n1 * nbc : n1 * nbc * n2);
        it.alh = a.take((size_t)nbc); it.beh = a.take((size_t)nbc);
        it.col = a.take(8 * (size_t)nbc);
        r.A1 = a.take(post ? m1 * nbc : 0); r.A2 = a.take(post ? m2 * nbc : 0);
        r.U1 = a.take(post ? m1 * nbc : 0); r.U2 = a.take(post ? m2 * nbc : 0);
        r.cells = reinterpret_cast<long long*>(a.take((size_t)nbc));
        it.krs = a.take(sc ? vg_kr_back_scratch((int)m1, (int)m2, (long)n1, nbc) : 0);
        it.nact = reinterpret_cast<int*>(a.take(8));
        it.part = a.take(2 * (size_t)nbc);
        r.mean = a.take(sample ? M : 0);
    });
    if (rc) return rc;
    r.p = vgi_obs_fraction(c, sc, n_obs);
    it.nbc = nbc; it.maxit = 1;
    if (!sc)
        hipLaunchKernelGGL(vgi_transpose_kernel, dim3((unsigned)((n1 + 31) / 32), (unsigned)((n2 + 31) / 32)), dim3(32, 8), 0, st, W, (long)n1, (long)n2,
                           it.Wt);
    return VGGP_OK;
}

// Sigma~ X = T for the block in r.T: the step's PCG (vgi_pcg) without the coefficient history and with the two-column field kernel.
// A function of (the step's operands, r.T) -> r.it.X for either data kind
static int vgi_readout_solve(vggp_ctx* c, VgMasked& w, VgReadout& r, double tol, int max_iter, int* iters, int* nact, hipStream_t st) {
    VG_HIP(hipMemcpyAsync(r.it.R, r.T, sizeof(double) * w.M * r.it.nbc, hipMemcpyDeviceToDevice, st));
    return vgi_pcg(c, w, r.it, r.p, tol, max_iter, /*history=*/false, /*field2=*/true, /*stale_limit=*/0, iters, nact, st);
}
// ... and what a read-out entry keeps of it: the number of block solves, the most iterations of one, VGGP_ENOCONV
static int vgi_solve_block(vggp_ctx* c, VgMasked& w, VgReadout& r, const char* fn, double tol, int max_iter, int* solves, int* max_its,
                           vggp_info* info, hipStream_t st) {
    int rc, iters = 0, nact = 0;
    if ((rc = vgi_readout_solve(c, w, r, tol, max_iter, &iters, &nact, st))) return rc;
    ++*solves;
    *max_its = std::max(*max_its, iters);
    if (info) { info->rounds1 = *max_its; info->sweeps1 = *solves; }
    if (nact > 0) {
        vg_set_error("%s: PCG did not reach %.1e in %d iterations (%d columns left, block solve %d)", fn, tol, max_iter, nact, *solves);
        return VGGP_ENOCONV;
    }
    return VGGP_OK;
}

// the cell list of a q(v) read-out: var comes with n_cells > 0, a null list means all n_all cells (`what`: the caller's name for n_all)
static int vgi_check_cells(const char* fn, const int64_t* cells, int64_t n_cells, const double* var, long n_all, const char* what) {
    VG_REQUIRE((n_cells == 0 && !var) || (n_cells > 0 && var), "%s: var and n_cells must be given together (NULL with 0: mean only)", fn);
    VG_REQUIRE(cells || n_cells == 0 || n_cells == n_all, "%s: cells = NULL means every cell: n_cells must be %s = %ld", fn, what, n_all);
    if (cells)
        for (int64_t k = 0; k < n_cells; ++k)
            VG_REQUIRE(cells[k] >= 0 && cells[k] < n_all, "%s: cells[%lld] = %lld is outside [0, %s = %ld)", fn, (long long)k, (long long)cells[k],
                       what, n_all);
    return VGGP_OK;
}

// mode 0: posterior at (xs1, xs2)[ncols];  mode 1: q(v) variance at cells[ncols] (host; null: every cell) and the mean of all cells
// scattered: the read-outs of vggp_elbo_step_scattered_iter (no W, n_obs: the Khatri-Rao operator over the n1 = N points, p = 1 / N)
static int vgi_readout_run(vggp_ctx* c, const char* fn, int mode, bool scattered, const double* W, double n_obs, const int64_t* cells,
                           const double* xs1, const double* xs2, int64_t ncols, double tol, int max_iter, int block, double* mean, double* var,
                           vggp_info* info, void* stream) {
    int rc = vgi_readout_enter(c, fn, scattered, /*gridded=*/false, "plan the context with VGGP_FLAG_SCATTERED", "the context was planned for scattered points",
                               "bad argument", W, n_obs, block);
    if (rc) return rc;
    const long m1 = c->desc.m1, m2 = c->desc.m2, M = m1 * m2;
    VG_REQUIRE(ncols >= 0, "%s: bad argument", fn);
    if (mode == 0) VG_REQUIRE(xs1 && xs2 && mean && var, "%s: null argument", fn);
    else if ((rc = vgi_check_cells(fn, cells, ncols, var, M, "M"))) return rc;
    if ((rc = vgi_readout_defaults(c, fn, scattered, &block, &tol, &max_iter, info))) return rc;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const int e1 = vg_uexp(d1.basis), e2 = vg_uexp(d2.basis);
    if (mode == 1 && mean && (rc = vgi_qv_mean(c, w, mean, st))) return rc;
    if (ncols == 0) { VGI_WAIT(c, st); return VGGP_OK; }
    const int nbc = (int)std::min<int64_t>(block, ncols);
    VgReadout r;
    if ((rc = vgi_readout_prepare(c, w, r, nbc, mode == 0, W, n_obs, st))) return rc;
    VgIter& it = r.it;
    const long nb = M * nbc;
    int max_its = 0, solves = 0;
    for (int64_t off = 0; off < ncols; off += nbc) {
        const int cn = (int)std::min<int64_t>(nbc, ncols - off);
        if (mode == 0) {
            if ((rc = vg_whitened_columns(c, xs1 + off, xs2 + off, cn, r.A1, r.A2, r.U1, r.U2, st))) return rc;
            VGM_LAUNCH1D(vgi_rank1_kernel, nb, st, VgRank1Factor{r.U1, cn, 1}, VgRank1Factor{r.U2, cn, 1}, VgCellRule{nullptr, 0, 0}, (int)m1, nbc,
                         (int)m2, cn, r.T);
        } else {
            if (cells) VG_HIP(hipMemcpyAsync(r.cells, cells + off, sizeof(long long) * cn, hipMemcpyHostToDevice, st));
            VGM_LAUNCH1D(vgi_rank1_kernel, nb, st, VgRank1Factor{d1.L0, 1, m1}, VgRank1Factor{d2.L0, 1, m2},
                         VgCellRule{cells ? r.cells : (const long long*)nullptr, (long)off, m2}, (int)m1, nbc, (int)m2, cn, r.T);
        }
        if ((rc = vgi_solve_block(c, w, r, fn, tol, max_iter, &solves, &max_its, info, st))) return rc;
        if (mode == 0)
            hipLaunchKernelGGL(vgi_readout_reduce_kernel<VgiPostEpilogue>, dim3(cn), dim3(256), 0, st, r.T, it.X, w.a0, (int)m1, nbc, (int)m2, c->theta,
                               VgiPostEpilogue{mean + off, var + off});
        else
            hipLaunchKernelGGL(vgi_readout_reduce_kernel<VgiQvEpilogue>, dim3(cn), dim3(256), 0, st, r.T, it.X, w.a0, (int)m1, nbc, (int)m2, c->theta,
                               VgiQvEpilogue{e1, e2, var + off});
    }
    VG_HIP(hipGetLastError());
    VGI_WAIT(c, st);
    return VGGP_OK;
}

extern "C" int vggp_qv_masked_iter(vggp_ctx* c, const double* W, double n_obs, const int64_t* cells, int64_t n_cells, double tol, int max_iter,
                                   int block, double* mean, double* var, vggp_info* info, void* stream) {
    return vgi_readout_run(c, "vggp_qv_masked_iter", 1, false, W, n_obs, cells, nullptr, nullptr, n_cells, tol, max_iter, block, mean, var, info, stream);
}

extern "C" int vggp_posterior_masked_iter(vggp_ctx* c, const double* W, double n_obs, const double* xs1, const double* xs2, int64_t ns,
                                          double tol, int max_iter, int block, double* mean, double* var, vggp_info* info, void* stream) {
    return vgi_readout_run(c, "vggp_posterior_masked_iter", 0, false, W, n_obs, nullptr, xs1, xs2, ns, tol, max_iter, block, mean, var, info, stream);
}

// q(v) mean of the last iterative scattered step: (s1 s2 / v) L1 A0 L2^T, scaled as vggp_qv_masked_iter scales it (no solve)
extern "C" int vggp_qv_scattered_iter(vggp_ctx* c, double* mean, void* stream) {
    static const char* fn = "vggp_qv_scattered_iter";
    int rc = vgs_check(c, fn);
    if (rc) return rc;
    VG_REQUIRE(mean, "%s: null output", fn);
    if (!c->have_iter || !c->masked) { vg_set_error("%s: no finished vggp_elbo_step_scattered_iter on this context", fn); return VGGP_ESTATE; }
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    if ((rc = vgi_qv_mean(c, w, mean, st))) return rc;
    VGI_WAIT(c, st);
    return VGGP_OK;
}

// posterior(x*) mean of the last iterative scattered step: (s1 s2 / v) u1^T A0 u2, u_d = L0_d^-1 a_d(x*_d), in chunks of points
extern "C" int vggp_posterior_scattered_iter(vggp_ctx* c, const double* xs1, const double* xs2, int64_t ns, double* mean, void* stream) {
    static const char* fn = "vggp_posterior_scattered_iter";
    int rc = vgs_check(c, fn);
    if (rc) return rc;
    VG_REQUIRE(xs1 && xs2 && mean && ns >= 0, "%s: bad argument", fn);
    if (!c->have_iter || !c->masked) { vg_set_error("%s: no finished vggp_elbo_step_scattered_iter on this context", fn); return VGGP_ESTATE; }
    if (ns == 0) return VGGP_OK;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    const long m1 = w.m1, m2 = w.m2;
    const long chunk = std::min<long>(ns, 1L << 16);
    if ((rc = vg_ensure_misc(c, (size_t)chunk * (3 * m1 + 2 * m2) * sizeof(double)))) return rc;
    double* p = (double*)c->misc;
    double* A1 = p; p += m1 * chunk;
    double* U1 = p; p += m1 * chunk;
    double* T = p; p += m1 * chunk;
    double* A2 = p; p += m2 * chunk;
    double* U2 = p;
    for (long off = 0; off < ns; off += chunk) {
        const int cn = (int)std::min<long>(chunk, ns - off);
        if ((rc = vg_whitened_columns(c, xs1 + off, xs2 + off, cn, A1, A2, U1, U2, st))) return rc;
        if ((rc = gemm1(w.a0, m2, 1, U2, cn, 1, T, cn, (int)m1, cn, (int)m2, st))) return rc;                   // A0 U2
        VGM_LAUNCH1D(vgm_coldot_kernel, cn, st, U1, T, (int)m1, (long)cn, mean + off);
        VGM_LAUNCH1D(vgs_scale_mean_kernel, cn, st, mean + off, (long)cn, c->theta);
    }
    VG_HIP(hipGetLastError());
    VGI_WAIT(c, st);
    return VGGP_OK;
}

// q(v) and posterior(x*) WITH their point-wise variances after the iterative scattered step: the iterative masked read-outs
// (vgi_readout_run) on the Khatri-Rao operator, ceil(columns / block) block PCG solves in the read-outs' own workspace
extern "C" int vggp_qv_var_scattered_iter(vggp_ctx* c, const int64_t* cells, int64_t n_cells, double tol, int max_iter, int block, double* mean,
                                          double* var, vggp_info* info, void* stream) {
    return vgi_readout_run(c, "vggp_qv_var_scattered_iter", 1, true, nullptr, 0.0, cells, nullptr, nullptr, n_cells, tol, max_iter, block, mean,
                           var, info, stream);
}
extern "C" int vggp_posterior_var_scattered_iter(vggp_ctx* c, const double* xs1, const double* xs2, int64_t ns, double tol, int max_iter,
                                                 int block, double* mean, double* var, vggp_info* info, void* stream) {
    return vgi_readout_run(c, "vggp_posterior_var_scattered_iter", 0, true, nullptr, 0.0, nullptr, xs1, xs2, ns, tol, max_iter, block, mean, var,
                           info, stream);
}

// ================================================================================================================================
// Joint samples of q(v) after an iterative step (vggp_qv_sample_masked_iter, vggp_qv_sample_scattered_iter), pathwise and without
// any M x M matrix.  Cov q(v) = s1^e1 s2^e2 (L0_1 (x) L0_2) Sigma~^-1 (L0_1 (x) L0_2)^T, so
//     V_s = mean + sqrt(s1^e1 s2^e2) L0_1 X_s L0_2^T,   X_s = Sigma~^-1 Z_s,   Z_s = E_s + sqrt(rho) K F_s,
// with E_s standard normal over the m1 x m2 cells, F_s standard normal over the data (grid nodes / points) and K the second half of
// the step's operator (masked grid: B1 (W^T o F) B2^T; points: sum_k F_k b1_k b2_k^T): Cov(vec Z_s) = I + rho Phi~ = Sigma~ exactly
// (W o W = W), hence Cov(vec X_s) = Sigma~^-1.  ONE block solve of the read-outs (vgi_readout_solve) serves up to 64 samples; all
// products work on the interleaved layout [m1][nbc][m2], one GEMM each, so a sample's bits do not depend on its block.  The noise is
// the caller's (eps_u, eps_obs) or the counter-based generator's (sample.hip).  Specification: tests/qv_sample_spec.py.
// ================================================================================================================================
// What the samplers of an iterative state check before anything is launched (vggp_qv_sample_*_iter, vggp_posterior_raster_sample_*_iter):
// the context and its plan kind, W / n_obs, the sample arguments (noise_ok: the entry's own all-or-none rule over its noise arrays), a
// finished iterative step; then the defaults of block, tol, max_iter and a zeroed info
int vgi_sample_enter(vggp_ctx* c, const char* fn, bool scattered, const double* W, double n_obs, int64_t n_samples, int64_t first, const void* out,
                     bool noise_ok, const char* noise_rule, double* tol, int* max_iter, int* block, vggp_info* info) {
    if (c && c->planned && !c->is_paired)
        VG_REQUIRE(!vgi_multi(c), "%s: joint samples run on single-rank contexts only (this context is multi-rank)", fn);
    int rc = vgi_readout_enter(c, fn, scattered, /*gridded=*/false, "plan the context with VGGP_FLAG_SCATTERED", "the context was planned for scattered points",
                               "bad argument", W, n_obs, *block);
    if (rc) return rc;
    VG_REQUIRE(n_samples >= 1 && n_samples < (1LL << 31), "%s: n_samples = %lld must be at least 1", fn, (long long)n_samples);
    VG_REQUIRE(first >= 0 && out, "%s: bad argument", fn);
    VG_REQUIRE(noise_ok, "%s: %s", fn, noise_rule);
    return vgi_readout_defaults(c, fn, scattered, block, tol, max_iter, info);
}
// the read-outs' workspace for blocks of nbc samples (qv_mean: room for the q(v) mean in r.mean)
int vgi_sample_prepare(vggp_ctx* c, VgReadout& r, int nbc, const double* W, double n_obs, bool qv_mean, hipStream_t st) {
    return vgi_readout_prepare(c, *reinterpret_cast<VgMasked*>(c->masked), r, nbc, false, W, n_obs, st, /*sample=*/qv_mean);
}
// The coefficient draw of the samplers of an iterative state, one block of nbc columns (cn live, first sample s0):
//     Z_s = E_s + sqrt(rho) K F_s,   X_s = Sigma~^-1 Z_s   by ONE block PCG solve  ->  r.it.X  [m1][nbc][m2]
// (E: eps_u or stream 0, F: eps_obs or stream 1; both point at the block's first sample)
int vgi_sample_coeffs(vggp_ctx* c, VgReadout& r, const char* fn, bool scattered, const double* eps_u, const double* eps_obs, uint64_t seed,
                      unsigned long long s0, int cn, double tol, int max_iter, int* solves, int* max_its, vggp_info* info, hipStream_t st) {
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    VgIter& it = r.it;
    const int m1 = w.m1, m2 = w.m2, nbc = it.nbc;
    const long n1 = w.n1, n2 = w.n2, nb = w.M * nbc;
    int rc;
    VG_HIP(vg_sample_block_noise_launch(r.T, eps_u, seed, s0, m1, nbc, m2, cn, st));
    VG_HIP(vg_sample_field_noise_launch(it.F0, scattered ? nullptr : it.Wt, eps_obs, seed, s0, n1, nbc, n2, cn, st));
    if (scattered) VG_HIP(vg_kr_back_launch(d1.BV, d2.BV, it.F0, m1, m2, n1, nbc, it.AP, it.krs, st));
    else if ((rc = vgi_back(w, it, d1.BV, it.F0, d2.BV, it.AP, st))) return rc;
    VG_HIP(vg_sample_fuse_launch(r.T, it.AP, c->theta, nb, st));                                               // Z = E + sqrt(rho) K F
    return vgi_solve_block(c, w, r, fn, tol, max_iter, solves, max_its, info, st);
}
static int vgi_sample_run(vggp_ctx* c, const char* fn, bool scattered, const double* W, double n_obs, int64_t n_samples, uint64_t seed,
                          int64_t first, const double* eps_u, const double* eps_obs, double tol, int max_iter, int block, double* out,
                          vggp_info* info, void* stream) {
    int rc = vgi_sample_enter(c, fn, scattered, W, n_obs, n_samples, first, out, (eps_u == nullptr) == (eps_obs == nullptr),
                              "eps_u and eps_obs are either both NULL (generated noise) or both given", &tol, &max_iter, &block, info);
    if (rc) return rc;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const int m1 = w.m1, m2 = w.m2, e1 = vg_uexp(d1.basis), e2 = vg_uexp(d2.basis);
    const long M = w.M, n1 = w.n1, n2 = w.n2;
    const long nodes = scattered ? n1 : n1 * n2;
    const int nbc = (int)std::min<int64_t>(block, n_samples);
    VgReadout r;
    if ((rc = vgi_sample_prepare(c, r, nbc, W, n_obs, /*qv_mean=*/true, st))) return rc;
    VgIter& it = r.it;
    if ((rc = vgi_qv_mean(c, w, r.mean, st))) return rc;
    int max_its = 0, solves = 0;
    for (int64_t off = 0; off < n_samples; off += nbc) {
        const int cn = (int)std::min<int64_t>(nbc, n_samples - off);
        if ((rc = vgi_sample_coeffs(c, r, fn, scattered, eps_u ? eps_u + off * M : nullptr, eps_obs ? eps_obs + off * nodes : nullptr, seed,
                                    (unsigned long long)(first + off), cn, tol, max_iter, &solves, &max_its, info, st)))
            return rc;
        if ((rc = gemm1(d1.L0, m1, 1, it.X, (long)nbc * m2, 1, it.Tm, nbc * m2, m1, nbc * m2, m1, st))) return rc;     // L0_1 X
        if ((rc = gemm1(it.Tm, m2, 1, d2.L0, 1, m2, it.Tm2, m2, m1 * nbc, m2, m2, st))) return rc;                     // (.) L0_2^T
        VG_HIP(vg_sample_out_launch(it.Tm2, r.mean, c->theta, e1, e2, m1, nbc, m2, cn, out + off * M, st));
    }
    VGI_WAIT(c, st);
    return VGGP_OK;
}
extern "C" int vggp_qv_sample_masked_iter(vggp_ctx* c, const double* W, double n_obs, int64_t n_samples, uint64_t seed, int64_t first,
                                          const double* eps_u, const double* eps_obs, double tol, int max_iter, int block, double* out,
                                          vggp_info* info, void* stream) {
    return vgi_sample_run(c, "vggp_qv_sample_masked_iter", false, W, n_obs, n_samples, seed, first, eps_u, eps_obs, tol, max_iter, block, out, info,
                          stream);
}
extern "C" int vggp_qv_sample_scattered_iter(vggp_ctx* c, int64_t n_samples, uint64_t seed, int64_t first, const double* eps_u,
                                             const double* eps_obs, double tol, int max_iter, int block, double* out, vggp_info* info,
                                             void* stream) {
    return vgi_sample_run(c, "vggp_qv_sample_scattered_iter", true, nullptr, 0.0, n_samples, seed, first, eps_u, eps_obs, tol, max_iter, block, out,
                          info, stream);
}

// ================================================================================================================================
// Gridded read-out q(v) of B0 cell features after an ITERATIVE step (vggp_readout_masked_iter, vggp_readout_scattered_iter): the
// algebra and scaling of vggp_readout_masked with Sigma~^-1 applied instead of stored.  U_d = L0_d^-1 C_d^T (m_d x mv_d); cell (a, b)
// owns the rank-one column t = U1[:, a] (x) U2[:, b];  rho = s1 s2 / sigma^2.
//   mean       rho U1^T A0 U2 for all cells: two GEMMs on the a0 the step left, no solve
//   literal    var = s1 s2 (kd1_a kd2_b - |t|^2 + t^T Sigma~ t): the |t|^2 cancel and t^T Phi t is a Gram product over the data,
//                  var[a][b] = s1 s2 (kd1[a] kd2[b] + rho S[a][b]),   P_d = U_d^T B_d (mv_d x n_d)
//                  scattered   S = (P1 o P1)(P2 o P2)^T over the N points: vg_kr_sqgram on chunks of points (P_d exists for one chunk only;
//                              the partial S are accumulated in chunk order)
//                  masked      S = (P1 o P1) W^T (P2 o P2)^T: two of the step's GEMMs on the squared P_d
//              no solve (info->sweeps1 = 0), all cells for about one operator application
//   conditional var = s1 s2 (kd1_a kd2_b - |t|^2 + t^T Sigma~^-1 t): block PCG solves Sigma~ X = T (vgi_readout_solve) over `block` <= 64
//              cells at a time, deterministic
// Specification: tests/gridded_iter_readout_spec.py.
// ================================================================================================================================
// literal: var[q] = s1 s2 (kd1[a] kd2[b] + rho S[a][b]) at cell p = cells[q] (or q)
__global__ void vgi_readout_literal_kernel(const double* S, const double* kd1, const double* kd2, const double* theta, const long long* cells,
                                           long mv2, long n, double* var) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const long p = cells ? (long)cells[q] : q;
    const long a = p / mv2, b = p - a * mv2;
    const double ss = theta[2] * theta[3];
    var[q] = ss * (kd1[a] * kd2[b] + (ss / theta[4]) * S[p]);
}

static int vgi_gridded_run(vggp_ctx* c, const char* fn, bool scattered, const double* W, double n_obs, const double* C1, int64_t mv1,
                           const double* C2, int64_t mv2, const double* kd1, const double* kd2, const int64_t* cells, int64_t n_cells,
                           double tol, int max_iter, int block, double* mean, double* var, int flags, vggp_info* info, void* stream) {
    int rc = vgi_readout_enter(c, fn, scattered, /*gridded=*/true, "the context was planned for a grid (vggp_readout_masked_iter reads those)",
                               "the context was planned for scattered points (vggp_readout_scattered_iter reads those)", "bad argument (W, n_obs)",
                               W, n_obs, block);
    if (rc) return rc;
    const long m1 = c->desc.m1, m2 = c->desc.m2, n1 = c->desc.n1, n2 = c->desc.n2, M = m1 * m2;
    VG_REQUIRE(C1 && C2 && kd1 && kd2 && mv1 > 0 && mv2 > 0 && mv1 < (1L << 20) && mv2 < (1L << 20) && mv1 * mv2 < (1L << 28) && n_cells >= 0,
               "%s: bad argument (C_d, kd_d non-null, mv_d >= 1, mv1 mv2 < 2^28)", fn);
    const long ncell_all = mv1 * mv2;
    if ((rc = vgi_check_cells(fn, cells, n_cells, var, ncell_all, "mv1 mv2"))) return rc;
    VG_REQUIRE(mean || var, "%s: nothing to compute (mean and var are NULL)", fn);      // (both null: n_cells is 0 and the list is not read)
    if ((rc = vgi_readout_defaults(c, fn, scattered, &block, &tol, &max_iter, info))) return rc;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const double *B1 = d1.BV, *B2 = d2.BV;
    const bool literal = (flags & VGGP_READOUT_LITERAL) != 0;
    const bool lit = literal && n_cells > 0;
    // the literal path forms P_d = U_d^T B_d for `chunk` points (scattered) / the n_d grid nodes (masked) at a time
    long chunk = 0;
    if (lit && scattered) {
        chunk = std::min<long>(n1, 1L << 16);
        while ((mv1 + mv2) * chunk > (1L << 25) && chunk > 4096) chunk >>= 1;
    }
    const long np1 = lit ? (scattered ? chunk : n1) : 0, np2 = lit ? (scattered ? chunk : n2) : 0;
    const size_t sq = lit && scattered ? vg_kr_sqgram_scratch((int)mv1, (int)mv2, chunk) : 0;
    size_t need = 0;
    auto room = [&](size_t count) { const size_t o = need; need += (count + 31) & ~size_t(31); return o; };
    const size_t oU1 = room(m1 * mv1), oU2 = room(m2 * mv2), oTm = room(mv1 * std::max(m2, lit && !scattered ? n2 : 0L));
    const size_t oCells = room(cells ? (size_t)n_cells : 0);
    const size_t oP1 = room(mv1 * np1), oP2 = room(mv2 * np2), oS = room(lit ? ncell_all : 0), oSq = room(sq);
    rc = vg_ensure_misc(c, need * sizeof(double));
    if (rc) return rc;
    double* base = (double*)c->misc;
    double *U1 = base + oU1, *U2 = base + oU2, *Tm = base + oTm, *P1 = base + oP1, *P2 = base + oP2, *S = base + oS, *Sq = base + oSq;
    long long* dcells = cells ? reinterpret_cast<long long*>(base + oCells) : nullptr;
    if (cells && n_cells > 0) VG_HIP(hipMemcpyAsync(dcells, cells, sizeof(long long) * n_cells, hipMemcpyHostToDevice, st));
    if ((rc = vg_whitened_cross(c, C1, mv1, C2, mv2, U1, U2, st))) return rc;
    if (mean) {          // rho U1^T A0 U2
        if ((rc = gemm1(U1, 1, mv1, w.a0, m2, 1, Tm, (int)m2, (int)mv1, (int)m2, (int)m1, st))) return rc;
        if ((rc = gemm1(Tm, m2, 1, U2, mv2, 1, mean, (int)mv2, (int)mv1, (int)mv2, (int)m2, st))) return rc;
        VGM_LAUNCH1D(vgs_scale_mean_kernel, ncell_all, st, mean, ncell_all, c->theta);
        VG_HIP(hipGetLastError());
    }
    if (n_cells == 0) { VG_HIP(hipStreamSynchronize(st)); return VGGP_OK; }
    if (literal) {
        if (scattered) {
            for (long off = 0; off < n1; off += chunk) {
                const long cn = std::min<long>(chunk, n1 - off);
                VgGemmBatch g;
                vg_gemm_init(&g);          // P_d[:, chunk] = U_d^T B_d[:, chunk]
                vg_gemm_add(&g, U1, 1, mv1, B1 + off, n1, 1, P1, (int)cn, (int)mv1, (int)cn, (int)m1);
                vg_gemm_add(&g, U2, 1, mv2, B2 + off, n1, 1, P2, (int)cn, (int)mv2, (int)cn, (int)m2);
                VG_HIP(vg_gemm_launch(&g, st));
                VG_HIP(vg_kr_sqgram_launch(P1, P2, (int)mv1, (int)mv2, cn, S, Sq, off > 0 ? 1 : 0, st));
            }
        } else {
            VgGemmBatch g;
            vg_gemm_init(&g);
            vg_gemm_add(&g, U1, 1, mv1, B1, n1, 1, P1, (int)n1, (int)mv1, (int)n1, (int)m1);
            vg_gemm_add(&g, U2, 1, mv2, B2, n2, 1, P2, (int)n2, (int)mv2, (int)n2, (int)m2);
            VG_HIP(vg_gemm_launch(&g, st));
            VGM_LAUNCH1D(vgi_mul_kernel, mv1 * n1, st, P1, P1, mv1 * n1, P1);
            VGM_LAUNCH1D(vgi_mul_kernel, mv2 * n2, st, P2, P2, mv2 * n2, P2);
            // Tm[a][j] = sum_i P1^2[a][i] W[j][i];   S[a][b] = sum_j Tm[a][j] P2^2[b][j]
            if ((rc = gemm1(P1, n1, 1, W, 1, n1, Tm, (int)n2, (int)mv1, (int)n2, (int)n1, st))) return rc;
            if ((rc = gemm1(Tm, n2, 1, P2, 1, n2, S, (int)mv2, (int)mv1, (int)mv2, (int)n2, st))) return rc;
        }
        VGM_LAUNCH1D(vgi_readout_literal_kernel, n_cells, st, S, kd1, kd2, c->theta, dcells, (long)mv2, (long)n_cells, var);
        VG_HIP(hipGetLastError());
        VG_HIP(hipStreamSynchronize(st));
        return VGGP_OK;
    }
    const int nbc = (int)std::min<int64_t>(block, n_cells);
    VgReadout r;
    if ((rc = vgi_readout_prepare(c, w, r, nbc, false, W, n_obs, st))) return rc;
    const long nb = M * nbc;
    int max_its = 0, solves = 0;
    for (int64_t off = 0; off < n_cells; off += nbc) {
        const int cn = (int)std::min<int64_t>(nbc, n_cells - off);
        const VgCellRule rule{dcells ? dcells + off : nullptr, (long)off, (long)mv2};
        VGM_LAUNCH1D(vgi_rank1_kernel, nb, st, VgRank1Factor{U1, (long)mv1, 1}, VgRank1Factor{U2, (long)mv2, 1}, rule, (int)m1, nbc, (int)m2, cn, r.T);
        if ((rc = vgi_solve_block(c, w, r, fn, tol, max_iter, &solves, &max_its, info, st))) return rc;
        hipLaunchKernelGGL(vgi_readout_reduce_kernel<VgiGridEpilogue>, dim3(cn), dim3(256), 0, st, r.T, r.it.X, w.a0, (int)m1, nbc, (int)m2, c->theta,
                           VgiGridEpilogue{kd1, kd2, rule, var + off});
    }
    VG_HIP(hipGetLastError());
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

extern "C" int vggp_readout_masked_iter(vggp_ctx* c, const double* W, double n_obs, const double* C1, int64_t mv1, const double* C2, int64_t mv2,
                                        const double* kd1, const double* kd2, const int64_t* cells, int64_t n_cells, double tol, int max_iter,
                                        int block, double* mean, double* var, int flags, vggp_info* info, void* stream) {
    return vgi_gridded_run(c, "vggp_readout_masked_iter", false, W, n_obs, C1, mv1, C2, mv2, kd1, kd2, cells, n_cells, tol, max_iter, block, mean,
                           var, flags, info, stream);
}
extern "C" int vggp_readout_scattered_iter(vggp_ctx* c, const double* C1, int64_t mv1, const double* C2, int64_t mv2, const double* kd1,
                                           const double* kd2, const int64_t* cells, int64_t n_cells, double tol, int max_iter, int block,
                                           double* mean, double* var, int flags, vggp_info* info, void* stream) {
    return vgi_gridded_run(c, "vggp_readout_scattered_iter", true, nullptr, 0.0, C1, mv1, C2, mv2, kd1, kd2, cells, n_cells, tol, max_iter, block,
                           mean, var, flags, info, stream);
}
