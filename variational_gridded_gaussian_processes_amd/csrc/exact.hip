// Exact GP on N scattered points (the reference's Matern12GP / Matern32GP / Matern52GP, src/models/exact/bivariate_structure.py, and
// GriddedMatern12ExactGP, src/models/sparse/gridded_kronecker_structure.py:21-211): the dense N x N baseline the sparse models are
// measured against.  kernel = kernel_1 * kernel_2 on active dims 0 and 1, theta = (ell1, ell2, s1, s2, v), s = s1 s2:
//     K0[i, j] = k1(|x_i1 - x_j1| / ell1) k2(|x_i2 - x_j2| / ell2),  Sigma = s K0 + (v + eps) I  (eps: psd_safe_cholesky on Sigma itself),
//     alpha = Sigma^-1 y,  MLL = -1/2 [y^T alpha + log|Sigma| + N log 2 pi],
//     W = alpha alpha^T - Sigma^-1:  dMLL/dell_d = (s / 2) <W, dK0/dell_d>,  dMLL/ds1 = <W, K0> s2 / 2,  dMLL/dv = tr W / 2.
// One step = Sigma from the coordinates, the blocked MFMA Cholesky + inverse (masked.hip), alpha = X^T (X y), and ONE pass over the upper
// tiles of Sigma^-1 that evaluates k_d and dk_d/dell_d on chip and accumulates the three contractions and tr W (neither dK nor W is
// stored); per-workgroup partials are summed in a fixed order (no float atomics): every result is bitwise repeatable.
// Read-outs: posterior(x*) mean s B*^T alpha, variance s - s^2 diag(B*^T Sigma^-1 B*) through the generated-operand GEMM (gen_gemm.h);
// q(v) of B0 cells with F = s (C1 face-split C2): mean F alpha, variance s kd1 kd2 - diag(F Sigma^-1 F^T) (conditional) or
// s kd1 kd2 + (F o F) 1 / v (the reference's :177-191, since P^-1 = Kxx^-1 + I / v for P = Kxx - Kxx Sigma^-1 Kxx).
// The workspace hangs off the context (c->exact) and shares nothing with a vggp_plan: either may be replaced without the other noticing.
// Specification: tests/exact_gp_spec.py.
#include "arena.h"
#include "gen_gemm.h"

#include <algorithm>
#include <cmath>

#define EX_MAX_N 16384        // four N x N matrices: 8 GiB at the cap
#define EX_GT 64              // tile of the gradient pass (256 threads: 64 columns x 4 rows, 16 rows each)

// Sigma = s K0 + d I, both triangles (the blocked Cholesky reads the lower one and the diagonal blocks)
__global__ void ex_sigma_kernel(const double* x1, const double* x2, int N, int kind1, int kind2, double inv1, double inv2, double s,
                                double d, double* S) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)N * N) return;
    const int i = (int)(idx / N), j = (int)(idx - (long)i * N);
    double v1, d1, v2, d2;
    vg_kappa(kind1, fabs(x1[i] - x1[j]), inv1, v1, d1);
    vg_kappa(kind2, fabs(x2[i] - x2[j]), inv2, v2, d2);
    S[idx] = s * v1 * v2 + (i == j ? d : 0.0);
}

// One upper tile (tn >= tm) of W = alpha alpha^T - Sinv against K0, dK0/dell1, dK0/dell2 (generated from the coordinates), weight 2 off
// the diagonal tiles; tr W from the diagonal tiles.  part[tile][4] = {<W, K0>, <W, dK0/dell1>, <W, dK0/dell2>, tr W}.
__global__ __launch_bounds__(256) void ex_grad_kernel(const double* Sinv, const double* alpha, const double* x1, const double* x2, int N,
                                                      int kind1, int kind2, double inv1, double inv2, int tiles, double* part) {
    __shared__ double sh[256];
    __shared__ double r1[EX_GT], r2[EX_GT], ra[EX_GT];
    int tm = 0, rem = blockIdx.x;
    while (rem >= tiles - tm) { rem -= tiles - tm; ++tm; }
    const int tn = tm + rem;
    const int row0 = tm * EX_GT, col0 = tn * EX_GT;
    const int tid = threadIdx.x, cj = tid & 63, rq = tid >> 6;
    if (tid < EX_GT) {
        const int i = row0 + tid;
        const bool in = i < N;
        r1[tid] = in ? x1[i] : 0.0; r2[tid] = in ? x2[i] : 0.0; ra[tid] = in ? alpha[i] : 0.0;
    }
    __syncthreads();
    const int j = col0 + cj;
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    if (j < N) {
        const double xj1 = x1[j], xj2 = x2[j], aj = alpha[j];
#pragma unroll 4
        for (int k = 0; k < EX_GT / 4; ++k) {
            const int li = rq + 4 * k, i = row0 + li;
            if (i >= N) break;
            const double w = ra[li] * aj - Sinv[(long)i * N + j];
            double v1, l1, v2, l2;
            vg_kappa(kind1, fabs(r1[li] - xj1), inv1, v1, l1);
            vg_kappa(kind2, fabs(r2[li] - xj2), inv2, v2, l2);
            q[0] += w * (v1 * v2); q[1] += w * (l1 * v2); q[2] += w * (v1 * l2);
            if (i == j) q[3] += w;
        }
    }
    const double wt = tm == tn ? 1.0 : 2.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double t = pz_block_sum(q[k], sh);
        if (tid == 0) part[(long)blockIdx.x * 4 + k] = (k < 3 ? wt : 1.0) * t;
    }
}

// fixed-order sums of the tile partials, log L_ii and |X y|^2, then the value and the five gradient components
struct ExFinal {
    const double *part, *L, *wv;
    int ntile, N;
    double s1, s2;
    double* out;
};
__global__ __launch_bounds__(256) void ex_final_kernel(const ExFinal a) {
    __shared__ double sh[256];
    double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < a.ntile; t += 256) {
        const double* p = a.part + (long)t * 4;
        q[0] += p[0]; q[1] += p[1]; q[2] += p[2]; q[3] += p[3];
    }
    for (int i = threadIdx.x; i < a.N; i += 256) { q[4] += log(a.L[(long)i * a.N + i]); q[5] += a.wv[i] * a.wv[i]; }
    double t[6];
    for (int k = 0; k < 6; ++k) t[k] = pz_block_sum(q[k], sh);
    if (threadIdx.x != 0) return;
    const double s = a.s1 * a.s2;
    a.out[0] = -0.5 * (t[5] + 2.0 * t[4] + (double)a.N * log(2.0 * M_PI));
    a.out[1] = 0.5 * s * t[1]; a.out[2] = 0.5 * s * t[2];
    a.out[3] = 0.5 * t[0] * a.s2; a.out[4] = 0.5 * t[0] * a.s1; a.out[5] = 0.5 * t[3];
}

// var[p] = prior + w vsum[p], prior = s (point) or s kd1[a] kd2[b] (cell p = a mv2 + b)
__global__ void ex_var_kernel(const double* vsum, const double* kd1, const double* kd2, int mv2, long n, double s, double w, double* var) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const double prior = kd1 ? s * kd1[p / mv2] * kd2[p % mv2] : s;
    var[p] = prior + w * vsum[p];
}
// posterior_cov: B*[i][p] explicitly (the output is dense anyway), then cov = w cov + s k1 k2
__global__ void ex_bstar_kernel(const PzPts g, int N, long ns, double* Bs) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)N * ns) return;
    const int i = (int)(idx / ns);
    Bs[idx] = g.val(i, (int)(idx - (long)i * ns));
}
__global__ void ex_prior_kernel(const double* xs1, const double* xs2, long ns, int kind1, int kind2, double inv1, double inv2, double s,
                                double w, double* cov) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ns * ns) return;
    const long p = idx / ns, q = idx - p * ns;
    double k1, k2, d;
    vg_kappa(kind1, fabs(xs1[p] - xs1[q]), inv1, k1, d);
    vg_kappa(kind2, fabs(xs2[p] - xs2[q]), inv2, k2, d);
    cov[idx] = w * cov[idx] + s * k1 * k2;
}

// ---- workspace -------------------------------------------------------------------------------------------------------------
struct ExHost { double out[8]; int status[2]; };
struct VgExact {
    long N = 0;
    int kind1 = 0, kind2 = 0, nblk = 0, tiles = 0, ntile = 0;
    double *x1, *x2;
    double *S, *L, *X, *Sinv;                                // N x N
    double *DI, *Tmp, *cholscratch, *jit;
    int* status;
    double *wv, *alpha, *part, *out;
    void* mem = nullptr;
    ExHost* host = nullptr;                                  // pinned read-back block of its own (c->h_out belongs to the planned model)
    // state of the last step
    bool have_step = false;
    double theta[5] = {0, 0, 0, 0, 0}, eps = 0.0;
};

static void ex_layout(VgExact& w, VgArena& a) {
    const size_t N = w.N, NN = N * N;
    w.x1 = a.take(N); w.x2 = a.take(N);
    w.S = a.take(NN); w.L = a.take(NN); w.X = a.take(NN); w.Sinv = a.take(NN);
    w.DI = a.take((size_t)w.nblk * PZ_MB * PZ_MB); w.Tmp = a.take((size_t)PZ_MB * N);
    w.cholscratch = a.take(PZ_MB * (PZ_MB + 1)); w.jit = a.take(8);
    w.status = reinterpret_cast<int*>(a.take(8));
    w.wv = a.take(N); w.alpha = a.take(N); w.part = a.take((size_t)w.ntile * 4); w.out = a.take(8);
}

void vg_exact_free(vggp_ctx* c) {
    VgExact* w = reinterpret_cast<VgExact*>(c->exact);
    if (!w) return;
    if (w->mem) (void)hipFree(w->mem);
    if (w->host) (void)hipHostFree(w->host);
    delete w;
    c->exact = nullptr;
}

static VgExact* ex_ws(vggp_ctx* c) { return reinterpret_cast<VgExact*>(c->exact); }

static int ex_gemv(const double* A, long sa_m, long sa_k, const double* x, double* y, int M, int K, hipStream_t st) {
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, A, sa_m, sa_k, x, 1, 1, y, 1, M, 1, K);
    VG_HIP(vg_gemm_launch(&g, st));
    return VGGP_OK;
}

extern "C" int vggp_exact_plan(vggp_ctx* c, int kind1, int kind2, const double* x1, const double* x2, int64_t N) {
    if (!c) { vg_set_error("vggp_exact_plan: null context"); return VGGP_EINVAL; }
    VG_REQUIRE(c->n_ranks == 1 && !c->comm && !c->cb, "vggp_exact_plan: the exact GP is single-rank only");
    VG_REQUIRE(N >= 1 && N <= EX_MAX_N, "vggp_exact_plan: N = %lld outside [1, %d] (dense N x N solver)", (long long)N, EX_MAX_N);
    VG_REQUIRE(kind1 >= 0 && kind1 <= 3 && kind2 >= 0 && kind2 <= 3, "vggp_exact_plan: bad kind");
    VG_REQUIRE(x1 && x2, "vggp_exact_plan: null coordinate arrays");
    for (int64_t i = 0; i < N; ++i)
        VG_REQUIRE(std::isfinite(x1[i]) && std::isfinite(x2[i]), "vggp_exact_plan: point %lld is not finite", (long long)i);
    VG_ENTER_DEVICE(c->device);
    VgExact tmp;
    tmp.N = N; tmp.kind1 = kind1; tmp.kind2 = kind2;
    tmp.nblk = (int)((N + PZ_MB - 1) / PZ_MB);
    tmp.tiles = (int)((N + EX_GT - 1) / EX_GT);
    tmp.ntile = tmp.tiles * (tmp.tiles + 1) / 2;
    const size_t bytes = vg_arena_measure([&](VgArena& a) { ex_layout(tmp, a); });
    int rc;
    if ((rc = vg_quiesce(c))) return rc;
    if (c->exact) { VG_HIP(hipDeviceSynchronize()); vg_exact_free(c); }      // (the earlier exact plan: its read-outs may be in flight)
    size_t free_b = 0;
    if (!vg_arena_fits(bytes, &free_b)) {
        vg_set_error("vggp_exact_plan: the exact GP (N = %lld) needs %.1f GiB of workspace, %.1f GiB are free", (long long)N,
                     (double)bytes / 1073741824.0, (double)free_b / 1073741824.0);
        return VGGP_ENOMEM;
    }
    VgExact* w = new VgExact(tmp);
    c->exact = w;                        // owned by the context from here on (vg_exact_free releases it on any later failure)
    VG_HIP(hipHostMalloc((void**)&w->host, sizeof(ExHost), hipHostMallocDefault));
    if ((rc = vg_arena_alloc(&w->mem, bytes, [&](VgArena& a) { ex_layout(*w, a); }))) return rc;
    VG_HIP(hipMemcpy(w->x1, x1, sizeof(double) * N, hipMemcpyHostToDevice));
    VG_HIP(hipMemcpy(w->x2, x2, sizeof(double) * N, hipMemcpyHostToDevice));
    return VGGP_OK;
}

// one step at jitter w.eps; leaves out[6] and the status on the device
static int ex_step_enqueue(vggp_ctx* c, VgExact& w, const double* y, hipStream_t st) {
    const int N = (int)w.N;
    const double s1 = w.theta[2], s2 = w.theta[3], v = w.theta[4];
    const double inv1 = 1.0 / w.theta[0], inv2 = 1.0 / w.theta[1];
    int rc;
    // under vggp_profile: Sigma build -> stage 0, Cholesky + inverse -> stage 1, alpha -> stage 5, gradient pass + final sums -> stage 18
    auto mark = [&](int id) -> int {
        if (c->prof && c->nev < VG_MAXEV) { VG_HIP(hipEventRecord(c->ev[c->nev], st)); c->ev_stage[c->nev++] = id; }
        return VGGP_OK;
    };
    if ((rc = mark(-1))) return rc;
    VG_HIP(hipMemsetAsync(w.status, 0, 2 * sizeof(int), st));
    PZ_LAUNCH1D(ex_sigma_kernel, w.N * w.N, st, w.x1, w.x2, N, w.kind1, w.kind2, inv1, inv2, s1 * s2, v + w.eps, w.S);
    VG_HIP(hipGetLastError());
    if ((rc = mark(0))) return rc;
    VgDenseChol d{w.S, w.L, w.X, w.DI, w.Tmp, w.cholscratch, w.jit, w.status, w.N, w.Sinv};
    if ((rc = vg_blocked_chol_inverse(d, st))) return rc;
    if ((rc = mark(1))) return rc;
    // wv = X y (y^T alpha = |wv|^2 without the explicit inverse), alpha = X^T wv
    if ((rc = ex_gemv(w.X, N, 1, y, w.wv, N, N, st))) return rc;
    if ((rc = ex_gemv(w.X, 1, N, w.wv, w.alpha, N, N, st))) return rc;
    if ((rc = mark(5))) return rc;
    hipLaunchKernelGGL(ex_grad_kernel, dim3((unsigned)w.ntile), dim3(256), 0, st, w.Sinv, w.alpha, w.x1, w.x2, N, w.kind1, w.kind2, inv1,
                       inv2, w.tiles, w.part);
    ExFinal fa{w.part, w.L, w.wv, w.ntile, N, s1, s2, w.out};
    hipLaunchKernelGGL(ex_final_kernel, dim3(1), dim3(256), 0, st, fa);
    VG_HIP(hipGetLastError());
    return mark(18);
}

extern "C" int vggp_exact_step(vggp_ctx* c, const double* y, const double theta[5], double* mll_out, double grad_out[5], vggp_info* info,
                               void* stream) {
    if (!c) { vg_set_error("vggp_exact_step: null context"); return VGGP_EINVAL; }
    if (!c->exact) { vg_set_error("vggp_exact_step: no exact plan (vggp_exact_plan)"); return VGGP_ESTATE; }
    VG_REQUIRE(y && theta && mll_out && grad_out, "vggp_exact_step: null argument");
    VG_REQUIRE(c->n_ranks == 1 && !c->comm && !c->cb, "vggp_exact_step: the exact GP is single-rank only");
    VgExact& w = *ex_ws(c);
    w.have_step = false;
    for (int i = 0; i < 5; ++i) {
        VG_REQUIRE(theta[i] > 0.0 && std::isfinite(theta[i]), "theta[%d]=%g must be positive and finite", i, theta[i]);
        w.theta[i] = theta[i];
    }
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    int rc;
    if ((rc = vg_quiesce(c))) return rc;
    int failed = 0;
    rc = pz_jitter_retry(&w.eps, &failed, [&](bool) {
        c->nev = 0;
        int r = ex_step_enqueue(c, w, y, st);
        if (r) return r;
        VG_HIP(hipMemcpyAsync(w.host->out, w.out, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
        VG_HIP(hipMemcpyAsync(w.host->status, w.status, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        VG_HIP(hipStreamSynchronize(st));                           // the one host synchronisation of the step
        return w.host->status[0] ? 1 : 0;
    });
    if (c->prof && c->nev > 1 && rc == VGGP_OK) {
        for (int i = 1; i < c->nev; ++i) {
            const int id = c->ev_stage[i];
            float ms = 0.f;
            if (id >= 0 && id < VGGP_NSTAGE && hipEventElapsedTime(&ms, c->ev[i - 1], c->ev[i]) == hipSuccess) c->prof_ms[id] += ms;
        }
        c->prof_steps++;
    }
    c->nev = 0;
    if (rc < 0) return rc;
    if (info) {
        info->jitter1 = failed ? -1.0 : w.eps; info->jitter2 = 0.0;
        info->sweeps1 = info->sweeps2 = info->rounds1 = info->rounds2 = 0;
        info->status = failed ? w.host->status[0] : 0; info->polished = 0;
    }
    if (failed) { vg_set_error("vggp_exact_step: Sigma = K + sigma^2 I is not positive definite after jitter 1e-6"); return VGGP_ENOTPD; }
    *mll_out = w.host->out[0];
    for (int i = 0; i < 5; ++i) grad_out[i] = w.host->out[1 + i];
    w.have_step = true;
    return VGGP_OK;
}

// common entry of the read-outs: the workspace of a context whose current exact plan has a finished step
static int ex_readout_enter(vggp_ctx* c, const char* fn, VgExact** w) {
    if (!c) { vg_set_error("%s: null context", fn); return VGGP_EINVAL; }
    if (!c->exact || !ex_ws(c)->have_step) { vg_set_error("%s: no finished vggp_exact_step on the current exact plan", fn); return VGGP_ESTATE; }
    *w = ex_ws(c);
    return VGGP_OK;
}

// vsum[p] = sum_ij g(i, p) Sinv[i][j] g(j, p) for the ncol columns of a generated operand (scratch: c->misc)
template <class G>
static int ex_quadform(vggp_ctx* c, VgExact& w, const G& g, long ncol, double** vsum_out, hipStream_t st) {
    const int N = (int)w.N;
    const int tiles_m = (N + PZ_T - 1) / PZ_T;
    int rc;
    if ((rc = vg_ensure_misc(c, sizeof(double) * ((size_t)tiles_m * ncol + ncol + 64)))) return rc;
    double* part = reinterpret_cast<double*>(c->misc);
    double* vsum = part + (size_t)tiles_m * ncol;
    VG_HIP((pz_gen_gemm<PZ_EPI_COL1>(PzAMat{w.Sinv, w.N}, PzBRow<G>{g}, PzEpCol<G>{g, part, ncol}, N, (int)ncol, N, 1, false, st)));
    VgRedBatch r;
    vg_red_init(&r);
    vg_red_add(&r, part, vsum, ncol, ncol, tiles_m);
    VG_HIP(vg_red_launch(&r, st));
    *vsum_out = vsum;
    return VGGP_OK;
}

extern "C" int vggp_exact_posterior(vggp_ctx* c, const double* xs1, const double* xs2, int64_t ns, double* mean, double* var,
                                    void* stream) {
    VgExact* wp;
    int rc;
    if ((rc = ex_readout_enter(c, "vggp_exact_posterior", &wp))) return rc;
    VgExact& w = *wp;
    VG_REQUIRE(xs1 && xs2 && mean && var && ns >= 0 && ns < (1L << 30), "vggp_exact_posterior: bad argument");
    if (ns == 0) return VGGP_OK;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    if ((rc = vg_quiesce(c))) return rc;
    const double s = w.theta[2] * w.theta[3];
    const PzPts g{w.x1, w.x2, xs1, xs2, w.kind1, w.kind2, 1.0 / w.theta[0], 1.0 / w.theta[1]};
    hipLaunchKernelGGL(pz_mean_kernel<PzPts>, dim3((unsigned)ns), dim3(256), 0, st, g, w.alpha, (int)w.N, s, mean);
    VG_HIP(hipGetLastError());
    double* vsum;
    if ((rc = ex_quadform(c, w, g, (long)ns, &vsum, st))) return rc;
    PZ_LAUNCH1D(ex_var_kernel, ns, st, vsum, (const double*)nullptr, (const double*)nullptr, 1, (long)ns, s, -s * s, var);
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}

extern "C" int vggp_exact_posterior_cov(vggp_ctx* c, const double* xs1, const double* xs2, int64_t ns, double* cov, void* stream) {
    if (!c) { vg_set_error("vggp_exact_posterior_cov: null context"); return VGGP_EINVAL; }
    VG_REQUIRE(ns >= 1 && ns <= 8192, "vggp_exact_posterior_cov: ns = %lld outside [1, 8192]", (long long)ns);
    VgExact* wp;
    int rc;
    if ((rc = ex_readout_enter(c, "vggp_exact_posterior_cov", &wp))) return rc;
    VgExact& w = *wp;
    VG_REQUIRE(xs1 && xs2 && cov, "vggp_exact_posterior_cov: null argument");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    if ((rc = vg_quiesce(c))) return rc;
    const int N = (int)w.N;
    const double s = w.theta[2] * w.theta[3], inv1 = 1.0 / w.theta[0], inv2 = 1.0 / w.theta[1];
    if ((rc = vg_ensure_misc(c, sizeof(double) * (2 * (size_t)N * ns + 64)))) return rc;
    double* Bs = reinterpret_cast<double*>(c->misc);
    double* T = Bs + (size_t)N * ns;
    PZ_LAUNCH1D(ex_bstar_kernel, (long)N * ns, st, (PzPts{w.x1, w.x2, xs1, xs2, w.kind1, w.kind2, inv1, inv2}), N, (long)ns, Bs);
    VG_HIP(hipGetLastError());
    VgGemmBatch g;
    vg_gemm_init(&g);                                                                        // T = Sinv B*
    vg_gemm_add(&g, w.Sinv, N, 1, Bs, ns, 1, T, (int)ns, N, (int)ns, N);
    VG_HIP(vg_gemm_launch(&g, st));
    vg_gemm_init(&g);                                                                        // B*^T T
    vg_gemm_add(&g, Bs, 1, ns, T, ns, 1, cov, (int)ns, (int)ns, (int)ns, N);
    VG_HIP(vg_gemm_launch(&g, st));
    PZ_LAUNCH1D(ex_prior_kernel, (long)ns * ns, st, xs1, xs2, (long)ns, w.kind1, w.kind2, inv1, inv2, s, -s * s, cov);
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}

extern "C" int vggp_exact_readout(vggp_ctx* c, const double* C1, int64_t mv1, const double* C2, int64_t mv2, const double* kd1,
                                  const double* kd2, double* mean, double* var, int flags, void* stream) {
    VgExact* wp;
    int rc;
    if ((rc = ex_readout_enter(c, "vggp_exact_readout", &wp))) return rc;
    VgExact& w = *wp;
    VG_REQUIRE(C1 && C2 && kd1 && kd2 && mean && var && mv1 >= 1 && mv2 >= 1, "vggp_exact_readout: bad argument");
    VG_REQUIRE(w.kind1 == VGGP_KIND_MATERN12 && w.kind2 == VGGP_KIND_MATERN12,
               "vggp_exact_readout: the B0 cell features are Matern-1/2 integrals; the plan uses another kernel");
    VG_REQUIRE(mv1 < (1L << 20) && mv2 < (1L << 20) && mv1 * mv2 < (1L << 28), "vggp_exact_readout: too many cells");
    const long nv = mv1 * mv2;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    if ((rc = vg_quiesce(c))) return rc;
    const int N = (int)w.N;
    const double s = w.theta[2] * w.theta[3], v = w.theta[4];
    const PzFace f{C1, C2, (int)mv2, N};
    hipLaunchKernelGGL(pz_mean_kernel<PzFace>, dim3((unsigned)nv), dim3(256), 0, st, f, w.alpha, N, s, mean);
    VG_HIP(hipGetLastError());
    double* vsum;
    double wt;
    if (flags & VGGP_READOUT_LITERAL) {          // (F o F) 1: the squared Gram product over the points, no solve
        const size_t sc = vg_kr_sqgram_scratch((int)mv1, (int)mv2, w.N);
        if ((rc = vg_ensure_misc(c, sizeof(double) * (sc + (size_t)nv + 64)))) return rc;
        vsum = reinterpret_cast<double*>(c->misc) + sc;
        VG_HIP(vg_kr_sqgram_launch(C1, C2, (int)mv1, (int)mv2, w.N, vsum, reinterpret_cast<double*>(c->misc), 0, st));
        wt = s * s / v;
    } else {
        if ((rc = ex_quadform(c, w, f, nv, &vsum, st))) return rc;
        wt = -s * s;
    }
    PZ_LAUNCH1D(ex_var_kernel, nv, st, vsum, kd1, kd2, (int)mv2, nv, s, wt, var);
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}
