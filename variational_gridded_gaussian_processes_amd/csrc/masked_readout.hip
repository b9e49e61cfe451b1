// Read-outs of the dense masked / scattered steps (masked.hip) from the M-space state they leave -- Sigma~^-1, its factor and a0:
// q(v) with its diagonal or dense covariance, posterior(x*) with its variances or dense covariance, and the gridded read-out of B0 cell
// features.  The whitened columns every read-out of the library starts from (vg_whitened_columns, vg_whitened_cross) live here too.
#include "mspace_ws.h"

// q(v) diagonal: var[a] = s1 s2 sum_{b,c} Lk[a][b] Sinv[b][c] Lk[a][c] with Lk = L1 (x) L2, computed as rowdot(Lk Sinv, Lk)
__global__ void vgm_kron_kernel(const double* L1, const double* L2, int m1, int m2, double* Lk) {
    const long M = (long)m1 * m2;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * M) return;
    const long row = idx / M, col = idx - row * M;
    Lk[idx] = L1[(row / m2) * m1 + col / m2] * L2[(row % m2) * m2 + col % m2];
}
// e_d = +1: Kuu_d = s_d K0;  e_d = -1: Kuu_d = K0 / s_d (inter-domain VFF / B1 features): q(v) = L (...) with L = s^(e/2) L0
__global__ void vgm_rowdot_scale_kernel(const double* A, const double* B, long M, const double* theta, double* out, int e1, int e2) {
    const long a = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= M) return;
    double s = 0.0;
    for (long b = 0; b < M; ++b) s += A[a * M + b] * B[a * M + b];
    out[a] = (e1 > 0 ? theta[2] : 1.0 / theta[2]) * (e2 > 0 ? theta[3] : 1.0 / theta[3]) * s;
}
// x *= s1^((1 + e1) / 2) s2^((1 + e2) / 2) / sigma^2: the scale of a q(v) mean
__global__ void vgm_scale_rho_kernel(double* x, long n, const double* theta, int e1, int e2) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= (e1 > 0 ? theta[2] : 1.0) * (e2 > 0 ? theta[3] : 1.0) / theta[4];      // s_d^((1 + e_d) / 2) / sigma^2
}

// q(v) mean of every cell from the a0 an iterative step left: L0_1 A0 L0_2^T, scaled as vggp_qv_masked scales it (two GEMMs, no solve)
int vgi_qv_mean(vggp_ctx* c, VgMasked& w, double* mean, hipStream_t st) {
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const int m1 = w.m1, m2 = w.m2;
    int rc;
    if ((rc = gemm1(d1.L0, m1, 1, w.a0, m2, 1, w.MkA1, m2, m1, m2, m1, st))) return rc;
    if ((rc = gemm1(w.MkA1, m2, 1, d2.L0, 1, m2, mean, m2, m1, m2, m2, st))) return rc;
    VGM_LAUNCH1D(vgm_scale_rho_kernel, w.M, st, mean, w.M, c->theta, vg_uexp(d1.basis), vg_uexp(d2.basis));
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}
// posterior(x*): factor columns A_d = a_d(x*_d) and U_d = L0_d^-1 A_d ([m_d][cn]) of cn points
int vg_whitened_columns(vggp_ctx* c, const double* xs1, const double* xs2, int cn, double* A1, double* A2, double* U1, double* U2,
                        hipStream_t st) {
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    VgFactorJob fj[2] = {VgFactorJob{xs1, d1.grid, A1, nullptr, nullptr, nullptr, cn, d1.m, d1.kind, d1.basis, 0, 0.0, c->desc.flags},
                         VgFactorJob{xs2, d2.grid, A2, nullptr, nullptr, nullptr, cn, d2.m, d2.kind, d2.basis, 1, 0.0, c->desc.flags}};
    VG_HIP(vg_factor_build_launch(fj, 2, c->theta, st));
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, d1.Linv0, d1.m, 1, A1, cn, 1, U1, cn, d1.m, cn, d1.m);
    vg_gemm_add(&g, d2.Linv0, d2.m, 1, A2, cn, 1, U2, cn, d2.m, cn, d2.m);
    VG_HIP(vg_gemm_launch(&g, st));
    return VGGP_OK;
}
// gridded read-outs: U_d = Linv0_d C_d^T (m_d x mv_d) from the cross-covariances C_d [mv_d][m_d]
int vg_whitened_cross(vggp_ctx* c, const double* C1, long mv1, const double* C2, long mv2, double* U1, double* U2, hipStream_t st) {
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, d1.Linv0, d1.m, 1, C1, 1, d1.m, U1, (int)mv1, d1.m, (int)mv1, d1.m);
    vg_gemm_add(&g, d2.Linv0, d2.m, 1, C2, 1, d2.m, U2, (int)mv2, d2.m, (int)mv2, d2.m);
    VG_HIP(vg_gemm_launch(&g, st));
    return VGGP_OK;
}

// q(v) of the last masked step: mean = (s1 s2 / v) L1 A0 L2^T, diag cov = s1 s2 rowdot((L1 (x) L2) Sinv, L1 (x) L2)
extern "C" int vggp_qv_masked(vggp_ctx* c, double* mean, double* var, void* stream) {
    VG_FORWARD_PAIRED(c, vg_paired_qv(c, mean, var, stream ? (hipStream_t)stream : c->own_stream));
    if (!c || !c->have_masked || !c->masked) { vg_set_error("vggp_qv_masked: no finished masked step"); return VGGP_ESTATE; }
    VG_REQUIRE(mean && var, "vggp_qv_masked: null output");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    const long m1 = w.m1, m2 = w.m2, M = w.M;
    int rc;
    if ((rc = vgi_qv_mean(c, w, mean, st))) return rc;
    VGM_LAUNCH1D(vgm_kron_kernel, M * M, st, c->d[0].L0, c->d[1].L0, (int)m1, (int)m2, w.R);
    if ((rc = gemm1(w.R, M, 1, w.Sinv, M, 1, w.Sg, (int)M, (int)M, (int)M, (int)M, st))) return rc;
    VGM_LAUNCH1D(vgm_rowdot_scale_kernel, M, st, w.Sg, w.R, M, c->theta, var, vg_uexp(c->d[0].basis), vg_uexp(c->d[1].basis));
    VG_HIP(hipGetLastError());
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

// mean[p] = rho * sum_u T[u][p] a0[u] ;  var[p] = s1 s2 (1 - sum_u T[u][p]^2 + sum_u T[u][p] ST[u][p])
__global__ void vgm_post_kernel(const double* T, const double* ST, const double* a0, long M, long cn, const double* theta,
                                double* mean, double* var) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= cn) return;
    double lin = 0.0, nrm = 0.0, quad = 0.0;
    for (long u = 0; u < M; ++u) {
        const double t = T[u * cn + p];
        lin += t * a0[u];
        nrm += t * t;
        quad += t * ST[u * cn + p];
    }
    const double ss = theta[2] * theta[3];
    mean[p] = (ss / theta[4]) * lin;
    var[p] = ss * (1.0 - nrm + quad);
}

// gridded read-out: cell p = a * mv2 + b; column p of T1x / T2x is column a of U1 / column b of U2
__global__ void vgm_expand_kernel(const double* U1, const double* U2, int m1, int m2, long mv1, long mv2, long p0, long cn,
                                  double* T1x, double* T2x) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)(m1 + m2) * cn) return;
    const long row = idx / cn, q = idx - row * cn, p = p0 + q;
    const long a = p / mv2, b = p - a * mv2;
    if (row < m1) T1x[row * cn + q] = U1[row * mv1 + a];
    else T2x[(row - m1) * cn + q] = U2[(row - m1) * mv2 + b];
}
// mean = (s1 s2 / v) t^T a0;  var = s1 s2 (kd1_a kd2_b - |t|^2 + quad), quad = t^T Sinv t (conditional) or |Lc^T t|^2 (literal:
// t^T Sigma~ t, i.e. X = S_u^-1 in the reference's expression)
__global__ void vgm_readout_kernel(const double* T, const double* ST, const double* a0, long M, long cn, const double* theta,
                                   const double* kd1, const double* kd2, long mv2, long p0, int literal, double* mean, double* var) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= cn) return;
    double lin = 0.0, nrm = 0.0, quad = 0.0;
    for (long u = 0; u < M; ++u) {
        const double t = T[u * cn + q], s = ST[u * cn + q];
        lin += t * a0[u];
        nrm += t * t;
        quad += literal ? s * s : t * s;
    }
    const long p = p0 + q, a = p / mv2, b = p - a * mv2;
    const double ss = theta[2] * theta[3];
    mean[p] = (ss / theta[4]) * lin;
    var[p] = ss * (kd1[a] * kd2[b] - nrm + quad);
}

// Gridded read-out q(v) of B0 cell features from the M-space state of the last masked / scattered step (the Gridded* models of
// gridded_kronecker_structure.py:396-438 / :613-654 / :903-947 on data that is no full grid -- the along-track case of notebook
// 61): arguments and meaning as vggp_readout.  t = (L0_1^-1 C1^T)[:, a] (x) (L0_2^-1 C2^T)[:, b]: the point-wise posterior's algebra
// with the cross-covariances in place of the kernel columns and kd1_a kd2_b in place of the unit prior variance.
extern "C" int vggp_readout_masked(vggp_ctx* c, const double* C1, int64_t mv1, const double* C2, int64_t mv2, const double* kd1,
                                   const double* kd2, double* mean, double* var, int flags, void* stream) {
    VG_FORWARD_PAIRED(c, vg_paired_readout(c, C1, mv1, C2, mv2, kd1, kd2, mean, var, flags, stream ? (hipStream_t)stream : c->own_stream));
    if (!c || !c->have_masked || !c->masked) { vg_set_error("vggp_readout_masked: no finished masked / scattered step"); return VGGP_ESTATE; }
    VG_REQUIRE(C1 && C2 && kd1 && kd2 && mean && var && mv1 > 0 && mv2 > 0, "vggp_readout_masked: bad argument");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    const long m1 = w.m1, m2 = w.m2, M = w.M, ns = mv1 * mv2;
    const int literal = (flags & VGGP_READOUT_LITERAL) ? 1 : 0;
    const long chunk = std::min<long>(ns, M);            // T and (Sinv | Lc^T) T live in the two M x M scratch matrices
    int rc = vg_ensure_misc(c, (size_t)(m1 * mv1 + m2 * mv2 + chunk * (m1 + m2)) * sizeof(double));
    if (rc) return rc;
    double* p = (double*)c->misc;
    double* U1 = p; p += m1 * mv1;
    double* U2 = p; p += m2 * mv2;
    double* T1x = p; p += m1 * chunk;
    double* T2x = p;
    if ((rc = vg_whitened_cross(c, C1, mv1, C2, mv2, U1, U2, st))) return rc;
    for (long off = 0; off < ns; off += chunk) {
        const long cn = std::min<long>(chunk, ns - off);
        VGM_LAUNCH1D(vgm_expand_kernel, (m1 + m2) * cn, st, U1, U2, (int)m1, (int)m2, (long)mv1, (long)mv2, off, cn, T1x, T2x);
        VGM_LAUNCH1D(vgm_pairprod_kernel, M * cn, st, T1x, T2x, (int)m1, (int)m2, cn, w.R);
        if (literal) { if ((rc = gemm1(w.Lg, 1, M, w.R, cn, 1, w.Sg, (int)cn, (int)M, (int)cn, (int)M, st))) return rc; }     // Lc^T T
        else if ((rc = gemm1(w.Sinv, M, 1, w.R, cn, 1, w.Sg, (int)cn, (int)M, (int)cn, (int)M, st))) return rc;
        VGM_LAUNCH1D(vgm_readout_kernel, cn, st, w.R, w.Sg, w.a0, M, cn, c->theta, kd1, kd2, (long)mv2, off, literal, mean, var);
    }
    VG_HIP(hipGetLastError());
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

// posterior(x*) of the last masked step (kronecker_structure.py:199-230 on the observed subset):
//   t = (L1^{-1} a1(x*)) (x) (L2^{-1} a2(x*)),  mean = rho t^T a0,  var = s1 s2 (1 - |t|^2 + t^T Sigma~^{-1} t)
extern "C" int vggp_posterior_masked(vggp_ctx* c, const double* xs1, const double* xs2, int64_t ns, double* mean, double* var,
                                     void* stream) {
    VG_FORWARD_PAIRED(c, vg_paired_posterior(c, xs1, xs2, ns, mean, var, stream ? (hipStream_t)stream : c->own_stream));
    if (!c || !c->have_masked || !c->masked) { vg_set_error("vggp_posterior_masked: no finished masked step"); return VGGP_ESTATE; }
    VG_REQUIRE(xs1 && xs2 && mean && var && ns >= 0, "vggp_posterior_masked: bad argument");
    if (ns == 0) return VGGP_OK;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    const long m1 = w.m1, m2 = w.m2, M = w.M;
    const long chunk = std::min<long>(ns, M);            // T and Sigma~^{-1} T live in the two M x M scratch matrices
    int rc = vg_ensure_misc(c, (size_t)chunk * 2 * (m1 + m2) * sizeof(double));
    if (rc) return rc;
    double* p = (double*)c->misc;
    double* A1 = p; p += m1 * chunk;
    double* B1 = p; p += m1 * chunk;
    double* A2 = p; p += m2 * chunk;
    double* B2 = p;
    for (long off = 0; off < ns; off += chunk) {
        const int cn = (int)std::min<long>(chunk, ns - off);
        if ((rc = vg_whitened_columns(c, xs1 + off, xs2 + off, cn, A1, A2, B1, B2, st))) return rc;
        VGM_LAUNCH1D(vgm_pairprod_kernel, M * cn, st, B1, B2, (int)m1, (int)m2, (long)cn, w.R);
        if ((rc = gemm1(w.Sinv, M, 1, w.R, cn, 1, w.Sg, cn, (int)M, cn, (int)M, st))) return rc;
        VGM_LAUNCH1D(vgm_post_kernel, cn, st, w.R, w.Sg, w.a0, M, (long)cn, c->theta, mean + off, var + off);
    }
    VG_HIP(hipGetLastError());
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

hipError_t vg_prior_cov_launch(const double* xs1, const double* xs2, long ns, int kind1, int kind2, const double* theta,
                               double* cov, hipStream_t st);

// dense covariance of posterior(x*) of the last masked step: cov = K** + s1 s2 (T^T Sigma~^{-1} T - T^T T), T = (L1^{-1} a1*) (x) (L2^{-1} a2*)
extern "C" int vggp_posterior_cov_masked(vggp_ctx* c, const double* xs1, const double* xs2, int64_t ns, double* cov, void* stream) {
    VG_FORWARD_PAIRED(c, vg_paired_posterior_cov(c, xs1, xs2, ns, cov, stream ? (hipStream_t)stream : c->own_stream));
    if (!c || !c->have_masked || !c->masked) { vg_set_error("vggp_posterior_cov_masked: no finished masked step"); return VGGP_ESTATE; }
    VG_REQUIRE(xs1 && xs2 && cov && ns >= 1, "vggp_posterior_cov_masked: bad argument");
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    const long m1 = w.m1, m2 = w.m2, M = w.M;
    VG_REQUIRE(ns <= M, "vggp_posterior_cov_masked: at most M = %ld points per call (the scratch is M x M)", M);
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    int rc = vg_ensure_misc(c, (size_t)ns * 2 * (m1 + m2) * sizeof(double));
    if (rc) return rc;
    double* p = (double*)c->misc;
    double* A1 = p; p += m1 * ns;
    double* B1 = p; p += m1 * ns;
    double* A2 = p; p += m2 * ns;
    double* B2 = p;
    const int cn = (int)ns;
    if ((rc = vg_whitened_columns(c, xs1, xs2, cn, A1, A2, B1, B2, st))) return rc;
    VGM_LAUNCH1D(vgm_pairprod_kernel, M * cn, st, B1, B2, (int)m1, (int)m2, (long)cn, w.R);                 // T  (M x ns)
    if ((rc = gemm1(w.Sinv, M, 1, w.R, cn, 1, w.Sg, cn, (int)M, cn, (int)M, st))) return rc;                  // Sigma~^{-1} T
    const double ss = c->h_theta[2] * c->h_theta[3];
    if ((rc = gemm1(w.R, 1, cn, w.Sg, cn, 1, cov, cn, cn, cn, (int)M, st, ss, 0))) return rc;                  // + s1 s2 T^T Sigma~^{-1} T
    if ((rc = gemm1(w.R, 1, cn, w.R, cn, 1, cov, cn, cn, cn, (int)M, st, -ss, 1))) return rc;                  // - s1 s2 T^T T
    VG_HIP(vg_prior_cov_launch(xs1, xs2, ns, c->d[0].kind, c->d[1].kind, c->theta, cov, st));
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

// dense M x M covariance of q(v) of the last masked step: S = s1^e1 s2^e2 (L1 (x) L2) Sigma~^{-1} (L1 (x) L2)^T
// x *= s1^e1 s2^e2: the scale of a q(v) covariance
__global__ void vgm_scale_e_kernel(double* x, long n, const double* theta, int e1, int e2) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= (e1 > 0 ? theta[2] : 1.0 / theta[2]) * (e2 > 0 ? theta[3] : 1.0 / theta[3]);
}
extern "C" int vggp_qv_cov_masked(vggp_ctx* c, double* cov, void* stream) {
    VG_FORWARD_PAIRED(c, vg_paired_qv_cov(c, cov, stream ? (hipStream_t)stream : c->own_stream));
    if (!c || !c->have_masked || !c->masked) { vg_set_error("vggp_qv_cov_masked: no finished masked step"); return VGGP_ESTATE; }
    VG_REQUIRE(cov, "vggp_qv_cov_masked: null output");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    const long m1 = w.m1, m2 = w.m2, M = w.M;
    int rc;
    VGM_LAUNCH1D(vgm_kron_kernel, M * M, st, c->d[0].L0, c->d[1].L0, (int)m1, (int)m2, w.R);
    if ((rc = gemm1(w.R, M, 1, w.Sinv, M, 1, w.Sg, (int)M, (int)M, (int)M, (int)M, st))) return rc;
    if ((rc = gemm1(w.Sg, M, 1, w.R, 1, M, cov, (int)M, (int)M, (int)M, (int)M, st))) return rc;
    VGM_LAUNCH1D(vgm_scale_e_kernel, M * M, st, cov, M * M, c->theta, vg_uexp(c->d[0].basis), vg_uexp(c->d[1].basis));
    VG_HIP(hipGetLastError());
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}
