// Raster read-out: posterior(x*) on the cartesian grid of two coordinate axes (kronecker_structure.py:199-230 at the points of a
// meshgrid).  On a raster the whitened factors separate -- T_d = Q_d^T L0_d^-1 A_d(axis_d) is needed at the P_d axis coordinates only --
// and mean and variance are two-sided products,
//     mean = T1^T (Wm T2),      var = s1 s2 (1 + (T1 o T1)^T (Wv (T2 o T2))),
// O(P1 P2 q1) instead of the O(P1 P2 q1 q2) of the point-wise entries.  vg_raster_kernel does the last product of both in one launch.
#include "mspace_ws.h"

typedef double vr_d4 __attribute__((ext_vector_type(4)));

#define VR_T 64                   // output tile: 64 x 64, four waves 2 x 2, each 32 x 32 = 2 x 2 MFMA blocks
#define VR_BK 16                  // k-tile
#define VR_KS (VR_T + 16)         // LDS row of a k-slice: 80 doubles, so the four k-rows of a fragment read fall on disjoint banks
#define VR_MAXP (1L << 20)        // axis length limit of the entries

// mean[a][b] = sum_i T1[i][a] U[i][b];   var[a][b] = c0 + c1 sum_i T1[i][a]^2 Uv[i][b]      (theta: c0, c1 *= theta[2] theta[3])
// T1 [q][P1], U, Uv [q][P2], outputs [P1][P2].  All three operands are contiguous along the output index, so a k-slice is staged as
// LDS [k][64 + 16] and both MFMA operands read it as av = S[k = lane >> 4][i = lane & 15]: 16 consecutive doubles per k-row, rows 160
// dwords = 32 banks apart -- conflict-free within each 32-lane half.  The variance product's A fragment is the square of the mean
// product's, taken in registers.  Edges: rows / columns past P1 / P2 and k past q are loaded as zeros and never stored.
template <bool HV>
__global__ __launch_bounds__(256) void vg_raster_kernel(const double* __restrict__ T1, const double* __restrict__ U, const double* __restrict__ Uv,
                                                        int q, long P1, long P2, double c0, double c1, const double* __restrict__ theta,
                                                        double* __restrict__ mean, double* __restrict__ var, int tiles_n) {
    __shared__ double As[VR_BK * VR_KS], Bs[VR_BK * VR_KS], Vs[HV ? VR_BK * VR_KS : 1];
    const int tm = (int)(blockIdx.x / (unsigned)tiles_n), tn = (int)(blockIdx.x - (unsigned)tm * (unsigned)tiles_n);
    const long row0 = (long)tm * VR_T, col0 = (long)tn * VR_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, fi = lane & 15, fk = lane >> 4;
    // global -> register -> LDS: thread (j = tid & 63, kb = tid >> 6) moves elements (k = kb + 4 r, j), r = 0 .. 3, of each operand
    const int j = tid & 63, kb = tid >> 6;
    const bool aok = row0 + j < P1, bok = col0 + j < P2;
    const double* pa = T1 + (aok ? row0 + j : 0);
    const double* pb = U + (bok ? col0 + j : 0);
    const double* pv = HV ? Uv + (bok ? col0 + j : 0) : nullptr;
    double ra[4], rb[4], rv[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + kb + 4 * r;
            const bool kok = k < q;
            ra[r] = (aok && kok) ? pa[(long)k * P1] : 0.0;
            rb[r] = (bok && kok) ? pb[(long)k * P2] : 0.0;
            if (HV) rv[r] = (bok && kok) ? pv[(long)k * P2] : 0.0;
        }
    };
    vr_d4 am[2][2], av[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { am[a][b] = (vr_d4){0.0, 0.0, 0.0, 0.0}; av[a][b] = (vr_d4){0.0, 0.0, 0.0, 0.0}; }
    load(0);
    for (int k0 = 0; k0 < q; k0 += VR_BK) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            As[(kb + 4 * r) * VR_KS + j] = ra[r];
            Bs[(kb + 4 * r) * VR_KS + j] = rb[r];
            if (HV) Vs[(kb + 4 * r) * VR_KS + j] = rv[r];
        }
        __syncthreads();
        if (k0 + VR_BK < q) load(k0 + VR_BK);           // the next k-tile is in flight while this one is multiplied
#pragma unroll
        for (int kk = 0; kk < VR_BK; kk += 4) {
            double fa[2], fb[2], fv[2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) fa[mb] = As[(kk + fk) * VR_KS + wr * 32 + mb * 16 + fi];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                fb[nb] = Bs[(kk + fk) * VR_KS + wc * 32 + nb * 16 + fi];
                if (HV) fv[nb] = Vs[(kk + fk) * VR_KS + wc * 32 + nb * 16 + fi];
            }
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                const double fa2 = fa[mb] * fa[mb];
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    am[mb][nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[mb], fb[nb], am[mb][nb], 0, 0, 0);
                    if (HV) av[mb][nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa2, fv[nb], av[mb][nb], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    if (HV && theta) { const double s12 = theta[2] * theta[3]; c0 *= s12; c1 *= s12; }
    // C/D fragment of the fp64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = row0 + wr * 32 + mb * 16 + fk + 4 * r, col = col0 + wc * 32 + nb * 16 + fi;
                if (row < P1 && col < P2) {
                    mean[row * P2 + col] = am[mb][nb][r];
                    if (HV) var[row * P2 + col] = c0 + c1 * av[mb][nb][r];
                }
            }
}

static hipError_t vg_raster_launch(const double* T1, const double* U, const double* Uv, int q, long P1, long P2, double c0, double c1,
                                   const double* theta, double* mean, double* var, hipStream_t st) {
    const long tiles_m = (P1 + VR_T - 1) / VR_T, tiles_n = (P2 + VR_T - 1) / VR_T;
    if (q < 1 || P1 < 1 || P2 < 1 || P1 > VR_MAXP || P2 > VR_MAXP || (var && !Uv)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(tiles_m * tiles_n));           // (at most 2^14 x 2^14 tiles)
    if (var)
        hipLaunchKernelGGL(vg_raster_kernel<true>, grid, dim3(256), 0, st, T1, U, Uv, q, P1, P2, c0, c1, theta, mean, var, (int)tiles_n);
    else
        hipLaunchKernelGGL(vg_raster_kernel<false>, grid, dim3(256), 0, st, T1, U, Uv, q, P1, P2, c0, c1, theta, mean, var, (int)tiles_n);
    return hipGetLastError();
}

extern "C" int vggp_raster_contract(vggp_ctx* c, const double* T1, const double* U, const double* Uv, int64_t q, int64_t P1, int64_t P2,
                                    double c0, double c1, double* mean, double* var, void* stream) {
    static const char* fn = "vggp_raster_contract";
    if (!c) { vg_set_error("%s: null context", fn); return VGGP_EINVAL; }
    VG_REQUIRE(T1 && U && mean && (!var || Uv), "%s: null argument (var needs Uv)", fn);
    VG_REQUIRE(q >= 1 && q <= VR_MAXP && P1 >= 1 && P1 <= VR_MAXP && P2 >= 1 && P2 <= VR_MAXP, "%s: need 1 <= q, P1, P2 <= 2^20", fn);
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VG_HIP(vg_raster_launch(T1, U, Uv, (int)q, (long)P1, (long)P2, c0, c1, nullptr, mean, var, st));
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

// x *= s1 s2 / sigma^2: the scale of a posterior mean of the M-space states (whitened columns: no basis exponents)
__global__ void vg_raster_rho_kernel(double* x, long n, const double* theta) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= theta[2] * theta[3] / theta[4];
}

// factor columns of the two axes, A_d = a_d(g_d)  ([m_d][p_d]; vg_whitened_columns with one length per dimension)
int vg_raster_factors(vggp_ctx* c, const double* g1, long p1, const double* g2, long p2, double* A1, double* A2, hipStream_t st) {
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    VgFactorJob fj[2] = {VgFactorJob{g1, d1.grid, A1, nullptr, nullptr, nullptr, (int)p1, d1.m, d1.kind, d1.basis, 0, 0.0, c->desc.flags},
                         VgFactorJob{g2, d2.grid, A2, nullptr, nullptr, nullptr, (int)p2, d2.m, d2.kind, d2.basis, 1, 0.0, c->desc.flags}};
    VG_HIP(vg_factor_build_launch(fj, 2, c->theta, st));
    return VGGP_OK;
}

// full-grid state: vggp_posterior's preamble (accurate state or thin read-out, compact q1 x q2 weights, W_d = Q_d^T L0_d^-1), once per axis
int vg_raster_full(vggp_ctx* c, const double* g1, long p1, const double* g2, long p2, double* mean, double* var, hipStream_t st) {
    const long m1 = c->desc.m1, m2 = c->desc.m2;
    const bool thin_ro = vg_thin_readout(c);
    int rc = thin_ro ? VGGP_OK : vg_accurate_state(c, st);
    if (rc) return rc;
    const int q1 = thin_ro ? c->d[0].thin_rows : (int)m1, q2 = thin_ro ? c->d[1].thin_rows : (int)m2;
    // A1, T1 (m1 x p1); A2 (later T2 o T2), T2 (m2 x p2); U, Uv (m1 x p2); W_d (m_d x m_d)
    const size_t need = (size_t)(2 * m1 * p1 + 2 * m2 * p2 + 2 * m1 * p2 + m1 * m1 + m2 * m2);
    if ((rc = vg_ensure_misc(c, need * sizeof(double)))) return rc;
    double* p = (double*)c->misc;
    double* A1 = p; p += m1 * p1;
    double* T1 = p; p += m1 * p1;
    double* A2 = p; p += m2 * p2;
    double* T2 = p; p += m2 * p2;
    double* U = p; p += m1 * p2;
    double* Uv = p; p += m1 * p2;
    double* W1 = p; p += m1 * m1;
    double* W2 = p;
    double* T2sq = A2;                     // (the factor columns are consumed by then)
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    VG_HIP(vg_qv_weights_launch(c->theta, c->beta, c->invD, c->wq, (long)q1 * q2, st));   // wq = [beta rs / v | invD - 1]  (q1 x q2, compact)
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, d1.QtPrev, m1, 1, d1.Linv0, m1, 1, W1, (int)m1, q1, (int)m1, (int)m1);
    vg_gemm_add(&g, d2.QtPrev, m2, 1, d2.Linv0, m2, 1, W2, (int)m2, q2, (int)m2, (int)m2);
    VG_HIP(vg_gemm_launch(&g, st));
    if ((rc = vg_raster_factors(c, g1, p1, g2, p2, A1, A2, st))) return rc;
    vg_gemm_init(&g);
    vg_gemm_add(&g, W1, m1, 1, A1, p1, 1, T1, (int)p1, q1, (int)p1, (int)m1);
    vg_gemm_add(&g, W2, m2, 1, A2, p2, 1, T2, (int)p2, q2, (int)p2, (int)m2);
    VG_HIP(vg_gemm_launch(&g, st));
    if (var) VG_HIP(vg_scale_sq_launch(T2, T2sq, (long)q2 * p2, st));
    vg_gemm_init(&g);
    vg_gemm_add(&g, c->wq, q2, 1, T2, p2, 1, U, (int)p2, q1, (int)p2, q2);
    if (var) vg_gemm_add(&g, c->wq + (long)q1 * q2, q2, 1, T2sq, p2, 1, Uv, (int)p2, q1, (int)p2, q2);
    VG_HIP(vg_gemm_launch(&g, st));
    VG_HIP(vg_raster_launch(T1, U, var ? Uv : nullptr, q1, p1, p2, 1.0, 1.0, c->theta, mean, var, st));   // var = s1 s2 (1 + .)
    return VGGP_OK;
}

// M-space states (dense masked / scattered, iterative masked, iterative scattered): mean = (s1 s2 / v) U1^T A0 U2 with the state's own
// m1 x m2 coefficients A0 = mat(a0) and whitened axis factors U_d = L0_d^-1 A_d  (ax: where those sit in the scratch afterwards)
int vg_raster_mspace(vggp_ctx* c, const double* g1, long p1, const double* g2, long p2, double* mean, hipStream_t st, VgRasterAxes* ax) {
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    const long m1 = w.m1, m2 = w.m2;
    int rc = vg_ensure_misc(c, (size_t)(2 * m1 * p1 + 2 * m2 * p2 + m1 * p2) * sizeof(double));
    if (rc) return rc;
    double* p = (double*)c->misc;
    double* A1 = p; p += m1 * p1;
    double* U1 = p; p += m1 * p1;
    double* A2 = p; p += m2 * p2;
    double* U2 = p; p += m2 * p2;
    double* V = p;
    if (ax) *ax = VgRasterAxes{A1, U1, A2, U2};
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    if ((rc = vg_raster_factors(c, g1, p1, g2, p2, A1, A2, st))) return rc;
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, d1.Linv0, m1, 1, A1, p1, 1, U1, (int)p1, (int)m1, (int)p1, (int)m1);
    vg_gemm_add(&g, d2.Linv0, m2, 1, A2, p2, 1, U2, (int)p2, (int)m2, (int)p2, (int)m2);
    VG_HIP(vg_gemm_launch(&g, st));
    if ((rc = gemm1(w.a0, m2, 1, U2, p2, 1, V, (int)p2, (int)m1, (int)p2, (int)m2, st))) return rc;                 // A0 U2
    VGM_LAUNCH1D(vg_raster_rho_kernel, m1 * p2, st, V, m1 * p2, c->theta);
    VG_HIP(hipGetLastError());
    VG_HIP(vg_raster_launch(U1, V, nullptr, (int)m1, p1, p2, 0.0, 0.0, nullptr, mean, nullptr, st));
    return VGGP_OK;
}

extern "C" int vggp_posterior_raster(vggp_ctx* c, const double* g1, int64_t p1, const double* g2, int64_t p2, double* mean, double* var,
                                     void* stream) {
    static const char* fn = "vggp_posterior_raster";
    if (c && c->is_paired) {
        vg_set_error("%s: paired inducing points (VGGP_FLAG_PAIRED_Z) have no Kronecker factors to separate; use vggp_posterior_masked", fn);
        return VGGP_EINVAL;
    }
    if (!c || !c->planned) { vg_set_error("%s: context not planned", fn); return VGGP_ESTATE; }
    VG_REQUIRE(p1 >= 1 && p1 <= VR_MAXP && p2 >= 1 && p2 <= VR_MAXP, "%s: need 1 <= p1, p2 <= 2^20 (got %lld, %lld)", fn, (long long)p1,
               (long long)p2);
    VG_REQUIRE(g1 && g2 && mean, "%s: null argument", fn);
    // the last finished step, whichever kind: its own flag must still stand (a failed step, a re-plan or moved inducing points clear it)
    const bool iter = c->last_kind == VG_LAST_ITER && c->have_iter && c->masked;
    const bool dense = c->last_kind == VG_LAST_DENSE && c->have_masked && c->masked;
    const bool full = c->last_kind == VG_LAST_FULL && c->have_step;
    if (!iter && !dense && !full) { vg_set_error("%s: no finished ELBO step on this context", fn); return VGGP_ESTATE; }
    if (!full && var) {
        const bool sc = (c->desc.flags & VGGP_FLAG_SCATTERED) != 0;
        vg_set_error("%s: this state gives the raster mean only (var must be NULL): its variances t^T Sigma~^-1 t are no Kronecker sums; "
                     "use %s at the points", fn, dense ? "vggp_posterior_masked" : (sc ? "vggp_posterior_var_scattered_iter" : "vggp_posterior_masked_iter"));
        return VGGP_EINVAL;
    }
    if (iter) { const int vrc = vg_comm_verify(c, fn); if (vrc) return vrc; }        // (as the iterative point-wise entries)
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    int rc;
    if (full) return vg_raster_full(c, g1, (long)p1, g2, (long)p2, mean, var, st);
    if ((rc = vg_raster_mspace(c, g1, (long)p1, g2, (long)p2, mean, st))) return rc;
    if (iter) VGI_WAIT(c, st);
    else VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}
