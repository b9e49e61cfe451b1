// Joint samples of posterior(x*) on a RASTER: S correlated realisations of f on the p1 x p2 cartesian grid of two coordinate axes
// (vggp_posterior_raster_sample, vggp_posterior_raster_sample_masked_iter, vggp_posterior_raster_sample_scattered_iter), without any
// p1 p2 x p1 p2 matrix.  The covariance of the reference's posterior (kronecker_structure.py:223-229) on cartesian_prod(g1, g2) is
//     K** + Kuf*^T Sigma^-1 Kuf* - Kuf*^T Kuu^-1 Kuf*  =  (B1 (x) B2)^T Sigma~^-1 (B1 (x) B2)  +  s1 s2 (k1 (x) k2 - q1 (x) q2),
// a q(u) part, which the samplers of q(v) draw on every solver, plus the prior residual: a DIFFERENCE of two Kronecker products that
// splits exactly into a SUM of two positive semi-definite ones,
//     k1 (x) k2 - q1 (x) q2  =  (k1 - q1) (x) k2  +  q1 (x) (k2 - q2).
// State of the last finished step: theta = (ell1, ell2, s1, s2, sigma^2), L0_d the factor of K0_d at the step's jitter level, X_s the
// whitened coefficient draw of the vggp_qv_sample* entries ([m1][m2], Cov(vec X_s) = Sigma~^-1: the Kronecker eigenbasis on a full
// grid, one block PCG solve per <= 64 samples on the iterative solvers -- the SAME stage, called from here:
// vg_sample_full_coeffs in api.hip, vgi_sample_coeffs in iter_readout.hip).  For raster axes g_d of length p_d:
//     U_d = L0_d^-1 A0_d(g_d)  (m_d x p_d; vggp_posterior_raster's),     B_d = sqrt(s_d) U_d  (the same form for the 1/s bases, VFF)
//     k_d[a][a'] = kappa_d(|g_d[a] - g_d[a']| / ell_d)   the unit POINT kernel, for every basis of the model (vggp_factor_build's K0 with
//                                                        VGGP_BASIS_POINTS and grid = g_d)
//     r_d = k_d - U_d^T U_d  (= k_d - B_d^T B_d / s_d = k_d - q_d)
//     C_d = chol(r_d + eta I),   Kc_2 = chol(k_2 + eta I),     eta = VG_RS_NUGGET = 1e-8 at unit outputscale
// and sample s is
//     F_s = mu + B1^T W_s + sqrt(s1 s2) C1 T_s,     W_s = X_s B2 + sqrt(s2) H_s C2^T  (m1 x p2),     T_s = G_s Kc2^T  (p1 x p2)
// with mu the mean vggp_posterior_raster returns in the same state, G_s [p1][p2] and H_s [m1][p2] standard normals:
//     Cov(vec F_s) = (B1 (x) B2)^T Sigma~^-1 (B1 (x) B2) + s1 s2 [(r1 + eta I) (x) (k2 + eta I)] + (B1^T B1) (x) s2 (r2 + eta I).
// The nugget keeps the roots of the (often numerically singular: RBF, raster nodes on inducing points) residuals defined; it inflates
// the sample variance by about 2 eta s1 s2.  The roots come from vggp_cholesky_inverse with its jitter schedule ON TOP of the nugget
// (levels 0, 1e-8, 1e-7, 1e-6); info->jitter1 = the level C1 took, info->jitter2 = the larger of C2's and Kc2's; VGGP_ENOTPD when a
// root fails every level.  B1 hats: k_d - q_d is INDEFINITE there (the reference's ASVGP covariance is no Schur complement), refused.
// The roots are recomputed per call; nothing is cached on the axes.
//
// Noise: the counter-based generator of sample.hip; streams 0 (E) and 1 (F) exactly as the vggp_qv_sample* entries use them, and
//     stream 2  G  idx = s p1 p2 + a p2 + b          stream 3  H  idx = s m1 p2 + i p2 + b          (s = first + local sample)
// so sample s of a seed is the same numbers whatever n_samples, block or call asks for it, and shares E_s with sample s of q_v().
//
// Blocks.  Samples are processed in blocks of nbc <= min(64, block) samples, nbc chosen so that the p1 x p2 scratch T of a block stays
// under VG_RS_SCRATCH_CAP (1 GiB; one sample if a single map is larger).  G is generated straight into the block's part of `out` (an
// explicit eps_g is read where it is).  Per block, whatever the number of samples in it: the coefficient draw; H into the
// interleaved rows [m1][nbc][p2]; W = X B2' (one GEMM, rows (i, c)); W += H C2'^T and T = G Kc2'^T (one GEMM each; their tiles skip
// the zero half of the root); vg_rs_kernel.  (B2', C2', Kc2': times sqrt(s1 s2) on the device, once per call, so the kernel's c is 1.)
// Specification: tests/raster_sample_spec.py.
#include "mspace_ws.h"

typedef double vs_d4 __attribute__((ext_vector_type(4)));

#define VS_T 64                   // output tile: 64 x 64, four waves 2 x 2, each 32 x 32 = 2 x 2 MFMA blocks (as vg_raster_kernel)
#define VS_BK 16                  // k-tile
#define VS_KS (VS_T + 16)         // LDS row of a k-slice of an operand that is contiguous along the output index (80 doubles: raster.hip)
#define VS_CLD (VS_BK + 2)        // LDS row of C1's tile, stored [row][k]: 18 doubles, so the 16 rows x 2 k of a half-wave's fragment read
                                  // fall on 32 distinct 8-byte banks
#define VS_MAXP (1L << 20)        // axis length limit of the building block
#define VG_RS_MAXP 8192           // ... and of the entries: the Cholesky's limit
#define VG_RS_NUGGET 1e-8
#define VG_RS_SCRATCH_CAP (1L << 27)     // doubles of the block scratch T: 1 GiB

// out[s][a][b] = mean[a][b] + sum_i B1[i][a] W[s][i][b] + cs sum_{a' <= a} C1[a][a'] T[s][a'][b]
// B1 [q][P1]; W element (s, i, b) at W[s w_ss + i w_sr + b] (the exported block: [S][q][P2]; the entries: [q][nbc][P2]); C1 [P1][P1]
// lower triangular, NOTHING above its diagonal is read; T, out [S][P1][P2]; mean [P1][P2] or null.  One workgroup per 64 x 64 tile of
// one sample (blockIdx.y = s).  Both products accumulate in the same registers: first the k-range q of B1^T W, staged as in
// vg_raster_kernel (both operands contiguous along the output index: LDS [k][64 + 16]); then the k-range [0, min(row0 + 64, P1)) of
// C1 T -- it ends at the tile's last row, the triangular skip -- where C1's tile is contiguous along k: 16 lanes read 16 consecutive
// doubles of a row, the tile is stored [row][16 + 2] and the A fragment reads row = lane & 15, k = lane >> 4.  cs multiplies C1's
// elements on their way into LDS; cs = 0 skips the second product.  The mean is added in the epilogue.  Edges: rows / columns past
// P1 / P2, k past the range and a' > a are loaded as zeros, nothing past the edges is stored.  Output indices are 64-bit.
__global__ __launch_bounds__(256) void vg_rs_kernel(const double* __restrict__ B1, const double* __restrict__ W, long w_ss, long w_sr,
                                                    const double* __restrict__ C1, const double* __restrict__ T, double cs,
                                                    const double* __restrict__ mean, double* __restrict__ out, int q, long P1, long P2,
                                                    int tiles_n) {
    __shared__ double As[VS_BK * VS_KS], Bs[VS_BK * VS_KS], Cs[VS_T * VS_CLD];
    const int tm = (int)(blockIdx.x / (unsigned)tiles_n), tn = (int)(blockIdx.x - (unsigned)tm * (unsigned)tiles_n);
    const long row0 = (long)tm * VS_T, col0 = (long)tn * VS_T, s = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, fi = lane & 15, fk = lane >> 4;
    // operands contiguous along the output index: thread (j = tid & 63, kb = tid >> 6) moves elements (k = kb + 4 r, j), r = 0 .. 3
    const int j = tid & 63, kb = tid >> 6;
    // C1's tile: thread (ck = tid & 15, cr = tid >> 4) moves elements (row = cr + 16 r, k = ck), r = 0 .. 3
    const int ck = tid & 15, cr = tid >> 4;
    const bool aok = row0 + j < P1, bok = col0 + j < P2;
    const double* Ws = W + s * w_ss + (bok ? col0 + j : 0);
    const double* Ts = T + s * P1 * P2 + (bok ? col0 + j : 0);
    const double* pa = B1 + (aok ? row0 + j : 0);
    double ra[4], rb[4];
    vs_d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (vs_d4){0.0, 0.0, 0.0, 0.0};

    // ---- B1^T W over k < q
    auto load1 = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + kb + 4 * r;
            const bool kok = k < q;
            ra[r] = (aok && kok) ? pa[(long)k * P1] : 0.0;
            rb[r] = (bok && kok) ? Ws[(long)k * w_sr] : 0.0;
        }
    };
    load1(0);
    for (int k0 = 0; k0 < q; k0 += VS_BK) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            As[(kb + 4 * r) * VS_KS + j] = ra[r];
            Bs[(kb + 4 * r) * VS_KS + j] = rb[r];
        }
        __syncthreads();
        if (k0 + VS_BK < q) load1(k0 + VS_BK);          // the next k-tile is in flight while this one is multiplied
#pragma unroll
        for (int kk = 0; kk < VS_BK; kk += 4) {
            double fa[2], fb[2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) fa[mb] = As[(kk + fk) * VS_KS + wr * 32 + mb * 16 + fi];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) fb[nb] = Bs[(kk + fk) * VS_KS + wc * 32 + nb * 16 + fi];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[mb], fb[nb], acc[mb][nb], 0, 0, 0);
        }
        __syncthreads();
    }

    // ---- cs C1 T over a' < min(row0 + 64, P1): the rows of this tile read nothing right of the diagonal
    const long kend = cs != 0.0 ? (row0 + VS_T < P1 ? row0 + VS_T : P1) : 0;
    auto load2 = [&](long k0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long row = row0 + cr + 16 * r, kc = k0 + ck, kt = k0 + kb + 4 * r;
            ra[r] = (row < P1 && kc <= row) ? cs * C1[row * P1 + kc] : 0.0;
            rb[r] = (bok && kt < kend) ? Ts[kt * P2] : 0.0;
        }
    };
    if (kend > 0) load2(0);
    for (long k0 = 0; k0 < kend; k0 += VS_BK) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Cs[(cr + 16 * r) * VS_CLD + ck] = ra[r];
            Bs[(kb + 4 * r) * VS_KS + j] = rb[r];
        }
        __syncthreads();
        if (k0 + VS_BK < kend) load2(k0 + VS_BK);
#pragma unroll
        for (int kk = 0; kk < VS_BK; kk += 4) {
            double fa[2], fb[2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) fa[mb] = Cs[(wr * 32 + mb * 16 + fi) * VS_CLD + kk + fk];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) fb[nb] = Bs[(kk + fk) * VS_KS + wc * 32 + nb * 16 + fi];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[mb], fb[nb], acc[mb][nb], 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D fragment of the fp64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * reg
    double* os = out + s * P1 * P2;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = row0 + wr * 32 + mb * 16 + fk + 4 * r, col = col0 + wc * 32 + nb * 16 + fi;
                if (row < P1 && col < P2) os[row * P2 + col] = mean ? mean[row * P2 + col] + acc[mb][nb][r] : acc[mb][nb][r];
            }
}

static hipError_t vg_rs_launch(const double* B1, const double* W, long w_ss, long w_sr, const double* C1, const double* T, double cs,
                               const double* mean, double* out, int q, long P1, long P2, int S, hipStream_t st) {
    const long tiles_m = (P1 + VS_T - 1) / VS_T, tiles_n = (P2 + VS_T - 1) / VS_T;
    if (q < 1 || P1 < 1 || P2 < 1 || P1 > VS_MAXP || P2 > VS_MAXP || S < 1 || S > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vg_rs_kernel, dim3((unsigned)(tiles_m * tiles_n), (unsigned)S), dim3(256), 0, st, B1, W, w_ss, w_sr, C1, T, cs, mean, out,
                       q, P1, P2, (int)tiles_n);
    return hipGetLastError();
}

extern "C" int vggp_raster_sample_contract(vggp_ctx* c, const double* B1, const double* Wt, const double* C1, const double* Tt, int64_t S,
                                           int64_t q, int64_t P1, int64_t P2, double cs, const double* mean, double* out, void* stream) {
    static const char* fn = "vggp_raster_sample_contract";
    if (!c) { vg_set_error("%s: null context", fn); return VGGP_EINVAL; }
    VG_REQUIRE(B1 && Wt && C1 && Tt && out, "%s: null argument (only mean may be NULL)", fn);
    VG_REQUIRE(q >= 1 && q <= VS_MAXP && P1 >= 1 && P1 <= VS_MAXP && P2 >= 1 && P2 <= VS_MAXP, "%s: need 1 <= q, P1, P2 <= 2^20", fn);
    VG_REQUIRE(S >= 1 && S <= 65535, "%s: need 1 <= S <= 65535 samples per launch", fn);
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VG_HIP(vg_rs_launch(B1, Wt, (long)q * P2, (long)P2, C1, Tt, cs, mean, out, (int)q, (long)P1, (long)P2, (int)S, st));
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

// ---- what the three entries share -------------------------------------------------------------------------------------------------
struct VgRasterSample {
    long m1, m2, p1, p2;
    int nbc;
    double *mean, *A1, *U1, *A2, *U2, *R1, *C1, *R2, *C2, *Kc2, *Linv, *Hb, *Wb, *T, *Xa, *Xb;
};

// samples per block: the caller's block (0: 64), at most 64 and n_samples, and T = nbc p1 p2 doubles under the cap
static int vg_rs_block(int block, int64_t n_samples, long p1, long p2) {
    const long fit = std::max<long>(1, VG_RS_SCRATCH_CAP / (p1 * p2));
    return (int)std::min<long>(std::min<long>(block > 0 ? block : 64, 64), std::min<long>((long)n_samples, fit));
}

// the arguments every entry refuses before anything is launched or written (the context is planned and not paired here)
static int vg_rs_check(const vggp_ctx* c, const char* fn, const double* g1, int64_t p1, const double* g2, int64_t p2, const double* eps_u,
                       const double* eps_g, const double* eps_h, const double* eps_obs, bool has_obs) {
    for (int k = 0; k < 2; ++k)
        VG_REQUIRE(c->d[k].basis != VGGP_BASIS_B1, "%s: dimension %d uses B1 hats, whose prior residual k - q is indefinite (the covariance of "
                   "that basis is no Schur complement): it has no root and no joint sample", fn, k + 1);
    VG_REQUIRE(p1 >= 1 && p1 <= VG_RS_MAXP && p2 >= 1 && p2 <= VG_RS_MAXP, "%s: need 1 <= p1, p2 <= 8192, the Cholesky's limit (got %lld, %lld)",
               fn, (long long)p1, (long long)p2);
    VG_REQUIRE(g1 && g2, "%s: null axis", fn);
    const int given = (eps_u != nullptr) + (eps_g != nullptr) + (eps_h != nullptr) + (has_obs && eps_obs != nullptr);
    VG_REQUIRE(given == 0 || given == (has_obs ? 4 : 3), "%s: the noise arrays are either all NULL (generated noise) or all given", fn);
    return VGGP_OK;
}

// the samplers' own scratch (also vggp_qv_sample_masked's, dense_sample.hip): kept while it is large enough, replaced when it is not
int vg_rs_reserve(vggp_ctx* c, const char* fn, size_t need, int nbc) {
    if (c->rs_bytes < need) {
        if (c->rs_mem) { VG_HIP(hipFree(c->rs_mem)); c->rs_mem = nullptr; c->rs_bytes = 0; }
        if (hipMalloc(&c->rs_mem, need) != hipSuccess) {
            (void)hipGetLastError();
            c->rs_mem = nullptr;
            vg_set_error("%s: the workspace of a block of %d samples needs %.1f GiB of device memory (a smaller block needs less)", fn, nbc,
                         (double)need / (1024.0 * 1024.0 * 1024.0));
            return VGGP_ENOMEM;
        }
        c->rs_bytes = need;
    }
    return VGGP_OK;
}

// workspace, the axis factors and the three roots.  xab: doubles of each of the coefficient draw's two block vectors where the draw
// lives here (full grid: eigenbasis coefficients and draw; dense states: E and X = Xg^T E; 0 on the iterative states, whose draw lives
// in the read-outs' workspace)
static int vg_rs_setup(vggp_ctx* c, const char* fn, VgRasterSample& z, const double* g1, const double* g2, long xab, vggp_info* info, hipStream_t st) {
    const long m1 = z.m1, m2 = z.m2, p1 = z.p1, p2 = z.p2, pm = std::max(p1, p2);
    const size_t need = (size_t)(p1 * p2 + 2 * m1 * p1 + 2 * m2 * p2 + 2 * p1 * p1 + 3 * p2 * p2 + pm * pm + 2 * m1 * z.nbc * p2 +
                                 (long)z.nbc * p1 * p2 + 2 * xab) * sizeof(double);
    int rrc = vg_rs_reserve(c, fn, need, z.nbc);
    if (rrc) return rrc;
    double* p = (double*)c->rs_mem;
    z.mean = p; p += p1 * p2;
    z.A1 = p; p += m1 * p1;
    z.U1 = p; p += m1 * p1;
    z.A2 = p; p += m2 * p2;
    z.U2 = p; p += m2 * p2;
    z.R1 = p; p += p1 * p1;
    z.C1 = p; p += p1 * p1;
    z.R2 = p; p += p2 * p2;
    z.C2 = p; p += p2 * p2;
    z.Kc2 = p; p += p2 * p2;
    z.Linv = p; p += pm * pm;
    z.Hb = p; p += m1 * z.nbc * p2;
    z.Wb = p; p += m1 * z.nbc * p2;
    z.T = p; p += (long)z.nbc * p1 * p2;
    z.Xa = p; p += xab;
    z.Xb = p;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    int rc;
    if ((rc = vg_raster_factors(c, g1, p1, g2, p2, z.A1, z.A2, st))) return rc;
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, d1.Linv0, m1, 1, z.A1, p1, 1, z.U1, (int)p1, (int)m1, (int)p1, (int)m1);                      // U_d = L0_d^-1 A_d
    vg_gemm_add(&g, d2.Linv0, m2, 1, z.A2, p2, 1, z.U2, (int)p2, (int)m2, (int)p2, (int)m2);
    VG_HIP(vg_gemm_launch(&g, st));
    // k_d: the unit point kernel of the dimension on its axis
    VgFactorJob fj[2] = {VgFactorJob{nullptr, g1, nullptr, nullptr, z.R1, nullptr, 0, (int)p1, d1.kind, VGGP_BASIS_POINTS, 0, 0.0, c->desc.flags},
                         VgFactorJob{nullptr, g2, nullptr, nullptr, z.R2, nullptr, 0, (int)p2, d2.kind, VGGP_BASIS_POINTS, 1, 0.0, c->desc.flags}};
    VG_HIP(vg_factor_build_launch(fj, 2, c->theta, st));
    VG_HIP(vg_sample_nugget_launch(z.R1, p1, VG_RS_NUGGET, st));
    VG_HIP(vg_sample_nugget_launch(z.R2, p2, VG_RS_NUGGET, st));
    double jk2 = 0.0, j1 = 0.0, j2 = 0.0;
    if ((rc = vggp_cholesky_inverse(c, z.R2, p2, z.Kc2, z.Linv, &jk2, st))) return rc;                                // Kc2 = chol(k2 + eta I)
    vg_gemm_init(&g);                                                                                                 // r_d = k_d - U_d^T U_d
    vg_gemm_add(&g, z.U1, 1, p1, z.U1, p1, 1, z.R1, (int)p1, (int)p1, (int)p1, (int)m1, 1, 0, 1, 0, -1.0, 1);
    vg_gemm_add(&g, z.U2, 1, p2, z.U2, p2, 1, z.R2, (int)p2, (int)p2, (int)p2, (int)m2, 1, 0, 1, 0, -1.0, 1);
    VG_HIP(vg_gemm_launch(&g, st));
    if ((rc = vggp_cholesky_inverse(c, z.R2, p2, z.C2, z.Linv, &j2, st))) return rc;
    if ((rc = vggp_cholesky_inverse(c, z.R1, p1, z.C1, z.Linv, &j1, st))) return rc;
    if (info) { info->jitter1 = j1; info->jitter2 = std::max(j2, jk2); }
    // sqrt(s1 s2) goes into the right-hand factors once, so that the kernel's scalar is 1 and theta stays on the device
    VG_HIP(vg_sample_scale_root_launch(z.U2, m2 * p2, c->theta, st));
    VG_HIP(vg_sample_scale_root_launch(z.C2, p2 * p2, c->theta, st));
    VG_HIP(vg_sample_scale_root_launch(z.Kc2, p2 * p2, c->theta, st));
    return VGGP_OK;
}

// one block: X [m1][nbc][m2] (the coefficient draw) -> out[cn][p1][p2].  eps_g, eps_h: the block's first sample, or null (streams 2, 3)
static int vg_rs_block_out(vggp_ctx* c, const VgRasterSample& z, const double* X, const double* eps_g, const double* eps_h, uint64_t seed,
                           unsigned long long s0, int cn, double* out, hipStream_t st) {
    const long m1 = z.m1, m2 = z.m2, p1 = z.p1, p2 = z.p2;
    const int nbc = z.nbc;
    VG_HIP(vg_sample_rows_noise_launch(z.Hb, eps_h, seed, 3u, s0, (int)m1, nbc, p2, cn, st));
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, X, m2, 1, z.U2, p2, 1, z.Wb, (int)p2, (int)(m1 * nbc), (int)p2, (int)m2);                          // W = X B2'
    VG_HIP(vg_gemm_launch(&g, st));
    vg_gemm_init(&g);
    int i = vg_gemm_add(&g, z.Hb, p2, 1, z.C2, 1, p2, z.Wb, (int)p2, (int)(m1 * nbc), (int)p2, (int)p2, 1, 0, 1, 0, 1.0, 1);   // W += H C2'^T
    g.p[i].tri = VG_TRI_B_UPPER;
    VG_HIP(vg_gemm_launch(&g, st));
    const double* G = eps_g;
    if (!G) {
        VG_HIP(vg_normal_fill_launch(seed, 2u, s0 * (unsigned long long)(p1 * p2), (long)cn * p1 * p2, out, st));     // G into the output block
        G = out;
    }
    vg_gemm_init(&g);
    i = vg_gemm_add(&g, G, p2, 1, z.Kc2, 1, p2, z.T, (int)p2, (int)(cn * p1), (int)p2, (int)p2);                       // T = G Kc2'^T
    g.p[i].tri = VG_TRI_B_UPPER;
    VG_HIP(vg_gemm_launch(&g, st));
    VG_HIP(vg_rs_launch(z.U1, z.Wb, p2, (long)nbc * p2, z.C1, z.T, 1.0, z.mean, out, (int)m1, p1, p2, cn, st));
    return VGGP_OK;
}

extern "C" int vggp_posterior_raster_sample(vggp_ctx* c, const double* g1, int64_t p1, const double* g2, int64_t p2, int64_t n_samples,
                                            uint64_t seed, int64_t first, const double* eps_u, const double* eps_g, const double* eps_h,
                                            double* out, vggp_info* info, void* stream) {
    static const char* fn = "vggp_posterior_raster_sample";
    VG_NOT_PAIRED(c, fn);
    if (!c || !c->planned) { vg_set_error("%s: context not planned", fn); return VGGP_ESTATE; }
    VG_REQUIRE(c->n_ranks == 1 && !c->comm && !c->cb, "%s: joint samples run on single-rank contexts only (this context is multi-rank)", fn);
    int rc = vg_rs_check(c, fn, g1, p1, g2, p2, eps_u, eps_g, eps_h, nullptr, false);
    if (rc) return rc;
    VG_REQUIRE(n_samples >= 1 && n_samples < (1LL << 31), "%s: n_samples = %lld must be at least 1", fn, (long long)n_samples);
    VG_REQUIRE(first >= 0 && out, "%s: bad argument", fn);
    if (!c->have_step || c->last_kind != VG_LAST_FULL) { vg_set_error("%s: no finished full-grid ELBO step on this context", fn); return VGGP_ESTATE; }
    if (info) { info->jitter1 = info->jitter2 = 0.0; info->sweeps1 = info->sweeps2 = info->rounds1 = info->rounds2 = 0; info->status = 0; info->polished = 0; }
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgRasterSample z{};
    z.m1 = c->desc.m1; z.m2 = c->desc.m2; z.p1 = p1; z.p2 = p2;
    z.nbc = vg_rs_block(0, n_samples, p1, p2);
    const long M = z.m1 * z.m2;
    if ((rc = vg_rs_setup(c, fn, z, g1, g2, M * z.nbc, info, st))) return rc;
    // the mean first: in the state vggp_posterior_raster reads (a thin step's range read-out included); then the samplers' state
    if ((rc = vg_raster_full(c, g1, p1, g2, p2, z.mean, nullptr, st))) return rc;
    if ((rc = vg_accurate_state(c, st))) return rc;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const int wide = z.nbc * (int)z.m2, tall = (int)z.m1 * z.nbc;
    for (int64_t off = 0; off < n_samples; off += z.nbc) {
        const int cn = (int)std::min<int64_t>(z.nbc, n_samples - off);
        const unsigned long long s0 = (unsigned long long)(first + off);
        if ((rc = vg_sample_full_coeffs(c, eps_u ? eps_u + off * M : nullptr, seed, s0, z.nbc, cn, z.Xa, z.Xb, st))) return rc;
        VgGemmBatch g;                                                    // X = Q1 (.) Q2^T: back from the eigenbasis (rows of QtPrev = eigenvectors)
        vg_gemm_init(&g);
        vg_gemm_add(&g, z.Xa, z.m2, 1, d2.QtPrev, z.m2, 1, z.Xb, (int)z.m2, tall, (int)z.m2, (int)z.m2);
        VG_HIP(vg_gemm_launch(&g, st));
        vg_gemm_init(&g);
        vg_gemm_add(&g, d1.QtPrev, 1, z.m1, z.Xb, wide, 1, z.Xa, wide, (int)z.m1, wide, (int)z.m1);
        VG_HIP(vg_gemm_launch(&g, st));
        if ((rc = vg_rs_block_out(c, z, z.Xa, eps_g ? eps_g + off * p1 * p2 : nullptr, eps_h ? eps_h + off * z.m1 * p2 : nullptr, seed, s0, cn,
                                  out + off * p1 * p2, st)))
            return rc;
    }
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

static int vg_rs_iter_run(vggp_ctx* c, const char* fn, bool scattered, const double* g1, int64_t p1, const double* g2, int64_t p2, const double* W,
                          double n_obs, int64_t n_samples, uint64_t seed, int64_t first, const double* eps_u, const double* eps_obs,
                          const double* eps_g, const double* eps_h, double tol, int max_iter, int block, double* out, vggp_info* info,
                          void* stream) {
    VG_NOT_PAIRED(c, fn);
    if (!c || !c->planned) { vg_set_error("%s: context not planned", fn); return VGGP_ESTATE; }
    int rc = vg_rs_check(c, fn, g1, p1, g2, p2, eps_u, eps_g, eps_h, eps_obs, true);
    if (rc) return rc;
    if ((rc = vgi_sample_enter(c, fn, scattered, W, n_obs, n_samples, first, out, true, "", &tol, &max_iter, &block, info))) return rc;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    VgRasterSample z{};
    z.m1 = w.m1; z.m2 = w.m2; z.p1 = p1; z.p2 = p2;
    z.nbc = vg_rs_block(block, n_samples, p1, p2);
    const long M = w.M, nodes = scattered ? w.n1 : w.n1 * w.n2;
    if ((rc = vg_rs_setup(c, fn, z, g1, g2, 0, info, st))) return rc;
    if ((rc = vg_raster_mspace(c, g1, p1, g2, p2, z.mean, st))) return rc;
    VgReadout r;
    if ((rc = vgi_sample_prepare(c, r, z.nbc, W, n_obs, /*qv_mean=*/false, st))) return rc;
    int max_its = 0, solves = 0;
    for (int64_t off = 0; off < n_samples; off += z.nbc) {
        const int cn = (int)std::min<int64_t>(z.nbc, n_samples - off);
        const unsigned long long s0 = (unsigned long long)(first + off);
        if ((rc = vgi_sample_coeffs(c, r, fn, scattered, eps_u ? eps_u + off * M : nullptr, eps_obs ? eps_obs + off * nodes : nullptr, seed, s0, cn,
                                    tol, max_iter, &solves, &max_its, info, st)))
            return rc;
        if ((rc = vg_rs_block_out(c, z, r.it.X, eps_g ? eps_g + off * p1 * p2 : nullptr, eps_h ? eps_h + off * z.m1 * p2 : nullptr, seed, s0, cn,
                                  out + off * p1 * p2, st)))
            return rc;
    }
    VGI_WAIT(c, st);
    return VGGP_OK;
}

// the dense masked / scattered states: the coefficient draw is X = Xg^T E, one launch of dense_sample.hip's triangular product on the
// inverse factor the step keeps (no solve: info->rounds* and sweeps* stay 0); E and X are the setup's two block vectors
extern "C" int vggp_posterior_raster_sample_masked(vggp_ctx* c, const double* g1, int64_t p1, const double* g2, int64_t p2, int64_t n_samples,
                                                   uint64_t seed, int64_t first, const double* eps_u, const double* eps_g, const double* eps_h,
                                                   int block, double* out, vggp_info* info, void* stream) {
    static const char* fn = "vggp_posterior_raster_sample_masked";
    VG_NOT_PAIRED(c, fn);
    if (!c || !c->planned) { vg_set_error("%s: context not planned", fn); return VGGP_ESTATE; }
    VG_REQUIRE(!vgi_multi(c), "%s: joint samples run on single-rank contexts only (this context is multi-rank)", fn);
    int rc = vg_rs_check(c, fn, g1, p1, g2, p2, eps_u, eps_g, eps_h, nullptr, false);
    if (rc) return rc;
    if ((rc = vg_dense_sample_enter(c, fn, n_samples, first, out, block, info))) return rc;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    VgRasterSample z{};
    z.m1 = w.m1; z.m2 = w.m2; z.p1 = p1; z.p2 = p2;
    z.nbc = vg_rs_block(block, n_samples, p1, p2);
    const long M = w.M;
    if ((rc = vg_rs_setup(c, fn, z, g1, g2, M * z.nbc, info, st))) return rc;
    if ((rc = vg_raster_mspace(c, g1, p1, g2, p2, z.mean, st))) return rc;
    for (int64_t off = 0; off < n_samples; off += z.nbc) {
        const int cn = (int)std::min<int64_t>(z.nbc, n_samples - off);
        const unsigned long long s0 = (unsigned long long)(first + off);
        VG_HIP(vg_sample_block_noise_launch(z.Xa, eps_u ? eps_u + off * M : nullptr, seed, s0, (int)z.m1, z.nbc, (int)z.m2, cn, st));
        VG_HIP(vg_tri_t_apply_launch(w.Xg, z.m1, z.m2, z.Xa, z.nbc, cn, z.Xb, st));
        if ((rc = vg_rs_block_out(c, z, z.Xb, eps_g ? eps_g + off * p1 * p2 : nullptr, eps_h ? eps_h + off * z.m1 * p2 : nullptr, seed, s0, cn,
                                  out + off * p1 * p2, st)))
            return rc;
    }
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

extern "C" int vggp_posterior_raster_sample_masked_iter(vggp_ctx* c, const double* g1, int64_t p1, const double* g2, int64_t p2, const double* W,
                                                        double n_obs, int64_t n_samples, uint64_t seed, int64_t first, const double* eps_u,
                                                        const double* eps_obs, const double* eps_g, const double* eps_h, double tol,
                                                        int max_iter, int block, double* out, vggp_info* info, void* stream) {
    return vg_rs_iter_run(c, "vggp_posterior_raster_sample_masked_iter", false, g1, p1, g2, p2, W, n_obs, n_samples, seed, first, eps_u, eps_obs,
                          eps_g, eps_h, tol, max_iter, block, out, info, stream);
}
extern "C" int vggp_posterior_raster_sample_scattered_iter(vggp_ctx* c, const double* g1, int64_t p1, const double* g2, int64_t p2,
                                                           int64_t n_samples, uint64_t seed, int64_t first, const double* eps_u,
                                                           const double* eps_obs, const double* eps_g, const double* eps_h, double tol,
                                                           int max_iter, int block, double* out, vggp_info* info, void* stream) {
    return vg_rs_iter_run(c, "vggp_posterior_raster_sample_scattered_iter", true, g1, p1, g2, p2, nullptr, 0.0, n_samples, seed, first, eps_u,
                          eps_obs, eps_g, eps_h, tol, max_iter, block, out, info, stream);
}
