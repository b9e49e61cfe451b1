// Paired (general) inducing points: Z = {(z_i1, z_i2)}, i < M, any set of points -- the reference's Matern12SVGP /
// GriddedMatern12SVGP with a Z that is no cartesian grid (gridded_kronecker_structure.py:235-264, :396-438; bound
// kronecker_structure.py:249-278).  kernel = kernel_1 * kernel_2 on active_dims 0 and 1, so
//     Kuu = s (K1 o K2),  Kuf[i, k] = s k1(z_i1, x_k1) k2(z_i2, x_k2) = s B[i, k],  s = s1 s2,
// a Hadamard / face-splitting structure, not a Kronecker one.  Everything is dense in M-space (M <= 16384):
//     Kj = Kuu + eps I (psd_safe_cholesky schedule on Kuu itself),  Phi = s^2 P0 (P0 = B B^T),  c = s b (b = B y),
//     Sigma = Kj + Phi / v,  alpha = Sigma^-1 c,
//     ELBO = -1/2 [N log 2 pi v + log|Sigma| - log|Kj| + y^T y / v - c^T alpha / v^2] - (N s - tr(Kj^-1 Phi)) / (2 v).
// Sensitivities (M x M):  Kb = dE/dKuu = (Kinv - Sinv - alpha alpha^T / v^2) / 2 - Kinv Phi Kinv / (2 v),
//                         Pb = dE/dPhi = (Kinv - Sinv - alpha alpha^T / v^2) / (2 v),  cb = dE/dc = alpha / v^2,
// and dE/dKuf = 2 Pb Kuf + cb y^T is contracted against dKuf/d(ell_d, s, z_id) without forming the M x N matrix:
//   full grid   B[i, (a, b)] = A1[i, a] A2[i, b]:  P0 = (A1 A1^T) o (A2 A2^T), b = rowdot(A1 Y^T, A2); the Pb part of the
//               contraction separates through the Grams (dA1 A1^T) o (A2 A2^T) ..., the cb part through rowdots with A2 Y, A1 Y^T
//   scattered   one generated-operand MFMA kernel (pz_gen_gemm_kernel): the B tiles are evaluated on chip from (z, x), never
//               stored -- pass 1 P0 (upper tiles) and b, pass 2 R = Pb B with the contraction in its epilogue; the read-outs'
//               variances diag(F Q F^T) go through the same kernel with F generated from (z, x*) or from C1, C2.
// Split reductions are summed in a fixed order (no float atomics): every result is bitwise repeatable.
// Specification: tests/general_z_spec.py.
#include "arena.h"
#include "gen_gemm.h"

#include <algorithm>
#include <cmath>

// ---- element-wise / row kernels ----------------------------------------------------------------------------------------------

// unit-outputscale K1 o K2 at the inducing points
__global__ void pz_kuu_kernel(const double* z1, const double* z2, int M, int kind1, int kind2, double inv1, double inv2, double* K0) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)M * M) return;
    const int i = (int)(idx / M), j = (int)(idx - (long)i * M);
    double v1, d1, v2, d2;
    vg_kappa(kind1, fabs(z1[i] - z1[j]), inv1, v1, d1);
    vg_kappa(kind2, fabs(z2[i] - z2[j]), inv2, v2, d2);
    K0[idx] = v1 * v2;
}
// A_d[i][a] = k_d(z_id, x_a), dA_d = d/d ell_d, zA_d = d/d z_id  (M x n, full grid)
__global__ void pz_afac_kernel(const double* z, const double* x, int M, long n, int kind, double inv, double* A, double* dA, double* zA) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)M * n) return;
    const int i = (int)(idx / n);
    const long a = idx - (long)i * n;
    double v, dl, dz;
    vg_kappa_z(kind, z[i] - x[a], inv, v, dl, dz);
    A[idx] = v; dA[idx] = dl; zA[idx] = dz;
}
// out = s K0 + eps I (+ rho P0)
__global__ void pz_fill_kernel(const double* K0, const double* P0, int M, double s, double eps, double rho, double* out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)M * M) return;
    const int i = (int)(idx / M), j = (int)(idx - (long)i * M);
    double v = s * K0[idx] + (i == j ? eps : 0.0);
    if (P0) v += rho * P0[idx];
    out[idx] = v;
}
__global__ void pz_hadamard_kernel(const double* a, const double* b, long n, double* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] * b[i];
}
__global__ void pz_scale_kernel(const double* a, long n, double w, double* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = w * a[i];
}
// Pb = (Kinv - Sinv - alpha alpha^T / v^2) / (2 v)
__global__ void pz_phib_kernel(const double* Kinv, const double* Sinv, const double* alpha, int M, double v, double* Pb) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)M * M) return;
    const int i = (int)(idx / M), j = (int)(idx - (long)i * M);
    Pb[idx] = (Kinv[idx] - Sinv[idx] - alpha[i] * alpha[j] / (v * v)) / (2.0 * v);
}
// Q = Sinv - Kinv (conditional) or s^2 Kinv P0 Kinv / v (literal: S_u^-1 - Kinv)
__global__ void pz_q_kernel(const double* Kinv, const double* Sinv, const double* KPK, long n, double w, int literal, double* Q) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) Q[i] = literal ? w * KPK[i] : Sinv[i] - Kinv[i];
}


// per-row scalars of the bound: sum_j Kinv P0, sum_j Sinv P0, log Lk_ii, log Ls_ii, alpha_i (P0 alpha)_i, b_i alpha_i, wv_i^2
__global__ __launch_bounds__(256) void pz_rowa_kernel(const double* Kinv, const double* Sinv, const double* P0, const double* Lk,
                                                      const double* Ls, const double* alpha, const double* Pa, const double* b,
                                                      const double* wv, int M, double* rowA) {
    __shared__ double sh[256];
    const int i = blockIdx.x;
    const long o = (long)i * M;
    double tk = 0.0, ts = 0.0;
    for (int j = threadIdx.x; j < M; j += 256) { tk += Kinv[o + j] * P0[o + j]; ts += Sinv[o + j] * P0[o + j]; }
    tk = pz_block_sum(tk, sh);
    ts = pz_block_sum(ts, sh);
    if (threadIdx.x == 0) {
        double* r = rowA + (long)i * 8;
        r[0] = tk; r[1] = ts; r[2] = log(Lk[o + i]); r[3] = log(Ls[o + i]); r[4] = alpha[i] * Pa[i]; r[5] = b[i] * alpha[i]; r[6] = wv[i] * wv[i];
    }
}

// per-row gradient parts of the Kuu sensitivity (kernel derivatives generated at (z_i, z_j)) and, on a full grid, of the Phi
// sensitivity through the Grams: rowC[i] = {sum_j Kb dK0/dell1, .. dell2, sum_j Kb dK0/dz_i1, .. dz_i2, <Kb, K0>_i, <Pb, P0>_i,
// sum_j Pb (H1 o G2), Pb (G1 o H2), Pb (Z1 o G2), Pb (G1 o Z2)}
struct PzRowC {
    const double *Kinv, *Sinv, *KPK, *Pb, *P0, *alpha, *z1, *z2;
    const double *G1, *H1, *Z1, *G2, *H2, *Z2;      // null on scattered data
    int M, kind1, kind2;
    double inv1, inv2, v, s2v;                       // s2v = s^2 / v
    double* rowC;
};
__global__ __launch_bounds__(256) void pz_rowc_kernel(const PzRowC a) {
    __shared__ double sh[256];
    const int i = blockIdx.x, M = a.M;
    const long o = (long)i * M;
    const double zi1 = a.z1[i], zi2 = a.z2[i], ai = a.alpha[i], iv2 = 1.0 / (a.v * a.v);
    double q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = threadIdx.x; j < M; j += 256) {
        const double kb = 0.5 * (a.Kinv[o + j] - a.Sinv[o + j] - ai * a.alpha[j] * iv2) - 0.5 * a.s2v * a.KPK[o + j];
        double v1, l1, d1, v2, l2, d2;
        vg_kappa_z(a.kind1, zi1 - a.z1[j], a.inv1, v1, l1, d1);
        vg_kappa_z(a.kind2, zi2 - a.z2[j], a.inv2, v2, l2, d2);
        q[0] += kb * l1 * v2; q[1] += kb * v1 * l2; q[2] += kb * d1 * v2; q[3] += kb * v1 * d2; q[4] += kb * v1 * v2;
        const double pb = a.Pb[o + j];
        q[5] += pb * a.P0[o + j];
        if (a.G1) {
            q[6] += pb * a.H1[o + j] * a.G2[o + j];
            q[7] += pb * a.G1[o + j] * a.H2[o + j];
            q[8] += pb * a.Z1[o + j] * a.G2[o + j];
            q[9] += pb * a.G1[o + j] * a.Z2[o + j];
        }
    }
    for (int k = 0; k < 10; ++k) {
        const double t = pz_block_sum(q[k], sh);
        if (threadIdx.x == 0) a.rowC[(long)i * 12 + k] = t;
    }
}

// full grid: rd[i] = {rowdot(T, A2) = b_i, rowdot(U, dA1), rowdot(U, zA1), rowdot(T, dA2), rowdot(T, zA2)},  T = A1 Y^T, U = A2 Y
__global__ __launch_bounds__(256) void pz_rowdot_kernel(const double* T, const double* U, const double* A2, const double* dA1,
                                                        const double* zA1, const double* dA2, const double* zA2, long n1, long n2,
                                                        double* rd, double* b) {
    __shared__ double sh[256];
    const int i = blockIdx.x;
    const long o1 = (long)i * n1, o2 = (long)i * n2;
    double q[5] = {0, 0, 0, 0, 0};
    for (long a = threadIdx.x; a < n1; a += 256) { const double u = U[o1 + a]; q[1] += u * dA1[o1 + a]; q[2] += u * zA1[o1 + a]; }
    for (long c = threadIdx.x; c < n2; c += 256) {
        const double t = T[o2 + c];
        q[0] += t * A2[o2 + c]; q[3] += t * dA2[o2 + c]; q[4] += t * zA2[o2 + c];
    }
    for (int k = 0; k < 5; ++k) {
        const double t = pz_block_sum(q[k], sh);
        if (threadIdx.x == 0) { rd[(long)i * 8 + k] = t; if (k == 0) b[i] = t; }
    }
}

struct PzFinal {
    const double *rowA, *rowC, *rowD, *alpha;     // rowD: [M][8] (grid: rd; scattered: the pass-2 row sums, 4 per row)
    int M, grid;
    double N, yy, s, v, s1, s2;
    double *out, *gz1, *gz2;
};
// per-row gradient: g_ell_d and g_z_id parts, then (block 0) the fixed-order sums
__device__ __forceinline__ void pz_row_grad(const PzFinal& a, int i, double (&g)[4]) {
    const double* C = a.rowC + (long)i * 12;
    const double* D = a.rowD + (long)i * (a.grid ? 8 : 4);
    const double s = a.s, cb = a.alpha[i] / (a.v * a.v);
    if (a.grid) {
        g[0] = s * C[0] + s * (2.0 * s * C[6] + cb * D[1]);
        g[1] = s * C[1] + s * (2.0 * s * C[7] + cb * D[3]);
        g[2] = 2.0 * s * C[2] + s * (2.0 * s * C[8] + cb * D[2]);
        g[3] = 2.0 * s * C[3] + s * (2.0 * s * C[9] + cb * D[4]);
    } else {
        g[0] = s * C[0] + s * D[0];
        g[1] = s * C[1] + s * D[1];
        g[2] = 2.0 * s * C[2] + s * D[2];
        g[3] = 2.0 * s * C[3] + s * D[3];
    }
}
__global__ void pz_gz_kernel(const PzFinal a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    double g[4];
    pz_row_grad(a, i, g);
    a.gz1[i] = g[2];
    a.gz2[i] = g[3];
}
__global__ __launch_bounds__(256) void pz_final_kernel(const PzFinal a) {
    __shared__ double sh[256];
    double q[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < a.M; i += 256) {
        const double* A = a.rowA + (long)i * 8;
        const double* C = a.rowC + (long)i * 12;
        double g[4];
        pz_row_grad(a, i, g);
        q[0] += A[0]; q[1] += A[1]; q[2] += A[2]; q[3] += A[3]; q[4] += A[4]; q[5] += A[5];
        q[6] += C[4]; q[7] += C[5]; q[8] += g[0]; q[9] += g[1]; q[10] += A[6];
    }
    double t[11];
    for (int k = 0; k < 11; ++k) t[k] = pz_block_sum(q[k], sh);
    if (threadIdx.x != 0) return;
    const double s = a.s, v = a.v, N = a.N, s2 = s * s;
    const double trKP = s2 * t[0], trSP = s2 * t[1], ldK = 2.0 * t[2], ldS = 2.0 * t[3], aPa = s2 * t[4], ca = t[10];
    const double elbo = -0.5 * (N * log(2.0 * M_PI * v) + ldS - ldK + a.yy / v - ca / (v * v)) - (N * s - trKP) / (2.0 * v);
    const double gv = -N / (2.0 * v) + trSP / (2.0 * v * v) + a.yy / (2.0 * v * v) - ca / (v * v * v) + aPa / (2.0 * v * v * v * v) +
                      (N * s - trKP) / (2.0 * v * v);
    const double gs = t[6] + 2.0 * s * t[7] + t[5] / (v * v) - N / (2.0 * v);
    a.out[0] = elbo; a.out[1] = t[8]; a.out[2] = t[9]; a.out[3] = gs * a.s2; a.out[4] = gs * a.s1; a.out[5] = gv;
}

// read-outs (the mean: pz_mean_kernel, gen_gemm.h): var[p] = prior + s^2 vsum[p]
__global__ void pz_var_kernel(const double* vsum, const double* kd1, const double* kd2, int mv2, long n, double s, double* var) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const double prior = kd1 ? s * kd1[p / mv2] * kd2[p % mv2] : s;
    var[p] = prior + s * s * vsum[p];
}
__global__ __launch_bounds__(256) void pz_rowdot2_kernel(const double* X, const double* Y, int M, double* out) {   // out[i] = sum_j X_ij Y_ij
    __shared__ double sh[256];
    const long o = (long)blockIdx.x * M;
    double acc = 0.0;
    for (int j = threadIdx.x; j < M; j += 256) acc += X[o + j] * Y[o + j];
    acc = pz_block_sum(acc, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = acc;
}
// posterior_cov: B*[i][p] explicitly (dense ns x ns output anyway) and the prior part
__global__ void pz_bstar_kernel(const PzPts g, int M, long ns, double* Bs) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)M * ns) return;
    const int i = (int)(idx / ns);
    Bs[idx] = g.val(i, (int)(idx - (long)i * ns));
}
__global__ void pz_prior_kernel(const double* xs1, const double* xs2, long ns, int kind1, int kind2, double inv1, double inv2, double s,
                                double w, double* cov) {     // cov = w cov + s k1 k2
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ns * ns) return;
    const long p = idx / ns, q = idx - p * ns;
    double k1, k2, d;
    vg_kappa(kind1, fabs(xs1[p] - xs1[q]), inv1, k1, d);
    vg_kappa(kind2, fabs(xs2[p] - xs2[q]), inv2, k2, d);
    cov[idx] = w * cov[idx] + s * k1 * k2;
}

// ---- workspace -------------------------------------------------------------------------------------------------------------
struct VgPaired {
    long M = 0, n1 = 0, n2 = 0, N = 0;       // scattered: n1 = n2 = N points; grid: N = n1 n2
    bool scattered = false;
    int nblk = 0, ns1 = 1, runs2 = 1, tn_per2 = 1, gsplit[2] = {1, 1};   // runs2 x tn_per2: pass 2's column tiles
    double *z1, *z2, *x1, *x2;
    double *K0, *P0, *S, *Lk, *Xk, *Kinv, *Ls, *Xs, *Sinv, *KP, *KPK, *Pb;   // M x M
    double *G[6];                                                            // grid: G1, H1, Z1, G2, H2, Z2
    double *A[6];                                                            // grid: A1, dA1, zA1 (M x n1), A2, dA2, zA2 (M x n2)
    double *T, *U, *gslab;                                                   // grid: A1 Y^T, A2 Y, split-K slabs of the Grams
    double *slab1, *bpart, *part2;                                           // scattered: pass-1 slabs, pass-2 row partials
    double *DI, *Tmp, *cholscratch, *jit;
    int* status;                                                             // [0] Kuu, [1] Sigma
    double *b, *alpha, *Pa, *wv, *gz1, *gz2, *rowA, *rowC, *rowD, *out;
    void* mem = nullptr;
    // state of the last step
    bool have_step = false;
    const double* step_y = nullptr;
    double theta[5] = {0, 0, 0, 0, 0}, eps = 0.0;
};

static void pz_layout(VgPaired& w, VgArena& a) {
    const size_t M = w.M, MM = M * M, n1 = w.n1, n2 = w.n2;
    w.z1 = a.take(M); w.z2 = a.take(M); w.x1 = a.take(n1); w.x2 = a.take(n2);
    w.K0 = a.take(MM); w.P0 = a.take(MM); w.S = a.take(MM); w.Lk = a.take(MM); w.Xk = a.take(MM); w.Kinv = a.take(MM);
    w.Ls = a.take(MM); w.Xs = a.take(MM); w.Sinv = a.take(MM); w.KP = a.take(MM); w.KPK = a.take(MM); w.Pb = a.take(MM);
    for (int k = 0; k < 6; ++k) { w.G[k] = nullptr; w.A[k] = nullptr; }
    w.T = w.U = w.gslab = w.slab1 = w.bpart = w.part2 = nullptr;
    if (w.scattered) {
        w.slab1 = w.ns1 > 1 ? a.take((size_t)w.ns1 * MM) : nullptr;
        w.bpart = w.ns1 > 1 ? a.take((size_t)w.ns1 * M) : nullptr;
        w.part2 = a.take((size_t)w.runs2 * M * 4);               // per run of column tiles: O(M), not O(M N)
    } else {
        for (int k = 0; k < 6; ++k) w.G[k] = a.take(MM);
        for (int k = 0; k < 6; ++k) w.A[k] = a.take(M * (k < 3 ? n1 : n2));
        w.T = a.take(M * n2); w.U = a.take(M * n1);
        const int gs = std::max(w.gsplit[0], w.gsplit[1]);
        w.gslab = gs > 1 ? a.take((size_t)gs * 3 * MM) : nullptr;
    }
    w.DI = a.take((size_t)w.nblk * PZ_MB * PZ_MB); w.Tmp = a.take((size_t)PZ_MB * M);
    w.cholscratch = a.take(PZ_MB * (PZ_MB + 1)); w.jit = a.take(8);
    w.status = reinterpret_cast<int*>(a.take(8));
    w.b = a.take(M); w.alpha = a.take(M); w.Pa = a.take(M); w.wv = a.take(M); w.gz1 = a.take(M); w.gz2 = a.take(M);
    w.rowA = a.take(M * 8); w.rowC = a.take(M * 12); w.rowD = a.take(M * 8); w.out = a.take(8);
}

void vg_paired_free(vggp_ctx* c) {
    VgPaired* w = reinterpret_cast<VgPaired*>(c->paired);
    if (!w) return;
    if (w->mem) (void)hipFree(w->mem);
    delete w;
    c->paired = nullptr;
}

static VgPaired* pz_ws(vggp_ctx* c) { return reinterpret_cast<VgPaired*>(c->paired); }

// Split of the point sum of pass 1: enough workgroups to fill the GPU when the M x M triangle has few tiles.
static int pz_pass1_split(long M, long N) {
    const long tn = (M + PZ_T - 1) / PZ_T, tiles = tn * (tn + 1) / 2;
    long s = (1024 + tiles - 1) / tiles;
    s = std::min(s, std::max(1L, N / (PZ_BK * 32)));
    return (int)std::max(1L, std::min(s, 128L));
}
static int pz_gram_split(long M, long n) {
    const long t = (M + 63) / 64;
    long s = (1024 + 3 * t * t - 1) / (3 * t * t);
    s = std::min(s, std::max(1L, n / 256));
    return (int)std::max(1L, std::min(s, 16L));
}

// Everything a paired plan can refuse for its arguments, before the context is touched: a refused plan leaves the previous one usable.
int vg_paired_check(const vggp_desc* desc) {
    const long M = desc->m1;
    VG_REQUIRE(desc->m1 == desc->m2, "vggp_plan: VGGP_FLAG_PAIRED_Z needs m1 == m2 == M (one coordinate pair per inducing point)");
    VG_REQUIRE(M >= 1 && M <= PZ_MAX_M, "vggp_plan: paired inducing points: M = %ld outside [1, %d]", M, PZ_MAX_M);
    VG_REQUIRE(desc->basis1 == VGGP_BASIS_POINTS && desc->basis2 == VGGP_BASIS_POINTS,
               "vggp_plan: VGGP_FLAG_PAIRED_Z needs VGGP_BASIS_POINTS in both dimensions");
    VG_REQUIRE(desc->kind1 >= 0 && desc->kind1 <= 3 && desc->kind2 >= 0 && desc->kind2 <= 3, "vggp_plan: bad kind");
    VG_REQUIRE(desc->x1 && desc->x2 && desc->grid1 && desc->grid2, "vggp_plan: null coordinate arrays");
    VG_REQUIRE(desc->n1 >= 1 && desc->n2 >= 1, "vggp_plan: no observations");
    if (desc->flags & VGGP_FLAG_SCATTERED) {
        VG_REQUIRE(desc->n1 == desc->n2, "vggp_plan: scattered points need n1 == n2 (one coordinate pair per point)");
        VG_REQUIRE(desc->n1 < (1L << 30), "vggp_plan: too many scattered points");
    } else {
        VG_REQUIRE(desc->n1 < (1L << 24) && desc->n2 < (1L << 24) && M * desc->n1 < (1L << 34) && M * desc->n2 < (1L << 34),
                   "vggp_plan: grid too large for the paired inducing points");
    }
    for (long i = 0; i < M; ++i)
        VG_REQUIRE(std::isfinite(desc->grid1[i]) && std::isfinite(desc->grid2[i]), "vggp_plan: inducing point %ld is not finite", i);
    for (long i = 0; i < desc->n1; ++i)
        VG_REQUIRE(std::isfinite(desc->x1[i]), "vggp_plan: observation coordinate x1[%ld] is not finite", i);
    for (long i = 0; i < desc->n2; ++i)
        VG_REQUIRE(std::isfinite(desc->x2[i]), "vggp_plan: observation coordinate x2[%ld] is not finite", i);
    return VGGP_OK;
}

// (desc has passed vg_paired_check)
int vg_paired_plan(vggp_ctx* c, const vggp_desc* desc) {
    const long M = desc->m1;
    VgPaired tmp;
    tmp.M = M; tmp.n1 = desc->n1; tmp.n2 = desc->n2;
    tmp.scattered = (desc->flags & VGGP_FLAG_SCATTERED) != 0;
    if (tmp.scattered) {
        tmp.N = desc->n1;
        tmp.ns1 = pz_pass1_split(M, tmp.N);
        {   // pass 2: about 8192 workgroups, each summing a run of column tiles in order (partials <= 8192 x 256 doubles + 4 M: not O(N))
            const long tiles_m = (M + PZ_T - 1) / PZ_T, tiles_n = (tmp.N + PZ_T - 1) / PZ_T;
            const long runs = std::max(1L, std::min(tiles_n, 8192 / tiles_m));
            tmp.tn_per2 = (int)((tiles_n + runs - 1) / runs);
            tmp.runs2 = (int)((tiles_n + tmp.tn_per2 - 1) / tmp.tn_per2);
        }
    } else {
        tmp.N = desc->n1 * desc->n2;
        tmp.gsplit[0] = pz_gram_split(M, desc->n1);
        tmp.gsplit[1] = pz_gram_split(M, desc->n2);
    }
    tmp.nblk = (int)((M + PZ_MB - 1) / PZ_MB);
    const size_t bytes = vg_arena_measure([&](VgArena& a) { pz_layout(tmp, a); });
    size_t free_b = 0;
    if (!vg_arena_fits(bytes, &free_b)) {      // (asked while the old workspace is still there)
        vg_set_error("vggp_plan: the paired inducing points (M = %ld) need %.1f GiB of workspace, %.1f GiB are free", M,
                     (double)bytes / 1073741824.0, (double)free_b / 1073741824.0);
        return VGGP_ENOMEM;
    }
    vg_paired_free(c);
    VgPaired* w = new VgPaired(tmp);
    w->mem = nullptr;
    c->paired = w;                       // owned by the context from here on (vg_paired_free releases it on any later failure)
    int rc;
    if ((rc = vg_arena_alloc(&w->mem, bytes, [&](VgArena& a) { pz_layout(*w, a); }))) return rc;
    VG_HIP(hipMemcpy(w->z1, desc->grid1, sizeof(double) * M, hipMemcpyHostToDevice));
    VG_HIP(hipMemcpy(w->z2, desc->grid2, sizeof(double) * M, hipMemcpyHostToDevice));
    VG_HIP(hipMemcpy(w->x1, desc->x1, sizeof(double) * w->n1, hipMemcpyHostToDevice));
    VG_HIP(hipMemcpy(w->x2, desc->x2, sizeof(double) * w->n2, hipMemcpyHostToDevice));
    c->arena_used = bytes;
    return VGGP_OK;
}

int vg_paired_set_inducing(vggp_ctx* c, int dim, const double* z, int64_t m) {
    VgPaired* w = pz_ws(c);
    VG_REQUIRE(dim == 0 || dim == 1, "vggp_set_inducing: dim must be 0 or 1");
    VG_REQUIRE(z && m == w->M, "vggp_set_inducing: expected %ld coordinates, got %lld", w->M, (long long)m);
    for (int64_t i = 0; i < m; ++i) VG_REQUIRE(std::isfinite(z[i]), "vggp_set_inducing: z[%lld] is not finite", (long long)i);
    // one blocking copy on the null stream: ordered after the work of every blocking stream (the context's own one and torch's
    // default stream), so no step still reads the old coordinates; no further synchronisation
    VG_HIP(hipMemcpy(dim == 0 ? w->z1 : w->z2, z, sizeof(double) * m, hipMemcpyHostToDevice));
    w->have_step = false;
    return VGGP_OK;
}

static int pz_gemm(const double* A, long sa_m, long sa_k, const double* B, long sb_k, long sb_n, double* C, int ldc, int M, int N, int K,
                   hipStream_t st, double alpha = 1.0) {
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, A, sa_m, sa_k, B, sb_k, sb_n, C, ldc, M, N, K, 1, 0, 1, 0, alpha, 0);
    VG_HIP(vg_gemm_launch(&g, st));
    return VGGP_OK;
}

static PzPts pz_pts(const vggp_ctx* c, const VgPaired& w, const double* x1, const double* x2) {
    return PzPts{w.z1, w.z2, x1, x2, c->desc.kind1, c->desc.kind2, 1.0 / w.theta[0], 1.0 / w.theta[1]};
}

// unit-scale P0 = B B^T and b = B y
static int pz_assemble(vggp_ctx* c, VgPaired& w, const double* Y, hipStream_t st) {
    const int M = (int)w.M;
    const double inv1 = 1.0 / w.theta[0], inv2 = 1.0 / w.theta[1];
    int rc;
    if (w.scattered) {
        const PzPts g = pz_pts(c, w, w.x1, w.x2);
        const int N = (int)w.N;
        PzEpSym ep{w.ns1 > 1 ? w.slab1 : w.P0, Y, w.ns1 > 1 ? w.bpart : w.b, w.M};
        VG_HIP((pz_gen_gemm<PZ_EPI_SYM>(PzARow<PzPts>{g}, PzBCol<PzPts>{g}, ep, M, M, N, w.ns1, true, st)));
        if (w.ns1 > 1) {
            VgRedBatch r;
            vg_red_init(&r);
            vg_red_add(&r, w.slab1, w.P0, w.M * w.M, w.M * w.M, w.ns1);
            vg_red_add(&r, w.bpart, w.b, w.M, w.M, w.ns1);
            VG_HIP(vg_red_launch(&r, st));
        }
        return VGGP_OK;
    }
    const long n1 = w.n1, n2 = w.n2;
    PZ_LAUNCH1D(pz_afac_kernel, (long)M * n1, st, w.z1, w.x1, M, n1, c->desc.kind1, inv1, w.A[0], w.A[1], w.A[2]);
    PZ_LAUNCH1D(pz_afac_kernel, (long)M * n2, st, w.z2, w.x2, M, n2, c->desc.kind2, inv2, w.A[3], w.A[4], w.A[5]);
    VG_HIP(hipGetLastError());
    // Grams G_d = A_d A_d^T, H_d = dA_d A_d^T, Z_d = zA_d A_d^T (split over the grid axis when the M x M output has few tiles)
    for (int d = 0; d < 2; ++d) {
        const long n = d == 0 ? n1 : n2;
        const int ks = w.gsplit[d];
        VgGemmBatch g;
        vg_gemm_init(&g);
        int idx[3];
        for (int q = 0; q < 3; ++q) {
            double* C = ks > 1 ? w.gslab + (long)q * M * M : w.G[3 * d + q];
            idx[q] = vg_gemm_add(&g, w.A[3 * d + q], n, 1, w.A[3 * d], 1, n, C, M, M, M, (int)n, ks, ks > 1 ? 3L * M * M : 0);
        }
        VG_HIP(vg_gemm_launch(&g, st));
        if (ks > 1) {
            VgRedBatch r;
            vg_red_init(&r);
            for (int q = 0; q < 3; ++q)
                vg_red_add(&r, w.gslab + (long)q * M * M, w.G[3 * d + q], (long)M * M, 3L * M * M, g.p[idx[q]].ksplit);
            VG_HIP(vg_red_launch(&r, st));
        }
    }
    PZ_LAUNCH1D(pz_hadamard_kernel, (long)M * M, st, w.G[0], w.G[3], (long)M * M, w.P0);
    // the two passes over Y: T = A1 Y^T (M x n2), U = A2 Y (M x n1)
    if ((rc = pz_gemm(w.A[0], n1, 1, Y, 1, n1, w.T, (int)n2, M, (int)n2, (int)n1, st))) return rc;
    if ((rc = pz_gemm(w.A[3], n2, 1, Y, n1, 1, w.U, (int)n1, M, (int)n1, (int)n2, st))) return rc;
    hipLaunchKernelGGL(pz_rowdot_kernel, dim3(M), dim3(256), 0, st, w.T, w.U, w.A[3], w.A[1], w.A[2], w.A[4], w.A[5], n1, n2, w.rowD, w.b);
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}

static int pz_chol(VgPaired& w, double* L, double* X, double* inv, int which, hipStream_t st) {
    VgDenseChol d{w.S, L, X, w.DI, w.Tmp, w.cholscratch, w.jit, w.status + which, w.M, inv};
    return vg_blocked_chol_inverse(d, st);
}

// one step at jitter eps; leaves out[8], gz and the statuses on the device
// assemble = false: a retry at the next jitter level -- K0, P0 and b (and on a full grid the Grams) do not depend on it
static int pz_step_enqueue(vggp_ctx* c, VgPaired& w, const double* Y, double yy, hipStream_t st, bool assemble) {
    const int M = (int)w.M;
    const long MM = w.M * w.M;
    const double s1 = w.theta[2], s2 = w.theta[3], s = s1 * s2, v = w.theta[4];
    const double inv1 = 1.0 / w.theta[0], inv2 = 1.0 / w.theta[1];
    int rc;
    VG_HIP(hipMemsetAsync(w.status, 0, 2 * sizeof(int), st));
    if (assemble) {
        PZ_LAUNCH1D(pz_kuu_kernel, MM, st, w.z1, w.z2, M, c->desc.kind1, c->desc.kind2, inv1, inv2, w.K0);
        if ((rc = pz_assemble(c, w, Y, st))) return rc;
    }
    // Kj = s K0 + eps I  ->  Lk, Kinv ;  Sigma = Kj + (s^2 / v) P0  ->  Ls, Sinv
    PZ_LAUNCH1D(pz_fill_kernel, MM, st, w.K0, (const double*)nullptr, M, s, w.eps, 0.0, w.S);
    if ((rc = pz_chol(w, w.Lk, w.Xk, w.Kinv, 0, st))) return rc;
    PZ_LAUNCH1D(pz_fill_kernel, MM, st, w.K0, w.P0, M, s, w.eps, s * s / v, w.S);
    if ((rc = pz_chol(w, w.Ls, w.Xs, w.Sinv, 1, st))) return rc;
    // wv = Ls^-1 (s b) (c^T Sigma^-1 c = |wv|^2 without the explicit Sigma^-1), alpha = Ls^-T wv, P0 alpha, Kinv P0 Kinv
    if ((rc = pz_gemm(w.Xs, M, 1, w.b, 1, 1, w.wv, 1, M, 1, M, st, s))) return rc;
    if ((rc = pz_gemm(w.Xs, 1, M, w.wv, 1, 1, w.alpha, 1, M, 1, M, st))) return rc;
    if ((rc = pz_gemm(w.P0, M, 1, w.alpha, 1, 1, w.Pa, 1, M, 1, M, st))) return rc;
    if ((rc = pz_gemm(w.Kinv, M, 1, w.P0, M, 1, w.KP, M, M, M, M, st))) return rc;
    if ((rc = pz_gemm(w.KP, M, 1, w.Kinv, M, 1, w.KPK, M, M, M, M, st))) return rc;
    hipLaunchKernelGGL(pz_rowa_kernel, dim3(M), dim3(256), 0, st, w.Kinv, w.Sinv, w.P0, w.Lk, w.Ls, w.alpha, w.Pa, w.b, w.wv, M, w.rowA);
    PZ_LAUNCH1D(pz_phib_kernel, MM, st, w.Kinv, w.Sinv, w.alpha, M, v, w.Pb);
    PzRowC rc_{w.Kinv, w.Sinv, w.KPK, w.Pb, w.P0, w.alpha, w.z1, w.z2,
               w.G[0], w.G[1], w.G[2], w.G[3], w.G[4], w.G[5], M, c->desc.kind1, c->desc.kind2, inv1, inv2, v, s * s / v, w.rowC};
    hipLaunchKernelGGL(pz_rowc_kernel, dim3(M), dim3(256), 0, st, rc_);
    VG_HIP(hipGetLastError());
    if (w.scattered) {
        // pass 2: R = Pb B (K = M inducing points), contracted in the epilogue against dB; cb = alpha / v^2 goes into Pa (free now)
        PZ_LAUNCH1D(pz_scale_kernel, M, st, w.alpha, (long)M, 1.0 / (v * v), w.Pa);
        const PzPts g = pz_pts(c, w, w.x1, w.x2);
        PzEpGrad ep{g, Y, w.Pa, 2.0 * s, w.part2, w.M};
        // (skipped on the device when Kuu failed at this jitter level: the retry pays the M-space work, not the O(M^2 N) pass)
        VG_HIP((pz_gen_gemm<PZ_EPI_ROW4>(PzAMat{w.Pb, w.M}, PzBRow<PzPts>{g}, ep, M, (int)w.N, M, 1, false, st, w.tn_per2, w.status)));
        VgRedBatch r;
        vg_red_init(&r);
        vg_red_add(&r, w.part2, w.rowD, 4 * w.M, 4 * w.M, w.runs2);
        VG_HIP(vg_red_launch(&r, st));
    }
    PzFinal fa{w.rowA, w.rowC, w.rowD, w.alpha, M, w.scattered ? 0 : 1, (double)c->desc.n_total, yy, s, v, s1, s2, w.out, w.gz1, w.gz2};
    hipLaunchKernelGGL(pz_final_kernel, dim3(1), dim3(256), 0, st, fa);
    hipLaunchKernelGGL(pz_gz_kernel, dim3((M + 255) / 256), dim3(256), 0, st, fa);
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}

int vg_paired_step(vggp_ctx* c, const double* Y, double yy, const double theta[5], double* elbo_out, double grad_out[5],
                   vggp_info* info, hipStream_t st, bool scattered_entry) {
    VgPaired& w = *pz_ws(c);
    const char* fn = scattered_entry ? "vggp_elbo_step_scattered" : "vggp_elbo_step";
    VG_REQUIRE(Y && theta && elbo_out && grad_out, "%s: null argument", fn);
    VG_REQUIRE(w.scattered == scattered_entry, "%s: the paired context was planned %s VGGP_FLAG_SCATTERED", fn,
               w.scattered ? "with" : "without");
    VG_REQUIRE(c->n_ranks == 1 && !c->comm && !c->cb, "%s: paired inducing points (VGGP_FLAG_PAIRED_Z) are single-rank only", fn);
    // (all five checked before any is stored: a refused theta leaves the state of the last step, which the read-outs scale by w.theta)
    for (int i = 0; i < 5; ++i)
        VG_REQUIRE(theta[i] > 0.0 && std::isfinite(theta[i]), "theta[%d]=%g must be positive and finite", i, theta[i]);
    for (int i = 0; i < 5; ++i) w.theta[i] = theta[i];
    w.have_step = false;
    int st_k = 0, st_s = 0;
    // (a jitter level is retried only when Kuu itself failed)
    const int rcj = pz_jitter_retry(&w.eps, &st_k, [&](bool first) {
        int rc = pz_step_enqueue(c, w, Y, yy, st, first);
        if (rc) return rc;
        VG_HIP(hipMemcpyAsync(c->h_out->out, w.out, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
        VG_HIP(hipMemcpyAsync(c->h_out->status, w.status, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        VG_HIP(hipStreamSynchronize(st));                           // the one host synchronisation of the step
        st_s = c->h_out->status[1];
        return c->h_out->status[0] ? 1 : 0;
    });
    if (rcj < 0) return rcj;
    if (st_k) st_k = c->h_out->status[0];
    if (info) {
        info->jitter1 = st_k ? -1.0 : w.eps; info->jitter2 = 0.0;
        info->sweeps1 = info->sweeps2 = info->rounds1 = info->rounds2 = 0;
        info->status = st_k ? st_k : st_s; info->polished = 0;
    }
    if (st_k) { vg_set_error("%s: Kuu is not positive definite after jitter 1e-6", fn); return VGGP_ENOTPD; }
    if (st_s) { vg_set_error("%s: Sigma = Kuu + Phi / sigma^2 is not positive definite", fn); return VGGP_ENOTPD; }
    *elbo_out = c->h_out->out[0];
    for (int i = 0; i < 5; ++i) grad_out[i] = c->h_out->out[1 + i];
    w.have_step = true;
    w.step_y = Y;
    return VGGP_OK;
}

int vg_paired_zgrad(vggp_ctx* c, const double* Y, double* gz1, double* gz2, hipStream_t st, bool scattered_entry) {
    VgPaired& w = *pz_ws(c);
    const char* fn = scattered_entry ? "vggp_zgrad_scattered" : "vggp_zgrad";
    VG_REQUIRE(gz1 && gz2, "%s: null output", fn);
    VG_REQUIRE(w.scattered == scattered_entry, "%s: the paired context was planned %s VGGP_FLAG_SCATTERED", fn,
               w.scattered ? "with" : "without");
    if (!w.have_step) { vg_set_error("%s: no step on the current inducing points", fn); return VGGP_ESTATE; }
    VG_REQUIRE(Y == w.step_y, "%s: Y is not the array of the last step", fn);
    // (the Z-gradient is a by-product of the step's contraction: copy it out)
    VG_HIP(hipMemcpyAsync(gz1, w.gz1, sizeof(double) * w.M, hipMemcpyDeviceToDevice, st));
    VG_HIP(hipMemcpyAsync(gz2, w.gz2, sizeof(double) * w.M, hipMemcpyDeviceToDevice, st));
    return VGGP_OK;
}

static int pz_need_step(VgPaired& w, const char* fn) {
    if (!w.have_step) { vg_set_error("%s: no step on the current inducing points", fn); return VGGP_ESTATE; }
    return VGGP_OK;
}

// q(u): mean = Kj Sigma^-1 c / v = Kj alpha / v, var = diag(Kj Sigma^-1 Kj)  (S <- Kj, KP <- Kj Sinv: scratch after the step)
int vg_paired_qv(vggp_ctx* c, double* mean, double* var, hipStream_t st) {
    VgPaired& w = *pz_ws(c);
    int rc;
    if ((rc = pz_need_step(w, "vggp_qv_masked"))) return rc;
    VG_REQUIRE(mean && var, "vggp_qv_masked: null output");
    const int M = (int)w.M;
    const double s = w.theta[2] * w.theta[3], v = w.theta[4];
    PZ_LAUNCH1D(pz_fill_kernel, w.M * w.M, st, w.K0, (const double*)nullptr, M, s, w.eps, 0.0, w.S);
    if ((rc = pz_gemm(w.S, M, 1, w.alpha, 1, 1, mean, 1, M, 1, M, st, 1.0 / v))) return rc;
    if ((rc = pz_gemm(w.S, M, 1, w.Sinv, M, 1, w.KP, M, M, M, M, st))) return rc;
    hipLaunchKernelGGL(pz_rowdot2_kernel, dim3(M), dim3(256), 0, st, w.KP, w.S, M, var);
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}

int vg_paired_qv_cov(vggp_ctx* c, double* cov, hipStream_t st) {
    VgPaired& w = *pz_ws(c);
    int rc;
    if ((rc = pz_need_step(w, "vggp_qv_cov_masked"))) return rc;
    VG_REQUIRE(cov, "vggp_qv_cov_masked: null output");
    const int M = (int)w.M;
    const double s = w.theta[2] * w.theta[3];
    PZ_LAUNCH1D(pz_fill_kernel, w.M * w.M, st, w.K0, (const double*)nullptr, M, s, w.eps, 0.0, w.S);
    if ((rc = pz_gemm(w.S, M, 1, w.Sinv, M, 1, w.KP, M, M, M, M, st))) return rc;
    return pz_gemm(w.KP, M, 1, w.S, M, 1, cov, M, M, M, M, st);
}

// Gridded read-out with F = Kvu / s = C1 face-split C2 ([mv1 mv2] x M, never stored):
// mean = (s / v) F alpha, var = s kd1 kd2 + s^2 diag(F Q F^T), Q = S_u^-1 - Kinv (literal) or Sigma^-1 - Kinv (conditional)
int vg_paired_readout(vggp_ctx* c, const double* C1, int64_t mv1, const double* C2, int64_t mv2, const double* kd1, const double* kd2,
                      double* mean, double* var, int flags, hipStream_t st) {
    VgPaired& w = *pz_ws(c);
    int rc;
    if ((rc = pz_need_step(w, "vggp_readout_masked"))) return rc;
    VG_REQUIRE(C1 && C2 && kd1 && kd2 && mean && var && mv1 >= 1 && mv2 >= 1, "vggp_readout_masked: bad argument");
    const long nv = mv1 * mv2;
    VG_REQUIRE(nv < (1L << 30), "vggp_readout_masked: too many cells");
    const int M = (int)w.M;
    const double s = w.theta[2] * w.theta[3], v = w.theta[4];
    const int tiles_m = (M + PZ_T - 1) / PZ_T;
    if ((rc = vg_ensure_misc(c, sizeof(double) * ((size_t)tiles_m * nv + nv + 64)))) return rc;
    double* part = reinterpret_cast<double*>(c->misc);
    double* vsum = part + (size_t)tiles_m * nv;
    PZ_LAUNCH1D(pz_q_kernel, w.M * w.M, st, w.Kinv, w.Sinv, w.KPK, w.M * w.M, s * s / v, (flags & VGGP_READOUT_LITERAL) ? 1 : 0, w.S);
    const PzFace f{C1, C2, (int)mv2, M};
    hipLaunchKernelGGL(pz_mean_kernel<PzFace>, dim3((unsigned)nv), dim3(256), 0, st, f, w.alpha, M, s / v, mean);
    VG_HIP(hipGetLastError());
    VG_HIP((pz_gen_gemm<PZ_EPI_COL1>(PzAMat{w.S, w.M}, PzBRow<PzFace>{f}, PzEpCol<PzFace>{f, part, nv}, M, (int)nv, M, 1, false, st)));
    VgRedBatch r;
    vg_red_init(&r);
    vg_red_add(&r, part, vsum, nv, nv, tiles_m);
    VG_HIP(vg_red_launch(&r, st));
    PZ_LAUNCH1D(pz_var_kernel, nv, st, vsum, kd1, kd2, (int)mv2, nv, s, var);
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}

// posterior(x*): mean = (s / v) B*^T alpha, var = s + s^2 diag(B*^T (Sigma^-1 - Kinv) B*)
int vg_paired_posterior(vggp_ctx* c, const double* xs1, const double* xs2, int64_t ns, double* mean, double* var, hipStream_t st) {
    VgPaired& w = *pz_ws(c);
    int rc;
    if ((rc = pz_need_step(w, "vggp_posterior_masked"))) return rc;
    VG_REQUIRE(xs1 && xs2 && mean && var && ns >= 0 && ns < (1L << 30), "vggp_posterior_masked: bad argument");
    if (ns == 0) return VGGP_OK;
    const int M = (int)w.M;
    const double s = w.theta[2] * w.theta[3], v = w.theta[4];
    const int tiles_m = (M + PZ_T - 1) / PZ_T;
    if ((rc = vg_ensure_misc(c, sizeof(double) * ((size_t)tiles_m * ns + ns + 64)))) return rc;
    double* part = reinterpret_cast<double*>(c->misc);
    double* vsum = part + (size_t)tiles_m * ns;
    PZ_LAUNCH1D(pz_q_kernel, w.M * w.M, st, w.Kinv, w.Sinv, w.KPK, w.M * w.M, 0.0, 0, w.S);
    const PzPts g = pz_pts(c, w, xs1, xs2);
    hipLaunchKernelGGL(pz_mean_kernel<PzPts>, dim3((unsigned)ns), dim3(256), 0, st, g, w.alpha, M, s / v, mean);
    VG_HIP(hipGetLastError());
    VG_HIP((pz_gen_gemm<PZ_EPI_COL1>(PzAMat{w.S, w.M}, PzBRow<PzPts>{g}, PzEpCol<PzPts>{g, part, (long)ns}, M, (int)ns, M, 1, false, st)));
    VgRedBatch r;
    vg_red_init(&r);
    vg_red_add(&r, part, vsum, ns, ns, tiles_m);
    VG_HIP(vg_red_launch(&r, st));
    PZ_LAUNCH1D(pz_var_kernel, ns, st, vsum, (const double*)nullptr, (const double*)nullptr, 1, (long)ns, s, var);
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}

int vg_paired_posterior_cov(vggp_ctx* c, const double* xs1, const double* xs2, int64_t ns, double* cov, hipStream_t st) {
    VgPaired& w = *pz_ws(c);
    int rc;
    if ((rc = pz_need_step(w, "vggp_posterior_cov_masked"))) return rc;
    VG_REQUIRE(xs1 && xs2 && cov && ns >= 1 && ns <= 8192 && w.M * ns <= (1L << 27), "vggp_posterior_cov_masked: bad argument (ns <= 8192, M ns <= 2^27)");
    const int M = (int)w.M;
    const double s = w.theta[2] * w.theta[3];
    if ((rc = vg_ensure_misc(c, sizeof(double) * (2 * (size_t)M * ns + 64)))) return rc;
    double* Bs = reinterpret_cast<double*>(c->misc);
    double* W = Bs + (size_t)M * ns;
    PZ_LAUNCH1D(pz_q_kernel, w.M * w.M, st, w.Kinv, w.Sinv, w.KPK, w.M * w.M, 0.0, 0, w.S);
    PZ_LAUNCH1D(pz_bstar_kernel, (long)M * ns, st, pz_pts(c, w, xs1, xs2), M, (long)ns, Bs);
    VG_HIP(hipGetLastError());
    if ((rc = pz_gemm(w.S, M, 1, Bs, ns, 1, W, (int)ns, M, (int)ns, M, st))) return rc;                 // W = Q B*
    if ((rc = pz_gemm(Bs, 1, ns, W, ns, 1, cov, (int)ns, (int)ns, (int)ns, M, st))) return rc;          // B*^T W
    PZ_LAUNCH1D(pz_prior_kernel, (long)ns * ns, st, xs1, xs2, (long)ns, c->desc.kind1, c->desc.kind2, 1.0 / w.theta[0],
                1.0 / w.theta[1], s, s * s, cov);
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}
