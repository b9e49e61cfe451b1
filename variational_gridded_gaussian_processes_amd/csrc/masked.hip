// Masked / partially observed grids (BASELINE config 5): only the grid points with W[j][i] = 1 are observed, which
// is how the reference sees scattered data (it simply receives the subset as X, y and runs the dense algebra of
// kronecker_structure.py:249-278).  Phi = Kuf W Kuf^T is then no Kronecker product, so
//     Sigma~ = I + rho Phi~0,   rho = s1 s2 / sigma^2,   Phi~0 = sum_obs (b1_i (x) b2_j)(b1_i (x) b2_j)^T
// is ASSEMBLED in M-space (M = m1 m2) from the per-dimension factors and factored densely.  The N x N / M x N
// matrices of the reference are still never formed.  Specification: oracle/kron.py elbo_step_masked().
//
//   assembly   T[i,(a,b)] = sum_j W[j,i] B2[a,j] B2[b,j]                (one GEMM over the mask)
//              R[(i1,k1),(a,b)] = sum_i B1[i1,i] B1[k1,i] T[i,(a,b)]    (one GEMM)  -> permuted into Sigma~
//              (the same two GEMMs with V in place of one B give the two derivative matrices Phi~'_1, Phi~'_2)
//   factor     blocked right-looking Cholesky with 128-wide panels: diagonal blocks by the register-resident
//              single-workgroup kernel (chol.hip), panels and trailing updates by the MFMA GEMM; then the blocked
//              inverse of the factor and Sigma~^{-1} = L^{-T} L^{-1} by GEMM
//   gradient   analytic, from Sigma~^{-1}, its partial traces, <Sigma~^{-1}, Phi~'_d> and three n2 x n1 products.
#include "arena.h"
#include "block_pcg.h"
#include "ctx.h"
#include "lanczos_quad.h"

#include <algorithm>

#define VG_MB 128                 // panel width of the blocked Cholesky
#define VG_MD_NPART 256           // partial sums per reduction job
#define VG_MD_MAXJOBS 24

// ---- small kernels -------------------------------------------------------------------------------------------------
__global__ void vgm_pairprod_kernel(const double* Xa, const double* Xb, int ma, int mb, long n, double* out) {
    // out[(a*mb + b)][j] = Xa[a][j] * Xb[b][j]
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)ma * mb * n) return;
    const long ab = idx / n, j = idx - ab * n;
    const int a = (int)(ab / mb), b = (int)(ab - (long)a * mb);
    out[idx] = Xa[a * n + j] * Xb[b * n + j];
}

// R[(i1*m1+k1)][(i2*m2+k2)] -> out[(i1*m2+i2)][(k1*m2+k2)] ; mode 1: out = I + rho R (rho = s1 s2 / v from theta)
__global__ void vgm_permute_kernel(const double* R, int m1, int m2, const double* theta, int mode, double* out) {
    const long M = (long)m1 * m2;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * M) return;
    const long row = idx / M, col = idx - row * M;
    const int i1 = (int)(row / m2), i2 = (int)(row - (long)i1 * m2);
    const int k1 = (int)(col / m2), k2 = (int)(col - (long)k1 * m2);
    const double r = R[((long)i1 * m1 + k1) * ((long)m2 * m2) + ((long)i2 * m2 + k2)];
    if (mode == 1) {
        const double rho = theta[2] * theta[3] / theta[4];
        out[idx] = (row == col ? 1.0 : 0.0) + rho * r;
    } else {
        out[idx] = r;
    }
}

// out[j] = sum_a Xa[a][j] * Xb[a][j]   (column dot products, X is [m][n])
__global__ void vgm_coldot_kernel(const double* Xa, const double* Xb, int m, long n, double* out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int a = 0; a < m; ++a) s += Xa[a * n + j] * Xb[a * n + j];
    out[j] = s;
}

// wcol[i] = sum_j W[j][i] v[j]  (n1 outputs) ; wrow[j] = sum_i W[j][i] u[i]  (n2 outputs)
// two stages (row slabs, then a deterministic sum over the slabs): a single pass with one thread per column is 8 workgroups
// walking 2048 rows each -- 0.5 ms of pure latency at n = 2048
__global__ void vgm_wcol_part_kernel(const double* W, const double* v, long n1, long n2, int nslab, double* part) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n1) return;
    const long per = (n2 + nslab - 1) / nslab, j0 = blockIdx.y * per, j1 = j0 + per < n2 ? j0 + per : n2;
    double s = 0.0;
    for (long j = j0; j < j1; ++j) s += W[j * n1 + i] * v[j];
    part[(long)blockIdx.y * n1 + i] = s;
}
__global__ void vgm_wcol_sum_kernel(const double* part, long n1, int nslab, double* wcol) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n1) return;
    double s = 0.0;
    for (int k = 0; k < nslab; ++k) s += part[(long)k * n1 + i];
    wcol[i] = s;
}
__global__ __launch_bounds__(256) void vgm_wrow_kernel(const double* W, const double* u, long n1, long n2, double* wrow) {
    __shared__ double red[4];
    const long j = blockIdx.x;
    double s = 0.0;
    for (long i = threadIdx.x; i < n1; i += 256) s += W[j * n1 + i] * u[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) wrow[j] = red[0] + red[1] + red[2] + red[3];
}

// Xs[a][j] = X[a][j] * w[j]
__global__ void vgm_scalecols_kernel(const double* X, const double* w, int m, long n, double* Xs) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)m * n) return;
    Xs[idx] = X[idx] * w[idx % n];
}

// partial traces of the M x M matrix S (M = m1 m2): which = 1: out[a][b] = sum_j S[(a,j)][(b,j)]  (m1 x m1)
//                                                   which = 2: out[a][b] = sum_i S[(i,a)][(i,b)]  (m2 x m2)
__global__ void vgm_ptrace_kernel(const double* S, int m1, int m2, int which, double* out) {
    const long M = (long)m1 * m2;
    const int md = which == 1 ? m1 : m2;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)md * md) return;
    const int a = (int)(idx / md), b = (int)(idx - (long)a * md);
    double s = 0.0;
    if (which == 1) for (int j = 0; j < m2; ++j) s += S[((long)a * m2 + j) * M + ((long)b * m2 + j)];
    else            for (int i = 0; i < m1; ++i) s += S[((long)i * m2 + a) * M + ((long)i * m2 + b)];
    out[idx] = s;
}

// generic reductions, VG_MD_NPART partial sums per job:
//   op 0: sum a[i*sa] * b[i*sb]     op 1: sum log(a[i*sa])     op 2: sum a[i*sa]     op 3: sum a[i] * b[i] * c[i]
struct VgmRedJob { const double* a; const double* b; const double* c; long n, sa, sb; int op; };
struct VgmRedArgs { VgmRedJob job[VG_MD_MAXJOBS]; int njobs; double* partial; };
__global__ __launch_bounds__(256) void vgm_red_kernel(const VgmRedArgs A) {
    __shared__ double red[4];
    const VgmRedJob& J = A.job[blockIdx.y];
    double s = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < J.n; i += (long)VG_MD_NPART * 256) {
        if (J.op == 0) s += J.a[i * J.sa] * J.b[i * J.sb];
        else if (J.op == 1) s += log(J.a[i * J.sa]);
        else if (J.op == 2) s += J.a[i * J.sa];
        else s += J.a[i] * J.b[i] * J.c[i];
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) A.partial[blockIdx.y * VG_MD_NPART + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// job indices of the masked step (order of the partial-sum buffer)
enum { RJ_LOGDET = 0, RJ_Q, RJ_AA, RJ_TRS, RJ_TRPHI, RJ_MK1PTS, RJ_TRMK1, RJ_SPHI1, RJ_AC1, RJ_MKA1, RJ_Z1, RJ_HV1, RJ_MK1PT,
       RJ_MK2PTS, RJ_TRMK2, RJ_SPHI2, RJ_AC2, RJ_MKA2, RJ_Z2, RJ_HV2, RJ_MK2PT, RJ_COUNT };

// partial[job][VG_MD_NPART] -> scal[job].  Row-sharded step: the sums over this rank's grid rows (local_mask bit set) add up
// over the ranks; every other scalar is computed identically on every rank from all-reduced inputs, so only rank 0
// contributes it to the second (tiny) all-reduce -- exact, and all ranks end up with identical scalars.
__global__ void vgm_sum_kernel(const double* partial, double* scal, unsigned local_mask, int keep_replicated) {
    const int j = threadIdx.x;
    if (j >= RJ_COUNT) return;
    double s = 0.0;
    for (int k = 0; k < VG_MD_NPART; ++k) s += partial[j * VG_MD_NPART + k];
    scal[j] = (((local_mask >> j) & 1u) || keep_replicated) ? s : 0.0;
}

struct VgmFinalArgs { const double* theta; const double* scal; double* out; double N, yy; int m1, m2; };
__global__ void vgm_final_kernel(const VgmFinalArgs A) {
    __shared__ double S[RJ_COUNT];
    if (threadIdx.x < RJ_COUNT) S[threadIdx.x] = A.scal[threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double s1 = A.theta[2], s2 = A.theta[3], v = A.theta[4], N = A.N, yy = A.yy;
    const double M = (double)A.m1 * A.m2, rho = s1 * s2 / v, ss = s1 * s2;
    const double logdet = 2.0 * S[RJ_LOGDET], q = S[RJ_Q], aa = S[RJ_AA], trS = S[RJ_TRS], trPhi = S[RJ_TRPHI];
    const double elbo = -0.5 * (N * 1.8378770664093453 + N * log(v) + logdet + yy / v - (ss / (v * v)) * q)
                        - (N * ss - ss * trPhi) / (2.0 * v);
    const double trSP = (M - trS) / rho, aPa = (q - aa) / rho;
    const double common = -0.5 * (rho * trSP - (ss / (v * v)) * q + (ss / (v * v)) * rho * aPa);
    const double g_s1 = common / s1 - (N * s2 - s2 * trPhi) / (2.0 * v);
    const double g_s2 = common / s2 - (N * s1 - s1 * trPhi) / (2.0 * v);
    const double g_v = -0.5 * (N / v - (rho / v) * trSP - yy / (v * v) + 2.0 * ss * q / (v * v * v) - (ss * rho / (v * v * v)) * aPa)
                       + (N * ss - ss * trPhi) / (2.0 * v * v);
    const double ld1 = S[RJ_MK1PTS] - (double)A.m2 * S[RJ_TRMK1] + 2.0 * rho * S[RJ_SPHI1];
    const double quad1 = 2.0 * S[RJ_AC1] - S[RJ_MKA1] - 2.0 * rho * S[RJ_Z1];
    const double g_l1 = -0.5 * (ld1 - (ss / (v * v)) * quad1) + (ss / (2.0 * v)) * (2.0 * S[RJ_HV1] - S[RJ_MK1PT]);
    const double ld2 = S[RJ_MK2PTS] - (double)A.m1 * S[RJ_TRMK2] + 2.0 * rho * S[RJ_SPHI2];
    const double quad2 = 2.0 * S[RJ_AC2] - S[RJ_MKA2] - 2.0 * rho * S[RJ_Z2];
    const double g_l2 = -0.5 * (ld2 - (ss / (v * v)) * quad2) + (ss / (2.0 * v)) * (2.0 * S[RJ_HV2] - S[RJ_MK2PT]);
    A.out[0] = elbo; A.out[1] = g_l1; A.out[2] = g_l2; A.out[3] = g_s1; A.out[4] = g_s2; A.out[5] = g_v;
}

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
__global__ void vgm_scale_rho_kernel(double* x, long n, const double* theta, int e1, int e2) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= (e1 > 0 ? theta[2] : 1.0) * (e2 > 0 ? theta[3] : 1.0) / theta[4];      // s_d^((1 + e_d) / 2) / sigma^2
}

#define VGM_MAX_M 16384      // dense M x M solver: ~10 M^2 doubles of workspace (21 GB at the limit), O(M^3) per step
#define VGM_LAUNCH1D(kern, n, st, ...) \
    hipLaunchKernelGGL(kern, dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, st, __VA_ARGS__)

// ---- masked workspace ------------------------------------------------------------------------------------------------
struct VgMasked {
    long M = 0, n1 = 0, n2 = 0;
    int m1 = 0, m2 = 0, nblk = 0;
    bool scattered = false;        // n1 == n2 == number of points: the [n2][n1] grid buffers shrink to per-point vectors
    bool iter = false;             // iterative step (vggp_elbo_step_masked_iter): none of the M x M / pair-product buffers exist
    void* imem = nullptr;          // its own workspace (VgIter, below)
    size_t ibytes = 0;
    void* rmem = nullptr;          // workspace of the iterative step's read-outs (VgReadout, below): apart from imem, so that a read-out
    size_t rbytes = 0;             // leaves the kept preconditioner basis and everything else of the step where it is
    // the iterative step's kept preconditioner basis: valid, steps since the cold solve, PCG iterations right after it / last step
    bool ib_valid = false, ib_fresh = false;
    int ib_age = 0, ib_ref_its = 0, ib_last_its = 0, ib_nbc = 0, ib_maxit = 0;
    double *Sg, *Lg, *Xg, *Sinv, *R, *Phip, *DI, *Tmp;          // M x M (Phip: two of them; Tmp: 128 x M)
    double *PP1, *PP1v, *PP2, *PP2v, *T, *Tv;
    double *UB, *UV, *Zb, *Zv1, *Zv2, *B1s, *B2s;
    double *nb1, *nb2, *hv1, *hv2, *wn1, *wn2, *PT1, *PT2, *PTS1, *PTS2, *MkA1, *MkA2, *a0, *partial, *out;
    double *cholscratch, *choljit;
    int* cholstatus;
    // the all-reduce buffer of the row-sharded masked step: [slack 2 m2^2 | C, C1, C2 (3 M) | wn2 (n1) | R3 (3 M^2)];
    // the collective covers everything after the slack (vg_partials_enqueue leaves G2, H2 in it, which this path ignores)
    double *mpay, *R3, *scal;
    void* mem = nullptr;
    size_t bytes = 0;
};

static void vgm_layout(VgMasked& w, VgArena& a) {
    const size_t M = w.M, MM = w.iter ? 0 : M * M, n1 = w.n1, n2 = w.n2, m1 = w.m1, m2 = w.m2;
    const size_t mmax2 = m1 > m2 ? m1 * m1 : m2 * m2;
    if (!w.iter) {
        w.Sg = a.take(MM); w.Lg = a.take(MM); w.Xg = a.take(MM); w.Sinv = a.take(MM); w.R = a.take(MM); w.Phip = a.take(2 * MM);
        w.DI = a.take((size_t)w.nblk * VG_MB * VG_MB); w.Tmp = a.take((size_t)VG_MB * M);
        w.PP1 = a.take(m1 * m1 * n1); w.PP1v = a.take(m1 * m1 * n1); w.PP2 = a.take(m2 * m2 * n2); w.PP2v = a.take(m2 * m2 * n2);
    }
    const size_t grid = w.scattered ? n1 : n1 * n2;            // scattered: zb, zv1, zv2 are per-point vectors
    // T: the assembly's n1 x m2^2 buffer, later slab scratch of the long-K products (scattered / iterative: only the latter)
    w.T = a.take((w.scattered || w.iter) ? std::max<size_t>(256 * mmax2, 64 * n1) : n1 * m2 * m2);
    w.Tv = a.take((w.scattered || w.iter) ? 256 : n1 * m2 * m2);
    w.UB = a.take(m1 * n2); w.UV = a.take(m1 * n2); w.Zb = a.take(grid); w.Zv1 = a.take(grid); w.Zv2 = a.take(grid);
    w.B1s = a.take(m1 * n1); w.B2s = a.take(m2 * n2);
    w.nb1 = a.take(n1); w.nb2 = a.take(n2); w.hv1 = a.take(n1); w.hv2 = a.take(n2); w.wn1 = a.take(n2);
    const size_t wn2len = w.scattered ? 0 : n1;                 // (scattered: the all-reduce payload is C, C1, C2 | R3, the same
    // length on every rank whatever its number of points).  Iterative scattered step: its Gram matrices live in the payload too,
    // G2 in the slack and G1 behind C2 (vgi_g1_offset), so that one collective carries G2 | C0, C1, C2 | G1
    const size_t g1len = (w.iter && w.scattered) ? 32 + m1 * m1 : 0;
    w.mpay = a.take(2 * m2 * m2 + 3 * M + wn2len + 3 * MM + 8 + g1len);
    w.wn2 = a.base ? w.mpay + 2 * m2 * m2 + 3 * M : nullptr;
    w.R3 = a.base ? w.wn2 + wn2len : nullptr;
    w.scal = a.take(32);
    w.PT1 = a.take(m1 * m1); w.PT2 = a.take(m2 * m2); w.PTS1 = a.take(m1 * m1); w.PTS2 = a.take(m2 * m2);
    w.MkA1 = a.take(M); w.MkA2 = a.take(M); w.a0 = a.take(M);
    w.partial = a.take(VG_MD_MAXJOBS * VG_MD_NPART); w.out = a.take(8);
    w.cholscratch = a.take(VG_MB * (VG_MB + 1)); w.choljit = a.take(8);
    w.cholstatus = reinterpret_cast<int*>(a.take(8));
}

// iterative scattered step: G1 sits behind [G2 | . | C0, C1, C2] in w.mpay, on a 256-byte boundary
static size_t vgi_g1_offset(long m1, long m2) { return ((size_t)(2 * m2 * m2 + 3 * m1 * m2) + 31) & ~size_t(31); }

static int vgm_prepare(vggp_ctx* c, bool iter = false) {
    VgMasked* w = reinterpret_cast<VgMasked*>(c->masked);
    if (!w) { w = new VgMasked(); c->masked = w; }
    const long m1 = c->desc.m1, m2 = c->desc.m2;
    const bool sc = (c->desc.flags & VGGP_FLAG_SCATTERED) != 0;
    if (w->mem && w->M == m1 * m2 && w->n1 == c->desc.n1 && w->n2 == c->desc.n2 && w->m1 == m1 && w->scattered == sc && w->iter == iter)
        return VGGP_OK;
    if (w->mem) { VG_HIP(hipFree(w->mem)); w->mem = nullptr; }
    if (w->imem) { VG_HIP(hipFree(w->imem)); w->imem = nullptr; w->ibytes = 0; }
    if (w->rmem) { VG_HIP(hipFree(w->rmem)); w->rmem = nullptr; w->rbytes = 0; }
    w->ib_valid = false;
    w->M = m1 * m2; w->m1 = (int)m1; w->m2 = (int)m2; w->n1 = c->desc.n1; w->n2 = c->desc.n2; w->scattered = sc; w->iter = iter;
    w->nblk = (int)((w->M + VG_MB - 1) / VG_MB);
    const auto lay = [&](VgArena& a) { vgm_layout(*w, a); };
    w->bytes = vg_arena_measure(lay);
    {   // say what does not fit instead of failing inside hipMalloc (the scattered / masked assemblies are not chunked over N)
        size_t free_b = 0;
        if (!vg_arena_fits(w->bytes, &free_b)) {
            vg_set_error("the dense M-space workspace of this %s step needs %.1f GiB (M = %ld, n1 = %ld, n2 = %ld, m1 = %ld, m2 = %ld; "
                         "~10 M^2 + (m1^2 + m2^2) N doubles) but only %.1f GiB of device memory are free%s",
                         sc ? "scattered" : "masked", (double)w->bytes / 1073741824.0, (long)(m1 * m2), (long)c->desc.n1, (long)c->desc.n2,
                         (long)m1, (long)m2, (double)free_b / 1073741824.0,
                         (sc || iter) ? "" : "; vggp_elbo_step_masked_iter needs no M x M matrix");
            w->M = 0;
            return VGGP_ENOMEM;
        }
    }
    return vg_arena_alloc(&w->mem, w->bytes, lay);
}

void vg_masked_new_plan(vggp_ctx* c) {          // vggp_plan: the iterative step's kept preconditioner basis belongs to the old plan
    VgMasked* w = reinterpret_cast<VgMasked*>(c->masked);
    if (w) w->ib_valid = false;
}

void vg_masked_free(vggp_ctx* c) {
    VgMasked* w = reinterpret_cast<VgMasked*>(c->masked);
    if (!w) return;
    if (w->mem) (void)hipFree(w->mem);
    if (w->imem) (void)hipFree(w->imem);
    if (w->rmem) (void)hipFree(w->rmem);
    delete w;
    c->masked = nullptr;
}

static int gemm1(const double* A, long sa_m, long sa_k, const double* B, long sb_k, long sb_n, double* C, int ldc, int M,
                 int N, int K, hipStream_t st, double alpha = 1.0, int accum = 0) {
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, A, sa_m, sa_k, B, sb_k, sb_n, C, ldc, M, N, K, 1, 0, 1, 0, alpha, accum);
    VG_HIP(vg_gemm_launch(&g, st));
    return VGGP_OK;
}

// C (M x N, contiguous) = A B with a SHORT output and a LONG reduction (m x m results summed over 1e5 points): one workgroup per
// tile would walk the whole K alone (5.8 ms at K = 100 000, measured), so the reduction is split over up to 256 workgroups whose
// slabs are summed in fixed order.  scratch: >= 256 * M * N doubles.
static int gemm_longk(const double* A, long sa_m, long sa_k, const double* B, long sb_k, long sb_n, double* C, int M, int N, int K,
                      double* scratch, hipStream_t st) {
    int ks = K / 512;
    if (ks > 256) ks = 256;
    if (ks < 2) return gemm1(A, sa_m, sa_k, B, sb_k, sb_n, C, N, M, N, K, st);
    VgGemmBatch g;
    vg_gemm_init(&g);
    const int ip = vg_gemm_add(&g, A, sa_m, sa_k, B, sb_k, sb_n, scratch, N, M, N, K, ks, (long)M * N);
    const int slabs = g.p[ip].ksplit;
    VG_HIP(vg_gemm_launch(&g, st));
    VgRedBatch r;
    vg_red_init(&r);
    vg_red_add(&r, scratch, C, (long)M * N, (long)M * N, slabs);
    VG_HIP(vg_red_launch(&r, st));
    return VGGP_OK;
}

// S (M x M, SPD, destroyed) -> L (lower), X = L^{-1}, optionally Sinv = S^{-1}.  Blocked right-looking Cholesky with
// VG_MB-wide panels: diagonal blocks by the single-workgroup kernel (chol.hip), panels and trailing updates by the MFMA
// GEMM; then the blocked inverse of the factor.  Shared with vggp_cholesky_inverse for m > 128 (ctx.h).
int vg_blocked_chol_inverse(const VgDenseChol& w, hipStream_t st) {
    const int M = (int)w.M;
    const int nblk = (M + VG_MB - 1) / VG_MB;
    int rc;
    VG_HIP(hipMemsetAsync(w.L, 0, sizeof(double) * w.M * w.M, st));
    VG_HIP(hipMemsetAsync(w.X, 0, sizeof(double) * w.M * w.M, st));
    for (int kb = 0; kb < nblk; ++kb) {
        const int k0 = kb * VG_MB, nbk = std::min(VG_MB, M - k0), rest = M - k0 - nbk;
        VgClearArgs clr;
        clr.n = 1; clr.ptr[0] = reinterpret_cast<int*>(w.scratch); clr.nwords[0] = 16;
        VG_HIP(vg_clear_launch(&clr, st));
        VgCholJob j{w.S + (long)k0 * M + k0, w.L + (long)k0 * M + k0, w.DI + (long)kb * VG_MB * VG_MB, w.scratch, w.jit,
                    w.status, nbk};
        j.ldk = M; j.ldl = M; j.only_level0 = 1;
        VG_HIP(vg_chol_launch(&j, 1, st));
        if (rest > 0) {
            // panel: L[i, kb] = A[i, kb] Linv_kk^T ;  trailing: A[i, j] -= L[i, kb] L[j, kb]^T
            const double* DIk = w.DI + (long)kb * VG_MB * VG_MB;
            if ((rc = gemm1(w.S + (long)(k0 + nbk) * M + k0, M, 1, DIk, 1, nbk, w.L + (long)(k0 + nbk) * M + k0, M, rest, nbk, nbk, st))) return rc;
            // (only the lower triangle of the trailing matrix is read later: column strips that start on the diagonal, one launch)
            const double* Lp = w.L + (long)(k0 + nbk) * M + k0;
            double* St = w.S + (long)(k0 + nbk) * M + (k0 + nbk);
            const int nstrip = std::min(VG_GEMM_MAXP, (rest + 1023) / 1024);
            const int wd = (((rest + nstrip - 1) / nstrip) + VG_MB - 1) / VG_MB * VG_MB;
            VgGemmBatch g;
            vg_gemm_init(&g);
            for (int c0 = 0; c0 < rest; c0 += wd)
                vg_gemm_add(&g, Lp + (long)c0 * M, M, 1, Lp + (long)c0 * M, 1, M, St + (long)c0 * M + c0, M, rest - c0, std::min(wd, rest - c0),
                            nbk, 1, 0, 1, 0, -1.0, 1);
            VG_HIP(vg_gemm_launch(&g, st));
        }
    }
    // blocked inverse of the lower factor: X[k,k] = inv(L_kk); X[i, :i] = -inv(L_ii) (L[i, :i] X[:i, :i])
    for (int kb = 0; kb < nblk; ++kb) {
        const int k0 = kb * VG_MB, nbk = std::min(VG_MB, M - k0);
        VG_HIP(hipMemcpy2DAsync(w.X + (long)k0 * M + k0, sizeof(double) * M, w.DI + (long)kb * VG_MB * VG_MB, sizeof(double) * nbk,
                                sizeof(double) * nbk, nbk, hipMemcpyDeviceToDevice, st));
        if (kb == 0) continue;
        {   // (X[:k0, :k0] is lower triangular: the tiles skip the k-range above their columns)
            VgGemmBatch g;
            vg_gemm_init(&g);
            const int i = vg_gemm_add(&g, w.L + (long)k0 * M, M, 1, w.X, M, 1, w.Tmp, k0, nbk, k0, k0);
            g.p[i].tri = VG_TRI_B_LOWER;
            VG_HIP(vg_gemm_launch(&g, st));
        }
        if ((rc = gemm1(w.DI + (long)kb * VG_MB * VG_MB, nbk, 1, w.Tmp, k0, 1, w.X + (long)k0 * M, M, nbk, k0, nbk, st, -1.0, 0))) return rc;
    }
    if (!w.Sinv) return VGGP_OK;
    VgGemmBatch g;                                                     // Sinv = X^T X, X lower triangular: the sum runs over k >= max(i, j)
    vg_gemm_init(&g);
    const int i = vg_gemm_add(&g, w.X, 1, M, w.X, M, 1, w.Sinv, M, M, M, M);
    g.p[i].tri = VG_TRI_A_UPPER_B_LOWER;
    VG_HIP(vg_gemm_launch(&g, st));
    return VGGP_OK;
}

// ---- pieces shared by the dense and the iterative masked step ----------------------------------------------------------------
// column statistics of the whitened factors: |b_i|^2, v_i . b_i, and their mask-weighted sums along the other axis
static int vgm_colstats(vggp_ctx* c, VgMasked& w, const double* W, hipStream_t st) {
    const long m1 = c->desc.m1, m2 = c->desc.m2, n1 = c->desc.n1, n2 = c->desc.n2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const double *B1 = d1.BV, *V1 = d1.BV + m1 * n1, *B2 = d2.BV, *V2 = d2.BV + m2 * n2;
    VGM_LAUNCH1D(vgm_coldot_kernel, n1, st, B1, B1, (int)m1, n1, w.nb1);
    VGM_LAUNCH1D(vgm_coldot_kernel, n2, st, B2, B2, (int)m2, n2, w.nb2);
    VGM_LAUNCH1D(vgm_coldot_kernel, n1, st, V1, B1, (int)m1, n1, w.hv1);
    VGM_LAUNCH1D(vgm_coldot_kernel, n2, st, V2, B2, (int)m2, n2, w.hv2);
    {
        const long mm = m2 * m2;                                // w.T (written by the assembly later / slab scratch) is the scratch
        const int nslab = (int)(mm < 64 ? mm : 64);
        hipLaunchKernelGGL(vgm_wcol_part_kernel, dim3((unsigned)((n1 + 255) / 256), (unsigned)nslab), dim3(256), 0, st, W, w.nb2,
                           n1, n2, nslab, w.T);
        VGM_LAUNCH1D(vgm_wcol_sum_kernel, n1, st, w.T, n1, nslab, w.wn2);           // partial over this rank's rows
    }
    hipLaunchKernelGGL(vgm_wrow_kernel, dim3((unsigned)n2), dim3(256), 0, st, W, w.nb1, n1, n2, w.wn1);
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}
// everything of the gradient that needs a0 = Sigma~^-1 c0 only (w.a0 as an m1 x m2 matrix) and the two PT matrices
static int vgm_a0_terms(vggp_ctx* c, VgMasked& w, hipStream_t st) {
    const long m1 = c->desc.m1, m2 = c->desc.m2, n1 = c->desc.n1, n2 = c->desc.n2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const double *B1 = d1.BV, *V1 = d1.BV + m1 * n1, *B2 = d2.BV, *V2 = d2.BV + m2 * n2;
    int rc;
    // Mk1 A0, A0 Mk2 ; UB = A0 B2, UV = A0 V2 ; Zb^T = UB^T B1, Zv1^T = UB^T V1, Zv2^T = UV^T B1   ([n2][n1] like W)
    if ((rc = gemm1(d1.Mk, m1, 1, w.a0, m2, 1, w.MkA1, (int)m2, (int)m1, (int)m2, (int)m1, st))) return rc;
    if ((rc = gemm1(w.a0, m2, 1, d2.Mk, m2, 1, w.MkA2, (int)m2, (int)m1, (int)m2, (int)m2, st))) return rc;
    if ((rc = gemm1(w.a0, m2, 1, B2, n2, 1, w.UB, (int)n2, (int)m1, (int)n2, (int)m2, st))) return rc;
    if ((rc = gemm1(w.a0, m2, 1, V2, n2, 1, w.UV, (int)n2, (int)m1, (int)n2, (int)m2, st))) return rc;
    if ((rc = gemm1(w.UB, 1, n2, B1, n1, 1, w.Zb, (int)n1, (int)n2, (int)n1, (int)m1, st))) return rc;
    if ((rc = gemm1(w.UB, 1, n2, V1, n1, 1, w.Zv1, (int)n1, (int)n2, (int)n1, (int)m1, st))) return rc;
    if ((rc = gemm1(w.UV, 1, n2, B1, n1, 1, w.Zv2, (int)n1, (int)n2, (int)n1, (int)m1, st))) return rc;
    // PT_d = B_d diag(w) B_d^T
    VGM_LAUNCH1D(vgm_scalecols_kernel, m1 * n1, st, B1, w.wn2, (int)m1, n1, w.B1s);
    VGM_LAUNCH1D(vgm_scalecols_kernel, m2 * n2, st, B2, w.wn1, (int)m2, n2, w.B2s);
    // (short outputs, long reductions: split-K with the T buffer -- free by now -- as slab scratch)
    if ((rc = gemm_longk(w.B1s, n1, 1, B1, 1, n1, w.PT1, (int)m1, (int)m1, (int)n1, w.T, st))) return rc;
    if ((rc = gemm_longk(w.B2s, n2, 1, B2, 1, n2, w.PT2, (int)m2, (int)m2, (int)n2, w.T, st))) return rc;
    return VGGP_OK;
}

static int dense_chol_inverse(vggp_ctx* c, VgMasked& w, hipStream_t st) {
    (void)c;
    VgDenseChol d{w.Sg, w.Lg, w.Xg, w.DI, w.Tmp, w.cholscratch, w.choljit, w.cholstatus, w.M, w.Sinv};
    return vg_blocked_chol_inverse(d, st);
}

extern "C" int vggp_elbo_step_masked(vggp_ctx* c, const double* Ym, const double* W, double n_obs, double yy_obs,
                                     const double theta[5], double* elbo_out, double grad_out[5], vggp_info* info,
                                     void* stream) {
    VG_NOT_PAIRED(c, "vggp_elbo_step_masked");
    if (!c || !c->planned) { vg_set_error("vggp_elbo_step_masked: context not planned"); return VGGP_ESTATE; }
    VG_REQUIRE(Ym && W && theta && elbo_out && grad_out, "vggp_elbo_step_masked: null argument");
    c->have_masked = false;          // a failed step must not leave an earlier step's state readable (qv_masked / posterior_masked)
    c->have_iter = false;
    VG_REQUIRE(!(c->desc.flags & VGGP_FLAG_SCATTERED), "vggp_elbo_step_masked: the context was planned for scattered points");
    const long m1 = c->desc.m1, m2 = c->desc.m2, n1 = c->desc.n1, n2 = c->desc.n2, M = m1 * m2;
    VG_REQUIRE(M <= VGM_MAX_M, "vggp_elbo_step_masked: M = m1*m2 = %ld too large for the dense masked solver (<= %d)", M, VGM_MAX_M);
    VG_REQUIRE(m1 * m1 * n1 < (1L << 31) && m2 * m2 * n2 < (1L << 31) && M * M < (1L << 31) * 4, "masked problem too large");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    for (int i = 0; i < 5; ++i) {
        VG_REQUIRE(theta[i] > 0.0 && std::isfinite(theta[i]), "theta[%d]=%g must be positive and finite", i, theta[i]);
        c->h_theta[i] = theta[i];
    }
    int rc = vgm_prepare(c);
    if (rc) return rc;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    // factor build, Cholesky, B|V, Mk and the projections C, C1, C2 of the masked observations (unit outputscale).
    // Row-sharded job (n_ranks > 1): Ym, W are this rank's row slab; every sum over grid rows below is a PARTIAL sum that
    // lands in the all-reduce buffer w.mpay (C, C1, C2 | wn2 | the three M x M assembly matrices) -- ONE collective --
    // after which Sigma~, its factorisation and a0 are replicated on every rank.
    if ((rc = vg_partials_enqueue(c, Ym, w.mpay, st))) return rc;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const double *B1 = d1.BV, *V1 = d1.BV + m1 * n1, *B2 = d2.BV, *V2 = d2.BV + m2 * n2;
    const double *C0 = w.mpay + 2 * m2 * m2, *C1 = C0 + M, *C2 = C1 + M;

    if ((rc = vgm_colstats(c, w, W, st))) return rc;
    // assembly (partial over this rank's rows: T sums over j, R = PP1 T is linear in T)
    VGM_LAUNCH1D(vgm_pairprod_kernel, m2 * m2 * n2, st, B2, B2, (int)m2, (int)m2, n2, w.PP2);
    VGM_LAUNCH1D(vgm_pairprod_kernel, m2 * m2 * n2, st, B2, V2, (int)m2, (int)m2, n2, w.PP2v);
    VGM_LAUNCH1D(vgm_pairprod_kernel, m1 * m1 * n1, st, B1, B1, (int)m1, (int)m1, n1, w.PP1);
    VGM_LAUNCH1D(vgm_pairprod_kernel, m1 * m1 * n1, st, B1, V1, (int)m1, (int)m1, n1, w.PP1v);
    VG_HIP(hipGetLastError());
    if ((rc = gemm1(W, 1, n1, w.PP2, 1, n2, w.T, (int)(m2 * m2), (int)n1, (int)(m2 * m2), (int)n2, st))) return rc;
    if ((rc = gemm1(W, 1, n1, w.PP2v, 1, n2, w.Tv, (int)(m2 * m2), (int)n1, (int)(m2 * m2), (int)n2, st))) return rc;
    if ((rc = gemm1(w.PP1, n1, 1, w.T, m2 * m2, 1, w.R3, (int)(m2 * m2), (int)(m1 * m1), (int)(m2 * m2), (int)n1, st))) return rc;
    if ((rc = gemm1(w.PP1v, n1, 1, w.T, m2 * m2, 1, w.R3 + M * M, (int)(m2 * m2), (int)(m1 * m1), (int)(m2 * m2), (int)n1, st))) return rc;
    if ((rc = gemm1(w.PP1, n1, 1, w.Tv, m2 * m2, 1, w.R3 + 2 * M * M, (int)(m2 * m2), (int)(m1 * m1), (int)(m2 * m2), (int)n1, st))) return rc;
    // the collective of the masked step (no-op on a single-rank context)
    if ((rc = vg_allreduce(c, w.mpay + 2 * m2 * m2, 3 * M + n1 + 3 * M * M, st))) return rc;
    VGM_LAUNCH1D(vgm_permute_kernel, M * M, st, w.R3, (int)m1, (int)m2, c->theta, 1, w.Sg);
    VGM_LAUNCH1D(vgm_permute_kernel, M * M, st, w.R3 + M * M, (int)m1, (int)m2, c->theta, 0, w.Phip);
    VGM_LAUNCH1D(vgm_permute_kernel, M * M, st, w.R3 + 2 * M * M, (int)m1, (int)m2, c->theta, 0, w.Phip + M * M);
    // dense factorisation and inverse of Sigma~
    if ((rc = dense_chol_inverse(c, w, st))) return rc;
    // a0 = Sinv c0 ; A0 = mat(a0) (m1 x m2)
    if ((rc = gemm1(w.Sinv, M, 1, C0, 1, 1, w.a0, 1, (int)M, 1, (int)M, st))) return rc;
    if ((rc = vgm_a0_terms(c, w, st))) return rc;
    // partial traces of Sinv
    VGM_LAUNCH1D(vgm_ptrace_kernel, m1 * m1, st, w.Sinv, (int)m1, (int)m2, 1, w.PTS1);
    VGM_LAUNCH1D(vgm_ptrace_kernel, m2 * m2, st, w.Sinv, (int)m1, (int)m2, 2, w.PTS2);
    // reductions
    VgmRedArgs ra;
    ra.njobs = RJ_COUNT;
    ra.partial = w.partial;
    auto job = [&](int k, const double* a, const double* b, long n, long sa, long sb, int op, const double* cc = nullptr) {
        ra.job[k] = VgmRedJob{a, b, cc, n, sa, sb, op};
    };
    job(RJ_LOGDET, w.Lg, nullptr, M, M + 1, 0, 1);
    job(RJ_Q, C0, w.a0, M, 1, 1, 0);
    job(RJ_AA, w.a0, w.a0, M, 1, 1, 0);
    job(RJ_TRS, w.Sinv, nullptr, M, M + 1, 0, 2);
    job(RJ_TRPHI, w.nb1, w.wn2, n1, 1, 1, 0);
    job(RJ_MK1PTS, d1.Mk, w.PTS1, m1 * m1, 1, 1, 0);
    job(RJ_TRMK1, d1.Mk, nullptr, m1, m1 + 1, 0, 2);
    job(RJ_SPHI1, w.Sinv, w.Phip, M * M, 1, 1, 0);
    job(RJ_AC1, w.a0, C1, M, 1, 1, 0);
    job(RJ_MKA1, w.MkA1, w.a0, M, 1, 1, 0);
    job(RJ_Z1, W, w.Zb, n1 * n2, 1, 1, 3, w.Zv1);
    job(RJ_HV1, w.hv1, w.wn2, n1, 1, 1, 0);
    job(RJ_MK1PT, d1.Mk, w.PT1, m1 * m1, 1, 1, 0);
    job(RJ_MK2PTS, d2.Mk, w.PTS2, m2 * m2, 1, 1, 0);
    job(RJ_TRMK2, d2.Mk, nullptr, m2, m2 + 1, 0, 2);
    job(RJ_SPHI2, w.Sinv, w.Phip + M * M, M * M, 1, 1, 0);
    job(RJ_AC2, w.a0, C2, M, 1, 1, 0);
    job(RJ_MKA2, w.MkA2, w.a0, M, 1, 1, 0);
    job(RJ_Z2, W, w.Zb, n1 * n2, 1, 1, 3, w.Zv2);
    job(RJ_HV2, w.hv2, w.wn1, n2, 1, 1, 0);
    job(RJ_MK2PT, d2.Mk, w.PT2, m2 * m2, 1, 1, 0);
    hipLaunchKernelGGL(vgm_red_kernel, dim3(VG_MD_NPART, RJ_COUNT), dim3(256), 0, st, ra);
    // scalars that are sums over this rank's grid rows (everything else is replicated): second, tiny collective
    const unsigned local_mask = (1u << RJ_Z1) | (1u << RJ_Z2) | (1u << RJ_HV2) | (1u << RJ_MK2PT);
    const bool multi = c->n_ranks > 1 || c->comm || c->cb;
    hipLaunchKernelGGL(vgm_sum_kernel, dim3(1), dim3(64), 0, st, w.partial, w.scal, local_mask, (!multi || c->rank == 0) ? 1 : 0);
    if ((rc = vg_allreduce(c, w.scal, RJ_COUNT, st))) return rc;
    VgmFinalArgs fa{c->theta, w.scal, w.out, n_obs, yy_obs, (int)m1, (int)m2};
    hipLaunchKernelGGL(vgm_final_kernel, dim3(1), dim3(64), 0, st, fa);
    VG_HIP(hipGetLastError());
    // readback
    VG_HIP(hipMemcpyAsync(c->h_out->out, w.out, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
    for (int k = 0; k < 2; ++k) {
        VG_HIP(hipMemcpyAsync(&c->h_out->jitter[k], c->d[k].jitter, sizeof(double), hipMemcpyDeviceToHost, st));
        VG_HIP(hipMemcpyAsync(&c->h_out->status[k], c->d[k].status, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    VG_HIP(hipMemcpyAsync(&c->h_out->counters[1][3], w.cholstatus, sizeof(int), hipMemcpyDeviceToHost, st));
    { const int wrc_ = vg_comm_wait(c, st); if (wrc_) return wrc_; }      // (polls the communicator: a dead peer is an error, not a hang)
    const int hs = c->h_out->counters[1][3];
    *elbo_out = c->h_out->out[0];
    for (int i = 0; i < 5; ++i) grad_out[i] = c->h_out->out[1 + i];
    int status = c->h_out->status[0] ? c->h_out->status[0] : (c->h_out->status[1] ? c->h_out->status[1] : hs);
    if (info) {
        info->jitter1 = c->h_out->jitter[0]; info->jitter2 = c->h_out->jitter[1];
        info->sweeps1 = info->sweeps2 = info->rounds1 = info->rounds2 = 0;
        info->status = status; info->polished = 0;
    }
    if (status) { vg_set_error("masked step: a factor is not positive definite"); return VGGP_ENOTPD; }
    c->have_masked = true;
    return VGGP_OK;
}

// ---- scattered observations ----------------------------------------------------------------------------------------------
// N points (x1_k, x2_k, y_k) that form no grid (satellite tracks: the reference's notebooks 6 / 61 / 7 feed them to the same
// _elbo(), kronecker_structure.py:249-278, whose _Kuf(x) :808-823 takes any x).  Kuf[:, k] = a1(x1_k) (x) a2(x2_k): with the
// per-dimension factors evaluated AT THE POINTS (B_d is m_d x N), Phi~0 = sum_k (b1_k (x) b2_k)(b1_k (x) b2_k)^T is a single
// GEMM over the points between the row-pair products, R[(i1,k1),(i2,k2)] = sum_k (B1[i1,k] B1[k1,k]) (B2[i2,k] B2[k2,k]);
// everything after the assembly -- dense factorisation of Sigma~ = I + rho Phi~0, a0, the gradient's scalars, the final
// combination, the read-outs -- is the masked step's, with sums over observed grid points replaced by sums over the points.
// Specification: oracle/kron.py elbo_step_scattered (== the literal dense restatement to 1e-14).  Several ranks: each plans ITS
// points (desc.n_total = the number of points over all ranks, yy = the global sum of squares) -- two all-reduces, see below.
extern "C" int vggp_elbo_step_scattered(vggp_ctx* c, const double* y, double yy, const double theta[5], double* elbo_out,
                                        double grad_out[5], vggp_info* info, void* stream) {
    if (c && c->is_paired) {
        if (!c->planned) { vg_set_error("context not planned"); return VGGP_ESTATE; }
        VG_ENTER_DEVICE(c->device);
        return vg_paired_step(c, y, yy, theta, elbo_out, grad_out, info, stream ? (hipStream_t)stream : c->own_stream, true);
    }
    if (!c || !c->planned) { vg_set_error("vggp_elbo_step_scattered: context not planned"); return VGGP_ESTATE; }
    VG_REQUIRE(y && theta && elbo_out && grad_out, "vggp_elbo_step_scattered: null argument");
    VG_REQUIRE(c->desc.flags & VGGP_FLAG_SCATTERED, "vggp_elbo_step_scattered: plan the context with VGGP_FLAG_SCATTERED");
    c->have_masked = false;
    c->have_iter = false;            // (the read-outs of vggp_elbo_step_scattered_iter belong to that step alone)
    const long m1 = c->desc.m1, m2 = c->desc.m2, N = c->desc.n1, M = m1 * m2;
    VG_REQUIRE(M <= VGM_MAX_M, "vggp_elbo_step_scattered: M = m1*m2 = %ld too large for the dense solver (<= %d)", M, VGM_MAX_M);
    VG_REQUIRE(m1 * m1 * N < (1L << 31) && m2 * m2 * N < (1L << 31) && M * M < (1L << 31) * 4, "scattered problem too large");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    for (int i = 0; i < 5; ++i) {
        VG_REQUIRE(theta[i] > 0.0 && std::isfinite(theta[i]), "theta[%d]=%g must be positive and finite", i, theta[i]);
        c->h_theta[i] = theta[i];
    }
    int rc = vgm_prepare(c);
    if (rc) return rc;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    if ((rc = vg_partials_enqueue(c, nullptr, nullptr, st))) return rc;          // factors at the points: B|V, Mk (unit outputscale)
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const double *B1 = d1.BV, *V1 = d1.BV + m1 * N, *B2 = d2.BV, *V2 = d2.BV + m2 * N;
    double *C0 = w.mpay + 2 * m2 * m2, *C1 = C0 + M, *C2 = C1 + M;
    // projections: C0 = B1 diag(y) B2^T, C1 = V1 diag(y) B2^T, C2 = B1 diag(y) V2^T   (m1 x m2, K = N)
    VGM_LAUNCH1D(vgm_scalecols_kernel, m1 * N, st, B1, y, (int)m1, N, w.B1s);
    VGM_LAUNCH1D(vgm_scalecols_kernel, m1 * N, st, V1, y, (int)m1, N, w.UV);           // (UV is free until the a0 stage)
    if ((rc = gemm_longk(w.B1s, N, 1, B2, 1, N, C0, (int)m1, (int)m2, (int)N, w.T, st))) return rc;
    if ((rc = gemm_longk(w.UV, N, 1, B2, 1, N, C1, (int)m1, (int)m2, (int)N, w.T, st))) return rc;
    if ((rc = gemm_longk(w.B1s, N, 1, V2, 1, N, C2, (int)m1, (int)m2, (int)N, w.T, st))) return rc;
    // per-point statistics
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, B1, B1, (int)m1, N, w.nb1);
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, B2, B2, (int)m2, N, w.nb2);
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, V1, B1, (int)m1, N, w.hv1);
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, V2, B2, (int)m2, N, w.hv2);
    // assembly: one GEMM over the points per matrix
    VGM_LAUNCH1D(vgm_pairprod_kernel, m2 * m2 * N, st, B2, B2, (int)m2, (int)m2, N, w.PP2);
    VGM_LAUNCH1D(vgm_pairprod_kernel, m2 * m2 * N, st, B2, V2, (int)m2, (int)m2, N, w.PP2v);
    VGM_LAUNCH1D(vgm_pairprod_kernel, m1 * m1 * N, st, B1, B1, (int)m1, (int)m1, N, w.PP1);
    VGM_LAUNCH1D(vgm_pairprod_kernel, m1 * m1 * N, st, B1, V1, (int)m1, (int)m1, N, w.PP1v);
    VG_HIP(hipGetLastError());
    if ((rc = gemm1(w.PP1, N, 1, w.PP2, 1, N, w.R3, (int)(m2 * m2), (int)(m1 * m1), (int)(m2 * m2), (int)N, st))) return rc;
    if ((rc = gemm1(w.PP1v, N, 1, w.PP2, 1, N, w.R3 + M * M, (int)(m2 * m2), (int)(m1 * m1), (int)(m2 * m2), (int)N, st))) return rc;
    if ((rc = gemm1(w.PP1, N, 1, w.PP2v, 1, N, w.R3 + 2 * M * M, (int)(m2 * m2), (int)(m1 * m1), (int)(m2 * m2), (int)N, st))) return rc;
    // point-sharded job (n_ranks > 1: every rank holds its own points): C0, C1, C2 and the three assembly matrices are partial
    // sums over this rank's points -- ONE all-reduce of 3 M + 3 M^2 doubles, then Sigma~, its factorisation and a0 are replicated
    if ((rc = vg_allreduce(c, C0, 3 * M + 3 * M * M, st))) return rc;
    VGM_LAUNCH1D(vgm_permute_kernel, M * M, st, w.R3, (int)m1, (int)m2, c->theta, 1, w.Sg);
    VGM_LAUNCH1D(vgm_permute_kernel, M * M, st, w.R3 + M * M, (int)m1, (int)m2, c->theta, 0, w.Phip);
    VGM_LAUNCH1D(vgm_permute_kernel, M * M, st, w.R3 + 2 * M * M, (int)m1, (int)m2, c->theta, 0, w.Phip + M * M);
    if ((rc = dense_chol_inverse(c, w, st))) return rc;
    if ((rc = gemm1(w.Sinv, M, 1, C0, 1, 1, w.a0, 1, (int)M, 1, (int)M, st))) return rc;
    if ((rc = gemm1(d1.Mk, m1, 1, w.a0, m2, 1, w.MkA1, (int)m2, (int)m1, (int)m2, (int)m1, st))) return rc;
    if ((rc = gemm1(w.a0, m2, 1, d2.Mk, m2, 1, w.MkA2, (int)m2, (int)m1, (int)m2, (int)m2, st))) return rc;
    // UB = A0 B2, UV = A0 V2 (m1 x N); zb_k = b1_k^T A0 b2_k, zv1_k = v1_k^T A0 b2_k, zv2_k = b1_k^T A0 v2_k
    if ((rc = gemm1(w.a0, m2, 1, B2, N, 1, w.UB, (int)N, (int)m1, (int)N, (int)m2, st))) return rc;
    if ((rc = gemm1(w.a0, m2, 1, V2, N, 1, w.UV, (int)N, (int)m1, (int)N, (int)m2, st))) return rc;
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, B1, w.UB, (int)m1, N, w.Zb);
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, V1, w.UB, (int)m1, N, w.Zv1);
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, B1, w.UV, (int)m1, N, w.Zv2);
    // PT_d = B_d diag(|b_other|^2) B_d^T, partial traces of Sinv
    VGM_LAUNCH1D(vgm_scalecols_kernel, m1 * N, st, B1, w.nb2, (int)m1, N, w.B1s);
    VGM_LAUNCH1D(vgm_scalecols_kernel, m2 * N, st, B2, w.nb1, (int)m2, N, w.B2s);
    if ((rc = gemm_longk(w.B1s, N, 1, B1, 1, N, w.PT1, (int)m1, (int)m1, (int)N, w.T, st))) return rc;
    if ((rc = gemm_longk(w.B2s, N, 1, B2, 1, N, w.PT2, (int)m2, (int)m2, (int)N, w.T, st))) return rc;
    VGM_LAUNCH1D(vgm_ptrace_kernel, m1 * m1, st, w.Sinv, (int)m1, (int)m2, 1, w.PTS1);
    VGM_LAUNCH1D(vgm_ptrace_kernel, m2 * m2, st, w.Sinv, (int)m1, (int)m2, 2, w.PTS2);
    VgmRedArgs ra;
    ra.njobs = RJ_COUNT;
    ra.partial = w.partial;
    auto job = [&](int k, const double* a, const double* b, long n, long sa, long sb, int op) {
        ra.job[k] = VgmRedJob{a, b, nullptr, n, sa, sb, op};
    };
    job(RJ_LOGDET, w.Lg, nullptr, M, M + 1, 0, 1);
    job(RJ_Q, C0, w.a0, M, 1, 1, 0);
    job(RJ_AA, w.a0, w.a0, M, 1, 1, 0);
    job(RJ_TRS, w.Sinv, nullptr, M, M + 1, 0, 2);
    job(RJ_TRPHI, w.nb1, w.nb2, N, 1, 1, 0);
    job(RJ_MK1PTS, d1.Mk, w.PTS1, m1 * m1, 1, 1, 0);
    job(RJ_TRMK1, d1.Mk, nullptr, m1, m1 + 1, 0, 2);
    job(RJ_SPHI1, w.Sinv, w.Phip, M * M, 1, 1, 0);
    job(RJ_AC1, w.a0, C1, M, 1, 1, 0);
    job(RJ_MKA1, w.MkA1, w.a0, M, 1, 1, 0);
    job(RJ_Z1, w.Zb, w.Zv1, N, 1, 1, 0);
    job(RJ_HV1, w.hv1, w.nb2, N, 1, 1, 0);
    job(RJ_MK1PT, d1.Mk, w.PT1, m1 * m1, 1, 1, 0);
    job(RJ_MK2PTS, d2.Mk, w.PTS2, m2 * m2, 1, 1, 0);
    job(RJ_TRMK2, d2.Mk, nullptr, m2, m2 + 1, 0, 2);
    job(RJ_SPHI2, w.Sinv, w.Phip + M * M, M * M, 1, 1, 0);
    job(RJ_AC2, w.a0, C2, M, 1, 1, 0);
    job(RJ_MKA2, w.MkA2, w.a0, M, 1, 1, 0);
    job(RJ_Z2, w.Zb, w.Zv2, N, 1, 1, 0);
    job(RJ_HV2, w.hv2, w.nb1, N, 1, 1, 0);
    job(RJ_MK2PT, d2.Mk, w.PT2, m2 * m2, 1, 1, 0);
    hipLaunchKernelGGL(vgm_red_kernel, dim3(VG_MD_NPART, RJ_COUNT), dim3(256), 0, st, ra);
    // scalars that are sums over this rank's points (everything else is replicated): second, tiny collective
    const unsigned local_mask = (1u << RJ_TRPHI) | (1u << RJ_Z1) | (1u << RJ_HV1) | (1u << RJ_MK1PT) | (1u << RJ_Z2) | (1u << RJ_HV2) |
                                (1u << RJ_MK2PT);
    const bool multi = c->n_ranks > 1 || c->comm || c->cb;
    hipLaunchKernelGGL(vgm_sum_kernel, dim3(1), dim3(64), 0, st, w.partial, w.scal, local_mask, (!multi || c->rank == 0) ? 1 : 0);
    if ((rc = vg_allreduce(c, w.scal, RJ_COUNT, st))) return rc;
    VgmFinalArgs fa{c->theta, w.scal, w.out, (double)(c->desc.n_total > N ? c->desc.n_total : N), yy, (int)m1, (int)m2};
    hipLaunchKernelGGL(vgm_final_kernel, dim3(1), dim3(64), 0, st, fa);
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(c->h_out->out, w.out, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
    for (int k = 0; k < 2; ++k) {
        VG_HIP(hipMemcpyAsync(&c->h_out->jitter[k], c->d[k].jitter, sizeof(double), hipMemcpyDeviceToHost, st));
        VG_HIP(hipMemcpyAsync(&c->h_out->status[k], c->d[k].status, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    VG_HIP(hipMemcpyAsync(&c->h_out->counters[1][3], w.cholstatus, sizeof(int), hipMemcpyDeviceToHost, st));
    { const int wrc_ = vg_comm_wait(c, st); if (wrc_) return wrc_; }      // (polls the communicator: a dead peer is an error, not a hang)
    const int hs = c->h_out->counters[1][3];
    *elbo_out = c->h_out->out[0];
    for (int i = 0; i < 5; ++i) grad_out[i] = c->h_out->out[1 + i];
    const int status = c->h_out->status[0] ? c->h_out->status[0] : (c->h_out->status[1] ? c->h_out->status[1] : hs);
    if (info) {
        info->jitter1 = c->h_out->jitter[0]; info->jitter2 = c->h_out->jitter[1];
        info->sweeps1 = info->sweeps2 = info->rounds1 = info->rounds2 = 0;
        info->status = status; info->polished = 0;
    }
    if (status) { vg_set_error("scattered step: a factor is not positive definite"); return VGGP_ENOTPD; }
    c->have_masked = true;
    return VGGP_OK;
}

// ---- gradient of the scattered ELBO w.r.t. the inducing coordinates (SVGP's trainable Z on along-track data) -------------------
// G_B1[i1][k] = -rho sum_i2 U[(i1,i2)][k] B2[i2][k] + w_k UB1[i1][k] + (s1 s2 / v) |b2_k|^2 B1[i1][k],  U = Sigma~^-1 (B1 kr B2),
// w_k = (s1 s2 / v^2)(y_k - rho b1_k^T A0 b2_k), UB1 = A0 B2 (dimension 2: the mirror image, `other` = B1, UBs = A0^T B1).
__global__ void vgm_zg_kernel(const double* U, const double* Bs, const double* Bo, const double* UBs, const double* y, const double* zb,
                              const double* nbo, const double* theta, int ms, int mo, long N, int dim, double* G) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)ms * N) return;
    const int i = (int)(idx / N);
    const long k = idx - (long)i * N;
    const double s12 = theta[2] * theta[3], v = theta[4], rho = s12 / v;
    double u = 0.0;
    if (dim == 0) for (int j = 0; j < mo; ++j) u += U[((long)i * mo + j) * N + k] * Bo[(long)j * N + k];       // rows (i, j) of U
    else          for (int j = 0; j < mo; ++j) u += U[((long)j * ms + i) * N + k] * Bo[(long)j * N + k];       // rows (j, i)
    G[idx] = -rho * u + (s12 / (v * v)) * (y[k] - rho * zb[k]) * UBs[idx] + (s12 / v) * nbo[k] * Bs[idx];
}
__global__ void vgm_scal_kernel(double* x, long n, double a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= a;
}

// dELBO/dz after vggp_elbo_step_scattered on the same y (oracle/kron.py z_grad_scattered; the reference: autograd through _elbo()
// into the Z Parameter of its SVGP classes, kronecker_structure.py:303-304).  The ELBO is a function of A0^T K0^-1 A0 alone, so
// Abar = L0^-T G_B and Kbar = -1/2 L0^-T (G_B B^T) L0^-1; the contraction with d kappa / d z is vggp_zgrad's.  One extra
// M x M x N product (U) on top of the step's three; workspace 2 M N doubles.
extern "C" int vggp_zgrad_scattered(vggp_ctx* c, const double* y, double* gz1, double* gz2, void* stream) {
    if (c && c->is_paired) {
        if (!c->planned) { vg_set_error("context not planned"); return VGGP_ESTATE; }
        VG_ENTER_DEVICE(c->device);
        return vg_paired_zgrad(c, y, gz1, gz2, stream ? (hipStream_t)stream : c->own_stream, true);
    }
    if (!c || !c->have_masked || !c->masked || !(c->desc.flags & VGGP_FLAG_SCATTERED)) {
        vg_set_error("vggp_zgrad_scattered: no finished scattered step");
        return VGGP_ESTATE;
    }
    VG_REQUIRE(y && gz1 && gz2, "vggp_zgrad_scattered: null argument");
    // point-sharded job: every term is a sum over points (Kbar through G_B B^T), so each rank contracts its own points and ONE
    // all-reduce of m1 + m2 doubles adds the parts
    const bool multi = c->n_ranks > 1 || c->comm || c->cb;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    const long m1 = w.m1, m2 = w.m2, M = w.M, N = c->desc.n1;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const bool pts[2] = {d1.basis == VGGP_BASIS_POINTS, d2.basis == VGGP_BASIS_POINTS};
    if (!pts[0]) VG_HIP(hipMemsetAsync(gz1, 0, sizeof(double) * m1, st));
    if (!pts[1]) VG_HIP(hipMemsetAsync(gz2, 0, sizeof(double) * m2, st));
    if (!pts[0] && !pts[1]) return VGGP_OK;
    VG_REQUIRE(M * N < (1L << 31), "vggp_zgrad_scattered: M N = %ld too large", M * N);
    int rc = vg_ensure_misc(c, sizeof(double) * (size_t)(2 * M * N + 2 * (m1 + m2) * N + 3 * N + m1 * m1 + m2 * m2 + m1 + m2 + 64));
    if (rc) return rc;
    double* p = reinterpret_cast<double*>(c->misc);
    double *Zt = p; p += M * N;
    double *U = p; p += M * N;
    double *G[2], *UBs[2];
    G[0] = p; p += m1 * N; G[1] = p; p += m2 * N; UBs[0] = p; p += m1 * N; UBs[1] = p; p += m2 * N;
    double *zb = p; p += N;
    double *nb1 = p; p += N;
    double *nb2 = p; p += N;
    double* WM[2] = {p, p + m1 * m1};
    double* gzbuf = p + m1 * m1 + m2 * m2;
    const double *B1 = d1.BV, *B2 = d2.BV;
    VGM_LAUNCH1D(vgm_pairprod_kernel, M * N, st, B1, B2, (int)m1, (int)m2, N, Zt);
    VG_HIP(hipGetLastError());
    if ((rc = gemm1(w.Sinv, M, 1, Zt, N, 1, U, (int)N, (int)M, (int)N, (int)M, st))) return rc;
    if ((rc = gemm1(w.a0, m2, 1, B2, N, 1, UBs[0], (int)N, (int)m1, (int)N, (int)m2, st))) return rc;       // A0 B2
    if ((rc = gemm1(w.a0, 1, m2, B1, N, 1, UBs[1], (int)N, (int)m2, (int)N, (int)m1, st))) return rc;       // A0^T B1
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, B1, UBs[0], (int)m1, N, zb);
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, B1, B1, (int)m1, N, nb1);
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, B2, B2, (int)m2, N, nb2);
    VGM_LAUNCH1D(vgm_zg_kernel, m1 * N, st, U, B1, B2, UBs[0], y, zb, nb2, c->theta, (int)m1, (int)m2, N, 0, G[0]);
    VGM_LAUNCH1D(vgm_zg_kernel, m2 * N, st, U, B2, B1, UBs[1], y, zb, nb1, c->theta, (int)m2, (int)m1, N, 1, G[1]);
    VG_HIP(hipGetLastError());
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        if (!pts[k]) continue;
        if ((rc = gemm_longk(G[k], N, 1, d.BV, 1, N, WM[k], d.m, d.m, (int)N, w.T, st))) return rc;          // G_B B^T
        VGM_LAUNCH1D(vgm_scal_kernel, (long)d.m * d.m, st, WM[k], (long)d.m * d.m, -0.5);
    }
    for (int pass = 0; pass < 2; ++pass) {
        VgTrsmSpec q[4];
        int nq = 0;
        for (int k = 0; k < 2; ++k) {
            VgDim& d = c->d[k];
            if (!pts[k]) continue;
            const bool dv = d.m <= VG_TRSM_BLK && d.Dinv0 && c->dinv_valid;
            const double* dp = dv ? d.Dinv0 : d.Linv0;
            const long blk = dv ? 256 : 16L * d.m + 16, dld = dv ? 16 : d.m;
            if (pass == 0) {
                q[nq++] = VgTrsmSpec{d.L0, d.m, dp, blk, dld, G[k], N, 1, N, d.m, 1};                       // Abar = L0^-T G_B
                q[nq++] = VgTrsmSpec{d.L0, d.m, dp, blk, dld, WM[k], d.m, 1, d.m, d.m, 1};                  // L0^-T W_M
            } else {
                q[nq++] = VgTrsmSpec{d.L0, d.m, dp, blk, dld, WM[k], 1, d.m, d.m, d.m, 1};                  // (.) L0^-1
            }
        }
        if ((rc = vg_trsm_batch(q, nq, st))) return rc;
    }
    double *o1 = multi ? gzbuf : gz1, *o2 = multi ? gzbuf + m1 : gz2;
    if (multi) VG_HIP(hipMemsetAsync(gzbuf, 0, sizeof(double) * (m1 + m2), st));
    if (pts[0]) VG_HIP(vg_zdot_launch(c->theta, 0, d1.grid, d1.x, (int)m1, N, G[0], d1.AD + m1 * N, WM[0], d1.dK0, o1, st));
    if (pts[1]) VG_HIP(vg_zdot_launch(c->theta, 1, d2.grid, d2.x, (int)m2, N, G[1], d2.AD + m2 * N, WM[1], d2.dK0, o2, st));
    if (multi) {
        if ((rc = vg_allreduce(c, gzbuf, m1 + m2, st))) return rc;
        VG_HIP(hipMemcpyAsync(gz1, gzbuf, sizeof(double) * m1, hipMemcpyDeviceToDevice, st));
        VG_HIP(hipMemcpyAsync(gz2, gzbuf + m1, sizeof(double) * m2, hipMemcpyDeviceToDevice, st));
    }
    { const int wrc_ = vg_comm_wait(c, st); if (wrc_) return wrc_; }      // (polls the communicator: a dead peer is an error, not a hang)
    return VGGP_OK;
}

// q(v) of the last masked step: mean = (s1 s2 / v) L1 A0 L2^T, diag cov = s1 s2 rowdot((L1 (x) L2) Sinv, L1 (x) L2)
extern "C" int vggp_qv_masked(vggp_ctx* c, double* mean, double* var, void* stream) {
    if (c && c->is_paired) {
        if (!c->planned) { vg_set_error("context not planned"); return VGGP_ESTATE; }
        VG_ENTER_DEVICE(c->device);
        return vg_paired_qv(c, mean, var, stream ? (hipStream_t)stream : c->own_stream);
    }
    if (!c || !c->have_masked || !c->masked) { vg_set_error("vggp_qv_masked: no finished masked step"); return VGGP_ESTATE; }
    VG_REQUIRE(mean && var, "vggp_qv_masked: null output");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    const long m1 = w.m1, m2 = w.m2, M = w.M;
    int rc;
    if ((rc = gemm1(c->d[0].L0, m1, 1, w.a0, m2, 1, w.MkA1, (int)m2, (int)m1, (int)m2, (int)m1, st))) return rc;      // L1 A0
    if ((rc = gemm1(w.MkA1, m2, 1, c->d[1].L0, 1, m2, mean, (int)m2, (int)m1, (int)m2, (int)m2, st))) return rc;     // . L2^T
    const int e1 = (c->d[0].basis == VGGP_BASIS_VFF || c->d[0].basis == VGGP_BASIS_B1) ? -1 : 1;
    const int e2 = (c->d[1].basis == VGGP_BASIS_VFF || c->d[1].basis == VGGP_BASIS_B1) ? -1 : 1;
    VGM_LAUNCH1D(vgm_scale_rho_kernel, M, st, mean, M, c->theta, e1, e2);
    VGM_LAUNCH1D(vgm_kron_kernel, M * M, st, c->d[0].L0, c->d[1].L0, (int)m1, (int)m2, w.R);
    if ((rc = gemm1(w.R, M, 1, w.Sinv, M, 1, w.Sg, (int)M, (int)M, (int)M, (int)M, st))) return rc;
    VGM_LAUNCH1D(vgm_rowdot_scale_kernel, M, st, w.Sg, w.R, M, c->theta, var, e1, e2);
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
    if (c && c->is_paired) {
        if (!c->planned) { vg_set_error("context not planned"); return VGGP_ESTATE; }
        VG_ENTER_DEVICE(c->device);
        return vg_paired_readout(c, C1, mv1, C2, mv2, kd1, kd2, mean, var, flags, stream ? (hipStream_t)stream : c->own_stream);
    }
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
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    VgGemmBatch g;
    vg_gemm_init(&g);                                    // U_d = Linv0_d C_d^T   (m_d x mv_d)
    vg_gemm_add(&g, d1.Linv0, m1, 1, C1, 1, m1, U1, (int)mv1, (int)m1, (int)mv1, (int)m1);
    vg_gemm_add(&g, d2.Linv0, m2, 1, C2, 1, m2, U2, (int)mv2, (int)m2, (int)mv2, (int)m2);
    VG_HIP(vg_gemm_launch(&g, st));
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
    if (c && c->is_paired) {
        if (!c->planned) { vg_set_error("context not planned"); return VGGP_ESTATE; }
        VG_ENTER_DEVICE(c->device);
        return vg_paired_posterior(c, xs1, xs2, ns, mean, var, stream ? (hipStream_t)stream : c->own_stream);
    }
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
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    for (long off = 0; off < ns; off += chunk) {
        const int cn = (int)std::min<long>(chunk, ns - off);
        VgFactorJob fj[2] = {
            VgFactorJob{xs1 + off, d1.grid, A1, nullptr, nullptr, nullptr, cn, d1.m, d1.kind, d1.basis, 0, 0.0, c->desc.flags},
            VgFactorJob{xs2 + off, d2.grid, A2, nullptr, nullptr, nullptr, cn, d2.m, d2.kind, d2.basis, 1, 0.0, c->desc.flags}};
        VG_HIP(vg_factor_build_launch(fj, 2, c->theta, st));
        VgGemmBatch g;
        vg_gemm_init(&g);
        vg_gemm_add(&g, d1.Linv0, m1, 1, A1, cn, 1, B1, cn, (int)m1, cn, (int)m1);
        vg_gemm_add(&g, d2.Linv0, m2, 1, A2, cn, 1, B2, cn, (int)m2, cn, (int)m2);
        VG_HIP(vg_gemm_launch(&g, st));
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
    if (c && c->is_paired) {
        if (!c->planned) { vg_set_error("context not planned"); return VGGP_ESTATE; }
        VG_ENTER_DEVICE(c->device);
        return vg_paired_posterior_cov(c, xs1, xs2, ns, cov, stream ? (hipStream_t)stream : c->own_stream);
    }
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
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const int cn = (int)ns;
    VgFactorJob fj[2] = {
        VgFactorJob{xs1, d1.grid, A1, nullptr, nullptr, nullptr, cn, d1.m, d1.kind, d1.basis, 0, 0.0, c->desc.flags},
        VgFactorJob{xs2, d2.grid, A2, nullptr, nullptr, nullptr, cn, d2.m, d2.kind, d2.basis, 1, 0.0, c->desc.flags}};
    VG_HIP(vg_factor_build_launch(fj, 2, c->theta, st));
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, d1.Linv0, m1, 1, A1, cn, 1, B1, cn, (int)m1, cn, (int)m1);
    vg_gemm_add(&g, d2.Linv0, m2, 1, A2, cn, 1, B2, cn, (int)m2, cn, (int)m2);
    VG_HIP(vg_gemm_launch(&g, st));
    VGM_LAUNCH1D(vgm_pairprod_kernel, M * cn, st, B1, B2, (int)m1, (int)m2, (long)cn, w.R);                 // T  (M x ns)
    if ((rc = gemm1(w.Sinv, M, 1, w.R, cn, 1, w.Sg, cn, (int)M, cn, (int)M, st))) return rc;                  // Sigma~^{-1} T
    const double ss = c->h_theta[2] * c->h_theta[3];
    if ((rc = gemm1(w.R, 1, cn, w.Sg, cn, 1, cov, cn, cn, cn, (int)M, st, ss, 0))) return rc;                  // + s1 s2 T^T Sigma~^{-1} T
    if ((rc = gemm1(w.R, 1, cn, w.R, cn, 1, cov, cn, cn, cn, (int)M, st, -ss, 1))) return rc;                  // - s1 s2 T^T T
    VG_HIP(vg_prior_cov_launch(xs1, xs2, ns, d1.kind, d2.kind, c->theta, cov, st));
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

// dense M x M covariance of q(v) of the last masked step: S = s1^e1 s2^e2 (L1 (x) L2) Sigma~^{-1} (L1 (x) L2)^T
__global__ void vgm_scale_e_kernel(double* x, long n, const double* theta, int e1, int e2) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= (e1 > 0 ? theta[2] : 1.0 / theta[2]) * (e2 > 0 ? theta[3] : 1.0 / theta[3]);
}
extern "C" int vggp_qv_cov_masked(vggp_ctx* c, double* cov, void* stream) {
    if (c && c->is_paired) {
        if (!c->planned) { vg_set_error("context not planned"); return VGGP_ESTATE; }
        VG_ENTER_DEVICE(c->device);
        return vg_paired_qv_cov(c, cov, stream ? (hipStream_t)stream : c->own_stream);
    }
    if (!c || !c->have_masked || !c->masked) { vg_set_error("vggp_qv_cov_masked: no finished masked step"); return VGGP_ESTATE; }
    VG_REQUIRE(cov, "vggp_qv_cov_masked: null output");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    const long m1 = w.m1, m2 = w.m2, M = w.M;
    int rc;
    const int e1 = (c->d[0].basis == VGGP_BASIS_VFF || c->d[0].basis == VGGP_BASIS_B1) ? -1 : 1;
    const int e2 = (c->d[1].basis == VGGP_BASIS_VFF || c->d[1].basis == VGGP_BASIS_B1) ? -1 : 1;
    VGM_LAUNCH1D(vgm_kron_kernel, M * M, st, c->d[0].L0, c->d[1].L0, (int)m1, (int)m2, w.R);
    if ((rc = gemm1(w.R, M, 1, w.Sinv, M, 1, w.Sg, (int)M, (int)M, (int)M, (int)M, st))) return rc;
    if ((rc = gemm1(w.Sg, M, 1, w.R, 1, M, cov, (int)M, (int)M, (int)M, (int)M, st))) return rc;
    VGM_LAUNCH1D(vgm_scale_e_kernel, M * M, st, cov, M * M, c->theta, e1, e2);
    VG_HIP(hipGetLastError());
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

// ================================================================================================================================
// Iterative masked step: what gpytorch does for the reference above max_cholesky_size = 800 --
// `inv_matmul` by conjugate gradients, `log_prob` by stochastic Lanczos quadrature (kronecker_structure.py:269, :273) -- rebuilt for
// the Kronecker structure, preconditioned and with FIXED probes, so that no M x M matrix exists and M = m1 m2 is not limited by
// O(M^2) memory or O(M^3) time.  Specification: oracle/kron.py elbo_step_masked_iter (tolerances against the dense step: ELBO 1e-5,
// gradient 1e-4 of its largest component).
//
//   operator        Sigma~ V = V + rho B1 (W^T o (B1^T V B2)) B2^T          V: m1 x m2; four MFMA GEMMs + one mask pass over n1 x n2
//   block vectors   nbc = 1 + n_probes right-hand sides, stored interleaved [m1][nbc][m2]: then every GEMM of the operator is ONE
//                   plain GEMM for the whole block ([m1][(nbc m2)] as B operand, [(m1 nbc)][m2] / [(n1 nbc)][.] as A operand)
//   preconditioner  P = I + rho p G1 (x) G2 (p = observed fraction): E[Phi~] for an unstructured mask, diagonal in the Kronecker
//                   eigenbasis Q1 (x) Q2 of the full-grid path (the step's own eigensolver), applied by four m x m x m GEMMs
//   log|Sigma~|     log|P| + mean_z M e1^T log(T_z) e1, T_z = Lanczos tridiagonal of P^-1/2 Sigma~ P^-1/2 from the PCG coefficients of
//                   the probe z = P^1/2 z0, z0 Rademacher from a counter-based hash (bitwise reproducible)
//   traces          tr(Sigma~^-1 D) = tr(P^-1 D) [closed form, two GEMMs over the mask] + mean_z (Sigma~^-1 z - P^-1 z)^T D P^-1 z
// ================================================================================================================================
#define VGI_NTS 16                                // the scalars vgi_combine_kernel reads (14 used)
struct VgIter {
    int nbc = 0, maxit = 0;
    double *Wt;                                   // [n1][n2] mask, transposed once per step (masked data only)
    double *X, *R, *Zp, *Pd, *AP, *Wz, *Tm, *Tm2; // block vectors [m1][nbc][m2]
    double *T1;                                   // [n1][nbc][max(m1, m2)] (masked data only)
    double *F0, *F1, *F2;                         // fields [n1][nbc][n2]; scattered points: [nbc][N]
    double *alh, *beh;                            // [maxit][nbc] PCG coefficients
    double *part;                                 // [2][nbc] the PCG's column dots on their way to the scalars (one chunk)
    double *col;                                  // per-column scalars: [0] rz, [1] pAp, [2] r0^2, [3] rr, [4] alpha, [5] beta, [6] active, [7] k
    double *Rr1, *Rr2, *Rv1, *Rv2, *RR1, *RRV1, *RR2, *RRV2, *TW, *TWv, *Ex;   // rotated factors and the exact traces' temporaries
    double *dg1, *dg2, *Tq;                       // diag(Q^T Mk Q), m x m temporary
    double *Qk1, *Qk2;                            // the preconditioner's eigenbasis of the last cold solve (rows = eigenvectors), kept across steps
    double *ts;                                   // [VGI_NTS] scalars
    double *pc;                                   // [nbc] per-column sums: the probes' quadratures, later the column dots of the Mk terms
    double *fpart;                                // [1024] block partials of the field sums
    double *krs;                                  // scattered points: split scratch of the back kernel
    int* nact;                                    // device word: number of active columns
};

// out[a][c][b] = in[a][c][b] * f(dP[a][b]),  dP = 1 + rho p max(lam1,0) max(lam2,0);  mode 0: 1/dP, 1: sqrt(dP), 2: 1/sqrt(dP)
__global__ void vgi_scale_kernel(const double* in, double* out, const double* lam1, const double* lam2, const double* theta, double p,
                                 int m1, int nbc, int m2, int mode, int c_from) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)m1 * nbc * m2) return;
    const int b = (int)(idx % m2), c = (int)((idx / m2) % nbc), a = (int)(idx / ((long)m2 * nbc));
    const double rho = theta[2] * theta[3] / theta[4];
    const double d = 1.0 + rho * p * fmax(lam1[a], 0.0) * fmax(lam2[b], 0.0);
    const double f = mode == 0 ? 1.0 / d : (mode == 1 ? sqrt(d) : 1.0 / sqrt(d));
    out[idx] = c >= c_from ? in[idx] * f : 0.0;
}
__global__ void vgi_transpose_kernel(const double* W, long n1, long n2, double* Wt) {      // Wt[i][j] = W[j][i]
    __shared__ double tile[32][33];
    const long i0 = (long)blockIdx.x * 32, j0 = (long)blockIdx.y * 32;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const long j = j0 + r, i = i0 + threadIdx.x;
        tile[r][threadIdx.x] = (j < n2 && i < n1) ? W[j * n1 + i] : 0.0;
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {
        const long i = i0 + r, j = j0 + threadIdx.x;
        if (i < n1 && j < n2) Wt[i * n2 + j] = tile[threadIdx.x][r];
    }
}
// F[i][c][j] *= Wt[i][j]
__global__ void vgi_mask_kernel(double* F, const double* Wt, long n1, int nbc, long n2) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n1 * nbc * n2) return;
    const long j = idx % n2, i = idx / (n2 * nbc);
    F[idx] *= Wt[i * n2 + j];
}
// column c of the block vector <- the m1 x m2 matrix src (mode 0) / the matrix dst <- column c (mode 1)
__global__ void vgi_col_kernel(double* blk, double* mat, int m1, int nbc, int m2, int c, int mode) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)m1 * m2) return;
    const int a = (int)(idx / m2), b = (int)(idx - (long)a * m2);
    double* e = blk + ((long)a * nbc + c) * m2 + b;
    if (mode == 0) *e = mat[idx]; else mat[idx] = *e;
}
// per-column dot products of block vectors: out0[c] = <A, B>_c, out1[c] = <C, D>_c (second pair optional); one workgroup per
// column, fixed summation order
__global__ __launch_bounds__(256) void vgi_coldots_kernel(const double* A, const double* B, const double* C, const double* D, int m1, int nbc,
                                                          int m2, double* out0, double* out1) {
    __shared__ double red[8];
    const int c = blockIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (long e = threadIdx.x; e < (long)m1 * m2; e += 256) {
        const long a = e / m2, b = e - a * m2, o = (a * nbc + c) * m2 + b;
        s0 += A[o] * B[o];
        if (C) s1 += C[o] * D[o];
    }
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_xor(s0, off); s1 += __shfl_xor(s1, off); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = s0; red[4 + (threadIdx.x >> 6)] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out0[c] = (red[0] + red[1]) + (red[2] + red[3]);
        if (out1) out1[c] = (red[4] + red[5]) + (red[6] + red[7]);
    }
}
// out = a + rho b   (AP = P + rho Phi~ P)
__global__ void vgi_axpy_rho_kernel(const double* a, const double* b, const double* theta, long n, double* out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) out[idx] = a[idx] + (theta[2] * theta[3] / theta[4]) * b[idx];
}
__global__ void vgi_sub_kernel(const double* a, const double* b, long n, double* out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) out[idx] = a[idx] - b[idx];
}
__global__ void vgi_mul_kernel(const double* a, const double* b, long n, double* out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) out[idx] = a[idx] * b[idx];
}
// out[a] = sum_k A[a][k] B[a][k]
__global__ void vgi_rowdot_kernel(const double* A, const double* B, int m, double* out) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= m) return;
    double s = 0.0;
    for (int k = 0; k < m; ++k) s += A[(long)a * m + k] * B[(long)a * m + k];
    out[a] = s;
}
// Gauss quadrature of log on the Lanczos tridiagonal of each probe column (vg_lanczos_logquad: implicit QL with shifts, first
// eigenvector components only): one lane per probe, k <= VGI_MAXIT.  out[c - 1] = M sum_j tau_j^2 log(theta_j), nbc - 1 values;
// fail |= 1: an eigenvalue did not converge, 2: an eigenvalue is not positive
#define VGI_MAXIT 128
__global__ void vgi_slq_kernel(const double* alh, const double* beh, const double* col, int nbc, double Mdim, double* out, int* fail) {
    const int c = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nbc) return;
    const int k = (int)col[7 * nbc + c];
    double d[VGI_MAXIT], e[VGI_MAXIT], z[VGI_MAXIT];
    for (int j = 0; j < k; ++j) {
        const double a = alh[(long)j * nbc + c];
        d[j] = 1.0 / a + (j > 0 ? beh[(long)(j - 1) * nbc + c] / alh[(long)(j - 1) * nbc + c] : 0.0);
        e[j] = j + 1 < k ? sqrt(beh[(long)j * nbc + c]) / a : 0.0;
        z[j] = j == 0 ? 1.0 : 0.0;
    }
    double acc;
    const int code = vg_lanczos_logquad(d, e, z, k, &acc);
    if (code) atomicOr(fail, code);
    out[c - 1] = Mdim * acc;
}
// scalars of the iterative step -> the slots of the dense step's reduction buffer (vgm_final_kernel reads them)
//   ts: [0] sum log dP, [1] sum of the quadratures, [2] exact tr(P^-1 Phi), [3] est BB, [4] exact V1, [5] est 1a, [6] est 1b,
//       [7] exact V2, [8] est 2a, [9] est 2b, [10] exact Mk1, [11] est Mk1, [12] exact Mk2, [13] est Mk2
__global__ void vgi_combine_kernel(const double* ts, const double* theta, double Mdim, int nz, double* scal) {
    if (threadIdx.x != 0) return;
    const double rho = theta[2] * theta[3] / theta[4], inz = 1.0 / nz;
    scal[RJ_LOGDET] = 0.5 * (ts[0] + ts[1] * inz);
    const double trSP = ts[2] + ts[3] * inz;
    scal[RJ_TRS] = Mdim - rho * trSP;
    scal[RJ_SPHI1] = 0.5 * (2.0 * ts[4] + (ts[5] + ts[6]) * inz);
    scal[RJ_SPHI2] = 0.5 * (2.0 * ts[7] + (ts[8] + ts[9]) * inz);
    scal[RJ_MK1PTS] = ts[10] + ts[11] * inz;
    scal[RJ_MK2PTS] = ts[12] + ts[13] * inz;
}
// out[0] = sum_{a,b} f(dP[a,b]) * E[a][b] (E null: 1) * (dg1 ? dg1[a] : 1) * (dg2 ? dg2[b] : 1);  mode 0: f = 1/dP, 1: f = log dP
__global__ __launch_bounds__(256) void vgi_dpsum_kernel(const double* lam1, const double* lam2, const double* theta, double p, int m1, int m2,
                                                        const double* E, const double* dg1, const double* dg2, int mode, double* out) {
    __shared__ double red[4];
    const double rho = theta[2] * theta[3] / theta[4];
    double s = 0.0;
    for (long e = threadIdx.x; e < (long)m1 * m2; e += 256) {
        const int a = (int)(e / m2), b = (int)(e - (long)a * m2);
        const double d = 1.0 + rho * p * fmax(lam1[a], 0.0) * fmax(lam2[b], 0.0);
        double v = mode == 0 ? 1.0 / d : log(d);
        if (E) v *= E[e];
        if (dg1) v *= dg1[a];
        if (dg2) v *= dg2[b];
        s += v;
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}
// out[0] = sum over i, c >= 1, j of Wt[i][j] Fa[i][c][j] Fb[i][c][j]   (two stages, fixed order)
__global__ __launch_bounds__(256) void vgi_fieldsum_part_kernel(const double* Fa, const double* Fb, const double* Wt, long n1, int nbc, long n2,
                                                                double* part) {
    __shared__ double red[4];
    const long total = n1 * nbc * n2;
    double s = 0.0;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long j = idx % n2, c = (idx / n2) % nbc, i = idx / (n2 * nbc);
        if (c >= 1) s += Wt[i * n2 + j] * Fa[idx] * Fb[idx];
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void vgi_sum_kernel(const double* part, int n, double* out, int c_from) {           // out[0] = sum_{k >= c_from} part[k]
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int k = c_from; k < n; ++k) s += part[k];
    out[0] = s;
}

// ---- the iterative steps on a multi-rank context ------------------------------------------------------------------------------------------
// Split: as the dense sharded steps.  Masked grid: a rank holds the row slab Ym[rows], W[rows] and is planned with x2[rows]
// (d2.n = its rows; n_obs, yy_obs and desc.n_total = n1 n2 are global).  Scattered points: a rank holds its own points (uneven
// shares are fine; desc.n_total = N over all ranks, yy global).  The block vectors [m1][nbc][m2], the probes, the preconditioner,
// its kept basis and the PCG scalars are replicated.  Three kinds of collective, all vg_allreduce on the step's stream, in the same
// order on every rank:
//   before the solve    ONE packed all-reduce of w.mpay: G2 | C0, C1, C2 | wn2 (masked; G1 is over the unsharded axis) or
//                       G2 | C0, C1, C2 | G1 (scattered).  The observed fraction p of the preconditioner is the global one
//   per PCG iteration   ONE all-reduce of the partial Phi~ Pd block (M nbc doubles) in vgi_apply -- the step's solve and every block
//                       solve of the read-outs pass through there
//   after the solve     ONE packed all-reduce of w.scal: the reduction jobs that are sums over this rank's rows / points (the dense
//                       steps' local_mask; rank 0 alone contributes the replicated ones) and, behind them, ts[2 .. 9]: the five
//                       control-variate field sums and the three exact-trace products (vgi_exact_sum is linear in Ex)
// Invariants:
//   1. Every host decision is taken from all-reduced or replicated data only -- the active-column count read per iteration,
//      VG_PCG_ESTALE / vgi_retry_stale, the cold-versus-kept choice of vgi_basis (host counters fed by iteration counts), VGGP_ENOCONV,
//      the status words -- so all ranks take the same branch and issue the same number of collectives.  The eigen-decomposition
//      runs redundantly on the all-reduced Gram matrices.
//   2. Every host wait inside the iterative path is vg_comm_wait, which polls the communicator: a dead peer is an error, not a hang.
//   (Before any of this the entries ask vg_comm_verify, once per context, whether the transport sums over n_ranks ranks at all:
//   invariant 1 is worth nothing over one that does not, and the entry returns VGGP_EINVAL.)
//   3. On a single-rank context nothing changes: vg_allreduce returns at once, vg_comm_wait is hipStreamSynchronize, the packing
//      kernel is not launched, and the same kernels run in the same order on the same operands.
#define VGI_TS_SLOT 24                            // w.scal: [RJ_COUNT reduction jobs | . | ts[2 .. 9] at VGI_TS_SLOT], 32 doubles
static_assert(RJ_COUNT <= VGI_TS_SLOT, "the packed scalars of the iterative step overlap");
// ts[2 .. 9] -> scal[VGI_TS_SLOT ..] (unpack = 0) and back (1): plain stores, one lane each
__global__ void vgi_pack_ts_kernel(double* ts, double* scal, int unpack) {
    const int k = threadIdx.x;
    if (k >= 8) return;
    if (unpack) ts[2 + k] = scal[VGI_TS_SLOT + k];
    else scal[VGI_TS_SLOT + k] = ts[2 + k];
}
static bool vgi_multi(const vggp_ctx* c) { return c->n_ranks > 1 || c->comm || c->cb; }
#define VGI_WAIT(c, st) do { const int wrc_ = vg_comm_wait(c, st); if (wrc_) return wrc_; } while (0)
// the observed fraction of the preconditioner: n_obs / (grid nodes) resp. 1 / N, on a multi-rank context over ALL ranks (desc.n_total)
static double vgi_obs_fraction(const vggp_ctx* c, bool scattered, double n_obs) {
    const long n1 = c->desc.n1, n2 = c->desc.n2, nt = vgi_multi(c) ? c->desc.n_total : 0;
    if (scattered) return 1.0 / (double)(nt > n1 ? nt : n1);
    return nt > n1 * n2 ? n_obs / (double)nt : n_obs / ((double)n1 * (double)n2);
}

// The step's arena (w.imem) for either data kind.  Scattered points (n1 = N): no mask and no grid-sized buffers, fields [nbc][N],
// rotated factors [m_d][N], the back kernel's split scratch.
static int vgi_prepare(VgMasked& w, VgIter& it, int nbc, int maxit) {
    const size_t m1 = w.m1, m2 = w.m2, n1 = w.n1, n2 = w.scattered ? w.n1 : w.n2, M = w.M, mx = std::max(m1, m2);
    const bool sc = w.scattered;
    const size_t nf = sc ? n1 * nbc : n1 * nbc * n2;
    char oom[256];
    snprintf(oom, sizeof(oom), "the workspace of the iterative scattered step needs %%.1f GiB (m1 = %d, m2 = %d, N = %ld, %d columns) but only "
             "%%.1f GiB of device memory are free", w.m1, w.m2, (long)n1, nbc);
    bool grew = false;
    const int rc = vg_arena_carve(&w.imem, &w.ibytes, sc ? oom : nullptr, &grew, [&](VgArena& a) {
        it.Wt = a.take(sc ? 0 : n1 * n2);
        it.X = a.take(M * nbc); it.R = a.take(M * nbc); it.Zp = a.take(M * nbc); it.Pd = a.take(M * nbc); it.AP = a.take(M * nbc);
        it.Wz = a.take(M * nbc); it.Tm = a.take(M * nbc); it.Tm2 = a.take(M * nbc);
        it.T1 = a.take(sc ? 0 : n1 * nbc * mx);
        it.F0 = a.take(nf); it.F1 = a.take(nf); it.F2 = a.take(nf);
        it.alh = a.take((size_t)maxit * nbc); it.beh = a.take((size_t)maxit * nbc);
        it.col = a.take(8 * (size_t)nbc);
        it.Rr1 = a.take(m1 * n1); it.Rv1 = a.take(m1 * n1); it.RR1 = a.take(m1 * n1); it.RRV1 = a.take(m1 * n1);
        it.Rr2 = a.take(m2 * n2); it.Rv2 = a.take(m2 * n2); it.RR2 = a.take(m2 * n2); it.RRV2 = a.take(m2 * n2);
        it.TW = a.take(sc ? 0 : n1 * m2); it.TWv = a.take(sc ? 0 : n1 * m2); it.Ex = a.take(M);
        it.dg1 = a.take(m1); it.dg2 = a.take(m2); it.Tq = a.take(mx * mx);
        it.Qk1 = a.take(m1 * m1); it.Qk2 = a.take(m2 * m2);
        it.ts = a.take(VGI_NTS);
        it.pc = a.take((size_t)nbc);
        it.fpart = a.take(1024);                  // (its own: a block vector has M nbc doubles, which may be fewer than the 1024 partials)
        it.krs = a.take(sc ? vg_kr_back_scratch((int)m1, (int)m2, (long)n1, nbc) : 0);
        it.nact = reinterpret_cast<int*>(a.take(8));
        it.part = a.take(2 * (size_t)nbc);
    });
    if (grew || w.ib_nbc != nbc || w.ib_maxit != maxit) w.ib_valid = false;      // (the layout moves: the kept basis is gone)
    w.ib_nbc = nbc; w.ib_maxit = maxit;
    it.nbc = nbc; it.maxit = maxit;
    return rc;
}

// G = L^T-side product: block field F[i][c][j] = l_i^T V_c r_j for all columns (V block [m1][nbc][m2], L: m1 x n1, R: m2 x n2)
static int vgi_field(const VgMasked& w, const VgIter& it, const double* L, const double* V, const double* R, double* F, hipStream_t st) {
    const int m1 = w.m1, m2 = w.m2, nbc = it.nbc;
    const long n1 = w.n1, n2 = w.n2;
    int rc;
    // T1[i][(c,b)] = sum_a L[a][i] V[a][(c,b)]
    if ((rc = gemm1(L, 1, n1, V, (long)nbc * m2, 1, it.T1, nbc * m2, (int)n1, nbc * m2, m1, st))) return rc;
    // F[(i,c)][j] = sum_b T1[(i,c)][b] R[b][j]
    return gemm1(it.T1, m2, 1, R, n2, 1, F, (int)n2, (int)(n1 * nbc), (int)n2, m2, st);
}
// out[a][(c,b)] = sum_{i,j} L[a][i] F[i][c][j] R[b][j]
static int vgi_back(const VgMasked& w, const VgIter& it, const double* L, const double* F, const double* R, double* out, hipStream_t st) {
    const int m1 = w.m1, m2 = w.m2, nbc = it.nbc;
    const long n1 = w.n1, n2 = w.n2;
    int rc;
    // T1[(i,c)][b] = sum_j F[(i,c)][j] R[b][j]
    if ((rc = gemm1(F, n2, 1, R, 1, n2, it.T1, m2, (int)(n1 * nbc), m2, (int)n2, st))) return rc;
    return gemm1(L, n1, 1, it.T1, (long)nbc * m2, 1, out, nbc * m2, m1, nbc * m2, (int)n1, st);
}
// out = Q1 ((Q1^T V Q2) o f(dP)) Q2^T for the whole block (Qt rows = eigenvectors); mode as vgi_scale_kernel; c_from: columns below are zeroed
static int vgi_rot(vggp_ctx* c, const VgMasked& w, const VgIter& it, const double* V, double* out, int mode, int c_from, double p, hipStream_t st,
                   double* rotated_out = nullptr) {
    const int m1 = w.m1, m2 = w.m2, nbc = it.nbc;
    const long nb = (long)m1 * nbc * m2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    int rc;
    if ((rc = gemm1(d1.Qt, m1, 1, V, (long)nbc * m2, 1, it.Tm, nbc * m2, m1, nbc * m2, m1, st))) return rc;            // Q1^T V
    if ((rc = gemm1(it.Tm, m2, 1, d2.Qt, 1, m2, it.Tm2, m2, m1 * nbc, m2, m2, st))) return rc;                      // (.) Q2
    if (rotated_out) VG_HIP(hipMemcpyAsync(rotated_out, it.Tm2, sizeof(double) * nb, hipMemcpyDeviceToDevice, st));
    VGM_LAUNCH1D(vgi_scale_kernel, nb, st, it.Tm2, it.Tm2, d1.lam0, d2.lam0, c->theta, p, m1, nbc, m2, mode, c_from);
    if ((rc = gemm1(it.Tm2, m2, 1, d2.Qt, m2, 1, it.Tm, m2, m1 * nbc, m2, m2, st))) return rc;                      // (.) Q2^T
    return gemm1(d1.Qt, 1, m1, it.Tm, (long)nbc * m2, 1, out, nbc * m2, m1, nbc * m2, m1, st);                     // Q1 (.)
}

// ---- the stages both iterative steps (and the block solves of their read-outs) are made of --------------------------------------------
// AP = Pd + rho Phi~ Pd for the block.  Masked grid: Phi~ V = B1 (Wt o (B1^T V B2)) B2^T.  Scattered points (w.scattered):
// Phi~ V = sum_k b1_k (b1_k^T V b2_k) b2_k^T by the two kernels of kr.hip, the field kernel in its four-column instantiation or
// (field2) in its two-column one: the same bits at 2.2 x the rate at 64 columns and at 16; the read-outs run that one
static int vgi_apply(vggp_ctx* c, const VgMasked& w, const VgIter& it, bool field2, hipStream_t st) {
    const int m1 = w.m1, m2 = w.m2, nbc = it.nbc;
    const long n1 = w.n1, n2 = w.n2, nb = w.M * nbc;
    const double *B1 = c->d[0].BV, *B2 = c->d[1].BV;
    int rc;
    if (w.scattered) {
        if (field2) VG_HIP(vg_kr_field2_launch(B1, B2, it.Pd, m1, m2, n1, nbc, it.F0, st));
        else VG_HIP(vg_kr_field_launch(B1, B2, it.Pd, m1, m2, n1, nbc, it.F0, st));
        VG_HIP(vg_kr_back_launch(B1, B2, it.F0, m1, m2, n1, nbc, it.AP, it.krs, st));
    } else {
        if ((rc = vgi_field(w, it, B1, it.Pd, B2, it.F0, st))) return rc;
        VGM_LAUNCH1D(vgi_mask_kernel, n1 * nbc * n2, st, it.F0, it.Wt, n1, nbc, n2);
        if ((rc = vgi_back(w, it, B1, it.F0, B2, it.AP, st))) return rc;
    }
    if ((rc = vg_allreduce(c, it.AP, nb, st))) return rc;      // Phi~ Pd is a sum over this rank's rows / points (no-op on one rank)
    VGM_LAUNCH1D(vgi_axpy_rho_kernel, nb, st, it.Pd, it.AP, c->theta, nb, it.AP);
    return VGGP_OK;
}

// Block PCG for Sigma~ X = R (vg_block_pcg, block_pcg.h): the right-hand sides are in it.R on entry, the solution is in it.X on return.
// The caller object: the operator is vgi_apply, the preconditioner the rotation by d.Qt with d.lam0 and p, a column dot is ONE
// workgroup per column (vgi_coldots_kernel into the one-chunk partial buffer it.part), and the host waits with vg_comm_wait
// (invariant 2 above) before it reads the active count.  No read-back of that count after the start: the read-outs run one solve per
// 64 cells.  A solve that runs past stale_limit gives the kept basis up (VG_PCG_ESTALE, vgi_retry_stale).
static int vgi_pcg(vggp_ctx* c, VgMasked& w, const VgIter& it, double p, double tol, int max_iter, bool history, bool field2, int stale_limit,
                   int* iters_out, int* nact_out, hipStream_t st) {
    struct Ops {
        vggp_ctx* c; VgMasked& w; const VgIter& it; double p; bool field2; hipStream_t st;
        int apply() { return vgi_apply(c, w, it, field2, st); }
        int precond() { return vgi_rot(c, w, it, it.R, it.Zp, 0, 0, p, st); }
        int dots(int phase) {
            const bool pAp = phase == 1;
            hipLaunchKernelGGL(vgi_coldots_kernel, dim3(it.nbc), dim3(256), 0, st, pAp ? it.Pd : it.R, pAp ? it.AP : it.Zp,
                               pAp ? (const double*)nullptr : it.R, pAp ? (const double*)nullptr : it.R, w.m1, it.nbc, w.m2, it.part,
                               pAp ? (double*)nullptr : it.part + it.nbc);
            return VGGP_OK;
        }
        int active(int* nact) {
            VG_HIP(hipMemcpyAsync(&c->h_out->counters[0][0], it.nact, sizeof(int), hipMemcpyDeviceToHost, st));
            VGI_WAIT(c, st);
            *nact = c->h_out->counters[0][0];                          // (from replicated block vectors: the same on every rank)
            return VGGP_OK;
        }
    };
    const VgBlockPcg b{it.X, it.R, it.Pd, it.AP, it.Zp, it.part, 1, it.col, it.nbc, it.alh, it.beh, it.nact, w.m1, it.nbc, w.m2, it.nbc,
                       /*count_at_start=*/false};
    const int rc = vg_block_pcg(b, Ops{c, w, it, p, field2, st}, tol, max_iter, history, stale_limit, iters_out, nact_out, st);
    if (rc == VG_PCG_ESTALE) w.ib_valid = false;                       // the kept basis has drifted too far: not worth iterating on
    return rc;
}

// Eigenbasis of the preconditioner from the Gram matrices G1, G2 of this step, into d.Qt / d.lam0; *reused: the kept basis serves.
// Everything the steps do is exact in expectation for ANY orthonormal Q_d and any positive
// dP = 1 + rho p l1 l2 -- P~ = (Q1 (x) Q2) diag(dP) (Q1 (x) Q2)^T is then simply another SPD preconditioner with a known
// determinant: log|Sigma~| = sum log dP + tr log(P~^-1/2 Sigma~ P~^-1/2), the exact traces are traces against P~^-1 -- so the
// cold Jacobi solve of G1, G2 (1.7 ms at m_d = 128, 74 ms at m_d = 256 where the solver works in global memory: 70 % of that
// step) runs only on the first step of a plan, every 64 steps, and when the PCG needed 4 iterations more than right after the
// last solve; in between the kept basis is reused with the Rayleigh quotients l_i = q_i^T G q_i of the CURRENT Gram matrices.
// A reused basis on which the PCG takes 12 iterations more than right after the last solve is given up inside the step
// (vgi_pcg's stale_limit, vgi_retry_stale).  VGGP_ITER_COLD_BASIS=1: solve every step.
static int vgi_basis(vggp_ctx* c, VgMasked& w, const VgIter& it, const double* G1, const double* G2, bool* reused, hipStream_t st) {
    static const bool always = getenv("VGGP_ITER_COLD_BASIS") != nullptr;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const double* G[2] = {G1, G2};
    int rc;
    // (not for RBF factors: rho lam1 lam2 spans eight decades there, and a basis that is 1e-2 off leaves P~^-1 Sigma~ with a
    //  condition number of 1e4 -- the PCG stalls; measured.  Matern spectra are flat enough: 8 -> 11 -> 13 iterations over 4 % drift)
    *reused = !always && w.ib_valid && w.ib_age < 64 && w.ib_last_its <= w.ib_ref_its + 4 && d1.kind != VGGP_KIND_RBF &&
              d2.kind != VGGP_KIND_RBF;
    if (*reused) {
        double* Qk[2] = {it.Qk1, it.Qk2};
        for (int k = 0; k < 2; ++k) {
            VgDim& d = c->d[k];
            VG_HIP(hipMemcpyAsync(d.Qt, Qk[k], sizeof(double) * d.m * d.m, hipMemcpyDeviceToDevice, st));
            if ((rc = gemm1(d.Qt, d.m, 1, G[k], d.m, 1, it.Tq, d.m, d.m, d.m, d.m, st))) return rc;         // Q^T-rows times G
            VGM_LAUNCH1D(vgi_rowdot_kernel, d.m, st, it.Tq, d.Qt, d.m, d.lam0);
        }
        ++w.ib_age;
        w.ib_fresh = false;
    } else {
        VgEigJob ej[2];
        for (int k = 0; k < 2; ++k) {
            VgDim& d = c->d[k];
            ej[k] = VgEigJob{G[k], d.lam0, d.Qt, nullptr, d.gwork, d.rotlog, d.roundlog, d.counters, d.m, d.max_rounds,
                             (long)vg_eigh_log_bytes(d.m), 0};
            ej[k].perm = d.perm;
            ej[k].err = d.status + 1;
        }
        VG_HIP(vg_eigh_launch(ej, 2, st));
        VG_HIP(hipMemcpyAsync(it.Qk1, d1.Qt, sizeof(double) * d1.m * d1.m, hipMemcpyDeviceToDevice, st));
        VG_HIP(hipMemcpyAsync(it.Qk2, d2.Qt, sizeof(double) * d2.m * d2.m, hipMemcpyDeviceToDevice, st));
        w.ib_valid = false;            // ... until this step has returned without an error
        w.ib_fresh = true;
    }
    return VGGP_OK;
}
// ... and its book-keeping at the end of a step that returned without an error
static void vgi_basis_done(VgMasked& w, int iters) {
    if (w.ib_fresh) { w.ib_valid = true; w.ib_age = 0; w.ib_ref_its = iters; }
    w.ib_last_its = iters;
}
// a step that gave its kept basis up (VG_PCG_ESTALE) runs once more, now with a cold solve
template <class Once>
static int vgi_retry_stale(const char* fn, Once&& once) {
    int rc = once();
    if (rc == VG_PCG_ESTALE) rc = once();
    if (rc == VG_PCG_ESTALE) { vg_set_error("%s: internal (stale basis after a cold solve)", fn); rc = VGGP_ESTATE; }
    return rc;
}

// right-hand sides (column 0 = c0, columns 1.. = z = P^1/2 z0;  Wz = P^-1 z = P^-1/2 z0) and the block solve Sigma~ X = R
static int vgi_step_solve(vggp_ctx* c, VgMasked& w, const VgIter& it, const char* fn, double* C0, double p, double tol, int max_iter,
                          bool reused, int* iters, hipStream_t st) {
    const int m1 = w.m1, m2 = w.m2, nbc = it.nbc;
    int rc, nact = 0;
    VGM_LAUNCH1D(vg_pcg_probe_kernel, w.M * nbc, st, it.X, (long)m1, nbc, m2, nbc, 0x5647475000000001ULL);
    if ((rc = vgi_rot(c, w, it, it.X, it.R, 1, 1, p, st))) return rc;
    if ((rc = vgi_rot(c, w, it, it.X, it.Wz, 2, 1, p, st))) return rc;
    VGM_LAUNCH1D(vgi_col_kernel, w.M, st, it.R, C0, m1, nbc, m2, 0, 0);
    if ((rc = vgi_pcg(c, w, it, p, tol, max_iter, /*history=*/true, /*field2=*/false, reused ? w.ib_ref_its + 12 : 0, iters, &nact, st))) return rc;
    if (nact > 0) { vg_set_error("%s: PCG did not reach %.1e in %d iterations (%d columns left)", fn, tol, max_iter, nact); return VGGP_ENOCONV; }
    return VGGP_OK;
}
// log det: ts[0] = log|P|, ts[1] = the sum of the probes' quadratures
static int vgi_logdet(vggp_ctx* c, VgMasked& w, const VgIter& it, double p, hipStream_t st) {
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    VG_HIP(hipMemsetAsync(it.ts, 0, VGI_NTS * sizeof(double), st));
    VG_HIP(hipMemsetAsync(w.cholstatus, 0, sizeof(int), st));
    hipLaunchKernelGGL(vgi_dpsum_kernel, dim3(1), dim3(256), 0, st, d1.lam0, d2.lam0, c->theta, p, w.m1, w.m2, (const double*)nullptr,
                       (const double*)nullptr, (const double*)nullptr, 1, it.ts + 0);
    hipLaunchKernelGGL(vgi_slq_kernel, dim3(1), dim3(64), 0, st, it.alh, it.beh, it.col, it.nbc, (double)w.M, it.pc, w.cholstatus);
    hipLaunchKernelGGL(vgi_sum_kernel, dim3(1), dim3(64), 0, st, it.pc, it.nbc - 1, it.ts + 1, 0);
    return VGGP_OK;
}
// stochastic parts of the traces: fields of dU and of Wz with (B1,B2), (V1,B2), (B1,V2).  field(L, V, R, F): F = the field l^T V r of
// the data kind; fsum(Fa, Fb, out): out = the sum of Fa Fb over the probe columns and the observations
template <class Field, class FSum>
static int vgi_field_terms(vggp_ctx* c, const VgMasked& w, const VgIter& it, const double* dU, Field&& field, FSum&& fsum) {
    const double *B1 = c->d[0].BV, *V1 = B1 + (long)w.m1 * w.n1, *B2 = c->d[1].BV, *V2 = B2 + (long)w.m2 * (w.scattered ? w.n1 : w.n2);
    int rc;
    if ((rc = field(B1, it.Wz, B2, it.F0))) return rc;              // F0 = Fw^BB
    if ((rc = field(B1, dU, B2, it.F1))) return rc;                 // F1 = Fu^BB
    fsum(it.F1, it.F0, it.ts + 3);
    if ((rc = field(V1, dU, B2, it.F2))) return rc;                 // Fu^VB
    fsum(it.F2, it.F0, it.ts + 6);                                  // (u-w)^T Phi'_1^T w
    if ((rc = field(B1, dU, V2, it.F2))) return rc;                 // Fu^BV
    fsum(it.F2, it.F0, it.ts + 9);
    if ((rc = field(V1, it.Wz, B2, it.F0))) return rc;              // Fw^VB
    fsum(it.F1, it.F0, it.ts + 5);
    if ((rc = field(B1, it.Wz, V2, it.F0))) return rc;              // Fw^BV
    fsum(it.F1, it.F0, it.ts + 8);
    return VGGP_OK;
}
// Mk terms: ts[11] = <dU, Mk1 Wz>, ts[13] = <dU, Wz Mk2^T> over the probe columns
static int vgi_mk_terms(vggp_ctx* c, const VgMasked& w, const VgIter& it, const double* dU, hipStream_t st) {
    const int m1 = w.m1, m2 = w.m2, nbc = it.nbc;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    int rc;
    if ((rc = gemm1(d1.Mk, m1, 1, it.Wz, (long)nbc * m2, 1, it.Tm, nbc * m2, m1, nbc * m2, m1, st))) return rc;
    hipLaunchKernelGGL(vgi_coldots_kernel, dim3(nbc), dim3(256), 0, st, dU, it.Tm, (const double*)nullptr, (const double*)nullptr, m1, nbc, m2,
                       it.pc, (double*)nullptr);
    hipLaunchKernelGGL(vgi_sum_kernel, dim3(1), dim3(64), 0, st, it.pc, nbc, it.ts + 11, 1);
    if ((rc = gemm1(it.Wz, m2, 1, d2.Mk, 1, m2, it.Tm, m2, m1 * nbc, m2, m2, st))) return rc;
    hipLaunchKernelGGL(vgi_coldots_kernel, dim3(nbc), dim3(256), 0, st, dU, it.Tm, (const double*)nullptr, (const double*)nullptr, m1, nbc, m2,
                       it.pc, (double*)nullptr);
    hipLaunchKernelGGL(vgi_sum_kernel, dim3(1), dim3(64), 0, st, it.pc, nbc, it.ts + 13, 1);
    return VGGP_OK;
}
// exact parts: the factors rotated into the eigenbasis of P (Rr_d = Q_d^T B_d, Rv_d = Q_d^T V_d) and their products RR_d = Rr_d o Rr_d,
// RRV_d = Rr_d o Rv_d
static int vgi_rotate_factors(vggp_ctx* c, const VgMasked& w, const VgIter& it, hipStream_t st) {
    const int m1 = w.m1, m2 = w.m2;
    const long n1 = w.n1, n2 = w.scattered ? w.n1 : w.n2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const double *B1 = d1.BV, *V1 = B1 + m1 * n1, *B2 = d2.BV, *V2 = B2 + m2 * n2;
    int rc;
    if ((rc = gemm1(d1.Qt, m1, 1, B1, n1, 1, it.Rr1, (int)n1, m1, (int)n1, m1, st))) return rc;
    if ((rc = gemm1(d1.Qt, m1, 1, V1, n1, 1, it.Rv1, (int)n1, m1, (int)n1, m1, st))) return rc;
    if ((rc = gemm1(d2.Qt, m2, 1, B2, n2, 1, it.Rr2, (int)n2, m2, (int)n2, m2, st))) return rc;
    if ((rc = gemm1(d2.Qt, m2, 1, V2, n2, 1, it.Rv2, (int)n2, m2, (int)n2, m2, st))) return rc;
    VGM_LAUNCH1D(vgi_mul_kernel, m1 * n1, st, it.Rr1, it.Rr1, m1 * n1, it.RR1);
    VGM_LAUNCH1D(vgi_mul_kernel, m1 * n1, st, it.Rr1, it.Rv1, m1 * n1, it.RRV1);
    VGM_LAUNCH1D(vgi_mul_kernel, m2 * n2, st, it.Rr2, it.Rr2, m2 * n2, it.RR2);
    VGM_LAUNCH1D(vgi_mul_kernel, m2 * n2, st, it.Rr2, it.Rv2, m2 * n2, it.RRV2);
    return VGGP_OK;
}
// out[0] = sum (1 / dP) o Ex for the m1 x m2 product the data kind has left in it.Ex
static void vgi_exact_sum(vggp_ctx* c, const VgMasked& w, const VgIter& it, double p, double* out, hipStream_t st) {
    hipLaunchKernelGGL(vgi_dpsum_kernel, dim3(1), dim3(256), 0, st, c->d[0].lam0, c->d[1].lam0, c->theta, p, w.m1, w.m2, it.Ex,
                       (const double*)nullptr, (const double*)nullptr, 0, out);
}
// ts[10] = tr(P^-1 (Mk1 (x) I)) = sum_ab diag(Q1^T Mk1 Q1)_a / dP_ab, ts[12]: likewise dimension 2
static int vgi_mk_traces(vggp_ctx* c, const VgMasked& w, const VgIter& it, double p, hipStream_t st) {
    const int m1 = w.m1, m2 = w.m2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    int rc;
    if ((rc = gemm1(d1.Qt, m1, 1, d1.Mk, m1, 1, it.Tq, m1, m1, m1, m1, st))) return rc;
    VGM_LAUNCH1D(vgi_rowdot_kernel, m1, st, it.Tq, d1.Qt, m1, it.dg1);
    if ((rc = gemm1(d2.Qt, m2, 1, d2.Mk, m2, 1, it.Tq, m2, m2, m2, m2, st))) return rc;
    VGM_LAUNCH1D(vgi_rowdot_kernel, m2, st, it.Tq, d2.Qt, m2, it.dg2);
    hipLaunchKernelGGL(vgi_dpsum_kernel, dim3(1), dim3(256), 0, st, d1.lam0, d2.lam0, c->theta, p, m1, m2, (const double*)nullptr, it.dg1,
                       (const double*)nullptr, 0, it.ts + 10);
    hipLaunchKernelGGL(vgi_dpsum_kernel, dim3(1), dim3(256), 0, st, d1.lam0, d2.lam0, c->theta, p, m1, m2, (const double*)nullptr,
                       (const double*)nullptr, it.dg2, 0, it.ts + 12);
    return VGGP_OK;
}
// The dense step's reductions that do not involve Sigma~^-1 as a matrix (the six that do come from the combine kernel): the ones both
// data kinds share.  The drivers add RJ_TRPHI, RJ_Z1, RJ_HV1, RJ_Z2, RJ_HV2 over their observations.
static void vgi_red_job(VgmRedArgs& ra, int k, const double* a, const double* b, long n, long sa, long sb, int op, const double* cc = nullptr) {
    ra.job[k] = VgmRedJob{a, b, cc, n, sa, sb, op};
}
static void vgi_red_jobs(vggp_ctx* c, const VgMasked& w, const double* C0, VgmRedArgs& ra) {
    const long m1 = w.m1, m2 = w.m2, M = w.M;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const double *C1 = C0 + M, *C2 = C1 + M;
    ra.njobs = RJ_COUNT;
    ra.partial = w.partial;
    for (int k = 0; k < RJ_COUNT; ++k) vgi_red_job(ra, k, w.a0, w.a0, 0, 1, 1, 0);
    vgi_red_job(ra, RJ_Q, C0, w.a0, M, 1, 1, 0);
    vgi_red_job(ra, RJ_AA, w.a0, w.a0, M, 1, 1, 0);
    vgi_red_job(ra, RJ_TRMK1, d1.Mk, nullptr, m1, m1 + 1, 0, 2);
    vgi_red_job(ra, RJ_AC1, w.a0, C1, M, 1, 1, 0);
    vgi_red_job(ra, RJ_MKA1, w.MkA1, w.a0, M, 1, 1, 0);
    vgi_red_job(ra, RJ_MK1PT, d1.Mk, w.PT1, m1 * m1, 1, 1, 0);
    vgi_red_job(ra, RJ_TRMK2, d2.Mk, nullptr, m2, m2 + 1, 0, 2);
    vgi_red_job(ra, RJ_AC2, w.a0, C2, M, 1, 1, 0);
    vgi_red_job(ra, RJ_MKA2, w.MkA2, w.a0, M, 1, 1, 0);
    vgi_red_job(ra, RJ_MK2PT, d2.Mk, w.PT2, m2 * m2, 1, 1, 0);
}
// reductions, combine, final, copy-back and the status of the step (`what`: "masked" / "scattered", n observations with sum of squares yy)
// local_mask: the reduction jobs that are sums over this rank's rows / points.  Multi-rank: those, rank 0's copy of the replicated
// jobs and ts[2 .. 9] travel in ONE all-reduce of w.scal before the combine kernel reads any of them
static int vgi_finish(vggp_ctx* c, VgMasked& w, const VgIter& it, const char* what, const VgmRedArgs& ra, unsigned local_mask, double n, double yy,
                      int iters, double* elbo_out, double grad_out[5], vggp_info* info, hipStream_t st) {
    const int n_probes = it.nbc - 1;
    const bool multi = vgi_multi(c);
    int rc;
    hipLaunchKernelGGL(vgm_red_kernel, dim3(VG_MD_NPART, RJ_COUNT), dim3(256), 0, st, ra);
    hipLaunchKernelGGL(vgm_sum_kernel, dim3(1), dim3(64), 0, st, w.partial, w.scal, local_mask, (!multi || c->rank == 0) ? 1 : 0);
    if (multi) {
        hipLaunchKernelGGL(vgi_pack_ts_kernel, dim3(1), dim3(64), 0, st, it.ts, w.scal, 0);
        if ((rc = vg_allreduce(c, w.scal, 32, st))) return rc;
        hipLaunchKernelGGL(vgi_pack_ts_kernel, dim3(1), dim3(64), 0, st, it.ts, w.scal, 1);
    }
    hipLaunchKernelGGL(vgi_combine_kernel, dim3(1), dim3(64), 0, st, it.ts, c->theta, (double)w.M, n_probes, w.scal);
    VgmFinalArgs fa{c->theta, w.scal, w.out, n, yy, w.m1, w.m2};
    hipLaunchKernelGGL(vgm_final_kernel, dim3(1), dim3(64), 0, st, fa);
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(c->h_out->out, w.out, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
    for (int k = 0; k < 2; ++k) {
        VG_HIP(hipMemcpyAsync(&c->h_out->jitter[k], c->d[k].jitter, sizeof(double), hipMemcpyDeviceToHost, st));
        VG_HIP(hipMemcpyAsync(&c->h_out->status[k], c->d[k].status, sizeof(int), hipMemcpyDeviceToHost, st));
        VG_HIP(hipMemcpyAsync(&c->h_out->counters[k][2], c->d[k].counters + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    VG_HIP(hipMemcpyAsync(&c->h_out->counters[1][3], w.cholstatus, sizeof(int), hipMemcpyDeviceToHost, st));
    VGI_WAIT(c, st);
    *elbo_out = c->h_out->out[0];
    for (int i = 0; i < 5; ++i) grad_out[i] = c->h_out->out[1 + i];
    int status = c->h_out->status[0] ? c->h_out->status[0] : (c->h_out->status[1] ? c->h_out->status[1] : 0);
    if (!status) status = c->h_out->counters[0][2] ? c->h_out->counters[0][2] : c->h_out->counters[1][2];
    if (info) {
        info->jitter1 = c->h_out->jitter[0]; info->jitter2 = c->h_out->jitter[1];
        info->sweeps1 = n_probes; info->sweeps2 = 0; info->rounds1 = iters; info->rounds2 = 0;
        info->status = status; info->polished = 0;
    }
    if (status == VGGP_ENOTPD) { vg_set_error("iterative %s step: a factor is not positive definite", what); return VGGP_ENOTPD; }
    if (status) { vg_set_error("iterative %s step: the preconditioner's eigensolver failed (status %d)", what, status); return VGGP_ENOCONV; }
    if (c->h_out->counters[1][3]) { vg_set_error("iterative %s step: the Lanczos quadrature failed (code %d)", what, c->h_out->counters[1][3]); return VGGP_ENOCONV; }
    vgi_basis_done(w, iters);
    c->have_step = false; c->have_partials = false;
    c->have_iter = true;             // a0, the factors and the preconditioner's basis are there for the iterative read-outs
    return VGGP_OK;
}

// ---- the masked step -------------------------------------------------------------------------------------------------------------------
static int masked_iter_once(vggp_ctx* c, const double* Ym, const double* W, double n_obs, double yy_obs, const double theta[5],
                            int n_probes, double tol, int max_iter, double* elbo_out, double grad_out[5], vggp_info* info, void* stream) {
    static const char* fn = "vggp_elbo_step_masked_iter";
    if (!c || !c->planned) { vg_set_error("vggp_elbo_step_masked_iter: context not planned"); return VGGP_ESTATE; }
    VG_REQUIRE(Ym && W && theta && elbo_out && grad_out, "vggp_elbo_step_masked_iter: null argument");
    c->have_masked = false;
    c->have_iter = false;            // ... and a failed iterative step leaves nothing for vggp_qv_masked_iter / vggp_posterior_masked_iter
    VG_REQUIRE(!(c->desc.flags & VGGP_FLAG_SCATTERED), "vggp_elbo_step_masked_iter: the context was planned for scattered points");
    { const int vrc_ = vg_comm_verify(c, fn); if (vrc_) return vrc_; }
    if (n_probes <= 0) n_probes = 16;
    if (max_iter <= 0) max_iter = 100;
    if (!(tol > 0.0)) tol = 1e-10;
    VG_REQUIRE(n_probes <= 63 && max_iter <= VGI_MAXIT, "vggp_elbo_step_masked_iter: n_probes <= 63, max_iter <= %d", VGI_MAXIT);
    const long m1 = c->desc.m1, m2 = c->desc.m2, n1 = c->desc.n1, n2 = c->desc.n2, M = m1 * m2;
    const int nbc = n_probes + 1;
    VG_REQUIRE(n1 * nbc * n2 < (1L << 31) * 4 && n1 * nbc < (1L << 31) && M * nbc < (1L << 31), "vggp_elbo_step_masked_iter: problem too large");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    for (int i = 0; i < 5; ++i) {
        VG_REQUIRE(theta[i] > 0.0 && std::isfinite(theta[i]), "theta[%d]=%g must be positive and finite", i, theta[i]);
        c->h_theta[i] = theta[i];
    }
    int rc = vgm_prepare(c, /*iter=*/true);
    if (rc) return rc;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    VgIter it;
    if ((rc = vgi_prepare(w, it, nbc, max_iter))) return rc;
    // factors, Cholesky, B|V, Mk, the projections C0, C1, C2 and the full-grid Gram matrices G1 (d1.GH), G2 (mpay)
    if ((rc = vg_partials_enqueue(c, Ym, w.mpay, st))) return rc;
    double* C0 = w.mpay + 2 * m2 * m2;
    if ((rc = vgm_colstats(c, w, W, st))) return rc;
    hipLaunchKernelGGL(vgi_transpose_kernel, dim3((unsigned)((n1 + 31) / 32), (unsigned)((n2 + 31) / 32)), dim3(32, 8), 0, st, W, n1, n2, it.Wt);
    // row-sharded job: G2 (H2), C0, C1, C2 and wn2 are sums over this rank's rows and lie side by side in w.mpay -- the ONE collective
    // before the solve; G1 runs over the unsharded axis and is replicated as it is
    if ((rc = vg_allreduce(c, w.mpay, 2 * m2 * m2 + 3 * M + n1, st))) return rc;
    bool reused = false;
    if ((rc = vgi_basis(c, w, it, c->d[0].GH, w.mpay, &reused, st))) return rc;
    const double p = vgi_obs_fraction(c, false, n_obs);
    int iters = 0;
    if ((rc = vgi_step_solve(c, w, it, fn, C0, p, tol, max_iter, reused, &iters, st))) return rc;
    if ((rc = vgi_logdet(c, w, it, p, st))) return rc;
    // a0 and the a0 terms of the gradient
    VGM_LAUNCH1D(vgi_col_kernel, M, st, it.X, w.a0, (int)m1, nbc, (int)m2, 0, 1);
    if ((rc = vgm_a0_terms(c, w, st))) return rc;
    // dU = Sigma~^-1 z - P^-1 z (probe columns); the control variates' fields are weighted by the mask
    VGM_LAUNCH1D(vgi_sub_kernel, M * nbc, st, it.X, it.Wz, M * nbc, it.Zp);
    const double* dU = it.Zp;
    auto field = [&](const double* L, const double* V, const double* R, double* F) { return vgi_field(w, it, L, V, R, F, st); };
    auto fsum = [&](const double* Fa, const double* Fb, double* out) {
        hipLaunchKernelGGL(vgi_fieldsum_part_kernel, dim3(1024), dim3(256), 0, st, Fa, Fb, it.Wt, n1, nbc, n2, it.fpart);
        hipLaunchKernelGGL(vgi_sum_kernel, dim3(1), dim3(64), 0, st, it.fpart, 1024, out, 0);
    };
    if ((rc = vgi_field_terms(c, w, it, dU, field, fsum))) return rc;
    if ((rc = vgi_mk_terms(c, w, it, dU, st))) return rc;
    // exact parts tr(P^-1 Phi(.)): the mask enters through TW = Wt RR2^T (n1 x m2), then one m1 x m2 product over the n1 rows each
    if ((rc = vgi_rotate_factors(c, w, it, st))) return rc;
    if ((rc = gemm1(it.Wt, n2, 1, it.RR2, 1, n2, it.TW, (int)m2, (int)n1, (int)m2, (int)n2, st))) return rc;
    if ((rc = gemm1(it.Wt, n2, 1, it.RRV2, 1, n2, it.TWv, (int)m2, (int)n1, (int)m2, (int)n2, st))) return rc;
    auto exact = [&](const double* RRa, const double* TWb, double* out) -> int {
        int r2 = gemm_longk(RRa, n1, 1, TWb, m2, 1, it.Ex, (int)m1, (int)m2, (int)n1, w.T, st);
        if (r2) return r2;
        vgi_exact_sum(c, w, it, p, out, st);
        return VGGP_OK;
    };
    if ((rc = exact(it.RR1, it.TW, it.ts + 2))) return rc;
    if ((rc = exact(it.RRV1, it.TW, it.ts + 4))) return rc;
    if ((rc = exact(it.RR1, it.TWv, it.ts + 7))) return rc;
    if ((rc = vgi_mk_traces(c, w, it, p, st))) return rc;
    VgmRedArgs ra;
    vgi_red_jobs(c, w, C0, ra);
    vgi_red_job(ra, RJ_TRPHI, w.nb1, w.wn2, n1, 1, 1, 0);
    vgi_red_job(ra, RJ_Z1, W, w.Zb, n1 * n2, 1, 1, 3, w.Zv1);
    vgi_red_job(ra, RJ_HV1, w.hv1, w.wn2, n1, 1, 1, 0);
    vgi_red_job(ra, RJ_Z2, W, w.Zb, n1 * n2, 1, 1, 3, w.Zv2);
    vgi_red_job(ra, RJ_HV2, w.hv2, w.wn1, n2, 1, 1, 0);
    // (the dense masked step's: wn2 is all-reduced, so the jobs over n1 and PT1 are replicated; wn1 and PT2 belong to this rank's rows)
    const unsigned local_mask = (1u << RJ_Z1) | (1u << RJ_Z2) | (1u << RJ_HV2) | (1u << RJ_MK2PT);
    return vgi_finish(c, w, it, "masked", ra, local_mask, n_obs, yy_obs, iters, elbo_out, grad_out, info, st);
}
extern "C" int vggp_elbo_step_masked_iter(vggp_ctx* c, const double* Ym, const double* W, double n_obs, double yy_obs, const double theta[5],
                                          int n_probes, double tol, int max_iter, double* elbo_out, double grad_out[5], vggp_info* info,
                                          void* stream) {
    VG_NOT_PAIRED(c, "vggp_elbo_step_masked_iter");
    return vgi_retry_stale("vggp_elbo_step_masked_iter", [&] {
        return masked_iter_once(c, Ym, W, n_obs, yy_obs, theta, n_probes, tol, max_iter, elbo_out, grad_out, info, stream);
    });
}

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
struct VgReadout {
    VgIter it;                  // the block vectors the step's helpers work on (alh, beh: one row each; no Wz; the rest of VgIter unused)
    double p;                   // the step's observed fraction (scattered: 1 / N)
    double *T;                  // the right-hand sides, kept for the reductions
    double *A1, *A2, *U1, *U2;  // posterior(x*): factor columns a_d(x*) and U_d = L0_d^-1 a_d  [m_d][cn]
    long long* cells;           // q(v): this block's flat cell indices
    double* mean;               // joint samples: the q(v) mean every sample starts from  [m1][m2]
};

// T[a][c][b] = U1[a][c] U2[b][c] for the cn columns of this block (U_d: [m_d][cn]); the unused columns of a ragged block are zero
__global__ void vgi_rank1_kernel(const double* U1, const double* U2, int m1, int nbc, int m2, int cn, double* T) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)m1 * nbc * m2) return;
    const int b = (int)(idx % m2), c = (int)((idx / m2) % nbc), a = (int)(idx / ((long)m2 * nbc));
    T[idx] = c < cn ? U1[(long)a * cn + c] * U2[(long)b * cn + c] : 0.0;
}
// q(v): column c belongs to cell u = cells[c] (or u0 + c): T[a][c][b] = L0_1[i1][a] L0_2[i2][b], u = i1 m2 + i2
__global__ void vgi_rank1_cells_kernel(const double* L1, const double* L2, const long long* cells, long u0, int m1, int nbc, int m2, int cn,
                                       double* T) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)m1 * nbc * m2) return;
    const int b = (int)(idx % m2), c = (int)((idx / m2) % nbc), a = (int)(idx / ((long)m2 * nbc));
    if (c >= cn) { T[idx] = 0.0; return; }
    const long u = cells ? (long)cells[c] : u0 + c;
    const long i1 = u / m2, i2 = u - i1 * m2;
    T[idx] = L1[i1 * m1 + a] * L2[i2 * m2 + b];
}
// one workgroup per column: lin = <T, a0>, nrm = <T, T>, quad = <T, X> in one pass, then the scaled outputs of the column.
// mode 0 (posterior): mean = (s1 s2 / v) lin, var = s1 s2 (1 - nrm + quad);   mode 1 (q(v)): var = s1^e1 s2^e2 quad
__global__ __launch_bounds__(256) void vgi_readout_reduce_kernel(const double* T, const double* X, const double* a0, int m1, int nbc, int m2,
                                                                 const double* theta, int mode, int e1, int e2, double* mean, double* var) {
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
        const double ss = theta[2] * theta[3];
        if (mode == 0) {
            mean[c] = (ss / theta[4]) * lin;
            var[c] = ss * (1.0 - nrm + quad);
        } else {
            var[c] = (e1 > 0 ? theta[2] : 1.0 / theta[2]) * (e2 > 0 ? theta[3] : 1.0 / theta[3]) * quad;
        }
    }
}

// q(v) mean of every cell from the a0 an iterative step left: L0_1 A0 L0_2^T, scaled as vggp_qv_masked scales it (two GEMMs, no solve)
static int vgi_qv_mean(vggp_ctx* c, VgMasked& w, double* mean, hipStream_t st) {
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
static int vgi_whitened_columns(vggp_ctx* c, const double* xs1, const double* xs2, int cn, double* A1, double* A2, double* U1, double* U2,
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
    else {
        VG_REQUIRE((ncols == 0 && !var) || (ncols > 0 && var), "%s: var and n_cells must be given together (NULL with 0: mean only)", fn);
        VG_REQUIRE(cells || ncols == 0 || ncols == M, "%s: cells = NULL means every cell: n_cells must be M = %ld", fn, M);
        if (cells)
            for (int64_t k = 0; k < ncols; ++k)
                VG_REQUIRE(cells[k] >= 0 && cells[k] < M, "%s: cells[%lld] = %lld is outside [0, M = %ld)", fn, (long long)k, (long long)cells[k], M);
    }
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
            if ((rc = vgi_whitened_columns(c, xs1 + off, xs2 + off, cn, r.A1, r.A2, r.U1, r.U2, st))) return rc;
            VGM_LAUNCH1D(vgi_rank1_kernel, nb, st, r.U1, r.U2, (int)m1, nbc, (int)m2, cn, r.T);
        } else {
            if (cells) VG_HIP(hipMemcpyAsync(r.cells, cells + off, sizeof(long long) * cn, hipMemcpyHostToDevice, st));
            VGM_LAUNCH1D(vgi_rank1_cells_kernel, nb, st, d1.L0, d2.L0, cells ? r.cells : (const long long*)nullptr, (long)off, (int)m1, nbc, (int)m2,
                         cn, r.T);
        }
        if ((rc = vgi_solve_block(c, w, r, fn, tol, max_iter, &solves, &max_its, info, st))) return rc;
        hipLaunchKernelGGL(vgi_readout_reduce_kernel, dim3(cn), dim3(256), 0, st, r.T, it.X, w.a0, (int)m1, nbc, (int)m2, c->theta, mode, e1, e2,
                           mode == 0 ? mean + off : (double*)nullptr, var + off);
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

// ================================================================================================================================
// Iterative SCATTERED step (vggp_elbo_step_scattered_iter): the iterative masked step above with the sum over the observed grid nodes
// replaced by a sum over the points -- a Khatri-Rao operator instead of a masked Kronecker one,
//     Sigma~ V = V + rho sum_k b1_k (b1_k^T V b2_k) b2_k^T,
// applied by the two kernels of kr.hip (field: the per-point scalars; back: their weighted outer products), so that neither an
// M x M matrix nor an m_d x nbc x N / m_d^2 x N buffer exists.  Preconditioner P = I + (rho / N) G1 (x) G2, G_d = B_d B_d^T over the
// points (the independence approximation E[Phi] = G1 (x) G2 / N; exact for a full grid): the masked step's with p = 1 / N, the same
// kept-basis rules, probes, PCG, Lanczos quadrature and control-variate traces.  Every masked field W^T o (L^T V R) becomes the
// per-point vector l_k^T V r_k ([nbc][N]).  Specification: tests/scattered_iter_spec.py; scalar terms as elbo_step_scattered.
// ================================================================================================================================
// part[block] = sum over this block's share of a[i] b[i] (fixed order); summed by vgi_sum_kernel
__global__ __launch_bounds__(256) void vgs_dot_part_kernel(const double* a, const double* b, long n, double* part) {
    __shared__ double red[4];
    double s = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) s += a[i] * b[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void vgs_scale_mean_kernel(double* x, long n, const double* theta) {       // x *= s1 s2 / sigma^2
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= theta[2] * theta[3] / theta[4];
}

// entry checks shared by the step and its read-outs
static int vgs_check(vggp_ctx* c, const char* fn) {
    if (!c || !c->planned) { vg_set_error("%s: context not planned", fn); return VGGP_ESTATE; }
    VG_NOT_PAIRED(c, fn);
    VG_REQUIRE(c->desc.flags & VGGP_FLAG_SCATTERED, "%s: plan the context with VGGP_FLAG_SCATTERED", fn);
    return vg_comm_verify(c, fn);
}

static int scattered_iter_once(vggp_ctx* c, const double* y, double yy, const double theta[5], int n_probes, double tol, int max_iter,
                               double* elbo_out, double grad_out[5], vggp_info* info, void* stream) {
    static const char* fn = "vggp_elbo_step_scattered_iter";
    int rc = vgs_check(c, fn);
    if (rc) return rc;
    VG_REQUIRE(y && theta && elbo_out && grad_out, "%s: null argument", fn);
    c->have_masked = false;
    c->have_iter = false;
    if (n_probes <= 0) n_probes = 16;
    if (max_iter <= 0) max_iter = 100;
    if (!(tol > 0.0)) tol = 1e-10;
    VG_REQUIRE(n_probes <= 63 && max_iter <= VGI_MAXIT, "%s: n_probes <= 63, max_iter <= %d", fn, VGI_MAXIT);
    const long m1 = c->desc.m1, m2 = c->desc.m2, N = c->desc.n1, M = m1 * m2;
    const int nbc = n_probes + 1;
    VG_REQUIRE(N * nbc < (1L << 31) && M * nbc < (1L << 31), "%s: problem too large", fn);
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    for (int i = 0; i < 5; ++i) {
        VG_REQUIRE(theta[i] > 0.0 && std::isfinite(theta[i]), "theta[%d]=%g must be positive and finite", i, theta[i]);
        c->h_theta[i] = theta[i];
    }
    if ((rc = vgm_prepare(c, /*iter=*/true))) return rc;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    VgIter it;
    if ((rc = vgi_prepare(w, it, nbc, max_iter))) return rc;
    if ((rc = vg_partials_enqueue(c, nullptr, nullptr, st))) return rc;          // factors at the points: B|V, Mk (unit outputscale)
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const double *B1 = d1.BV, *V1 = d1.BV + m1 * N, *B2 = d2.BV, *V2 = d2.BV + m2 * N;
    double *C0 = w.mpay + 2 * m2 * m2, *C1 = C0 + M, *C2 = C1 + M;
    // projections C0 = B1 diag(y) B2^T, C1 = V1 diag(y) B2^T, C2 = B1 diag(y) V2^T and the per-point statistics: the dense step's
    VGM_LAUNCH1D(vgm_scalecols_kernel, m1 * N, st, B1, y, (int)m1, N, w.B1s);
    VGM_LAUNCH1D(vgm_scalecols_kernel, m1 * N, st, V1, y, (int)m1, N, w.UV);           // (UV is free until the a0 stage)
    if ((rc = gemm_longk(w.B1s, N, 1, B2, 1, N, C0, (int)m1, (int)m2, (int)N, w.T, st))) return rc;
    if ((rc = gemm_longk(w.UV, N, 1, B2, 1, N, C1, (int)m1, (int)m2, (int)N, w.T, st))) return rc;
    if ((rc = gemm_longk(w.B1s, N, 1, V2, 1, N, C2, (int)m1, (int)m2, (int)N, w.T, st))) return rc;
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, B1, B1, (int)m1, N, w.nb1);
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, B2, B2, (int)m2, N, w.nb2);
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, V1, B1, (int)m1, N, w.hv1);
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, V2, B2, (int)m2, N, w.hv2);
    // Gram matrices over the points, in the payload beside the projections: G2 | . | C0, C1, C2 | G1
    double *G1 = w.mpay + vgi_g1_offset(m1, m2), *G2 = w.mpay;
    if ((rc = gemm_longk(B1, N, 1, B1, 1, N, G1, (int)m1, (int)m1, (int)N, w.T, st))) return rc;
    if ((rc = gemm_longk(B2, N, 1, B2, 1, N, G2, (int)m2, (int)m2, (int)N, w.T, st))) return rc;
    // point-sharded job: all of them are sums over this rank's points -- the ONE collective before the solve (the gaps of the
    // payload hold zeros on every rank)
    if ((rc = vg_allreduce(c, w.mpay, (long)vgi_g1_offset(m1, m2) + m1 * m1, st))) return rc;
    bool reused = false;
    if ((rc = vgi_basis(c, w, it, G1, G2, &reused, st))) return rc;
    const double p = vgi_obs_fraction(c, true, 0.0);
    int iters = 0;
    if ((rc = vgi_step_solve(c, w, it, fn, C0, p, tol, max_iter, reused, &iters, st))) return rc;
    if ((rc = vgi_logdet(c, w, it, p, st))) return rc;
    // a0 and the a0 terms of the gradient (the dense scattered step's)
    VGM_LAUNCH1D(vgi_col_kernel, M, st, it.X, w.a0, (int)m1, nbc, (int)m2, 0, 1);
    if ((rc = gemm1(d1.Mk, m1, 1, w.a0, m2, 1, w.MkA1, (int)m2, (int)m1, (int)m2, (int)m1, st))) return rc;
    if ((rc = gemm1(w.a0, m2, 1, d2.Mk, m2, 1, w.MkA2, (int)m2, (int)m1, (int)m2, (int)m2, st))) return rc;
    if ((rc = gemm1(w.a0, m2, 1, B2, N, 1, w.UB, (int)N, (int)m1, (int)N, (int)m2, st))) return rc;
    if ((rc = gemm1(w.a0, m2, 1, V2, N, 1, w.UV, (int)N, (int)m1, (int)N, (int)m2, st))) return rc;
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, B1, w.UB, (int)m1, N, w.Zb);
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, V1, w.UB, (int)m1, N, w.Zv1);
    VGM_LAUNCH1D(vgm_coldot_kernel, N, st, B1, w.UV, (int)m1, N, w.Zv2);
    VGM_LAUNCH1D(vgm_scalecols_kernel, m1 * N, st, B1, w.nb2, (int)m1, N, w.B1s);
    VGM_LAUNCH1D(vgm_scalecols_kernel, m2 * N, st, B2, w.nb1, (int)m2, N, w.B2s);
    if ((rc = gemm_longk(w.B1s, N, 1, B1, 1, N, w.PT1, (int)m1, (int)m1, (int)N, w.T, st))) return rc;
    if ((rc = gemm_longk(w.B2s, N, 1, B2, 1, N, w.PT2, (int)m2, (int)m2, (int)N, w.T, st))) return rc;
    // dU = Sigma~^-1 z - P^-1 z (probe columns); the control variates' fields are per-point vectors [nbc][N]
    VGM_LAUNCH1D(vgi_sub_kernel, M * nbc, st, it.X, it.Wz, M * nbc, it.Zp);
    const double* dU = it.Zp;
    auto field = [&](const double* L, const double* V, const double* R, double* F) -> int {
        VG_HIP(vg_kr_field_launch(L, R, V, (int)m1, (int)m2, N, nbc, F, st));
        return VGGP_OK;
    };
    auto fsum = [&](const double* Fa, const double* Fb, double* out) {          // sum over the probe columns c >= 1 and the points
        hipLaunchKernelGGL(vgs_dot_part_kernel, dim3(1024), dim3(256), 0, st, Fa + N, Fb + N, N * nbc - N, it.fpart);
        hipLaunchKernelGGL(vgi_sum_kernel, dim3(1), dim3(64), 0, st, it.fpart, 1024, out, 0);
    };
    if ((rc = vgi_field_terms(c, w, it, dU, field, fsum))) return rc;
    if ((rc = vgi_mk_terms(c, w, it, dU, st))) return rc;
    // exact parts tr(P^-1 Phi(.)) = sum (1/dP) o ((Ra o Rb)(Sa o Sb)^T): one m1 x m2 GEMM over the points each
    if ((rc = vgi_rotate_factors(c, w, it, st))) return rc;
    auto exact = [&](const double* RRa, const double* RRb, double* out) -> int {
        int r2 = gemm_longk(RRa, N, 1, RRb, 1, N, it.Ex, (int)m1, (int)m2, (int)N, w.T, st);
        if (r2) return r2;
        vgi_exact_sum(c, w, it, p, out, st);
        return VGGP_OK;
    };
    if ((rc = exact(it.RR1, it.RR2, it.ts + 2))) return rc;
    if ((rc = exact(it.RRV1, it.RR2, it.ts + 4))) return rc;
    if ((rc = exact(it.RR1, it.RRV2, it.ts + 7))) return rc;
    if ((rc = vgi_mk_traces(c, w, it, p, st))) return rc;
    VgmRedArgs ra;
    vgi_red_jobs(c, w, C0, ra);
    vgi_red_job(ra, RJ_TRPHI, w.nb1, w.nb2, N, 1, 1, 0);
    vgi_red_job(ra, RJ_Z1, w.Zb, w.Zv1, N, 1, 1, 0);
    vgi_red_job(ra, RJ_HV1, w.hv1, w.nb2, N, 1, 1, 0);
    vgi_red_job(ra, RJ_Z2, w.Zb, w.Zv2, N, 1, 1, 0);
    vgi_red_job(ra, RJ_HV2, w.hv2, w.nb1, N, 1, 1, 0);
    // (the dense scattered step's: PT1, PT2 are sums over this rank's points and enter through their scalars <Mk_d, PT_d> alone)
    const unsigned local_mask = (1u << RJ_TRPHI) | (1u << RJ_Z1) | (1u << RJ_HV1) | (1u << RJ_MK1PT) | (1u << RJ_Z2) | (1u << RJ_HV2) |
                                (1u << RJ_MK2PT);
    const long Ntot = (vgi_multi(c) && c->desc.n_total > N) ? c->desc.n_total : N;          // the observation count over all ranks
    return vgi_finish(c, w, it, "scattered", ra, local_mask, (double)Ntot, yy, iters, elbo_out, grad_out, info, st);
}

extern "C" int vggp_elbo_step_scattered_iter(vggp_ctx* c, const double* y, double yy, const double theta[5], int n_probes, double tol,
                                             int max_iter, double* elbo_out, double grad_out[5], vggp_info* info, void* stream) {
    return vgi_retry_stale("vggp_elbo_step_scattered_iter", [&] {
        return scattered_iter_once(c, y, yy, theta, n_probes, tol, max_iter, elbo_out, grad_out, info, stream);
    });
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
        if ((rc = vgi_whitened_columns(c, xs1 + off, xs2 + off, cn, A1, A2, U1, U2, st))) return rc;
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
static int vgi_sample_run(vggp_ctx* c, const char* fn, bool scattered, const double* W, double n_obs, int64_t n_samples, uint64_t seed,
                          int64_t first, const double* eps_u, const double* eps_obs, double tol, int max_iter, int block, double* out,
                          vggp_info* info, void* stream) {
    if (c && c->planned && !c->is_paired)
        VG_REQUIRE(!vgi_multi(c), "%s: joint samples run on single-rank contexts only (this context is multi-rank)", fn);
    int rc = vgi_readout_enter(c, fn, scattered, /*gridded=*/false, "plan the context with VGGP_FLAG_SCATTERED", "the context was planned for scattered points",
                               "bad argument", W, n_obs, block);
    if (rc) return rc;
    VG_REQUIRE(n_samples >= 1 && n_samples < (1LL << 31), "%s: n_samples = %lld must be at least 1", fn, (long long)n_samples);
    VG_REQUIRE(first >= 0 && out, "%s: bad argument", fn);
    VG_REQUIRE((eps_u == nullptr) == (eps_obs == nullptr), "%s: eps_u and eps_obs are either both NULL (generated noise) or both given", fn);
    if ((rc = vgi_readout_defaults(c, fn, scattered, &block, &tol, &max_iter, info))) return rc;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const int m1 = w.m1, m2 = w.m2, e1 = vg_uexp(d1.basis), e2 = vg_uexp(d2.basis);
    const long M = w.M, n1 = w.n1, n2 = w.n2;
    const long nodes = scattered ? n1 : n1 * n2;
    const int nbc = (int)std::min<int64_t>(block, n_samples);
    VgReadout r;
    if ((rc = vgi_readout_prepare(c, w, r, nbc, false, W, n_obs, st, /*sample=*/true))) return rc;
    VgIter& it = r.it;
    if ((rc = vgi_qv_mean(c, w, r.mean, st))) return rc;
    const long nb = M * nbc;
    int max_its = 0, solves = 0;
    for (int64_t off = 0; off < n_samples; off += nbc) {
        const int cn = (int)std::min<int64_t>(nbc, n_samples - off);
        const unsigned long long s0 = (unsigned long long)(first + off);
        VG_HIP(vg_sample_block_noise_launch(r.T, eps_u ? eps_u + off * M : nullptr, seed, s0, m1, nbc, m2, cn, st));
        VG_HIP(vg_sample_field_noise_launch(it.F0, scattered ? nullptr : it.Wt, eps_obs ? eps_obs + off * nodes : nullptr, seed, s0, n1, nbc, n2, cn,
                                            st));
        if (scattered) VG_HIP(vg_kr_back_launch(d1.BV, d2.BV, it.F0, m1, m2, n1, nbc, it.AP, it.krs, st));
        else if ((rc = vgi_back(w, it, d1.BV, it.F0, d2.BV, it.AP, st))) return rc;
        VG_HIP(vg_sample_fuse_launch(r.T, it.AP, c->theta, nb, st));                                               // Z = E + sqrt(rho) K F
        if ((rc = vgi_solve_block(c, w, r, fn, tol, max_iter, &solves, &max_its, info, st))) return rc;
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

// building blocks, exported for tests: the two kernels of kr.hip on caller-supplied device arrays
extern "C" int vggp_kr_field(vggp_ctx* c, const double* L, const double* R, const double* V, int64_t m1, int64_t m2, int64_t N, int64_t nb,
                             double* F, void* stream) {
    if (!c) { vg_set_error("vggp_kr_field: null context"); return VGGP_EINVAL; }
    VG_REQUIRE(L && R && V && F, "vggp_kr_field: null argument");
    VG_REQUIRE(m1 >= 1 && m1 <= 256 && m2 >= 1 && m2 <= 256 && nb >= 1 && nb <= 64 && N >= 1 && N < (1L << 24),
               "vggp_kr_field: need 1 <= m_d <= 256, 1 <= nb <= 64, 1 <= N < 2^24");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VG_HIP(vg_kr_field_launch(L, R, V, (int)m1, (int)m2, (long)N, (int)nb, F, st));
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}
// the two-column instantiation of the field kernel (bitwise equal to vggp_kr_field; the read-outs' block solves run it)
extern "C" int vggp_kr_field2(vggp_ctx* c, const double* L, const double* R, const double* V, int64_t m1, int64_t m2, int64_t N, int64_t nb,
                              double* F, void* stream) {
    if (!c) { vg_set_error("vggp_kr_field2: null context"); return VGGP_EINVAL; }
    VG_REQUIRE(L && R && V && F, "vggp_kr_field2: null argument");
    VG_REQUIRE(m1 >= 1 && m1 <= 256 && m2 >= 1 && m2 <= 256 && nb >= 1 && nb <= 64 && N >= 1 && N < (1L << 24),
               "vggp_kr_field2: need 1 <= m_d <= 256, 1 <= nb <= 64, 1 <= N < 2^24");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VG_HIP(vg_kr_field2_launch(L, R, V, (int)m1, (int)m2, (long)N, (int)nb, F, st));
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}
extern "C" int vggp_kr_back(vggp_ctx* c, const double* L, const double* R, const double* F, int64_t m1, int64_t m2, int64_t N, int64_t nb,
                            double* out, void* stream) {
    if (!c) { vg_set_error("vggp_kr_back: null context"); return VGGP_EINVAL; }
    VG_REQUIRE(L && R && F && out, "vggp_kr_back: null argument");
    VG_REQUIRE(m1 >= 1 && m1 <= 256 && m2 >= 1 && m2 <= 256 && nb >= 1 && nb <= 64 && N >= 1 && N < (1L << 24),
               "vggp_kr_back: need 1 <= m_d <= 256, 1 <= nb <= 64, 1 <= N < 2^24");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const size_t sc = vg_kr_back_scratch((int)m1, (int)m2, (long)N, (int)nb);
    int rc = vg_ensure_misc(c, (sc + 32) * sizeof(double));
    if (rc) return rc;
    VG_HIP(vg_kr_back_launch(L, R, F, (int)m1, (int)m2, (long)N, (int)nb, out, (double*)c->misc, st));
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}
extern "C" int vggp_kr_sqgram(vggp_ctx* c, const double* P1, const double* P2, int64_t mv1, int64_t mv2, int64_t N, double* out, void* stream) {
    if (!c) { vg_set_error("vggp_kr_sqgram: null context"); return VGGP_EINVAL; }
    VG_REQUIRE(P1 && P2 && out, "vggp_kr_sqgram: null argument");
    VG_REQUIRE(mv1 >= 1 && mv2 >= 1 && mv1 < (1L << 20) && mv2 < (1L << 20) && mv1 * mv2 < (1L << 28) && N >= 1 && N < (1L << 31) - 64,
               "vggp_kr_sqgram: need mv_d >= 1, mv1 mv2 < 2^28, 1 <= N < 2^31");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    int rc = vg_ensure_misc(c, (vg_kr_sqgram_scratch((int)mv1, (int)mv2, (long)N) + 32) * sizeof(double));
    if (rc) return rc;
    VG_HIP(vg_kr_sqgram_launch(P1, P2, (int)mv1, (int)mv2, (long)N, out, (double*)c->misc, 0, st));
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
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
// T[i][c][j] = U1[i][a_c] U2[j][b_c], cell p_c = cells[c] (or p0 + c) = a mv2 + b; the unused columns of a ragged block are zero
__global__ void vgi_rank1_grid_kernel(const double* U1, const double* U2, const long long* cells, long p0, int m1, int nbc, int m2, long mv1,
                                      long mv2, int cn, double* T) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)m1 * nbc * m2) return;
    const int j = (int)(idx % m2), c = (int)((idx / m2) % nbc), i = (int)(idx / ((long)m2 * nbc));
    if (c >= cn) { T[idx] = 0.0; return; }
    const long p = cells ? (long)cells[c] : p0 + c;
    const long a = p / mv2, b = p - a * mv2;
    T[idx] = U1[(long)i * mv1 + a] * U2[(long)j * mv2 + b];
}
// one workgroup per column (vgi_readout_reduce_kernel with kd1[a] kd2[b] in place of kappa): var = s1 s2 (kd1_a kd2_b - <T,T> + <T,X>)
__global__ __launch_bounds__(256) void vgi_readout_reduce_grid_kernel(const double* T, const double* X, int m1, int nbc, int m2,
                                                                      const double* theta, const double* kd1, const double* kd2,
                                                                      const long long* cells, long p0, long mv2, double* var) {
    __shared__ double red[8];
    const int c = blockIdx.x;
    double nrm = 0.0, quad = 0.0;
    for (long e = threadIdx.x; e < (long)m1 * m2; e += 256) {
        const long a = e / m2, b = e - a * m2, o = (a * nbc + c) * m2 + b;
        const double t = T[o];
        nrm += t * t;
        quad += t * X[o];
    }
    for (int off = 32; off > 0; off >>= 1) { nrm += __shfl_xor(nrm, off); quad += __shfl_xor(quad, off); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = nrm; red[4 + (threadIdx.x >> 6)] = quad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        nrm = (red[0] + red[1]) + (red[2] + red[3]);
        quad = (red[4] + red[5]) + (red[6] + red[7]);
        const long p = cells ? (long)cells[c] : p0 + c;
        const long a = p / mv2, b = p - a * mv2;
        var[c] = theta[2] * theta[3] * (kd1[a] * kd2[b] - nrm + quad);
    }
}
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
    VG_REQUIRE((n_cells == 0 && !var) || (n_cells > 0 && var), "%s: var and n_cells must be given together (NULL with 0: mean only)", fn);
    VG_REQUIRE(mean || var, "%s: nothing to compute (mean and var are NULL)", fn);
    VG_REQUIRE(cells || n_cells == 0 || n_cells == ncell_all, "%s: cells = NULL means every cell: n_cells must be mv1 mv2 = %ld", fn, ncell_all);
    if (cells)
        for (int64_t k = 0; k < n_cells; ++k)
            VG_REQUIRE(cells[k] >= 0 && cells[k] < ncell_all, "%s: cells[%lld] = %lld is outside [0, mv1 mv2 = %ld)", fn, (long long)k,
                       (long long)cells[k], ncell_all);
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
    {   // U_d = Linv0_d C_d^T   (m_d x mv_d)
        VgGemmBatch g;
        vg_gemm_init(&g);
        vg_gemm_add(&g, d1.Linv0, m1, 1, C1, 1, m1, U1, (int)mv1, (int)m1, (int)mv1, (int)m1);
        vg_gemm_add(&g, d2.Linv0, m2, 1, C2, 1, m2, U2, (int)mv2, (int)m2, (int)mv2, (int)m2);
        VG_HIP(vg_gemm_launch(&g, st));
    }
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
        const long long* cl = dcells ? dcells + off : nullptr;
        VGM_LAUNCH1D(vgi_rank1_grid_kernel, nb, st, U1, U2, cl, (long)off, (int)m1, nbc, (int)m2, (long)mv1, (long)mv2, cn, r.T);
        if ((rc = vgi_solve_block(c, w, r, fn, tol, max_iter, &solves, &max_its, info, st))) return rc;
        hipLaunchKernelGGL(vgi_readout_reduce_grid_kernel, dim3(cn), dim3(256), 0, st, r.T, r.it.X, (int)m1, nbc, (int)m2, c->theta, kd1, kd2, cl,
                           (long)off, (long)mv2, var + off);
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
