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
#include "mspace_ws.h"
#include "lanczos_quad.h"

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
// the observed fraction of the preconditioner: n_obs / (grid nodes) resp. 1 / N, on a multi-rank context over ALL ranks (desc.n_total)
double vgi_obs_fraction(const vggp_ctx* c, bool scattered, double n_obs) {
    const long n1 = c->desc.n1, n2 = c->desc.n2, nt = vgi_multi(c) ? c->desc.n_total : 0;
    if (scattered) return 1.0 / (double)(nt > n1 ? nt : n1);
    return nt > n1 * n2 ? n_obs / (double)nt : n_obs / ((double)n1 * (double)n2);
}

// iterative scattered step: G1 sits behind [G2 | . | C0, C1, C2] in w.mpay, on a 256-byte boundary
static size_t vgi_g1_offset(long m1, long m2) { return ((size_t)(2 * m2 * m2 + 3 * m1 * m2) + 31) & ~size_t(31); }

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
int vgi_back(const VgMasked& w, const VgIter& it, const double* L, const double* F, const double* R, double* out, hipStream_t st) {
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
int vgi_pcg(vggp_ctx* c, VgMasked& w, const VgIter& it, double p, double tol, int max_iter, bool history, bool field2, int stale_limit,
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
void vgi_red_job(VgmRedArgs& ra, int k, const double* a, const double* b, long n, long sa, long sb, int op, const double* cc) {
    ra.job[k] = VgmRedJob{a, b, cc, n, sa, sb, op};
}
void vgi_red_jobs(vggp_ctx* c, const VgMasked& w, const double* C0, VgmRedArgs& ra) {
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
    c->last_kind = VG_LAST_ITER;
    c->have_iter = true;             // a0, the factors and the preconditioner's basis are there for the iterative read-outs
    return VGGP_OK;
}

// what both iterative steps take for n_probes, max_iter and tol left at zero, and their limits
static int vgi_step_limits(const char* fn, int* n_probes, int* max_iter, double* tol) {
    if (*n_probes <= 0) *n_probes = 16;
    if (*max_iter <= 0) *max_iter = 100;
    if (!(*tol > 0.0)) *tol = 1e-10;
    VG_REQUIRE(*n_probes <= VGI_MAX_PROBES && *max_iter <= VGI_MAXIT, "%s: n_probes <= %d, max_iter <= %d", fn, VGI_MAX_PROBES, VGI_MAXIT);
    return VGGP_OK;
}

// ---- the masked step -------------------------------------------------------------------------------------------------------------------
static int masked_iter_once(vggp_ctx* c, const double* Ym, const double* W, double n_obs, double yy_obs, const double theta[5],
                            int n_probes, double tol, int max_iter, double* elbo_out, double grad_out[5], vggp_info* info, void* stream) {
    static const char* fn = "vggp_elbo_step_masked_iter";
    if (!c || !c->planned) { vg_set_error("vggp_elbo_step_masked_iter: context not planned"); return VGGP_ESTATE; }
    VG_REQUIRE(Ym && W && theta && elbo_out && grad_out, "vggp_elbo_step_masked_iter: null argument");
    int rc = vgm_step_enter(c, theta);          // (a failed iterative step leaves nothing for vggp_qv_masked_iter / vggp_posterior_masked_iter)
    if (rc) return rc;
    VG_REQUIRE(!(c->desc.flags & VGGP_FLAG_SCATTERED), "vggp_elbo_step_masked_iter: the context was planned for scattered points");
    if ((rc = vg_comm_verify(c, fn))) return rc;
    if ((rc = vgi_step_limits(fn, &n_probes, &max_iter, &tol))) return rc;
    const long m1 = c->desc.m1, m2 = c->desc.m2, n1 = c->desc.n1, n2 = c->desc.n2, M = m1 * m2;
    const int nbc = n_probes + 1;
    VG_REQUIRE(n1 * nbc * n2 < (1L << 31) * 4 && n1 * nbc < (1L << 31) && M * nbc < (1L << 31), "vggp_elbo_step_masked_iter: problem too large");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    if ((rc = vgm_prepare(c, /*iter=*/true))) return rc;
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
        int r2 = gemm_longk(RRa, n1, 1, TWb, m2, 1, it.Ex, (int)m1, (int)m2, (int)n1, w.T, w.Tcap, st);
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

// entry checks shared by the step and its read-outs
int vgs_check(vggp_ctx* c, const char* fn) {
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
    if ((rc = vgm_step_enter(c, theta))) return rc;
    if ((rc = vgi_step_limits(fn, &n_probes, &max_iter, &tol))) return rc;
    const long m1 = c->desc.m1, m2 = c->desc.m2, N = c->desc.n1, M = m1 * m2;
    const int nbc = n_probes + 1;
    VG_REQUIRE(N * nbc < (1L << 31) && M * nbc < (1L << 31), "%s: problem too large", fn);
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    if ((rc = vgm_prepare(c, /*iter=*/true))) return rc;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    VgIter it;
    if ((rc = vgi_prepare(w, it, nbc, max_iter))) return rc;
    if ((rc = vg_partials_enqueue(c, nullptr, nullptr, st))) return rc;          // factors at the points: B|V, Mk (unit outputscale)
    const double *B1 = c->d[0].BV, *B2 = c->d[1].BV;
    double* C0 = w.mpay + 2 * m2 * m2;
    // projections C0, C1, C2 and the per-point statistics: the dense step's
    if ((rc = vgs_projections(c, w, y, st))) return rc;
    // Gram matrices over the points, in the payload beside the projections: G2 | . | C0, C1, C2 | G1
    double *G1 = w.mpay + vgi_g1_offset(m1, m2), *G2 = w.mpay;
    if ((rc = gemm_longk(B1, N, 1, B1, 1, N, G1, (int)m1, (int)m1, (int)N, w.T, w.Tcap, st))) return rc;
    if ((rc = gemm_longk(B2, N, 1, B2, 1, N, G2, (int)m2, (int)m2, (int)N, w.T, w.Tcap, st))) return rc;
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
    if ((rc = vgs_a0_terms(c, w, st))) return rc;
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
        int r2 = gemm_longk(RRa, N, 1, RRb, 1, N, it.Ex, (int)m1, (int)m2, (int)N, w.T, w.Tcap, st);
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
