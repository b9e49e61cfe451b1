// Matrix-free kernel-matrix product of the exact GP: the building block of an iterative (conjugate-gradient) exact solver beyond the
// dense N <= 16384 of exact.hip.
//     out0[i][c] = sum_j K0(xr_i, xc_j) V[j][c],   out1, out2 = the same with dK0/d ell1, dK0/d ell2 (optional, same pass),
//     K0(a, b) = k1(|a1 - b1| / ell1) k2(|a2 - b2| / ell2) at unit outputscale (the K0 of exact.hip).
// K0 is never in memory: every lane generates its own A fragment of v_mfma_f64_16x16x4_f64 (one f64: row lane & 15, k lane >> 4)
// from the coordinates of its row, which stay in registers, and the coordinates of the current chunk of 64 columns, which are staged
// in LDS with the chunk's rows of V (the B fragments).  A workgroup owns 64 rows (4 waves x 16) and walks all columns in ascending
// order: no split reduction, no atomics, bitwise repeatable.  Each wave keeps nb16 = ceil(nb / 16) accumulators (x 3 in the derivative
// mode) and feeds all of them from one generated fragment.
// Every product of two kernels is a polynomial in a = |d1| / ell1, b = |d2| / ell2 times ONE exp of the summed exponents, and both
// length-scale derivatives share it; the kernel kinds are template parameters (dispatch per launch, nothing per element).
#include "arena.h"
#include "block_pcg.h"
#include "ctx.h"
#include "lanczos_quad.h"

#include <cmath>

#define EXI_ROWS 64           // rows per workgroup (4 waves x 16)
#define EXI_JC 64             // columns per LDS chunk (16 MFMA k-steps)
#define EXI_MAX_NB 64

typedef double exi_d4 __attribute__((ext_vector_type(4)));

// k(r) = p(r) exp(-g(r)),  dk/d ell = q(r) exp(-g(r)) / ell,  r = |d| / ell   (the profiles of vg_kappa, factor_elem.h)
template <int KIND, bool DER>
__device__ __forceinline__ void exi_profile(double r, double& p, double& q, double& g) {
    if constexpr (KIND == VGGP_KIND_MATERN12) {
        p = 1.0; g = r;
        if constexpr (DER) q = r;
    } else if constexpr (KIND == VGGP_KIND_MATERN32) {
        const double a = 1.7320508075688772 * r;
        p = 1.0 + a; g = a;
        if constexpr (DER) q = a * a;
    } else if constexpr (KIND == VGGP_KIND_MATERN52) {
        const double a = 2.23606797749979 * r;
        const double a3 = a * a * (1.0 / 3.0);
        p = 1.0 + a + a3; g = a;
        if constexpr (DER) q = a3 * (1.0 + a);
    } else {   // RBF
        const double r2 = r * r;
        p = 1.0; g = 0.5 * r2;
        if constexpr (DER) q = r2;
    }
}

struct ExiKmv {
    const double *xr1, *xr2, *xc1, *xc2;
    const double* V;          // [Nc][ldv], columns [0, nb) read
    double *o0, *o1, *o2;     // [Nr][ldo], columns [0, nb) written
    int Nr, Nc, nb;
    long ldv, ldo;
    double inv1, inv2;
    double sc;                // o0 = sc * (K0 V) + sh * add   (add may be NULL; the solver's Sigma p = s K0 p + v p in one launch)
    const double* add;        // [Nr][ldo]
    double sh;
};

template <int K1, int K2, bool DER, int NT>
__global__ __launch_bounds__(256) void exi_kmv_kernel(const ExiKmv a) {
    __shared__ double sx1[EXI_JC], sx2[EXI_JC];
    __shared__ double sV[NT * EXI_JC * 16];                      // [t][j][16]: a k-step reads 64 consecutive doubles per t
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, fk = lane >> 4;
    const int row0 = blockIdx.x * EXI_ROWS + wave * 16;
    const int myrow = min(row0 + fi, a.Nr - 1);                  // rows past the end repeat the last one and are not stored
    const double x1 = a.xr1[myrow], x2 = a.xr2[myrow];
    exi_d4 acc0[NT], acc1[DER ? NT : 1], acc2[DER ? NT : 1];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc0[t] = (exi_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < (DER ? NT : 1); ++t) acc1[t] = acc2[t] = (exi_d4){0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < a.Nc; j0 += EXI_JC) {
        if (tid < EXI_JC) {                                      // columns past the end repeat the last one against zero rows of V
            const int j = min(j0 + tid, a.Nc - 1);
            sx1[tid] = a.xc1[j]; sx2[tid] = a.xc2[j];
        }
        for (int e = tid; e < EXI_JC * 16 * NT; e += 256) {
            const int j = e / (16 * NT), cc = e - j * (16 * NT);
            const int gj = j0 + j;
            sV[((cc >> 4) * EXI_JC + j) * 16 + (cc & 15)] = (gj < a.Nc && cc < a.nb) ? a.V[(long)gj * a.ldv + cc] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int s = 0; s < EXI_JC / 4; ++s) {
            const int j = 4 * s + fk;
            double p1, q1, g1, p2, q2, g2;
            exi_profile<K1, DER>(fabs(x1 - sx1[j]) * a.inv1, p1, q1, g1);
            exi_profile<K2, DER>(fabs(x2 - sx2[j]) * a.inv2, p2, q2, g2);
            const double E = exp(-(g1 + g2));
            const double k0 = (p1 * p2) * E;
            double kd1 = 0.0, kd2 = 0.0;
            if constexpr (DER) { kd1 = (q1 * a.inv1) * p2 * E; kd2 = p1 * (q2 * a.inv2) * E; }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double bv = sV[(t * EXI_JC + j) * 16 + fi];
                acc0[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(k0, bv, acc0[t], 0, 0, 0);
                if constexpr (DER) {
                    acc1[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(kd1, bv, acc1[t], 0, 0, 0);
                    acc2[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(kd2, bv, acc2[t], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // MFMA 16x16x4 f64 result layout: lane holds column (lane & 15), rows (lane >> 4) + 4 r
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + fk + 4 * r, col = t * 16 + fi;
            if (row < a.Nr && col < a.nb) {
                const long o = (long)row * a.ldo + col;
                a.o0[o] = a.add ? a.sc * acc0[t][r] + a.sh * a.add[o] : a.sc * acc0[t][r];
                if constexpr (DER) { a.o1[o] = acc1[t][r]; a.o2[o] = acc2[t][r]; }
            }
        }
}

template <int K1, int K2, bool DER>
static void exi_launch_nt(const ExiKmv& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.Nr + EXI_ROWS - 1) / EXI_ROWS)), block(256);
    switch ((a.nb + 15) / 16) {
        case 1: hipLaunchKernelGGL((exi_kmv_kernel<K1, K2, DER, 1>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((exi_kmv_kernel<K1, K2, DER, 2>), grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL((exi_kmv_kernel<K1, K2, DER, 3>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((exi_kmv_kernel<K1, K2, DER, 4>), grid, block, 0, st, a); break;
    }
}
template <int K1, int K2>
static void exi_launch_der(const ExiKmv& a, hipStream_t st) {
    if (a.o1) exi_launch_nt<K1, K2, true>(a, st); else exi_launch_nt<K1, K2, false>(a, st);
}
template <int K1>
static void exi_launch_k2(int kind2, const ExiKmv& a, hipStream_t st) {
    switch (kind2) {
        case VGGP_KIND_MATERN12: exi_launch_der<K1, VGGP_KIND_MATERN12>(a, st); break;
        case VGGP_KIND_MATERN32: exi_launch_der<K1, VGGP_KIND_MATERN32>(a, st); break;
        case VGGP_KIND_MATERN52: exi_launch_der<K1, VGGP_KIND_MATERN52>(a, st); break;
        default: exi_launch_der<K1, VGGP_KIND_RBF>(a, st); break;
    }
}
// one launch: the kinds, the mode and the accumulator count select the instantiation here, once
static hipError_t exi_kmv_launch(int kind1, int kind2, const ExiKmv& a, hipStream_t st) {
    switch (kind1) {
        case VGGP_KIND_MATERN12: exi_launch_k2<VGGP_KIND_MATERN12>(kind2, a, st); break;
        case VGGP_KIND_MATERN32: exi_launch_k2<VGGP_KIND_MATERN32>(kind2, a, st); break;
        case VGGP_KIND_MATERN52: exi_launch_k2<VGGP_KIND_MATERN52>(kind2, a, st); break;
        default: exi_launch_k2<VGGP_KIND_RBF>(kind2, a, st); break;
    }
    return hipGetLastError();
}

extern "C" int vggp_exact_kmv(vggp_ctx* c, int kind1, int kind2, double ell1, double ell2, const double* xr1, const double* xr2, int64_t Nr,
                              const double* xc1, const double* xc2, int64_t Nc, const double* V, int64_t nb, double* out0, double* out1,
                              double* out2, void* stream) {
    if (!c) { vg_set_error("vggp_exact_kmv: null context"); return VGGP_EINVAL; }
    VG_REQUIRE(c->n_ranks == 1 && !c->comm && !c->cb, "vggp_exact_kmv: the exact GP is single-rank only");
    VG_REQUIRE(kind1 >= 0 && kind1 <= 3 && kind2 >= 0 && kind2 <= 3, "vggp_exact_kmv: bad kind");
    VG_REQUIRE(ell1 > 0.0 && std::isfinite(ell1) && ell2 > 0.0 && std::isfinite(ell2), "vggp_exact_kmv: the lengthscales must be positive and finite");
    VG_REQUIRE(Nr >= 1 && Nc >= 1 && Nr * 64 < (1LL << 31) && Nc * 64 < (1LL << 31), "vggp_exact_kmv: Nr = %lld, Nc = %lld outside [1, 2^25)",
               (long long)Nr, (long long)Nc);
    VG_REQUIRE(nb >= 1 && nb <= EXI_MAX_NB, "vggp_exact_kmv: nb = %lld outside [1, %d]", (long long)nb, EXI_MAX_NB);
    VG_REQUIRE(xr1 && xr2 && xc1 && xc2 && V && out0, "vggp_exact_kmv: null argument");
    VG_REQUIRE((out1 == nullptr) == (out2 == nullptr), "vggp_exact_kmv: out1 and out2 are given together (both derivatives) or both NULL");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const ExiKmv a{xr1, xr2, xc1, xc2, V, out0, out1, out2, (int)Nr, (int)Nc, (int)nb, (long)nb, (long)nb, 1.0 / ell1, 1.0 / ell2, 1.0, nullptr, 0.0};
    VG_HIP(exi_kmv_launch(kind1, kind2, a, st));
    return VGGP_OK;
}

// ================================================================================================================================
// Iterative exact GP (vggp_exact_iter_plan / _step_iter / _posterior_iter / _readout_iter): N beyond the dense solver of exact.hip.
//     Sigma = s K0 + v I is applied through the product above (never stored; no jitter: positive definite for v > 0).
//     Preconditioner: Nystroem on r = min(rank, N) strided landmarks idx_j = ((2 j + 1) N) / (2 r) -- deterministic, no pivot search:
//         Lz Lz^T = s K0[idx, idx] (psd_safe jitter schedule, info.jitter1),  L = s K0[:, idx] Lz^-T,  P = v I + L L^T,
//         L^T L = V diag(lam) V^T (vggp_eigh; lam_i <= 1e-14 lam_max dropped),  Q = L V lam^-1/2,
//         P^w = v^w (I + Q diag((1 + lam / v)^w - 1) Q^T) for w = -1, 1/2,  log|P| = N log v + sum log1p(lam / v).
//     Block PCG on [y, z_1 .. z_p], z_c = P^1/2 z0_c (z0: vg_pcg_probe_kernel's counter hash keyed on (c, i)); the loop, the per-column
//     scalars and the stopping rule are vg_block_pcg's (block_pcg.h); log|Sigma| = log|P| + mean_c N e1^T log(T_c) e1 from the PCG coefficients (the small
//     tridiagonal eigenproblems run on the host: k <= max_iter unknowns per probe); traces mean_c u_c^T D w_c with ONE derivative-mode
//     product on [alpha, w_1 .. w_p].  Block vectors are [N][nbp], nbp = 16 ceil(nb / 16), zero-padded.  Every sum over the points is
//     taken per 512-row chunk and the chunk partials are added in ascending order: bitwise repeatable.
// Specification: tests/exact_iter_spec.py.
// ================================================================================================================================
#include <algorithm>
#include <vector>

#define EXI_CHUNK 512         // rows per partial of the column dots
#define EXI_MAX_RANK 256
#define EXI_MAX_PROBES 63
#define EXI_EIG_CUT 1e-14

struct ExiHost { int nact; int pad; };                     // pinned: the count of active columns, read once per iteration
struct VgExactIter {
    long N = 0;
    int kind1 = 0, kind2 = 0, nchunk = 0;
    std::vector<double> hx1, hx2;                            // host copy of the coordinates (landmarks are gathered on the host)
    double *x1 = nullptr, *x2 = nullptr, *alpha = nullptr;   // [N]
    double *X = nullptr, *R = nullptr, *Pd = nullptr, *AP = nullptr, *Zp = nullptr, *Wz = nullptr, *Bk = nullptr;   // [N][64]
    double *part = nullptr;                                  // [nchunk][2][64]
    double *col = nullptr;                                   // [8][64] PCG scalars (rows as vg_pcg_scalars_kernel) + [4][64] sums
    double *T = nullptr;                                     // [256][64]
    double *zx1 = nullptr, *zx2 = nullptr, *lam = nullptr, *cf = nullptr;   // [256] landmarks, eigenvalues; [3][256] coefficients
    double *Kzz = nullptr, *Lz = nullptr, *Lzi = nullptr, *G = nullptr, *Vt = nullptr;   // [256][256]
    long long* cells = nullptr;                              // [64]
    int* nact = nullptr;
    void* mem = nullptr;
    double *L = nullptr, *Q = nullptr; void* lq = nullptr; size_t lq_rank = 0;          // [N][r], grown with the rank
    double *alh = nullptr, *beh = nullptr; void* hist = nullptr; size_t hist_it = 0;    // [max_iter][64]
    double* scr = nullptr; size_t scr_n = 0;                                            // split-K partials
    ExiHost* host = nullptr;
    // state of the last successful step
    bool have_step = false;
    double theta[5] = {0, 0, 0, 0, 0};
    int rq = 0;                                              // columns of Q (0: P = v I)
};

static void exi_layout(VgExactIter& w, VgArena& a) {
    const size_t N = w.N, R2 = (size_t)EXI_MAX_RANK * EXI_MAX_RANK;
    w.x1 = a.take(N); w.x2 = a.take(N); w.alpha = a.take(N);
    w.X = a.take(N * 64); w.R = a.take(N * 64); w.Pd = a.take(N * 64); w.AP = a.take(N * 64); w.Zp = a.take(N * 64); w.Wz = a.take(N * 64);
    w.Bk = a.take(N * 64);
    w.part = a.take((size_t)w.nchunk * 128); w.col = a.take(12 * 64); w.T = a.take((size_t)EXI_MAX_RANK * 64);
    w.zx1 = a.take(EXI_MAX_RANK); w.zx2 = a.take(EXI_MAX_RANK); w.lam = a.take(EXI_MAX_RANK); w.cf = a.take(3 * EXI_MAX_RANK);
    w.Kzz = a.take(R2); w.Lz = a.take(R2); w.Lzi = a.take(R2); w.G = a.take(R2); w.Vt = a.take(R2);
    w.cells = reinterpret_cast<long long*>(a.take(64));
    w.nact = reinterpret_cast<int*>(a.take(8));
}

static VgExactIter* exi_ws(vggp_ctx* c) { return reinterpret_cast<VgExactIter*>(c->exact_iter); }

void vg_exact_iter_free(vggp_ctx* c) {
    VgExactIter* w = exi_ws(c);
    if (!w) return;
    if (w->mem) (void)hipFree(w->mem);
    if (w->lq) (void)hipFree(w->lq);
    if (w->hist) (void)hipFree(w->hist);
    if (w->scr) (void)hipFree(w->scr);
    if (w->host) (void)hipHostFree(w->host);
    delete w;
    c->exact_iter = nullptr;
}

// grow-only side buffers (the device is idle when one is replaced)
static int exi_grow(void** buf, size_t bytes) {
    if (*buf) { VG_HIP(hipDeviceSynchronize()); VG_HIP(hipFree(*buf)); *buf = nullptr; }
    hipError_t e = hipMalloc(buf, bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); *buf = nullptr; vg_set_error("exact GP (iterative): out of device memory (%.1f MiB)", bytes / 1048576.0); return VGGP_ENOMEM; }
    return VGGP_OK;
}
static int exi_need_scr(VgExactIter& w, size_t n) {
    if (w.scr_n >= n) return VGGP_OK;
    w.scr_n = 0;
    int rc = exi_grow(reinterpret_cast<void**>(&w.scr), n * sizeof(double));
    if (!rc) w.scr_n = n;
    return rc;
}

// ---- small kernels -------------------------------------------------------------------------------------------------------------
// one kernel element with the kinds as run-time arguments (landmark block, explicit right-hand sides: O(N r) elements, not N^2)
__device__ __forceinline__ double exi_k0(int kind1, int kind2, double d1, double d2, double inv1, double inv2) {
    double p1, q1, g1, p2, q2, g2;
    const double r1 = fabs(d1) * inv1, r2 = fabs(d2) * inv2;
    switch (kind1) {
        case VGGP_KIND_MATERN12: exi_profile<VGGP_KIND_MATERN12, false>(r1, p1, q1, g1); break;
        case VGGP_KIND_MATERN32: exi_profile<VGGP_KIND_MATERN32, false>(r1, p1, q1, g1); break;
        case VGGP_KIND_MATERN52: exi_profile<VGGP_KIND_MATERN52, false>(r1, p1, q1, g1); break;
        default: exi_profile<VGGP_KIND_RBF, false>(r1, p1, q1, g1); break;
    }
    switch (kind2) {
        case VGGP_KIND_MATERN12: exi_profile<VGGP_KIND_MATERN12, false>(r2, p2, q2, g2); break;
        case VGGP_KIND_MATERN32: exi_profile<VGGP_KIND_MATERN32, false>(r2, p2, q2, g2); break;
        case VGGP_KIND_MATERN52: exi_profile<VGGP_KIND_MATERN52, false>(r2, p2, q2, g2); break;
        default: exi_profile<VGGP_KIND_RBF, false>(r2, p2, q2, g2); break;
    }
    return (p1 * p2) * exp(-(g1 + g2));
}
#define EXI_LAUNCH1D(kern, n, st, ...) \
    hipLaunchKernelGGL(kern, dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, st, __VA_ARGS__)

// dst[i * ldd] = src[i * lds]
__global__ void exi_copycol_kernel(const double* src, long lds, double* dst, long ldd, long N) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) dst[i * ldd] = src[i * lds];
}
// out[r][c] = sc K0(a_r, b_c) (ld = ldo) for r < na, c < nbcols; columns nbcols <= c < ldo are zeroed when pad
__global__ void exi_kblock_kernel(const double* a1, const double* a2, long na, const double* b1, const double* b2, int nbcols, int kind1,
                                  int kind2, double inv1, double inv2, double sc, double* out, int ldo) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= na * ldo) return;
    const long r = idx / ldo;
    const int cc = (int)(idx - r * ldo);
    out[idx] = cc < nbcols ? sc * exi_k0(kind1, kind2, a1[r] - b1[cc], a2[r] - b2[cc], inv1, inv2) : 0.0;
}
// Vt[j][c] = sc Lzi[c][j]   (r x r; Lzi lower-triangular, its upper part is not read)
__global__ void exi_tscale_kernel(const double* Lzi, int r, double sc, double* Vt) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= r * r) return;
    const int j = idx / r, cc = idx - j * r;
    Vt[idx] = cc >= j ? sc * Lzi[(long)cc * r + j] : 0.0;
}
// M[i][j] *= f[j]
__global__ void exi_colscale_kernel(double* M, long n, int r, const double* f) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n * r) M[idx] *= f[idx % r];
}
// T[j][c] *= f[j]
__global__ void exi_rowscale_kernel(double* T, int r, int nbp, const double* f) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < r * nbp) T[idx] *= f[idx / nbp];
}
// out = vw (in + add)   (add may be NULL)
__global__ void exi_pfin_kernel(const double* in, const double* add, double vw, long n, double* out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) out[idx] = add ? vw * (in[idx] + add[idx]) : vw * in[idx];
}
// per-column dots of [N][ld] blocks over one chunk of rows: part[chunk][0][c] = <A, B>_c, part[chunk][1][c] = <C, D>_c (C optional)
__global__ __launch_bounds__(256) void exi_coldots_kernel(const double* A, long lda, const double* B, long ldb, const double* Cc, long ldc,
                                                          const double* D, long ldd, long N, int ncols, double* part) {
    __shared__ double sh[2][4][64];
    const int cidx = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const long r0 = (long)blockIdx.x * EXI_CHUNK, r1 = min(N, r0 + EXI_CHUNK);
    double s0 = 0.0, s1 = 0.0;
    if (cidx < ncols)
        for (long i = r0 + rl; i < r1; i += 4) {
            s0 += A[i * lda + cidx] * B[i * ldb + cidx];
            if (Cc) s1 += Cc[i * ldc + cidx] * D[i * ldd + cidx];
        }
    sh[0][rl][cidx] = s0; sh[1][rl][cidx] = s1;
    __syncthreads();
    if (threadIdx.x < 128) {
        const int q = threadIdx.x >> 6;
        part[((long)blockIdx.x * 2 + q) * 64 + cidx] = (sh[q][0][cidx] + sh[q][1][cidx]) + (sh[q][2][cidx] + sh[q][3][cidx]);
    }
}
// R[i][c] = s C1[a_c][i] C2[b_c][i] for the listed cells (c < cn), 0 in the unused columns
__global__ void exi_cellrhs_kernel(const double* C1, const double* C2, const long long* cells, int cn, long mv2, long N, double s, double* R) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * 64) return;
    const long i = idx >> 6;
    const int c = (int)(idx & 63);
    if (c >= cn) { R[idx] = 0.0; return; }
    const long a = cells[c] / mv2, b = cells[c] - a * mv2;
    R[idx] = s * C1[a * N + i] * C2[b * N + i];
}
// T[b][i] = s alpha_i C2[b][i]
__global__ void exi_alphascale_kernel(const double* C2, const double* alpha, long mv2, long N, double s, double* T) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < mv2 * N) T[idx] = s * alpha[idx % N] * C2[idx];
}
// var[p] = s kd1[a] kd2[b] + wt vsum[p]   (p = a mv2 + b)
__global__ void exi_litvar_kernel(const double* vsum, const double* kd1, const double* kd2, long mv2, long n, double s, double wt, double* var) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) var[p] = s * kd1[p / mv2] * kd2[p % mv2] + wt * vsum[p];
}
// var[c] = prior_c - wt dots[c]: prior s (points) or s kd1[a] kd2[b] (cells)
__global__ void exi_varfin_kernel(const double* dots, const long long* cells, const double* kd1, const double* kd2, long mv2, int cn, double s,
                                  double wt, double* var) {
    const int c = threadIdx.x;
    if (c >= cn) return;
    double prior = s;
    if (cells) { const long a = cells[c] / mv2, b = cells[c] - a * mv2; prior = s * kd1[a] * kd2[b]; }
    var[c] = prior - wt * dots[c];
}

// ---- host helpers --------------------------------------------------------------------------------------------------------------
// C[M][Nn] = op(A) op(B) with the K range split into slabs that are added in ascending order (deterministic, many workgroups)
static int exi_gemm_splitk(VgExactIter& w, const double* A, long sa_m, long sa_k, const double* B, long sb_k, long sb_n, double* Cm, int M,
                           int Nn, long K, hipStream_t st) {
    int ks = (int)std::min<long>(64, std::max<long>(1, K / 1024));
    int rc;
    if (ks > 1 && (rc = exi_need_scr(w, (size_t)ks * M * Nn))) return rc;
    VgGemmBatch g;
    vg_gemm_init(&g);
    if (ks == 1) {
        vg_gemm_add(&g, A, sa_m, sa_k, B, sb_k, sb_n, Cm, Nn, M, Nn, (int)K);
        VG_HIP(vg_gemm_launch(&g, st));
        return VGGP_OK;
    }
    const int idx = vg_gemm_add(&g, A, sa_m, sa_k, B, sb_k, sb_n, w.scr, Nn, M, Nn, (int)K, ks, (long)M * Nn);
    ks = g.p[idx].ksplit;
    VG_HIP(vg_gemm_launch(&g, st));
    VgRedBatch r;
    vg_red_init(&r);
    vg_red_add(&r, w.scr, Cm, (long)M * Nn, (long)M * Nn, ks);
    VG_HIP(vg_red_launch(&r, st));
    return VGGP_OK;
}
static hipError_t exi_kmv_self(const VgExactIter& w, const double* V, int nb, int ld, double* o0, double* o1, double* o2, double sc,
                               const double* add, double sh, hipStream_t st) {
    const ExiKmv a{w.x1, w.x2, w.x1, w.x2, V, o0, o1, o2, (int)w.N, (int)w.N, nb, (long)ld, (long)ld, 1.0 / w.theta[0], 1.0 / w.theta[1],
                   sc, add, sh};
    return exi_kmv_launch(w.kind1, w.kind2, a, st);
}
// out = P^w in for a block [N][nbp]; wi: 0 -> w = -1, 1 -> w = 1/2 (coefficient rows of w.cf).  out must not alias in.
static int exi_apply_p(VgExactIter& w, const double* in, double* out, int nbp, int wi, hipStream_t st) {
    const double v = w.theta[4], vw = wi == 0 ? 1.0 / v : sqrt(v);
    const long n = w.N * nbp;
    int rc;
    if (w.rq == 0) {
        EXI_LAUNCH1D(exi_pfin_kernel, n, st, in, (const double*)nullptr, vw, n, out);
        VG_HIP(hipGetLastError());
        return VGGP_OK;
    }
    const int r = w.rq;
    if ((rc = exi_gemm_splitk(w, w.Q, 1, r, in, nbp, 1, w.T, r, nbp, w.N, st))) return rc;              // T = Q^T in
    EXI_LAUNCH1D(exi_rowscale_kernel, (long)r * nbp, st, w.T, r, nbp, w.cf + (size_t)(1 + wi) * EXI_MAX_RANK);
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, w.Q, r, 1, w.T, nbp, 1, out, nbp, (int)w.N, nbp, r);                                 // out = Q T
    VG_HIP(vg_gemm_launch(&g, st));
    EXI_LAUNCH1D(exi_pfin_kernel, n, st, out, in, vw, n, out);
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}
static void exi_coldots(VgExactIter& w, const double* A, long lda, const double* B, long ldb, const double* Cc, long ldc, const double* D, long ldd,
                        int ncols, hipStream_t st) {
    hipLaunchKernelGGL(exi_coldots_kernel, dim3((unsigned)w.nchunk), dim3(256), 0, st, A, lda, B, ldb, Cc, ldc, D, ldd, w.N, ncols, w.part);
}
// plain column sums <A, B>_c, <C, D>_c (C optional) into rows [8], [9] of w.col
static int exi_sums(VgExactIter& w, const double* A, long lda, const double* B, long ldb, const double* Cc, long ldc, const double* D, long ldd,
                    int ncols, hipStream_t st) {
    exi_coldots(w, A, lda, B, ldb, Cc, ldc, D, ldd, ncols, st);
    hipLaunchKernelGGL(vg_pcg_scalars_kernel, dim3(1), dim3(64), 0, st, w.part, w.nchunk, w.col, 64, ncols, 3, 0, 0.0, (double*)nullptr,
                       (double*)nullptr, w.nact);
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}
// Block PCG on Sigma X = R (vg_block_pcg, block_pcg.h; R holds the right-hand sides on entry, [N][nbp], ncols of them).  The caller
// object: the operator is ONE matrix-free product Sigma p = s K0 p + v p, the preconditioner P^-1 of exi_apply_p, a column dot is the
// sum of 512-row chunk partials in ascending order, and the host waits with a stream sync on the workspace's own pinned word
// (single-rank only).  The active count is read after the start too: an all-zero block reports zero iterations.
static int exi_pcg(VgExactIter& w, int nbp, int ncols, double tol, int max_iter, bool hist, int* iters, int* nact_out, hipStream_t st) {
    struct Ops {
        VgExactIter& w; int nbp, ncols; hipStream_t st;
        int apply() {                                                   // AP = s K0 p + v p
            VG_HIP(exi_kmv_self(w, w.Pd, nbp, nbp, w.AP, nullptr, nullptr, w.theta[2] * w.theta[3], w.Pd, w.theta[4], st));
            return VGGP_OK;
        }
        int precond() { return exi_apply_p(w, w.R, w.Zp, nbp, 0, st); }
        int dots(int phase) {
            if (phase == 1) exi_coldots(w, w.Pd, nbp, w.AP, nbp, nullptr, 0, nullptr, 0, ncols, st);
            else exi_coldots(w, w.R, nbp, w.Zp, nbp, w.R, nbp, w.R, nbp, ncols, st);
            return VGGP_OK;
        }
        int active(int* nact) {
            VG_HIP(hipMemcpyAsync(&w.host->nact, w.nact, sizeof(int), hipMemcpyDeviceToHost, st));
            VG_HIP(hipStreamSynchronize(st));
            *nact = w.host->nact;
            return VGGP_OK;
        }
    };
    const VgBlockPcg b{w.X, w.R, w.Pd, w.AP, w.Zp, w.part, w.nchunk, w.col, 64, hist ? w.alh : nullptr, hist ? w.beh : nullptr, w.nact,
                       w.N, nbp, 1, ncols, /*count_at_start=*/true};
    return vg_block_pcg(b, Ops{w, nbp, ncols, st}, tol, max_iter, hist, /*stale_limit=*/0, iters, nact_out, st);
}

static void exi_fill_info(vggp_info* info, double jit, int sweeps, int rounds, int status) {
    if (!info) return;
    info->jitter1 = jit; info->jitter2 = 0.0;
    info->sweeps1 = sweeps; info->sweeps2 = 0; info->rounds1 = rounds; info->rounds2 = 0;
    info->status = status; info->polished = 0;
}

extern "C" int vggp_exact_iter_plan(vggp_ctx* c, int kind1, int kind2, const double* x1, const double* x2, int64_t N) {
    if (!c) { vg_set_error("vggp_exact_iter_plan: null context"); return VGGP_EINVAL; }
    VG_REQUIRE(c->n_ranks == 1 && !c->comm && !c->cb, "vggp_exact_iter_plan: the exact GP is single-rank only");
    VG_REQUIRE(N >= 1 && N * 64 < (1LL << 31), "vggp_exact_iter_plan: N = %lld outside [1, 2^25)", (long long)N);
    VG_REQUIRE(kind1 >= 0 && kind1 <= 3 && kind2 >= 0 && kind2 <= 3, "vggp_exact_iter_plan: bad kind");
    VG_REQUIRE(x1 && x2, "vggp_exact_iter_plan: null coordinate arrays");
    for (int64_t i = 0; i < N; ++i)
        VG_REQUIRE(std::isfinite(x1[i]) && std::isfinite(x2[i]), "vggp_exact_iter_plan: point %lld is not finite", (long long)i);
    VG_ENTER_DEVICE(c->device);
    VgExactIter tmp;
    tmp.N = N; tmp.kind1 = kind1; tmp.kind2 = kind2;
    tmp.nchunk = (int)((N + EXI_CHUNK - 1) / EXI_CHUNK);
    const size_t bytes = vg_arena_measure([&](VgArena& a) { exi_layout(tmp, a); });
    int rc;
    if ((rc = vg_quiesce(c))) return rc;
    if (c->exact_iter) { VG_HIP(hipDeviceSynchronize()); vg_exact_iter_free(c); }
    size_t free_b = 0;
    if (!vg_arena_fits(bytes, &free_b)) {
        vg_set_error("vggp_exact_iter_plan: the iterative exact GP (N = %lld) needs %.1f GiB of workspace, %.1f GiB are free", (long long)N,
                     (double)bytes / 1073741824.0, (double)free_b / 1073741824.0);
        return VGGP_ENOMEM;
    }
    VgExactIter* w = new VgExactIter(tmp);
    c->exact_iter = w;                   // owned by the context from here on
    w->hx1.assign(x1, x1 + N); w->hx2.assign(x2, x2 + N);
    if (hipHostMalloc((void**)&w->host, sizeof(ExiHost), hipHostMallocDefault) != hipSuccess || hipMalloc(&w->mem, bytes) != hipSuccess) {
        (void)hipGetLastError();
        vg_exact_iter_free(c);           // (a half-built workspace must not be left for a later step to find)
        vg_set_error("vggp_exact_iter_plan: out of memory (%.1f GiB of workspace for N = %lld)", (double)bytes / 1073741824.0, (long long)N);
        return VGGP_ENOMEM;
    }
    if ((rc = vg_arena_place(w->mem, bytes, [&](VgArena& a) { exi_layout(*w, a); }))) return rc;
    VG_HIP(hipMemcpy(w->x1, x1, sizeof(double) * N, hipMemcpyHostToDevice));
    VG_HIP(hipMemcpy(w->x2, x2, sizeof(double) * N, hipMemcpyHostToDevice));
    return VGGP_OK;
}

// the Nystroem factors of the step's theta: Q, the coefficient rows of P^-1 and P^1/2, log|P|; *jit: the landmark factor's jitter
static int exi_precond(vggp_ctx* c, VgExactIter& w, int rank, double* jit, double* logdetP, hipStream_t st) {
    const long N = w.N;
    const double s = w.theta[2] * w.theta[3], v = w.theta[4], inv1 = 1.0 / w.theta[0], inv2 = 1.0 / w.theta[1];
    const int r = (int)std::min<long>(rank, N);
    *jit = 0.0;
    *logdetP = (double)N * log(v);
    w.rq = 0;
    if (r == 0) return VGGP_OK;
    int rc;
    if (w.lq_rank < (size_t)r) {
        w.lq_rank = 0;
        if ((rc = exi_grow(&w.lq, sizeof(double) * 2 * (size_t)N * r + 512))) return rc;
        w.lq_rank = r;
    }
    w.L = reinterpret_cast<double*>(w.lq);
    w.Q = w.L + (((size_t)N * r + 31) & ~size_t(31));
    std::vector<double> z1(r), z2(r);
    for (int j = 0; j < r; ++j) {
        const long idx = ((2L * j + 1) * N) / (2L * r);
        z1[j] = w.hx1[idx]; z2[j] = w.hx2[idx];
    }
    VG_HIP(hipMemcpyAsync(w.zx1, z1.data(), sizeof(double) * r, hipMemcpyHostToDevice, st));
    VG_HIP(hipMemcpyAsync(w.zx2, z2.data(), sizeof(double) * r, hipMemcpyHostToDevice, st));
    VG_HIP(hipStreamSynchronize(st));                                   // (z1, z2 leave scope)
    EXI_LAUNCH1D(exi_kblock_kernel, (long)r * r, st, w.zx1, w.zx2, (long)r, w.zx1, w.zx2, r, w.kind1, w.kind2, inv1, inv2, s, w.Kzz, r);
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemsetAsync(w.Lzi, 0, sizeof(double) * r * r, st));
    if ((rc = vggp_cholesky_inverse(c, w.Kzz, r, w.Lz, w.Lzi, jit, st))) return rc;
    EXI_LAUNCH1D(exi_tscale_kernel, r * r, st, w.Lzi, r, s, w.Vt);      // Vt = s Lz^-T
    VG_HIP(hipGetLastError());
    for (int c0 = 0; c0 < r; c0 += 64) {                                // L = K0[:, idx] (s Lz^-T), 64 columns a launch
        const ExiKmv a{w.x1, w.x2, w.zx1, w.zx2, w.Vt + c0, w.L + c0, nullptr, nullptr, (int)N, r, std::min(64, r - c0), (long)r, (long)r,
                       inv1, inv2, 1.0, nullptr, 0.0};
        VG_HIP(exi_kmv_launch(w.kind1, w.kind2, a, st));
    }
    if ((rc = exi_gemm_splitk(w, w.L, 1, r, w.L, r, 1, w.G, r, r, N, st))) return rc;                     // G = L^T L
    int32_t sweeps = 0;
    if ((rc = vggp_eigh(c, w.G, r, w.lam, w.Vt, &sweeps, 0, st))) return rc;                              // rows of Vt = eigenvectors
    std::vector<double> lam(r), cf(3 * (size_t)EXI_MAX_RANK, 0.0);
    VG_HIP(hipMemcpy(lam.data(), w.lam, sizeof(double) * r, hipMemcpyDeviceToHost));
    double lmax = 0.0, ld = 0.0;
    for (int j = 0; j < r; ++j) lmax = std::max(lmax, lam[j]);
    for (int j = 0; j < r; ++j) {
        if (!(lam[j] > EXI_EIG_CUT * lmax)) continue;                   // dropped: a zero column of Q, zero coefficients
        const double x = lam[j] / v;
        cf[j] = 1.0 / sqrt(lam[j]);
        cf[EXI_MAX_RANK + j] = 1.0 / (1.0 + x) - 1.0;
        cf[2 * EXI_MAX_RANK + j] = sqrt(1.0 + x) - 1.0;
        ld += log1p(x);
    }
    *logdetP += ld;
    VG_HIP(hipMemcpy(w.cf, cf.data(), sizeof(double) * cf.size(), hipMemcpyHostToDevice));
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, w.L, r, 1, w.Vt, 1, r, w.Q, r, (int)N, r, r);                                         // Q = L V
    VG_HIP(vg_gemm_launch(&g, st));
    EXI_LAUNCH1D(exi_colscale_kernel, N * r, st, w.Q, N, r, w.cf);
    VG_HIP(hipGetLastError());
    w.rq = r;
    return VGGP_OK;
}

extern "C" int vggp_exact_step_iter(vggp_ctx* c, const double* y, const double theta[5], int n_probes, int rank, double tol, int max_iter,
                                    double* mll_out, double grad_out[5], vggp_info* info, void* stream) {
    if (!c) { vg_set_error("vggp_exact_step_iter: null context"); return VGGP_EINVAL; }
    if (!c->exact_iter) { vg_set_error("vggp_exact_step_iter: no iterative exact plan (vggp_exact_iter_plan)"); return VGGP_ESTATE; }
    VG_REQUIRE(y && theta && mll_out && grad_out, "vggp_exact_step_iter: null argument");
    VG_REQUIRE(c->n_ranks == 1 && !c->comm && !c->cb, "vggp_exact_step_iter: the exact GP is single-rank only");
    VgExactIter& w = *exi_ws(c);
    w.have_step = false;
    if (n_probes <= 0) n_probes = 16;
    if (rank < 0) rank = 64;
    if (!(tol > 0.0)) tol = 1e-10;
    if (max_iter <= 0) max_iter = 1000;
    VG_REQUIRE(n_probes <= EXI_MAX_PROBES, "vggp_exact_step_iter: n_probes = %d above %d", n_probes, EXI_MAX_PROBES);
    VG_REQUIRE(rank <= EXI_MAX_RANK, "vggp_exact_step_iter: rank = %d above %d", rank, EXI_MAX_RANK);
    VG_REQUIRE(max_iter <= (1 << 20), "vggp_exact_step_iter: max_iter = %d above 2^20", max_iter);
    for (int i = 0; i < 5; ++i) {
        VG_REQUIRE(theta[i] > 0.0 && std::isfinite(theta[i]), "theta[%d]=%g must be positive and finite", i, theta[i]);
        w.theta[i] = theta[i];
    }
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    int rc;
    if ((rc = vg_quiesce(c))) return rc;
    const long N = w.N;
    const int nbc = 1 + n_probes, nbp = 16 * ((nbc + 15) / 16);
    const long n = N * nbp;
    const double s1 = w.theta[2], s2 = w.theta[3], s = s1 * s2;
    if (w.hist_it < (size_t)max_iter) {
        w.hist_it = 0;
        if ((rc = exi_grow(&w.hist, sizeof(double) * 2 * (size_t)max_iter * 64))) return rc;
        w.hist_it = max_iter;
    }
    w.alh = reinterpret_cast<double*>(w.hist);
    w.beh = w.alh + (size_t)w.hist_it * 64;
    double jit = 0.0, logdetP = 0.0;
    rc = exi_precond(c, w, rank, &jit, &logdetP, st);
    if (rc) { exi_fill_info(info, rc == VGGP_ENOTPD ? -1.0 : jit, n_probes, 0, rc); return rc; }
    // right-hand sides: column 0 = y, columns c >= 1 = P^1/2 z0_c;  Wz = P^-1 of them
    EXI_LAUNCH1D(vg_pcg_probe_kernel, n, st, w.Bk, N, nbp, 1, nbc, 0x5647475000000001ULL);
    VG_HIP(hipGetLastError());
    if ((rc = exi_apply_p(w, w.Bk, w.R, nbp, 1, st))) return rc;
    if ((rc = exi_apply_p(w, w.R, w.Wz, nbp, 0, st))) return rc;
    EXI_LAUNCH1D(exi_copycol_kernel, N, st, y, 1L, w.R, (long)nbp, N);
    VG_HIP(hipGetLastError());
    int iters = 0, nact = 0;
    if ((rc = exi_pcg(w, nbp, nbc, tol, max_iter, true, &iters, &nact, st))) return rc;
    if (nact > 0) {
        exi_fill_info(info, jit, n_probes, iters, nact);
        vg_set_error("vggp_exact_step_iter: %d of %d columns not converged after %d iterations (tol %g)", nact, nbc, iters, tol);
        return VGGP_ENOCONV;
    }
    // alpha = x_0; ONE derivative-mode product on [alpha, w_1 .. w_p]
    EXI_LAUNCH1D(exi_copycol_kernel, N, st, w.X, (long)nbp, w.alpha, 1L, N);
    EXI_LAUNCH1D(exi_copycol_kernel, N, st, w.X, (long)nbp, w.Wz, (long)nbp, N);
    VG_HIP(hipGetLastError());
    VG_HIP(exi_kmv_self(w, w.Wz, nbc, nbp, w.AP, w.Zp, w.Pd, 1.0, nullptr, 0.0, st));
    std::vector<double> hcol(12 * 64), dK(64), d1(64), d2(64), dI(64);
    if ((rc = exi_sums(w, w.X, nbp, w.AP, nbp, w.X, nbp, w.Zp, nbp, nbc, st))) return rc;
    VG_HIP(hipMemcpyAsync(hcol.data(), w.col, sizeof(double) * 12 * 64, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < 64; ++k) { dK[k] = hcol[512 + k]; d1[k] = hcol[576 + k]; }
    const std::vector<double> kc(hcol.begin() + 448, hcol.begin() + 512);
    if ((rc = exi_sums(w, w.X, nbp, w.Pd, nbp, w.X, nbp, w.Wz, nbp, nbc, st))) return rc;
    VG_HIP(hipMemcpyAsync(hcol.data(), w.col, sizeof(double) * 12 * 64, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < 64; ++k) { d2[k] = hcol[512 + k]; dI[k] = hcol[576 + k]; }
    if ((rc = exi_sums(w, y, 1, w.alpha, 1, nullptr, 0, nullptr, 0, 1, st))) return rc;
    VG_HIP(hipMemcpyAsync(hcol.data(), w.col, sizeof(double) * 12 * 64, hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    const double yalpha = hcol[512];
    // Lanczos quadrature of the probe columns
    std::vector<double> alh((size_t)iters * 64), beh((size_t)iters * 64);
    if (iters > 0) {
        VG_HIP(hipMemcpy(alh.data(), w.alh, sizeof(double) * alh.size(), hipMemcpyDeviceToHost));
        VG_HIP(hipMemcpy(beh.data(), w.beh, sizeof(double) * beh.size(), hipMemcpyDeviceToHost));
    }
    double ldsum = 0.0;
    std::vector<double> td(iters + 1), te(iters + 1), tz(iters + 1);
    for (int cidx = 1; cidx < nbc; ++cidx) {
        const int k = (int)kc[cidx];
        for (int j = 0; j < k; ++j) {
            const double a = alh[(size_t)j * 64 + cidx];
            td[j] = 1.0 / a + (j > 0 ? beh[(size_t)(j - 1) * 64 + cidx] / alh[(size_t)(j - 1) * 64 + cidx] : 0.0);
            te[j] = j + 1 < k ? sqrt(beh[(size_t)j * 64 + cidx]) / a : 0.0;
            tz[j] = j == 0 ? 1.0 : 0.0;
        }
        double q = 0.0;
        if (vg_lanczos_logquad(td.data(), te.data(), tz.data(), k, &q) != 0) {      // (lanczos_quad.h: the routine of vgi_slq_kernel)
            exi_fill_info(info, jit, n_probes, iters, -1);
            vg_set_error("vggp_exact_step_iter: the Lanczos quadrature of probe %d failed", cidx);
            return VGGP_ENOCONV;
        }
        ldsum += (double)N * q;
    }
    const double logdet = logdetP + ldsum / n_probes;
    auto tr = [&](const std::vector<double>& d) { double t = 0.0; for (int k = 1; k < nbc; ++k) t += d[k]; return t / n_probes; };
    const double gK = dK[0] - tr(dK);
    *mll_out = -0.5 * (yalpha + logdet + (double)N * log(2.0 * M_PI));
    grad_out[0] = 0.5 * s * (d1[0] - tr(d1));
    grad_out[1] = 0.5 * s * (d2[0] - tr(d2));
    grad_out[2] = 0.5 * s2 * gK;
    grad_out[3] = 0.5 * s1 * gK;
    grad_out[4] = 0.5 * (dI[0] - tr(dI));
    exi_fill_info(info, jit, n_probes, iters, 0);
    w.have_step = true;
    return VGGP_OK;
}

static int exi_readout_enter(vggp_ctx* c, const char* fn, VgExactIter** w) {
    if (!c) { vg_set_error("%s: null context", fn); return VGGP_EINVAL; }
    if (!c->exact_iter || !exi_ws(c)->have_step) {
        vg_set_error("%s: no finished vggp_exact_step_iter on the current iterative exact plan", fn);
        return VGGP_ESTATE;
    }
    *w = exi_ws(c);
    return VGGP_OK;
}
// one block of <= 64 explicit right-hand sides in w.R (kept in w.Bk): solve, dots[c] = rhs_c^T Sigma^-1 rhs_c into w.col row 8
static int exi_solve_block(VgExactIter& w, const char* fn, double tol, int max_iter, int cn, int* iters_max, hipStream_t st) {
    int rc, iters = 0, nact = 0;
    VG_HIP(hipMemcpyAsync(w.Bk, w.R, sizeof(double) * w.N * 64, hipMemcpyDeviceToDevice, st));
    if ((rc = exi_pcg(w, 64, cn, tol, max_iter, false, &iters, &nact, st))) return rc;
    *iters_max = std::max(*iters_max, iters);
    if (nact > 0) {
        w.have_step = false;
        vg_set_error("%s: %d columns not converged after %d iterations (tol %g)", fn, nact, iters, tol);
        return VGGP_ENOCONV;
    }
    return exi_sums(w, w.Bk, 64, w.X, 64, nullptr, 0, nullptr, 0, cn, st);
}

extern "C" int vggp_exact_posterior_iter(vggp_ctx* c, const double* xs1, const double* xs2, int64_t ns, double tol, int max_iter, double* mean,
                                         double* var, vggp_info* info, void* stream) {
    VgExactIter* wp;
    int rc;
    if ((rc = exi_readout_enter(c, "vggp_exact_posterior_iter", &wp))) return rc;
    VgExactIter& w = *wp;
    VG_REQUIRE(xs1 && xs2 && mean && ns >= 0 && ns * 64 < (1LL << 31), "vggp_exact_posterior_iter: bad argument");
    if (!(tol > 0.0)) tol = 1e-10;
    if (max_iter <= 0) max_iter = 1000;
    exi_fill_info(info, 0.0, 0, 0, 0);
    if (ns == 0) return VGGP_OK;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    if ((rc = vg_quiesce(c))) return rc;
    const double s = w.theta[2] * w.theta[3], inv1 = 1.0 / w.theta[0], inv2 = 1.0 / w.theta[1];
    const ExiKmv a{xs1, xs2, w.x1, w.x2, w.alpha, mean, nullptr, nullptr, (int)ns, (int)w.N, 1, 1L, 1L, inv1, inv2, s, nullptr, 0.0};
    VG_HIP(exi_kmv_launch(w.kind1, w.kind2, a, st));                   // mean = s K0(x*, X) alpha
    if (!var) return VGGP_OK;
    int iters = 0, nblk = 0;
    for (int64_t p0 = 0; p0 < ns; p0 += 64, ++nblk) {
        const int cn = (int)std::min<int64_t>(64, ns - p0);
        EXI_LAUNCH1D(exi_kblock_kernel, w.N * 64, st, w.x1, w.x2, w.N, xs1 + p0, xs2 + p0, cn, w.kind1, w.kind2, inv1, inv2, 1.0, w.R, 64);
        VG_HIP(hipGetLastError());
        if ((rc = exi_solve_block(w, "vggp_exact_posterior_iter", tol, max_iter, cn, &iters, st))) return rc;
        hipLaunchKernelGGL(exi_varfin_kernel, dim3(1), dim3(64), 0, st, w.col + 512, (const long long*)nullptr, (const double*)nullptr,
                           (const double*)nullptr, 1L, cn, s, s * s, var + p0);
        VG_HIP(hipGetLastError());
    }
    exi_fill_info(info, 0.0, nblk, iters, 0);
    return VGGP_OK;
}

extern "C" int vggp_exact_readout_iter(vggp_ctx* c, const double* C1, int64_t mv1, const double* C2, int64_t mv2, const double* kd1,
                                       const double* kd2, const int64_t* cells, int64_t n_cells, double tol, int max_iter, double* mean,
                                       double* var, int flags, vggp_info* info, void* stream) {
    VgExactIter* wp;
    int rc;
    if ((rc = exi_readout_enter(c, "vggp_exact_readout_iter", &wp))) return rc;
    VgExactIter& w = *wp;
    VG_REQUIRE(C1 && C2 && kd1 && kd2 && mean && mv1 >= 1 && mv2 >= 1, "vggp_exact_readout_iter: bad argument");
    VG_REQUIRE(w.kind1 == VGGP_KIND_MATERN12 && w.kind2 == VGGP_KIND_MATERN12,
               "vggp_exact_readout_iter: the B0 cell features are Matern-1/2 integrals; the plan uses another kernel");
    VG_REQUIRE(mv1 < (1L << 20) && mv2 < (1L << 20) && mv1 * mv2 < (1L << 28), "vggp_exact_readout_iter: too many cells");
    const bool literal = (flags & VGGP_READOUT_LITERAL) != 0;
    const long nv = mv1 * mv2;
    if (var && !literal) {
        VG_REQUIRE(cells && n_cells >= 1, "vggp_exact_readout_iter: the conditional variance needs a list of cells (no dense solve on this solver)");
        for (int64_t k = 0; k < n_cells; ++k)
            VG_REQUIRE(cells[k] >= 0 && cells[k] < nv, "vggp_exact_readout_iter: cell %lld outside [0, %ld)", (long long)cells[k], nv);
    }
    if (!(tol > 0.0)) tol = 1e-10;
    if (max_iter <= 0) max_iter = 1000;
    exi_fill_info(info, 0.0, 0, 0, 0);
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    if ((rc = vg_quiesce(c))) return rc;
    const long N = w.N;
    const double s = w.theta[2] * w.theta[3], v = w.theta[4];
    // mean = s C1 diag(alpha) C2^T: one GEMM over the points (split into slabs added in order)
    if ((rc = vg_ensure_misc(c, sizeof(double) * ((size_t)mv2 * N + 64)))) return rc;
    double* Tm = reinterpret_cast<double*>(c->misc);
    EXI_LAUNCH1D(exi_alphascale_kernel, mv2 * N, st, C2, w.alpha, (long)mv2, N, s, Tm);
    VG_HIP(hipGetLastError());
    if ((rc = exi_gemm_splitk(w, C1, N, 1, Tm, 1, N, mean, (int)mv1, (int)mv2, N, st))) return rc;
    if (!var) return VGGP_OK;
    if (literal) {                       // s kd1 kd2 + s^2 (C1 o C1)(C2 o C2)^T / v: a Gram product over the points, no solve
        const size_t sc = vg_kr_sqgram_scratch((int)mv1, (int)mv2, N);
        if ((rc = exi_need_scr(w, sc + (size_t)nv + 64))) return rc;
        double* vsum = w.scr + sc;
        VG_HIP(vg_kr_sqgram_launch(C1, C2, (int)mv1, (int)mv2, N, vsum, w.scr, 0, st));
        EXI_LAUNCH1D(exi_litvar_kernel, nv, st, vsum, kd1, kd2, (long)mv2, nv, s, s * s / v, var);
        VG_HIP(hipGetLastError());
        return VGGP_OK;
    }
    int iters = 0, nblk = 0;
    for (int64_t p0 = 0; p0 < n_cells; p0 += 64, ++nblk) {
        const int cn = (int)std::min<int64_t>(64, n_cells - p0);
        VG_HIP(hipMemcpyAsync(w.cells, cells + p0, sizeof(long long) * cn, hipMemcpyHostToDevice, st));
        EXI_LAUNCH1D(exi_cellrhs_kernel, N * 64, st, C1, C2, w.cells, cn, (long)mv2, N, s, w.R);
        VG_HIP(hipGetLastError());
        if ((rc = exi_solve_block(w, "vggp_exact_readout_iter", tol, max_iter, cn, &iters, st))) return rc;
        hipLaunchKernelGGL(exi_varfin_kernel, dim3(1), dim3(64), 0, st, w.col + 512, w.cells, kd1, kd2, (long)mv2, cn, s, 1.0, var + p0);
        VG_HIP(hipGetLastError());
        VG_HIP(hipStreamSynchronize(st));                               // (w.cells is overwritten by the next block)
    }
    exi_fill_info(info, 0.0, nblk, iters, 0);
    return VGGP_OK;
}
