// What the M-space solvers share: the workspaces, the reduction table and the helpers that cross a file boundary.
//   masked.hip          small kernels, workspace, blocked Cholesky, the two dense steps, vggp_zgrad_scattered
//   masked_readout.hip  the dense read-outs
//   iter_step.hip       VgIter machinery (block PCG, basis policy, traces), the two iterative steps
//   iter_readout.hip    the iterative read-outs: point-wise, joint samples, gridded
//   dense_sample.hip    joint samples on the dense states: the triangular product X = Xg^T E, vggp_qv_sample_masked
// A kernel or helper named here is defined in the file its comment names; everything else is static to its file.
#pragma once
#include "arena.h"
#include "block_pcg.h"
#include "ctx.h"

#include <algorithm>

#define VG_MB 128                 // panel width of the blocked Cholesky
#define VG_MD_NPART 256           // partial sums per reduction job
#define VG_MD_MAXJOBS 24
#define VGM_MAX_M 16384      // dense M x M solver: ~10 M^2 doubles of workspace (21 GB at the limit), O(M^3) per step
#define VGM_LAUNCH1D(kern, n, st, ...) \
    hipLaunchKernelGGL(kern, dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, st, __VA_ARGS__)
#define VGI_MAXIT 128             // PCG iterations of an iterative step: the Lanczos tridiagonal of vgi_slq_kernel lives in registers
#define VGI_MAX_PROBES 63         // probes of an iterative step: one block solve carries the data column and the probes, 64 columns
#define VGI_NTS 16                                // the scalars vgi_combine_kernel reads (14 used)
#define VGI_WAIT(c, st) do { const int wrc_ = vg_comm_wait(c, st); if (wrc_) return wrc_; } while (0)

// generic reductions, VG_MD_NPART partial sums per job:
//   op 0: sum a[i*sa] * b[i*sb]     op 1: sum log(a[i*sa])     op 2: sum a[i*sa]     op 3: sum a[i] * b[i] * c[i]
struct VgmRedJob { const double* a; const double* b; const double* c; long n, sa, sb; int op; };
struct VgmRedArgs { VgmRedJob job[VG_MD_MAXJOBS]; int njobs; double* partial; };
// job indices of the masked step (order of the partial-sum buffer)
enum { RJ_LOGDET = 0, RJ_Q, RJ_AA, RJ_TRS, RJ_TRPHI, RJ_MK1PTS, RJ_TRMK1, RJ_SPHI1, RJ_AC1, RJ_MKA1, RJ_Z1, RJ_HV1, RJ_MK1PT,
       RJ_MK2PTS, RJ_TRMK2, RJ_SPHI2, RJ_AC2, RJ_MKA2, RJ_Z2, RJ_HV2, RJ_MK2PT, RJ_COUNT };
struct VgmFinalArgs { const double* theta; const double* scal; double* out; double N, yy; int m1, m2; };

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
    size_t Tcap = 0;               // doubles T holds (vgm_layout): what every gemm_longk on it is checked against
    void* mem = nullptr;
    size_t bytes = 0;
};

// ---- workspace of an iterative step (w.imem; the algebra: iter_step.hip) --------------------------------------------------
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

// ---- workspace of the iterative read-outs (w.rmem; iter_readout.hip) ---------------------------------------------------------
struct VgReadout {
    VgIter it;                  // the block vectors the step's helpers work on (alh, beh: one row each; no Wz; the rest of VgIter unused)
    double p;                   // the step's observed fraction (scattered: 1 / N)
    double *T;                  // the right-hand sides, kept for the reductions
    double *A1, *A2, *U1, *U2;  // posterior(x*): factor columns a_d(x*) and U_d = L0_d^-1 a_d  [m_d][cn]
    long long* cells;           // q(v): this block's flat cell indices
    double* mean;               // joint samples: the q(v) mean every sample starts from  [m1][m2]
};

static inline bool vgi_multi(const vggp_ctx* c) { return c->n_ranks > 1 || c->comm || c->cb; }

// ---- masked.hip ------------------------------------------------------------------------------------------------------
__global__ void vgm_pairprod_kernel(const double* Xa, const double* Xb, int ma, int mb, long n, double* out);
__global__ void vgm_coldot_kernel(const double* Xa, const double* Xb, int m, long n, double* out);
__global__ __launch_bounds__(256) void vgm_red_kernel(const VgmRedArgs A);
__global__ void vgm_sum_kernel(const double* partial, double* scal, unsigned local_mask, int keep_replicated);
__global__ void vgm_final_kernel(const VgmFinalArgs A);
int vgm_prepare(vggp_ctx* c, bool iter = false);
int gemm1(const double* A, long sa_m, long sa_k, const double* B, long sb_k, long sb_n, double* C, int ldc, int M, int N, int K,
          hipStream_t st, double alpha = 1.0, int accum = 0);
int gemm_longk(const double* A, long sa_m, long sa_k, const double* B, long sb_k, long sb_n, double* C, int M, int N, int K,
               double* scratch, size_t scratch_doubles, hipStream_t st);
int vg_longk_slabs(long K);       // slabs gemm_longk writes for a reduction of length K (1: no split, no scratch)
// what each of the four steps does once its arguments are non-null: no earlier step's state stays readable, theta is checked and kept
int vgm_step_enter(vggp_ctx* c, const double theta[5]);
int vgm_colstats(vggp_ctx* c, VgMasked& w, const double* W, hipStream_t st);
int vgm_a0_terms(vggp_ctx* c, VgMasked& w, hipStream_t st);
int vgs_projections(vggp_ctx* c, VgMasked& w, const double* y, hipStream_t st);
int vgs_a0_terms(vggp_ctx* c, VgMasked& w, hipStream_t st);
// ---- masked_readout.hip (vg_whitened_columns, vg_whitened_cross: ctx.h) ------------------------------------------------
int vgi_qv_mean(vggp_ctx* c, VgMasked& w, double* mean, hipStream_t st);
// ---- iter_readout.hip: the stages the samplers of an iterative state share (joint samples of q(v), raster samples) ----
int vgi_sample_enter(vggp_ctx* c, const char* fn, bool scattered, const double* W, double n_obs, int64_t n_samples, int64_t first, const void* out,
                     bool noise_ok, const char* noise_rule, double* tol, int* max_iter, int* block, vggp_info* info);
int vgi_sample_prepare(vggp_ctx* c, VgReadout& r, int nbc, const double* W, double n_obs, bool qv_mean, hipStream_t st);
int vgi_sample_coeffs(vggp_ctx* c, VgReadout& r, const char* fn, bool scattered, const double* eps_u, const double* eps_obs, uint64_t seed,
                      unsigned long long s0, int cn, double tol, int max_iter, int* solves, int* max_its, vggp_info* info, hipStream_t st);
// ---- raster.hip: the raster mean of the last step (full-grid state: mean and, with var, variance), axis factor columns A_d = a_d(g_d) ----
int vg_raster_factors(vggp_ctx* c, const double* g1, long p1, const double* g2, long p2, double* A1, double* A2, hipStream_t st);
int vg_raster_full(vggp_ctx* c, const double* g1, long p1, const double* g2, long p2, double* mean, double* var, hipStream_t st);
struct VgRasterAxes { double *A1, *U1, *A2, *U2; };     // [m_d][p_d] each, in the context's scratch: factor columns, U_d = L0_d^-1 A_d
int vg_raster_mspace(vggp_ctx* c, const double* g1, long p1, const double* g2, long p2, double* mean, hipStream_t st,
                     VgRasterAxes* ax = nullptr);
// ---- raster_sample.hip: the samplers' own scratch (c->rs_mem), grown to `bytes` when it is smaller ----
int vg_rs_reserve(vggp_ctx* c, const char* fn, size_t bytes, int nbc);
// ---- dense_sample.hip: the coefficient draw of the dense states, out = Xl^T E on block vectors [m1][nbc][m2] (Xl [M][M] lower
// triangular, cn live columns, the others written as zeros; out != E), and what both of their samplers check before they launch ----
hipError_t vg_tri_t_apply_launch(const double* Xl, long m1, long m2, const double* E, int nbc, int cn, double* out, hipStream_t st);
int vg_dense_sample_enter(vggp_ctx* c, const char* fn, int64_t n_samples, int64_t first, const void* out, int block, vggp_info* info);
// ---- iter_step.hip ---------------------------------------------------------------------------------------------------
__global__ void vgi_transpose_kernel(const double* W, long n1, long n2, double* Wt);
__global__ void vgi_mul_kernel(const double* a, const double* b, long n, double* out);
void vgi_red_job(VgmRedArgs& ra, int k, const double* a, const double* b, long n, long sa, long sb, int op, const double* cc = nullptr);
void vgi_red_jobs(vggp_ctx* c, const VgMasked& w, const double* C0, VgmRedArgs& ra);
double vgi_obs_fraction(const vggp_ctx* c, bool scattered, double n_obs);
int vgi_back(const VgMasked& w, const VgIter& it, const double* L, const double* F, const double* R, double* out, hipStream_t st);
int vgi_pcg(vggp_ctx* c, VgMasked& w, const VgIter& it, double p, double tol, int max_iter, bool history, bool field2, int stale_limit,
            int* iters_out, int* nact_out, hipStream_t st);
int vgs_check(vggp_ctx* c, const char* fn);
