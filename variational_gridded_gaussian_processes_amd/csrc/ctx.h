// Context and per-dimension workspace of libvggp_hip.so (shared by api.hip, step.hip and the M-space solvers of mspace_ws.h).
#pragma once
#include "common.h"

#define VG_MAXEV 40
#define VG_NFORK 4
#define VG_SP_SLABS 4             // split-K slabs of the early projection S' = [A2;dA2] Y (riding in the Cholesky launch)

struct VgDim {
    int kind = 0, basis = 0, n = 0, m = 0;
    double *x = nullptr, *grid = nullptr;
    double *K0 = nullptr, *dK0 = nullptr, *AD = nullptr, *L0 = nullptr, *Linv0 = nullptr, *BV = nullptr;
    double *Kc = nullptr, *Lc = nullptr, *Dc = nullptr;   // 128 < m <= 256: four jittered copies of K0, their factors, their diagonal-block inverses
    int* st8 = nullptr;               // ... and the status words [level][block] of the eight block factorisations
    double* Dinv0 = nullptr;          // [ceil(m/16)][16][16]: inverses of the diagonal blocks of L0 (left by the Cholesky launch)
    double *X = nullptr, *Mk = nullptr, *GH = nullptr, *GHslab = nullptr, *Gw = nullptr;
    double *lam0 = nullptr, *Qt = nullptr, *QtPrev = nullptr, *QtPrev2 = nullptr, *U = nullptr;
    double *Ep = nullptr, *Fp = nullptr, *Wp = nullptr;      // prediction of the next start basis (step.hip rotate_and_reduce)
    double *TM = nullptr, *TH = nullptr, *E = nullptr, *F = nullptr, *RQ = nullptr, *RQsq = nullptr;
    double *chol_scratch = nullptr, *gwork = nullptr, *jitter = nullptr;
    double2* rotlog = nullptr;
    int *roundlog = nullptr, *counters = nullptr, *status = nullptr, *perm = nullptr;
    int gh_split = 1, max_rounds = 0;
    // subspace start (numerically rank-deficient Gram matrices, e.g. RBF): scratch for the r leading rows and the small eigenproblem
    double* Id = nullptr;             // m x m identity ("Id G" through the slab-summing GEMM = the reduced G)
    double *Zs = nullptr, *V1s = nullptr, *Hs = nullptr, *Ws = nullptr, *lam_s = nullptr, *gwork2 = nullptr;
    double2* rotlog2 = nullptr;
    int *roundlog2 = nullptr, *counters2 = nullptr, *perm2 = nullptr;
    int sub_r = 0;                    // rows treated as the numerical range in the next step (0: subspace start off)
    // thin chain (thin.hip): V1 Mk0, V1 H0 (r x m) and V1 Mk0 V1^T, V1 H0 V1^T (r x r)
    double *tMV = nullptr, *tHV = nullptr, *tAM = nullptr, *tAH = nullptr;
    double* Omega = nullptr;          // [VG_THIN_MAXR][m] fixed pseudo-random rows: start of the thin chain's cold range finder
    int thin_rows = 0;                // leading rows of QtPrev that hold eigenvectors (m after a full solve, r after a thin step)
    bool have_prev = false, have_prev2 = false;     // QtPrev / QtPrev2 hold the bases of the last / the step before
};

struct VgGraphKey {
    const void* y = nullptr;
    const void* payload = nullptr;
    double yy = 0.0;
    bool operator==(const VgGraphKey& o) const { return y == o.y && payload == o.payload && yy == o.yy; }
};

typedef VgHostOut HostOut;   // pinned readback block (common.h)

enum { VG_LAST_NONE = 0, VG_LAST_FULL, VG_LAST_DENSE, VG_LAST_ITER };      // vggp_ctx::last_kind

struct vggp_ctx {
    int device = 0;
    bool planned = false;
    vggp_desc desc{};
    VgDim d[2];
    void* arena = nullptr;
    size_t arena_bytes = 0, arena_used = 0;
    // cross-dimension buffers
    double* Sp = nullptr;             // [A2;dA2] Y (split-K slabs): the early projection of the thin chain
    double *St = nullptr, *CCslab = nullptr, *payload = nullptr, *GH1 = nullptr;
    double *T3 = nullptr, *P3 = nullptr, *beta = nullptr, *bl2 = nullptr, *bl1 = nullptr, *invD = nullptr;
    double *rowpart = nullptr, *r1 = nullptr, *r1l = nullptr, *r2 = nullptr, *r2l = nullptr, *dotpart = nullptr, *ol = nullptr;
    double *out = nullptr, *theta = nullptr, *wq = nullptr;
    int st_split = 1, cc_split = 1;
    int st_slabs = 1;                            // ... of S = [B2;V2] Y
    bool dinv_valid = false;                     // Dinv0 holds the diagonal-block inverses of the current L0 (m <= 128 Cholesky path)
    int ride_stage0 = 0;                         // first pending rider of the fused warm step: 0 = S, 1 = [C;C1;C2] (S came out of the early projection)
    int gh_slabs[2] = {1, 1}, cc_slabs = 1;      // split-K slab counts actually produced by the last partials launch
    long payload_len = 0;
    bool have_partials = false, have_step = false, have_masked = false;
    int last_kind = 0;               // VG_LAST_*: which kind of step finished last (vggp_posterior_raster reads "the last step, whichever kind")
    bool have_iter = false;          // the last finished step was a successful vggp_elbo_step_masked_iter / vggp_elbo_step_scattered_iter
                                     // (which of the two: the plan's VGGP_FLAG_SCATTERED; their read-outs: iter_readout.hip)
    void* masked = nullptr;          // VgMasked workspace (mspace_ws.h), allocated on first use
    void* paired = nullptr;          // VgPaired workspace (paired.hip): allocated by a plan with VGGP_FLAG_PAIRED_Z
    bool is_paired = false;          // the current plan is a paired one: only the entries listed in vggp.h apply
    // pinned host staging
    double* h_theta = nullptr;
    HostOut* h_out = nullptr;
    HostOut* d_hout = nullptr;       // device-visible address of h_out
    double* d_htheta = nullptr;      // device-visible address of h_theta
    int* ticket = nullptr;           // last-block ticket of the fused final reduction
    // scratch for the exported building blocks / posterior (lazy)
    void* misc = nullptr;
    size_t misc_bytes = 0;
    void* rs_mem = nullptr;           // workspace of the raster samples (raster_sample.hip): apart from misc, which the roots' Cholesky uses
    size_t rs_bytes = 0;
    double* sumsq_partial = nullptr;
    double* sumsq_out = nullptr;
    // captured step graphs.  Capture is illegal on the legacy default stream, so when the caller passes stream 0 the
    // step runs on `own_stream`, a BLOCKING stream: it is implicitly ordered with the legacy default stream in both
    // directions (uploads / all-reduce issued by torch on stream 0 before, q(v) / posterior calls after).
    hipStream_t own_stream = nullptr;
    // side stream for the branches of a step that do not depend on each other (extrapolated basis || factor + Cholesky;
    // projection of Y || eigensolver chain); under capture the fork / join events become graph edges
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork[VG_NFORK] = {}, ev_join[VG_NFORK] = {};
    bool use_graph = true;
    hipGraphExec_t gexec[20] = {};
    VgGraphKey gkey[20];
    // what the accurate (cold) recompute of the read-outs needs from the last step (step.hip vg_accurate_state)
    bool last_warm = false, last_slabs = false, acc_valid = false;
    const double* last_payload = nullptr;
    double last_yy = 0.0;
    VgGemmBatch ride_proj, ride_cc;   // the projection launches of a fused warm step, deferred to the eigensolver chain as riders
    bool ride_pending = false;
    double last_ell[2] = {0.0, 0.0};  // lengthscales of the previous step (jump detection, vggp_elbo_step)
    bool pred_consumed = false;       // this prediction's Newton-Schulz step has been applied to Fp (it accumulates: once only)
    bool refine_next = false;
    bool sub_next = false;            // the last step's numerical ranks allow the subspace start
    int sub_r_cap[2] = {0, 0};        // ranks the _S graphs were captured with
    double *tCV = nullptr, *tAC = nullptr;   // thin chain: {C, C1, C2} V1_2^T  [3 m1][r2]  and  V1_1 (.)  [3][r1][r2]
    bool cur_thin = false;            // the step in flight runs the thin chain, with these ranks (vg_start_prepare -> finish_collect)
    int cur_r[2] = {0, 0};
    bool cur_extrap = false;          // the step in flight starts from the extrapolated basis
    int cur_newton = 0;               // Newton-chain iterations of the step in flight (0: another chain)
    bool last_newton = false, newton_next = false;
    int newton_block = 0;             // steps for which the Newton chain stays off after a miss
    int newton_iters = 3, newton_cap = 0;
    int newton_ok_run = 0;           // Newton-chain steps since the last miss (the iteration count decays after 64)
    bool last_thin = false;           // the last finished step ran the thin chain: QtPrev holds r rows, the m-space state (beta, 1/D, E, F) is not there
    int thin_block = 0;               // steps for which the thin chain stays off after it missed
    bool thin_off = false;            // a caller needed the full m-space state of a warm step (vggp_zgrad): keep to the full chain from now on
    bool sub_mode = false;            // the current step uses the subspace start (U then holds the identity)         // the last step ended in the polish in both dimensions: refine the next start basis
    // the context's collective (comm.hip)
    int n_ranks = 1, rank = 0;
    void* comm = nullptr;             // ncclComm_t
    bool comm_dead = false;           // the communicator was aborted (a peer failed or timed out): multi-rank steps return VGGP_ERCCL
    vggp_allreduce_fn cb = nullptr;   // host-callback transport (rehearsal / other transports)
    void* cb_user = nullptr;
    int comm_probe = 0;               // vg_comm_verify: 0 not probed yet, 1 the all-reduce sums over n_ranks ranks, -1 it does not
    double comm_probe_sum = 0.0;      // ... and what the probe of 1.0 came back as
    double* h_stage = nullptr;        // pinned staging of the callback transport
    long h_stage_count = 0;
    hipStream_t poll_stream = nullptr;   // the last step's completion was seen in the pinned result block, not through the runtime:
    bool poll_stream_valid = false;      // this stream may still be finishing its graph (step.hip vg_quiesce)
    long seq = 0;                     // step sequence number (h_theta[5] -> device theta[5] -> VgHostOut::seq)
    int warm_run = 0;                 // consecutive warm-started steps (periodic cold restart bounds orthogonality drift)
    // per-stage profiling (bench.py): event e[i] is recorded after stage i-1's launches
    bool prof = false;
    hipEvent_t ev[VG_MAXEV] = {};
    int ev_stage[VG_MAXEV] = {};      // stage charged with the time since the previous event (-1: clock restart)
    int nev = 0;
    double prof_ms[VGGP_NSTAGE] = {};
    int prof_steps = 0;
    void* exact = nullptr;           // VgExact workspace (exact.hip): allocated by vggp_exact_plan, independent of vggp_plan's state
    void* exact_iter = nullptr;      // VgExactIter workspace (exact_iter.hip): allocated by vggp_exact_iter_plan, independent of both
};


// +1: Kuu_d = s_d K0, Kuf_d = s_d A0 (kernel-evaluated bases);  -1: Kuu_d = K0 / s_d, Kuf_d = A0 (inter-domain VFF / B1).
// B = L^{-1} Kuf is sqrt(s) L0^{-1} A0 either way, so only u-space results (q(v)) need the sign.
static inline int vg_uexp(int basis) { return (basis == VGGP_BASIS_VFF || basis == VGGP_BASIS_B1) ? -1 : 1; }

int vg_ensure_misc(vggp_ctx* c, size_t bytes);
// ---- the full-grid step (step.hip)
// a step whose completion was only seen in its pinned block may still be finishing on its stream: wait for that stream
int vg_quiesce(vggp_ctx* c);
void vg_graphs_clear(vggp_ctx* c);                       // drop every captured step graph (re-planning)
int vg_accurate_state(vggp_ctx* c, hipStream_t st);      // read-outs after a warm step: re-run the finish half cold on the resident G, H, C
bool vg_thin_readout(const vggp_ctx* c);                 // api.hip: the read-outs come straight from the last (thin) step's range directions
// the partials half.  early: 1 = thin chain, 2 = regular warm chains ([C;C1;C2] is then the first rider of the eigensolver chain)
struct VgPartials { bool reduce = true, extrap = false, fused = false, apply_ns = false; int early = 0; };
int vg_partials_enqueue(vggp_ctx* c, const double* Y, double* payload, hipStream_t st, const VgPartials& o = VgPartials());
int vg_comm_init(vggp_ctx* c, int n_ranks, int rank, const void* unique_id);
void vg_comm_destroy(vggp_ctx* c);
int vg_allreduce(vggp_ctx* c, double* buf, long count, hipStream_t st);
void vg_comm_abort(vggp_ctx* c);
int vg_comm_wait(vggp_ctx* c, hipStream_t st, const volatile double* seq = nullptr, double want = 0.0);
int vg_comm_verify(vggp_ctx* c, const char* fn);      // the iterative entries: VGGP_EINVAL unless the transport sums over n_ranks ranks
// blocked dense Cholesky + inverse for matrices beyond one workgroup (masked.hip); S is destroyed; status != 0 on failure
#define VG_DENSE_MB 128
struct VgDenseChol { double *S, *L, *X, *DI, *Tmp, *scratch, *jit; int* status; long M; double* Sinv; };
int vg_blocked_chol_inverse(const VgDenseChol& w, hipStream_t st);
void vg_masked_free(vggp_ctx* c);
// paired inducing points (paired.hip; VGGP_FLAG_PAIRED_Z): the entries of vggp.h that apply to a paired plan forward here
int vg_paired_check(const vggp_desc* desc);          // argument checks of a paired plan: touches no state
int vg_paired_plan(vggp_ctx* c, const vggp_desc* desc);
void vg_paired_free(vggp_ctx* c);
int vg_paired_set_inducing(vggp_ctx* c, int dim, const double* z, int64_t m);
int vg_paired_step(vggp_ctx* c, const double* Y, double yy, const double theta[5], double* elbo_out, double grad_out[5],
                   vggp_info* info, hipStream_t st, bool scattered_entry);
int vg_paired_zgrad(vggp_ctx* c, const double* Y, double* gz1, double* gz2, hipStream_t st, bool scattered_entry);
int vg_paired_qv(vggp_ctx* c, double* mean, double* var, hipStream_t st);
int vg_paired_qv_cov(vggp_ctx* c, double* cov, hipStream_t st);
int vg_paired_readout(vggp_ctx* c, const double* C1, int64_t mv1, const double* C2, int64_t mv2, const double* kd1, const double* kd2,
                      double* mean, double* var, int flags, hipStream_t st);
int vg_paired_posterior(vggp_ctx* c, const double* xs1, const double* xs2, int64_t ns, double* mean, double* var, hipStream_t st);
int vg_paired_posterior_cov(vggp_ctx* c, const double* xs1, const double* xs2, int64_t ns, double* cov, hipStream_t st);
void vg_exact_free(vggp_ctx* c);      // exact GP (exact.hip)
void vg_exact_iter_free(vggp_ctx* c); // iterative exact GP (exact_iter.hip)
// entries that have no paired meaning: VGGP_EINVAL with a message
#define VG_NOT_PAIRED(c, fn)                                                                                            \
    do {                                                                                                                \
        if ((c) && (c)->is_paired) {                                                                                    \
            vg_set_error("%s: not available on a context planned with VGGP_FLAG_PAIRED_Z (see vggp.h)", fn);          \
            return VGGP_EINVAL;                                                                                         \
        }                                                                                                               \
    } while (0)
// entries that a paired plan serves through paired.hip: `call` is the vg_paired_* forward, made on the context's device
#define VG_FORWARD_PAIRED(c, call)                                                                                      \
    do {                                                                                                                \
        if ((c) && (c)->is_paired) {                                                                                    \
            if (!(c)->planned) { vg_set_error("context not planned"); return VGGP_ESTATE; }                             \
            VG_ENTER_DEVICE((c)->device);                                                                               \
            return call;                                                                                                \
        }                                                                                                               \
    } while (0)
void vg_masked_new_plan(vggp_ctx* c);
// whitened read-out columns (masked_readout.hip).  columns: factor columns A_d = a_d(x*_d) of cn points and U_d = L0_d^-1 A_d
// ([m_d][cn]);  cross: U_d = L0_d^-1 C_d^T of a gridded read-out's cross-covariances C_d [mv_d][m_d]  ([m_d][mv_d])
int vg_whitened_columns(vggp_ctx* c, const double* xs1, const double* xs2, int cn, double* A1, double* A2, double* U1, double* U2,
                        hipStream_t st);
int vg_whitened_cross(vggp_ctx* c, const double* C1, long mv1, const double* C2, long mv2, double* U1, double* U2, hipStream_t st);
// the Khatri-Rao operator of the iterative scattered step (kr.hip): L [m1][N], R [m2][N], block vectors [m1][nb][m2], fields [nb][N]
hipError_t vg_kr_field_launch(const double* L, const double* R, const double* V, int m1, int m2, long N, int nb, double* F, hipStream_t st);
hipError_t vg_kr_field2_launch(const double* L, const double* R, const double* V, int m1, int m2, long N, int nb, double* F, hipStream_t st);
size_t vg_kr_back_scratch(int m1, int m2, long N, int nb);      // doubles of split scratch vg_kr_back_launch needs (bounded whatever N)
hipError_t vg_kr_back_launch(const double* L, const double* R, const double* F, int m1, int m2, long N, int nb, double* out, double* scratch,
                             hipStream_t st);
// out [mv1][mv2] (+)= sum_k P1[a][k]^2 P2[b][k]^2, P_d [mv_d][N]; scratch: vg_kr_sqgram_scratch doubles (unused when that is mv1 mv2 and !accum)
size_t vg_kr_sqgram_scratch(int mv1, int mv2, long N);
hipError_t vg_kr_sqgram_launch(const double* P1, const double* P2, int mv1, int mv2, long N, double* out, double* scratch, int accum,
                               hipStream_t st);
// joint samples of q(v) (sample.hip): the counter-based normal generator and the elementwise kernels around the block solves.
// Block vectors [m1][nbc][m2], grid fields [n1][nbc][n2] (Wt [n1][n2]), point fields [nbc][N] (Wt null, n1 = N); cn live columns,
// s0 = global number of the block's first sample; eps null: generated from (seed, s0)
hipError_t vg_normal_fill_launch(unsigned long long seed, unsigned stream_id, unsigned long long first, long n, double* out, hipStream_t st);
hipError_t vg_sample_block_noise_launch(double* E, const double* eps, unsigned long long seed, unsigned long long s0, int m1, int nbc, int m2,
                                        int cn, hipStream_t st);
hipError_t vg_sample_field_noise_launch(double* F, const double* Wt, const double* eps, unsigned long long seed, unsigned long long s0, long n1,
                                        int nbc, long n2, int cn, hipStream_t st);
hipError_t vg_sample_fuse_launch(double* Z, const double* K, const double* theta, long n, hipStream_t st);                 // Z += sqrt(rho) K
hipError_t vg_sample_root_scale_launch(double* X, const double* invD, int m1, int nbc, int m2, hipStream_t st);           // X o= sqrt(invD)
hipError_t vg_sample_out_launch(const double* Y, const double* mean, const double* theta, int e1, int e2, int m1, int nbc, int m2, int cn,
                                double* out, hipStream_t st);                                                            // out[c] = mean + sqrt(s1^e1 s2^e2) Y[:, c, :]
// the same noise kernels on any stream of the generator (raster samples): rows [m1][nbc][w] from eps[c][a][b] or idx = (s0 + c) m1 w + a w + b
hipError_t vg_sample_rows_noise_launch(double* E, const double* eps, unsigned long long seed, unsigned stream_id, unsigned long long s0, int m1,
                                       int nbc, long w, int cn, hipStream_t st);
// x[i] *= sqrt(s1 s2) for i < n  (theta: the device hyper-parameters)
hipError_t vg_sample_scale_root_launch(double* x, long n, const double* theta, hipStream_t st);
// A[i][i] += eta (p x p)
hipError_t vg_sample_nugget_launch(double* A, long p, double eta, hipStream_t st);
// the coefficient draw of the full-grid samplers (api.hip): Xa [m1][nbc][m2] = (Q1^T E Q2) o D^-1/2; Xb: scratch of the same size
int vg_sample_full_coeffs(vggp_ctx* c, const double* eps, unsigned long long seed, unsigned long long s0, int nbc, int cn, double* Xa, double* Xb,
                          hipStream_t st);
// batch of triangular solves, each in place on its X (api.hip: element (row k, column c) at X[k * sk + c * sc])
#define VG_TRSM_BLK 128
struct VgTrsmSpec {
    const double* L; long ldl;
    const double* Dinv; long dinv_blk, dinv_ld;
    double* X; long sk, sc, ncols;
    long m; int trans;
};
int vg_trsm_batch(const VgTrsmSpec* sp, int n, hipStream_t st);
