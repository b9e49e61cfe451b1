// C-ABI of libvggp_hip.so (include/vggp.h): context, plan and workspace arena, the read-outs (q(v), posterior,
// gridded read-out), the stand-alone building blocks, vggp_zgrad and the profiling / diagnostic entries.  The ELBO step
// itself lives in step.hip.  Host logic only -- every number is produced by the HIP kernels in factor_build.hip,
// chol.hip, gemm.hip, eigh.hip and mspace.hip.  There is no CPU fallback: without a gfx950 device every entry point
// returns VGGP_EHIP.
#include "common.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

// ---------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void vg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* vggp_last_error(void) { return g_err; }
extern "C" int vggp_version(void) { return VGGP_VERSION; }

#include "arena.h"
#include "ctx.h"
#include "factor_elem.h"

static const char* VG_STAGE_NAMES[VGGP_NSTAGE] = {
    "factor_build", "cholesky_inverse", "trsm_BV(L^-1[A|dA|dK])", "extrap_basis(3 small gemms)", "gemm_project(S=[B2;V2]Y)",
    "gemm_C(B1*S)", "gemm_gram(G,H,Mk)", "reduce_slabs", "warm_first_gemm([Z,G]|TM)", "rowqr|refine", "warm_mid_gemms",
    "ritz_eigh", "warm_last_gemms(->Gw)", "jacobi_eigh+replay(fused)", "gemm_rotate_right", "gemm_rotate_left", "dstage",
    "gemm_betaGram", "final_reduce", "(unused)"};
extern "C" const char* vggp_stage_name(int i) { return (i >= 0 && i < VGGP_NSTAGE) ? VG_STAGE_NAMES[i] : ""; }

int vg_ensure_misc(vggp_ctx* c, size_t bytes) {
    if (c->misc_bytes >= bytes) return VGGP_OK;
    if (c->misc) { VG_HIP(hipFree(c->misc)); c->misc = nullptr; c->misc_bytes = 0; }
    VG_HIP(hipMalloc(&c->misc, bytes));
    c->misc_bytes = bytes;
    return VGGP_OK;
}

extern "C" int vggp_create(vggp_ctx** out, int device, int n_ranks, int rank, const void* unique_id) {
    if (!out) { vg_set_error("vggp_create: null out"); return VGGP_EINVAL; }
    VG_REQUIRE(n_ranks >= 1 && rank >= 0 && rank < n_ranks, "vggp_create: rank %d of %d", rank, n_ranks);
    int ndev = 0;
    VG_HIP(hipGetDeviceCount(&ndev));
    VG_REQUIRE(device >= 0 && device < ndev, "vggp_create: device %d out of range (%d devices)", device, ndev);
    VG_ENTER_DEVICE(device);
    hipDeviceProp_t prop;
    VG_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        vg_set_error("vggp_create: device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
        return VGGP_EHIP;
    }
    VG_HIP(vg_chol_setup());
    VG_HIP(vg_eigh_setup());
    VG_HIP(vg_trsm_setup());
    VG_HIP(vg_thin_tail_setup());
    vggp_ctx* c = new (std::nothrow) vggp_ctx();
    if (!c) { vg_set_error("out of host memory"); return VGGP_ENOMEM; }
    c->device = device;
    const char* ng = getenv("VGGP_NO_GRAPH");
    c->use_graph = !(ng && ng[0] == '1');
    VG_HIP(hipStreamCreate(&c->own_stream));
    VG_HIP(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
    for (int i = 0; i < VG_NFORK; ++i) {
        VG_HIP(hipEventCreateWithFlags(&c->ev_fork[i], hipEventDisableTiming));
        VG_HIP(hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming));
    }
    VG_HIP(hipHostMalloc((void**)&c->h_theta, 8 * sizeof(double), hipHostMallocDefault));
    VG_HIP(hipHostMalloc((void**)&c->h_out, sizeof(HostOut), hipHostMallocDefault));
    VG_HIP(hipHostGetDevicePointer((void**)&c->d_hout, c->h_out, 0));
    VG_HIP(hipHostGetDevicePointer((void**)&c->d_htheta, c->h_theta, 0));
    VG_HIP(hipMalloc((void**)&c->ticket, 4 * sizeof(int)));
    VG_HIP(hipMemset(c->ticket, 0, 4 * sizeof(int)));
    VG_HIP(hipMalloc((void**)&c->sumsq_partial, 1024 * sizeof(double)));
    VG_HIP(hipMalloc((void**)&c->sumsq_out, 8 * sizeof(double)));
    const int rcc = vg_comm_init(c, n_ranks, rank, unique_id);
    if (rcc) { (void)vggp_destroy(c); return rcc; }
    *out = c;
    return VGGP_OK;
}

extern "C" int vggp_destroy(vggp_ctx* c) {
    if (!c) return VGGP_OK;
    VgDeviceGuard guard;
    (void)guard.enter(c->device);
    (void)vg_quiesce(c);
    for (int i = 0; i < 20; ++i) if (c->gexec[i]) (void)hipGraphExecDestroy(c->gexec[i]);
    for (int i = 0; i < VG_MAXEV; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    for (int i = 0; i < VG_NFORK; ++i) {
        if (c->ev_fork[i]) (void)hipEventDestroy(c->ev_fork[i]);
        if (c->ev_join[i]) (void)hipEventDestroy(c->ev_join[i]);
    }
    if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
    vg_masked_free(c);
    vg_paired_free(c);
    vg_exact_free(c);
    vg_exact_iter_free(c);
    vg_comm_destroy(c);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->arena) (void)hipFree(c->arena);
    if (c->misc) (void)hipFree(c->misc);
    if (c->rs_mem) (void)hipFree(c->rs_mem);
    if (c->h_theta) (void)hipHostFree(c->h_theta);
    if (c->h_out) (void)hipHostFree(c->h_out);
    if (c->ticket) (void)hipFree(c->ticket);
    if (c->sumsq_partial) (void)hipFree(c->sumsq_partial);
    if (c->sumsq_out) (void)hipFree(c->sumsq_out);
    delete c;
    return VGGP_OK;
}

static int pick_split(int tiles, int K, int target) {
    int s = (target + tiles - 1) / tiles;
    int maxs = std::max(1, K / (4 * VG_BK));
    return std::max(1, std::min(s, maxs));
}

// number of doubles in the host/device `grid` array of a dimension
static long vg_grid_len(int basis, long m) {
    if (basis == VGGP_BASIS_B0 || basis == VGGP_BASIS_B0K) return m + 1;      // mesh knots
    if (basis == VGGP_BASIS_VFF) return 2 + (m - 1) / 2 + 1;  // a, b, omega_0 .. omega_M (m = 2M + 1)
    return m;                                                 // points / B1 knots / trivial
}
static void layout(vggp_ctx* c, VgArena& b) {
    // Allocation ORDER matters: the small kernels of a step are latency chains whose first loads miss everything
    // (the producer ran on another XCD), and each distinct 2 MB region they touch adds an address-translation miss on
    // top.  So the arrays are grouped by the stage that reads them -- tail (m-space) arrays together, eigen-stage arrays
    // together, factor-stage arrays together -- and the large streaming buffers (operands over the grid, split-K slabs,
    // rotation log) come last.
    const vggp_desc& D = c->desc;
    const long n1 = D.n1, n2 = D.n2, m1 = D.m1, m2 = D.m2;
    // ---- tail: m-space stage and final reduction
    c->out = b.take<double>(8);
    c->theta = b.take<double>(8);
    c->rowpart = b.take<double>(m1 * 8);
    c->r1 = b.take<double>(m1);
    c->r1l = b.take<double>(m1);
    c->r2 = b.take<double>(2 * m2);          // [r2; r2l]: the two rows of one GEMM output
    c->r2l = c->r2 + m2;
    c->dotpart = b.take<double>(64 * 4);    // [4][64] per-tile partial sums (unused slots stay zero: the arena is cleared at plan time)
    c->ol = b.take<double>(2 * m1);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        const long m = d.m, m2e = m + (m & 1);
        d.lam0 = b.take<double>(m);
        d.jitter = b.take<double>(2);
        d.counters = b.take<int>(8);
        d.counters2 = d.counters + 4;
        d.perm = b.take<int>(m2e);
        d.perm2 = b.take<int>(m2e);
        d.lam_s = b.take<double>(m);
        d.status = b.take<int>(2);
    }
    c->invD = b.take<double>(m1 * m2);
    c->beta = b.take<double>(m1 * m2);
    c->bl2 = b.take<double>(m1 * m2);
    c->bl1 = b.take<double>(m1 * m2);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        d.E = b.take<double>((long)d.m * d.m);
        d.F = b.take<double>((long)d.m * d.m);
    }
    c->P3 = b.take<double>(3 * m1 * m2);
    c->T3 = b.take<double>(3 * m1 * m2);
    // ---- eigen stage
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        const long m = d.m;
        d.TM = b.take<double>(m * m);
        d.TH = b.take<double>(m * m);
        d.Qt = b.take<double>(m * m);
        d.QtPrev = b.take<double>(m * m);
        d.QtPrev2 = b.take<double>(m * m);
        d.U = b.take<double>(m * m);
        d.Ep = b.take<double>(m * m);
        d.Fp = b.take<double>(m * m);
        d.Wp = b.take<double>(m * m);
        d.Id = b.take<double>(m * m);
        d.Gw = b.take<double>(m * m);
        d.GH = b.take<double>(2 * m * m);
        d.Mk = b.take<double>(m * m);
    }
    c->payload_len = 2 * m2 * m2 + 3 * m1 * m2;
    c->payload = b.take<double>(c->payload_len + 8);      // + the peer-failure word of a multi-rank step (payload[payload_len])
    // ---- factor stage
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        const long m = d.m;
        const int glen = (int)vg_grid_len(d.basis, m);
        d.grid = b.take<double>(glen);
        d.K0 = b.take<double>(m * m);
        d.dK0 = b.take<double>(m * m);
        d.L0 = b.take<double>(m * m);
        d.Linv0 = b.take<double>(m * m);
        d.Dinv0 = b.take<double>(((m + 15) / 16) * 256);
        if (m > 128) {                   // blocked Cholesky of the step (vg_chol_big_enqueue)
            d.Kc = b.take<double>(4 * m * m); d.Lc = b.take<double>(4 * m * m); d.Dc = b.take<double>(4 * ((m + 15) / 16) * 256);
            d.st8 = b.take<int>(8);
        }
        d.X = b.take<double>(m * m);
        d.chol_scratch = b.take<double>(m * (m + 1));
        d.RQ = b.take<double>(m * m);
        d.RQsq = b.take<double>(m * m);
    }
    c->wq = b.take<double>(2 * m1 * m2);
    // ---- large streaming buffers
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        const long m = d.m, n = d.n, m2e = m + (m & 1);
        d.x = b.take<double>(n);
        d.AD = b.take<double>(2 * m * n);
        d.BV = b.take<double>(2 * m * n);
        static const char* ghe = getenv("VGGP_GH_TARGET");
        d.gh_split = pick_split((int)(((m + 63) / 64) * ((m + 63) / 64)), (int)n, ghe ? atoi(ghe) : 32);
        d.GHslab = b.take<double>((size_t)d.gh_split * 2 * m * m);
        d.gwork = b.take<double>(m2e * (m2e + 1));
        d.max_rounds = (int)(VG_EIG_MAXSWEEP * (m2e - 1));
        d.rotlog = b.take<double2>(vg_eigh_log_bytes((int)m) / sizeof(double2) + 1);
        d.roundlog = b.take<int>(d.max_rounds);
        if (m >= 24 && m <= 256) {       // subspace start: the small problem has at most m/2 rows (m > 128: the thin chain only)
            d.gwork2 = b.take<double>(m2e * (m2e + 1));
            d.rotlog2 = b.take<double2>(vg_eigh_log_bytes((int)m) / sizeof(double2) + 1);
            d.roundlog2 = b.take<int>(d.max_rounds);
            d.Zs = b.take<double>(m * m); d.V1s = b.take<double>(m * m); d.Hs = b.take<double>(m * m); d.Ws = b.take<double>(m * m);
            d.tMV = b.take<double>(VG_THIN_MAXR * m); d.tHV = b.take<double>(VG_THIN_MAXR * m);
            d.tAM = b.take<double>(VG_THIN_MAXR * VG_THIN_MAXR); d.tAH = b.take<double>(VG_THIN_MAXR * VG_THIN_MAXR);
            d.Omega = b.take<double>(VG_THIN_MAXR * m);
        }
    }
    const int st_tiles = (int)(((2 * m2 + 63) / 64) * ((n1 + 63) / 64));
    static const char* ste = getenv("VGGP_ST_TARGET");
    c->st_split = pick_split(st_tiles, (int)n2, ste ? atoi(ste) : 256);
    c->St = b.take<double>((size_t)std::max(c->st_split, VG_SP_SLABS) * 2 * m2 * n1);   // (the early projection leaves up to VG_SP_SLABS slabs of S here)
    c->Sp = b.take<double>((size_t)VG_SP_SLABS * 2 * m2 * n1);       // [A2;dA2] Y of the thin chain's early projection (split-K slabs)
    const int cc_tiles = (int)(((2 * m1 + 63) / 64) * ((m2 + 63) / 64));
    const char* cce = getenv("VGGP_CC_TARGET");
    c->cc_split = pick_split(cc_tiles, (int)n1, cce ? atoi(cce) : 64);
    c->CCslab = b.take<double>((size_t)c->cc_split * 3 * m1 * m2);
    c->tCV = b.take<double>(3 * m1 * VG_THIN_MAXR);
    c->tAC = b.take<double>(3 * VG_THIN_MAXR * VG_THIN_MAXR + 64);      // (+ 64 words of phase stamps in diagnostic builds)
}

static int check_dim(int kind, int basis, long n, long m, const char* which) {
    VG_REQUIRE(kind >= 0 && kind <= 3, "vggp_plan: bad kind for %s", which);
    VG_REQUIRE(basis >= 0 && basis <= 5, "vggp_plan: bad basis for %s", which);
    VG_REQUIRE(!((basis == VGGP_BASIS_VFF || basis == VGGP_BASIS_B1) && kind != VGGP_KIND_MATERN12),
               "vggp_plan: the VFF and B1 features exist for Matern-1/2 only (%s)", which);
    VG_REQUIRE(!(basis == VGGP_BASIS_VFF && (m < 3 || (m & 1) == 0)), "vggp_plan: VFF needs m = 2M + 1 >= 3 (%s)", which);
    VG_REQUIRE(!(basis == VGGP_BASIS_B1 && m < 2), "vggp_plan: B1 needs at least 2 knots (%s)", which);
    VG_REQUIRE(!(basis == VGGP_BASIS_B0 && kind != VGGP_KIND_MATERN12),
               "vggp_plan: the B0 basis exists for Matern-1/2 only (%s)", which);
    VG_REQUIRE(!(basis == VGGP_BASIS_B0K && kind == VGGP_KIND_RBF),
               "vggp_plan: the B0K cells exist for the Matern-1/2, -3/2 and -5/2 kernels (%s)", which);
    VG_REQUIRE(n >= 1, "vggp_plan: %s has no observations", which);
    VG_REQUIRE(m >= 1 && m <= 256, "vggp_plan: m=%ld for %s outside [1, 256]", m, which);
    VG_REQUIRE(!(basis == VGGP_BASIS_ONE && m != 1), "vggp_plan: BASIS_ONE needs m=1 (%s)", which);
    return VGGP_OK;
}

extern "C" int vggp_plan(vggp_ctx* c, const vggp_desc* desc) {
    if (!c || !desc) { vg_set_error("vggp_plan: null argument"); return VGGP_EINVAL; }
    VG_ENTER_DEVICE(c->device);
    int rc;
    if (desc->flags & VGGP_FLAG_PAIRED_Z) {        // paired inducing points: a workspace of their own (paired.hip), no per-dimension plan
        if ((rc = vg_paired_check(desc))) return rc;          // (refused arguments: the previous plan and its state stay as they are)
        c->planned = false;
        vg_graphs_clear(c);
        VG_HIP(hipDeviceSynchronize());
        c->have_partials = c->have_step = c->have_masked = c->have_iter = false;
        c->acc_valid = false; c->last_payload = nullptr;
        c->is_paired = false;
        if ((rc = vg_paired_plan(c, desc))) return rc;
        c->desc = *desc;
        c->desc.x1 = c->desc.x2 = c->desc.grid1 = c->desc.grid2 = nullptr;
        c->desc.n_total = (desc->flags & VGGP_FLAG_SCATTERED) ? desc->n1 : desc->n1 * desc->n2;     // (single-rank: all observations)
        c->payload_len = 0;
        c->is_paired = true;
        c->planned = true;
        return VGGP_OK;
    }
    if (c->is_paired || c->paired) { VG_HIP(hipDeviceSynchronize()); vg_paired_free(c); c->is_paired = false; }
    if ((rc = check_dim(desc->kind1, desc->basis1, desc->n1, desc->m1, "dimension 1"))) return rc;
    if ((rc = check_dim(desc->kind2, desc->basis2, desc->n2, desc->m2, "dimension 2"))) return rc;
    VG_REQUIRE(!((desc->basis1 == VGGP_BASIS_B0K || desc->basis2 == VGGP_BASIS_B0K) && (desc->flags & VGGP_FLAG_B0_F32_KDELTA)),
               "vggp_plan: VGGP_FLAG_B0_F32_KDELTA does not go with VGGP_BASIS_B0K");
    VG_REQUIRE(desc->x1 && desc->x2, "vggp_plan: null coordinate arrays");
    VG_REQUIRE((desc->basis1 == VGGP_BASIS_ONE || desc->grid1) && (desc->basis2 == VGGP_BASIS_ONE || desc->grid2),
               "vggp_plan: null grid arrays");
    if (desc->flags & VGGP_FLAG_SCATTERED)
        VG_REQUIRE(desc->n1 == desc->n2 && desc->basis1 != VGGP_BASIS_ONE && desc->basis2 != VGGP_BASIS_ONE,
                   "vggp_plan: scattered points need n1 == n2 (one coordinate pair per point) and two real dimensions");
    else
        VG_REQUIRE(desc->n_total >= desc->n1 * desc->n2, "vggp_plan: n_total smaller than the local grid");
    VG_REQUIRE(desc->n1 < (1L << 24) && desc->n2 < (1L << 24), "vggp_plan: grid axis too long");
    c->planned = false;
    vg_graphs_clear(c);
    VG_HIP(hipDeviceSynchronize());
    c->warm_run = 0;
    c->refine_next = false;
    c->sub_next = false; c->sub_mode = false; c->sub_r_cap[0] = c->sub_r_cap[1] = 0;
    c->pred_consumed = false;
    c->acc_valid = false; c->last_warm = false; c->last_slabs = false; c->last_payload = nullptr;
    c->last_thin = false; c->thin_off = false; c->thin_block = 0;
    c->cur_newton = 0; c->last_newton = false; c->newton_next = false; c->newton_block = 0; c->newton_iters = 3; c->newton_ok_run = 0;
    c->desc = *desc;
    c->d[0] = VgDim();
    c->d[1] = VgDim();
    c->d[0].kind = desc->kind1; c->d[0].basis = desc->basis1; c->d[0].n = (int)desc->n1; c->d[0].m = (int)desc->m1;
    c->d[1].kind = desc->kind2; c->d[1].basis = desc->basis2; c->d[1].n = (int)desc->n2; c->d[1].m = (int)desc->m2;
    bool grew = false;      // (grow-only; the whole used part is cleared: "unused slots stay zero")
    if ((rc = vg_arena_carve(&c->arena, &c->arena_bytes, nullptr, &grew, [&](VgArena& a) { layout(c, a); }, &c->arena_used))) return rc;
    VG_HIP(hipMemset(c->arena, 0, c->arena_used));
    const double one = 1.0;
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        const double* hx = k == 0 ? desc->x1 : desc->x2;
        const double* hg = k == 0 ? desc->grid1 : desc->grid2;
        VG_HIP(hipMemcpy(d.x, hx, sizeof(double) * d.n, hipMemcpyHostToDevice));
        if (d.basis == VGGP_BASIS_ONE) {
            VG_HIP(hipMemcpy(d.grid, &one, sizeof(double), hipMemcpyHostToDevice));
        } else {
            const int glen = (int)vg_grid_len(d.basis, d.m);
            VG_HIP(hipMemcpy(d.grid, hg, sizeof(double) * glen, hipMemcpyHostToDevice));
        }
    }
    for (int k = 0; k < 2; ++k) VG_HIP(vg_identity_launch(c->d[k].Id, c->d[k].m, nullptr));
    for (int k = 0; k < 2; ++k) {          // start rows of the cold range finder (vg_cold_thin_prepass): fixed pseudo-random numbers in (-1, 1)
        VgDim& d = c->d[k];
        if (!d.Omega) continue;
        std::vector<double> om((size_t)VG_THIN_MAXR * d.m);
        unsigned long long z = 0x9E3779B97F4A7C15ull * (unsigned long long)(k + 1);
        for (double& v : om) {
            z += 0x9E3779B97F4A7C15ull;                          // splitmix64
            unsigned long long x = z;
            x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; x ^= x >> 31;
            v = (double)(x >> 11) * (2.0 / 9007199254740992.0) - 1.0;
        }
        VG_HIP(hipMemcpy(d.Omega, om.data(), sizeof(double) * om.size(), hipMemcpyHostToDevice));
    }
    VG_HIP(hipDeviceSynchronize());
    c->desc.x1 = c->desc.x2 = c->desc.grid1 = c->desc.grid2 = nullptr;   // host pointers not retained
    c->have_partials = c->have_step = c->have_masked = c->have_iter = false;
    vg_masked_new_plan(c);
    c->planned = true;
    return VGGP_OK;
}

// New coordinates for the inducing points of a "points" basis WITHOUT re-planning: the device array is overwritten in place, so
// the arena, the captured graphs (they hold the pointer, not the values) and the warm start all stay -- a small move of Z changes
// the Gram matrices as little as a small move of the lengthscale does, and the subspace start checks itself (VG_ESUBMISS).  This
// is what an optimiser that trains Z (kronecker_structure.py:303-304) calls between steps.
extern "C" int vggp_set_inducing(vggp_ctx* c, int dim, const double* z, int64_t m) {
    VG_FORWARD_PAIRED(c, vg_paired_set_inducing(c, dim, z, m));
    if (!c || !c->planned) { vg_set_error("vggp_set_inducing: context not planned"); return VGGP_ESTATE; }
    VG_REQUIRE(dim == 0 || dim == 1, "vggp_set_inducing: dim must be 0 or 1");
    VgDim& d = c->d[dim];
    VG_REQUIRE(d.basis == VGGP_BASIS_POINTS, "vggp_set_inducing: dimension %d does not use the points basis", dim + 1);
    VG_REQUIRE(z && m == d.m, "vggp_set_inducing: expected %d coordinates, got %lld", d.m, (long long)m);
    for (int64_t i = 0; i < m; ++i) VG_REQUIRE(std::isfinite(z[i]), "vggp_set_inducing: z[%lld] is not finite", (long long)i);
    VG_ENTER_DEVICE(c->device);
    VG_HIP(hipStreamSynchronize(c->own_stream));              // no step of this context is reading the old coordinates
    VG_HIP(hipMemcpy(d.grid, z, sizeof(double) * m, hipMemcpyHostToDevice));
    c->have_step = false; c->have_partials = false; c->have_masked = false; c->have_iter = false; c->acc_valid = false;      // read-outs need a new step
    return VGGP_OK;
}

extern "C" int64_t vggp_payload_len(const vggp_ctx* c) { return (c && c->planned) ? c->payload_len : 0; }
extern "C" int64_t vggp_workspace_bytes(const vggp_ctx* c) { return c ? (int64_t)c->arena_used : 0; }

// ---------------------------------------------------------------------------------
// ---- triangular solves for any m: blocked substitution ------------------------------------------------------------------
// A batch of solves, each in place on its X (element (row k, column c) at X[k * sk + c * sc], one of the two strides is 1).
// m <= 128: one launch of the strip kernel (trsm.hip).  Larger m: block rows of VG_TRSM_BLK = 128; per block row ONE MFMA
// GEMM launch subtracts the contribution of the block rows already solved (L[b, :b] X[:b], all workgroups of the chip, all
// jobs of the batch) and ONE strip-kernel launch solves the 128 x 128 diagonal blocks (factor staged in LDS).
// Dinv: inverses of the 16 x 16 diagonal blocks of L, block b16 at Dinv + b16 * dinv_blk, row stride dinv_ld.
int vg_trsm_batch(const VgTrsmSpec* sp, int n, hipStream_t st) {
    int max_nblk = 0;
    for (int j = 0; j < n; ++j) max_nblk = std::max(max_nblk, (int)((sp[j].m + VG_TRSM_BLK - 1) / VG_TRSM_BLK));
    for (int s = 0; s < max_nblk; ++s) {
        VgGemmBatch g;
        vg_gemm_init(&g);
        VgTrsmJob tj[12];
        int nt = 0;
        for (int j = 0; j < n; ++j) {
            const VgTrsmSpec& q = sp[j];
            const int nblk = (int)((q.m + VG_TRSM_BLK - 1) / VG_TRSM_BLK);
            if (s >= nblk) continue;
            const int b = q.trans ? nblk - 1 - s : s;
            const long r0 = (long)b * VG_TRSM_BLK, rb = std::min<long>(VG_TRSM_BLK, q.m - r0), r1 = r0 + rb;
            // rows of X already solved: [0, r0) for L X = R, [r1, m) for L^T X = R
            const long k0 = q.trans ? r1 : 0, kn = q.trans ? q.m - r1 : r0;
            if (kn > 0) {
                // operator block T (rb x kn): T[i][k] = L[r0 + i][k0 + k] (no trans) or L[k0 + k][r0 + i] (trans)
                const double* Tp = q.trans ? q.L + k0 * q.ldl + r0 : q.L + r0 * q.ldl + k0;
                const long t_i = q.trans ? 1 : q.ldl, t_k = q.trans ? q.ldl : 1;
                if (q.sc == 1)        // X row-major: X[r0:r1, :] -= T X[k0:k0+kn, :]
                    vg_gemm_add(&g, Tp, t_i, t_k, q.X + k0 * q.sk, q.sk, 1, q.X + r0 * q.sk, (int)q.sk, (int)rb, (int)q.ncols, (int)kn,
                                1, 0, 1, 0, -1.0, 1);
                else                  // X holds the transposed right-hand sides: X'[:, r0:r1] -= X'[:, k0:k0+kn] T^T
                    vg_gemm_add(&g, q.X + k0, q.sc, 1, Tp, t_k, t_i, q.X + r0, (int)q.sc, (int)q.ncols, (int)rb, (int)kn, 1, 0, 1, 0,
                                -1.0, 1);
            }
            if (nt >= 12) { vg_set_error("trsm_batch: too many jobs"); return VGGP_EINVAL; }
            tj[nt++] = VgTrsmJob{q.L + r0 * q.ldl + r0, q.Dinv + (r0 / 16) * q.dinv_blk, q.X + r0 * q.sk, q.X + r0 * q.sk, q.ldl,
                                 q.dinv_blk, q.dinv_ld, q.sk, q.sc, q.sk, q.sc, q.ncols, (int)rb, q.trans};
        }
        if (g.nprob) VG_HIP(vg_gemm_launch(&g, st));
        if (nt) VG_HIP(vg_trsm_launch(tj, nt, st));
    }
    return VGGP_OK;
}
static int trsm_inplace(const double* L, long m, long ldl, const double* Dinv, double* X, long x_sk, long x_sc, long ncols,
                        int trans, hipStream_t st) {
    VgTrsmSpec q{L, ldl, Dinv, 256, 16, X, x_sk, x_sc, ncols, m, trans};
    return vg_trsm_batch(&q, 1, st);
}

// ---------------------------------------------------------------------------------
// q(v): mean = R1 (beta/v) R2^T, diag cov = (R1 o R1)(1/D)(R2 o R2)^T, R_d = sqrt(s_d) L0_d Q_d
// Read-outs straight from a THIN step (no cold recompute): beta and 1/D - 1 vanish outside range x range, so
//   q(v) mean      = R1r (beta sqrt(s1 s2) / v) R2r^T,                              R_dr = L0_d E_r^T  (m_d x r_d: range columns only)
//   q(v) variance  = s1 s2 [ rowsq(L0_1) rowsq(L0_2)^T + (R1r o R1r)(1/D - 1)(R2r o R2r)^T ]   (sum over ALL directions of R^2 = diag L0 L0^T)
//   posterior(x*)  = the full formulas with t_d = E_r L0_d^-1 a_d(x*)  (r_d x n*)
// and the range eigenpairs of a thin step are exact Ritz pairs of G on span(V1) = range(G) -- consistent (eigenvalue, eigenvector)
// pairs, unlike the projected-off complement rows of the full warm chain whose mixtures made the cold recompute necessary
// (DESIGN.md section 2).  VGGP_NO_THIN_READOUT=1: recompute cold as after any warm step.
bool vg_thin_readout(const vggp_ctx* c) {
    static const bool off = getenv("VGGP_NO_THIN_READOUT") != nullptr;
    return !off && c->have_step && c->last_thin && !c->acc_valid;
}
__global__ void vg_rowsq_kernel(const double* L, int m, double* out) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= m) return;
    double s = 0.0;
    for (int k = 0; k <= a; ++k) s += L[(long)a * m + k] * L[(long)a * m + k];
    out[a] = s;
}
__global__ void vg_add_outer_kernel(double* x, const double* u, const double* v, int m1, int m2) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (long)m1 * m2) x[i] += u[i / m2] * v[i % m2];
}
static int vg_qv_thin(vggp_ctx* c, double* mean, double* var, hipStream_t st) {
    const long m1 = c->desc.m1, m2 = c->desc.m2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const int r1 = d1.thin_rows, r2 = d2.thin_rows;
    VgGemmBatch g;
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        vg_gemm_add(&g, d.L0, d.m, 1, d.QtPrev, 1, d.m, d.RQ, d.thin_rows, d.m, d.thin_rows, d.m);           // L0 E_r^T  (m x r)
    }
    VG_HIP(vg_gemm_launch(&g, st));
    for (int k = 0; k < 2; ++k) VG_HIP(vg_scale_sq_launch(c->d[k].RQ, c->d[k].RQsq, (long)c->d[k].m * c->d[k].thin_rows, st));
    VG_HIP(vg_qv_weights_launch(c->theta, c->beta, c->invD, c->wq, (long)r1 * r2, st, vg_uexp(d1.basis), vg_uexp(d2.basis)));
    vg_gemm_init(&g);
    vg_gemm_add(&g, d1.RQ, r1, 1, c->wq, r2, 1, c->T3, r2, (int)m1, r2, r1);
    vg_gemm_add(&g, d1.RQsq, r1, 1, c->wq + (long)r1 * r2, r2, 1, c->T3 + m1 * m2, r2, (int)m1, r2, r1);
    VG_HIP(vg_gemm_launch(&g, st));
    vg_gemm_init(&g);
    vg_gemm_add(&g, c->T3, r2, 1, d2.RQ, 1, r2, mean, (int)m2, (int)m1, (int)m2, r2);
    vg_gemm_add(&g, c->T3 + m1 * m2, r2, 1, d2.RQsq, 1, r2, var, (int)m2, (int)m1, (int)m2, r2);
    VG_HIP(vg_gemm_launch(&g, st));
    double* rs1 = c->rowpart;            // (m1 * 8 doubles of scratch, free outside a step)
    double* rs2 = c->r2;                 // (2 * m2)
    hipLaunchKernelGGL(vg_rowsq_kernel, dim3((unsigned)((m1 + 127) / 128)), dim3(128), 0, st, d1.L0, (int)m1, rs1);
    hipLaunchKernelGGL(vg_rowsq_kernel, dim3((unsigned)((m2 + 127) / 128)), dim3(128), 0, st, d2.L0, (int)m2, rs2);
    hipLaunchKernelGGL(vg_add_outer_kernel, dim3((unsigned)((m1 * m2 + 255) / 256)), dim3(256), 0, st, var, rs1, rs2, (int)m1, (int)m2);
    VG_HIP(hipGetLastError());
    VG_HIP(vg_scale_launch(var, m1 * m2, c->theta, 0, st, vg_uexp(d1.basis), vg_uexp(d2.basis)));
    return VGGP_OK;
}

static int build_RQ(vggp_ctx* c, hipStream_t st) {
    VgGemmBatch g;
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        vg_gemm_add(&g, d.L0, d.m, 1, d.QtPrev, 1, d.m, d.RQ, d.m, d.m, d.m, d.m);   // L0 Q (QtPrev = last basis)
    }
    VG_HIP(vg_gemm_launch(&g, st));
    for (int k = 0; k < 2; ++k) VG_HIP(vg_scale_sq_launch(c->d[k].RQ, c->d[k].RQsq, (long)c->d[k].m * c->d[k].m, st));
    return VGGP_OK;
}

extern "C" int vggp_qv(vggp_ctx* c, double* mean, double* var, void* stream) {
    VG_NOT_PAIRED(c, "vggp_qv");
    if (!c || !c->have_step) { vg_set_error("vggp_qv: no finished ELBO step"); return VGGP_ESTATE; }
    VG_REQUIRE(mean && var, "vggp_qv: null output");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const long m1 = c->desc.m1, m2 = c->desc.m2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    if (vg_thin_readout(c)) return vg_qv_thin(c, mean, var, st);
    int rc = vg_accurate_state(c, st);
    if (rc) return rc;
    if ((rc = build_RQ(c, st))) return rc;
    VG_HIP(vg_qv_weights_launch(c->theta, c->beta, c->invD, c->wq, m1 * m2, st, vg_uexp(d1.basis), vg_uexp(d2.basis)));
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, d1.RQ, m1, 1, c->wq, m2, 1, c->T3, (int)m2, (int)m1, (int)m2, (int)m1);
    vg_gemm_add(&g, d1.RQsq, m1, 1, c->invD, m2, 1, c->T3 + m1 * m2, (int)m2, (int)m1, (int)m2, (int)m1);
    VG_HIP(vg_gemm_launch(&g, st));
    vg_gemm_init(&g);
    vg_gemm_add(&g, c->T3, m2, 1, d2.RQ, 1, m2, mean, (int)m2, (int)m1, (int)m2, (int)m2);
    vg_gemm_add(&g, c->T3 + m1 * m2, m2, 1, d2.RQsq, 1, m2, var, (int)m2, (int)m1, (int)m2, (int)m2);
    VG_HIP(vg_gemm_launch(&g, st));
    VG_HIP(vg_scale_launch(var, m1 * m2, c->theta, 0, st, vg_uexp(d1.basis), vg_uexp(d2.basis)));
    return VGGP_OK;
}

__global__ void vg_kron_rows_kernel(const double* R1, const double* R2, const double* w, int m1, int m2, double* Rk,
                                    double* Rs) {
    // Rk[(a,b)][(i1,i2)] = R1[a][i1] R2[b][i2];  Rs = Rk * w[(i1,i2)]
    const long M = (long)m1 * m2;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * M) return;
    const long row = idx / M, col = idx - row * M;
    const int a = (int)(row / m2), b = (int)(row - (long)a * m2);
    const int i1 = (int)(col / m2), i2 = (int)(col - (long)i1 * m2);
    const double v = R1[a * m1 + i1] * R2[b * m2 + i2];
    Rk[idx] = v;
    Rs[idx] = v * w[col];
}

extern "C" int vggp_qv_cov(vggp_ctx* c, double* cov, void* stream) {
    VG_NOT_PAIRED(c, "vggp_qv_cov");
    if (!c || !c->have_step) { vg_set_error("vggp_qv_cov: no finished ELBO step"); return VGGP_ESTATE; }
    VG_REQUIRE(cov, "vggp_qv_cov: null output");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const long m1 = c->desc.m1, m2 = c->desc.m2, M = m1 * m2;
    VG_REQUIRE(M <= 8192, "vggp_qv_cov: M=%ld too large for a dense covariance (use vggp_qv for mean/variance)", M);
    int rc = vg_accurate_state(c, st);
    if (rc) return rc;
    if ((rc = build_RQ(c, st))) return rc;
    rc = vg_ensure_misc(c, 2 * M * M * sizeof(double));
    if (rc) return rc;
    double* Rk = (double*)c->misc;
    double* Rs = Rk + M * M;
    hipLaunchKernelGGL(vg_kron_rows_kernel, dim3((unsigned)((M * M + 255) / 256)), dim3(256), 0, st, c->d[0].RQ,
                       c->d[1].RQ, c->invD, (int)m1, (int)m2, Rk, Rs);
    VG_HIP(hipGetLastError());
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, Rs, M, 1, Rk, 1, M, cov, (int)M, (int)M, (int)M, (int)M);
    VG_HIP(vg_gemm_launch(&g, st));
    VG_HIP(vg_scale_launch(cov, M * M, c->theta, 0, st, vg_uexp(c->d[0].basis), vg_uexp(c->d[1].basis)));
    return VGGP_OK;
}

// The coefficient draw of the full-grid samplers (vggp_qv_sample, vggp_posterior_raster_sample), one block of up to nbc samples on the
// interleaved layout [m1][nbc][m2]:  Xa = (Q1^T E Q2) o D^-1/2, the eigenbasis coordinates of X_s = Sigma~^-1/2 E_s (cn live columns,
// E from eps or stream 0 at sample s0).  Two GEMMs and two elementwise kernels; Xb is scratch of the same size.  After vg_accurate_state.
int vg_sample_full_coeffs(vggp_ctx* c, const double* eps, unsigned long long seed, unsigned long long s0, int nbc, int cn, double* Xa, double* Xb,
                          hipStream_t st) {
    const long m1 = c->desc.m1, m2 = c->desc.m2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const int wide = nbc * (int)m2, tall = (int)m1 * nbc;
    VgGemmBatch g;
    VG_HIP(vg_sample_block_noise_launch(Xa, eps, seed, s0, (int)m1, nbc, (int)m2, cn, st));
    vg_gemm_init(&g);
    vg_gemm_add(&g, d1.QtPrev, m1, 1, Xa, wide, 1, Xb, wide, (int)m1, wide, (int)m1);                // Q1^T E    (rows of QtPrev = eigenvectors)
    VG_HIP(vg_gemm_launch(&g, st));
    vg_gemm_init(&g);
    vg_gemm_add(&g, Xb, m2, 1, d2.QtPrev, 1, m2, Xa, (int)m2, tall, (int)m2, (int)m2);               // (.) Q2
    VG_HIP(vg_gemm_launch(&g, st));
    VG_HIP(vg_sample_root_scale_launch(Xa, c->invD, (int)m1, nbc, (int)m2, st));                     // o D^-1/2
    return VGGP_OK;
}

// Joint samples of q(v) of the last full-grid step, without the M x M covariance.  Sigma~ = I + rho Phi is diagonal in the kept
// Kronecker eigenbasis, D = 1 + rho lam1 lam2^T, so with E_s standard normal over the cells
//     V_s = mean + sqrt(s1^e1 s2^e2) L0_1 X_s L0_2^T,   X_s = Sigma~^-1/2 E_s = Q1 ((Q1^T E_s Q2) o D^-1/2) Q2^T
// -- the SYMMETRIC root, which does not depend on the signs, order or cluster bases of the eigenvectors.  Up to 64 samples per pass
// on the interleaved block layout [m1][nbc][m2] of the iterative solvers: four GEMMs (L0_d Q_d comes from build_RQ) and two
// elementwise kernels per pass.  The route of vggp_qv_cov: vg_accurate_state, then Q_d, 1/D, L0_d; the mean is vggp_qv's.
extern "C" int vggp_qv_sample(vggp_ctx* c, int64_t n_samples, uint64_t seed, int64_t first, const double* eps_u, double* out, void* stream) {
    static const char* fn = "vggp_qv_sample";
    VG_NOT_PAIRED(c, fn);
    if (c) VG_REQUIRE(c->n_ranks == 1 && !c->comm && !c->cb, "%s: joint samples run on single-rank contexts only (this context is multi-rank)", fn);
    if (!c || !c->have_step) { vg_set_error("%s: no finished ELBO step", fn); return VGGP_ESTATE; }
    VG_REQUIRE(n_samples >= 1 && n_samples < (1LL << 31), "%s: n_samples = %lld must be at least 1", fn, (long long)n_samples);
    VG_REQUIRE(first >= 0 && out, "%s: bad argument", fn);
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const long m1 = c->desc.m1, m2 = c->desc.m2, M = m1 * m2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const int e1 = vg_uexp(d1.basis), e2 = vg_uexp(d2.basis);
    const int nbc = (int)std::min<int64_t>(64, n_samples);
    int rc = vg_accurate_state(c, st);
    if (rc) return rc;
    if ((rc = build_RQ(c, st))) return rc;
    if ((rc = vg_ensure_misc(c, (size_t)(2 * M * nbc + M) * sizeof(double)))) return rc;
    double* Xa = (double*)c->misc;
    double* Xb = Xa + M * nbc;
    double* mean = Xb + M * nbc;
    VG_HIP(vg_qv_weights_launch(c->theta, c->beta, c->invD, c->wq, M, st, e1, e2));                  // the mean: vggp_qv's two GEMMs
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, d1.RQ, m1, 1, c->wq, m2, 1, c->T3, (int)m2, (int)m1, (int)m2, (int)m1);
    VG_HIP(vg_gemm_launch(&g, st));
    vg_gemm_init(&g);
    vg_gemm_add(&g, c->T3, m2, 1, d2.RQ, 1, m2, mean, (int)m2, (int)m1, (int)m2, (int)m2);
    VG_HIP(vg_gemm_launch(&g, st));
    const int wide = nbc * (int)m2, tall = (int)m1 * nbc;
    auto gemm = [&](const double* A, long sa_m, long sa_k, const double* B, long sb_k, long sb_n, double* C, int ldc, int Mr, int Nc, int K) {
        vg_gemm_init(&g);
        vg_gemm_add(&g, A, sa_m, sa_k, B, sb_k, sb_n, C, ldc, Mr, Nc, K);
        return vg_gemm_launch(&g, st);
    };
    for (int64_t off = 0; off < n_samples; off += nbc) {
        const int cn = (int)std::min<int64_t>(nbc, n_samples - off);
        if ((rc = vg_sample_full_coeffs(c, eps_u ? eps_u + off * M : nullptr, seed, (unsigned long long)(first + off), nbc, cn, Xa, Xb, st)))
            return rc;                                                                                // (Q1^T E Q2) o D^-1/2
        VG_HIP(gemm(Xa, m2, 1, d2.RQ, 1, m2, Xb, (int)m2, tall, (int)m2, (int)m2));                  // (.) (L0_2 Q2)^T
        VG_HIP(gemm(d1.RQ, m1, 1, Xb, wide, 1, Xa, wide, (int)m1, wide, (int)m1));                   // (L0_1 Q1) (.)
        VG_HIP(vg_sample_out_launch(Xa, mean, c->theta, e1, e2, (int)m1, nbc, (int)m2, cn, out + off * M, st));
    }
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

// posterior at scattered points, processed in chunks so the workspace stays bounded
extern "C" int vggp_posterior(vggp_ctx* c, const double* xs1, const double* xs2, int64_t ns, double* mean, double* var,
                              void* stream) {
    VG_NOT_PAIRED(c, "vggp_posterior");
    if (!c || !c->have_step) { vg_set_error("vggp_posterior: no finished ELBO step"); return VGGP_ESTATE; }
    VG_REQUIRE(xs1 && xs2 && mean && var && ns >= 0, "vggp_posterior: bad argument");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const long m1 = c->desc.m1, m2 = c->desc.m2;
    // chunks of 64 Ki points: 6 launches each; 8 Ki-point chunks left the 1 M-point prediction launch-bound (15.4 ms, 13 TFLOP/s)
    const long chunk = std::min<long>(ns, 65536);
    if (ns == 0) return VGGP_OK;
    // per chunk: A(m x c), T(m x c) for both dims, T2sq, U, Uv (m1 x c); once: W_d = Q_d^T L0_d^-1 (m x m)
    const size_t per = (size_t)chunk * (2 * m1 + 3 * m2 + 2 * m1) + (size_t)(m1 * m1 + m2 * m2);
    // after a thin step: the same formulas on the range directions only (q1 x q2 instead of m1 x m2), no cold recompute
    const bool thin_ro = vg_thin_readout(c);
    int rc = thin_ro ? VGGP_OK : vg_accurate_state(c, st);
    if (rc) return rc;
    const int q1 = thin_ro ? c->d[0].thin_rows : (int)m1, q2 = thin_ro ? c->d[1].thin_rows : (int)m2;
    if ((rc = vg_ensure_misc(c, per * sizeof(double)))) return rc;
    double* p = (double*)c->misc;
    double* A1 = p; p += m1 * chunk;
    double* T1 = p; p += m1 * chunk;
    double* A2 = p; p += m2 * chunk;
    double* T2 = p; p += m2 * chunk;
    double* T2sq = p; p += m2 * chunk;
    double* U = p; p += m1 * chunk;
    double* Uv = p; p += m1 * chunk;
    double* W1 = p; p += m1 * m1;
    double* W2 = p;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    VG_HIP(vg_qv_weights_launch(c->theta, c->beta, c->invD, c->wq, (long)q1 * q2, st));   // wq = [beta rs / v | invD - 1]  (q1 x q2, compact)
    {
        VgGemmBatch g;                                                              // whitening and rotation in one operand
        vg_gemm_init(&g);
        vg_gemm_add(&g, d1.QtPrev, m1, 1, d1.Linv0, m1, 1, W1, (int)m1, q1, (int)m1, (int)m1);
        vg_gemm_add(&g, d2.QtPrev, m2, 1, d2.Linv0, m2, 1, W2, (int)m2, q2, (int)m2, (int)m2);
        VG_HIP(vg_gemm_launch(&g, st));
    }
    for (long off = 0; off < ns; off += chunk) {
        const int cn = (int)std::min<long>(chunk, ns - off);
        VgFactorJob fj[2] = {
            VgFactorJob{xs1 + off, d1.grid, A1, nullptr, nullptr, nullptr, cn, d1.m, d1.kind, d1.basis, 0, 0.0, c->desc.flags},
            VgFactorJob{xs2 + off, d2.grid, A2, nullptr, nullptr, nullptr, cn, d2.m, d2.kind, d2.basis, 1, 0.0, c->desc.flags}};
        VG_HIP(vg_factor_build_launch(fj, 2, c->theta, st));
        VgGemmBatch g;
        vg_gemm_init(&g);
        vg_gemm_add(&g, W1, m1, 1, A1, cn, 1, T1, cn, q1, cn, (int)m1);
        vg_gemm_add(&g, W2, m2, 1, A2, cn, 1, T2, cn, q2, cn, (int)m2);
        VG_HIP(vg_gemm_launch(&g, st));
        VG_HIP(vg_scale_sq_launch(T2, T2sq, (long)q2 * cn, st));
        vg_gemm_init(&g);
        vg_gemm_add(&g, c->wq, q2, 1, T2, cn, 1, U, cn, q1, cn, q2);
        vg_gemm_add(&g, c->wq + (long)q1 * q2, q2, 1, T2sq, cn, 1, Uv, cn, q1, cn, q2);
        VG_HIP(vg_gemm_launch(&g, st));
        VG_HIP(vg_post_combine_launch(c->theta, T1, U, Uv, nullptr, q1, q2, cn, mean + off, var + off, st));
    }
    return VGGP_OK;
}

// ---- dense posterior covariance at scattered points (kronecker_structure.py:223-229) ---------------------------------------
// T[(i1, i2)][p] = U1[i1][p] U2[i2][p]  (column-wise Khatri-Rao product), Tw = T * w[(i1, i2)]
__global__ void vg_khatri_rao_kernel(const double* U1, const double* U2, const double* w, int m1, int m2, long ns, double* T,
                                     double* Tw) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)m1 * m2 * ns;
    if (idx >= total) return;
    const long u = idx / ns, p = idx - u * ns;
    const int i1 = (int)(u / m2), i2 = (int)(u - (long)i1 * m2);
    const double v = U1[(long)i1 * ns + p] * U2[(long)i2 * ns + p];
    T[idx] = v;
    if (Tw) Tw[idx] = v * w[u];
}
// cov[p][q] += s1 s2 kappa1(|x1_p - x1_q| / ell1) kappa2(|x2_p - x2_q| / ell2): the prior term K** of the product kernel
__global__ void vg_prior_cov_kernel(const double* xs1, const double* xs2, long ns, int kind1, int kind2, const double* theta,
                                    double* cov) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ns * ns) return;
    const long p = idx / ns, q = idx - p * ns;
    double k1, k2, d;
    vg_kappa(kind1, fabs(xs1[p] - xs1[q]), 1.0 / theta[0], k1, d);
    vg_kappa(kind2, fabs(xs2[p] - xs2[q]), 1.0 / theta[1], k2, d);
    cov[idx] += theta[2] * theta[3] * k1 * k2;
}
hipError_t vg_prior_cov_launch(const double* xs1, const double* xs2, long ns, int kind1, int kind2, const double* theta,
                               double* cov, hipStream_t st) {
    hipLaunchKernelGGL(vg_prior_cov_kernel, dim3((unsigned)((ns * ns + 255) / 256)), dim3(256), 0, st, xs1, xs2, ns, kind1,
                       kind2, theta, cov);
    return hipGetLastError();
}

// whitened, rotated cross-covariances at x*: U_d = Q_d^T L0_d^{-1} A0_d(x*)  (m_d x ns, unit outputscale), by substitution
static int posterior_factors(vggp_ctx* c, const double* xs1, const double* xs2, int ns, double* A1, double* A2, double* U1,
                             double* U2, hipStream_t st, bool rotate) {
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    VgFactorJob fj[2] = {
        VgFactorJob{xs1, d1.grid, A1, nullptr, nullptr, nullptr, ns, d1.m, d1.kind, d1.basis, 0, 0.0, c->desc.flags},
        VgFactorJob{xs2, d2.grid, A2, nullptr, nullptr, nullptr, ns, d2.m, d2.kind, d2.basis, 1, 0.0, c->desc.flags}};
    VG_HIP(vg_factor_build_launch(fj, 2, c->theta, st));
    VgTrsmSpec q[2] = {{d1.L0, d1.m, d1.Linv0, 16L * d1.m + 16, d1.m, A1, ns, 1, ns, d1.m, 0},
                       {d2.L0, d2.m, d2.Linv0, 16L * d2.m + 16, d2.m, A2, ns, 1, ns, d2.m, 0}};
    int rc = vg_trsm_batch(q, 2, st);
    if (rc || !rotate) return rc;
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, d1.QtPrev, d1.m, 1, A1, ns, 1, U1, ns, d1.m, ns, d1.m);
    vg_gemm_add(&g, d2.QtPrev, d2.m, 1, A2, ns, 1, U2, ns, d2.m, ns, d2.m);
    VG_HIP(vg_gemm_launch(&g, st));
    return VGGP_OK;
}

extern "C" int vggp_posterior_cov(vggp_ctx* c, const double* xs1, const double* xs2, int64_t ns, double* cov, void* stream) {
    VG_NOT_PAIRED(c, "vggp_posterior_cov");
    if (!c || !c->have_step) { vg_set_error("vggp_posterior_cov: no finished ELBO step"); return VGGP_ESTATE; }
    VG_REQUIRE(xs1 && xs2 && cov && ns >= 1, "vggp_posterior_cov: bad argument");
    const long m1 = c->desc.m1, m2 = c->desc.m2, M = m1 * m2;
    VG_REQUIRE(ns <= 8192 && M * ns <= (1L << 27), "vggp_posterior_cov: ns=%ld points x M=%ld is too large for a dense covariance "
               "(use vggp_posterior for mean / variance)", (long)ns, M);
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const size_t need = (size_t)(2 * (m1 + m2) * ns + 2 * M * ns + M) * sizeof(double);
    int rc = vg_accurate_state(c, st);
    if (rc) return rc;
    if ((rc = vg_ensure_misc(c, need))) return rc;
    double* p = (double*)c->misc;
    double* A1 = p; p += m1 * ns;
    double* A2 = p; p += m2 * ns;
    double* U1 = p; p += m1 * ns;
    double* U2 = p; p += m2 * ns;
    double* T = p; p += M * ns;
    double* Tw = p; p += M * ns;
    if ((rc = posterior_factors(c, xs1, xs2, (int)ns, A1, A2, U1, U2, st, true))) return rc;
    VG_HIP(vg_qv_weights_launch(c->theta, c->beta, c->invD, c->wq, M, st));             // wq[M ..] = 1/D - 1
    hipLaunchKernelGGL(vg_khatri_rao_kernel, dim3((unsigned)((M * ns + 255) / 256)), dim3(256), 0, st, U1, U2, c->wq + M, (int)m1,
                       (int)m2, (long)ns, T, Tw);
    VG_HIP(hipGetLastError());
    // cov = s1 s2 Tw^T T  (t_p = sqrt(s1 s2) u1_p (x) u2_p for both Kuu scalings)  +  K**
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, Tw, 1, ns, T, ns, 1, cov, (int)ns, (int)ns, (int)ns, (int)M, 1, 0, 1, 0, c->h_theta[2] * c->h_theta[3], 0);
    VG_HIP(vg_gemm_launch(&g, st));
    VG_HIP(vg_prior_cov_launch(xs1, xs2, ns, c->d[0].kind, c->d[1].kind, c->theta, cov, st));
    return VGGP_OK;
}

// Gridded read-out (include/vggp.h): t_d = sqrt(s_d) Q_d^T L0_d^{-1} C_d^T; mean = T1^T (beta / v) T2;
// var = s1 s2 (kd1 kd2^T + (T1 o T1)^T W (T2 o T2)), W = D - 1 (literal) or 1/D - 1.
extern "C" int vggp_readout(vggp_ctx* c, const double* C1, int64_t mv1, const double* C2, int64_t mv2, const double* kd1,
                            const double* kd2, double* mean, double* var, int flags, void* stream) {
    VG_NOT_PAIRED(c, "vggp_readout");
    if (!c || !c->have_step) { vg_set_error("vggp_readout: no finished ELBO step"); return VGGP_ESTATE; }
    VG_REQUIRE(C1 && C2 && kd1 && kd2 && mean && var && mv1 >= 1 && mv2 >= 1, "vggp_readout: bad argument");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const long m1 = c->desc.m1, m2 = c->desc.m2;
    const size_t need = (size_t)(3 * (m1 * mv1 + m2 * mv2) + 2 * m1 * mv2) * sizeof(double);
    int rc = vg_accurate_state(c, st);
    if (rc) return rc;
    if ((rc = vg_ensure_misc(c, need))) return rc;
    double* p = (double*)c->misc;
    double* X1 = p; p += m1 * mv1;
    double* T1 = p; p += m1 * mv1;
    double* S1 = p; p += m1 * mv1;
    double* X2 = p; p += m2 * mv2;
    double* T2 = p; p += m2 * mv2;
    double* S2 = p; p += m2 * mv2;
    double* U = p; p += m1 * mv2;
    double* Uv = p;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    VG_HIP(vg_readout_weights_launch(c->theta, c->beta, c->invD, c->wq, m1 * m2, (flags & VGGP_READOUT_LITERAL) ? 1 : 0, st));
    if ((rc = vg_whitened_cross(c, C1, mv1, C2, mv2, X1, X2, st))) return rc;      // X_d = Linv0_d C_d^T   (m_d x mv_d)
    VgGemmBatch g;
    vg_gemm_init(&g);                                    // T_d = Q_d^T X_d  (rows of QtPrev are the eigenvectors)
    vg_gemm_add(&g, d1.QtPrev, m1, 1, X1, mv1, 1, T1, (int)mv1, (int)m1, (int)mv1, (int)m1);
    vg_gemm_add(&g, d2.QtPrev, m2, 1, X2, mv2, 1, T2, (int)mv2, (int)m2, (int)mv2, (int)m2);
    VG_HIP(vg_gemm_launch(&g, st));
    VG_HIP(vg_scale_sq_launch(T1, S1, m1 * mv1, st));
    VG_HIP(vg_scale_sq_launch(T2, S2, m2 * mv2, st));
    vg_gemm_init(&g);                                    // U = Wm T2, Uv = Wv (T2 o T2)   (m1 x mv2)
    vg_gemm_add(&g, c->wq, m2, 1, T2, mv2, 1, U, (int)mv2, (int)m1, (int)mv2, (int)m2);
    vg_gemm_add(&g, c->wq + m1 * m2, m2, 1, S2, mv2, 1, Uv, (int)mv2, (int)m1, (int)mv2, (int)m2);
    VG_HIP(vg_gemm_launch(&g, st));
    vg_gemm_init(&g);                                    // mean = T1^T U, var' = (T1 o T1)^T Uv   (mv1 x mv2)
    vg_gemm_add(&g, T1, 1, mv1, U, mv2, 1, mean, (int)mv2, (int)mv1, (int)mv2, (int)m1);
    vg_gemm_add(&g, S1, 1, mv1, Uv, mv2, 1, var, (int)mv2, (int)mv1, (int)mv2, (int)m1);
    VG_HIP(vg_gemm_launch(&g, st));
    VG_HIP(vg_readout_var_launch(c->theta, kd1, kd2, mv1, mv2, var, st));
    return VGGP_OK;
}

// ---------------------------------------------------------------------------------
// exported building blocks
extern "C" int vggp_factor_build(vggp_ctx* c, int kind, int basis, const double* x, int64_t n, const double* grid,
                                 int64_t m, double ell, int flags, double* A0, double* dA0, double* K0, double* dK0, void* stream) {
    if (!c) { vg_set_error("null context"); return VGGP_EINVAL; }
    VG_REQUIRE(kind >= 0 && kind <= 3 && basis >= 0 && basis <= 5, "vggp_factor_build: bad kind/basis");
    VG_REQUIRE(!((basis == VGGP_BASIS_VFF || basis == VGGP_BASIS_B1) && kind != VGGP_KIND_MATERN12),
               "vggp_factor_build: VFF / B1 are Matern-1/2 only");
    VG_REQUIRE(!(basis == VGGP_BASIS_B0 && kind != VGGP_KIND_MATERN12), "vggp_factor_build: B0 is Matern-1/2 only");
    VG_REQUIRE(!(basis == VGGP_BASIS_B0K && (kind == VGGP_KIND_RBF || (flags & VGGP_FLAG_B0_F32_KDELTA))),
               "vggp_factor_build: B0K takes Matern-1/2, -3/2, -5/2 and no VGGP_FLAG_B0_F32_KDELTA");
    VG_REQUIRE(n >= 0 && m >= 1 && ell > 0.0, "vggp_factor_build: bad sizes / lengthscale");
    VG_REQUIRE(grid || basis == VGGP_BASIS_ONE, "vggp_factor_build: null grid");
    VG_REQUIRE((x || !(A0 || dA0)), "vggp_factor_build: null x");
    VG_ENTER_DEVICE(c->device);
    VgFactorJob j{x, grid, n > 0 ? A0 : nullptr, n > 0 ? dA0 : nullptr, K0, dK0, (int)n, (int)m, kind, basis, -1, ell, flags};
    VG_HIP(vg_factor_build_launch(&j, 1, nullptr, stream ? (hipStream_t)stream : c->own_stream));
    return VGGP_OK;
}

// adds jit to the diagonal of the m x m copy W of K (one launch per jitter attempt of the blocked path)
__global__ void vg_copy_jitter_kernel(const double* K, double* W, long m, double jit) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * m) return;
    W[idx] = K[idx] + ((idx / m == idx % m) ? jit : 0.0);
}

extern "C" int vggp_cholesky_inverse(vggp_ctx* c, const double* K, int64_t m, double* L, double* Linv, double* jitter_out,
                                     void* stream) {
    if (!c) { vg_set_error("null context"); return VGGP_EINVAL; }
    VG_REQUIRE(K && L && Linv && m >= 1 && m <= 8192, "vggp_cholesky_inverse: bad argument (1 <= m <= 8192)");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    if (m > 128) {
        // beyond one workgroup: blocked factorisation (128-wide panels by the single-workgroup kernel, the rest by MFMA
        // GEMMs); the jitter schedule is walked on the host, one attempt per level
        const size_t nblk = (size_t)(m + VG_DENSE_MB - 1) / VG_DENSE_MB;
        const size_t need = ((size_t)m * m + nblk * VG_DENSE_MB * VG_DENSE_MB + (size_t)VG_DENSE_MB * m + VG_DENSE_MB * (VG_DENSE_MB + 1) + 64) * sizeof(double);
        int rc = vg_ensure_misc(c, need);
        if (rc) return rc;
        double* p = (double*)c->misc;
        VgDenseChol w{};
        w.S = p; p += (size_t)m * m;
        w.DI = p; p += nblk * VG_DENSE_MB * VG_DENSE_MB;
        w.Tmp = p; p += (size_t)VG_DENSE_MB * m;
        w.scratch = p; p += VG_DENSE_MB * (VG_DENSE_MB + 1);
        w.jit = p; p += 8;
        w.status = reinterpret_cast<int*>(p);
        w.L = L; w.X = Linv; w.M = m; w.Sinv = nullptr;
        static const double levels[4] = {0.0, 1e-8, 1e-7, 1e-6};
        for (int lvl = 0; lvl < 4; ++lvl) {
            VG_HIP(hipMemsetAsync(w.status, 0, 2 * sizeof(int), st));
            hipLaunchKernelGGL(vg_copy_jitter_kernel, dim3((unsigned)(((size_t)m * m + 255) / 256)), dim3(256), 0, st, K, w.S, (long)m, levels[lvl]);
            VG_HIP(hipGetLastError());
            if ((rc = vg_blocked_chol_inverse(w, st))) return rc;
            int hs = 0;
            VG_HIP(hipMemcpyAsync(&hs, w.status, sizeof(int), hipMemcpyDeviceToHost, st));
            VG_HIP(hipStreamSynchronize(st));
            if (!hs) { if (jitter_out) *jitter_out = levels[lvl]; return VGGP_OK; }
        }
        if (jitter_out) *jitter_out = -1.0;
        vg_set_error("vggp_cholesky_inverse: not positive definite after jitter 1e-6");
        return VGGP_ENOTPD;
    }
    int rc = vg_ensure_misc(c, (size_t)(m * (m + 1) + 16) * sizeof(double));
    if (rc) return rc;
    double* scratch = (double*)c->misc;
    double* jit = scratch + m * (m + 1);
    int* status = (int*)(jit + 2);
    VgClearArgs clr;
    clr.n = 2;
    clr.ptr[0] = reinterpret_cast<int*>(jit); clr.nwords[0] = 16;
    clr.ptr[1] = reinterpret_cast<int*>(scratch); clr.nwords[1] = 16;
    VG_HIP(vg_clear_launch(&clr, st));
    VgCholJob j{K, L, Linv, scratch, jit, status, (int)m};
    VG_HIP(vg_chol_launch(&j, 1, st));
    double hj = 0.0;
    int hs = 0;
    VG_HIP(hipMemcpyAsync(&hj, jit, sizeof(double), hipMemcpyDeviceToHost, st));
    VG_HIP(hipMemcpyAsync(&hs, status, sizeof(int), hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    if (jitter_out) *jitter_out = hj;
    if (hs) { vg_set_error("vggp_cholesky_inverse: not positive definite after jitter 1e-6"); return VGGP_ENOTPD; }
    return VGGP_OK;
}

extern "C" int vggp_eigh(vggp_ctx* c, const double* G, int64_t m, double* lam, double* Qt, int32_t* sweeps_out, int flags,
                         void* stream) {
    if (!c) { vg_set_error("null context"); return VGGP_EINVAL; }
    VG_REQUIRE(G && lam && Qt && m >= 1 && m <= 256, "vggp_eigh: bad argument (1 <= m <= 256)");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const long m2e = m + (m & 1);
    const int max_rounds = (int)(VG_EIG_MAXSWEEP * (m2e - 1));
    const size_t logb = (vg_eigh_log_bytes((int)m) + 15) & ~size_t(15);
    const size_t need = (size_t)m2e * (m2e + 1) * 8 + logb + (size_t)max_rounds * 4 + 256 + (size_t)m2e * 4 + 64;
    int rc = vg_ensure_misc(c, need);
    if (rc) return rc;
    char* p = (char*)c->misc;
    double* gwork = (double*)p; p += (size_t)m2e * (m2e + 1) * 8;
    double2* rotlog = (double2*)p; p += logb;
    int* roundlog = (int*)p; p += (size_t)max_rounds * 4;
    p = (char*)(((uintptr_t)p + 63) & ~uintptr_t(63));
    int* counters = (int*)p;
    int* perm = counters + 16;
    VgClearArgs clr;
    clr.n = 1;
    clr.ptr[0] = counters; clr.nwords[0] = 8;
    VG_HIP(vg_clear_launch(&clr, st));
    VgEigJob j{G, lam, Qt, nullptr, gwork, rotlog, roundlog, counters, (int)m, max_rounds, (long)logb,
               (flags & VGGP_FLAG_BLOCK_JACOBI) ? 1 : 0};
    j.perm = perm;
    j.err = counters + 4;
    VG_HIP(vg_eigh_launch(&j, 1, st));
    int hc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    VG_HIP(hipMemcpyAsync(hc, counters, sizeof(hc), hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    if (sweeps_out) *sweeps_out = hc[1] & 0xff;
    if (hc[2] || hc[4]) { vg_set_error("vggp_eigh: no convergence"); return VGGP_ENOCONV; }
    return VGGP_OK;
}

// ---- the thin chain's kernels, one job each (exported for tests: tests/test_gpu_thin_chain_paths.py) ---------------------------------
extern "C" int vggp_pivchol(vggp_ctx* c, const double* G, const double* Omega, int64_t m, int64_t r, double* V, void* stream) {
    if (!c) { vg_set_error("null context"); return VGGP_EINVAL; }
    VG_REQUIRE(G && Omega && V, "vggp_pivchol: null argument");
    VG_REQUIRE(m >= 1 && m <= 256 && r >= 1 && r <= m && r <= 64, "vggp_pivchol: need 1 <= r <= min(m, 64), m <= 256");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const VgPivCholJob j{G, Omega, V, (int)m, (int)r};
    VG_HIP(vg_pivchol_launch(&j, 1, st));
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

extern "C" int vggp_rowqr(vggp_ctx* c, const double* Z, int64_t r, int64_t m, double* V1, const double* cp_src, double* cp_dst, int64_t cp_n,
                          void* stream) {
    if (!c) { vg_set_error("null context"); return VGGP_EINVAL; }
    VG_REQUIRE(Z && V1, "vggp_rowqr: null argument");
    VG_REQUIRE(r >= 1 && r <= 64 && m >= r && m <= 256, "vggp_rowqr: need 1 <= r <= min(m, 64), m <= 256");
    VG_REQUIRE(cp_n >= 0 && cp_n < (1L << 31) && (cp_n == 0 || (cp_src && cp_dst)), "vggp_rowqr: bad pass-through copy");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const VgRowQrJob j{Z, V1, (int)r, (int)m, cp_src, cp_dst, (long)cp_n};
    VG_HIP(vg_rowqr_launch(&j, 1, st));
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

extern "C" int vggp_ritz(vggp_ctx* c, const double* Hl, const double* Hr, int64_t r, int64_t hk, double* lam, double* W, int32_t* counters_out,
                         int32_t* err_out, void* stream) {
    if (!c) { vg_set_error("null context"); return VGGP_EINVAL; }
    VG_REQUIRE(Hl && Hr && lam && W, "vggp_ritz: null argument");
    VG_REQUIRE(r >= 1 && r <= 64 && hk >= r && hk <= 256, "vggp_ritz: need 1 <= r <= 64, r <= hk <= 256");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const long m2e = r + (r & 1);                                    // (scratch as vggp_eigh lays it out)
    const int max_rounds = (int)(VG_EIG_MAXSWEEP * (m2e - 1));
    const size_t logb = (vg_eigh_log_bytes((int)r) + 15) & ~size_t(15);
    const size_t need = (size_t)m2e * (m2e + 1) * 8 + logb + (size_t)max_rounds * 4 + 256 + (size_t)m2e * 4 + 64;
    int rc = vg_ensure_misc(c, need);
    if (rc) return rc;
    char* p = (char*)c->misc;
    double* gwork = (double*)p; p += (size_t)m2e * (m2e + 1) * 8;
    double2* rotlog = (double2*)p; p += logb;
    int* roundlog = (int*)p; p += (size_t)max_rounds * 4;
    p = (char*)(((uintptr_t)p + 63) & ~uintptr_t(63));
    int* counters = (int*)p;
    int* perm = counters + 16;
    VgClearArgs clr;
    clr.n = 1;
    clr.ptr[0] = counters; clr.nwords[0] = 8;
    VG_HIP(vg_clear_launch(&clr, st));
    const VgEigJob j = vg_make_ritz_job(Hl, Hr, (int)r, (int)hk, lam, W, gwork, rotlog, roundlog, counters, max_rounds, (long)logb, perm,
                                        counters + 4);
    VG_HIP(vg_eigh_launch(&j, 1, st));
    int hc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    VG_HIP(hipMemcpyAsync(hc, counters, sizeof(hc), hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    if (counters_out) for (int q = 0; q < 4; ++q) counters_out[q] = hc[q];
    if (err_out) *err_out = hc[4];
    if (hc[2] || hc[4]) { vg_set_error("vggp_ritz: no convergence"); return VGGP_ENOCONV; }
    return VGGP_OK;
}

extern "C" int vggp_thin_tail(vggp_ctx* c, const vggp_thin_tail_args* a, void* stream) {
    if (!c) { vg_set_error("null context"); return VGGP_EINVAL; }
    VG_REQUIRE(a, "vggp_thin_tail: null argument block");
    VG_REQUIRE(a->theta && a->W1 && a->W2 && a->lam1 && a->lam2 && a->AM1 && a->AH1 && a->AM2 && a->AH2 && a->AC && a->G1 && a->H1 && a->G2 &&
               a->H2, "vggp_thin_tail: null input");
    VG_REQUIRE(!a->beta_out == !a->invd_out, "vggp_thin_tail: beta_out and invd_out go together");
    VG_REQUIRE(a->r1 >= 1 && a->r2 >= 1 && a->r1 <= VG_THIN_MAXR && a->r2 <= VG_THIN_MAXR && a->r1 <= a->m1 && a->r2 <= a->m2 && a->m1 <= 256 &&
               a->m2 <= 256, "vggp_thin_tail: need 1 <= r_d <= min(m_d, 32), m_d <= 256");
    VG_REQUIRE(a->ac_nslab >= 1 && a->ac_nslab <= 64 && (a->ac_nslab == 1 || a->ac_slab >= 3L * a->r1 * a->r2),
               "vggp_thin_tail: need 1 <= ac_nslab <= 64 and slabs that do not overlap");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    static_assert(sizeof(VgHostOut) == 16 * sizeof(double), "vggp_thin_tail_args::hout is 16 doubles");
    static_assert(sizeof(vggp_thin_tail_args) == 248, "vggp_thin_tail_args layout (_lib.py ThinTailArgs)");
    VgThinTail tt{};
    tt.theta = a->theta; tt.n_total = a->n_total; tt.yy = a->yy;
    tt.r1 = a->r1; tt.r2 = a->r2; tt.m1 = a->m1; tt.m2 = a->m2;
    tt.W1 = a->W1; tt.W2 = a->W2; tt.lam1 = a->lam1; tt.lam2 = a->lam2;
    tt.AM1 = a->AM1; tt.AH1 = a->AH1; tt.AM2 = a->AM2; tt.AH2 = a->AH2; tt.AC = a->AC;
    tt.ac_nslab = a->ac_nslab; tt.ac_slab = (long)a->ac_slab;
    tt.G1 = a->G1; tt.H1 = a->H1; tt.G2 = a->G2; tt.H2 = a->H2;
    tt.out = a->out; tt.beta_out = a->beta_out; tt.invd_out = a->invd_out;
    tt.hout = reinterpret_cast<VgHostOut*>(a->hout);
    tt.peer_fail = a->peer_fail;
    for (int k = 0; k < 2; ++k) { tt.jit[k] = a->jit[k]; tt.status[k] = a->status[k]; tt.rcounters[k] = a->rcounters[k]; }
    VG_HIP(vg_thin_tail_launch(&tt, st));
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

extern "C" int vggp_gemm(vggp_ctx* c, const double* A, int64_t sa_m, int64_t sa_k, const double* B, int64_t sb_k,
                         int64_t sb_n, double* C, int64_t ldc, int64_t M, int64_t N, int64_t K, void* stream) {
    if (!c) { vg_set_error("null context"); return VGGP_EINVAL; }
    VG_REQUIRE(A && B && C && M >= 1 && N >= 1 && K >= 1 && ldc >= N, "vggp_gemm: bad argument");
    VG_REQUIRE(M < (1L << 30) && N < (1L << 30) && K < (1L << 30), "vggp_gemm: dimension too large");
    VG_ENTER_DEVICE(c->device);
    VgGemmBatch g;
    vg_gemm_init(&g);
    vg_gemm_add(&g, A, sa_m, sa_k, B, sb_k, sb_n, C, (int)ldc, (int)M, (int)N, (int)K);
    VG_HIP(vg_gemm_launch(&g, stream ? (hipStream_t)stream : c->own_stream));
    return VGGP_OK;
}

extern "C" int vggp_trsm(vggp_ctx* c, const double* L, int64_t m, const double* R, int64_t ncols, double* X, int trans,
                         void* stream) {
    if (!c) { vg_set_error("null context"); return VGGP_EINVAL; }
    VG_REQUIRE(L && R && X && m >= 1 && m <= 16384 && ncols >= 1, "vggp_trsm: bad argument (1 <= m <= 16384)");
    VG_REQUIRE(m * ncols < (1L << 31) && m * m < (1L << 31), "vggp_trsm: matrix too large");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const long nb16 = (m + 15) / 16;
    int rc = vg_ensure_misc(c, (size_t)nb16 * 256 * sizeof(double));
    if (rc) return rc;
    double* Dinv = (double*)c->misc;
    VG_HIP(vg_tri_diaginv_launch(L, m, (int)m, Dinv, st));
    if (X != R) VG_HIP(hipMemcpyAsync(X, R, sizeof(double) * m * ncols, hipMemcpyDeviceToDevice, st));
    return trsm_inplace(L, m, m, Dinv, X, ncols, 1, ncols, trans ? 1 : 0, st);
}

// Explicit inverse of a lower-triangular factor (n > 128) without ever inverting more than a 16 x 16 block directly:
// the 128 x 128 diagonal blocks by substitution on the identity (strip kernel, one launch for all blocks of all factors),
// then block doubling  inv([A 0; B C]) = [A^-1 0; -C^-1 B A^-1, C^-1]  with two MFMA GEMM launches per level
// (128 -> 256 -> 512 -> ...; every pair of every factor in the same launch).  The 128-blocks of Xinv above the diagonal are
// neither written nor read (triangular-aware products): consumers must skip them as well.
struct VgTriInvSpec { const double* L; long n; const double* Dinv16; double* Xinv; double* tmp; };
static int tri_inverse_batch(const VgTriInvSpec* sp, int nf, hipStream_t st) {
    VgTrsmJob tj[16];
    int nt = 0;
    for (int f = 0; f < nf; ++f)
        for (long r0 = 0; r0 < sp[f].n; r0 += VG_TRSM_BLK) {
            const long rb = std::min<long>(VG_TRSM_BLK, sp[f].n - r0);
            if (nt == 16) { VG_HIP(vg_trsm_launch(tj, nt, st)); nt = 0; }
            VgTrsmJob j{sp[f].L + r0 * sp[f].n + r0, sp[f].Dinv16 + (r0 / 16) * 256, nullptr, sp[f].Xinv + r0 * sp[f].n + r0, sp[f].n, 256, 16,
                        sp[f].n, 1, sp[f].n, 1, rb, (int)rb, 0};
            j.rhs_ident = 1;
            tj[nt++] = j;
        }
    if (nt) VG_HIP(vg_trsm_launch(tj, nt, st));
    long nmax = 0;
    for (int f = 0; f < nf; ++f) nmax = std::max(nmax, sp[f].n);
    for (long b = VG_TRSM_BLK; b < nmax; b *= 2) {
        for (int pass = 0; pass < 2; ++pass) {
            VgGemmBatch g;
            vg_gemm_init(&g);
            for (int f = 0; f < nf; ++f) {
                const long n = sp[f].n;
                for (long a0 = 0; a0 + b < n; a0 += 2 * b) {
                    const long c0 = a0 + b, cb = std::min<long>(b, n - c0);           // A = [a0, a0+b), C = [c0, c0+cb)
                    if (g.nprob == VG_GEMM_MAXP) { VG_HIP(vg_gemm_launch(&g, st)); vg_gemm_init(&g); }
                    int ip;
                    if (pass == 0) {      // T = B A^-1        (cb x b; A^-1 lower triangular: its upper 128-blocks are never read)
                        ip = vg_gemm_add(&g, sp[f].L + c0 * n + a0, n, 1, sp[f].Xinv + a0 * n + a0, n, 1, sp[f].tmp + c0 * n + a0, (int)n, (int)cb,
                                         (int)b, (int)b);
                        g.p[ip].tri = VG_TRI_B_LOWER;
                    } else {              // W = -C^-1 T
                        ip = vg_gemm_add(&g, sp[f].Xinv + c0 * n + c0, n, 1, sp[f].tmp + c0 * n + a0, n, 1, sp[f].Xinv + c0 * n + a0, (int)n,
                                         (int)cb, (int)b, (int)cb, 1, 0, 1, 0, -1.0, 0);
                        g.p[ip].tri = VG_TRI_A_LOWER;
                    }
                }
            }
            if (g.nprob) VG_HIP(vg_gemm_launch(&g, st));
        }
    }
    return VGGP_OK;
}

extern "C" int vggp_kron_solve(vggp_ctx* c, const double* L1, int64_t n1, const double* L2, int64_t n2, const double* Y,
                               double* X, void* stream) {
    if (!c) { vg_set_error("null context"); return VGGP_EINVAL; }
    VG_REQUIRE(L1 && L2 && Y && X && n1 >= 1 && n2 >= 1 && n1 <= 16384 && n2 <= 16384, "vggp_kron_solve: bad argument");
    VG_REQUIRE(n1 * n2 < (1L << 31) && n1 * n1 < (1L << 31) && n2 * n2 < (1L << 31), "vggp_kron_solve: matrix too large");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const long nb1 = (n1 + 15) / 16, nb2 = (n2 + 15) / 16;
    static const bool subst_only = getenv("VGGP_KRON_SUBST") != nullptr;
    const bool small = (n1 <= VG_TRSM_BLK && n2 <= VG_TRSM_BLK) || subst_only;
    const size_t need = (size_t)(nb1 + nb2) * 256 + (small ? 0 : (size_t)(2 * (n1 * n1 + n2 * n2) + 4 * n1 * n2));
    int rc = vg_ensure_misc(c, need * sizeof(double));
    if (rc) return rc;
    double* D1 = (double*)c->misc;
    double* D2 = D1 + nb1 * 256;
    VG_HIP(vg_tri_diaginv_launch(L1, n1, (int)n1, D1, st, L2, n2, (int)n2, D2));
    if (small) {
        // X = L1^{-T} ( L1^{-1} Y L2^{-T} ) L2^{-1}: four solves by substitution, in place on X ([n1][n2] row-major);
        // left solves see X as it is (row k = row of X), right solves see its transpose (row k = column k of X)
        if (X != Y) VG_HIP(hipMemcpyAsync(X, Y, sizeof(double) * n1 * n2, hipMemcpyDeviceToDevice, st));
        if ((rc = trsm_inplace(L1, n1, n1, D1, X, n2, 1, n2, 0, st))) return rc;        // L1 T = Y
        if ((rc = trsm_inplace(L2, n2, n2, D2, X, 1, n2, n1, 0, st))) return rc;        // L2 T'^T = T^T      (T' = T L2^{-T})
        if ((rc = trsm_inplace(L1, n1, n1, D1, X, n2, 1, n2, 1, st))) return rc;        // L1^T T'' = T'
        if ((rc = trsm_inplace(L2, n2, n2, D2, X, 1, n2, n1, 1, st))) return rc;        // L2^T X^T = T''^T   (X = T'' L2^{-1})
        return VGGP_OK;
    }
    // Larger factors: a substitution sweep over n / 128 block rows is a chain of 2 n / 128 dependent launches per solve (8 of
    // them: 1.3 ms at n = 1024, measured), so the factors are inverted -- 128 x 128 diagonal blocks by substitution, the
    // rest by block doubling (tri_inverse_batch) -- and applied as four triangular-aware MFMA GEMMs.  Everything is inside
    // this call (BASELINE metric ii is timed from the Cholesky factors).
    double* Li1 = D2 + nb2 * 256;
    double* Li2 = Li1 + n1 * n1;
    double* tmp1 = Li2 + n2 * n2;
    double* tmp2 = tmp1 + n1 * n1;
    double* T1 = tmp2 + n2 * n2;                 // two split-K slabs each
    double* T2 = T1 + 2 * n1 * n2;
    // (no clearing of Li: the substitution writes whole diagonal 128-blocks, and every product below skips the 128-blocks above them)
    VgTriInvSpec sp[2] = {{L1, (long)n1, D1, Li1, tmp1}, {L2, (long)n2, D2, Li2, tmp2}};
    if ((rc = tri_inverse_batch(sp, 2, st))) return rc;            // both factors ride in the same launches
    // X = P1 Y P2 with P_d = K_d^-1 = Linv_d^T Linv_d: one launch forms both P_d (X^T X of a lower-triangular X: tiles skip the
    // k-range where either operand vanishes), then TWO dense products instead of four triangular-aware ones -- a 1024^3 product is
    // 256 tiles = one workgroup per CU, and the triangular skip leaves the longest tile (full K) on the critical path, so each of
    // the four cost what a dense product costs (40 us at n = 1024).  The error is that of the explicit inverses either way
    // (eps cond(K_d) per side).  VGGP_KRON_FOUR=1 keeps the four-product form reachable (A/B).
    static const bool four = getenv("VGGP_KRON_FOUR") != nullptr;
    VgGemmBatch g;
    if (!four) {
        double* P1 = tmp1;                       // (the block-doubling scratch is free again)
        double* P2 = tmp2;
        vg_gemm_init(&g);
        { const int i = vg_gemm_add(&g, Li1, 1, n1, Li1, n1, 1, P1, (int)n1, (int)n1, (int)n1, (int)n1); g.p[i].tri = VG_TRI_A_UPPER_B_LOWER; }
        { const int i = vg_gemm_add(&g, Li2, 1, n2, Li2, n2, 1, P2, (int)n2, (int)n2, (int)n2, (int)n2); g.p[i].tri = VG_TRI_A_UPPER_B_LOWER; g.p[i].rev = 1; }
        VG_HIP(vg_gemm_launch(&g, st, VG_GEMM_TAG_WIDE));
        vg_gemm_init(&g);
        vg_gemm_add(&g, P1, n1, 1, Y, n2, 1, T1, (int)n2, (int)n1, (int)n2, (int)n1);           // P1 Y
        VG_HIP(vg_gemm_launch(&g, st, VG_GEMM_TAG_WIDE));
        vg_gemm_init(&g);
        vg_gemm_add(&g, T1, n2, 1, P2, n2, 1, X, (int)n2, (int)n1, (int)n2, (int)n2);           // . P2   (symmetric)
        VG_HIP(vg_gemm_launch(&g, st, VG_GEMM_TAG_WIDE));
        return VGGP_OK;
    }
    // Four triangular-aware GEMMs.  Splitting the reduction in two
    // (slabs summed on load by the next product, two workgroups per CU) was measured SLOWER (397 vs 336 us for the whole
    // solve: the slab-summing operand path); VGGP_KRON_KSPLIT=2 keeps it reachable.
    const long slab = (long)n1 * n2;
    static const char* kse = getenv("VGGP_KRON_KSPLIT");
    const int ks = kse ? atoi(kse) : 1;
    vg_gemm_init(&g);
    { const int i = vg_gemm_add(&g, Li1, n1, 1, Y, n2, 1, T1, (int)n2, (int)n1, (int)n2, (int)n1, ks, slab); g.p[i].tri = VG_TRI_A_LOWER; }  // L1inv Y
    const int s1 = g.p[0].ksplit;
    VG_HIP(vg_gemm_launch(&g, st, VG_GEMM_TAG_WIDE));
    vg_gemm_init(&g);
    { const int i = vg_gemm_add(&g, T1, n2, 1, Li2, 1, n2, T2, (int)n2, (int)n1, (int)n2, (int)n2, ks, slab); g.p[i].tri = VG_TRI_B_UPPER;  // . L2inv^T
      g.p[i].a_nslab = s1; g.p[i].a_slab = slab; }
    const int s2 = g.p[0].ksplit;
    VG_HIP(vg_gemm_launch(&g, st, VG_GEMM_TAG_WIDE));
    vg_gemm_init(&g);
    { const int i = vg_gemm_add(&g, Li1, 1, n1, T2, n2, 1, T1, (int)n2, (int)n1, (int)n2, (int)n1, ks, slab, s2, slab); g.p[i].tri = VG_TRI_A_UPPER; }  // L1inv^T .
    const int s3 = g.p[0].ksplit;
    VG_HIP(vg_gemm_launch(&g, st, VG_GEMM_TAG_WIDE));
    vg_gemm_init(&g);
    { const int i = vg_gemm_add(&g, T1, n2, 1, Li2, n2, 1, X, (int)n2, (int)n1, (int)n2, (int)n2); g.p[i].tri = VG_TRI_B_LOWER;            // . L2inv
      g.p[i].a_nslab = s3; g.p[i].a_slab = slab; }
    VG_HIP(vg_gemm_launch(&g, st, VG_GEMM_TAG_WIDE));
    return VGGP_OK;
}

// ---------------------------------------------------------------------------------
// Gradient of the ELBO with respect to the inducing-point coordinates (SVGP's trainable Z: kronecker_structure.py:303-304
// registers Z as a Parameter and autograd differentiates through kernel(Z), kernel(Z, x)).  Spec: oracle/kron.py z_grad.
// The analytic lengthscale gradient is linear in the perturbation (dK, dA) it is fed, dELBO = <W_M, L^-1 dK L^-T> + <W_V, L^-1 dA>,
// so Kbar = L^-T W_M L^-1 and Abar = L^-T W_V are the sensitivities, and for a stationary kernel
// d kappa(z_i, x) / d z_i = -(d kappa / d ell) ell / (z_i - x): the derivative factors dA0, dK0 of the step are reused.
// Uses the resident state of the last vggp_elbo_step on the same Y (warm-basis accuracy, like the lengthscale gradient); one
// extra pass over Y (B1 Y^T), ~25 small launches.
extern "C" int vggp_zgrad(vggp_ctx* c, const double* Y, double* gz1, double* gz2, void* stream) {
    VG_FORWARD_PAIRED(c, vg_paired_zgrad(c, Y, gz1, gz2, stream ? (hipStream_t)stream : c->own_stream, false));
    if (!c || !c->have_step) { vg_set_error("vggp_zgrad: no finished ELBO step"); return VGGP_ESTATE; }
    VG_REQUIRE(Y && gz1 && gz2, "vggp_zgrad: null argument");
    // Row-sharded job: every term of g is a sum over observations, so each rank forms the part of ITS rows -- the columns of dimension
    // 2 it owns, and for dimension 1 (whose n1 columns every rank holds) the projection term through its rows of Y -- while the terms
    // that only involve replicated state (Kbar, and s1 W_H B1 of dimension 1) are added by rank 0 alone; ONE all-reduce of m1 + m2 doubles.
    const bool multi = c->n_ranks > 1 || c->comm || c->cb;
    const bool lead = !multi || c->rank == 0;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    if (c->last_thin) {
        // the inducing-point gradient contracts the FULL m-space state (beta, 1/D, Q): a thin step leaves none.  Rebuild it from
        // the resident G, H, C (cold finish half) and keep this plan on the full chain from now on -- its caller trains Z.
        c->thin_off = true;
        const int rca = vg_accurate_state(c, st);
        if (rca) return rca;
    }
    const long n1 = c->desc.n1, n2 = c->desc.n2, m1 = c->desc.m1, m2 = c->desc.m2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const bool pts[2] = {d1.basis == VGGP_BASIS_POINTS, d2.basis == VGGP_BASIS_POINTS};
    if (!pts[0]) VG_HIP(hipMemsetAsync(gz1, 0, sizeof(double) * m1, st));
    if (!pts[1]) VG_HIP(hipMemsetAsync(gz2, 0, sizeof(double) * m2, st));
    if (!pts[0] && !pts[1]) return VGGP_OK;
    const double s1 = c->h_theta[2], s2 = c->h_theta[3], v = c->h_theta[4];
    // workspace
    const long mm1 = m1 * m1, mm2 = m2 * m2, m12 = m1 * m2;
    const size_t need = sizeof(double) * (size_t)(6 * mm1 + 6 * mm2 + 2 * m12 + m1 * n1 + m2 * n2 + m1 * n2 + m1 + m2);
    int rc = vg_ensure_misc(c, need);
    if (rc) return rc;
    double* w = reinterpret_cast<double*>(c->misc);
    double *Xa[2], *Xl[2], *WE[2], *WF[2], *TA[2], *TB[2];
    for (int k = 0; k < 2; ++k) {
        const long mm = k ? mm2 : mm1;
        Xa[k] = w; w += mm; Xl[k] = w; w += mm; WE[k] = w; w += mm; WF[k] = w; w += mm; TA[k] = w; w += mm; TB[k] = w; w += mm;
    }
    double* U = w; w += m12;
    double* T1 = w; w += m12;
    double* WV[2] = {w, w + m1 * n1}; w += m1 * n1 + m2 * n2;
    double* R1 = w; w += m1 * n2;
    double* gzbuf = w;                                   // [m1 + m2]: the all-reduce buffer of a row-sharded job
    VgGemmBatch g;
    // 1. the four beta Gram matrices
    vg_gemm_init(&g);
    vg_gemm_add(&g, c->beta, m2, 1, c->beta, 1, m2, Xa[0], (int)m1, (int)m1, (int)m1, (int)m2);    // beta beta^T
    vg_gemm_add(&g, c->bl2, m2, 1, c->beta, 1, m2, Xl[0], (int)m1, (int)m1, (int)m1, (int)m2);     // (beta lam2) beta^T
    vg_gemm_add(&g, c->beta, 1, m2, c->beta, m2, 1, Xa[1], (int)m2, (int)m2, (int)m2, (int)m1);    // beta^T beta
    vg_gemm_add(&g, c->bl1, 1, m2, c->beta, m2, 1, Xl[1], (int)m2, (int)m2, (int)m2, (int)m1);     // (lam1 beta)^T beta
    // ... and R1 = B1 Y^T (m1 x n2): the projection the step itself does not form
    if (pts[1]) vg_gemm_add(&g, d1.BV, n1, 1, Y, 1, n1, R1, (int)n2, (int)m1, (int)n2, (int)n1);
    VG_HIP(vg_gemm_launch(&g, st));
    // 2. weights
    VG_HIP(vg_zw_launch(c->theta, 0, d1.lam0, d2.lam0, (int)m1, (int)m2, Xa[0], Xl[0], c->r1, c->r1l, WE[0], WF[0], st));
    VG_HIP(vg_zw_launch(c->theta, 1, d2.lam0, d1.lam0, (int)m2, (int)m1, Xa[1], Xl[1], c->r2, c->r2l, WE[1], WF[1], st));
    // 3. back to the original basis: W_M = Q W_E Q^T, W_H = Q (W_F + W_F^T) Q^T (Q = Qt^T), T1 = Q1 (beta / v^2) Q2^T
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        vg_gemm_add(&g, WE[k], d.m, 1, d.Qt, d.m, 1, TA[k], d.m, d.m, d.m, d.m);
        vg_gemm_add(&g, WF[k], d.m, 1, d.Qt, d.m, 1, TB[k], d.m, d.m, d.m, d.m);
    }
    vg_gemm_add(&g, c->beta, m2, 1, d2.Qt, m2, 1, U, (int)m2, (int)m1, (int)m2, (int)m2, 1, 0, 1, 0, 1.0 / (v * v));
    VG_HIP(vg_gemm_launch(&g, st));
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        vg_gemm_add(&g, d.Qt, 1, d.m, TA[k], d.m, 1, WE[k], d.m, d.m, d.m, d.m, 1, 0, 1, 0, lead ? 1.0 : 0.0);       // W_M -> WE (replicated: rank 0 only)
        vg_gemm_add(&g, d.Qt, 1, d.m, TB[k], d.m, 1, WF[k], d.m, d.m, d.m, d.m);       // W_H -> WF
    }
    vg_gemm_add(&g, d1.Qt, 1, m1, U, m2, 1, T1, (int)m2, (int)m1, (int)m2, (int)m1);
    VG_HIP(vg_gemm_launch(&g, st));
    // 4. W_V = s W_H B0 (+ the projection term in the next launch)
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        if (!pts[k]) continue;
        vg_gemm_add(&g, WF[k], d.m, 1, d.BV, d.n, 1, WV[k], d.n, d.m, d.n, d.m, 1, 0, 1, 0, k ? s2 : (lead ? s1 : 0.0));       // (dimension 1: replicated)
    }
    VG_HIP(vg_gemm_launch(&g, st));
    vg_gemm_init(&g);
    const double rs = std::sqrt(s1 * s2);
    if (pts[0]) {
        const int ip = vg_gemm_add(&g, T1, m2, 1, c->St, n1, 1, WV[0], (int)n1, (int)m1, (int)n1, (int)m2, 1, 0, c->st_slabs, 2L * m2 * n1, rs, 1);
        (void)ip;
    }
    if (pts[1]) {
        vg_gemm_add(&g, T1, 1, m2, R1, n2, 1, WV[1], (int)n2, (int)m2, (int)n2, (int)m1, 1, 0, 1, 0, rs, 1);
    }
    VG_HIP(vg_gemm_launch(&g, st));
    // 5. Abar = L0^-T W_V and Kbar = L0^-T W_M L0^-1 by substitution, in place (W_M sits in WE: first from the left, then -- on the
    //    transposed view -- from the right).  Not through the explicit inverse: on RBF factors that costs digits (section 2 of
    //    DESIGN.md), and here they are multiplied by 1 / (z_i - z_j).
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
                q[nq++] = VgTrsmSpec{d.L0, d.m, dp, blk, dld, WV[k], d.n, 1, d.n, d.m, 1};
                q[nq++] = VgTrsmSpec{d.L0, d.m, dp, blk, dld, WE[k], d.m, 1, d.m, d.m, 1};          // L^-T W_M
            } else {
                q[nq++] = VgTrsmSpec{d.L0, d.m, dp, blk, dld, WE[k], 1, d.m, d.m, d.m, 1};          // (.) L^-1: L^-T on the transpose
            }
        }
        if ((rc = vg_trsm_batch(q, nq, st))) return rc;
    }
    // 6. contraction with d kappa / d z
    double *o1 = multi ? gzbuf : gz1, *o2 = multi ? gzbuf + m1 : gz2;
    if (multi) VG_HIP(hipMemsetAsync(gzbuf, 0, sizeof(double) * (m1 + m2), st));
    if (pts[0]) VG_HIP(vg_zdot_launch(c->theta, 0, d1.grid, d1.x, (int)m1, n1, WV[0], d1.AD + m1 * n1, WE[0], d1.dK0, o1, st));
    if (pts[1]) VG_HIP(vg_zdot_launch(c->theta, 1, d2.grid, d2.x, (int)m2, n2, WV[1], d2.AD + m2 * n2, WE[1], d2.dK0, o2, st));
    if (multi) {
        if ((rc = vg_allreduce(c, gzbuf, m1 + m2, st))) return rc;
        VG_HIP(hipMemcpyAsync(gz1, gzbuf, sizeof(double) * m1, hipMemcpyDeviceToDevice, st));
        VG_HIP(hipMemcpyAsync(gz2, gzbuf + m1, sizeof(double) * m2, hipMemcpyDeviceToDevice, st));
    }
    { const int wrc_ = vg_comm_wait(c, st); if (wrc_) return wrc_; }
    return VGGP_OK;
}

// Diagnostic builds only (tools/: -DVGGP_DIAG, or the stamp builds -DVG_EIG_RT / -DVG_CHOL_STAMP): the shipped library exports
// exactly the symbols include/vggp.h declares (tests/test_cabi.py checks the dynamic symbol table).
#if defined(VGGP_DIAG) || defined(VG_EIG_RT) || defined(VG_CHOL_STAMP)
extern "C" int vggp_debug_read_out(vggp_ctx* c, double* host8) {
    if (!c || !c->out) return VGGP_EINVAL;
    VG_HIP(hipMemcpy(host8, c->out, 8 * sizeof(double), hipMemcpyDeviceToHost));
    return VGGP_OK;
}

// diagnostic builds only (-DVG_EIG_RT): the eigensolver's global work area of dimension `dim` (which = 1: the Ritz problem's)
extern "C" int vggp_debug_read_gwork(vggp_ctx* c, int dim, int which, void* host, int64_t offset_doubles, int64_t bytes) {
    if (!c || !c->planned || dim < 0 || dim > 1) return VGGP_EINVAL;
    // which = 2: Gw (the matrix the main eigensolver started from), 3: the Ritz matrix Hs, 4: lam0, 5: the Ritz solve's counters (ints)
    if (which == 6) { VG_HIP(hipMemcpy(host, c->tAC + offset_doubles, bytes, hipMemcpyDeviceToHost)); return VGGP_OK; }
    const double* src = which == 5 ? reinterpret_cast<const double*>(c->d[dim].counters2) : which == 2 ? c->d[dim].Gw : which == 3 ? c->d[dim].Hs : which == 4 ? c->d[dim].lam0 : which ? c->d[dim].gwork2 : c->d[dim].gwork;
    if (!src) return VGGP_EINVAL;
    VG_HIP(hipMemcpy(host, src + offset_doubles, bytes, hipMemcpyDeviceToHost));
    return VGGP_OK;
}

extern "C" int vggp_debug_read_misc(vggp_ctx* c, void* host, int64_t bytes) {
    if (!c || !c->misc || (size_t)bytes > c->misc_bytes) return VGGP_EINVAL;
    VG_HIP(hipMemcpy(host, c->misc, bytes, hipMemcpyDeviceToHost));
    return VGGP_OK;
}
#endif

extern "C" const char* vggp_project_kernel_name(void) { return vg_last_project_kernel(); }

extern "C" int vggp_profile(vggp_ctx* c, int enable) {
    if (!c) { vg_set_error("null context"); return VGGP_EINVAL; }
    VG_ENTER_DEVICE(c->device);
    if (enable && !c->ev[0])
        for (int i = 0; i < VG_MAXEV; ++i) VG_HIP(hipEventCreate(&c->ev[i]));
    c->prof = enable != 0;
    return VGGP_OK;
}

extern "C" int vggp_profile_read(vggp_ctx* c, double ms_out[VGGP_NSTAGE], int32_t* steps_out, int reset) {
    if (!c || !ms_out) { vg_set_error("null argument"); return VGGP_EINVAL; }
    for (int i = 0; i < VGGP_NSTAGE; ++i) ms_out[i] = c->prof_ms[i];
    if (steps_out) *steps_out = c->prof_steps;
    if (reset) { for (int i = 0; i < VGGP_NSTAGE; ++i) c->prof_ms[i] = 0.0; c->prof_steps = 0; }
    return VGGP_OK;
}

extern "C" int vggp_sumsq(vggp_ctx* c, const double* y, int64_t n, double* out, void* stream) {
    if (!c) { vg_set_error("null context"); return VGGP_EINVAL; }
    VG_REQUIRE(y && out && n >= 0, "vggp_sumsq: bad argument");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VG_HIP(vg_sumsq_launch(y, n, c->sumsq_partial, c->sumsq_out, st));
    const int rca = vg_allreduce(c, c->sumsq_out, 1, st);          // total over the ranks of the context (no-op for one rank)
    if (rca) return rca;
    VG_HIP(hipMemcpyAsync(out, c->sumsq_out, sizeof(double), hipMemcpyDeviceToHost, st));
    { const int wrc_ = vg_comm_wait(c, st); if (wrc_) return wrc_; }
    return VGGP_OK;
}
