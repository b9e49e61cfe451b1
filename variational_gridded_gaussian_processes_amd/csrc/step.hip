// The full-grid ELBO step of libvggp_hip.so: the partials half (factors, Cholesky, projections, Gram products), the finish half
// (one function per eigensolver chain, the main solve, the rotations and the final reduction), the HIP-graph cache, the start
// policy that picks the chain, and the four vggp_elbo_* entries.  Host logic only, as in api.hip: every number comes out of the
// kernels in factor_build.hip, chol.hip, trsm.hip, gemm.hip, eigh.hip, thin.hip and mspace.hip.
#include "common.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include <algorithm>

#include "ctx.h"
#define VG_CHOL_MAXJOBS_HOST 8
#define VG_NEWTON_TOL 1e-12      // off-diagonal threshold of the Newton chain's rotations, relative to ||Gw||_F / m
#define VG_NEWTON_NULL 1e-12     // rows whose eigenvalue was below this fraction of the largest in the PREVIOUS step form the known null space:
                                 // pairs inside it are neither rotated nor judged (VgRefineJob::lam_prev)
#define VG_NEWTON_CLUSTER 1e-7   // ... and the rows below this fraction form the near-null cluster, whose internal pairs wait for the second iteration
#define VG_NEWTON_NOISE 1e-13    // diagonal entries below this fraction of the largest are "at the rounding floor" (VgRefineJob::noise)
#define VG_NEWTON_ACCEPT 1e-11   // ... of its convergence check: Gw = S G S^T comes out of two GEMMs with ~ eps sqrt(m) ||G|| of rounding noise per
                                 // element, 2e-15 ||G|| at m = 256 against 4e-15 ||G||_F for 1e-12 -- the chain converged TO the threshold and
                                 // missed by a hair (measured: 10 log10(offdiag / thr) = 0 at every miss); the ELBO sees such elements at second order

// Per-stage profiling (bench.py): in profiling mode the step runs as plain launches on ONE stream (no graph, no side stream)
// and an event is recorded after every launch group; stage `id` is charged the time since the previous event.
// VG_MARK(-1) only (re)starts the clock (start of the step, start of the finish half after the caller's all-reduce).
#define VG_MARK(id)                                                                                     \
    do {                                                                                                \
        if (c->prof && c->nev < VG_MAXEV) { VG_HIP(hipEventRecord(c->ev[c->nev], st)); c->ev_stage[c->nev++] = (id); } \
    } while (0)

// Fork / join onto the context's side stream (works eagerly and under stream capture, where it becomes a graph branch).
// OFF by default: measured on ROCm 7.2 / MI355X (gpurun_out/r2c), running the projection of Y (2 launches, 40 us) beside
// the eigensolver chain as a second graph branch made the 1024^2 step SLOWER (0.478 vs 0.453 ms) -- every cross-stream
// edge of a replayed graph costs more than the launches it hides; independent work is batched into shared launches
// instead (see the prediction GEMMs in rotate_and_reduce).  VGGP_FORK=1 switches the branch on for A/B runs.
// Profiling mode keeps everything on the one stream so that the per-stage events mean what they say.
static hipStream_t vg_side(vggp_ctx* c, hipStream_t st) {
    static const bool on = getenv("VGGP_FORK") != nullptr;
    return (c->prof || !on) ? st : c->side_stream;
}
#define VG_FORK(i)                                                                                      \
    do { if (sx != st) { VG_HIP(hipEventRecord(c->ev_fork[i], st)); VG_HIP(hipStreamWaitEvent(sx, c->ev_fork[i], 0)); } } while (0)
#define VG_JOIN_RECORD(i) do { if (sx != st) VG_HIP(hipEventRecord(c->ev_join[i], sx)); } while (0)
#define VG_JOIN_WAIT(i) do { if (sx != st) VG_HIP(hipStreamWaitEvent(st, c->ev_join[i], 0)); } while (0)

// Enqueue-only halves of the step (no host synchronisation, no host-side reads): they run either directly on the
// caller's stream (profiling mode) or once under stream capture, after which the step is a single graph launch.
// riders: see vg_partials_enqueue.  Off in profiling mode (every stage is then its own launch and can be timed) and with VGGP_NO_RIDE=1.
static bool vg_ride(const vggp_ctx* c) {
    static const bool off = getenv("VGGP_NO_RIDE") != nullptr;
    return !off && !c->prof && c->desc.m1 <= 128 && c->desc.m2 <= 128;
}

// Cholesky of a factor with 128 < m <= 256 inside the step: [[A11, .], [A21, A22]] with a 128-block A11, all four jitter levels
// side by side as independent plain factorisations of K + jitter I (the step's graph cannot walk the jitter ladder on the host):
// per level  L11 = chol(A11), L21 = A21 L11^-T (substitution), S22 = A22 - L21 L21^T (MFMA), L22 = chol(S22); the lowest level
// whose two blocks both survive is selected on the device.  Leaves L0, the inverses of its 16 x 16 diagonal blocks (Dinv0), the
// jitter value and the status word -- exactly what the m <= 128 launch leaves.  (The single-workgroup generic kernel this replaces
// took 3.0 ms at m = 256: profiles/r2_md256_kernel_stats.csv.)
static int vg_chol_big_enqueue(vggp_ctx* c, const int* dims, int ndims, hipStream_t st) {
    VgCholJob cj[VG_CHOL_MAXJOBS_HOST];
    int nj = 0;
    for (int t = 0; t < ndims; ++t) {
        VgDim& d = c->d[dims[t]];
        VG_HIP(vg_jitcopy_launch(d.K0, d.m, d.Kc, st));
    }
    const long NB = 128;
    for (int stage = 0; stage < 2; ++stage) {
        if (stage == 1) {
            // L21^T = L11^-1 A21^T by substitution (transposed views), then S22 = A22 + jitter I - L21 L21^T in place
            VgTrsmJob tj[8];
            int nt = 0;
            VgGemmBatch g;
            vg_gemm_init(&g);
            for (int t = 0; t < ndims; ++t) {
                VgDim& d = c->d[dims[t]];
                const long m = d.m, mm = m * m, rest = m - NB, nb16 = (m + 15) / 16;
                for (int l = 0; l < 4; ++l) {
                    double* Kl = d.Kc + l * mm;
                    double* Ll = d.Lc + l * mm;
                    // R(k, c) = A21[c][k], X(k, c) -> L21[c][k]: both with element (k, c) at base[k + c * m]
                    tj[nt++] = VgTrsmJob{Ll, d.Dc + l * nb16 * 256, Kl + NB * m, Ll + NB * m, m, 256, 16, 1, m, 1, m, rest, (int)NB, 0};
                    vg_gemm_add(&g, Ll + NB * m, m, 1, Ll + NB * m, 1, m, Kl + NB * m + NB, (int)m, (int)rest, (int)rest, (int)NB, 1, 0, 1, 0, -1.0, 1);
                }
            }
            VG_HIP(vg_trsm_launch(tj, nt, st));
            VG_HIP(vg_gemm_launch(&g, st));
        }
        nj = 0;
        for (int t = 0; t < ndims; ++t) {
            VgDim& d = c->d[dims[t]];
            const long m = d.m, mm = m * m, nb16 = (m + 15) / 16;
            const long o = stage ? NB : 0;
            const int mb = stage ? (int)(m - NB) : (int)NB;
            for (int l = 0; l < 4; ++l) {
                VgCholJob j{d.Kc + l * mm + o * m + o, d.Lc + l * mm + o * m + o, nullptr, d.chol_scratch, nullptr, d.st8 + 2 * l + stage, mb};
                j.ldk = (int)m; j.ldl = (int)m; j.only_level0 = 1;
                j.Dinv_out = d.Dc + l * nb16 * 256 + (o / 16) * 256;
                cj[nj++] = j;
            }
        }
        VG_HIP(vg_chol_launch(cj, nj, st));
    }
    for (int t = 0; t < ndims; ++t) {
        VgDim& d = c->d[dims[t]];
        VG_HIP(vg_cholsel_launch(d.Lc, d.Dc, d.st8, d.m, d.L0, d.Dinv0, d.jitter, d.status, st));
    }
    return VGGP_OK;
}

// The Newton-Schulz step of the predicted start basis, Fp += -0.5 Wp Ep, of both dimensions (operands left by the previous step's
// tail, see rotate_and_reduce): needs nothing of this step, so it rides in whichever early launch of the partials has room.
static void vg_add_ns(vggp_ctx* c, VgGemmBatch* b) {
    for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(b, d.Wp, d.m, 1, d.Ep, d.m, 1, d.Fp, d.m, d.m, d.m, d.m, 1, 0, 1, 0, -0.5, 1); }
}

int vg_partials_enqueue(vggp_ctx* c, const double* Y, double* payload, hipStream_t st, const VgPartials& o) {
    // early (1: thin chain of a fused single-rank step, chain_thin; 2: the regular warm chains, where [C;C1;C2] then is the first
    // rider of the eigensolver chain instead of S): the pass over Y is taken BEFORE the whitening --
    // S' = [A2;dA2] Y needs nothing but the factor build, so it rides in the Cholesky launch (250 idle CUs for 43 us), and
    // S = L2^-1 S' is a handful of extra strips of the substitution launch (L^-1 (A Y) instead of (L^-1 A) Y: the same
    // substitution, applied to other right-hand sides).  [C;C1;C2] is then complete before the Ritz solve and nothing that touches
    // Y or C is left behind it.
    const bool reduce = o.reduce, extrap = o.extrap, fused = o.fused, apply_ns = o.apply_ns;
    const int early = o.early;
    const long n1 = c->desc.n1, n2 = c->desc.n2, m1 = c->desc.m1, m2 = c->desc.m2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    hipStream_t sx = vg_side(c, st);
    VgGemmBatch g;
    VG_MARK(-1);

    // 1. factor build (unit outputscale): A0|dA0, K0, dK0 for both dimensions.  First node of the step: it reads the
    //    hyper-parameters from the pinned host block (and leaves a device copy for the later kernels), and its block 0
    //    zeroes the status words, the jitter-level flags and the Jacobi progress words of the step.
    VgFactorJob fj[2];
    VgCholJob cj[2];
    // m <= 128: the Cholesky launch only leaves L and the inverses of its 16 x 16 diagonal blocks; L^{-1} itself (wanted by
    // Mk = X L^{-T} and by the read-outs) comes out of the substitution launch as one more right-hand side, the identity
    static const bool chol_legacy = getenv("VGGP_CHOL_LEGACY") != nullptr;
    const bool dinv_path = d1.m <= VG_TRSM_BLK && d2.m <= VG_TRSM_BLK && !chol_legacy;
    VgClearArgs clr;
    clr.n = 0;
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        fj[k] = VgFactorJob{d.x, d.grid, d.AD, d.AD + (long)d.m * d.n, d.K0, d.dK0, d.n, d.m, d.kind, d.basis, k, 0.0, c->desc.flags};
        clr.ptr[clr.n] = d.status; clr.nwords[clr.n++] = 2;
        clr.ptr[clr.n] = reinterpret_cast<int*>(d.chol_scratch); clr.nwords[clr.n++] = 16;     // jitter-level flags
        clr.ptr[clr.n] = d.counters; clr.nwords[clr.n++] = 8;                                  // Jacobi progress words (counters, counters2)
        if (k == 0) { clr.ptr[clr.n] = reinterpret_cast<int*>(c->payload + c->payload_len); clr.nwords[clr.n++] = 2; }   // peer-failure word
        if (d.st8) { clr.ptr[clr.n] = d.st8; clr.nwords[clr.n++] = 8; }                        // block statuses of the m > 128 Cholesky
        cj[k] = VgCholJob{d.K0, d.L0, dinv_path ? nullptr : d.Linv0, d.chol_scratch, d.jitter, d.status, d.m};
        cj[k].Dinv_out = d.Dinv0;
    }
    VG_HIP(vg_factor_build_launch(fj, 2, c->d_htheta, st, c->theta, &clr));
    VG_MARK(0);

    // 2. Cholesky (+ jitter schedule) and explicit inverse of both factors
    // The Newton-Schulz step of the predicted start basis (vg_add_ns) rides in the Cholesky launch (8 workgroups on 256 CUs) when
    // that is the MFMA kernel, otherwise in a GEMM launch further down.
    const bool ns_on_chol = extrap && apply_ns && dinv_path;
    static const bool chol_big_off = getenv("VGGP_NO_CHOL_BIG") != nullptr;
    const bool any_big = (d1.m > VG_TRSM_BLK || d2.m > VG_TRSM_BLK) && !chol_legacy && !chol_big_off;
    VgGemmBatch gsp;
    vg_gemm_init(&gsp);
    int sp_slabs = 1;
    if (early) {
        // (two callers: the fused single-rank step -- no reduction, [C;C1;C2] becomes a rider of the eigensolver chain -- and the
        //  partials half of a multi-rank step -- reduce: [C;C1;C2] shares the Gram launch and the slab reduction fills the payload)
        const bool ok_fused = fused && !reduce && (vg_ride(c) || c->prof);
        const bool ok_partials = reduce;                 // (also the cold thin step: fused, reduced operands)
        if (!(dinv_path && !any_big && (ok_fused || ok_partials) && Y && sx == st)) {
            vg_set_error("internal: the early projection was requested where it cannot run");
            return VGGP_ESTATE;
        }
        // split-K only as far as the chip needs it: the plan's split of S (256 workgroups) capped at VG_SP_SLABS -- 4 slabs at 1024^2, ONE
        // for a 1024 x 4096 slab, whose 64 x 64 tiles fill the chip by themselves (no slab traffic, two substitution jobs instead of eight)
        vg_gemm_add(&gsp, d2.AD, n2, 1, Y, n1, 1, c->Sp, (int)n1, (int)(2 * m2), (int)n1, (int)n2, std::min(c->st_split, VG_SP_SLABS), 2L * m2 * n1);
        sp_slabs = gsp.p[0].ksplit;
        if (c->prof) {                 // profiling mode: every launch group by itself -- the pass over Y as a launch of its own
            vg_gemm_xcd_group(&gsp, 0);
            VG_HIP(vg_gemm_launch(&gsp, st, VG_GEMM_TAG_GRAM_PROJECT));
            VG_MARK(4);
        }
    }
    if (!any_big) {
        // riders of the Cholesky launch: the early pass over Y and / or the Newton-Schulz step of the predicted start basis
        VgGemmBatch gr2; vg_gemm_init(&gr2);
        if (early && !c->prof) gr2 = gsp;
        if (ns_on_chol) vg_add_ns(c, &gr2);
        VG_HIP(vg_chol_launch(cj, 2, st, ((early && !c->prof) || ns_on_chol) ? &gr2 : nullptr));
    } else {
        // a factor beyond one 128-block: blocked (vg_chol_big_enqueue); a small partner keeps the one-launch MFMA kernel.  Either
        // way the launch leaves L0 and the diagonal-block inverses only; L0^-1 comes out of the substitution below.
        int big[2], nbig = 0;
        for (int k = 0; k < 2; ++k) {
            if (c->d[k].m > VG_TRSM_BLK) big[nbig++] = k;
            else { cj[k].Linv = nullptr; VG_HIP(vg_chol_launch(&cj[k], 1, st)); }
        }
        const int rcb = vg_chol_big_enqueue(c, big, nbig, st);
        if (rcb) return rcb;
    }
    c->dinv_valid = dinv_path || any_big;
    VG_MARK(1);

    // 3. B|V = L0^{-1} [A0|dA0],  X = L0^{-1} dK0  by blocked substitution on the matrix cores (trsm.hip; the 16 x 16
    //    diagonal-block inverses are the diagonal blocks of Linv0).  Not "Linv0 times A0": on RBF factors that product
    //    carries cond(L0) into every element of B and shows in the posterior variance of large grids.
    {
        const bool big = d1.m > VG_TRSM_BLK || d2.m > VG_TRSM_BLK;
        if (!big) {
            VgTrsmJob tj[16];
            int nt = 0;
            for (int k = 0; k < 2; ++k) {
                VgDim& d = c->d[k];
                const long mn = (long)d.m * d.n;
                const double* dv = dinv_path ? d.Dinv0 : d.Linv0;
                const long dblk = dinv_path ? 256 : 16L * d.m + 16, dld = dinv_path ? 16 : d.m;
                for (int b = 0; b < 2; ++b)
                    tj[nt++] = VgTrsmJob{d.L0, dv, d.AD + b * mn, d.BV + b * mn, d.m, dblk, dld, d.n, 1, d.n, 1, d.n, d.m, 0};
                tj[nt++] = VgTrsmJob{d.L0, dv, d.dK0, d.X, d.m, dblk, dld, d.m, 1, d.m, 1, d.m, d.m, 0};
                if (dinv_path) {
                    tj[nt] = VgTrsmJob{d.L0, dv, d.L0, d.Linv0, d.m, dblk, dld, d.m, 1, d.m, 1, d.m, d.m, 0};      // Linv0 = L0^{-1} I
                    tj[nt++].rhs_ident = 1;
                }
            }
            if (early)               // S = L2^-1 S', slab by slab (the substitution is linear: the consumer sums the slabs)
                for (int sl = 0; sl < sp_slabs; ++sl)
                    for (int b = 0; b < 2; ++b) {
                        const long o = (long)sl * 2 * m2 * n1 + (long)b * m2 * n1;
                        tj[nt++] = VgTrsmJob{d2.L0, d2.Dinv0, c->Sp + o, c->St + o, m2, 256, 16, n1, 1, n1, 1, n1, (int)m2, 0};
                    }
            VG_HIP(vg_trsm_launch(tj, nt, st));
        } else {
            // 128 < m <= 256: blocked (128-row diagonal solves + one GEMM update between them), in place on copies
            VgTrsmSpec q[8];
            int nq = 0;
            for (int k = 0; k < 2; ++k) {
                VgDim& d = c->d[k];
                const long mn = (long)d.m * d.n;
                // diagonal-block inverses: Dinv0 when the Cholesky left them there, else the diagonal blocks of its explicit inverse
                const double* dv = any_big ? d.Dinv0 : d.Linv0;
                const long dblk = any_big ? 256 : 16L * d.m + 16, dld = any_big ? 16 : d.m;
                VG_HIP(hipMemcpyAsync(d.BV, d.AD, sizeof(double) * 2 * mn, hipMemcpyDeviceToDevice, st));
                VG_HIP(hipMemcpyAsync(d.X, d.dK0, sizeof(double) * d.m * d.m, hipMemcpyDeviceToDevice, st));
                for (int b = 0; b < 2; ++b) q[nq++] = VgTrsmSpec{d.L0, d.m, dv, dblk, dld, d.BV + b * mn, d.n, 1, d.n, d.m, 0};
                q[nq++] = VgTrsmSpec{d.L0, d.m, dv, dblk, dld, d.X, d.m, 1, d.m, d.m, 0};
                if (any_big) {           // L0^-1 = L0^-1 I, as in the m <= 128 launch
                    VG_HIP(hipMemcpyAsync(d.Linv0, d.Id, sizeof(double) * d.m * d.m, hipMemcpyDeviceToDevice, st));
                    q[nq++] = VgTrsmSpec{d.L0, d.m, dv, dblk, dld, d.Linv0, d.m, 1, d.m, d.m, 0};
                }
            }
            const int rc = vg_trsm_batch(q, nq, st);
            if (rc) return rc;
        }
    }
    VG_MARK(2);

    if (!Y) {          // factors only (scattered steps, masked.hip / iter_step.hip): B|V, X are done; Mk = X Linv0^T and nothing of the grid path
        vg_gemm_init(&g);
        for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(&g, d.X, d.m, 1, d.Linv0, 1, d.m, d.Mk, d.m, d.m, d.m, d.m); }
        VG_HIP(vg_gemm_launch(&g, st));
        return VGGP_OK;
    }
    // 4./5. (side stream in the fused step: overlaps the Gram products and the whole eigensolver chain, which need only G, H)
    //    S = [B2;V2] Y (split-K slabs): the only pass over Y; then [C;C1] = [B1;V1] S_B, C2 = B1 S_V (S slabs summed on
    //    load; split-K over n1).
    hipStream_t sp = (fused && !extrap) ? sx : st;
    // "Riders" (fused warm step): the two projection launches are not enqueued here at all -- their batches are handed to
    // finish_enqueue, which attaches them to the single-workgroup launches of the eigensolver chain (row QR / Ritz solve /
    // main solve) as extra workgroups, so they run BESIDE that chain on the 250 idle CUs instead of in front of it.
    const bool ride = fused && !reduce && sp == st && vg_ride(c);
    if (sp != st) VG_FORK(1);
    VgGemmBatch gp, gc;
    vg_gemm_init(&gp);
    vg_gemm_add(&gp, d2.BV, n2, 1, Y, n1, 1, c->St, (int)n1, (int)(2 * m2), (int)n1, (int)n2, c->st_split, 2L * m2 * n1);
    const int st_slabs = early ? sp_slabs : gp.p[0].ksplit;
    vg_gemm_xcd_group(&gp, 0);
    // predicted start basis of this step's eigensolvers: the previous step's tail left Qpred (Ep), 1.5 Qpred (Fp) and
    // W = Qpred Qpred^T (Wp); the Newton-Schulz step Fp += -0.5 W Qpred rides in this launch (see rotate_and_reduce)
    // -- or in the Gram launch when the projection itself is deferred
    const bool ns_late = extrap && apply_ns && !ns_on_chol;
    if (!ride && !early) {
        if (ns_late) vg_add_ns(c, &gp);
        VG_HIP(vg_gemm_launch(&gp, sp, VG_GEMM_TAG_GRAM_PROJECT));
        if (sp == st) VG_MARK(4);
    }
    vg_gemm_init(&gc);
    const long cc_slab = 3L * m1 * m2;
    vg_gemm_add(&gc, d1.BV, n1, 1, c->St, 1, n1, c->CCslab, (int)m2, (int)(2 * m1), (int)m2, (int)n1, c->cc_split, cc_slab,
                st_slabs, 2L * m2 * n1);
    vg_gemm_add(&gc, d1.BV, n1, 1, c->St + m2 * n1, 1, n1, c->CCslab + 2 * m1 * m2, (int)m2, (int)m1, (int)m2, (int)n1,
                c->cc_split, cc_slab, st_slabs, 2L * m2 * n1);
    const int cc_slabs = gc.p[0].ksplit;
    // 6. Gram pairs [G0;H0] = [B;V] B^T (split-K slabs), Mk = X Linv0^T: independent of the projection, so they share ITS
    //    second launch (whose own products fill less than half the chip) unless the projection branch runs on the side stream
    int gh_slabs[2] = {1, 1};
    auto add_gram = [&](VgGemmBatch* b) {
        for (int k = 0; k < 2; ++k) {
            VgDim& d = c->d[k];
            const int ig = vg_gemm_add(b, d.BV, d.n, 1, d.BV, 1, d.n, d.GHslab, d.m, 2 * d.m, d.m, d.n, d.gh_split, 2L * d.m * d.m);
            gh_slabs[k] = b->p[ig].ksplit;
            vg_gemm_add(b, d.X, d.m, 1, d.Linv0, 1, d.m, d.Mk, d.m, d.m, d.m, d.m);
        }
    };
    if (ride) {
        vg_gemm_init(&g);
        add_gram(&g);
        if (ns_late) vg_add_ns(c, &g);
        VG_HIP(vg_gemm_launch(&g, st));
        c->ride_proj = gp; c->ride_cc = gc;
        c->ride_pending = early != 1;      // (thin chain: S exists already and chain_thin places [C;C1;C2] itself)
        c->ride_stage0 = early == 2 ? 1 : 0;
    } else {
        if (sp == st) add_gram(&gc);
        VG_HIP(vg_gemm_launch(&gc, sp));
        if (sp == st) { VG_MARK(5); VG_MARK(6); }
        if (sp != st) {
            VG_JOIN_RECORD(1);
            vg_gemm_init(&g);
            add_gram(&g);
            VG_HIP(vg_gemm_launch(&g, st));
            VG_MARK(6);
        }
    }

    c->gh_slabs[0] = gh_slabs[0]; c->gh_slabs[1] = gh_slabs[1]; c->cc_slabs = cc_slabs; c->st_slabs = st_slabs;
    // 7. deterministic slab reduction into {G1,H1} (local) and the payload {G2,H2,C,C1,C2}.  Skipped inside a fused
    //    warm step: its consumers (three small GEMMs) then sum the slabs on load, one launch less on the critical path.
    if (!reduce) return VGGP_OK;          // fused warm step: the caller joins the projection branch before the rotations
    if (sp != st) VG_JOIN_WAIT(1);
    VgRedBatch r;
    vg_red_init(&r);
    vg_red_add(&r, d1.GHslab, d1.GH, 2L * m1 * m1, 2L * m1 * m1, gh_slabs[0]);
    vg_red_add(&r, d2.GHslab, payload, 2L * m2 * m2, 2L * m2 * m2, gh_slabs[1]);
    vg_red_add(&r, c->CCslab, payload + 2 * m2 * m2, 3L * m1 * m2, cc_slab, cc_slabs);
    VG_HIP(vg_red_launch(&r, st));
    VG_MARK(7);
    return VGGP_OK;
}

// The subspace start is fed the previous basis itself (U = I: the partials' extrapolation products reduce to its Newton-Schulz
// clean-up).  VGGP_SUB_EXTRAP=1 feeds it the extrapolated basis instead: 5 us faster at m = 128, but at m = 64 the main
// eigensolver was seen to need 55 rounds instead of ~10, so it is not the default.
static bool vg_sub_ident() { static const bool ex = getenv("VGGP_SUB_EXTRAP") != nullptr; return !ex; }

// ---- the finish half ------------------------------------------------------------------------------------------------------------
// What a finish half is told: the start-basis strategy picked by vg_start_prepare (extrap .. newton) and where its operands are.
struct VgChain {
    bool warm = false;                // start from the previous step's basis
    bool extrap = false, refine = false, subspace = false, thin = false;
    int newton = 0;                   // iterations of the Newton chain (0: another chain)
    bool from_slabs = false;          // fused warm step: G, H, C are still split-K slabs; every consumer is a GEMM that sums them on load
    bool copy_theta = false;          // stand-alone finish (multi-rank seam): refresh the device copy of the hyper-parameters
    bool thin_early = false;          // thin chain: the partials half took the early pass over Y (vg_partials_enqueue, early)
};
// The eigensolver chain of a finish half.  ONE mapping decides both the function that runs (finish_enqueue) and the graph slot
// that holds its capture (vg_graph_slot).  vg_start_prepare makes the flags exclusive: thin implies subspace, the Newton chain
// and the refinement exclude the subspace start and each other, and a refined start is an extrapolated one.
enum VgChainKind { VG_CHAIN_COLD, VG_CHAIN_THIN, VG_CHAIN_NEWTON, VG_CHAIN_SUBSPACE, VG_CHAIN_REFINE, VG_CHAIN_EXTRAP, VG_CHAIN_PLAIN };
static VgChainKind vg_chain_kind(const VgChain& ch) {
    if (!ch.warm) return VG_CHAIN_COLD;
    if (ch.thin) return VG_CHAIN_THIN;
    if (ch.newton) return VG_CHAIN_NEWTON;
    if (ch.subspace) return VG_CHAIN_SUBSPACE;
    if (ch.extrap) return ch.refine ? VG_CHAIN_REFINE : VG_CHAIN_EXTRAP;
    return VG_CHAIN_PLAIN;
}

// G, H and [C;C1;C2] as the finish half reads them: reduced (a payload), or the split-K slabs of a fused warm step.
struct VgStepOperands {
    const double *G0[2], *H0[2], *C3;
    int ghn[2], ccn;                  // slab counts
    long ghs[2], ccs;                 // slab strides
    // "current readers": G and H for the launches after a chain's first one -- the reduced copies once that launch made them
    const double *Gr[2], *Hr[2];
    int grn[2], hrn[2];
    double* gdst[2];                  // where the reduced copies go: [G;H] of dimension 1, the head of the context's payload

    VgStepOperands(vggp_ctx* c, const double* payload, bool from_slabs) {
        const long m1 = c->desc.m1, m2 = c->desc.m2;
        G0[0] = from_slabs ? c->d[0].GHslab : c->d[0].GH; G0[1] = from_slabs ? c->d[1].GHslab : payload;
        H0[0] = G0[0] + m1 * m1; H0[1] = G0[1] + m2 * m2;
        C3 = from_slabs ? c->CCslab : payload + 2 * m2 * m2;
        ghs[0] = 2L * m1 * m1; ghs[1] = 2L * m2 * m2; gdst[0] = c->d[0].GH; gdst[1] = c->payload;
        ccn = from_slabs ? c->cc_slabs : 1; ccs = 3L * m1 * m2;
        for (int k = 0; k < 2; ++k) {
            ghn[k] = grn[k] = hrn[k] = from_slabs ? c->gh_slabs[k] : 1;
            Gr[k] = G0[k]; Hr[k] = H0[k];
        }
    }
    // G is read several times in a warm chain; where it is still split-K slabs, the chain's first launch also leaves reduced copies
    // ("Id G", "Id H" through the slab-summing GEMM) for the later readers, which this repoints.  want_G = false: H only.
    void add_reduced(vggp_ctx* c, VgGemmBatch* g, int k, bool want_G) {
        if (ghn[k] <= 1) return;      // (reduced operands: nothing to sum)
        VgDim& d = c->d[k];
        const long mm = (long)d.m * d.m;
        if (want_G) {
            vg_gemm_add(g, d.Id, d.m, 1, G0[k], d.m, 1, gdst[k], d.m, d.m, d.m, d.m, 1, 0, ghn[k], ghs[k]);
            Gr[k] = gdst[k]; grn[k] = 1;
        }
        vg_gemm_add(g, d.Id, d.m, 1, H0[k], d.m, 1, gdst[k] + mm, d.m, d.m, d.m, d.m, 1, 0, ghn[k], ghs[k]);
        Hr[k] = gdst[k] + mm; hrn[k] = 1;
    }
};

// The projection launches a fused warm step deferred to the eigensolver chain (vg_partials_enqueue: ride_proj = S = [B2;V2] Y, then
// ride_cc = [C;C1;C2]; S is already there after an early projection): each single-workgroup launch of the chain takes the next one
// along as extra workgroups, and what no launch took runs by itself.
struct VgRiders {
    vggp_ctx* c;
    int stage;                        // 0: S pending, 1: [C;C1;C2] pending, 2: nothing pending (or nothing deferred)
    VgRiders(vggp_ctx* c_, bool from_slabs) : c(c_), stage((from_slabs && c_->ride_pending) ? c_->ride_stage0 : 2) {}
    bool pending() const { return stage < 2; }
    const VgGemmBatch* next() { return stage >= 2 ? nullptr : (stage++ == 0 ? &c->ride_proj : &c->ride_cc); }
    int flush(hipStream_t st) { while (const VgGemmBatch* b = next()) VG_HIP(vg_gemm_launch(b, st)); return VGGP_OK; }
};

// one finish half in flight: what its pieces share, and the pieces (finish_enqueue runs one chain, then the two tail pieces)
struct VgFinish {
    vggp_ctx* c; hipStream_t st; const double* payload; double yy_total;
    VgChain ch; VgChainKind kind;
    VgStepOperands op;
    VgRiders riders;
    int start_times_G(const double* S1, int rows1, const double* S2, int rows2, bool want_G);
    int chain_thin(), chain_subspace(), chain_newton(), chain_refine(), main_solve(), rotate_and_reduce();
};
// First launch of every warm chain: TM = S G for rows_d rows S_d of the start basis (all m, or the r range rows of the thin chain), G
// summed from its slabs on load, and the reduced copies of G (want_G) and H for the later readers (VgStepOperands::add_reduced).
int VgFinish::start_times_G(const double* S1, int rows1, const double* S2, int rows2, bool want_G) {
    VgGemmBatch g;
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        vg_gemm_add(&g, k ? S2 : S1, d.m, 1, op.G0[k], d.m, 1, d.TM, d.m, k ? rows2 : rows1, d.m, d.m, 1, 0, op.ghn[k], op.ghs[k]);
        op.add_reduced(c, &g, k, want_G);
    }
    VG_HIP(vg_gemm_launch(&g, st));
    VG_MARK(8);
    return VGGP_OK;
}

// Ritz problem of the subspace and thin chains: the launch forms H = T V1^T itself (Hl, Hr) and solves it from the Newton start
static VgEigJob vg_ritz_job(VgDim& d) {
    return vg_make_ritz_job(d.Zs, d.V1s, d.sub_r, d.m, d.lam_s, d.Ws, d.gwork2, d.rotlog2, d.roundlog2, d.counters2, d.max_rounds,
                            (long)vg_eigh_log_bytes(d.m), d.perm2, d.status + 1);
}

// multi-rank step: the word behind the payload travelled through the all-reduce; non-zero = some rank failed its partials
static const double* vg_peer_fail(const vggp_ctx* c, const double* payload) {
    return (payload == c->payload && (c->n_ranks > 1 || c->comm || c->cb)) ? c->payload + c->payload_len : nullptr;
}

// ---- THIN chain (thin.hip): numerically rank-deficient Gram matrices, r = numerical rank + margin <= 32 per dimension.
// V = the r leading eigenvectors of the previous step (rows of QtPrev); Z = V G (one step of subspace iteration: G
// annihilates every null component); V1 = orth(Z) spans range(G); Rayleigh-Ritz on V1 G V1^T gives the range eigenpairs
// (W, theta) -- and that is all the ELBO and its gradient need: every rotated quantity is W (V1 . V1^T) W^T of an
// r x r matrix, formed by the tail kernel itself.  No complement basis, no full eigensolve, no m x m rotation.
// early (vg_partials_enqueue took the pass over Y before the whitening: S is there): [C;C1;C2] rides beside the row QR,
// {C,C1,C2} V1_2^T joins the launch after it, V1_1 (.) rides in the Ritz launch, the tail kernel follows the Ritz solve directly
// and the new range basis E_r = W V1 -- which only the NEXT step reads -- trails behind the tail (the host has its results by then)
// (multi-rank step: the partials half took the early pass and [C;C1;C2] arrives reduced in the payload -- same placement,
//  no rider beside the row QR)
// This chain is the whole finish half: nothing of main_solve / rotate_and_reduce follows it.
int VgFinish::chain_thin() {
    const long m1 = c->desc.m1, m2 = c->desc.m2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const bool early = ch.thin_early && !riders.pending();
    auto add_cv = [&](VgGemmBatch* b) {                  // {C,C1,C2} V1_2^T
        const int ic = vg_gemm_add(b, op.C3, m2, 1, d2.V1s, 1, m2, c->tCV, d2.sub_r, (int)(3 * m1), d2.sub_r, (int)m2);
        b->p[ic].a_nslab = op.ccn; b->p[ic].a_slab = op.ccs;
    };
    auto add_ac = [&](VgGemmBatch* b) {                  // V1_1 ({C,C1,C2} V1_2^T)
        for (int q = 0; q < 3; ++q)
            vg_gemm_add(b, d1.V1s, m1, 1, c->tCV + (long)q * m1 * d2.sub_r, d2.sub_r, 1, c->tAC + (long)q * d1.sub_r * d2.sub_r, d2.sub_r,
                        d1.sub_r, d2.sub_r, (int)m1);
    };
    auto add_er = [&](VgGemmBatch* b) {                  // the new range basis E_r = W V1 into the leading rows of QtPrev (next step's V)
        for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(b, d.Ws, d.sub_r, 1, d.V1s, d.m, 1, d.QtPrev, d.m, d.sub_r, d.m, d.sub_r); }
    };
    if (int rc = start_times_G(d1.QtPrev, d1.sub_r, d2.QtPrev, d2.sub_r, true)) return rc;      // Z = V G
    VgGemmBatch g; VgRowQrJob qj[2];
    for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; qj[k] = VgRowQrJob{d.TM, d.V1s, d.sub_r, d.m, nullptr, nullptr, 0}; }
    // + rider: [C;C1;C2] (early; profiling mode has launched it by itself) / S = [B2;V2] Y
    VG_HIP(vg_rowqr_launch(qj, 2, st, early ? ((c->prof || !ch.from_slabs) ? nullptr : &c->ride_cc) : riders.next()));
    VG_MARK(9);
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        const int r = d.sub_r;
        vg_gemm_add(&g, d.V1s, d.m, 1, op.Gr[k], d.m, 1, d.Zs, d.m, r, d.m, d.m, 1, 0, op.grn[k], op.ghs[k]);        // T = V1 G
        vg_gemm_add(&g, d.V1s, d.m, 1, d.Mk, d.m, 1, d.tMV, d.m, r, d.m, d.m);                                     // V1 Mk0
        vg_gemm_add(&g, d.V1s, d.m, 1, op.Hr[k], d.m, 1, d.tHV, d.m, r, d.m, d.m, 1, 0, op.hrn[k], op.ghs[k]);       // V1 H0
    }
    if (early) add_cv(&g);
    VG_HIP(vg_gemm_launch(&g, st));
    VG_MARK(10);
    // Ritz solve (forms H = T V1^T itself, Newton iteration); riders: the r x r sandwiches, and [C;C1;C2] of the fused step
    VgGemmBatch gx; vg_gemm_init(&gx);
    if (const VgGemmBatch* cc = riders.next()) gx = *cc;
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        const int r = d.sub_r;
        vg_gemm_add(&gx, d.tMV, d.m, 1, d.V1s, 1, d.m, d.tAM, r, r, r, d.m);                                // V1 Mk0 V1^T
        vg_gemm_add(&gx, d.tHV, d.m, 1, d.V1s, 1, d.m, d.tAH, r, r, r, d.m);                                // V1 H0 V1^T
    }
    if (early) add_ac(&gx);
    VgEigJob sj[2] = {vg_ritz_job(d1), vg_ritz_job(d2)};
    VG_HIP(vg_eigh_launch(sj, 2, st, &gx));
    c->ride_pending = false;
    VG_MARK(11);
    if (!early) {
        vg_gemm_init(&g);
        add_cv(&g);
        add_er(&g);
        VG_HIP(vg_gemm_launch(&g, st));
        VG_MARK(14);
        vg_gemm_init(&g);
        add_ac(&g);
        VG_HIP(vg_gemm_launch(&g, st));
        VG_MARK(15);
    }
    VgThinTail tt{};
    tt.theta = c->theta; tt.n_total = (double)c->desc.n_total; tt.yy = yy_total;
    tt.r1 = d1.sub_r; tt.r2 = d2.sub_r; tt.m1 = (int)m1; tt.m2 = (int)m2;
    tt.W1 = d1.Ws; tt.W2 = d2.Ws; tt.lam1 = d1.lam_s; tt.lam2 = d2.lam_s;
    tt.AM1 = d1.tAM; tt.AH1 = d1.tAH; tt.AM2 = d2.tAM; tt.AH2 = d2.tAH; tt.AC = c->tAC;
    tt.ac_nslab = 1; tt.ac_slab = 3L * d1.sub_r * d2.sub_r;
    tt.G1 = op.Gr[0]; tt.H1 = op.Hr[0]; tt.G2 = op.Gr[1]; tt.H2 = op.Hr[1];
    tt.out = c->out; tt.hout = c->d_hout;
    tt.beta_out = c->beta; tt.invd_out = c->invD;
    tt.peer_fail = vg_peer_fail(c, payload);
    for (int k = 0; k < 2; ++k) { tt.jit[k] = c->d[k].jitter; tt.status[k] = c->d[k].status; tt.rcounters[k] = c->d[k].counters2; }
#ifdef VGGP_DIAG
    tt.stamps = reinterpret_cast<unsigned long long*>(c->tAC + 3 * VG_THIN_MAXR * VG_THIN_MAXR);
#endif
    VG_HIP(vg_thin_tail_launch(&tt, st));
    VG_MARK(18);
    if (early) {           // E_r = W V1 -> leading rows of QtPrev: behind the tail, whose pinned result block the host polls
        vg_gemm_init(&g);
        add_er(&g);
        VG_HIP(vg_gemm_launch(&g, st));
    }
    return VGGP_OK;
}

// ---- subspace start (numerically rank-deficient G, e.g. RBF: rank ~20 of 128).  S = d.Fp is the previous basis after
// one Newton-Schulz step (partials ran with U = I), rows sorted by decreasing eigenvalue; its r leading rows V span
// the previous numerical range.  One step of subspace iteration, Z = V G, removes every null-space component
// exactly (G annihilates them); V1 = orth(Z); Rayleigh-Ritz on H = V1 G V1^T gives the r leading eigenpairs;
// the other rows are the previous ones projected off span(V1) (the next step's Newton-Schulz restores their
// orthonormality, 1e-5 off after the projection).  Q G Q^T is then diagonal up to a handful of elements
// (tools/studies/subspace_rbf_study.py: 1-3 rotations left instead of ~12000), which the eigensolver finds by scan.
int VgFinish::chain_subspace() {
    // G is read three times in this chain; in the fused step it is still split-K slabs, so the first launch also leaves a
    // reduced copy ("Id G" through the slab-summing GEMM) for the other two
    if (int rc = start_times_G(c->d[0].Fp, c->d[0].m, c->d[1].Fp, c->d[1].m, true)) return rc;      // S G (rows < r: Z = V G)
    VgGemmBatch g; VgRowQrJob qj[2];
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        const long r = d.sub_r;
        qj[k] = VgRowQrJob{d.TM, d.V1s, d.sub_r, d.m, d.Fp + r * d.m, d.E + r * d.m, (long)(d.m - r) * d.m};   // + E[r:] <- S[r:]
    }
    VG_HIP(vg_rowqr_launch(qj, 2, st, riders.next()));      // + rider: S = [B2;V2] Y
    VG_MARK(9);
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        const long r = d.sub_r;
        vg_gemm_add(&g, d.V1s, d.m, 1, op.Gr[k], d.m, 1, d.Zs, d.m, (int)r, d.m, d.m, 1, 0, op.grn[k], op.ghs[k]);        // T = V1 G (Z is spent)
        vg_gemm_add(&g, d.Fp + r * d.m, d.m, 1, d.V1s, 1, d.m, d.TH, (int)r, (int)(d.m - r), (int)r, d.m);           // P = S[r:] V1^T
    }
    VG_HIP(vg_gemm_launch(&g, st));
    VG_MARK(10);
    // The Ritz matrix H = T V1^T is formed by the Ritz launch's producer workgroups themselves (VgEigJob::Hl/Hr).  The
    // complement rows do not wait for the Ritz vectors: E[r:] = S[r:] - P V1 and, by linearity,
    // (E G)[r:] = (S G)[r:] - P T -- both ride in the Ritz launch as extra workgroups (with [C;C1;C2] in the fused step).
    VgGemmBatch gx; vg_gemm_init(&gx);
    if (const VgGemmBatch* cc = riders.next()) gx = *cc;
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        const long r = d.sub_r;
        vg_gemm_add(&gx, d.TH, r, 1, d.V1s, d.m, 1, d.E + r * d.m, d.m, (int)(d.m - r), d.m, (int)r, 1, 0, 1, 0, -1.0, 1);    // E[r:] -= P V1
        vg_gemm_add(&gx, d.TH, r, 1, d.Zs, d.m, 1, d.TM + r * d.m, d.m, (int)(d.m - r), d.m, (int)r, 1, 0, 1, 0, -1.0, 1);   // (S G)[r:] -= P T
    }
    VgEigJob sj[2] = {vg_ritz_job(c->d[0]), vg_ritz_job(c->d[1])};
    VG_HIP(vg_eigh_launch(sj, 2, st, &gx));                              // Ritz pairs (+ riders)
    VG_MARK(11);
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        const long r = d.sub_r;
        vg_gemm_add(&g, d.Ws, r, 1, d.V1s, d.m, 1, d.E, d.m, (int)r, d.m, (int)r);                                // E[:r] = W V1
        vg_gemm_add(&g, d.Ws, r, 1, d.Zs, d.m, 1, d.TM, d.m, (int)r, d.m, (int)r);                                 // (E G)[:r] = W T
    }
    VG_HIP(vg_gemm_launch(&g, st));
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(&g, d.TM, d.m, 1, d.E, 1, d.m, d.Gw, d.m, d.m, d.m, d.m); }
    VG_HIP(vg_gemm_launch(&g, st));
    return VGGP_OK;
}

// ---- Newton chain: full-rank Gram matrices whose warm start is too far off for the first-order refinement (or too large
// for the LDS eigensolver, m > 128).  From the start basis S (rows), Gw = S G S^T; then `newton` times
//     E_ij = g_ij / (g_jj - g_ii) (skew, elements above the threshold),  S <- (I + E + E^2 / 2) S,
//     one Newton-Schulz step (not after the last iteration),  Gw = S G S^T
// -- quadratic: |E| 1e-1 -> 1e-2 -> 1e-4 -> 1e-8 -- every product a batched MFMA GEMM over the whole chip, no single-workgroup
// sweep.  The last look at Gw (vg_newton_check_kernel) takes the eigenvalues from its diagonal and raises the retry bit when
// an off-diagonal element is still above the threshold or a rotation was too large (a crossing, a degenerate pair): the
// host then repeats the step on the regular chain.  Eigenpairs stay in the ORDER of the start basis (no sort).
// Leaves lam0, Qt and QtPrev itself: main_solve launches no eigensolver behind it.
int VgFinish::chain_newton() {
    const long m1 = c->desc.m1, m2 = c->desc.m2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const int newton = ch.newton;
    const double* Scur[2] = {ch.extrap ? d1.Fp : d1.QtPrev, ch.extrap ? d2.Fp : d2.QtPrev};
    auto buf = [&](int k, int i) { VgDim& d = c->d[k]; return i == 0 ? d.E : i == 1 ? d.X : d.F; };      // the three basis buffers in rotation
    if (int rc = start_times_G(Scur[0], d1.m, Scur[1], d2.m, true)) return rc;      // (reduced copies: G is read once per iteration, H in the rotation)
    VgGemmBatch g;
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(&g, d.TM, d.m, 1, Scur[k], 1, d.m, d.Gw, d.m, d.m, d.m, d.m); }
    VG_HIP(vg_gemm_launch(&g, st));
    VG_MARK(12);
    static const bool newton_null = getenv("VGGP_NO_NULL_SKIP") == nullptr;
    int bi = 0;
    for (int it = 0; it < newton; ++it) {
        VgRefineJob rj[2];
        for (int k = 0; k < 2; ++k) {
            VgDim& d = c->d[k];
            rj[k] = VgRefineJob{d.Gw, d.U, d.TH, d.m, VG_NEWTON_TOL};
            rj[k].emax = 0.3; rj[k].flag = d.counters2; rj[k].noise = VG_NEWTON_NOISE;
            // first iteration: the whole near-null cluster is left alone (its block is dominated by delta^2 lam_range until the
            // range-cluster rotations have been applied); afterwards only the exactly-null rows
            if (newton_null) { rj[k].lam_prev = d.lam0; rj[k].null_cut = it == 0 ? VG_NEWTON_CLUSTER : VG_NEWTON_NULL; }
        }
        VG_HIP(vg_refine_launch(rj, 2, st, riders.next()));                // E -> U, I + E -> TH  (+ riders: S, then [C;C1;C2])
        VG_MARK(9);
        vg_gemm_init(&g);
        for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(&g, d.U, d.m, 1, d.U, d.m, 1, d.TH, d.m, d.m, d.m, d.m, 1, 0, 1, 0, 0.5, 1); }   // TH += E^2 / 2
        VG_HIP(vg_gemm_launch(&g, st));
        double* Snew[2];
        vg_gemm_init(&g);
        for (int k = 0; k < 2; ++k) {
            VgDim& d = c->d[k];
            Snew[k] = buf(k, bi);
            vg_gemm_add(&g, d.TH, d.m, 1, Scur[k], d.m, 1, Snew[k], d.m, d.m, d.m, d.m);                 // (I + E + E^2/2) S
        }
        VG_HIP(vg_gemm_launch(&g, st));
        bi = (bi + 1) % 3;
        if (it + 1 < newton) {                                            // Newton-Schulz: S <- 1.5 S - 0.5 (S S^T) S
            double* Sns[2];
            vg_gemm_init(&g);
            for (int k = 0; k < 2; ++k) {
                VgDim& d = c->d[k];
                Sns[k] = buf(k, bi);
                vg_gemm_add(&g, Snew[k], d.m, 1, Snew[k], 1, d.m, d.TM, d.m, d.m, d.m, d.m);             // W = S S^T
                vg_gemm_add(&g, d.Id, d.m, 1, Snew[k], d.m, 1, Sns[k], d.m, d.m, d.m, d.m, 1, 0, 1, 0, 1.5, 0);
            }
            VG_HIP(vg_gemm_launch(&g, st));
            vg_gemm_init(&g);
            for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(&g, d.TM, d.m, 1, Snew[k], d.m, 1, Sns[k], d.m, d.m, d.m, d.m, 1, 0, 1, 0, -0.5, 1); }
            VG_HIP(vg_gemm_launch(&g, st));
            bi = (bi + 1) % 3;
            for (int k = 0; k < 2; ++k) Scur[k] = Sns[k];
        } else {
            for (int k = 0; k < 2; ++k) Scur[k] = Snew[k];
        }
        vg_gemm_init(&g);
        for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(&g, Scur[k], d.m, 1, op.Gr[k], d.m, 1, d.TM, d.m, d.m, d.m, d.m, 1, 0, op.grn[k], op.ghs[k]); }
        VG_HIP(vg_gemm_launch(&g, st));
        vg_gemm_init(&g);
        for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(&g, d.TM, d.m, 1, Scur[k], 1, d.m, d.Gw, d.m, d.m, d.m, d.m); }
        VG_HIP(vg_gemm_launch(&g, st));
    }
    VgNewtonCheckJob nj[2];
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        nj[k] = VgNewtonCheckJob{d.Gw, d.lam0, d.counters, d.status + 1, d.counters2, d.m, newton, VG_NEWTON_ACCEPT, VG_NEWTON_NOISE};
        if (newton_null) nj[k].null_cut = VG_NEWTON_NULL;
        VG_HIP(hipMemcpyAsync(d.Qt, Scur[k], sizeof(double) * d.m * d.m, hipMemcpyDeviceToDevice, st));
    }
    VG_HIP(vg_newton_check_launch(nj, 2, st));
    {   // converged: QtPrev2 <- QtPrev (the basis before last, for the next extrapolation), QtPrev <- the new basis; a miss leaves
        // both alone, and the host repeats the step on the regular chain from the same warm start
        const int* er[2] = {d1.status + 1, d2.status + 1};
        const double* sa[2] = {Scur[0], Scur[1]};
        double* da[2] = {d1.QtPrev, d2.QtPrev};
        const double* sb[2] = {d1.QtPrev, d2.QtPrev};
        double* db[2] = {d1.QtPrev2, d2.QtPrev2};
        const long nn[2] = {m1 * m1, m2 * m2};
        VG_HIP(vg_copy_if_launch(er, sa, da, sb, db, nn, 2, st));
    }
    VG_MARK(13);
    return riders.flush(st);                                              // (fewer than two iterations: what is still pending)
}

// ---- plain warm start: Gw = S G S^T from the previous basis (or the extrapolated one), optionally refined to first order.
int VgFinish::chain_refine() {
    const bool refine = kind == VG_CHAIN_REFINE;
    const double* S0[2];                                 // the start basis: the previous one, or the extrapolated one
    for (int k = 0; k < 2; ++k) S0[k] = kind != VG_CHAIN_PLAIN ? c->d[k].Fp : c->d[k].QtPrev;
    // (reduced copies for the later readers: G after a refinement, H in the rotation)
    if (int rc = start_times_G(S0[0], c->d[0].m, S0[1], c->d[1].m, refine)) return rc;
    VgGemmBatch g;
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(&g, d.TM, d.m, 1, S0[k], 1, d.m, d.Gw, d.m, d.m, d.m, d.m); }
    VG_HIP(vg_gemm_launch(&g, st));
    VG_MARK(12);
    // First-order refinement of the start basis (used while the previous step ended in the polish, i.e. on
    // well-separated spectra): S' = (I + E + E^2/2) S with E from Gw = S G S^T, then Gw' = S' G S'^T.  Five short
    // launches that replace the one dense Jacobi sweep (127 rounds) the polish still needed: the eigensolver
    // then only scans, and the replay workgroups apply the final polish.  A start that is too far off (|E| > 1e-3)
    // gets E = 0 from the kernel and the eigensolver proceeds as usual.
    if (!refine) return VGGP_OK;
    VgRefineJob rj[2];
    static const bool null_skip = getenv("VGGP_NO_NULL_SKIP") == nullptr;
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        rj[k] = VgRefineJob{d.Gw, d.U, d.TH, d.m, 0.0};
        if (null_skip) { rj[k].lam_prev = d.lam0; rj[k].null_cut = 1e-12; }
    }
    // E -> U, I + E -> TH   (+ rider: S = [B2;V2] Y, or [C;C1;C2] when S came out of the early projection)
    VG_HIP(vg_refine_launch(rj, 2, st, riders.next()));
    VG_MARK(9);
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        vg_gemm_add(&g, d.TH, d.m, 1, S0[k], d.m, 1, d.E, d.m, d.m, d.m, d.m);    // (I + E) S -> E
        vg_gemm_add(&g, d.U, d.m, 1, d.U, d.m, 1, d.X, d.m, d.m, d.m, d.m);        // E E -> X
    }
    VG_HIP(vg_gemm_launch(&g, st));
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(&g, d.X, d.m, 1, S0[k], d.m, 1, d.E, d.m, d.m, d.m, d.m, 1, 0, 1, 0, 0.5, 1); }   // += E^2 S / 2
    VG_HIP(vg_gemm_launch(&g, st));
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(&g, d.E, d.m, 1, op.Gr[k], d.m, 1, d.TM, d.m, d.m, d.m, d.m, 1, 0, op.grn[k], op.ghs[k]); }
    VG_HIP(vg_gemm_launch(&g, st));
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(&g, d.TM, d.m, 1, d.E, 1, d.m, d.Gw, d.m, d.m, d.m, d.m); }
    VG_HIP(vg_gemm_launch(&g, st));
    return VGGP_OK;
}

// The main eigensolve (LDS Jacobi + replay, eigh.hip) from whatever start the chain left -- none after the Newton chain, which
// has left lam0, Qt, QtPrev itself -- then the riders no launch took, and the join of the projection branch.
int VgFinish::main_solve() {
    hipStream_t sx = vg_side(c, st);
    VG_MARK(12);
    if (kind != VG_CHAIN_NEWTON) {
        const bool warm = kind != VG_CHAIN_COLD, subspace = kind == VG_CHAIN_SUBSPACE, refine = kind == VG_CHAIN_REFINE;
        VgEigJob ej[2];
        for (int k = 0; k < 2; ++k) {
            VgDim& d = c->d[k];
            const double* start = !warm ? nullptr : (refine || subspace) ? d.E : (kind == VG_CHAIN_EXTRAP ? d.Fp : d.QtPrev);
            ej[k] = VgEigJob{warm ? d.Gw : op.G0[k], d.lam0, d.Qt, start, d.gwork, d.rotlog, d.roundlog,
                             d.counters, d.m, d.max_rounds, (long)vg_eigh_log_bytes(d.m),
                             (c->desc.flags & VGGP_FLAG_BLOCK_JACOBI) ? 1 : 0};
            ej[k].Qt2 = d.QtPrev;        // the replay workgroups leave the new basis in both places (next warm start, q(v))
            ej[k].perm = d.perm;
            ej[k].cp_src = d.QtPrev; ej[k].cp_dst = d.QtPrev2;      // the basis before last, for the next extrapolation
            ej[k].err = d.status + 1;      // replay timeout flag (folded into the step status by the final kernel)
            ej[k].polish0 = refine ? 1 : 0;
            ej[k].sparse_first = subspace ? 1 : 0;
            ej[k].null_from = subspace ? d.sub_r : 0;
        }
        // (counters were zeroed by the clear kernel at the start of the step)
        // riders of the main solve: whichever of the two projection launches is next (S when no earlier launch of the chain took
        // it; [C;C1;C2] when the refinement launch carried S); what is still pending afterwards runs as a launch of its own
        VG_HIP(vg_eigh_launch(ej, 2, st, riders.next()));
        VG_MARK(13);
    }
    if (int rc = riders.flush(st)) return rc;
    c->ride_pending = false;
    if (ch.from_slabs) VG_JOIN_WAIT(1);          // fused step: the projection branch (S, C slabs) ran beside the eigensolver chain
    return VGGP_OK;
}

// Stages 8-10: rotation into the eigenbasis, D-stage, the four beta Gram products, final reduction.
int VgFinish::rotate_and_reduce() {
    const long m1 = c->desc.m1, m2 = c->desc.m2;
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    VgGemmBatch g;
    // 8. rotate into the eigenbasis: first the right factors ...
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        vg_gemm_add(&g, d.Mk, d.m, 1, d.Qt, 1, d.m, d.TM, d.m, d.m, d.m, d.m);      // Mk Q
        const int ih = vg_gemm_add(&g, op.Hr[k], d.m, 1, d.Qt, 1, d.m, d.TH, d.m, d.m, d.m, d.m);     // H0 Q
        g.p[ih].a_nslab = op.hrn[k]; g.p[ih].a_slab = op.ghs[k];
    }
    const int ic = vg_gemm_add(&g, op.C3, m2, 1, d2.Qt, 1, m2, c->T3, (int)m2, (int)(3 * m1), (int)m2, (int)m2);   // [C;C1;C2] Q2
    g.p[ic].a_nslab = op.ccn; g.p[ic].a_slab = op.ccs;
    // Prediction of the NEXT step's start basis, riding in the three GEMM launches of this tail (and one of the next step's
    // head): the basis moved from Q(t-1) to Q(t) by the rotation U = Q(t) Q(t-1)^T; applying it once more predicts the next
    // basis, Qpred = U Q(t) (rows = eigenvectors).  A product of three bases triples their departure from orthogonality and
    // feeds it back into the next bases -- it would grow ~2.4x per step -- so one Newton-Schulz step follows:
    // Q' = 1.5 Qpred - 0.5 (Qpred Qpred^T) Qpred.  Here: U; next launch: Ep = Qpred, Fp = 1.5 Qpred; the beta-Gram launch:
    // Wp = Qpred Qpred^T; the next step's projection launch: Fp += -0.5 Wp Ep.  The subspace start is fed the previous basis
    // itself (U = I: only the Newton-Schulz clean-up), see vg_sub_ident().  (The eigensolver's replay workgroups have
    // already left Q(t) in QtPrev and Q(t-1) in QtPrev2.)
    const bool predict = c->desc.warm_start && !(c->desc.flags & VGGP_FLAG_BLOCK_JACOBI);
    const bool pred_ident = c->sub_mode && vg_sub_ident();
    if (predict && !pred_ident)
        for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(&g, d.QtPrev, d.m, 1, d.QtPrev2, 1, d.m, d.U, d.m, d.m, d.m, d.m); }
    VG_HIP(vg_gemm_launch(&g, st));
    VG_MARK(14);
    //    ... then the left factors
    vg_gemm_init(&g);
    for (int k = 0; k < 2; ++k) {
        VgDim& d = c->d[k];
        vg_gemm_add(&g, d.Qt, d.m, 1, d.TM, d.m, 1, d.E, d.m, d.m, d.m, d.m);       // E = Q^T Mk Q
        vg_gemm_add(&g, d.Qt, d.m, 1, d.TH, d.m, 1, d.F, d.m, d.m, d.m, d.m);       // F = Q^T H0 Q
    }
    for (int q = 0; q < 3; ++q)
        vg_gemm_add(&g, d1.Qt, m1, 1, c->T3 + q * m1 * m2, m2, 1, c->P3 + q * m1 * m2, (int)m2, (int)m1, (int)m2, (int)m1);
    if (predict)
        for (int k = 0; k < 2; ++k) {
            VgDim& d = c->d[k];
            const double* Uk = pred_ident ? d.Id : d.U;
            vg_gemm_add(&g, Uk, d.m, 1, d.QtPrev, d.m, 1, d.Ep, d.m, d.m, d.m, d.m);
            vg_gemm_add(&g, Uk, d.m, 1, d.QtPrev, d.m, 1, d.Fp, d.m, d.m, d.m, d.m, 1, 0, 1, 0, 1.5, 0);
        }
    VG_HIP(vg_gemm_launch(&g, st));
    VG_MARK(15);

    // 9. D-stage, the four beta Gram matrices, final reduction
    VgMspace ms;
    ms.theta = c->theta; ms.lam1 = d1.lam0; ms.lam2 = d2.lam0; ms.P3 = c->P3;
    ms.E1 = d1.E; ms.F1 = d1.F; ms.E2 = d2.E; ms.F2 = d2.F;
    ms.beta = c->beta; ms.bl2 = c->bl2; ms.bl1 = c->bl1; ms.invD = c->invD;
    ms.rowpart = c->rowpart; ms.r1 = c->r1; ms.r1l = c->r1l; ms.out = c->out;
    ms.r2 = c->r2; ms.r2l = c->r2l; ms.dotp = c->dotpart; ms.ol = c->ol;
    ms.m1 = (int)m1; ms.m2 = (int)m2; ms.n_total = (double)c->desc.n_total; ms.yy = yy_total;
    ms.ticket = c->ticket; ms.hout = c->d_hout;
    ms.peer_fail = vg_peer_fail(c, payload);
    for (int k = 0; k < 2; ++k) { ms.jit[k] = c->d[k].jitter; ms.status[k] = c->d[k].status; ms.counters[k] = c->d[k].counters; }
    VG_HIP(vg_dstage_launch(&ms, st));
    VG_MARK(16);
    vg_gemm_init(&g);
    // The four dot products of the gradient, sum(E1 o beta beta^T), sum(F1 o (beta lam2) beta^T), sum(E2 o beta^T beta),
    // sum(F2 o (lam1 beta)^T beta), never materialise the m x m Gram matrices: sum_ij E_ij (beta beta^T)_ij = sum((E^T beta) o beta),
    // so each is an m1 x m2 product whose tiles are multiplied by beta and summed in the GEMM's reduction epilogue (one word per
    // tile, fixed order).  The column sums [r2; r2l] = [1; s1 lam1] (1/D) ride along as a 2-row product.
    {
        const int idot[4] = {
            vg_gemm_add(&g, d1.E, 1, m1, c->beta, m2, 1, nullptr, (int)m2, (int)m1, (int)m2, (int)m1),     // E1^T beta
            vg_gemm_add(&g, d1.F, 1, m1, c->bl2, m2, 1, nullptr, (int)m2, (int)m1, (int)m2, (int)m1),      // F1^T (beta lam2)
            vg_gemm_add(&g, c->beta, m2, 1, d2.E, m2, 1, nullptr, (int)m2, (int)m1, (int)m2, (int)m2),     // beta E2
            vg_gemm_add(&g, c->bl1, m2, 1, d2.F, m2, 1, nullptr, (int)m2, (int)m1, (int)m2, (int)m2)};     // (lam1 beta) F2
        for (int q = 0; q < 4; ++q) { g.p[idot[q]].dotw = c->beta; g.p[idot[q]].dotw_ld = (int)m2; g.p[idot[q]].dot_out = c->dotpart + 64 * q; }
        vg_gemm_add(&g, c->ol, m1, 1, c->invD, m2, 1, c->r2, (int)m2, 2, (int)m2, (int)m1);
    }
    if (predict)                                                                          // W = Qpred Qpred^T
        for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; vg_gemm_add(&g, d.Ep, d.m, 1, d.Ep, 1, d.m, d.Wp, d.m, d.m, d.m, d.m); }
    VG_HIP(vg_gemm_launch(&g, st));
    VG_MARK(17);
    VG_HIP(vg_final_launch(&ms, st));
    VG_MARK(18);

    // 10. nothing to copy: the replay workgroups already left the new basis in QtPrev (next warm start, q(v), posterior)
    //     and the last workgroup of the final reduction wrote results + diagnostics into the pinned host block
    return VGGP_OK;
}

// The finish half: eigendecompositions of G1, G2 (optionally warm-started from the previous step's basis), then the tail.
static int finish_enqueue(vggp_ctx* c, const double* payload, double yy_total, hipStream_t st, const VgChain& ch) {
    // inside a fused step the factor kernel already refreshed the device copy of the hyper-parameters
    if (ch.copy_theta) VG_HIP(hipMemcpyAsync(c->theta, c->h_theta, 6 * sizeof(double), hipMemcpyHostToDevice, st));
    // riders: the projection launches were deferred to this chain (vg_partials_enqueue)
    VgFinish f{c, st, payload, yy_total, ch, vg_chain_kind(ch), VgStepOperands(c, payload, ch.from_slabs), VgRiders(c, ch.from_slabs)};
    VG_MARK(-1);                  // (re)start the stage clock: the caller's all-reduce sits between the two halves
    int rc = VGGP_OK;
    switch (f.kind) {
    case VG_CHAIN_COLD: break;
    case VG_CHAIN_THIN: return f.chain_thin();
    case VG_CHAIN_SUBSPACE: rc = f.chain_subspace(); break;
    case VG_CHAIN_NEWTON: rc = f.chain_newton(); break;
    case VG_CHAIN_REFINE: case VG_CHAIN_EXTRAP: case VG_CHAIN_PLAIN: rc = f.chain_refine(); break;
    }
    if (!rc) rc = f.main_solve();
    return rc ? rc : f.rotate_and_reduce();
}

// ---- HIP-graph cache: the launch sequence of a step is fixed for a plan, so it is captured once per
// (variant, data pointers) and replayed; hyper-parameters travel through the pinned theta buffer.
enum { VG_G_PARTIALS = 0, VG_G_PARTIALS_X, VG_G_FINISH_COLD, VG_G_FINISH_WARM, VG_G_FINISH_WARM_X, VG_G_STEP_COLD, VG_G_STEP_WARM,
       VG_G_STEP_WARM_X, VG_G_FINISH_WARM_XR, VG_G_STEP_WARM_XR, VG_G_FINISH_WARM_S, VG_G_STEP_WARM_S, VG_G_FINISH_WARM_T, VG_G_STEP_WARM_T,
       VG_G_FINISH_WARM_N, VG_G_STEP_WARM_N, VG_G_PARTIALS_E, VG_G_FINISH_WARM_TE, VG_G_STEP_COLD_T, VG_G_PARTIALS_XE, VG_G_COUNT };
static_assert(VG_G_COUNT <= 20, "vggp_ctx::gexec");
// _T: thin chain (subspace start without a complement basis, thin.hip); _N: Newton chain
// _S: subspace start (see chain_subspace)
// _X: warm start from the extrapolated basis; _XR: ... refined to first order before the eigensolver (see chain_refine)
// the slot of a finish half (fused = false) or of a fused single-rank step that ends in it
static int vg_graph_slot(const VgChain& ch, bool fused) {
    switch (vg_chain_kind(ch)) {
    case VG_CHAIN_COLD: return fused ? VG_G_STEP_COLD : VG_G_FINISH_COLD;
    case VG_CHAIN_THIN: return fused ? VG_G_STEP_WARM_T : (ch.thin_early ? VG_G_FINISH_WARM_TE : VG_G_FINISH_WARM_T);
    case VG_CHAIN_NEWTON: return fused ? VG_G_STEP_WARM_N : VG_G_FINISH_WARM_N;
    case VG_CHAIN_SUBSPACE: return fused ? VG_G_STEP_WARM_S : VG_G_FINISH_WARM_S;
    case VG_CHAIN_REFINE: return fused ? VG_G_STEP_WARM_XR : VG_G_FINISH_WARM_XR;
    case VG_CHAIN_EXTRAP: return fused ? VG_G_STEP_WARM_X : VG_G_FINISH_WARM_X;
    case VG_CHAIN_PLAIN: break;
    }
    return fused ? VG_G_STEP_WARM : VG_G_FINISH_WARM;
}

// destroy a captured graph and clear its key (the stream may still be finishing it: vg_quiesce first)
static void graph_drop(vggp_ctx* c, int slot) {
    if (c->gexec[slot]) { (void)vg_quiesce(c); (void)hipGraphExecDestroy(c->gexec[slot]); c->gexec[slot] = nullptr; }
    c->gkey[slot] = VgGraphKey();
}
void vg_graphs_clear(vggp_ctx* c) {
    (void)vg_quiesce(c);
    for (int i = 0; i < VG_G_COUNT; ++i) graph_drop(c, i);
}

template <typename F>
static int run_graph(vggp_ctx* c, int which, const VgGraphKey& key, hipStream_t st, F enqueue, bool bypass = false) {
    if (!c->use_graph || c->prof || bypass) return enqueue();
    if (!c->gexec[which] || !(c->gkey[which] == key)) {
        graph_drop(c, which);
        VG_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue();
        hipGraph_t graph = nullptr;
        const hipError_t e = hipStreamEndCapture(st, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess) { vg_set_error("hipStreamEndCapture -> %s", hipGetErrorString(e)); return VGGP_EHIP; }
        const hipError_t ei = hipGraphInstantiate(&c->gexec[which], graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ei != hipSuccess) { c->gexec[which] = nullptr; vg_set_error("hipGraphInstantiate -> %s", hipGetErrorString(ei)); return VGGP_EHIP; }
        c->gkey[which] = key;
    }
    VG_HIP(hipGraphLaunch(c->gexec[which], st));
    return VGGP_OK;
}

// ---- start policy ---------------------------------------------------------------------------------------------------------------
// the stored bases are not to be trusted (or not to be used): the next step starts cold
static void vg_drop_warm(vggp_ctx* c) { c->warm_run = 0; for (int k = 0; k < 2; ++k) c->d[k].have_prev = c->d[k].have_prev2 = false; }

// extrapolated warm start: needs the bases of the last two steps (scalar Jacobi variant; VGGP_NO_EXTRAP=1 switches it off)
static bool vg_refine(const vggp_ctx* c, bool extrap) {
    static const bool off = getenv("VGGP_NO_REFINE") != nullptr;
    return !off && extrap && c->refine_next;
}

static bool vg_extrapolate(const vggp_ctx* c) {
    static const bool off = getenv("VGGP_NO_EXTRAP") != nullptr;
    return !off && c->desc.warm_start && !(c->desc.flags & VGGP_FLAG_BLOCK_JACOBI) && c->d[0].have_prev && c->d[1].have_prev &&
           c->d[0].have_prev2 && c->d[1].have_prev2;
}

// The thin chain needs: ranks known and small, the leading rows of QtPrev valid, the step's payload owned by the context (its
// read-outs re-run the finish half cold on the resident G, H, C), and no caller that wanted the full m-space state of a warm step.
static bool vg_thin_ok(const vggp_ctx* c, bool own_payload) {
    static const bool off = getenv("VGGP_NO_THIN") != nullptr;
    if (off || c->thin_off || c->thin_block > 0 || !own_payload || !c->desc.warm_start || (c->desc.flags & VGGP_FLAG_BLOCK_JACOBI) || !c->sub_next) return false;
    for (int k = 0; k < 2; ++k) {
        const VgDim& d = c->d[k];
        if (!d.have_prev || !d.tMV || d.sub_r < 1 || d.sub_r > VG_THIN_MAXR || d.sub_r > d.thin_rows) return false;
    }
    return true;
}
// warm start possible?  After a thin step QtPrev holds range rows only: a step that cannot run thin then starts cold.
static bool vg_warm(vggp_ctx* c, bool own_payload) {
    bool warm = c->desc.warm_start && c->d[0].have_prev && c->d[1].have_prev;
    if (warm && (c->d[0].thin_rows < c->d[0].m || c->d[1].thin_rows < c->d[1].m) && !vg_thin_ok(c, own_payload)) {
        vg_drop_warm(c);
        warm = false;
    }
    return warm;
}
// start-basis strategy of this step (out->warm .. out->newton); switching the subspace mode on puts the identity into U (the
// partials then run a plain Newton-Schulz clean-up of QtPrev through the extrapolation products) and drops stale _S graphs when
// the ranks moved
static void vg_start_prepare(vggp_ctx* c, bool own_payload, VgChain* out) {
    const bool warm = out->warm = vg_warm(c, own_payload);
    out->thin = warm && vg_thin_ok(c, own_payload);
    out->extrap = !out->thin && vg_extrapolate(c);
    // (the full subspace chain -- complement basis, sparse-first main solve -- lives in the LDS eigensolver body: m <= 128)
    const bool lds_sized = c->d[0].m <= 128 && c->d[1].m <= 128;
    out->subspace = out->thin || (lds_sized && warm && out->extrap && c->sub_next && c->d[0].sub_r > 0 && c->d[1].sub_r > 0);
    // Newton chain: full-rank warm starts beyond the LDS eigensolver (m > 128) or where the last warm step still needed Jacobi rounds
    {
        static const bool off = getenv("VGGP_NO_NEWTON_CHAIN") != nullptr;
        static const char* ite = getenv("VGGP_NEWTON_ITERS");
        const bool big = c->d[0].m > 128 || c->d[1].m > 128;
        // (below m_d = 96 a sweep of the LDS solver is cheaper than an iteration of this chain -- seven launches whatever the size)
        const bool roomy = c->d[0].m >= 96 && c->d[1].m >= 96;
        const bool want = warm && !out->subspace && out->extrap && !off && c->newton_block == 0 && (big || (c->newton_next && roomy)) &&
                          !(c->desc.flags & VGGP_FLAG_BLOCK_JACOBI) && c->d[0].m >= 8 && c->d[1].m >= 8;
        out->newton = want ? (ite ? atoi(ite) : c->newton_iters) : 0;
        if (c->newton_block > 0) --c->newton_block;
    }
    out->refine = warm && !out->subspace && !out->newton && vg_refine(c, out->extrap);
    c->sub_mode = out->subspace;
    if (out->subspace && (c->sub_r_cap[0] != c->d[0].sub_r || c->sub_r_cap[1] != c->d[1].sub_r)) {
        for (int v : {(int)VG_G_FINISH_WARM_S, (int)VG_G_STEP_WARM_S, (int)VG_G_FINISH_WARM_T, (int)VG_G_STEP_WARM_T, (int)VG_G_FINISH_WARM_TE})
            graph_drop(c, v);
        c->sub_r_cap[0] = c->d[0].sub_r; c->sub_r_cap[1] = c->d[1].sub_r;
    }
    if (out->newton && out->newton != c->newton_cap) {          // the _N graphs hold a fixed number of iterations
        for (int v : {(int)VG_G_FINISH_WARM_N, (int)VG_G_STEP_WARM_N}) graph_drop(c, v);
        c->newton_cap = out->newton;
    }
    c->cur_thin = out->thin;
    c->cur_extrap = out->extrap;
    c->cur_newton = out->newton;
    c->cur_r[0] = c->d[0].sub_r; c->cur_r[1] = c->d[1].sub_r;
}

static int set_theta(vggp_ctx* c, const double theta[5]) {
    for (int i = 0; i < 5; ++i) {
        VG_REQUIRE(theta[i] > 0.0 && std::isfinite(theta[i]), "theta[%d]=%g must be positive and finite", i, theta[i]);
        c->h_theta[i] = theta[i];
    }
    c->h_theta[5] = (double)(++c->seq);        // travels through the step and comes back in the pinned result block
    return VGGP_OK;
}

// host side of the end of a step: the only synchronisation, then unpack the pinned block
// Completion of a single-rank step WITHOUT a HIP call: the last kernel of the step writes the 128-byte result block into pinned
// host memory as one burst whose last word is the step's sequence number, so the host polls that word.  hipStreamSynchronize
// returns only after the end-of-graph bookkeeping of the runtime (measured: ~8 us later); the stream itself keeps the order of
// whatever is enqueued next.  Anything that must not overlap with the tail of the graph (destroying a graph exec, re-planning)
// calls vg_quiesce first.  Falls back to the real synchronisation after 20 ms (a fault would otherwise spin for ever).
int vg_quiesce(vggp_ctx* c) {
    if (c->poll_stream_valid) { c->poll_stream_valid = false; VG_HIP(hipStreamSynchronize(c->poll_stream)); }
    return VGGP_OK;
}
static int vg_wait_step(vggp_ctx* c, hipStream_t st) {
    static const bool nopoll = getenv("VGGP_NO_POLL") != nullptr;
    const volatile double* seq = &c->h_out->seq;
    const double want = c->h_theta[5];
    if (nopoll || c->prof || (c->n_ranks > 1 && !c->comm && !c->cb)) { c->poll_stream_valid = false; return vg_comm_wait(c, st); }
    if (c->comm && !c->cb) {
        // RCCL transport: the same word, polled together with the communicator's health (a dead peer is an error, not a hang)
        const int wrc = vg_comm_wait(c, st, seq, want);
        c->poll_stream = st; c->poll_stream_valid = (wrc == VGGP_OK);
        return wrc;
    }
    timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (long spin = 0;; ++spin) {
        if (*seq == want) {
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            c->poll_stream = st; c->poll_stream_valid = true;
            return VGGP_OK;
        }
        __builtin_ia32_pause();
        if ((spin & 4095) == 4095) {
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec) > 0.02) break;
        }
    }
    c->poll_stream_valid = false;
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

// status of the step in the pinned result block: a factor's, else an eigensolver's
static int vg_step_status(const vggp_ctx* c) {
    int status = 0;
    for (int k = 0; k < 2; ++k) {
        if (c->h_out->status[k]) status = c->h_out->status[k];
        else if (c->h_out->counters[k][2]) status = c->h_out->counters[k][2];
    }
    return status;
}
static int finish_collect(vggp_ctx* c, double* elbo_out, double grad_out[5], vggp_info* info, hipStream_t st) {
    const int wrc = vg_wait_step(c, st);              // (single rank: polls the pinned result block; multi-rank: vg_comm_wait)
    if (wrc) { vg_drop_warm(c); c->have_step = false; return wrc; }
    c->pred_consumed = false;             // the tail of this step left a fresh prediction in Ep / Fp / Wp
    c->acc_valid = false;
    if (c->prof && c->nev > 1) {
        for (int i = 1; i < c->nev; ++i) {
            const int id = c->ev_stage[i];
            float ms = 0.f;
            if (id >= 0 && id < VGGP_NSTAGE && hipEventElapsedTime(&ms, c->ev[i - 1], c->ev[i]) == hipSuccess) c->prof_ms[id] += ms;
        }
        c->prof_steps++;
    }
    c->nev = 0;
    if (c->h_out->seq != c->h_theta[5]) {       // the block was not written by THIS step (a launch was lost or reordered)
        vg_set_error("step %.0f: the result block carries sequence number %.0f (stale results)", c->h_theta[5], c->h_out->seq);
        vg_drop_warm(c); c->have_step = false;
        return VGGP_ESTATE;
    }
    if (c->h_out->out[6] != 0.0) {          // the peer-failure word of the all-reduced payload: the sums miss a rank's contribution
        vg_set_error("rank %d / %d: %.0f rank(s) of the job failed their half of this step; the result is discarded", c->rank,
                     c->n_ranks, c->h_out->out[6]);
        vg_drop_warm(c); c->have_step = false;
        return VGGP_ERCCL;
    }
    *elbo_out = c->h_out->out[0];
    for (int i = 0; i < 5; ++i) grad_out[i] = c->h_out->out[1 + i];
    const int status = vg_step_status(c);
    if (info) {
        info->jitter1 = c->h_out->jitter[0]; info->jitter2 = c->h_out->jitter[1];
        info->sweeps1 = c->h_out->counters[0][1] & 0xff; info->sweeps2 = c->h_out->counters[1][1] & 0xff;
        info->rounds1 = c->h_out->counters[0][0]; info->rounds2 = c->h_out->counters[1][0];
        info->status = status;
        info->polished = ((c->h_out->counters[0][3] >> 28) & 1) | (((c->h_out->counters[1][3] >> 28) & 1) << 1);
    }
    // numerical ranks -> subspace start for the next step (rank-deficient Gram matrices only; hysteresis keeps the graph stable)
    {
        static const bool off = getenv("VGGP_NO_SUBSPACE") != nullptr;
        bool ok = !status && !off && c->desc.warm_start && !(c->desc.flags & VGGP_FLAG_BLOCK_JACOBI);
        for (int k = 0; k < 2; ++k) {
            VgDim& d = c->d[k];
            const int rank = (c->h_out->counters[k][1] >> 8) & 0x1ff;
            int want = 0;
            static const bool relax = getenv("VGGP_NO_SUB_RELAX") == nullptr;
            if (d.Zs && rank >= 1 && 3 * rank <= d.m) {
                // numerical rank (eigenvalues above 1e-14 of the largest) + 3 rows, rounded up to an even count (odd counts run a padded,
                // slower path: 21 rows 0.207 ms, 22 rows 0.190): at 1024^2, m_d = 128 that is 20 rows (rank 17), 22 when the rank reaches 18; the earlier rule (rank + 4 rounded to 8 = 24 rows) cost 11 us per step in the row QR, the
                // Ritz solve and the r-row products.  An RBF spectrum drops by ~6x per index and a fit-loop step moves it by a few
                // per cent, so the margin is consumed one row per many steps -- and the tail kernel's miss check catches the rest.
                // VGGP_SUB_MARGIN8=1: the earlier rule.
                static const bool m8 = getenv("VGGP_SUB_MARGIN8") != nullptr;
                want = m8 ? ((rank + 4 + 7) / 8) * 8 : ((rank + 3 + 1) / 2) * 2;
                if (want < 16) want = 16;
                if (want > 64 || 2 * want > d.m) want = 0;
            } else if (relax && d.Zs && rank >= 1 && d.m <= 64 && rank + 2 <= d.m - 8) {
                // small inducing counts (m_d = 32: numerical rank ~22): not "rank-deficient" by the rule above, but the near-null
                // cluster is what costs the warm Jacobi its 3-5 sweeps -- deflating the range part still pays as long as the Ritz
                // problem fits the Newton start (<= 48) and some rows are left over (195 -> 171 us at m_d = 32, 253 -> 203 at 48)
                want = ((rank + 2 + 3) / 4) * 4;
                if (want > d.m - 8) want = d.m - 8;
                if (want < 8 || want > 48) want = 0;
            }
            if (d.m > 128 && want > VG_THIN_MAXR) want = 0;      // beyond one LDS-resident matrix only the thin chain exists
            if (want == 0) d.sub_r = 0;
            else if (want > d.sub_r || want < d.sub_r - 8) d.sub_r = want;
            ok = ok && d.sub_r > 0;
        }
        c->sub_next = ok;
    }
    // refine the next start only where it can replace the last sweep: both dimensions polished after at most one sweep
    c->refine_next = !status && ((c->h_out->counters[0][3] >> 28) & 1) && ((c->h_out->counters[1][3] >> 28) & 1) &&
                     (c->h_out->counters[0][1] & 0xff) <= 1 && (c->h_out->counters[1][1] & 0xff) <= 1;
    if (status == VG_ESUBMISS && c->cur_newton) {
        // the Newton chain missed: it has not touched the stored bases -- repeat on the regular chain from the same warm start
        static const bool dbg = getenv("VGGP_NEWTON_DBG") != nullptr;
        if (dbg)
            fprintf(stderr, "[vggp] step %ld: Newton chain (%d iterations) missed: dim1 flags %d, 10 log10(offdiag / thr) = %d; dim2 flags %d, %d\n",
                    c->seq, c->cur_newton, c->h_out->counters[0][3] & 0xff, (c->h_out->counters[0][3] >> 8) - 100,
                    c->h_out->counters[1][3] & 0xff, (c->h_out->counters[1][3] >> 8) - 100);
        // (beyond the LDS eigensolver the regular chain is the global-memory Jacobi -- 18 ms per step at m = 256: there the chain is
        //  tried again as soon as BOTH stored bases come from the regular chain -- the eigensolver sorts, the Newton chain keeps its
        //  start order, and a pair of bases from different chains extrapolates badly; otherwise it rests for 16 steps)
        c->newton_block = (c->d[0].m > 128 || c->d[1].m > 128) ? 2 : 16; c->newton_next = false;
        if (c->newton_iters < 5) ++c->newton_iters;
        c->newton_ok_run = 0;
        c->have_step = false;
        return VG_ESUBMISS;
    }
    if (status) { vg_drop_warm(c); c->have_step = false; }      // the bases written by this step are not trustworthy: the next step starts cold
    if (status == VG_ESUBMISS) {            // (the caller repeats the step; the warm start was reset above)
        c->sub_next = false;
        if (c->cur_thin) c->thin_block = 32;      // the directions the thin chain leaves out mattered: full chains for a while
        return VG_ESUBMISS;
    }
    if (status == VGGP_ENOTPD) { vg_set_error("a Kuu factor is not positive definite after jitter 1e-6"); return VGGP_ENOTPD; }
    if (status == VGGP_ENOCONV) { vg_set_error("Jacobi eigensolver did not converge"); return VGGP_ENOCONV; }
    for (int k = 0; k < 2; ++k) {
        c->d[k].have_prev2 = c->d[k].have_prev;                // QtPrev2 <- previous basis (copied by the replay workgroups)
        c->d[k].have_prev = true;                              // QtPrev holds this step's basis
        c->d[k].thin_rows = c->cur_thin ? c->cur_r[k] : c->d[k].m;      // ... all of it, or the range rows of a thin step
    }
    c->last_thin = c->cur_thin;
    if (c->thin_block > 0) --c->thin_block;
    // (the Newton chain keeps the eigenpairs in the order of its start basis, the eigensolver sorts: after a crossing the two stored
    //  bases of a chain switch may not correspond row by row -- the extrapolated start is then poor, the chain that receives it
    //  notices: the regular one sweeps, the Newton chain misses and the step is repeated)
    c->last_newton = c->cur_newton > 0;
    if (c->cur_newton > 0 && ++c->newton_ok_run >= 64) {          // a long run without a miss: try one iteration less again
        c->newton_ok_run = 0;
        if (c->newton_iters > 3) --c->newton_iters;
    }
    // next step: stay on the Newton chain while it works; move to it when a warm step of the regular chain still needed rounds
    {
        const bool polished = ((c->h_out->counters[0][3] >> 28) & 1) && ((c->h_out->counters[1][3] >> 28) & 1);
        c->newton_next = c->cur_newton > 0 ||
                         (c->last_warm && c->cur_extrap && !c->cur_thin && !polished && (c->h_out->counters[0][0] + c->h_out->counters[1][0]) > 0) ||
                         // ... or ended in the polish only after more than a sweep and a half of rotations (B1 hats on a padded mesh: two
                         // dense sweeps per step, then the polish; an occasional single sweep of a Matern-3/2 step does not count)
                         // (m_d >= 96 only: an iteration of the chain is seven launches whatever the size, a sweep of a small matrix is cheap --
                         //  127 Fourier features gain, 63 lose)
                         (c->last_warm && c->cur_extrap && !c->cur_thin && c->d[0].m >= 96 && c->d[1].m >= 96 &&
                          (2 * c->h_out->counters[0][0] >= 3 * c->d[0].m || 2 * c->h_out->counters[1][0] >= 3 * c->d[1].m));
    }
    if (++c->warm_run >= 512) vg_drop_warm(c);                 // periodic cold restart: bounds the drift of orthogonality
    c->have_step = true;
    c->last_kind = VG_LAST_FULL;
    return VGGP_OK;
}

extern "C" int vggp_elbo_partials(vggp_ctx* c, const double* Y, const double theta[5], double* payload, void* stream) {
    VG_NOT_PAIRED(c, "vggp_elbo_partials");
    if (!c || !c->planned) { vg_set_error("vggp_elbo_partials: context not planned"); return VGGP_ESTATE; }
    VG_REQUIRE(Y && theta && payload, "vggp_elbo_partials: null argument");
    c->have_iter = false;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    int rc = set_theta(c, theta);
    if (rc) return rc;
    c->nev = 0;
    const VgGraphKey key{Y, payload, 0.0};
    VgChain ch;
    vg_start_prepare(c, /*own_payload=*/false, &ch);
    VgPartials po;
    // the Newton-Schulz step of the predicted basis accumulates into Fp: exactly once per prediction (a repeated partials
    // call without a finish in between runs un-captured without it)
    po.extrap = ch.extrap; po.apply_ns = ch.extrap && !c->pred_consumed;
    rc = run_graph(c, ch.extrap ? VG_G_PARTIALS_X : VG_G_PARTIALS, key, st, [&] { return vg_partials_enqueue(c, Y, payload, st, po); },
                   ch.extrap && !po.apply_ns);
    if (rc) return rc;
    if (ch.extrap) c->pred_consumed = true;
    c->have_partials = true;
    return VGGP_OK;
}

static int elbo_finish_once(vggp_ctx* c, const double* payload, double yy_total, const double theta[5],
                            double* elbo_out, double grad_out[5], vggp_info* info, void* stream) {
    if (!c || !c->planned || !c->have_partials) { vg_set_error("vggp_elbo_finish: call vggp_elbo_partials first"); return VGGP_ESTATE; }
    VG_REQUIRE(payload && theta && elbo_out && grad_out, "vggp_elbo_finish: null argument");
    c->have_iter = false;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    int rc = set_theta(c, theta);
    if (rc) return rc;
    const VgGraphKey key{nullptr, payload, yy_total};
    VgChain ch;                                   // same state as at the matching vggp_elbo_partials call
    vg_start_prepare(c, /*own_payload=*/false, &ch);
    ch.copy_theta = true;
    rc = run_graph(c, vg_graph_slot(ch, /*fused=*/false), key, st, [&] { return finish_enqueue(c, payload, yy_total, st, ch); });
    if (rc) return rc;
    // The read-outs after a WARM step re-run the finish half cold on the step's reduced G2, H2, C (vg_accurate_state), and the caller's
    // buffer is the caller's again once this call returns: keep a copy in the context's own payload buffer, which this entry point
    // leaves unused -- one device-to-device copy on the step's stream, behind the graph.  (A cold step's read-outs rebuild nothing.)
    const double* kept = payload;
    if (ch.warm && payload != c->payload) {
        VG_HIP(hipMemcpyAsync(c->payload, payload, sizeof(double) * c->payload_len, hipMemcpyDeviceToDevice, st));
        kept = c->payload;
    }
    c->last_warm = ch.warm; c->last_slabs = false; c->last_payload = kept; c->last_yy = yy_total;
    return finish_collect(c, elbo_out, grad_out, info, st);
}
extern "C" int vggp_elbo_finish(vggp_ctx* c, const double* payload, double yy_total, const double theta[5],
                                double* elbo_out, double grad_out[5], vggp_info* info, void* stream) {
    VG_NOT_PAIRED(c, "vggp_elbo_finish");
    int rc = elbo_finish_once(c, payload, yy_total, theta, elbo_out, grad_out, info, stream);
    if (rc == VG_ESUBMISS) rc = elbo_finish_once(c, payload, yy_total, theta, elbo_out, grad_out, info, stream);   // cold, same payload
    if (rc == VG_ESUBMISS) { vg_set_error("the eigensolver chain failed twice on the same step"); rc = VGGP_ENOCONV; }
    return rc;
}

// ---- cold start of the thin chain (RBF factors): a range finder instead of the full Jacobi solve.
// G = B B^T of an RBF factor has numerical rank ~17 of 128, and "Z = V G" maps ANY r-row start V onto range(G) exactly (G annihilates
// the null components) -- but the row-by-row orthonormalisation of Z keeps the small range directions only when the rows of V are
// GRADED (row i mostly within the i leading eigen-directions); a random sketch is not.  So:
//   pass 1:  r0 = 32 steps of diagonally pivoted Cholesky of G (thin.hip, vg_pivchol_kernel): graded columns spanning range(G),
//            orthonormalised in pivot order into the leading rows of QtPrev;
//   pass 2:  the warm thin chain itself from those rows;
// and the tail kernel's miss check (tr G - sum theta) decides as in every thin step: a spectrum that does not fit 32 rows is refused,
// the step is repeated with the full solve and the thin chain stays off for 32 steps.  VGGP_NO_COLD_THIN=1: always the full solve.
#define VG_COLD_THIN_R 32
static bool vg_cold_thin_ok(const vggp_ctx* c) {
    static const bool off = getenv("VGGP_NO_COLD_THIN") != nullptr || getenv("VGGP_NO_THIN") != nullptr || getenv("VGGP_NO_SUBSPACE") != nullptr;
    if (off || c->thin_off || c->thin_block > 0 || c->prof || (c->desc.flags & (VGGP_FLAG_BLOCK_JACOBI | VGGP_FLAG_SCATTERED))) return false;
    if (c->n_ranks > 1 || c->comm || c->cb) return false;
    for (int k = 0; k < 2; ++k) {
        const VgDim& d = c->d[k];
        if (!d.Omega || !d.tMV || d.kind != VGGP_KIND_RBF || d.m < 3 * VG_COLD_THIN_R || d.m > 256) return false;
    }
    return true;
}
static int vg_cold_thin_prepass(vggp_ctx* c, const double* payload, hipStream_t st) {
    const double* Gk[2] = {c->d[0].GH, payload};                  // reduced Gram matrices (the partials half ran with reduce)
    VgPivCholJob pj[2];
    for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; pj[k] = VgPivCholJob{Gk[k], d.Omega, d.TM, d.m, VG_COLD_THIN_R}; }
    VG_HIP(vg_pivchol_launch(pj, 2, st));
    VgRowQrJob qj[2];
    for (int k = 0; k < 2; ++k) { VgDim& d = c->d[k]; qj[k] = VgRowQrJob{d.TM, d.QtPrev, VG_COLD_THIN_R, d.m, nullptr, nullptr, 0}; }
    VG_HIP(vg_rowqr_launch(qj, 2, st, nullptr));
    return VGGP_OK;
}

// The early projection (vg_partials_enqueue, early) can run: both factors are single 128-blocks on the MFMA Cholesky path and the
// projection branch stays on the main stream.  (What else a caller needs -- no profiling, riders, no jitter -- is spelled out there.)
static bool vg_early_ok(vggp_ctx* c, hipStream_t st) {
    static const bool no_early = getenv("VGGP_NO_EARLY") != nullptr;
    return !no_early && c->desc.m1 <= 128 && c->desc.m2 <= 128 && vg_side(c, st) == st && getenv("VGGP_CHOL_LEGACY") == nullptr;
}
// The early pass over Y whitens afterwards, S = L^-1 (A Y): its rounding grows with cond(Kuu).  Where a factor needed jitter in the
// last step (RBF points: cond ~ 1e10) the REGULAR warm chains keep the late association (L^-1 A) Y -- with the early one the gradient
// of a warm step at 192 x 192, m_d = 24 was 3.4e-7 off the oracle.  (The thin chain's own early projection is not affected.)
static bool vg_jittered(const vggp_ctx* c) { return c->h_out->jitter[0] > 0.0 || c->h_out->jitter[1] > 0.0; }

static int elbo_step_once(vggp_ctx* c, const double* Y, double yy_total, const double theta[5], double* elbo_out,
                          double grad_out[5], vggp_info* info, void* stream) {
    if (!c || !c->planned) { vg_set_error("vggp_elbo_step: context not planned"); return VGGP_ESTATE; }
    if (c->desc.flags & VGGP_FLAG_SCATTERED) { vg_set_error("vggp_elbo_step: the context was planned for scattered points (use vggp_elbo_step_scattered)"); return VGGP_ESTATE; }
    VG_REQUIRE(Y && theta && elbo_out && grad_out, "vggp_elbo_step: null argument");
    c->have_iter = false;            // (the eigensolver chain overwrites the basis the iterative step's read-outs precondition with)
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    int rc = set_theta(c, theta);
    if (rc) return rc;
    c->nev = 0;
    VgChain ch;
    vg_start_prepare(c, /*own_payload=*/true, &ch);
    const bool warm = ch.warm, extrap = ch.extrap;
    VgPartials po;
    po.extrap = extrap; po.apply_ns = extrap && !c->pred_consumed;
    const bool bypass = extrap && !po.apply_ns;      // (the Newton-Schulz step was applied already: run un-captured without it)
    if (c->n_ranks > 1 || c->comm || c->cb) {
        // row-sharded job: partials graph -> the context's all-reduce of the packed payload (RCCL: enqueued on this stream)
        // -> finish graph; the one host synchronisation is in finish_collect.  Every rank finishes redundantly, so all ranks
        // hold the identical value and gradient without a broadcast.
        const VgGraphKey kp{Y, c->payload, 0.0}, kf{nullptr, c->payload, yy_total};
        // thin chain: the pass over the rank's slab of Y rides beside the Cholesky (vg_partials_enqueue, early), the finish half places
        // the small products of the reduced [C;C1;C2] as the fused single-rank step does
        const bool early_ok = !c->prof && vg_early_ok(c, st);
        ch.thin_early = ch.thin && early_ok && !extrap;
        // (the regular warm chains take the early association too, as in the fused single-rank step: the two must agree to rounding)
        static const bool no_early_reg_mr = getenv("VGGP_NO_EARLY_REG") != nullptr;
        const bool early_mr = ch.thin_early || (warm && !ch.thin && !ch.subspace && early_ok && !no_early_reg_mr && !vg_jittered(c));
        po.early = early_mr ? 1 : 0;
        rc = run_graph(c, early_mr ? (extrap ? VG_G_PARTIALS_XE : VG_G_PARTIALS_E) : extrap ? VG_G_PARTIALS_X : VG_G_PARTIALS, kp, st,
                       [&] { return vg_partials_enqueue(c, Y, c->payload, st, po); }, bypass);
        {
            // fault injection for the failure-path test (tests/test_gpu_dist.py): VGGP_FAULT_PARTIALS_AT=<step number>
            static const long fault_at = [] { const char* e = getenv("VGGP_FAULT_PARTIALS_AT"); return e ? atol(e) : -1L; }();
            if (!rc && fault_at >= 0 && c->seq == fault_at) { vg_set_error("injected fault in the partials of step %ld", c->seq); rc = VGGP_EHIP; }
        }
        if (rc) {
            // This rank cannot contribute, but its peers are about to enter the all-reduce: join it with a zero payload and the
            // failure word set, so that every rank leaves the collective and returns an error instead of hanging in it.
            char msg[512];
            snprintf(msg, sizeof(msg), "%s", vggp_last_error());
            static const double one = 1.0;
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) { hipGraph_t gdrop = nullptr; (void)hipStreamEndCapture(st, &gdrop); if (gdrop) (void)hipGraphDestroy(gdrop); }
            (void)hipMemsetAsync(c->payload, 0, sizeof(double) * c->payload_len, st);
            (void)hipMemcpyAsync(c->payload + c->payload_len, &one, sizeof(double), hipMemcpyHostToDevice, st);
            if (vg_allreduce(c, c->payload, c->payload_len + 1, st) == VGGP_OK) (void)vg_comm_wait(c, st);
            else vg_comm_abort(c);
            vg_drop_warm(c);
            c->have_step = false;
            vg_set_error("%s", msg);
            return rc;
        }
        if (extrap) c->pred_consumed = true;
        c->have_partials = true;
        if ((rc = vg_allreduce(c, c->payload, c->payload_len + 1, st))) return rc;
        rc = run_graph(c, vg_graph_slot(ch, /*fused=*/false), kf, st, [&] { return finish_enqueue(c, c->payload, yy_total, st, ch); });
        if (rc) return rc;
        c->last_warm = warm; c->last_slabs = false; c->last_payload = c->payload; c->last_yy = yy_total;
        return finish_collect(c, elbo_out, grad_out, info, st);
    }
    const VgGraphKey key{Y, c->payload, yy_total};
    static const bool no_ride = getenv("VGGP_NO_RIDE") != nullptr;
    po.fused = true;
    if (!warm && vg_cold_thin_ok(c)) {
        // cold step of a rank-deficient plan: range finder + thin chain (see vg_cold_thin_prepass) instead of the full Jacobi solve
        VgChain thin;                    // the warm thin chain from the range finder's rows, on reduced operands
        thin.warm = thin.subspace = thin.thin = true; thin.thin_early = vg_early_ok(c, st);
        VgPartials pc;
        pc.fused = true; pc.early = thin.thin_early;
        const int keep[2] = {c->d[0].sub_r, c->d[1].sub_r};
        c->d[0].sub_r = c->d[1].sub_r = VG_COLD_THIN_R;          // (sizes of the captured thin chain; the host's rank bookkeeping keeps its own)
        rc = run_graph(c, VG_G_STEP_COLD_T, key, st, [&] {
            int r1 = vg_partials_enqueue(c, Y, c->payload, st, pc);
            if (!r1) r1 = vg_cold_thin_prepass(c, c->payload, st);
            return r1 ? r1 : finish_enqueue(c, c->payload, yy_total, st, thin);
        });
        c->d[0].sub_r = keep[0]; c->d[1].sub_r = keep[1];
        if (rc) return rc;
        c->cur_thin = true; c->cur_extrap = false; c->cur_newton = 0;
        c->cur_r[0] = c->cur_r[1] = VG_COLD_THIN_R;
        c->have_partials = true;
        c->last_warm = true;             // (no full m-space state behind this step: the read-outs that need one rebuild it)
        c->last_slabs = false; c->last_payload = c->payload; c->last_yy = yy_total;
        return finish_collect(c, elbo_out, grad_out, info, st);
    }
    // thin chain with the early projection (vg_partials_enqueue): where the step defers its projection launches to the eigensolver
    // chain anyway, and both factors are single 128-blocks
    ch.thin_early = ch.thin && !no_ride && vg_early_ok(c, st);
    // the regular warm chains (refinement + polish, Newton chain) take the early pass over Y as well: [C;C1;C2] then rides where S
    // used to (beside the refinement kernel) and the main solve carries nothing.  VGGP_NO_EARLY_REG=1: riders as in round 2.
    static const bool no_early_reg = getenv("VGGP_NO_EARLY_REG") != nullptr;
    const bool early_reg = warm && !ch.thin && !ch.subspace && !no_early_reg && !no_ride && vg_early_ok(c, st) && (vg_ride(c) || c->prof) &&
                           !vg_jittered(c);
    ch.from_slabs = warm;
    po.reduce = !warm;
    po.early = ch.thin_early ? 1 : (early_reg ? 2 : 0);
    rc = run_graph(c, vg_graph_slot(ch, /*fused=*/true), key, st, [&] {
        const int r1 = vg_partials_enqueue(c, Y, c->payload, st, po);
        return r1 ? r1 : finish_enqueue(c, c->payload, yy_total, st, ch);
    }, bypass);
    if (rc) return rc;
    if (extrap) c->pred_consumed = true;
    c->have_partials = true;
    c->last_warm = warm; c->last_slabs = warm; c->last_payload = c->payload; c->last_yy = yy_total;
    return finish_collect(c, elbo_out, grad_out, info, st);
}
// A step whose subspace start turns out to have missed part of the range (VG_ESUBMISS: the hyper-parameters jumped) is repeated
// once, cold -- the failed attempt has already reset the warm start.  A jump the host can see beforehand (> 5 % in a lengthscale
// since the last step; the Gram matrices depend on nothing else) skips the attempt.
extern "C" int vggp_elbo_step(vggp_ctx* c, const double* Y, double yy_total, const double theta[5], double* elbo_out,
                              double grad_out[5], vggp_info* info, void* stream) {
    VG_FORWARD_PAIRED(c, vg_paired_step(c, Y, yy_total, theta, elbo_out, grad_out, info, stream ? (hipStream_t)stream : c->own_stream, false));
    if (c && c->planned && theta) {
        bool jump = false;
        for (int k = 0; k < 2; ++k) jump = jump || (c->last_ell[k] > 0.0 && std::fabs(theta[k] / c->last_ell[k] - 1.0) > 0.05);
        if (jump && c->sub_next) vg_drop_warm(c);
        c->last_ell[0] = theta[0]; c->last_ell[1] = theta[1];
    }
    int rc = elbo_step_once(c, Y, yy_total, theta, elbo_out, grad_out, info, stream);
    if (rc == VG_ESUBMISS) rc = elbo_step_once(c, Y, yy_total, theta, elbo_out, grad_out, info, stream);
    if (rc == VG_ESUBMISS) { vg_set_error("the eigensolver chain failed twice on the same step"); rc = VGGP_ENOCONV; }
    return rc;
}

// Read-outs after a WARM-started step.  The warm paths (subspace start, first-order refinement) diagonalise G to the
// eigensolver's ABSOLUTE threshold, which is all the ELBO and its gradient need; but the numerically-null block of an RBF Gram
// matrix is then only block-diagonalised -- its rows are the previous step's rows projected off the new range -- so the tiny
// eigenvalues lam_i (1e-13 lam_max) are mixtures.  The posterior VARIANCE sees that through D = 1 + lam1 lam2 / sigma^2 with
// lam1 ~ 1e3: 5e-4 relative at 1024 x 1024 RBF (measured; the cold solve's cyclic sweeps resolve that block to high RELATIVE
// accuracy and agree with the oracle to 6e-9).  So the first read-out after a warm step re-runs the finish half COLD on the
// step's own G, H, C (still resident): one cold eigensolve (~1 ms) per prediction request, nothing in the fit loop.
// VGGP_FAST_READOUT=1 skips it (read-outs then carry the warm basis' accuracy).
int vg_accurate_state(vggp_ctx* c, hipStream_t st) {
    static const bool skip = getenv("VGGP_FAST_READOUT") != nullptr;
    if ((skip && !c->last_thin) || !c->last_warm || c->acc_valid || !c->have_step) return VGGP_OK;     // (a thin step leaves no m-space state at all)
    if (c->last_payload != c->payload) return VGGP_OK;       // (a caller's payload is not retained; vggp_elbo_finish keeps a copy of a warm step's)
    const long m1 = c->desc.m1, m2 = c->desc.m2;
    if (c->last_slabs) {                                       // fused warm step: G, H, C are still split-K slabs
        VgRedBatch r;
        vg_red_init(&r);
        vg_red_add(&r, c->d[0].GHslab, c->d[0].GH, 2L * m1 * m1, 2L * m1 * m1, c->gh_slabs[0]);
        vg_red_add(&r, c->d[1].GHslab, c->payload, 2L * m2 * m2, 2L * m2 * m2, c->gh_slabs[1]);
        vg_red_add(&r, c->CCslab, c->payload + 2 * m2 * m2, 3L * m1 * m2, 3L * m1 * m2, c->cc_slabs);
        VG_HIP(vg_red_launch(&r, st));
    }
    VgClearArgs clr;                                           // the step's flag words (normally zeroed by the factor kernel)
    clr.n = 0;
    for (int k = 0; k < 2; ++k) { clr.ptr[clr.n] = c->d[k].counters; clr.nwords[clr.n++] = 8; clr.ptr[clr.n] = c->d[k].status + 1; clr.nwords[clr.n++] = 1; }
    VG_HIP(vg_clear_launch(&clr, st));
    const bool prof = c->prof; c->prof = false;
    const int rc = finish_enqueue(c, c->payload, c->last_yy, st, VgChain());      // cold, on the reduced operands
    c->prof = prof;
    if (rc) return rc;
    VG_HIP(hipStreamSynchronize(st));
    const int status = vg_step_status(c);
    if (status) { vg_set_error("accurate read-out: the cold eigensolve failed (status %d)", status); return status; }
    // QtPrev now holds the cold basis and QtPrev2 the warm basis of the SAME step: no extrapolation across that pair
    for (int k = 0; k < 2; ++k) { c->d[k].have_prev2 = false; c->d[k].thin_rows = c->d[k].m; }
    c->last_thin = false;
    c->pred_consumed = false;
    c->acc_valid = true;
    return VGGP_OK;
}
