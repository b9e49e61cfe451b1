// The block preconditioned conjugate-gradient solver of the library: one loop, one set of per-column scalars and one probe hash for
// the iterative Kronecker steps with their read-outs (iter_step.hip, iter_readout.hip) and for the iterative exact GP (exact_iter.hip).
// Block vectors are [rows][nbc][inner]: [m1][nbc][m2] on the Kronecker path, [N][nbp][1] on the exact one.  What differs between the
// two -- the operator, the preconditioner, how a column dot is summed and how the host waits -- comes in through the caller object
// of vg_block_pcg.
#pragma once
#include "common.h"

#define VG_PCG_ESTALE (-1001)   // internal: still active columns after more than stale_limit iterations (the caller gives its kept basis up)

__device__ __forceinline__ unsigned long long vg_pcg_mix(unsigned long long x) {    // splitmix64 finaliser
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}
// blk[a][c][b] = +-1 for the probe columns 1 <= c < ncols (counter-based, keyed on (c, a inner + b): the same probes on every device,
// every run), 0 for column 0 and the padding columns c >= ncols
static __global__ void vg_pcg_probe_kernel(double* blk, long rows, int nbc, int inner, int ncols, unsigned long long seed) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * nbc * inner) return;
    const int c = (int)((idx / inner) % nbc);
    const long a = idx / ((long)inner * nbc), b = idx % inner;
    const unsigned long long h = vg_pcg_mix(seed ^ vg_pcg_mix(((unsigned long long)c << 40) ^ ((unsigned long long)a * inner + b)));
    blk[idx] = (c == 0 || c >= ncols) ? 0.0 : ((h >> 17) & 1ULL ? 1.0 : -1.0);
}
// Partials part[nchunk][2][stride] -> two sums per column (ascending chunk order), then the PCG scalar logic, one lane per column.
// col rows of length stride: [0] rz, [1] pAp, [2] r0^2, [3] rr, [4] alpha, [5] beta, [6] active, [7] k.
// phase 0 (start): sums = <r, P^-1 r>, <r, r>;  1: <p, Ap>;  2: the new <r, P^-1 r>, <r, r>;  3: plain sums into rows [8], [9].
// alh / beh (may be null): the coefficients of this iteration go to their row `it`.  *nact: the active ones of the ncols live columns
static __global__ void vg_pcg_scalars_kernel(const double* part, int nchunk, double* col, int stride, int ncols, int phase, int it, double tol,
                                             double* alh, double* beh, int* nact) {
    const int c = threadIdx.x;
    double *rz = col, *pAp = col + stride, *r02 = col + 2 * stride, *rr = col + 3 * stride, *al = col + 4 * stride, *be = col + 5 * stride,
           *act = col + 6 * stride, *kc = col + 7 * stride;
    if (c < stride) {
        double s0 = 0.0, s1 = 0.0;
        for (int k = 0; k < nchunk; ++k) { s0 += part[((long)k * 2) * stride + c]; s1 += part[((long)k * 2 + 1) * stride + c]; }
        if (phase == 0) {
            rz[c] = s0; rr[c] = s1; r02[c] = s1; act[c] = (c < ncols && s1 > 0.0) ? 1.0 : 0.0; kc[c] = 0.0; al[c] = 0.0; be[c] = 0.0;
        } else if (phase == 1) {
            pAp[c] = s0;
            const double a = (act[c] != 0.0 && s0 > 0.0) ? rz[c] / s0 : 0.0;
            al[c] = a;
            if (alh) alh[(long)it * stride + c] = a;
        } else if (phase == 2) {
            rr[c] = s1;
            const double b = (act[c] != 0.0 && rz[c] > 0.0) ? s0 / rz[c] : 0.0;
            be[c] = b;
            if (beh) beh[(long)it * stride + c] = b;
            rz[c] = s0;
            if (act[c] != 0.0) kc[c] += 1.0;
            if (!(s1 > tol * tol * r02[c])) act[c] = 0.0;
        } else {
            col[8 * stride + c] = s0; col[9 * stride + c] = s1;
        }
    }
    __syncthreads();
    if ((phase == 0 || phase == 2) && threadIdx.x == 0) { int n = 0; for (int k = 0; k < ncols; ++k) n += act[k] != 0.0 ? 1 : 0; *nact = n; }
}
// phase 1: x += alpha_c p, r -= alpha_c ap;  phase 2: p = z + beta_c p
static __global__ void vg_pcg_update_kernel(double* X, double* R, double* Pd, const double* AP, const double* Zp, const double* col, long n,
                                            int nbc, int inner, int stride, int phase) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)((idx / inner) % nbc);
    if (phase == 1) { const double a = col[4 * stride + c]; X[idx] += a * Pd[idx]; R[idx] -= a * AP[idx]; }
    else Pd[idx] = Zp[idx] + col[5 * stride + c] * Pd[idx];
}

struct VgBlockPcg {
    double *X, *R, *Pd, *AP, *Zp;     // [rows][nbc][inner]: R holds the right-hand sides on entry, X the solution on return
    double* part; int nchunk;         // [nchunk][2][stride] partials of the column dots (filled by ops.dots)
    double* col; int stride;          // the per-column scalars (vg_pcg_scalars_kernel), stride <= 64
    double *alh, *beh;                // [max_iter][stride] coefficient history (null: none kept)
    int* nact;                        // device word: number of active columns
    long rows; int nbc, inner, ncols; // ncols <= nbc live columns (the rest is zero padding)
    bool count_at_start;              // read the active count back after phase 0 too: an all-zero block then reports 0 iterations
                                      // instead of 1, at the price of one more host round trip per solve
};
// Block PCG for A X = R with a per-column stopping rule (|r_c| <= tol |r0_c|; zero columns start inactive).  ops supplies
//     int apply()          AP = A Pd
//     int precond()        Zp = P^-1 R
//     int dots(int phase)  part = the column dots of the phase: 0 and 2 <R, Zp>, <R, R>;  1 <Pd, AP> (second slot unused)
//     int active(int* n)   *n = *b.nact, after whatever host wait the caller's context needs
// history: iteration k keeps its coefficients in row k of alh / beh instead of row 0.  stale_limit > 0: a solve that still has
// active columns after more iterations than that returns VG_PCG_ESTALE.  One host read-back of the active count per iteration.
template <class Ops>
static int vg_block_pcg(const VgBlockPcg& b, Ops&& ops, double tol, int max_iter, bool history, int stale_limit, int* iters_out,
                        int* nact_out, hipStream_t st) {
    const long n = b.rows * b.nbc * b.inner;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    auto scalars = [&](int phase, int row) {
        hipLaunchKernelGGL(vg_pcg_scalars_kernel, dim3(1), dim3(64), 0, st, b.part, b.nchunk, b.col, b.stride, b.ncols, phase, row, tol, b.alh,
                           b.beh, b.nact);
    };
    int rc;
    VG_HIP(hipMemsetAsync(b.X, 0, sizeof(double) * n, st));
    if ((rc = ops.precond())) return rc;
    VG_HIP(hipMemcpyAsync(b.Pd, b.Zp, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    if ((rc = ops.dots(0))) return rc;
    scalars(0, 0);
    int iters = 0, nact = b.ncols;
    if (b.count_at_start && (rc = ops.active(&nact))) return rc;
    for (int k = 0; k < max_iter && nact > 0; ++k) {
        const int row = history ? k : 0;
        if ((rc = ops.apply())) return rc;
        if ((rc = ops.dots(1))) return rc;
        scalars(1, row);
        hipLaunchKernelGGL(vg_pcg_update_kernel, grid, block, 0, st, b.X, b.R, b.Pd, b.AP, b.Zp, b.col, n, b.nbc, b.inner, b.stride, 1);
        if ((rc = ops.precond())) return rc;
        if ((rc = ops.dots(2))) return rc;
        scalars(2, row);
        hipLaunchKernelGGL(vg_pcg_update_kernel, grid, block, 0, st, b.X, b.R, b.Pd, b.AP, b.Zp, b.col, n, b.nbc, b.inner, b.stride, 2);
        VG_HIP(hipGetLastError());
        if ((rc = ops.active(&nact))) return rc;
        iters = k + 1;
        if (stale_limit > 0 && nact > 0 && iters > stale_limit) return VG_PCG_ESTALE;
    }
    *iters_out = iters;
    *nact_out = nact;
    return VGGP_OK;
}
