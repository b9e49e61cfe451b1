// Per-dimension factor build at unit outputscale: A0 = Kuf_d / s_d  (m x n), K0 = Kuu_d / s_d
// (m x m) and their derivatives with respect to the lengthscale, fused in one pass.
//
// Replaces (reference paths relative to the reference checkout):
//   pairwise  kernel_d(Z), kernel(Z, x)            kronecker_structure.py:318-319, :336-337
//   B0-spline _Kuu_along_dim / _Kuf_along_dim       kronecker_structure.py:723-739, :768-790
//                                                  (== gridded_kronecker_structure.py:1307-1374)
// The kernel is HBM-write-bound (16 B per output element: value + d/d ell, one exp() each).  2-D tiling: a 256-thread
// workgroup owns an (inducing-feature rows) x (observation columns) tile, WIDE (tmw rows x 512 columns, the four waves
// side by side) when the matrix has >= 512 columns, TALL (4 tmw rows x 128 columns, one wave per row group) otherwise.
// Lanes run along the observation index p (the contiguous axis of the row-major [m][n] outputs) and own TWO adjacent
// columns: their coordinates are read once (one coalesced 16-B load) and stay in registers for all rows of the tile, and
// every store is a 16-B store (a wave writes 1 KiB of one output row).  The mesh / inducing coordinates of the tile's
// rows are staged once in LDS and read as wave-uniform broadcasts.  No per-thread division anywhere (one 32-bit division
// per workgroup maps the block index to its tile).  B0 cell integrals: cell k's right edge is cell k+1's left edge, so a
// thread walking down the rows evaluates ONE exponential per element, not two.
#include "common.h"
#include "factor_elem.h"

#define VG_FB_MAXJOBS 4
struct VgFactorArgs {
    VgFactorJob job[VG_FB_MAXJOBS];
    int block_start[2 * VG_FB_MAXJOBS + 1];   // per job: A part then K part
    int njobs;
};

#define VG_FB_TN_WIDE 512
#define VG_FB_TN_TALL 128
#define VG_FB_MAXROWS 64          // rows per tile (tall tiles: 4 * tmw), bounds the LDS staging of the row coordinates

struct VgFbPart {                 // one output matrix pair (value, d/d ell) of one job
    int job, kpart;               // kpart: the m x m matrix K0 (columns = inducing features) instead of the m x n matrix A0
    int ncols, tiles_c, tmw, wide, block_start;
};
struct VgFactorArgs2 {
    VgFactorJob job[VG_FB_MAXJOBS];
    VgFbPart part[2 * VG_FB_MAXJOBS];
    int nparts;
};

#define VG_FB_KERNEL vg_factor_kernel
#define VG_FB_B0K 0
#include "factor_kernel_body.h"
#undef VG_FB_KERNEL
#undef VG_FB_B0K
#define VG_FB_KERNEL vg_factor_b0k_kernel
#define VG_FB_B0K 1
#include "factor_kernel_body.h"
#undef VG_FB_KERNEL
#undef VG_FB_B0K

hipError_t vg_factor_build_launch(const VgFactorJob* jobs, int njobs, const double* theta_dev, hipStream_t st,
                                  double* theta_copy, const VgClearArgs* clr) {
    if (njobs < 1 || njobs > VG_FB_MAXJOBS) return hipErrorInvalidValue;
    VgFactorArgs2 a;
    a.nparts = 0;
    int blocks = 0;
    long total = 0;
    bool b0k = false;
    for (int j = 0; j < njobs; ++j) {
        total += ((jobs[j].A0 || jobs[j].dA0) ? (long)jobs[j].m * jobs[j].n : 0) + ((jobs[j].K0 || jobs[j].dK0) ? (long)jobs[j].m * jobs[j].m : 0);
    }
    // rows per wave: small launches (the step's 2 MB of factors) are latency-bound and want many workgroups; large ones
    // amortise the per-thread set-up (coordinate loads, LDS staging) over more rows
    const int tmw = total >= (1L << 24) ? 16 : (total >= (1L << 21) ? 8 : (total >= (1L << 18) ? 4 : 2));
    for (int j = 0; j < njobs; ++j) {
        a.job[j] = jobs[j];
        if (jobs[j].basis == VGGP_BASIS_B0K) {
            // Matern-1/2 cells are the B0 cells: the same code, the same bits; the other kernels take the second instantiation
            if (jobs[j].kind == VGGP_KIND_MATERN12) a.job[j].basis = VGGP_BASIS_B0;
            else b0k = true;
        }
        for (int kp = 0; kp < 2; ++kp) {
            const bool want = kp ? (jobs[j].K0 || jobs[j].dK0) : (jobs[j].A0 || jobs[j].dA0);
            const int ncols = kp ? jobs[j].m : jobs[j].n;
            if (!want || ncols <= 0 || jobs[j].m <= 0) continue;
            VgFbPart& P = a.part[a.nparts++];
            P.job = j; P.kpart = kp; P.ncols = ncols; P.tmw = tmw;
            P.wide = ncols >= VG_FB_TN_WIDE ? 1 : 0;
            const int tn = P.wide ? VG_FB_TN_WIDE : VG_FB_TN_TALL, rows = P.wide ? tmw : 4 * tmw;
            P.tiles_c = (ncols + tn - 1) / tn;
            P.block_start = blocks;
            blocks += P.tiles_c * ((jobs[j].m + rows - 1) / rows);
        }
    }
    if (blocks == 0) return hipSuccess;
    VgClearArgs c0;
    c0.n = 0;
    if (b0k) hipLaunchKernelGGL(vg_factor_b0k_kernel, dim3(blocks), dim3(256), 0, st, a, theta_dev, theta_copy, clr ? *clr : c0);
    else hipLaunchKernelGGL(vg_factor_kernel, dim3(blocks), dim3(256), 0, st, a, theta_dev, theta_copy, clr ? *clr : c0);
    return hipGetLastError();
}
