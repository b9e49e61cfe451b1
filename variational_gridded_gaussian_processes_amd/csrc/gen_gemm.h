// The generated-operand fp64-MFMA GEMM of the dense point-set solvers: operands are evaluated element by element on chip (kernel
// values from coordinates, face-split cross-covariances) and never stored; the result is consumed by an epilogue.  Shared by the
// paired inducing points (paired.hip) and the exact GP (exact.hip), with the small helpers both use.
#pragma once
#include "ctx.h"
#include "factor_elem.h"

#define PZ_T 64               // output tile of the generated-operand kernel (4 waves, 2 x 2, each 32 x 32)
#define PZ_BK 16              // k-tile
#define PZ_MAX_M 16384        // dense M-space solver (twelve M x M matrices; 18 on a full grid)
#define PZ_MB 128             // panel width of vg_blocked_chol_inverse

typedef double pz_d4 __attribute__((ext_vector_type(4)));

// ---- operand generators ----------------------------------------------------------------------------------------------------
struct PzPts {                // unit-outputscale kernel element k(z_r, x_c): r an inducing point, c a data / test point
    const double *z1, *z2, *x1, *x2;
    int kind1, kind2;
    double inv1, inv2;
    __device__ __forceinline__ double val(int r, int c) const {
        double v1, d1, v2, d2;
        vg_kappa(kind1, fabs(z1[r] - x1[c]), inv1, v1, d1);
        vg_kappa(kind2, fabs(z2[r] - x2[c]), inv2, v2, d2);
        return v1 * v2;
    }
};
struct PzFace {               // face-split cross-covariance F0[v][r] = C1[a][r] C2[b][r], v = a mv2 + b (the reference's _Kvu order)
    const double *C1, *C2;
    int mv2, M;
    __device__ __forceinline__ double val(int r, int c) const {
        const int a = c / mv2, b = c - a * mv2;
        return C1[(long)a * M + r] * C2[(long)b * M + r];
    }
};
template <class G> struct PzARow { G g; __device__ __forceinline__ double a(int i, int k) const { return g.val(i, k); } };   // A[i][k] = g(i, k)
struct PzAMat { const double* X; long ld; __device__ __forceinline__ double a(int i, int k) const { return X[(long)i * ld + k]; } };
template <class G> struct PzBCol { G g; __device__ __forceinline__ double b(int k, int j) const { return g.val(j, k); } };   // B[k][j] = g(j, k)
template <class G> struct PzBRow { G g; __device__ __forceinline__ double b(int k, int j) const { return g.val(k, j); } };   // B[k][j] = g(k, j)

// ---- epilogues -------------------------------------------------------------------------------------------------------------
#define PZ_EPI_SYM 0          // store the tile and its mirror image into slab ks (+ b = B y on the diagonal tiles)
#define PZ_EPI_ROW4 1         // four per-row contractions, summed over the tile's columns -> part[tn][row][4]
#define PZ_EPI_COL1 2         // one per-column contraction, summed over the tile's rows -> part[tm][col]
struct PzEpSym { double* slab; const double* y; double* bpart; long M; };
struct PzEpGrad {             // pass 2: G = 2 s (Pb B)[i, n] + cb_i y_n against dB/d(ell1, ell2, z_i1, z_i2) at (i, n)
    PzPts g; const double* y; const double* cb; double two_s; double* part; long M;
    __device__ __forceinline__ void row4(int i, int n, double acc, double (&o)[4]) const {
        const double G = two_s * acc + cb[i] * y[n];
        double v1, l1, z1, v2, l2, z2;
        vg_kappa_z(g.kind1, g.z1[i] - g.x1[n], g.inv1, v1, l1, z1);
        vg_kappa_z(g.kind2, g.z2[i] - g.x2[n], g.inv2, v2, l2, z2);
        o[0] += G * l1 * v2; o[1] += G * v1 * l2; o[2] += G * z1 * v2; o[3] += G * v1 * z2;
    }
};
template <class G> struct PzEpCol {   // variance read-outs: (Q F^T)[i, p] F[p, i], summed over i
    G g; double* part; long ncol;
    __device__ __forceinline__ double col1(int i, int p, double acc) const { return acc * g.val(i, p); }
};

// C[Mr x Nc] = op(A) op(B) over k in [ks kchunk, min(K, (ks + 1) kchunk)), operands produced element by element by OA / OB (into
// LDS; generated ones are never in memory), result consumed by the epilogue.  tri: only tiles tn >= tm (symmetric products).
template <int MODE, class OA, class OB, class EP>
__global__ __launch_bounds__(256) void pz_gen_gemm_kernel(const OA oa, const OB ob, const EP ep, int Mr, int Nc, int K, int kchunk,
                                                          int tiles_n, int tri, int tn_per, const int* skip) {
    __shared__ double As[PZ_T][PZ_BK + 1];
    __shared__ double Bs[PZ_BK][PZ_T + 1];
    __shared__ double red[4][32][4];
    if (skip && *skip) return;                                   // (the step in flight already failed: nothing to compute)
    // tiles: tri -> the upper triangle tn >= tm, one per workgroup; otherwise row tile tm and a run of tn_per column tiles, taken
    // one after the other by the same workgroup (ROW4 sums them in that order: its partials are per run, not per column tile)
    int tm, tn_first, tn_last;
    if (tri) {
        tm = 0;
        int rem = blockIdx.x;
        while (rem >= tiles_n - tm) { rem -= tiles_n - tm; ++tm; }
        tn_first = tn_last = tm + rem;
    } else {
        const int nrun = (tiles_n + tn_per - 1) / tn_per;
        tm = blockIdx.x / nrun;
        const int run = blockIdx.x - tm * nrun;
        tn_first = run * tn_per;
        tn_last = min(tiles_n, tn_first + tn_per) - 1;
    }
    double racc = 0.0;                                           // ROW4: this thread's (row, quantity) sum over the run
  for (int tn = tn_first; tn <= tn_last; ++tn) {
    const int ks = blockIdx.y;
    const int row0 = tm * PZ_T, col0 = tn * PZ_T;
    const int kb = ks * kchunk, ke = min(K, kb + kchunk);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, fi = lane & 15, fk = lane >> 4;
    const bool diag = MODE == PZ_EPI_SYM && tm == tn;
    pz_d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (pz_d4){0.0, 0.0, 0.0, 0.0};
    double bacc = 0.0;
    for (int k0 = kb; k0 < ke; k0 += PZ_BK) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = tid + 256 * r;
            const int ai = e >> 4, ak = e & 15;                  // A: k fastest
            const int gi = row0 + ai, gk = k0 + ak;
            As[ai][ak] = (gi < Mr && gk < ke) ? oa.a(gi, gk) : 0.0;
            const int bk = e >> 6, bj = e & 63;                  // B: j fastest
            const int gkb = k0 + bk, gj = col0 + bj;
            Bs[bk][bj] = (gkb < ke && gj < Nc) ? ob.b(gkb, gj) : 0.0;
        }
        __syncthreads();
        if constexpr (MODE == PZ_EPI_SYM) {
            if (diag && tid < PZ_T) {
#pragma unroll
                for (int k = 0; k < PZ_BK; ++k)
                    if (k0 + k < ke) bacc += As[tid][k] * ep.y[k0 + k];
            }
        }
#pragma unroll
        for (int kk = 0; kk < PZ_BK; kk += 4) {
            double av[2], bv[2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) av[mb] = As[wr * 32 + mb * 16 + fi][kk + fk];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) bv[nb] = Bs[kk + fk][wc * 32 + nb * 16 + fi];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[mb], bv[nb], acc[mb][nb], 0, 0, 0);
        }
        __syncthreads();
    }
    // MFMA 16x16x4 f64 result layout: lane holds column (lane & 15), rows (lane >> 4) + 4 r
    if constexpr (MODE == PZ_EPI_SYM) {
        double* S = ep.slab + (long)ks * ep.M * ep.M;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = row0 + wr * 32 + mb * 16 + fk + 4 * r, col = col0 + wc * 32 + nb * 16 + fi;
                    if (row < Mr && col < Nc) {
                        S[(long)row * ep.M + col] = acc[mb][nb][r];
                        S[(long)col * ep.M + row] = acc[mb][nb][r];
                    }
                }
        if (diag && tid < PZ_T && row0 + tid < Mr) ep.bpart[(long)ks * ep.M + row0 + tid] = bacc;
    } else if constexpr (MODE == PZ_EPI_ROW4) {
        double rs[2][4][4];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int q = 0; q < 4; ++q) rs[mb][r][q] = 0.0;
                const int row = row0 + wr * 32 + mb * 16 + fk + 4 * r;
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const int col = col0 + wc * 32 + nb * 16 + fi;
                    if (row < Mr && col < Nc) ep.row4(row, col, acc[mb][nb][r], rs[mb][r]);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    double v = rs[mb][r][q];
                    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
                    rs[mb][r][q] = v;
                }
            }
        if (fi == 0) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int q = 0; q < 4; ++q) red[wave][mb * 16 + fk + 4 * r][q] = rs[mb][r][q];
        }
        __syncthreads();
        const int lr = tid >> 2, q = tid & 3;                   // 64 rows x 4 quantities, the two column halves in fixed order
        const int w0 = (lr >> 5) * 2;
        const int row = row0 + lr;
        racc += red[w0][lr & 31][q] + red[w0 + 1][lr & 31][q];
        if (tn == tn_last && row < Mr) ep.part[((long)(tn_first / tn_per) * ep.M + row) * 4 + q] = racc;
    } else {
        double cs[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int col = col0 + wc * 32 + nb * 16 + fi;
            double v = 0.0;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = row0 + wr * 32 + mb * 16 + fk + 4 * r;
                    if (row < Mr && col < Nc) v += ep.col1(row, col, acc[mb][nb][r]);
                }
            v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
            cs[nb] = v;
        }
        double* redc = &red[0][0][0];                           // [2 row halves][64 columns]
        if (fk == 0) {
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) redc[wr * 64 + wc * 32 + nb * 16 + fi] = cs[nb];
        }
        __syncthreads();
        if (tid < PZ_T && col0 + tid < Nc) ep.part[(long)tm * ep.ncol + col0 + tid] = redc[tid] + redc[64 + tid];
    }
  }
}

template <int MODE, class OA, class OB, class EP>
static hipError_t pz_gen_gemm(const OA& oa, const OB& ob, const EP& ep, int Mr, int Nc, int K, int nsplit, bool tri, hipStream_t st,
                              int tn_per = 1, const int* skip = nullptr) {
    const int tiles_m = (Mr + PZ_T - 1) / PZ_T, tiles_n = (Nc + PZ_T - 1) / PZ_T;
    const int kchunk = (((K + nsplit - 1) / nsplit) + PZ_BK - 1) / PZ_BK * PZ_BK;
    const int ntiles = tri ? tiles_n * (tiles_n + 1) / 2 : tiles_m * ((tiles_n + tn_per - 1) / tn_per);
    hipLaunchKernelGGL((pz_gen_gemm_kernel<MODE, OA, OB, EP>), dim3((unsigned)ntiles, (unsigned)nsplit), dim3(256), 0, st, oa, ob, ep,
                       Mr, Nc, K, kchunk, tiles_n, tri ? 1 : 0, tn_per, skip);
    return hipGetLastError();
}

#define PZ_LAUNCH1D(kern, n, st, ...) \
    hipLaunchKernelGGL(kern, dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, st, __VA_ARGS__)

// fixed-order block sum of 256 threads (every thread returns the total)
__device__ __forceinline__ double pz_block_sum(double v, double* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) sh[tid] += sh[tid + off];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// mean[p] = w sum_i g(i, p) alpha_i
template <class G>
__global__ __launch_bounds__(256) void pz_mean_kernel(const G g, const double* alpha, int M, double w, double* mean) {   // block per output
    __shared__ double sh[256];
    const int p = blockIdx.x;
    double acc = 0.0;
    for (int i = threadIdx.x; i < M; i += 256) acc += g.val(i, p) * alpha[i];
    acc = pz_block_sum(acc, sh);
    if (threadIdx.x == 0) mean[p] = w * acc;
}
// psd_safe_cholesky's float64 jitter schedule (0, 1e-8, 1e-7, 1e-6) on the matrix a dense step factors first: attempt(first) runs the
// whole step at *eps (first: nothing of an earlier level can be reused), synchronises, and returns a negative VGGP_E* code, 1 when
// that factorisation failed at this level, 0 when it went through.  *failed: it failed at every level.
template <class F>
static int pz_jitter_retry(double* eps, int* failed, F attempt) {
    static const double JIT[4] = {0.0, 1e-8, 1e-7, 1e-6};
    for (int lvl = 0; lvl < 4; ++lvl) {
        *eps = JIT[lvl];
        const int rc = attempt(lvl == 0);
        if (rc < 0) return rc;
        *failed = rc;
        if (!rc) break;
    }
    return VGGP_OK;
}
