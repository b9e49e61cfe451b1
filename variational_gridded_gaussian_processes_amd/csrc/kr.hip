// The Khatri-Rao operator of the iterative scattered step (iter_step.hip, vggp_elbo_step_scattered_iter): with one column of
// L (m1 x N) and R (m2 x N) per POINT and block vectors V [m1][nb][m2],
//     field   F[c][k]      = sum_a L[a][k] sum_b V[a][c][b] R[b][k]         (the per-point scalars l_k^T V_c r_k)
//     back    out[a][c][b] = sum_k L[a][k] F[c][k] R[b][k]
// Both are fp64-MFMA GEMMs (64 x 64 tiles, 16-deep k-tiles, 2 x 2 waves of 32 x 32, the register-staged pipeline of gemm_body.h)
// whose large intermediate never leaves the workgroup:
//   field   the (m1 nb) x N product V R is multiplied by L[a][k] and summed over a in the epilogue of every 64-row tile: a
//           workgroup owns 64 points and VG_KR_CG columns c (2 in the read-outs' instantiation) and walks ALL rows a, so F is written
//           once and m1 x nb x N never exists
//   back    the B operand F[c][k] R[b][k] is formed as the fragment is read from LDS; the L and R tiles of a k-tile are staged
//           once for VG_KR_CG columns.  The reduction over the points is split over workgroups (slabs summed in fixed order by
//           vg_red_launch): no atomics, bitwise reproducible.
#include "ctx.h"
#include "gemm_body.h"

#define VG_KR_T 64
#define VG_KR_BK 16
#define VG_KR_RS (VG_KR_BK + 1)        // K-contiguous operand in LDS: [row][BK + 1]
#define VG_KR_KS (VG_KR_T + 16)        // point-contiguous operand in LDS: [k][T + 16]
#define VG_KR_CG 4                     // columns c per workgroup

struct VgKrArgs {
    const double* L;      // [m1][N]
    const double* R;      // [m2][N]
    const double* V;      // field: [m1][nb][m2] (input)
    double* F;            // field: [nb][N] (output) / back: input
    double* out;          // back: [m1][nb][m2], slab s at out + s * slab
    long N, slab;
    int m1, m2, nb;
    int ksplit, kchunk;   // back: slabs and points per slab (multiple of VG_KR_BK)
    int tiles_a, tiles_b;
};

// The body for CG columns per workgroup.  A column's accumulators, k order, epilogue and butterfly do not depend on CG, so every
// instantiation writes the same bits.
template <int CG>
__device__ __forceinline__ void vg_kr_field_body(const VgKrArgs& A) {
    __shared__ double As[CG][VG_KR_T * VG_KR_RS];
    __shared__ double Bs[VG_KR_BK * VG_KR_KS];
    __shared__ double red[CG][2][VG_KR_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int fi = lane & 15, fk = lane >> 4;
    const int m1 = A.m1, m2 = A.m2, nb = A.nb;
    const long N = A.N, k0 = (long)blockIdx.x * VG_KR_T;
    const int c0 = blockIdx.y * CG;
    const int nc = min(CG, nb - c0);
    const int nat = (m1 + VG_KR_T - 1) / VG_KR_T, nbt = (m2 + VG_KR_BK - 1) / VG_KR_BK, nit = nat * nbt;
    // staging map: V tile [64 a][16 b] is b-contiguous, R tile [16 b][64 k] is k-contiguous; 4 elements per thread and operand
    const int va_b = tid & 15, va_i = tid >> 4;            // rows va_i + 16 r
    const int rb_j = tid & 63, rb_k = tid >> 6;            // k-rows rb_k + 4 r
    const long kcol = k0 + rb_j;
    const bool kok = kcol < N;
    const long kcl = kok ? kcol : N - 1;
    double ra[CG][4], rb[4];
    auto load = [&](int it) {
        const int at = it / nbt, bt = it - at * nbt;
        const int gb = bt * VG_KR_BK + va_b;
        const bool bok = gb < m2;
        const int gbc = bok ? gb : m2 - 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ga = at * VG_KR_T + va_i + 16 * r;
            const bool ok = bok && ga < m1;
            const int gac = ga < m1 ? ga : m1 - 1;
#pragma unroll
            for (int cc = 0; cc < CG; ++cc) {
                const int c = cc < nc ? c0 + cc : c0;
                const double v = A.V[((long)gac * nb + c) * m2 + gbc];
                ra[cc][r] = ok ? v : 0.0;
            }
            const int gk = bt * VG_KR_BK + rb_k + 4 * r;
            const int gkc = gk < m2 ? gk : m2 - 1;
            const double w = A.R[(long)gkc * N + kcl];
            rb[r] = (gk < m2 && kok) ? w : 0.0;
        }
    };
    vg_d4 acc[CG][2][2];
    double fsum[CG][2];
#pragma unroll
    for (int cc = 0; cc < CG; ++cc) {
        fsum[cc][0] = fsum[cc][1] = 0.0;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[cc][i][j] = (vg_d4){0.0, 0.0, 0.0, 0.0};
    }
    load(0);
    for (int it = 0; it < nit; ++it) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int cc = 0; cc < CG; ++cc) As[cc][(va_i + 16 * r) * VG_KR_RS + va_b] = ra[cc][r];
            Bs[(rb_k + 4 * r) * VG_KR_KS + rb_j] = rb[r];
        }
        __syncthreads();
        if (it + 1 < nit) load(it + 1);
#pragma unroll
        for (int kk = 0; kk < VG_KR_BK; kk += 4) {
            double bv[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = Bs[(kk + fk) * VG_KR_KS + wc * 32 + j * 16 + fi];
#pragma unroll
            for (int cc = 0; cc < CG; ++cc) {
                if (cc < nc) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const double av = As[cc][(wr * 32 + i * 16 + fi) * VG_KR_RS + kk + fk];
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[cc][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[j], acc[cc][i][j], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
        const int at = it / nbt;
        if (it - at * nbt == nbt - 1) {          // the 64-row tile is complete: times L[a][k], summed over its rows, accumulators cleared
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const long k = k0 + wc * 32 + j * 16 + fi;
                const long kc = k < N ? k : N - 1;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int a = at * VG_KR_T + wr * 32 + i * 16 + fk + 4 * r;
                        const double l = A.L[(long)(a < m1 ? a : m1 - 1) * N + kc];
                        const double lw = a < m1 ? l : 0.0;
#pragma unroll
                        for (int cc = 0; cc < CG; ++cc) {
                            fsum[cc][j] += lw * acc[cc][i][j][r];
                            acc[cc][i][j][r] = 0.0;
                        }
                    }
            }
        }
    }
    // rows of a 16 x 16 block live in the four lane groups fk: butterfly over them, then the two row-halves of the wave grid
#pragma unroll
    for (int cc = 0; cc < CG; ++cc)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double s = fsum[cc][j];
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            if (fk == 0) red[cc][wr][wc * 32 + j * 16 + fi] = s;
        }
    __syncthreads();
    if (tid < VG_KR_T && k0 + tid < N)
        for (int cc = 0; cc < nc; ++cc) A.F[(long)(c0 + cc) * N + k0 + tid] = red[cc][0][tid] + red[cc][1][tid];
}

__global__ __launch_bounds__(256) void vg_kr_field_kernel(const VgKrArgs A) { vg_kr_field_body<VG_KR_CG>(A); }
// Two columns per workgroup: half the accumulators and staging registers (126 VGPRs, no AGPRs, 29 KB LDS), so several waves share a SIMD
// and hide each other's LDS round trip where the 4-column instantiation runs one wave per SIMD.  The read-outs' block solves use it
// (vgi_readout_solve); measured at 2.2 x the 4-column rate at 16 and at 64 columns.
__global__ __launch_bounds__(256, 2) void vg_kr_field2_kernel(const VgKrArgs A) { vg_kr_field_body<2>(A); }

__global__ __launch_bounds__(256) void vg_kr_back_kernel(const VgKrArgs A) {
    __shared__ double As[VG_KR_T * VG_KR_RS];              // L tile [64 a][16 k]
    __shared__ double Bs[VG_KR_T * VG_KR_RS];              // R tile [64 b][16 k]
    __shared__ double Fs[VG_KR_CG][VG_KR_BK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int fi = lane & 15, fk = lane >> 4;
    const int m1 = A.m1, m2 = A.m2, nb = A.nb;
    const long N = A.N;
    int t = blockIdx.x;
    const int tb = t % A.tiles_b; t /= A.tiles_b;
    const int ta = t % A.tiles_a; t /= A.tiles_a;
    const int ks = t;
    const int c0 = blockIdx.y * VG_KR_CG;
    const int nc = min(VG_KR_CG, nb - c0);
    const long kb = (long)ks * A.kchunk;
    const long ke = kb + A.kchunk < N ? kb + A.kchunk : N;
    const int nkt = (int)((ke - kb + VG_KR_BK - 1) / VG_KR_BK);
    const int s_k = tid & 15, s_i = tid >> 4;              // both tiles are k-contiguous: rows s_i + 16 r
    double ra[4], rb[4], rf = 0.0;
    auto load = [&](int kt) {
        const long gk = kb + (long)kt * VG_KR_BK + s_k;
        const bool kok = gk < ke;
        const long gkc = kok ? gk : ke - 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ga = ta * VG_KR_T + s_i + 16 * r, gb = tb * VG_KR_T + s_i + 16 * r;
            const double l = A.L[(long)(ga < m1 ? ga : m1 - 1) * N + gkc];
            const double w = A.R[(long)(gb < m2 ? gb : m2 - 1) * N + gkc];
            ra[r] = (kok && ga < m1) ? l : 0.0;
            rb[r] = (kok && gb < m2) ? w : 0.0;
        }
        if (tid < VG_KR_CG * VG_KR_BK) {
            const int cc = tid >> 4;
            const double f = A.F[(long)(cc < nc ? c0 + cc : c0) * N + gkc];
            rf = (kok && cc < nc) ? f : 0.0;
        }
    };
    vg_d4 acc[VG_KR_CG][2][2];
#pragma unroll
    for (int cc = 0; cc < VG_KR_CG; ++cc)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[cc][i][j] = (vg_d4){0.0, 0.0, 0.0, 0.0};
    if (nkt > 0) load(0);
    for (int kt = 0; kt < nkt; ++kt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            As[(s_i + 16 * r) * VG_KR_RS + s_k] = ra[r];
            Bs[(s_i + 16 * r) * VG_KR_RS + s_k] = rb[r];
        }
        if (tid < VG_KR_CG * VG_KR_BK) Fs[tid >> 4][tid & 15] = rf;
        __syncthreads();
        if (kt + 1 < nkt) load(kt + 1);
#pragma unroll
        for (int kk = 0; kk < VG_KR_BK; kk += 4) {
            double av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = As[(wr * 32 + i * 16 + fi) * VG_KR_RS + kk + fk];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = Bs[(wc * 32 + j * 16 + fi) * VG_KR_RS + kk + fk];
#pragma unroll
            for (int cc = 0; cc < VG_KR_CG; ++cc) {
                if (cc < nc) {
                    const double f = Fs[cc][kk + fk];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const double bf = bv[j] * f;          // the B operand F[c][k] R[b][k], formed here
#pragma unroll
                        for (int i = 0; i < 2; ++i) acc[cc][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bf, acc[cc][i][j], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }
    double* out = A.out + (long)ks * A.slab;
#pragma unroll
    for (int cc = 0; cc < VG_KR_CG; ++cc) {
        if (cc < nc) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int a = ta * VG_KR_T + wr * 32 + i * 16 + fk + 4 * r;
                        const int b = tb * VG_KR_T + wc * 32 + j * 16 + fi;
                        if (a < m1 && b < m2) out[((long)a * nb + c0 + cc) * m2 + b] = acc[cc][i][j][r];
                    }
        }
    }
}

hipError_t vg_kr_field_launch(const double* L, const double* R, const double* V, int m1, int m2, long N, int nb, double* F, hipStream_t st) {
    VgKrArgs a{};
    a.L = L; a.R = R; a.V = V; a.F = F; a.N = N; a.m1 = m1; a.m2 = m2; a.nb = nb;
    hipLaunchKernelGGL(vg_kr_field_kernel, dim3((unsigned)((N + VG_KR_T - 1) / VG_KR_T), (unsigned)((nb + VG_KR_CG - 1) / VG_KR_CG)), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t vg_kr_field2_launch(const double* L, const double* R, const double* V, int m1, int m2, long N, int nb, double* F, hipStream_t st) {
    VgKrArgs a{};
    a.L = L; a.R = R; a.V = V; a.F = F; a.N = N; a.m1 = m1; a.m2 = m2; a.nb = nb;
    hipLaunchKernelGGL(vg_kr_field2_kernel, dim3((unsigned)((N + VG_KR_T - 1) / VG_KR_T), (unsigned)((nb + 1) / 2)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// slabs of the split reduction: enough workgroups for ~4 per CU, never more than VG_KR_MAXSPLIT and never shorter than 256 points
#define VG_KR_MAXSPLIT 64
static int kr_back_split(int m1, int m2, long N, int nb) {
    const long wg = (long)((m1 + VG_KR_T - 1) / VG_KR_T) * ((m2 + VG_KR_T - 1) / VG_KR_T) * ((nb + VG_KR_CG - 1) / VG_KR_CG);
    long ks = (1024 + wg - 1) / wg;
    if (ks > VG_KR_MAXSPLIT) ks = VG_KR_MAXSPLIT;
    if (ks > N / 256) ks = N / 256;
    return ks < 1 ? 1 : (int)ks;
}
size_t vg_kr_back_scratch(int m1, int m2, long N, int nb) {          // doubles; bounded by VG_KR_MAXSPLIT * m1 * nb * m2 whatever N
    const int ks = kr_back_split(m1, m2, N, nb);
    return ks > 1 ? (size_t)ks * m1 * nb * m2 : 0;
}
hipError_t vg_kr_back_launch(const double* L, const double* R, const double* F, int m1, int m2, long N, int nb, double* out, double* scratch,
                             hipStream_t st) {
    VgKrArgs a{};
    a.L = L; a.R = R; a.F = const_cast<double*>(F); a.N = N; a.m1 = m1; a.m2 = m2; a.nb = nb;
    a.tiles_a = (m1 + VG_KR_T - 1) / VG_KR_T; a.tiles_b = (m2 + VG_KR_T - 1) / VG_KR_T;
    int ks = kr_back_split(m1, m2, N, nb);
    long chunk = ((N + ks - 1) / ks + VG_KR_BK - 1) / VG_KR_BK * VG_KR_BK;
    ks = (int)((N + chunk - 1) / chunk);
    a.ksplit = ks; a.kchunk = (int)chunk;
    a.slab = (long)m1 * nb * m2;
    a.out = ks > 1 ? scratch : out;
    hipLaunchKernelGGL(vg_kr_back_kernel, dim3((unsigned)(a.tiles_a * a.tiles_b * ks), (unsigned)((nb + VG_KR_CG - 1) / VG_KR_CG)), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || ks == 1) return e;
    VgRedBatch r;
    vg_red_init(&r);
    vg_red_add(&r, scratch, out, a.slab, a.slab, ks);
    return vg_red_launch(&r, st);
}

// ---- squared Gram product of the gridded read-out (vggp_readout_scattered_iter, literal variance) -------------------------------------
//     out[a][b] = sum_k P1[a][k]^2 P2[b][k]^2          P1 [mv1][N], P2 [mv2][N], any mv_d >= 1
// The back kernel's GEMM with one column and F = 1: 64 x 64 tiles, 16-deep k-tiles, both operands k-contiguous ([row][BK + 1] in LDS),
// the operands squared as the fragments are read from LDS (no squared copy exists) and two register stages in flight as in
// gemm_body.h.  The reduction over the points is split over workgroups when the output has few tiles; the slabs are summed in fixed
// order (and, with accum, on top of what out already holds -- the chunks of a long point list): no atomics, bitwise reproducible.
struct VgKrSqArgs {
    const double* P1;
    const double* P2;
    double* out;          // slab s at out + s * slab
    long N, slab;
    int mv1, mv2, kchunk, tiles_a, tiles_b;
};

__global__ __launch_bounds__(256) void vg_kr_sqgram_kernel(const VgKrSqArgs A) {
    __shared__ double As[VG_KR_T * VG_KR_RS];
    __shared__ double Bs[VG_KR_T * VG_KR_RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int fi = lane & 15, fk = lane >> 4;
    const int mv1 = A.mv1, mv2 = A.mv2;
    const long N = A.N;
    int t = blockIdx.x;
    const int tb = t % A.tiles_b; t /= A.tiles_b;
    const int ta = t % A.tiles_a; t /= A.tiles_a;
    const int ks = t;
    const long kb = (long)ks * A.kchunk;
    const long ke = kb + A.kchunk < N ? kb + A.kchunk : N;
    const int nkt = ke > kb ? (int)((ke - kb + VG_KR_BK - 1) / VG_KR_BK) : 0;
    const int s_k = tid & 15, s_i = tid >> 4;              // both tiles are k-contiguous: rows s_i + 16 r
    const double* pa[4];
    const double* pb[4];
    bool aok[4], bok[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ga = ta * VG_KR_T + s_i + 16 * r, gb = tb * VG_KR_T + s_i + 16 * r;
        aok[r] = ga < mv1; bok[r] = gb < mv2;
        pa[r] = A.P1 + (long)(aok[r] ? ga : mv1 - 1) * N;
        pb[r] = A.P2 + (long)(bok[r] ? gb : mv2 - 1) * N;
    }
    double ra0[4], rb0[4], ra1[4], rb1[4];
    auto load = [&](int kt, double (&ra)[4], double (&rb)[4]) {
        const long gk = kb + (long)kt * VG_KR_BK + s_k;
        const bool kok = gk < ke;
        const long gkc = kok ? gk : ke - 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double l = pa[r][gkc], w = pb[r][gkc];
            ra[r] = (kok && aok[r]) ? l : 0.0;
            rb[r] = (kok && bok[r]) ? w : 0.0;
        }
    };
    vg_d4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (vg_d4){0.0, 0.0, 0.0, 0.0};
    auto ktile = [&](double (&ra)[4], double (&rb)[4], int knext) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            As[(s_i + 16 * r) * VG_KR_RS + s_k] = ra[r];
            Bs[(s_i + 16 * r) * VG_KR_RS + s_k] = rb[r];
        }
        __syncthreads();
        if (knext < nkt) load(knext, ra, rb);                 // refill this stage: two k-tiles ahead
#pragma unroll
        for (int kk = 0; kk < VG_KR_BK; kk += 4) {
            double av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const double v = As[(wr * 32 + i * 16 + fi) * VG_KR_RS + kk + fk];
                av[i] = v * v;                                // the operands P1^2, P2^2, formed here
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const double v = Bs[(wc * 32 + j * 16 + fi) * VG_KR_RS + kk + fk];
                bv[j] = v * v;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    };
    if (nkt > 0) load(0, ra0, rb0);
    if (nkt > 1) load(1, ra1, rb1);
    for (int kt = 0; kt < nkt; kt += 2) {
        ktile(ra0, rb0, kt + 2);
        if (kt + 1 < nkt) ktile(ra1, rb1, kt + 3);
    }
    double* out = A.out + (long)ks * A.slab;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = ta * VG_KR_T + wr * 32 + i * 16 + fk + 4 * r;
                const int b = tb * VG_KR_T + wc * 32 + j * 16 + fi;
                if (a < mv1 && b < mv2) out[(long)a * mv2 + b] = acc[i][j][r];
            }
}

// out[i] = (accum ? out[i] : 0) + slab 0 + slab 1 + ...   (fixed order, as vg_red_kernel)
__global__ __launch_bounds__(256) void vg_kr_sqred_kernel(const double* in, double* out, long n, int nslab, int accum) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v = in[i];
    for (int k = 1; k < nslab; ++k) v += in[(long)k * n + i];
    out[i] = accum ? out[i] + v : v;
}

static int kr_sq_split(int mv1, int mv2, long N) {          // as kr_back_split: ~4 workgroups per CU, slabs of at least 256 points
    const long wg = (long)((mv1 + VG_KR_T - 1) / VG_KR_T) * ((mv2 + VG_KR_T - 1) / VG_KR_T);
    long ks = (1024 + wg - 1) / wg;
    if (ks > VG_KR_MAXSPLIT) ks = VG_KR_MAXSPLIT;
    if (ks > N / 256) ks = N / 256;
    return ks < 1 ? 1 : (int)ks;
}
size_t vg_kr_sqgram_scratch(int mv1, int mv2, long N) {     // doubles; at most (1024 / tiles + 1) * mv1 * mv2 whatever N
    return (size_t)kr_sq_split(mv1, mv2, N) * mv1 * mv2;
}
hipError_t vg_kr_sqgram_launch(const double* P1, const double* P2, int mv1, int mv2, long N, double* out, double* scratch, int accum,
                               hipStream_t st) {
    VgKrSqArgs a{};
    a.P1 = P1; a.P2 = P2; a.N = N; a.mv1 = mv1; a.mv2 = mv2;
    a.tiles_a = (mv1 + VG_KR_T - 1) / VG_KR_T; a.tiles_b = (mv2 + VG_KR_T - 1) / VG_KR_T;
    int ks = kr_sq_split(mv1, mv2, N);
    const long chunk = ((N + ks - 1) / ks + VG_KR_BK - 1) / VG_KR_BK * VG_KR_BK;
    ks = (int)((N + chunk - 1) / chunk);
    a.kchunk = (int)chunk;
    a.slab = (long)mv1 * mv2;
    const bool direct = ks == 1 && !accum;
    a.out = direct ? out : scratch;
    hipLaunchKernelGGL(vg_kr_sqgram_kernel, dim3((unsigned)(a.tiles_a * a.tiles_b * ks)), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || direct) return e;
    hipLaunchKernelGGL(vg_kr_sqred_kernel, dim3((unsigned)((a.slab + 255) / 256)), dim3(256), 0, st, scratch, out, a.slab, ks, accum);
    return hipGetLastError();
}

// ---- building blocks, exported for tests: the kernels above on caller-supplied device arrays -------------------------------------------
// what the three block-vector exports share: the checks, the device, the stream and the wait; launch(st) enqueues the kernel
template <class Launch>
static int vg_kr_export(vggp_ctx* c, const char* fn, bool non_null, int64_t m1, int64_t m2, int64_t N, int64_t nb, void* stream, Launch&& launch) {
    if (!c) { vg_set_error("%s: null context", fn); return VGGP_EINVAL; }
    VG_REQUIRE(non_null, "%s: null argument", fn);
    VG_REQUIRE(m1 >= 1 && m1 <= 256 && m2 >= 1 && m2 <= 256 && nb >= 1 && nb <= 64 && N >= 1 && N < (1L << 24),
               "%s: need 1 <= m_d <= 256, 1 <= nb <= 64, 1 <= N < 2^24", fn);
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const int rc = launch(st);
    if (rc) return rc;
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}
extern "C" int vggp_kr_field(vggp_ctx* c, const double* L, const double* R, const double* V, int64_t m1, int64_t m2, int64_t N, int64_t nb,
                             double* F, void* stream) {
    return vg_kr_export(c, "vggp_kr_field", L && R && V && F, m1, m2, N, nb, stream, [&](hipStream_t st) -> int {
        VG_HIP(vg_kr_field_launch(L, R, V, (int)m1, (int)m2, (long)N, (int)nb, F, st));
        return VGGP_OK;
    });
}
// the two-column instantiation of the field kernel (bitwise equal to vggp_kr_field; the read-outs' block solves run it)
extern "C" int vggp_kr_field2(vggp_ctx* c, const double* L, const double* R, const double* V, int64_t m1, int64_t m2, int64_t N, int64_t nb,
                              double* F, void* stream) {
    return vg_kr_export(c, "vggp_kr_field2", L && R && V && F, m1, m2, N, nb, stream, [&](hipStream_t st) -> int {
        VG_HIP(vg_kr_field2_launch(L, R, V, (int)m1, (int)m2, (long)N, (int)nb, F, st));
        return VGGP_OK;
    });
}
extern "C" int vggp_kr_back(vggp_ctx* c, const double* L, const double* R, const double* F, int64_t m1, int64_t m2, int64_t N, int64_t nb,
                            double* out, void* stream) {
    return vg_kr_export(c, "vggp_kr_back", L && R && F && out, m1, m2, N, nb, stream, [&](hipStream_t st) -> int {
        const size_t sc = vg_kr_back_scratch((int)m1, (int)m2, (long)N, (int)nb);
        const int rc = vg_ensure_misc(c, (sc + 32) * sizeof(double));
        if (rc) return rc;
        VG_HIP(vg_kr_back_launch(L, R, F, (int)m1, (int)m2, (long)N, (int)nb, out, (double*)c->misc, st));
        return VGGP_OK;
    });
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
