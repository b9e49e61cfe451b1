// Joint samples on the DENSE M-space states (vggp_elbo_step_masked, vggp_elbo_step_scattered): the whitened coefficient draw from the
// inverse factor the step keeps.  The blocked Cholesky of the step (masked.hip vg_blocked_chol_inverse) leaves w.Lg = L with
// Sigma~ = L L^T and w.Xg = L^-1, lower triangular with true zeros above its diagonal; no read-out writes either.  With E_s standard
// normal over the M = m1 m2 cells
//     X_s = Xg^T E_s,     Cov(vec X_s) = Xg^T Xg = Sigma~^-1 (= w.Sinv),
// the draw the full-grid sampler takes from the Kronecker eigenbasis and the iterative samplers from a block PCG solve -- here one
// skinny, transposed, triangular product (vg_tri_t_kernel): no factorisation, no solve, no tolerance, no M x M temporary.  Everything
// after X_s is the other samplers' code: L0_1 X L0_2^T and vg_sample_out_launch for q(v) (vggp_qv_sample_masked, below), vg_rs_setup
// and vg_rs_block_out for the raster (vggp_posterior_raster_sample_masked, raster_sample.hip).
// Specification: tests/dense_sample_spec.py.
#include "mspace_ws.h"

#include <cstdlib>

typedef double vt_d4 __attribute__((ext_vector_type(4)));

#define VT_TW 32                  // columns of Xl per tile: 2 MFMA column blocks; M = 16384 gives 512 tiles = 256 mirror pairs, one per CU
#define VT_BK 64                  // rows of Xl per k-slab
#define VT_NC 64                  // sample columns per launch: 4 MFMA row blocks, one per wave
#define VT_BLD (VT_TW + 16)       // LDS row of the Xl slab [k][u]: 48 doubles, so rows k and k + 1 of a half-wave's B fragment (2 x 16
                                  // consecutive doubles) fall on the two halves of the 64 banks
#define VT_ELD (VT_BK + 2)        // LDS row of the E slab [c][k]: 66 doubles = 132 dwords, so the 16 rows x 2 k of a half-wave's A fragment
                                  // fall on 32 distinct 8-byte banks (row stride 4 dwords mod 64)

// out(u, c) = sum_{k >= u} Xl[k][u] E(k, c) for c < cn, zeros for cn <= c < nbc.  Xl [M][M] row-major, lower triangular: NOTHING above
// its diagonal is read.  E, out: block vectors [m1][nbc][m2], element (cell u = i1 m2 + i2, column c) at (i1 nbc + c) m2 + i2.
// As an MFMA product D = A B: A[c][k] = E(k, c) (the sample columns: rows of D), B[k][u] = Xl[k][u] (a 32-column tile of Xl: columns
// of D) -- row k of Xl is contiguous along u, so the slab streams in 256-byte runs.  Workgroup b takes column tile b and its mirror
// nt - 1 - b, the long one first: the triangle makes tile t stream M - 32 t rows, a pair streams 2 M - 32 (nt - 1) whatever b.  Four
// waves; wave w owns sample columns 16 w .. 16 w + 15 against the tile's 32 columns of Xl (two accumulators), so every output element
// is summed by ONE wave in ascending k from k = 32 t: no split-K, no atomics, and the bits of a sample depend neither on its column
// in the block nor on cn or nbc (a wave whose columns are all >= cn skips its products and stores zeros).  Per slab of 64 rows the
// workgroup stages Xl[k0 .. k0 + 63][tile] and E(k0 .. k0 + 63, all c) in LDS, the next slab's global loads in flight while this
// one is multiplied.  Edges: rows k >= M, columns u >= M, k < u (the triangle inside the first slab) and c >= cn are staged as zeros,
// nothing is padded or copied; a tile that straddles an i1 boundary of the interleaved layout stores each element at its own
// (i1, i2).  Indices into Xl, E and out are 64-bit.
__global__ __launch_bounds__(256) void vg_tri_t_kernel(const double* __restrict__ Xl, long M, int m2, const double* __restrict__ E, int nbc, int cn,
                                                       double* __restrict__ out, int nt) {
    __shared__ double Bs[VT_BK * VT_BLD], Es[VT_NC * VT_ELD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 15, fk = lane >> 4;
    // Xl slab: thread (bj = tid & 31, br = tid >> 5) moves elements (k = br + 8 r, u = bj), r = 0 .. 7
    const int bj = tid & 31, br = tid >> 5;
    // E slab: thread (ek = tid & 63, wave) moves elements (k = ek, c = wave + 4 r), r = 0 .. 15
    const int ek = lane;
    const bool live = wave * 16 < cn;                 // this wave has sample columns to sum
    const int t_hi = nt - 1 - (int)blockIdx.x;
    for (int half = 0; half < 2; ++half) {
        const int t = half == 0 ? (int)blockIdx.x : t_hi;
        if (half == 1 && t_hi == (int)blockIdx.x) break;      // odd tile count: the middle tile has no partner
        const long u0 = (long)t * VT_TW;
        const long ub = u0 + bj;
        const bool ubok = ub < M;
        double rb[8], re[16];
        vt_d4 acc[2];
        acc[0] = (vt_d4){0.0, 0.0, 0.0, 0.0};
        acc[1] = (vt_d4){0.0, 0.0, 0.0, 0.0};
        auto load = [&](long k0) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const long k = k0 + br + 8 * r;
                rb[r] = (ubok && k < M && k >= ub) ? Xl[k * M + ub] : 0.0;
            }
            const long k = k0 + ek;
            const bool kok = k < M;
            const long i1 = kok ? k / m2 : 0, i2 = kok ? k - i1 * m2 : 0;
            const double* pe = E + (i1 * nbc) * m2 + i2;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = wave + 4 * r;
                re[r] = (kok && c < cn) ? pe[(long)c * m2] : 0.0;
            }
        };
        load(u0);
        for (long k0 = u0; k0 < M; k0 += VT_BK) {
#pragma unroll
            for (int r = 0; r < 8; ++r) Bs[(br + 8 * r) * VT_BLD + bj] = rb[r];
#pragma unroll
            for (int r = 0; r < 16; ++r) Es[(wave + 4 * r) * VT_ELD + ek] = re[r];
            __syncthreads();
            if (k0 + VT_BK < M) load(k0 + VT_BK);
            if (live) {
#pragma unroll
                for (int kk = 0; kk < VT_BK; kk += 4) {
                    const double fa = Es[(wave * 16 + fi) * VT_ELD + kk + fk];
                    const double fb0 = Bs[(kk + fk) * VT_BLD + fi], fb1 = Bs[(kk + fk) * VT_BLD + 16 + fi];
                    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fb0, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fb1, acc[1], 0, 0, 0);
                }
            }
            __syncthreads();
        }
        // C/D fragment of the fp64 MFMA: column (u) = lane & 15, row (c) = (lane >> 4) + 4 * reg
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const long u = u0 + nb * 16 + fi;
            if (u >= M) continue;
            const long i1 = u / m2, i2 = u - i1 * m2;
            double* po = out + (i1 * nbc) * m2 + i2;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = wave * 16 + fk + 4 * r;
                if (c < nbc) po[(long)c * m2] = c < cn ? acc[nb][r] : 0.0;
            }
        }
    }
}

hipError_t vg_tri_t_apply_launch(const double* Xl, long m1, long m2, const double* E, int nbc, int cn, double* out, hipStream_t st) {
    const long M = m1 * m2;
    if (m1 < 1 || m2 < 1 || M > VGM_MAX_M || cn < 1 || cn > nbc || nbc > VT_NC || out == E) return hipErrorInvalidValue;
    const int nt = (int)((M + VT_TW - 1) / VT_TW);
    hipLaunchKernelGGL(vg_tri_t_kernel, dim3((unsigned)((nt + 1) / 2)), dim3(256), 0, st, Xl, M, (int)m2, E, nbc, cn, out, nt);
    return hipGetLastError();
}

// the same product through the batch GEMM and its 128-granular triangular skip (VG_TRI_B_LOWER): C[c][u] = sum_k E(k, c) Xl[k][u].
// The yardstick of tools/bench_dense_sample.py, selected by VGGP_TRI_T_GEMM=1 in the environment of a vggp_tri_t_apply call; m1 = 1
// only (there the interleaved layout is the plain [nbc][M] the GEMM writes).  Not a route any sampler takes.
static int vg_tri_t_gemm(const double* Xl, long M, const double* E, int nbc, int cn, double* out, hipStream_t st) {
    if (cn < nbc) VG_HIP(hipMemsetAsync(out + (long)cn * M, 0, sizeof(double) * (size_t)(nbc - cn) * M, st));
    VgGemmBatch g;
    vg_gemm_init(&g);
    const int i = vg_gemm_add(&g, E, M, 1, Xl, M, 1, out, (int)M, cn, (int)M, (int)M);
    g.p[i].tri = VG_TRI_B_LOWER;
    VG_HIP(vg_gemm_launch(&g, st));
    return VGGP_OK;
}

extern "C" int vggp_tri_t_apply(vggp_ctx* c, const double* Xl, int64_t m1, int64_t m2, const double* E, int nbc, int cn, double* out,
                                void* stream) {
    static const char* fn = "vggp_tri_t_apply";
    if (!c) { vg_set_error("%s: null context", fn); return VGGP_EINVAL; }
    VG_REQUIRE(Xl && E && out, "%s: null argument", fn);
    VG_REQUIRE(m1 >= 1 && m2 >= 1 && m1 <= VGM_MAX_M && m2 <= VGM_MAX_M && m1 * m2 <= VGM_MAX_M, "%s: need 1 <= m1 m2 <= %d", fn, VGM_MAX_M);
    VG_REQUIRE(cn >= 1 && cn <= nbc && nbc <= VT_NC, "%s: need 1 <= cn <= nbc <= 64 (got cn = %d, nbc = %d)", fn, cn, nbc);
    VG_REQUIRE(out != E, "%s: the product cannot run in place (out == E)", fn);
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    const char* env = getenv("VGGP_TRI_T_GEMM");
    if (env && env[0] == '1') {
        VG_REQUIRE(m1 == 1, "%s: VGGP_TRI_T_GEMM=1 (the batch GEMM as yardstick) serves m1 = 1 only", fn);
        return vg_tri_t_gemm(Xl, (long)m2, E, nbc, cn, out, st);
    }
    VG_HIP(vg_tri_t_apply_launch(Xl, (long)m1, (long)m2, E, nbc, cn, out, st));
    return VGGP_OK;
}

// What the two samplers of a dense state check, in this order, before anything is launched or written: the sample arguments, then the
// state (the context is planned, single-rank and not paired here)
int vg_dense_sample_enter(vggp_ctx* c, const char* fn, int64_t n_samples, int64_t first, const void* out, int block, vggp_info* info) {
    VG_REQUIRE(n_samples >= 1 && n_samples < (1LL << 31), "%s: n_samples = %lld must be at least 1", fn, (long long)n_samples);
    VG_REQUIRE(first >= 0 && out, "%s: bad argument", fn);
    VG_REQUIRE(block <= 64, "%s: block = %d exceeds 64 samples per block", fn, block);
    if (!(c->last_kind == VG_LAST_DENSE && c->have_masked && c->masked)) {
        vg_set_error("%s: the last finished step on this context is no dense masked / scattered step (vggp_elbo_step_masked, "
                     "vggp_elbo_step_scattered)", fn);
        return VGGP_ESTATE;
    }
    if (info) { info->jitter1 = info->jitter2 = 0.0; info->sweeps1 = info->sweeps2 = info->rounds1 = info->rounds2 = 0; info->status = 0; info->polished = 0; }
    return VGGP_OK;
}

// q(v): V_s = mean + sqrt(s1^e1 s2^e2) L0_1 X_s L0_2^T with the mean of vggp_qv_masked (the same launches, the same bits) and the tail
// of the iterative sampler (vgi_sample_run).  E, X and the two products: 4 M nbc doubles of the samplers' own scratch, the mean behind
extern "C" int vggp_qv_sample_masked(vggp_ctx* c, int64_t n_samples, uint64_t seed, int64_t first, const double* eps_u, int block, double* out,
                                     vggp_info* info, void* stream) {
    static const char* fn = "vggp_qv_sample_masked";
    VG_NOT_PAIRED(c, fn);
    if (!c || !c->planned) { vg_set_error("%s: context not planned", fn); return VGGP_ESTATE; }
    VG_REQUIRE(!vgi_multi(c), "%s: joint samples run on single-rank contexts only (this context is multi-rank)", fn);
    int rc = vg_dense_sample_enter(c, fn, n_samples, first, out, block, info);
    if (rc) return rc;
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    VgDim &d1 = c->d[0], &d2 = c->d[1];
    const int m1 = w.m1, m2 = w.m2, e1 = vg_uexp(d1.basis), e2 = vg_uexp(d2.basis);
    const long M = w.M;
    const int nbc = (int)std::min<int64_t>(block > 0 ? block : 64, n_samples);
    const long nb = M * nbc;
    if ((rc = vg_rs_reserve(c, fn, (size_t)(4 * nb + M) * sizeof(double), nbc))) return rc;
    double* p = (double*)c->rs_mem;
    double* Eb = p; p += nb;
    double* Xb = p; p += nb;
    double* Tm = p; p += nb;
    double* Tm2 = p; p += nb;
    double* mean = p;
    if ((rc = vgi_qv_mean(c, w, mean, st))) return rc;
    for (int64_t off = 0; off < n_samples; off += nbc) {
        const int cn = (int)std::min<int64_t>(nbc, n_samples - off);
        VG_HIP(vg_sample_block_noise_launch(Eb, eps_u ? eps_u + off * M : nullptr, seed, (unsigned long long)(first + off), m1, nbc, m2, cn, st));
        VG_HIP(vg_tri_t_apply_launch(w.Xg, m1, m2, Eb, nbc, cn, Xb, st));                                          // X = Xg^T E
        if ((rc = gemm1(d1.L0, m1, 1, Xb, (long)nbc * m2, 1, Tm, nbc * m2, m1, nbc * m2, m1, st))) return rc;      // L0_1 X
        if ((rc = gemm1(Tm, m2, 1, d2.L0, 1, m2, Tm2, m2, m1 * nbc, m2, m2, st))) return rc;                       // (.) L0_2^T
        VG_HIP(vg_sample_out_launch(Tm2, mean, c->theta, e1, e2, m1, nbc, m2, cn, out + off * M, st));
    }
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}
