// Raster variance of posterior(x*) on the dense M-space states (masked / scattered): var = s1 s2 (1 - |t|^2 + t^T Sinv t) at the P1 x P2
// points of a raster.  Sinv is a dense M x M matrix (no Kronecker sum), but every raster column is rank one, t_ab = u1_a (x) u2_b, so
// the quadratic form is a four-index contraction done one axis at a time:
//     Gt[(j,l)][a] = sum_{i,k} U1[i][a] U1[k][a] Sinv[(i m2 + j) M + k m2 + l]        (m2^2 x P1,  K = m1^2)
//     quad[a][b]   = sum_{j,l} Gt[(j,l)][a] U2[j][b] U2[l][b]                          (P1 x P2,    K = m2^2)
// 2 P1 M^2 + 2 P1 P2 m2^2 flops instead of the 2 P1 P2 M^2 of the point-wise route.  Both stages are ONE kernel: a GEMM whose second
// operand is a Khatri-Rao self-product V[p][c] V[q][c] (k = p m + q), formed while its fragments are staged and never stored.
#include "mspace_ws.h"

typedef double vq_d4 __attribute__((ext_vector_type(4)));

#define VQ_T 64                   // output tile: 64 x 64, four waves 2 x 2, each 32 x 32 = 2 x 2 MFMA blocks (vg_raster_kernel's shape)
#define VQ_BK 16                  // k-tile
#define VQ_KS (VQ_T + 16)         // LDS row of a k-slice: 80 doubles, so the four k-rows of a fragment read fall on disjoint banks
#define VQ_MAXP (1L << 20)        // axis length limit of the entries

struct VqArgs {
    const double* A;              // plain: A(k, r) = A[k ldA + r];  view: A((i,k'), (j,l)) = A[(i m2 + j) Mv + k' m2 + l], r = j m2 + l
    long ldA, Mv;
    int m2;
    const double* V;              // [m][ldV], columns 0 .. C
    long ldV;
    int m, K;                     // K = m^2
    long R, C;                    // output rows / columns
    double* out;                  // [R][ldo]
    long ldo;
    const double *nr, *nc;        // epilogue: out = scale (kd - nr[r] nc[c] + acc)   (nr == NULL: no product; theta: scale *= theta[2] theta[3])
    double kd, scale;
    const double* theta;
    int tiles_n;
};

// out[r][c] = sum_{k = p m + q} A(k, r) V[p][c] V[q][c].  A k-slice of both operands is staged as LDS [k][64 + 16] and read as the MFMA
// fragments av = S[k = lane >> 4][i = lane & 15] (conflict-free within each 32-lane half, as vg_raster_kernel).  Thread (j = tid & 63,
// kb = tid >> 6) moves elements (k = kb + 4 r, j): consecutive lanes read consecutive r of A (view: runs of m2 consecutive doubles, a run
// per j) and consecutive c of the two V rows.  Edges: rows past R, columns past C and k past K are staged as zeros (selected, never
// multiplied in) and never stored.  One wave sums each output element over k in ascending order: bitwise repeatable.
template <bool VIEW, bool EPI>
__global__ __launch_bounds__(256) void vg_krq_kernel(const VqArgs a) {
    __shared__ double As[VQ_BK * VQ_KS], Bs[VQ_BK * VQ_KS];
    const int tm = (int)(blockIdx.x / (unsigned)a.tiles_n), tn = (int)(blockIdx.x - (unsigned)tm * (unsigned)a.tiles_n);
    const long row0 = (long)tm * VQ_T, col0 = (long)tn * VQ_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, fi = lane & 15, fk = lane >> 4;
    const int j = tid & 63, kb = tid >> 6;
    const bool aok = row0 + j < a.R, bok = col0 + j < a.C;
    const long row = aok ? row0 + j : 0, col = bok ? col0 + j : 0;
    const int m = a.m, K = a.K;
    const long vstep = (long)a.m2 * a.Mv;                                  // view: one step of i
    const double* pa = a.A + (VIEW ? (row / a.m2) * a.Mv + row % a.m2 : row);
    const double* pv = a.V + col;
    double ra[4], rb[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + kb + 4 * r;
            const bool kok = k < K;
            const int p = kok ? (int)((unsigned)k / (unsigned)m) : 0, q = kok ? k - p * m : 0;
            if (VIEW) ra[r] = (aok && kok) ? pa[(long)p * vstep + (long)q * a.m2] : 0.0;
            else ra[r] = (aok && kok) ? pa[(long)k * a.ldA] : 0.0;
            rb[r] = (bok && kok) ? pv[(long)p * a.ldV] * pv[(long)q * a.ldV] : 0.0;
        }
    };
    vq_d4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (vq_d4){0.0, 0.0, 0.0, 0.0};
    load(0);
    for (int k0 = 0; k0 < K; k0 += VQ_BK) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            As[(kb + 4 * r) * VQ_KS + j] = ra[r];
            Bs[(kb + 4 * r) * VQ_KS + j] = rb[r];
        }
        __syncthreads();
        if (k0 + VQ_BK < K) load(k0 + VQ_BK);           // the next k-tile is in flight while this one is multiplied
#pragma unroll
        for (int kk = 0; kk < VQ_BK; kk += 4) {
            double fa[2], fb[2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) fa[mb] = As[(kk + fk) * VQ_KS + wr * 32 + mb * 16 + fi];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) fb[nb] = Bs[(kk + fk) * VQ_KS + wc * 32 + nb * 16 + fi];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[mb], fb[nb], acc[mb][nb], 0, 0, 0);
        }
        __syncthreads();
    }
    double sc = a.scale;
    if (EPI && a.theta) sc *= a.theta[2] * a.theta[3];
    // C/D fragment of the fp64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long orow = row0 + wr * 32 + mb * 16 + fk + 4 * r, ocol = col0 + wc * 32 + nb * 16 + fi;
                if (orow < a.R && ocol < a.C) {
                    double v = acc[mb][nb][r];
                    if (EPI) v = sc * ((a.kd - (a.nr ? a.nr[orow] * a.nc[ocol] : 0.0)) + v);
                    a.out[orow * a.ldo + ocol] = v;
                }
            }
}

static long vq_chunk(long m1, long P1) { return std::min<long>(P1, m1 * m1); }      // columns of the P1 axis per pass: Gt <= M^2 doubles

// out[a][b] = scale (kd - n1[a] n2[b] + (u1_a (x) u2_b)^T S (u1_a (x) u2_b)), scale *= theta[2] theta[3] on the device when theta is given.
// Gt: m2^2 x vq_chunk(m1, P1) doubles of scratch.  Two launches per chunk of the P1 axis.  The grid's fast index walks the tiles of a
// chunk's columns: the workgroups that read one 64-row slice of the view of S are neighbours.
static int vg_kron_quadform(const double* S, long m1, long m2, const double* U1, long P1, const double* U2, long P2, const double* n1,
                            const double* n2, double kd, double scale, const double* theta, double* Gt, double* out, hipStream_t st) {
    const long M = m1 * m2, R1 = m2 * m2, chunk = vq_chunk(m1, P1);
    for (long off = 0; off < P1; off += chunk) {
        const long cn = std::min<long>(chunk, P1 - off);
        const long tn1 = (cn + VQ_T - 1) / VQ_T, tm1 = (R1 + VQ_T - 1) / VQ_T, tn2 = (P2 + VQ_T - 1) / VQ_T;
        const VqArgs s1{S, 0, M, (int)m2, U1 + off, P1, (int)m1, (int)(m1 * m1), R1, cn, Gt, cn, nullptr, nullptr, 0.0, 1.0, nullptr, (int)tn1};
        hipLaunchKernelGGL((vg_krq_kernel<true, false>), dim3((unsigned)(tm1 * tn1)), dim3(256), 0, st, s1);
        const VqArgs s2{Gt, cn, 0, 1, U2, P2, (int)m2, (int)R1, cn, P2, out + off * P2, P2, n1 ? n1 + off : nullptr, n2, kd, scale, theta, (int)tn2};
        hipLaunchKernelGGL((vg_krq_kernel<false, true>), dim3((unsigned)(tn1 * tn2)), dim3(256), 0, st, s2);
    }
    VG_HIP(hipGetLastError());
    return VGGP_OK;
}

extern "C" int vggp_kron_quadform(vggp_ctx* c, const double* S, int64_t m1, int64_t m2, const double* U1, int64_t P1, const double* U2,
                                  int64_t P2, const double* n1, const double* n2, double kd, double scale, double* out, void* stream) {
    static const char* fn = "vggp_kron_quadform";
    if (!c) { vg_set_error("%s: null context", fn); return VGGP_EINVAL; }
    VG_REQUIRE(S && U1 && U2 && out && (!n1 == !n2), "%s: null argument (n1 and n2: both or neither)", fn);
    VG_REQUIRE(m1 >= 1 && m2 >= 1 && m1 <= VGM_MAX_M && m2 <= VGM_MAX_M && m1 * m2 <= VGM_MAX_M, "%s: need 1 <= m1 m2 <= %d", fn, VGM_MAX_M);
    VG_REQUIRE(P1 >= 1 && P1 <= VQ_MAXP && P2 >= 1 && P2 <= VQ_MAXP, "%s: need 1 <= P1, P2 <= 2^20", fn);
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    int rc = vg_ensure_misc(c, (size_t)(m2 * m2 * vq_chunk(m1, P1)) * sizeof(double));
    if (rc) return rc;
    if ((rc = vg_kron_quadform(S, m1, m2, U1, P1, U2, P2, n1, n2, kd, scale, nullptr, (double*)c->misc, out, st))) return rc;
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}

// mean and variance on the raster from the state of the last dense masked / scattered step: the mean of vg_raster_mspace, then the
// squared column norms of the U_d it left in the scratch and the two-stage contraction against w.Sinv, the chunk's Gt in w.R
extern "C" int vggp_posterior_raster_var_masked(vggp_ctx* c, const double* g1, int64_t p1, const double* g2, int64_t p2, double* mean,
                                                double* var, void* stream) {
    static const char* fn = "vggp_posterior_raster_var_masked";
    if (c && c->is_paired) {
        vg_set_error("%s: paired inducing points (VGGP_FLAG_PAIRED_Z) have no Kronecker factors to separate; use vggp_posterior_masked", fn);
        return VGGP_EINVAL;
    }
    if (!c || !c->planned) { vg_set_error("%s: context not planned", fn); return VGGP_ESTATE; }
    VG_REQUIRE(!vgi_multi(c), "%s: multi-rank contexts are not supported; use vggp_posterior_masked at the points", fn);
    VG_REQUIRE(p1 >= 1 && p1 <= VQ_MAXP && p2 >= 1 && p2 <= VQ_MAXP, "%s: need 1 <= p1, p2 <= 2^20 (got %lld, %lld)", fn, (long long)p1,
               (long long)p2);
    VG_REQUIRE(g1 && g2 && mean && var, "%s: null argument", fn);
    if (!(c->last_kind == VG_LAST_DENSE && c->have_masked && c->masked)) {
        vg_set_error("%s: the last finished step on this context is no dense masked / scattered step (vggp_elbo_step_masked, "
                     "vggp_elbo_step_scattered)", fn);
        return VGGP_ESTATE;
    }
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VgMasked& w = *reinterpret_cast<VgMasked*>(c->masked);
    const long m1 = w.m1, m2 = w.m2;
    VgRasterAxes ax;
    int rc;
    if ((rc = vg_raster_mspace(c, g1, (long)p1, g2, (long)p2, mean, st, &ax))) return rc;
    double *n1 = ax.A1, *n2 = ax.A2;                        // (the factor columns are consumed by then)
    VGM_LAUNCH1D(vgm_coldot_kernel, p1, st, ax.U1, ax.U1, (int)m1, (long)p1, n1);
    VGM_LAUNCH1D(vgm_coldot_kernel, p2, st, ax.U2, ax.U2, (int)m2, (long)p2, n2);
    if ((rc = vg_kron_quadform(w.Sinv, m1, m2, ax.U1, (long)p1, ax.U2, (long)p2, n1, n2, 1.0, 1.0, c->theta, w.R, var, st))) return rc;
    VG_HIP(hipStreamSynchronize(st));
    return VGGP_OK;
}
