// Joint posterior samples of q(v): the counter-based normal generator and the small kernels around the block solves
// (vggp_normal_fill, vggp_qv_sample in api.hip, vggp_qv_sample_*_iter in iter_readout.hip).
//
// Generator: Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments 0x9E3779B9 / 0xBB67AE85),
//     key = (seed lo, seed hi),  counter = (c lo, c hi, stream, 0),  c = idx >> 1,
//     a = w0 << 21 | w1 >> 11,  u1 = (a + 0.5) 2^-53;   b = w2 << 21 | w3 >> 11,  u2 = (b + 0.5) 2^-53;   r = sqrt(-2 ln u1),
//     element idx = r cos(2 pi u2) (idx even) or r sin(2 pi u2) (idx odd).
// One Philox call serves one element: the value of element idx is a function of (seed, stream, idx) alone, whatever kernel asks for
// it, in whatever order and layout.  Index spaces of a sampling call (s = global sample number):
//     stream 0  E  idx = s M + i1 m2 + i2
//     stream 1  F  idx = s n1 n2 + j n1 + i on a grid (the layout of Y and W),  idx = s N + k on scattered points
// and of a raster-sampling call (raster_sample.hip; p1 x p2 raster):
//     stream 2  G  idx = s p1 p2 + a p2 + b
//     stream 3  H  idx = s m1 p2 + i p2 + b
//     stream 4     idx = s p1 p2 + a p2 + b: the observation noise the host layer adds for posterior_predictive_grid().sample()
// Specification: tests/qv_sample_spec.py, tests/raster_sample_spec.py.
#include "ctx.h"

__device__ __forceinline__ double vgq_normal(unsigned long long seed, unsigned stream_id, unsigned long long idx) {
    const unsigned long long cnt = idx >> 1;
    unsigned c0 = (unsigned)cnt, c1 = (unsigned)(cnt >> 32), c2 = stream_id, c3 = 0u;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const unsigned long long a = ((unsigned long long)c0 << 21) | (c1 >> 11), b = ((unsigned long long)c2 << 21) | (c3 >> 11);
    const double u1 = ((double)a + 0.5) * 0x1p-53, u2 = ((double)b + 0.5) * 0x1p-53;
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
    return r * ((idx & 1ULL) ? sn : cs);
}

// out[k] = element first + k of (seed, stream)
__global__ void vgq_fill_kernel(unsigned long long seed, unsigned stream_id, unsigned long long first, long n, double* out) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = vgq_normal(seed, stream_id, first + (unsigned long long)k);
}
// E[a][c][b] (block vector [m1][nbc][m2]) = noise of sample s0 + c at cell (a, b): eps[c][a][b] when the caller brings it, stream 0
// otherwise; the padding columns c >= cn are zero
__global__ void vgq_block_noise_kernel(double* E, const double* eps, unsigned long long seed, unsigned long long s0, int m1, int nbc, int m2,
                                       int cn) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)m1 * nbc * m2) return;
    const int b = (int)(idx % m2), c = (int)((idx / m2) % nbc), a = (int)(idx / ((long)m2 * nbc));
    const unsigned long long M = (unsigned long long)m1 * m2, cell = (unsigned long long)a * m2 + b;
    E[idx] = c >= cn ? 0.0 : (eps ? eps[c * M + cell] : vgq_normal(seed, 0u, (s0 + c) * M + cell));
}
// F[i][c][j] (grid field [n1][nbc][n2]) = Wt[i][j] o noise of sample s0 + c at node (i, j): eps[c][j][i] or stream 1; unobserved nodes
// and padding columns are exact zeros (whatever eps holds there)
__global__ void vgq_field_noise_grid_kernel(double* F, const double* Wt, const double* eps, unsigned long long seed, unsigned long long s0,
                                            long n1, int nbc, long n2, int cn) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n1 * nbc * n2) return;
    const long j = idx % n2, i = idx / (n2 * nbc);
    const int c = (int)((idx / n2) % nbc);
    double v = 0.0;
    if (c < cn && Wt[i * n2 + j] != 0.0) {
        const unsigned long long nn = (unsigned long long)n1 * (unsigned long long)n2, node = (unsigned long long)j * n1 + i;
        v = eps ? eps[c * nn + node] : vgq_normal(seed, 1u, (s0 + c) * nn + node);
    }
    F[idx] = v;
}
// F[c][k] (point field [nbc][N]) = noise of sample s0 + c at point k: eps[c][k] or stream 1
__global__ void vgq_field_noise_pts_kernel(double* F, const double* eps, unsigned long long seed, unsigned long long s0, long N, int nbc,
                                           int cn) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * nbc) return;
    const long k = idx % N;
    const int c = (int)(idx / N);
    F[idx] = c >= cn ? 0.0 : (eps ? eps[(unsigned long long)c * N + k] : vgq_normal(seed, 1u, (s0 + c) * (unsigned long long)N + k));
}
// Z = E + sqrt(rho) K   (K: the back product of the noise field; Cov(vec Z) = I + rho Phi~)
__global__ void vgq_fuse_kernel(double* Z, const double* K, const double* theta, long n) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) Z[idx] = Z[idx] + sqrt(theta[2] * theta[3] / theta[4]) * K[idx];
}
// X[a][c][b] *= sqrt(invD[a][b])   (full grid: Sigma~^-1/2 in the Kronecker eigenbasis)
__global__ void vgq_root_scale_kernel(double* X, const double* invD, int m1, int nbc, int m2) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)m1 * nbc * m2) return;
    const int b = (int)(idx % m2), a = (int)(idx / ((long)m2 * nbc));
    X[idx] *= sqrt(invD[(long)a * m2 + b]);
}
// out[c][a][b] = mean[a][b] + sqrt(s1^e1 s2^e2) Y[a][c][b] for the cn live columns of the block
__global__ void vgq_out_kernel(const double* Y, const double* mean, const double* theta, int e1, int e2, int m1, int nbc, int m2, int cn,
                               double* out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)m1 * nbc * m2) return;
    const int b = (int)(idx % m2), c = (int)((idx / m2) % nbc), a = (int)(idx / ((long)m2 * nbc));
    if (c >= cn) return;
    const double sc = sqrt((e1 > 0 ? theta[2] : 1.0 / theta[2]) * (e2 > 0 ? theta[3] : 1.0 / theta[3]));
    const long cell = (long)a * m2 + b;
    out[(long)c * m1 * m2 + cell] = mean[cell] + sc * Y[idx];
}

// raster samples (raster_sample.hip): E[a][c][b] (rows [m1][nbc][w]) = eps[c][a][b] or element (s0 + c) m1 w + a w + b of `stream_id`
__global__ void vgq_rows_noise_kernel(double* E, const double* eps, unsigned long long seed, unsigned stream_id, unsigned long long s0, int m1,
                                      int nbc, long w, int cn) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)m1 * nbc * w) return;
    const long b = idx % w, a = idx / (w * nbc);
    const int c = (int)((idx / w) % nbc);
    const unsigned long long n = (unsigned long long)m1 * (unsigned long long)w, cell = (unsigned long long)a * w + b;
    E[idx] = c >= cn ? 0.0 : (eps ? eps[c * n + cell] : vgq_normal(seed, stream_id, (s0 + c) * n + cell));
}
__global__ void vgq_scale_root_kernel(double* x, long n, const double* theta) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= sqrt(theta[2] * theta[3]);
}
__global__ void vgq_nugget_kernel(double* A, long p, double eta) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < p) A[i * p + i] += eta;
}

#define VGQ_LAUNCH1D(kern, n, st, ...) hipLaunchKernelGGL(kern, dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, st, __VA_ARGS__)

hipError_t vg_normal_fill_launch(unsigned long long seed, unsigned stream_id, unsigned long long first, long n, double* out, hipStream_t st) {
    if (n > 0) VGQ_LAUNCH1D(vgq_fill_kernel, n, st, seed, stream_id, first, n, out);
    return hipGetLastError();
}
hipError_t vg_sample_block_noise_launch(double* E, const double* eps, unsigned long long seed, unsigned long long s0, int m1, int nbc, int m2,
                                        int cn, hipStream_t st) {
    VGQ_LAUNCH1D(vgq_block_noise_kernel, (long)m1 * nbc * m2, st, E, eps, seed, s0, m1, nbc, m2, cn);
    return hipGetLastError();
}
hipError_t vg_sample_field_noise_launch(double* F, const double* Wt, const double* eps, unsigned long long seed, unsigned long long s0, long n1,
                                        int nbc, long n2, int cn, hipStream_t st) {
    if (Wt) VGQ_LAUNCH1D(vgq_field_noise_grid_kernel, n1 * nbc * n2, st, F, Wt, eps, seed, s0, n1, nbc, n2, cn);
    else VGQ_LAUNCH1D(vgq_field_noise_pts_kernel, n1 * nbc, st, F, eps, seed, s0, n1, nbc, cn);
    return hipGetLastError();
}
hipError_t vg_sample_fuse_launch(double* Z, const double* K, const double* theta, long n, hipStream_t st) {
    VGQ_LAUNCH1D(vgq_fuse_kernel, n, st, Z, K, theta, n);
    return hipGetLastError();
}
hipError_t vg_sample_root_scale_launch(double* X, const double* invD, int m1, int nbc, int m2, hipStream_t st) {
    VGQ_LAUNCH1D(vgq_root_scale_kernel, (long)m1 * nbc * m2, st, X, invD, m1, nbc, m2);
    return hipGetLastError();
}
hipError_t vg_sample_out_launch(const double* Y, const double* mean, const double* theta, int e1, int e2, int m1, int nbc, int m2, int cn,
                                double* out, hipStream_t st) {
    VGQ_LAUNCH1D(vgq_out_kernel, (long)m1 * nbc * m2, st, Y, mean, theta, e1, e2, m1, nbc, m2, cn, out);
    return hipGetLastError();
}
hipError_t vg_sample_rows_noise_launch(double* E, const double* eps, unsigned long long seed, unsigned stream_id, unsigned long long s0, int m1,
                                       int nbc, long w, int cn, hipStream_t st) {
    VGQ_LAUNCH1D(vgq_rows_noise_kernel, (long)m1 * nbc * w, st, E, eps, seed, stream_id, s0, m1, nbc, w, cn);
    return hipGetLastError();
}
hipError_t vg_sample_scale_root_launch(double* x, long n, const double* theta, hipStream_t st) {
    VGQ_LAUNCH1D(vgq_scale_root_kernel, n, st, x, n, theta);
    return hipGetLastError();
}
hipError_t vg_sample_nugget_launch(double* A, long p, double eta, hipStream_t st) {
    VGQ_LAUNCH1D(vgq_nugget_kernel, p, st, A, p, eta);
    return hipGetLastError();
}

extern "C" int vggp_normal_fill(vggp_ctx* c, uint64_t seed, int stream_id, int64_t first_idx, int64_t n, double* out, void* stream) {
    VG_REQUIRE(c, "vggp_normal_fill: null context");
    VG_REQUIRE(stream_id >= 0 && first_idx >= 0 && n >= 0 && (out || n == 0), "vggp_normal_fill: bad argument");
    VG_ENTER_DEVICE(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
    VG_HIP(vg_normal_fill_launch(seed, (unsigned)stream_id, (unsigned long long)first_idx, (long)n, out, st));
    return VGGP_OK;
}
