// Gauss quadrature of log on a Lanczos tridiagonal: the stochastic Lanczos quadrature of the iterative solvers, on the device (one
// lane per probe: vgi_slq_kernel, iter_step.hip) and on the host (vggp_exact_step_iter, exact_iter.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

#define VG_LQ_NOCONV 1        // an eigenvalue did not converge in 60 QL sweeps
#define VG_LQ_NOTPOS 2        // an eigenvalue is not positive: log undefined

// T = tridiag(e, d, e), k x k, with e[k - 1] = 0 and z = e1 on entry; implicit QL with shifts that carries only the first components
// of the eigenvectors (z).  d, e, z are overwritten (d: the eigenvalues), *out = sum_j z_j^2 log d_j = e1^T log(T) e1 whatever the
// return value: 0, or the failures above ORed together.
__host__ __device__ inline int vg_lanczos_logquad(double* d, double* e, double* z, int k, double* out) {
    int code = 0;
    for (int l = 0; l < k; ++l) {
        int iter = 0, mm;
        do {
            for (mm = l; mm < k - 1; ++mm) {
                const double dd = fabs(d[mm]) + fabs(d[mm + 1]);
                if (fabs(e[mm]) <= 1e-16 * dd) break;
            }
            if (mm != l) {
                if (iter++ == 60) { code |= VG_LQ_NOCONV; break; }
                double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                double r = hypot(g, 1.0);
                g = d[mm] - d[l] + e[l] / (g + (g >= 0.0 ? fabs(r) : -fabs(r)));
                double s = 1.0, cc = 1.0, p = 0.0;
                int i;
                for (i = mm - 1; i >= l; --i) {
                    double f = s * e[i];
                    const double b = cc * e[i];
                    e[i + 1] = (r = hypot(f, g));
                    if (r == 0.0) { d[i + 1] -= p; e[mm] = 0.0; break; }
                    s = f / r; cc = g / r;
                    g = d[i + 1] - p;
                    r = (d[i] - g) * s + 2.0 * cc * b;
                    d[i + 1] = g + (p = s * r);
                    g = cc * r - b;
                    f = z[i + 1];
                    z[i + 1] = s * z[i] + cc * f;
                    z[i] = cc * z[i] - s * f;
                }
                if (r == 0.0 && i >= l) continue;
                d[l] -= p; e[l] = g; e[mm] = 0.0;
            }
        } while (mm != l);
    }
    double acc = 0.0;
    for (int j = 0; j < k; ++j) { if (!(d[j] > 0.0)) code |= VG_LQ_NOTPOS; acc += z[j] * z[j] * log(d[j]); }
    *out = acc;
    return code;
}
