// Element formulas of the per-dimension factors (unit outputscale): value and d/d ell of Kuf_d / Kuu_d for every basis.
// Shared by the factor kernel (factor_build.hip) and the kernels that evaluate prior covariances on the fly (api.hip).
// Reference: kronecker_structure.py:318-319, :336-337 (pairwise), :723-739, :768-790 (B0), :400-480 (VFF), :560-628 (B1).
#pragma once
#include "common.h"

// inv_ell = 1 / ell (a launch constant): two f64 divisions per element become multiplications (the divisions were a third of
// the pairwise kernel's instructions: 3.8 -> TB/s at 8192^2, profiles/r2_factor_build_8192.txt)
__device__ __forceinline__ void vg_kappa(int kind, double dist, double inv_ell, double& v, double& dv) {
    const double r = dist * inv_ell;
    if (kind == VGGP_KIND_MATERN12) {
        const double e = exp(-r);
        v = e;
        dv = e * r * inv_ell;
    } else if (kind == VGGP_KIND_MATERN32) {
        const double a = 1.7320508075688772 * r;
        const double e = exp(-a);
        v = (1.0 + a) * e;
        dv = a * a * e * inv_ell;
    } else if (kind == VGGP_KIND_MATERN52) {
        const double a = 2.23606797749979 * r;
        const double e = exp(-a);
        v = (1.0 + a + a * a * (1.0 / 3.0)) * e;
        dv = (a * a * (1.0 / 3.0)) * (1.0 + a) * e * inv_ell;
    } else {   // RBF
        const double e = exp(-0.5 * r * r);
        v = e;
        dv = e * r * r * inv_ell;
    }
}

// The same profile at the signed offset d = z - x, with its derivative in z as well: dz = d kappa / dz (0 at d = 0, as autograd
// differentiates |d| there).  Used by the paired inducing points (paired.hip), whose gradient runs through the coordinates of Z.
__device__ __forceinline__ void vg_kappa_z(int kind, double d, double inv_ell, double& v, double& dv, double& dz) {
    const double r = fabs(d) * inv_ell;
    const double sg = d > 0.0 ? inv_ell : (d < 0.0 ? -inv_ell : 0.0);
    if (kind == VGGP_KIND_MATERN12) {
        const double e = exp(-r);
        v = e;
        dv = e * r * inv_ell;
        dz = -e * sg;
    } else if (kind == VGGP_KIND_MATERN32) {
        const double a = 1.7320508075688772 * r;
        const double e = exp(-a);
        v = (1.0 + a) * e;
        dv = a * a * e * inv_ell;
        dz = -a * e * 1.7320508075688772 * sg;
    } else if (kind == VGGP_KIND_MATERN52) {
        const double a = 2.23606797749979 * r;
        const double e = exp(-a);
        v = (1.0 + a + a * a * (1.0 / 3.0)) * e;
        dv = (a * a * (1.0 / 3.0)) * (1.0 + a) * e * inv_ell;
        dz = -(a * (1.0 / 3.0)) * (1.0 + a) * e * 2.23606797749979 * sg;
    } else {   // RBF
        const double e = exp(-0.5 * r * r);
        v = e;
        dv = e * r * r * inv_ell;
        dz = -e * r * sg;
    }
}

// B0 cell-integral cross-covariance, cell k = (a, b], point x (kronecker_structure.py:768-790)
__device__ __forceinline__ void vg_b0_A(double a, double b, double x, double ell, double& v, double& dv) {
    const double ua = fabs(x - a), ub = fabs(x - b);
    const double ea = exp(-ua / ell), eb = exp(-ub / ell);
    const double E1 = ell * ea, E2 = ell * eb;
    const double dE1 = ea * (1.0 + ua / ell), dE2 = eb * (1.0 + ub / ell);
    if (x > a && x <= b) {
        v = 2.0 * ell - (E1 + E2);
        dv = 2.0 - (dE1 + dE2);
    } else {
        const double sg = (x <= a) ? 1.0 : -1.0;
        v = sg * (E1 - E2);
        dv = sg * (dE1 - dE2);
    }
}

// B0 cell-cell covariance, Toeplitz in kd = |i-j| (kronecker_structure.py:723-739), written in the
// cancellation-free and overflow-free form, t = delta/ell, em1 = expm1(-t), E = e^{-(k-1) t}:
//   r_k = E em1^2                                  (= e^{-(k-1)t} + e^{-(k+1)t} - 2 e^{-kt}),   r_0 = 2 (em1 + t)
//   dr_k/d ell = (t/ell) E (k em1^2 + expm1(-2t))  (= (delta/ell^2) [(k-1)e^{-(k-1)t} + (k+1)e^{-(k+1)t} - 2k e^{-kt}])
// No factor grows with t (the earlier e^{-kt} 4 sinh^2(t/2) overflowed to inf * 0 for t > 710): finite for every t > 0.
__device__ __forceinline__ void vg_b0_K(int kd, double delta, double ell, double& v, double& dv) {
    const double t = delta / ell;
    const double em1 = expm1(-t);
    double r, dr;
    if (kd == 0) {
        r = 2.0 * (em1 + t);
        dr = (2.0 * t / ell) * em1;
    } else {
        const double q = em1 * em1;
        const double e = exp(-(double)(kd - 1) * t);
        r = e * q;
        dr = (t / ell) * e * ((double)kd * q + expm1(-2.0 * t));
    }
    v = ell * ell * r;
    dv = 2.0 * ell * r + ell * ell * dr;
}

// Reference-literal variant (VGGP_FLAG_B0_F32_KDELTA): the products c*delta are rounded to float32 as in
// the reference (float32 mesh attributes), then exp(-(c delta)_f32 / ell) in float64, three-term form.
__device__ __forceinline__ void vg_b0_K_f32(int kd, double delta, double ell, double& v, double& dv) {
    const float df = (float)delta;
    double r, dr;
    if (kd == 0) {
        const double t = (double)df / ell;
        const double e = exp(-t);
        r = 2.0 * (e + t - 1.0);
        dr = 2.0 * (e * t / ell - t / ell);
    } else {
        const double a0 = (double)((float)(kd - 1) * df), a1 = (double)((float)(kd + 1) * df),
                     a2 = (double)((float)kd * df);
        const double e0 = exp(-a0 / ell), e1 = exp(-a1 / ell), e2 = exp(-a2 / ell);
        r = e0 + e1 - 2.0 * e2;
        dr = (e0 * a0 + e1 * a1 - 2.0 * e2 * a2) / (ell * ell);
    }
    v = ell * ell * r;
    dv = 2.0 * ell * r + ell * ell * dr;
}

// ---- B0 cells under the Matern-3/2 and Matern-5/2 kernels (VGGP_BASIS_B0K; forms, derivation and scales: tests/b0_kinds_spec.py) ----
// c = kappa0 / ell, kappa0 = sqrt(3) or sqrt(5).  Edge function of the cross-covariance: E(g) = int_{|x-g|}^inf kappa = P(u) e^{-u} / c,
// u = c |x - g|, P = 2 + u or (8 + 5u + u^2) / 3, and dE / d ell = Q(u) e^{-u} / kappa0, Q = 2 + 2u + u^2 or (8 + 8u + 4u^2 + u^3) / 3.
// A cell's integral is a difference (x outside) or 2 P(0) / c minus the sum (x inside) of its two edges' terms -- only decaying
// terms are subtracted, so a far cell keeps its relative accuracy -- and a row walk evaluates one exponential per element.
struct VgB0kA {
    double c, invc, invk0, in_v, in_d;      // in_v = 2 P(0) / c, in_d = 2 P(0) / kappa0: the whole-line integral and its d / d ell
    bool n52;
};
__device__ __forceinline__ VgB0kA vg_b0k_A_consts(int kind, double ell) {
    VgB0kA a;
    a.n52 = kind == VGGP_KIND_MATERN52;
    const double k0 = a.n52 ? 2.23606797749979 : 1.7320508075688772, P0 = a.n52 ? 8.0 / 3.0 : 2.0;
    a.c = k0 / ell; a.invc = ell / k0; a.invk0 = 1.0 / k0;
    a.in_v = 2.0 * P0 * a.invc; a.in_d = 2.0 * P0 * a.invk0;
    return a;
}
__device__ __forceinline__ void vg_b0k_edge(const VgB0kA& a, double g, double x, double& E, double& dE) {
    const double u = a.c * fabs(x - g), e = exp(-u);
    const double P = a.n52 ? (8.0 + u * (5.0 + u)) * (1.0 / 3.0) : 2.0 + u;
    const double Q = a.n52 ? (8.0 + u * (8.0 + u * (4.0 + u))) * (1.0 / 3.0) : 2.0 + u * (2.0 + u);
    E = P * e * a.invc;
    dE = Q * e * a.invk0;
}
// cell (ga, gb] from its two edges' terms
__device__ __forceinline__ void vg_b0k_cell(const VgB0kA& a, double ga, double gb, double x, double Ea, double dEa, double Eb, double dEb,
                                            double& v, double& dv) {
    if (x > ga && x <= gb) { v = a.in_v - (Ea + Eb); dv = a.in_d - (dEa + dEb); }
    else { const double sg = (x <= ga) ? 1.0 : -1.0; v = sg * (Ea - Eb); dv = sg * (dEa - dEb); }
}

// Cell-cell covariance, Toeplitz in kd = |i - j|: the second difference of G (G'' = kappa) whose linear term cancels for kd >= 1.
// With t = c delta, x = e^{-t}, em1 = expm1(-t), q = em1^2, e2 = expm1(-2t), s2 = x^2 + 1 and E = e^{-(kd-1) t}:
//   K0_kd = C E (a0 + kd a1 + kd^2 a2),   dK0_kd / d ell = 2 K0_kd / ell - (t / ell) C E (d0 + kd d1 + kd^2 d2 + kd^3 d3)
// the a_i, d_i constants of the mesh (3/2: a2 = d3 = 0), C = 1 / c^2 or 1 / (3 c^2); kd = 0 is 2 G(delta) through expm1.  No factor
// grows with t: finite for every t > 0.  One exponential per element.
struct VgB0kK {
    double t, toe, tol, C, a0, a1, a2, d0, d1, d2, d3, v0, dv0;      // toe = t / ell, tol = 2 / ell; v0, dv0: the diagonal
};
__device__ __forceinline__ VgB0kK vg_b0k_K_consts(int kind, double delta, double ell) {
    VgB0kK k;
    const bool n52 = kind == VGGP_KIND_MATERN52;
    const double c = (n52 ? 2.23606797749979 : 1.7320508075688772) / ell;
    const double t = c * delta, x = exp(-t), em1 = expm1(-t), e2 = expm1(-2.0 * t), q = em1 * em1, x2 = x * x, s2 = x2 + 1.0;
    double b0, b1, b2, F0, dF0;
    if (!n52) {
        k.C = 1.0 / (c * c);
        k.a0 = 3.0 * q + t * e2; k.a1 = t * q; k.a2 = 0.0;
        b0 = -6.0 * x * em1 + e2 - 2.0 * t * x2; b1 = q - 2.0 * t * x * em1; b2 = 0.0;
        F0 = 2.0 * ((3.0 + t) * em1 + 3.0 * t); dF0 = -2.0 * ((2.0 + t) * em1 + t);
        k.d0 = k.a0 + b0; k.d1 = (k.a1 + b1) - k.a0; k.d2 = -k.a1; k.d3 = 0.0;
    } else {
        const double t2 = t * t;
        k.C = 1.0 / (3.0 * c * c);
        k.a0 = 15.0 * q + 7.0 * t * e2 + t2 * s2; k.a1 = 7.0 * t * q + 2.0 * t2 * e2; k.a2 = t2 * q;
        b0 = -30.0 * x * em1 + 7.0 * e2 - 14.0 * t * x2 + 2.0 * t * s2 - 2.0 * t2 * x2;
        b1 = 7.0 * q - 14.0 * t * x * em1 + 4.0 * t * e2 - 4.0 * t2 * x2;
        b2 = 2.0 * t * q - 2.0 * t2 * x * em1;
        F0 = 2.0 * ((15.0 + 7.0 * t + t2) * em1 + 15.0 * t + t2); dF0 = -2.0 * ((8.0 + 5.0 * t + t2) * em1 + 5.0 * t + t2);
        k.d0 = k.a0 + b0; k.d1 = (k.a1 + b1) - k.a0; k.d2 = (k.a2 + b2) - k.a1; k.d3 = -k.a2;
    }
    k.t = t; k.toe = t / ell; k.tol = 2.0 / ell;
    k.v0 = k.C * F0;
    k.dv0 = k.tol * k.v0 - k.toe * (k.C * dF0);
    return k;
}
__device__ __forceinline__ void vg_b0k_K(const VgB0kK& k, int kd, double& v, double& dv) {
    const double kk = (double)kd, e = exp(-(double)(kd ? kd - 1 : 0) * k.t);
    const double F = e * (k.a0 + kk * (k.a1 + kk * k.a2)), dF = e * (k.d0 + kk * (k.d1 + kk * (k.d2 + kk * k.d3)));
    const double vk = k.C * F;
    v = kd ? vk : k.v0;
    dv = kd ? k.tol * vk - k.toe * (k.C * dF) : k.dv0;
}

// one element of any basis but VGGP_BASIS_B0K (whose two parts the factor kernel walks with the functions above; Matern-1/2 under B0K is
// launched as VGGP_BASIS_B0); x = coordinate of column p (an observation for the A part, an inducing coordinate for the K part)
__device__ __forceinline__ void vg_factor_elem(const VgFactorJob& J, bool kpart, int k, int p, double x, double gk, double gk1,
                                               double ell, double& v, double& dv) {
    const int m = J.m;
    if (J.basis == VGGP_BASIS_ONE) {
        v = 1.0;
        dv = 0.0;
    } else if (J.basis == VGGP_BASIS_B0) {
        if (kpart) {
            const int kd = k > p ? k - p : p - k;
            if (J.flags & VGGP_FLAG_B0_F32_KDELTA) vg_b0_K_f32(kd, J.grid[1] - J.grid[0], ell, v, dv);
            else vg_b0_K(kd, J.grid[1] - J.grid[0], ell, v, dv);
        } else {
            vg_b0_A(gk, gk1, x, ell, v, dv);
        }
    } else if (J.basis == VGGP_BASIS_VFF) {
        // grid = [a, b, omega_0 .. omega_M], m = 2M + 1: rows 0..M cosine features, M+1..2M sine features
        const double a = J.grid[0], b = J.grid[1];
        const int M = (m - 1) >> 1;
        const double w = J.grid[2 + (k <= M ? k : k - M)];
        if (kpart) {
            // unit-scale Kuu factor: diag(alpha0) + beta0 beta0^T, alpha0 = (b-a)/4 c (1/ell + w^2 ell), c = 2 at w = 0
            const double cc = (b - a) * 0.25 * (k == 0 ? 2.0 : 1.0);
            v = (k <= M && p <= M) ? 1.0 : 0.0;
            dv = 0.0;
            if (k == p) { v += cc * (1.0 / ell + w * w * ell); dv = cc * (-1.0 / (ell * ell) + w * w); }
        } else {
            const bool inside = x >= a && x < b;
            if (inside) {
                v = k <= M ? cos(w * (x - a)) : sin(w * (x - a));
                dv = 0.0;
            } else {
                const double r = fmin(fabs(x - a), fabs(x - b)), e = exp(-r / ell);
                v = k <= M ? e : 0.0;
                dv = k <= M ? r / (ell * ell) * e : 0.0;
            }
        }
    } else if (J.basis == VGGP_BASIS_B1) {
        // grid = knot mesh v_0 .. v_{m-1}
        const double d = J.grid[1] - J.grid[0];
        if (kpart) {
            // (A ell + B / ell + BC) / 2: A tridiagonal (2d/3, d/6; d/3 at the ends), B (2/d, -1/d; 1/d at the ends), BC = ends
            const int kd = k > p ? k - p : p - k;
            const bool end = (k == 0 || k == m - 1);
            double Aij = 0.0, Bij = 0.0, BCij = 0.0;
            if (kd == 0) { Aij = end ? d / 3.0 : 2.0 * d / 3.0; Bij = end ? 1.0 / d : 2.0 / d; BCij = end ? 1.0 : 0.0; }
            else if (kd == 1) { Aij = d / 6.0; Bij = -1.0 / d; }
            v = 0.5 * (Aij * ell + Bij / ell + BCij);
            dv = 0.5 * (Aij - Bij / (ell * ell));
        } else {
            const bool in = x >= J.grid[0] && x <= J.grid[m - 1];
            v = in ? fmax(0.0, 1.0 - fabs(x - gk) / d) : 0.0;
            dv = 0.0;
        }
    } else {
        vg_kappa(J.kind, fabs(gk - x), 1.0 / ell, v, dv);
    }
}

