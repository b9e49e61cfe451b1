// The factor kernel's definition, included twice by factor_build.hip: as vg_factor_kernel (VG_FB_B0K 0: the kernel of every launch
// without a VGGP_BASIS_B0K job -- the timed step among them -- whose text, and so whose code, the B0K paths leave as it was) and as
// vg_factor_b0k_kernel (VG_FB_B0K 1: the same plus the two paths of the B0 cells under the Matern-3/2 / -5/2 kernels).
__global__ __launch_bounds__(256) void VG_FB_KERNEL(const VgFactorArgs2 args, const double* __restrict__ theta,
                                                       double* theta_copy, const VgClearArgs clr) {
    __shared__ double s_grid[VG_FB_MAXROWS + 2];
    const int bid = blockIdx.x, tid = threadIdx.x;
    if (bid == 0) {                                  // step prologue duties (see vg_factor_build_launch)
        if (theta_copy && tid < 6) theta_copy[tid] = theta[tid];     // 5 hyper-parameters + the step's sequence number
        for (int k = 0; k < clr.n; ++k)
            for (int i = tid; i < clr.nwords[k]; i += 256) clr.ptr[k][i] = 0;
    }
    int pi = 0;
    for (int i = 1; i < args.nparts; ++i)
        if (bid >= args.part[i].block_start) pi = i;
    const VgFbPart& P = args.part[pi];
    const VgFactorJob& J = args.job[P.job];
    const bool kpart = P.kpart != 0;
    const double ell = (J.theta_idx >= 0) ? theta[J.theta_idx] : J.ell_imm;
    const int m = J.m, ncols = P.ncols, tmw = P.tmw;
    const int t = bid - P.block_start;
    const int tr = t / P.tiles_c, tc = t - tr * P.tiles_c;            // the only division: once per workgroup, 32-bit
    const int lane = tid & 63, wave = tid >> 6;
    const int rows_tile = P.wide ? tmw : 4 * tmw;
    const int row0 = tr * rows_tile;
    const int c = tc * (P.wide ? VG_FB_TN_WIDE : VG_FB_TN_TALL) + (P.wide ? wave * 128 : 0) + 2 * lane;
    const int rw0 = P.wide ? 0 : wave * tmw;                         // this wave's first row inside the tile

    // stage the row coordinates of the tile (mesh knots k .. k+rows for B0 cells, inducing coordinates otherwise)
#if VG_FB_B0K
    const bool b0k = J.basis == VGGP_BASIS_B0K;
    const int glen = (J.basis == VGGP_BASIS_B0 || b0k) ? m + 1 : m;
    const bool rowgrid = J.basis == VGGP_BASIS_B0 || J.basis == VGGP_BASIS_POINTS || J.basis == VGGP_BASIS_B1 || b0k;
#else
    const int glen = (J.basis == VGGP_BASIS_B0) ? m + 1 : m;
    const bool rowgrid = J.basis == VGGP_BASIS_B0 || J.basis == VGGP_BASIS_POINTS || J.basis == VGGP_BASIS_B1;
#endif
    if (tid <= rows_tile) {
        const int gi = row0 + tid;
        s_grid[tid] = (rowgrid && gi < glen) ? J.grid[gi] : 0.0;
    }
    // this lane's two column coordinates: one 16-B load when aligned
    const double* __restrict__ xsrc = kpart ? J.grid : J.x;
    const bool colcoord = !(kpart && (J.basis == VGGP_BASIS_VFF)) && J.basis != VGGP_BASIS_ONE && xsrc != nullptr;
    double x0 = 0.0, x1 = 0.0;
    if (colcoord) {
        if (c + 1 < ncols && ((reinterpret_cast<uintptr_t>(xsrc + c) & 15) == 0)) {
            const double2 xx = *reinterpret_cast<const double2*>(xsrc + c);
            x0 = xx.x; x1 = xx.y;
        } else {
            if (c < ncols) x0 = xsrc[c];
            if (c + 1 < ncols) x1 = xsrc[c + 1];
        }
    }
    __syncthreads();
    if (c >= ncols) return;
    double* __restrict__ O = kpart ? J.K0 : J.A0;
    double* __restrict__ dO = kpart ? J.dK0 : J.dA0;
    const bool vec = c + 1 < ncols && (ncols & 1) == 0 && ((reinterpret_cast<uintptr_t>(O) | reinterpret_cast<uintptr_t>(dO)) & 15) == 0;
    const bool two = c + 1 < ncols;

#if VG_FB_B0K
    if (b0k && !kpart) {
        // the rolling-edge walk of the Matern-1/2 cells below with the edge terms of the dimension's kernel (vg_b0k_edge)
        const VgB0kA ca = vg_b0k_A_consts(J.kind, ell);
        double Ea0, dEa0, Ea1, dEa1;
        vg_b0k_edge(ca, s_grid[rw0], x0, Ea0, dEa0);
        vg_b0k_edge(ca, s_grid[rw0], x1, Ea1, dEa1);
        for (int r = 0; r < tmw; ++r) {
            const int k = row0 + rw0 + r;
            if (k >= m) break;
            const double a = s_grid[rw0 + r], b = s_grid[rw0 + r + 1];
            double Eb0, dEb0, Eb1, dEb1;
            vg_b0k_edge(ca, b, x0, Eb0, dEb0);
            vg_b0k_edge(ca, b, x1, Eb1, dEb1);
            double v0, d0, v1, d1;
            vg_b0k_cell(ca, a, b, x0, Ea0, dEa0, Eb0, dEb0, v0, d0);
            vg_b0k_cell(ca, a, b, x1, Ea1, dEa1, Eb1, dEb1, v1, d1);
            const long o = (long)k * ncols + c;
            if (vec) {
                if (O) *reinterpret_cast<double2*>(O + o) = make_double2(v0, v1);
                if (dO) *reinterpret_cast<double2*>(dO + o) = make_double2(d0, d1);
            } else {
                if (O) { O[o] = v0; if (two) O[o + 1] = v1; }
                if (dO) { dO[o] = d0; if (two) dO[o + 1] = d1; }
            }
            Ea0 = Eb0; dEa0 = dEb0; Ea1 = Eb1; dEa1 = dEb1;
        }
        return;
    }
    if (b0k && kpart) {
        // Toeplitz in kd = |k - p| (vg_b0k_K): the polynomial coefficients are constants of the launch -- one exponential per element
        const VgB0kK ck = vg_b0k_K_consts(J.kind, J.grid[1] - J.grid[0], ell);
        for (int r = 0; r < tmw; ++r) {
            const int k = row0 + rw0 + r;
            if (k >= m) break;
            double v0, d0, v1, d1;
            vg_b0k_K(ck, k > c ? k - c : c - k, v0, d0);
            vg_b0k_K(ck, k > c + 1 ? k - c - 1 : c + 1 - k, v1, d1);
            const long o = (long)k * ncols + c;
            if (vec) {
                if (O) *reinterpret_cast<double2*>(O + o) = make_double2(v0, v1);
                if (dO) *reinterpret_cast<double2*>(dO + o) = make_double2(d0, d1);
            } else {
                if (O) { O[o] = v0; if (two) O[o + 1] = v1; }
                if (dO) { dO[o] = d0; if (two) dO[o + 1] = d1; }
            }
        }
        return;
    }
#endif
    if (J.basis == VGGP_BASIS_B0 && !kpart) {
        // cell k = (g_k, g_k+1]: E(g) = ell e^{-|x-g|/ell}, dE(g) = e^{-|x-g|/ell} (1 + |x-g|/ell); the right edge of one
        // row is the left edge of the next: one exponential per element
        auto edge = [&](double g, double x, double& E, double& dE) {
            const double u = fabs(x - g), e = exp(-u / ell);
            E = ell * e;
            dE = e * (1.0 + u / ell);
        };
        double Ea0, dEa0, Ea1, dEa1;
        edge(s_grid[rw0], x0, Ea0, dEa0);
        edge(s_grid[rw0], x1, Ea1, dEa1);
        for (int r = 0; r < tmw; ++r) {
            const int k = row0 + rw0 + r;
            if (k >= m) break;
            const double a = s_grid[rw0 + r], b = s_grid[rw0 + r + 1];
            double Eb0, dEb0, Eb1, dEb1;
            edge(b, x0, Eb0, dEb0);
            edge(b, x1, Eb1, dEb1);
            double v0, d0, v1, d1;
            if (x0 > a && x0 <= b) { v0 = 2.0 * ell - (Ea0 + Eb0); d0 = 2.0 - (dEa0 + dEb0); }
            else { const double sg = (x0 <= a) ? 1.0 : -1.0; v0 = sg * (Ea0 - Eb0); d0 = sg * (dEa0 - dEb0); }
            if (x1 > a && x1 <= b) { v1 = 2.0 * ell - (Ea1 + Eb1); d1 = 2.0 - (dEa1 + dEb1); }
            else { const double sg = (x1 <= a) ? 1.0 : -1.0; v1 = sg * (Ea1 - Eb1); d1 = sg * (dEa1 - dEb1); }
            const long o = (long)k * ncols + c;
            if (vec) {
                if (O) *reinterpret_cast<double2*>(O + o) = make_double2(v0, v1);
                if (dO) *reinterpret_cast<double2*>(dO + o) = make_double2(d0, d1);
            } else {
                if (O) { O[o] = v0; if (two) O[o + 1] = v1; }
                if (dO) { dO[o] = d0; if (two) dO[o + 1] = d1; }
            }
            Ea0 = Eb0; dEa0 = dEb0; Ea1 = Eb1; dEa1 = dEb1;
        }
        return;
    }
    if (J.basis == VGGP_BASIS_B0 && kpart && !(J.flags & VGGP_FLAG_B0_F32_KDELTA)) {
        // Toeplitz in kd = |k - p| (vg_b0_K): everything but e^{-kd t} is a constant of the launch -- one exponential per element
        const double t = (J.grid[1] - J.grid[0]) / ell, em1 = expm1(-t), q = em1 * em1, em2 = expm1(-2.0 * t);
        const double l2 = ell * ell, toe = t / ell;
        const double v_diag = l2 * 2.0 * (em1 + t), d_diag = 2.0 * ell * 2.0 * (em1 + t) + l2 * (2.0 * toe) * em1;
        auto el = [&](int kd, double& v, double& dv) {
            const double e = exp(-(double)(kd ? kd - 1 : 0) * t), r = e * q, dr = toe * e * ((double)kd * q + em2);
            v = kd ? l2 * r : v_diag;
            dv = kd ? 2.0 * ell * r + l2 * dr : d_diag;
        };
        for (int r = 0; r < tmw; ++r) {
            const int k = row0 + rw0 + r;
            if (k >= m) break;
            double v0, d0, v1, d1;
            el(k > c ? k - c : c - k, v0, d0);
            el(k > c + 1 ? k - c - 1 : c + 1 - k, v1, d1);
            const long o = (long)k * ncols + c;
            if (vec) {
                if (O) *reinterpret_cast<double2*>(O + o) = make_double2(v0, v1);
                if (dO) *reinterpret_cast<double2*>(dO + o) = make_double2(d0, d1);
            } else {
                if (O) { O[o] = v0; if (two) O[o + 1] = v1; }
                if (dO) { dO[o] = d0; if (two) dO[o + 1] = d1; }
            }
        }
        return;
    }
    for (int r = 0; r < tmw; ++r) {
        const int k = row0 + rw0 + r;
        if (k >= m) break;
        const double gk = s_grid[rw0 + r], gk1 = s_grid[rw0 + r + 1];
        double v0, d0, v1 = 0.0, d1 = 0.0;
        vg_factor_elem(J, kpart, k, c, x0, gk, gk1, ell, v0, d0);
        if (two) vg_factor_elem(J, kpart, k, c + 1, x1, gk, gk1, ell, v1, d1);
        const long o = (long)k * ncols + c;
        if (vec) {
            if (O) *reinterpret_cast<double2*>(O + o) = make_double2(v0, v1);
            if (dO) *reinterpret_cast<double2*>(dO + o) = make_double2(d0, d1);
        } else {
            if (O) { O[o] = v0; if (two) O[o + 1] = v1; }
            if (dO) { dO[o] = d0; if (two) dO[o + 1] = d1; }
        }
    }
}
