// cv_fold_tail.hpp -- what a hold-out block in LDS becomes: C C' = K_BB, W = C^-1, var_i = sum_j W_ji^2 and
// resid = W' (W U_B), every sum in a fixed order.  One workgroup of 256 threads; the callers differ in how the lower triangle
// of K_BB gets into M: cv_fold_kernel (cv.hip) gathers it from a matrix in memory, vecchia_cv_fold_kernel (vecchia_cv.hip)
// builds it from the rows of U.  Each caller compiles this text under its own translation unit's contraction setting.
//   M     the block, leading dimension BP + 1: the lower triangle holds K_BB on entry and its factor C afterwards (the
//         diagonal is not stored: dinv = 1 / C_jj); the upper triangle takes W' = C^-T, W(k, j), k > j, at (j, k)
//   ub, yb  256 doubles each: G = 256 / BP right-hand sides and intermediate vectors at a time
//   pos   the b members' positions in var, res and U (ascending)
// Returns whether a pivot was not positive and finite (the same in every thread).  The caller's stores into M need no
// barrier of their own in front of this: the first step begins with one.
#pragma once
#include <hip/hip_runtime.h>

namespace cocons {

template <int BP> __device__ __forceinline__ bool
cv_fold_tail(double *M, double *dinv, double *ub, double *yb, int b, const int *pos, const double *U, size_t ldu, int nr,
             double *var, double *res, size_t ldr)
{
    constexpr int LD = BP + 1, G = 256 / BP;
    const int tid = threadIdx.x, i = tid % BP, g = tid / BP;
    // C C' = K_BB, right-looking, column by column
    bool bad = false;
    for (int j = 0; j < b; ++j) {
        __syncthreads();
        double d = M[j + j * LD];
        if (!(d > 0.0) || !isfinite(d)) { bad = true; d = 1.0; }
        const double piv = sqrt(d);
        if (tid == 0) dinv[j] = 1.0 / piv;
        if (g == 0 && i > j && i < b) M[i + j * LD] /= piv;
        __syncthreads();
        if (i > j && i < b) {
            const double lij = M[i + j * LD];
            for (int c = j + 1 + g; c <= i; c += G) M[i + c * LD] -= lij * M[c + j * LD];
        }
    }
    __syncthreads();
    // W = C^-1: W(r, j) = -(sum_{k = r-1 .. j} C(r, k) W(k, j)) / C(r, r), W(j, j) = 1 / C(j, j)
    if (tid < b) {
        const int j = tid;
        const double wjj = dinv[j];
        for (int r = j + 1; r < b; ++r) {
            double s = 0.0;
            for (int k = r - 1; k > j; --k) s += M[r + k * LD] * M[j + k * LD];
            s += M[r + j * LD] * wjj;
            M[j + r * LD] = -s * dinv[r];
        }
        // var_j = sum_{k >= j} W(k, j)^2
        double v = wjj * wjj;
        for (int k = j + 1; k < b; ++k) v += M[j + k * LD] * M[j + k * LD];
        var[pos[j]] = v;
    }
    // resid = W' (W U_B), G realisations at a time
    for (int c0 = 0; c0 < nr; c0 += G) {
        const int c = c0 + g;
        const bool on = c < nr && i < b;
        __syncthreads();
        if (on) ub[g * BP + i] = U[(size_t)pos[i] + (size_t)c * ldu];
        __syncthreads();
        if (on) {
            double y = 0.0;
            for (int k = 0; k < i; ++k) y += M[k + i * LD] * ub[g * BP + k];      // W(i, k) at (k, i)
            y += dinv[i] * ub[g * BP + i];
            yb[g * BP + i] = y;
        }
        __syncthreads();
        if (on) {
            double e = dinv[i] * yb[g * BP + i];
            for (int k = i + 1; k < b; ++k) e += M[i + k * LD] * yb[g * BP + k];  // W(k, i) at (i, k)
            res[(size_t)pos[i] + (size_t)c * ldr] = e;
        }
    }
    return bad;
}

}  // namespace cocons
