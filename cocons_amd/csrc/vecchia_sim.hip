// vecchia_sim.hip -- U^-1 for a Vecchia fit (gfx950): the inverse of vecchia_value_kernel's whitening, from the
// records of vecchia_coef_kernel (vecchia.hip) or of the grouped coefficient launch.
//
//   vecchia_level_sweep_kernel : one relaxation sweep of level(i) = 1 + max level(neighbours) over all rows, in place.
//   vecchia_level_count_kernel, vecchia_level_scatter_kernel : the rows ordered by level (histogram and scatter; the prefix sum
//                                of the few hundred counts is the host's).
//   vecchia_sim_level_kernel   : x_i = (w_i - sum_t s_t x_{j_t}) / s_last for the rows of ONE level, all columns.
//   vecchia_sim_fused_kernel   : the same for a run of consecutive small levels in ONE workgroup, a barrier between levels.
//
// A row's result is a function of its own record and of its neighbours' results alone: the sum runs over the table's places
// in ascending order in one thread, whichever of the two solve kernels the row lands in.  No workgroup waits for another one
// anywhere here: the order between levels is the order of the launches on the stream, or a workgroup's own barrier.
//
// Compile with -ffp-contract=off (see matern_device.hpp).
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace cocons {

// ---------------------------------------------------------------------------
// Levels.  level[i] = 0 for the fixed rows i < n_fixed and never touched; every other row starts at 0 and only grows towards
// 1 + max over its neighbours.  A value read is a lower bound of its row's level whatever the races inside a sweep, so no store
// overshoots, and a sweep that stores nothing has seen the fixed point.
__global__ void __launch_bounds__(256)
vecchia_level_sweep_kernel(const int *nbr, int m, int n, int n_fixed, int *level, int *changed)
{
    const size_t i = (size_t)n_fixed + (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    int lv = 0;
    for (int t = 0; t < m; ++t) {
        const int j = nbr[i * m + t];
        if (j < 0) break;
        lv = max(lv, __hip_atomic_load(level + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    lv += 1;
    if (lv != __hip_atomic_load(level + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        __hip_atomic_store(level + i, lv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

void launch_vecchia_level_sweep(const int *nbr, int m, int n, int n_fixed, int *level, int *changed, hipStream_t s)
{
    if (n <= n_fixed) return;
    hipLaunchKernelGGL(vecchia_level_sweep_kernel, dim3((unsigned)((n - n_fixed + 255) / 256)), dim3(256), 0, s, nbr, m, n,
                       n_fixed, level, changed);
}

// count[level - 1] += 1 for every row that is not fixed, *depth = the largest level (integer atomics: the counts do not depend
// on their order)
__global__ void __launch_bounds__(256)
vecchia_level_count_kernel(const int *level, int n, int n_fixed, int *count, int *depth)
{
    const size_t i = (size_t)n_fixed + (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const int lv = level[i];
    atomicAdd(count + (lv - 1), 1);
    atomicMax(depth, lv);
}

// order[cursor[level - 1]++] = row: cursor starts as the levels' offsets.  The order of the rows INSIDE a level is that of the
// atomics and may differ from run to run; no result depends on it (the rows of a level are independent).
__global__ void __launch_bounds__(256)
vecchia_level_scatter_kernel(const int *level, int n, int n_fixed, int *cursor, int *order)
{
    const size_t i = (size_t)n_fixed + (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    order[atomicAdd(cursor + (level[i] - 1), 1)] = (int)i;
}

void launch_vecchia_level_count(const int *level, int n, int n_fixed, int *count, int *depth, hipStream_t s)
{
    if (n <= n_fixed) return;
    hipLaunchKernelGGL(vecchia_level_count_kernel, dim3((unsigned)((n - n_fixed + 255) / 256)), dim3(256), 0, s, level, n,
                       n_fixed, count, depth);
}

void launch_vecchia_level_scatter(const int *level, int n, int n_fixed, int *cursor, int *order, hipStream_t s)
{
    if (n <= n_fixed) return;
    hipLaunchKernelGGL(vecchia_level_scatter_kernel, dim3((unsigned)((n - n_fixed + 255) / 256)), dim3(256), 0, s, level, n,
                       n_fixed, cursor, order);
}

// ---------------------------------------------------------------------------
// The recursion for one row and one column: the places of the table in ascending order, one thread, no contraction.
__device__ __forceinline__ void vecchia_sim_row(const VecchiaSimArgs &a, int row, int q)
{
    const double *sr = a.coef + (size_t)row * (a.m + 1);
    const int *nb = a.nbr + (size_t)row * a.m;
    double *x = a.x + (size_t)q * a.ldx;
    double acc = a.W[(size_t)(row - a.w_row0) + (size_t)q * a.ldw];
    // no early way out of the loop, so that the loads of several places are in flight at once; a free place subtracts 0.0,
    // which leaves every bit of acc as it is
#pragma unroll 8
    for (int t = 0; t < a.m; ++t) {
        const int j = nb[t];
        const double term = sr[t] * x[j < 0 ? 0 : j];
        acc -= j < 0 ? 0.0 : term;
    }
    x[row] = acc / sr[a.m];
}

// the rows order[begin .. begin + rows) of one level: item e = q rows + r is row r, column q
__global__ void __launch_bounds__(256)
vecchia_sim_level_kernel(VecchiaSimArgs a, int begin, int rows)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)rows * a.c) return;
    vecchia_sim_row(a, a.order[begin + (int)(e % rows)], (int)(e / rows));
}

// the levels lv0 .. lv1 - 1 (0-based), each of at most VECCHIA_SIM_FUSE_ITEMS (row, column) pairs, in one workgroup.  The barrier orders the
// workgroup's own global stores before its later loads (workgroup scope: one CU, one L1), which is all a level needs of the
// levels of its own run; everything earlier was written by earlier launches.
__global__ void __launch_bounds__(VECCHIA_SIM_FUSE_THREADS)
vecchia_sim_fused_kernel(VecchiaSimArgs a, int lv0, int lv1)
{
    for (int lv = lv0; lv < lv1; ++lv) {
        const int begin = a.off[lv], rows = a.off[lv + 1] - begin;
        for (int e = threadIdx.x; e < rows * a.c; e += VECCHIA_SIM_FUSE_THREADS)
            vecchia_sim_row(a, a.order[begin + e % rows], e / rows);
        __syncthreads();
    }
}

void launch_vecchia_sim_level(const VecchiaSimArgs &a, int begin, int rows, hipStream_t s)
{
    if (rows <= 0) return;
    const size_t items = (size_t)rows * a.c;
    hipLaunchKernelGGL(vecchia_sim_level_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a, begin, rows);
}

void launch_vecchia_sim_fused(const VecchiaSimArgs &a, int lv0, int lv1, hipStream_t s)
{
    if (lv1 <= lv0) return;
    hipLaunchKernelGGL(vecchia_sim_fused_kernel, dim3(1), dim3(VECCHIA_SIM_FUSE_THREADS), 0, s, a, lv0, lv1);
}

// ---------------------------------------------------------------------------
// cocons_sim_vecchia's ends: the fixed rows x[i + q ldx] = z[i, z_col] - X_i mean for every column (the trend as
// vecchia_resid_kernel forms it), and out[(i - n_fixed) + q ldo] = X_i mean + x[i + q ldx] for the rows behind them.
struct VecchiaSimTrendArgs {
    int n, p, n_fixed, c;
    const double *X; int ldx_design;
    double mean[COCONS_P_MAX];
    const double *z;
    double *x; size_t ldx;
    double *out; size_t ldo;
};

__global__ void __launch_bounds__(256)
vecchia_sim_trend_kernel(VecchiaSimTrendArgs a, int fixed)
{
    const int i = (fixed ? 0 : a.n_fixed) + blockIdx.x * 256 + threadIdx.x;
    if (i >= (fixed ? a.n_fixed : a.n)) return;
    double trend = 0.0;
    for (int k = 0; k < a.p; ++k) trend += a.X[i + (size_t)k * a.ldx_design] * a.mean[k];
    if (fixed) {
        const double v = a.z[i] - trend;
        for (int q = 0; q < a.c; ++q) a.x[(size_t)i + (size_t)q * a.ldx] = v;
    } else {
        for (int q = 0; q < a.c; ++q) a.out[(size_t)(i - a.n_fixed) + (size_t)q * a.ldo] = trend + a.x[(size_t)i + (size_t)q * a.ldx];
    }
}

void launch_vecchia_sim_ends(bool fixed, int n, int p, int n_fixed, int c, const double *X, int ldx_design, const double *mean,
                             const double *z, double *x, size_t ldx, double *out, size_t ldo, hipStream_t s)
{
    const int rows = fixed ? n_fixed : n - n_fixed;
    if (rows <= 0) return;
    VecchiaSimTrendArgs a;
    a.n = n; a.p = p; a.n_fixed = n_fixed; a.c = c; a.X = X; a.ldx_design = ldx_design;
    for (int i = 0; i < COCONS_P_MAX; ++i) a.mean[i] = i < p ? mean[i] : 0.0;
    a.z = z; a.x = x; a.ldx = ldx; a.out = out; a.ldo = ldo;
    hipLaunchKernelGGL(vecchia_sim_trend_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, a, fixed ? 1 : 0);
}

}  // namespace cocons
