// vecchia_solve_t.hip -- U^-T for a Vecchia fit (gfx950): the descending solve over the transposed lists.
//
//   vecchia_tlevel_init_kernel  : tlevel = 1 for the rows n_fixed .. n - 1, 0 in front of them.
//   vecchia_tlevel_sweep_kernel : one push-form relaxation sweep: row k raises every neighbour j >= n_fixed to at least
//                                 tlevel[k] + 1 by an integer atomicMax.  No thread walks a transposed list.
//   vecchia_tkey_kernel         : key = 2 tlevel - 1 for a row of the one-wave tier, 2 tlevel for a row of the wide tier, so
//                                 that launch_vecchia_level_count / _scatter order the rows by (level, tier).
//   vecchia_solve_t_level_kernel: v_j = (w_j - sum_{k in list(j)} U(k, j) v_k) / s_last(j) for the one-wave rows of ONE level,
//                                 one wavefront per (row, group of up to VECCHIA_SOLVE_T_COLS columns).
//   vecchia_solve_t_wide_kernel : the same for the wide rows of one level, one workgroup per (row, group of columns).
//   vecchia_solve_t_fused_kernel: a run of consecutive narrow levels without wide rows in ONE workgroup, a barrier between two.
//   vecchia_unit_cols_kernel    : the unit columns of cocons_vecchia_cov_cols.
//
// The sum over a list is a function of the list alone (kernels.h states the rule); a column's sum does not know the other
// columns.  The only atomics are the integer ones of the levels.  No workgroup waits for another one: the order between
// levels is the order of the launches on the stream, or a workgroup's own barrier.
//
// Compile with -ffp-contract=off, like vecchia_cv.hip: the products and sums stand as written.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "kernels.h"

namespace cocons {

// ---------------------------------------------------------------------------
// Transposed levels
__global__ void __launch_bounds__(256)
vecchia_tlevel_init_kernel(int n, int n_fixed, int *tlevel)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    tlevel[i] = i >= (size_t)n_fixed ? 1 : 0;
}

// Every value is a lower bound of its row's level at any time (it starts as one and is only raised to 1 + such a bound of a row
// of its list), so no store overshoots; a sweep that raises nothing has seen tlevel[j] >= tlevel[k] + 1 for every entry of the
// table behind n_fixed, which with the lower bound is the fixed point.  The plain load in front of the atomic spares a column
// that a million rows name a million atomics per sweep.
__global__ void __launch_bounds__(256)
vecchia_tlevel_sweep_kernel(const int *nbr, int m, int n, int n_fixed, int *tlevel, int *changed)
{
    const size_t k = (size_t)n_fixed + (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (size_t)n) return;
    const int lv = __hip_atomic_load(tlevel + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
    bool raised = false;
    for (int t = 0; t < m; ++t) {
        const int j = nbr[k * m + t];
        if (j < 0) break;
        if (j < n_fixed) continue;
        if (__hip_atomic_load(tlevel + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= lv) continue;
        if (atomicMax(tlevel + j, lv) < lv) raised = true;
    }
    if (raised) __hip_atomic_store(changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256)
vecchia_tkey_kernel(const int *tlevel, const int *ptr, int n, int n_fixed, int wide, int *key)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const int lv = tlevel[i];
    key[i] = i < (size_t)n_fixed ? 0 : 2 * lv - (ptr[i + 1] - ptr[i] > wide ? 0 : 1);
}

void launch_vecchia_tlevel_init(int n, int n_fixed, int *tlevel, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(vecchia_tlevel_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, n_fixed, tlevel);
}

void launch_vecchia_tlevel_sweep(const int *nbr, int m, int n, int n_fixed, int *tlevel, int *changed, hipStream_t s)
{
    if (n <= n_fixed) return;
    hipLaunchKernelGGL(vecchia_tlevel_sweep_kernel, dim3((unsigned)((n - n_fixed + 255) / 256)), dim3(256), 0, s, nbr, m, n,
                       n_fixed, tlevel, changed);
}

void launch_vecchia_tkey(const int *tlevel, const int *ptr, int n, int n_fixed, int wide, int *key, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(vecchia_tkey_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tlevel, ptr, n, n_fixed, wide, key);
}

// ---------------------------------------------------------------------------
// The sum of one list for the columns q0 .. q0 + nq - 1 by `threads` threads of which this is number `tid`: thread t takes the
// entries t, t + threads, .. in ascending order, each as one product added to a sum that starts at 0.0; then the 64 sums of a
// wavefront meet in the butterfly of vecchia_ut_kernel.  Every lane ends with its wavefront's sum.
__device__ __forceinline__ void solve_t_sums(const VecchiaSolveTArgs &a, int beg, int end, int q0, int nq, int tid, int threads,
                                             double (&acc)[VECCHIA_SOLVE_T_COLS])
{
    const int kb = a.m + 1;
#pragma unroll
    for (int q = 0; q < VECCHIA_SOLVE_T_COLS; ++q) acc[q] = 0.0;
    for (int e = beg + tid; e < end; e += threads) {
        const size_t k = (size_t)a.rows[e];
        const double u = a.coef[k * kb + a.place[e]];
        const double *xk = a.x + (k - (size_t)a.row0);
#pragma unroll
        for (int q = 0; q < VECCHIA_SOLVE_T_COLS; ++q)
            if (q < nq) acc[q] += u * xk[(size_t)(q0 + q) * a.ldx];
    }
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
        for (int q = 0; q < VECCHIA_SOLVE_T_COLS; ++q) acc[q] += __shfl_xor(acc[q], d);
    }
}

// one wavefront, item = (row of the level, group of columns); list(j) = rows[beg .. end), piv = s_last(j)
__device__ __forceinline__ void solve_t_wave(const VecchiaSolveTArgs &a, int j, int beg, int end, double piv, int q0, int lane)
{
    const int nq = min(VECCHIA_SOLVE_T_COLS, a.c - q0);
    double acc[VECCHIA_SOLVE_T_COLS];
    solve_t_sums(a, beg, end, q0, nq, lane, 64, acc);
    if (lane == 0) {
        double *xj = a.x + ((size_t)j - (size_t)a.row0);
#pragma unroll
        for (int q = 0; q < VECCHIA_SOLVE_T_COLS; ++q)
            if (q < nq) xj[(size_t)(q0 + q) * a.ldx] = (xj[(size_t)(q0 + q) * a.ldx] - acc[q]) / piv;
    }
}

// the one-wave rows order[begin .. begin + rows) of one level: item e = g rows + r is row r, column group g
__global__ void __launch_bounds__(256)
vecchia_solve_t_level_kernel(VecchiaSolveTArgs a, int begin, int rows)
{
    const size_t e = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const size_t groups = (size_t)(a.c + VECCHIA_SOLVE_T_COLS - 1) / VECCHIA_SOLVE_T_COLS;
    if (e >= (size_t)rows * groups) return;                      // (the same in every lane of the wavefront)
    const int j = a.order[begin + (int)(e % rows)];
    solve_t_wave(a, j, a.ptr[j], a.ptr[j + 1], a.coef[(size_t)j * (a.m + 1) + a.m], (int)(e / rows) * VECCHIA_SOLVE_T_COLS,
                 threadIdx.x & 63);
}

// the wide rows order[begin .. begin + rows) of one level: workgroup b = g rows + r is row r, column group g.  The wavefronts'
// sums go to LDS and thread q adds column q's in ascending order of the wavefront, starting from wavefront 0's.
__global__ void __launch_bounds__(VECCHIA_SOLVE_T_WIDE_THREADS)
vecchia_solve_t_wide_kernel(VecchiaSolveTArgs a, int begin, int rows)
{
    constexpr int WAVES = VECCHIA_SOLVE_T_WIDE_THREADS / 64;
    __shared__ double part[WAVES][VECCHIA_SOLVE_T_COLS];
    const int j = a.order[begin + (int)(blockIdx.x % rows)], q0 = (int)(blockIdx.x / rows) * VECCHIA_SOLVE_T_COLS;
    const int nq = min(VECCHIA_SOLVE_T_COLS, a.c - q0);
    const int tid = threadIdx.x;
    double acc[VECCHIA_SOLVE_T_COLS];
    solve_t_sums(a, a.ptr[j], a.ptr[j + 1], q0, nq, tid, VECCHIA_SOLVE_T_WIDE_THREADS, acc);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < VECCHIA_SOLVE_T_COLS; ++q) part[tid >> 6][q] = acc[q];
    }
    __syncthreads();
    if (tid < nq) {
        double sum = part[0][tid];
        for (int w = 1; w < WAVES; ++w) sum += part[w][tid];
        const double piv = a.coef[(size_t)j * (a.m + 1) + a.m];
        double *xj = a.x + ((size_t)j - (size_t)a.row0) + (size_t)(q0 + tid) * a.ldx;
        *xj = (*xj - sum) / piv;
    }
}

// A wavefront's item of a fused level, fetched ahead of the level: which row, which columns, and this lane's FIRST entry of the
// row's list -- the row k that names it and U(k, row) -- neither of which an earlier level writes.
struct SolveTItem {
    int r = 0, q0 = 0, k = 0, place = 0;
    double u = 0.0;
    bool valid = false, has = false;
};

// solve_t_wave with the lane's first entry at hand: the same products in the same order -- entry `lane` first, then lane + 64, ..
__device__ __forceinline__ void solve_t_wave_ahead(const VecchiaSolveTArgs &a, const SolveTItem &it, int j, int beg, int end,
                                                   double piv, int lane)
{
    const int kb = a.m + 1, nq = min(VECCHIA_SOLVE_T_COLS, a.c - it.q0);
    double *xj = a.x + ((size_t)j - (size_t)a.row0);
    double acc[VECCHIA_SOLVE_T_COLS], w[VECCHIA_SOLVE_T_COLS];
#pragma unroll
    for (int q = 0; q < VECCHIA_SOLVE_T_COLS; ++q) {
        acc[q] = 0.0;
        w[q] = lane == 0 && q < nq ? xj[(size_t)(it.q0 + q) * a.ldx] : 0.0;
    }
    if (it.has) {
        const double *xk = a.x + ((size_t)it.k - (size_t)a.row0);
#pragma unroll
        for (int q = 0; q < VECCHIA_SOLVE_T_COLS; ++q)
            if (q < nq) acc[q] += it.u * xk[(size_t)(it.q0 + q) * a.ldx];
    }
    for (int e = beg + lane + 64; e < end; e += 64) {
        const size_t k = (size_t)a.rows[e];
        const double u = a.coef[k * kb + a.place[e]];
        const double *xk = a.x + (k - (size_t)a.row0);
#pragma unroll
        for (int q = 0; q < VECCHIA_SOLVE_T_COLS; ++q)
            if (q < nq) acc[q] += u * xk[(size_t)(it.q0 + q) * a.ldx];
    }
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
        for (int q = 0; q < VECCHIA_SOLVE_T_COLS; ++q) acc[q] += __shfl_xor(acc[q], d);
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < VECCHIA_SOLVE_T_COLS; ++q)
            if (q < nq) xj[(size_t)(it.q0 + q) * a.ldx] = (w[q] - acc[q]) / piv;
    }
}

// the levels lv0 .. lv1 - 1 (0-based), none with a wide row, each of at most VECCHIA_SOLVE_T_FUSE_ITEMS items -- one per
// wavefront at the most -- and together of at most VECCHIA_SOLVE_T_FUSE_ROWS rows, in one workgroup.  What a row's item needs
// and no earlier level writes is taken off the level's chain of dependent loads: the rows, the bounds of their lists and their
// pivots come to LDS for the whole run in one pass of all threads; then, while level l is solved, every wavefront loads its
// lane's first entry for level l + 2 and that entry's coefficient for level l + 1, so that level l itself waits for the values
// x alone.  The barrier orders the workgroup's own global stores before its later loads (vecchia_sim_fused_kernel's argument);
// everything earlier was written by earlier launches.  a.off holds two offsets per level; without wide rows the run's rows
// are order[off[2 lv0] .. off[2 lv1]) and level lv's start at off[2 lv].
__global__ void __launch_bounds__(VECCHIA_SOLVE_T_FUSE_THREADS)
vecchia_solve_t_fused_kernel(VecchiaSolveTArgs a, int lv0, int lv1)
{
    constexpr int WAVES = VECCHIA_SOLVE_T_FUSE_THREADS / 64, CAP = VECCHIA_SOLVE_T_FUSE_ROWS;
    static_assert(VECCHIA_SOLVE_T_FUSE_ITEMS <= WAVES, "one item per wavefront and level");
    __shared__ int s_beg[CAP + 1], s_row[CAP], s_lo[CAP], s_hi[CAP];
    __shared__ double s_piv[CAP];
    const int groups = (a.c + VECCHIA_SOLVE_T_COLS - 1) / VECCHIA_SOLVE_T_COLS;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kb = a.m + 1;
    const int nlev = lv1 - lv0, base = a.off[2 * lv0], total = a.off[2 * lv1] - base;
    if (nlev > CAP || total > CAP) return;                      // (the host's plan: never)
    for (int l = threadIdx.x; l <= nlev; l += VECCHIA_SOLVE_T_FUSE_THREADS) s_beg[l] = a.off[2 * (lv0 + l)] - base;
    for (int r = threadIdx.x; r < total; r += VECCHIA_SOLVE_T_FUSE_THREADS) {
        const int j = a.order[base + r];
        s_row[r] = j;
        s_lo[r] = a.ptr[j];
        s_hi[r] = a.ptr[j + 1];
        s_piv[r] = a.coef[(size_t)j * kb + a.m];
    }
    __syncthreads();
    // the item of level l for this wavefront and its lane's first entry (the row and the place; the coefficient comes a level later)
    auto item = [&](int l) {
        SolveTItem it;
        if (l >= nlev) return it;
        const int begin = s_beg[l], rows = s_beg[l + 1] - begin;
        if (wave >= rows * groups) return it;
        it.valid = true;
        it.r = begin + wave % rows;
        it.q0 = (wave / rows) * VECCHIA_SOLVE_T_COLS;
        const int e = s_lo[it.r] + lane;
        if (e < s_hi[it.r]) { it.has = true; it.k = a.rows[e]; it.place = a.place[e]; }
        return it;
    };
    auto coefficient = [&](SolveTItem &it) { if (it.has) it.u = a.coef[(size_t)it.k * kb + it.place]; };
    SolveTItem i0 = item(0), i1 = item(1);
    coefficient(i0);
    for (int l = 0; l < nlev; ++l) {
        SolveTItem i2 = item(l + 2);
        coefficient(i1);
        if (i0.valid) solve_t_wave_ahead(a, i0, s_row[i0.r], s_lo[i0.r], s_hi[i0.r], s_piv[i0.r], lane);
        __syncthreads();
        i0 = i1;
        i1 = i2;
    }
}

// A launch's threads stay below 2^32 whatever the level and the columns: the rows go in pieces of at most `piece` and the
// column groups in pieces of whatever then fits (a piece of rows or of column groups is as independent as a whole level).
template <class Launch>
static void solve_t_pieces(const VecchiaSolveTArgs &a, int begin, int rows, size_t piece, Launch launch)
{
    const int groups = (a.c + VECCHIA_SOLVE_T_COLS - 1) / VECCHIA_SOLVE_T_COLS;
    for (int r0 = 0; r0 < rows;) {
        const int nr = (int)std::min<size_t>((size_t)(rows - r0), piece);
        const int gmax = (int)std::max<size_t>(1, piece / (size_t)nr);
        for (int g0 = 0; g0 < groups; g0 += gmax) {
            VecchiaSolveTArgs b = a;
            b.x = a.x + (size_t)g0 * VECCHIA_SOLVE_T_COLS * a.ldx;
            b.c = std::min(a.c - g0 * VECCHIA_SOLVE_T_COLS, gmax * VECCHIA_SOLVE_T_COLS);
            launch(b, begin + r0, nr, (size_t)nr * ((b.c + VECCHIA_SOLVE_T_COLS - 1) / VECCHIA_SOLVE_T_COLS));
        }
        r0 += nr;
    }
}

void launch_vecchia_solve_t_level(const VecchiaSolveTArgs &a, int begin, int rows, hipStream_t s)
{
    if (rows <= 0 || a.c <= 0) return;
    solve_t_pieces(a, begin, rows, (size_t)1 << 24, [s](const VecchiaSolveTArgs &b, int b0, int nr, size_t items) {
        hipLaunchKernelGGL(vecchia_solve_t_level_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, b, b0, nr);
    });
}

void launch_vecchia_solve_t_wide(const VecchiaSolveTArgs &a, int begin, int rows, hipStream_t s)
{
    if (rows <= 0 || a.c <= 0) return;
    solve_t_pieces(a, begin, rows, (size_t)1 << 20, [s](const VecchiaSolveTArgs &b, int b0, int nr, size_t items) {
        hipLaunchKernelGGL(vecchia_solve_t_wide_kernel, dim3((unsigned)items), dim3(VECCHIA_SOLVE_T_WIDE_THREADS), 0, s, b, b0, nr);
    });
}

void launch_vecchia_solve_t_fused(const VecchiaSolveTArgs &a, int lv0, int lv1, hipStream_t s)
{
    if (lv1 <= lv0 || a.c <= 0) return;
    hipLaunchKernelGGL(vecchia_solve_t_fused_kernel, dim3(1), dim3(VECCHIA_SOLVE_T_FUSE_THREADS), 0, s, a, lv0, lv1);
}

// ---------------------------------------------------------------------------
// B[r + q ldb] = 1 where r + row0 = idx[q] (0-based row of the table), 0 elsewhere, for r < rows, q < nidx
__global__ void __launch_bounds__(256)
vecchia_unit_cols_kernel(const int *idx, int nidx, int rows, int row0, double *B, size_t ldb)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)rows * nidx) return;
    const size_t r = e % rows, q = e / rows;
    B[r + q * ldb] = (long long)r + row0 == (long long)idx[q] ? 1.0 : 0.0;
}

void launch_vecchia_unit_cols(const int *idx, int nidx, int rows, int row0, double *B, size_t ldb, hipStream_t s)
{
    const size_t items = (size_t)rows * nidx;
    if (items == 0) return;
    hipLaunchKernelGGL(vecchia_unit_cols_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, idx, nidx, rows, row0, B,
                       ldb);
}

}  // namespace cocons
