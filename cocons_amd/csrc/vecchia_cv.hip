// vecchia_cv.hip -- U' of a Vecchia fit and cross-validation from Q = U'U (gfx950).
//
// The table says which columns a row names; every kernel here that applies U' or forms Q needs the opposite, "which rows name
// me".  The transposed lists are built once per handle:
//   vecchia_t_count_kernel     in-degrees by integer atomics
//   vecchia_t_scan_*_kernel    their exclusive prefix sums in three launches (1024 counts per workgroup, the workgroups' totals
//                              by one workgroup, the totals added back); the last one also sorts the columns by list length
//   vecchia_t_fill_kernel      the rows into their lists through an atomic cursor: any order inside a list
//   vecchia_t_sort_*_kernel    every list ascending: a bitonic network in one wavefront's registers (up to 64 rows), in one
//                              workgroup's LDS (up to 4096) or in memory by one workgroup (longer: O(L log^2 L) steps, a barrier
//                              of the workgroup between two of them)
//   vecchia_t_place_kernel     where in its row each entry stands, so that U(k, j) is one load
// and used by
//   vecchia_umul_kernel        y = U b from the records (the formula of cocons_vecchia_unwhiten's header text)
//   vecchia_ut_kernel          U'W and diag(U'U), one wavefront per column
//   vecchia_cv_single_kernel   observations alone in their fold: var = 1 / Q_jj, resid = (U'y)_j var
//   vecchia_cv_fold_kernel     one workgroup per fold of 2 .. 128: Q_BB built in LDS from the rows of U, then cv_fold_tail
// Every floating-point sum runs in an order that is a function of the lists alone; the only atomics are integer ones (counts,
// cursors, the record of a failing fold).  No workgroup waits for another one.
//
// Compile with -ffp-contract=off, like vecchia_sim.hip: the products and sums stand as written.
#include <hip/hip_runtime.h>
#include <atomic>
#include <climits>
#include "kernels.h"
#include "cv_fold_tail.hpp"

namespace cocons {

// ---------------------------------------------------------------------------
// The transposed lists
__global__ void __launch_bounds__(256)
vecchia_t_count_kernel(const int *nbr, size_t entries, int *cnt)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= entries) return;
    const int j = nbr[e];
    if (j >= 0) atomicAdd(cnt + j, 1);
}

void launch_vecchia_t_count(const int *nbr, int m, int n, int *cnt, hipStream_t s)
{
    const size_t entries = (size_t)n * m;
    hipLaunchKernelGGL(vecchia_t_count_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, nbr, entries, cnt);
}

// the exclusive prefix sums of the workgroup's 256 values (one per thread) and, in *total, their sum; buf: 256 ints of LDS
__device__ __forceinline__ int scan256(int v, int *buf, int *total)
{
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int add = t >= d ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const int incl = buf[t];
    *total = buf[255];
    __syncthreads();
    return incl - v;
}

// stage 1: ptr[i] = the prefix sum inside the workgroup's VECCHIA_T_SCAN counts, bsum[workgroup] = their total
__global__ void __launch_bounds__(256)
vecchia_t_scan_local_kernel(const int *cnt, int n, int *ptr, int *bsum)
{
    __shared__ int buf[256];
    constexpr int PER = VECCHIA_T_SCAN / 256;
    const size_t i0 = (size_t)blockIdx.x * VECCHIA_T_SCAN + (size_t)threadIdx.x * PER;
    int v[PER], sum = 0;
    for (int k = 0; k < PER; ++k) {
        v[k] = i0 + k < (size_t)n ? cnt[i0 + k] : 0;
        sum += v[k];
    }
    int total;
    int run = scan256(sum, buf, &total);
    for (int k = 0; k < PER; ++k) {
        if (i0 + k < (size_t)n) ptr[i0 + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// stage 2, one workgroup: bsum[0 .. nb) becomes its exclusive prefix sums, ptr[n] the total
__global__ void __launch_bounds__(256)
vecchia_t_scan_sums_kernel(int *bsum, int nb, int *ptr_n)
{
    __shared__ int buf[256];
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int i = b0 + threadIdx.x;
        const int v = i < nb ? bsum[i] : 0;
        int total;
        const int ex = scan256(v, buf, &total);
        if (i < nb) bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *ptr_n = carry;
}

// stage 3: the workgroups' offsets added back, the columns sorted by list length, cnt zeroed for the fill's cursors
__global__ void __launch_bounds__(256)
vecchia_t_scan_add_kernel(int *cnt, int n, int *ptr, const int *bsum, int *stat, int *mid, int *big)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    ptr[i] += bsum[i / VECCHIA_T_SCAN];
    const int len = cnt[i];
    cnt[i] = 0;
    atomicMax(stat, len);
    if (len == 0) atomicAdd(stat + 1, 1);
    else if (len > VECCHIA_T_LDS) big[atomicAdd(stat + 3, 1)] = (int)i;
    else if (len > VECCHIA_T_WAVE) mid[atomicAdd(stat + 2, 1)] = (int)i;
}

void launch_vecchia_t_scan(int *cnt, int n, int *ptr, int *bsum, int *stat, int *mid, int *big, hipStream_t s)
{
    const int nb = (n + VECCHIA_T_SCAN - 1) / VECCHIA_T_SCAN;
    hipLaunchKernelGGL(vecchia_t_scan_local_kernel, dim3(nb), dim3(256), 0, s, cnt, n, ptr, bsum);
    hipLaunchKernelGGL(vecchia_t_scan_sums_kernel, dim3(1), dim3(256), 0, s, bsum, nb, ptr + n);
    hipLaunchKernelGGL(vecchia_t_scan_add_kernel, dim3((n + 255) / 256), dim3(256), 0, s, cnt, n, ptr, bsum, stat, mid, big);
}

__global__ void __launch_bounds__(256)
vecchia_t_fill_kernel(const int *nbr, int m, size_t entries, const int *ptr, int *cursor, int *rows)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= entries) return;
    const int j = nbr[e];
    if (j >= 0) rows[ptr[j] + atomicAdd(cursor + j, 1)] = (int)(e / m);
}

void launch_vecchia_t_fill(const int *nbr, int m, int n, const int *ptr, int *cursor, int *rows, hipStream_t s)
{
    const size_t entries = (size_t)n * m;
    hipLaunchKernelGGL(vecchia_t_fill_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, nbr, m, entries, ptr,
                       cursor, rows);
}

// lists of 2 .. VECCHIA_T_WAVE rows: wavefront w of the workgroup sorts column 4 blockIdx + w, one row a lane, INT_MAX in the
// lanes behind the list
__global__ void __launch_bounds__(256)
vecchia_t_sort_wave_kernel(int n, const int *ptr, int *rows)
{
    const int lane = threadIdx.x & 63;
    const size_t j = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= (size_t)n) return;
    const int beg = ptr[j], len = ptr[j + 1] - beg;
    if (len < 2 || len > VECCHIA_T_WAVE) return;            // (the same in every lane of the wavefront)
    int v = lane < len ? rows[beg + lane] : INT_MAX;
    for (int k = 2; k <= 64; k <<= 1)
        for (int d = k >> 1; d > 0; d >>= 1) {
            const int o = __shfl_xor(v, d);
            const bool up = (lane & k) == 0, low = (lane & d) == 0;
            v = low == up ? min(v, o) : max(v, o);
        }
    if (lane < len) rows[beg + lane] = v;
}

// lists of VECCHIA_T_WAVE + 1 .. VECCHIA_T_LDS rows: one workgroup per listed column, the list padded with INT_MAX to a power
// of two in LDS
__global__ void __launch_bounds__(256)
vecchia_t_sort_lds_kernel(const int *cols, const int *ptr, int *rows)
{
    __shared__ int buf[VECCHIA_T_LDS];
    const int j = cols[blockIdx.x], beg = ptr[j], len = ptr[j + 1] - beg;
    if (len < 2 || len > VECCHIA_T_LDS) return;
    int P = 2;
    while (P < len) P <<= 1;
    for (int i = threadIdx.x; i < P; i += 256) buf[i] = i < len ? rows[beg + i] : INT_MAX;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int d = k >> 1; d > 0; d >>= 1) {
            for (int i = threadIdx.x; i < P; i += 256) {
                const int o = i ^ d;
                if (o > i) {
                    const int x = buf[i], y = buf[o];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) { buf[i] = y; buf[o] = x; }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < len; i += 256) rows[beg + i] = buf[i];
}

// longer lists: one workgroup of 1024 threads per listed column, the network whose comparators all put the smaller value at
// the lower index (the first step of a merge mirrors its block), in memory.  The places behind the list count as +infinity: a
// comparator that reaches one never swaps, so it is skipped, and no padding is stored.  The workgroup's barrier orders its own
// stores before its later loads; no other workgroup touches the list.
__global__ void __launch_bounds__(1024)
vecchia_t_sort_mem_kernel(const int *cols, const int *ptr, int *rows)
{
    const int j = cols[blockIdx.x], beg = ptr[j], len = ptr[j + 1] - beg;
    if (len < 2) return;
    int *x = rows + beg;
    long long P = 2;
    while (P < len) P <<= 1;
    const long long half = P >> 1;
    for (long long k = 2; k <= P; k <<= 1)
        for (long long d = k >> 1; d > 0; d >>= 1) {
            const bool mirror = d == k >> 1;
            for (long long t = threadIdx.x; t < half; t += 1024) {
                const long long blk = t / d, off = t % d;
                const long long lo = blk * 2 * d + off, hi = mirror ? blk * 2 * d + 2 * d - 1 - off : lo + d;
                if (hi < len) {
                    const int a = x[lo], b = x[hi];
                    if (a > b) { x[lo] = b; x[hi] = a; }
                }
            }
            __syncthreads();
        }
}

void launch_vecchia_t_sort(int n, const int *ptr, int *rows, const int *mid, int nmid, const int *big, int nbig, hipStream_t s)
{
    hipLaunchKernelGGL(vecchia_t_sort_wave_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, n, ptr, rows);
    if (nmid > 0) hipLaunchKernelGGL(vecchia_t_sort_lds_kernel, dim3(nmid), dim3(256), 0, s, mid, ptr, rows);
    if (nbig > 0) hipLaunchKernelGGL(vecchia_t_sort_mem_kernel, dim3(nbig), dim3(1024), 0, s, big, ptr, rows);
}

__global__ void __launch_bounds__(256)
vecchia_t_place_kernel(const int *nbr, int m, size_t entries, const int *ptr, const int *rows, unsigned char *place)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= entries) return;
    const int j = nbr[e];
    if (j < 0) return;
    const int i = (int)(e / m);
    int lo = ptr[j], hi = ptr[j + 1] - 1;               // row i is in the list: the search ends on it
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (rows[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    if (rows[lo] == i) place[lo] = (unsigned char)(e % m);
}

void launch_vecchia_t_place(const int *nbr, int m, int n, const int *ptr, const int *rows, unsigned char *place, hipStream_t s)
{
    const size_t entries = (size_t)n * m;
    hipLaunchKernelGGL(vecchia_t_place_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, nbr, m, entries, ptr,
                       rows, place);
}

// ---------------------------------------------------------------------------
// y = U b: item e = q n + i is row i, column q
__global__ void __launch_bounds__(256)
vecchia_umul_kernel(VecchiaTArgs a, int c, const double *B, size_t ldb, double *Y, size_t ldy)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)a.n * c) return;
    const size_t i = e % a.n, q = e / a.n;
    const double *sr = a.coef + i * (a.m + 1);
    const int *nb = a.nbr + i * a.m;
    const double *b = B + q * ldb;
    double acc = 0.0;
    // (no early way out: a free place adds 0.0, which leaves every bit of acc as it is -- vecchia_sim_row's loop)
#pragma unroll 8
    for (int t = 0; t < a.m; ++t) {
        const int j = nb[t];
        const double term = sr[t] * b[j < 0 ? 0 : j];
        acc += j < 0 ? 0.0 : term;
    }
    acc += sr[a.m] * b[i];
    Y[i + q * ldy] = acc;
}

void launch_vecchia_umul(const VecchiaTArgs &a, int c, const double *B, size_t ldb, double *Y, size_t ldy, hipStream_t s)
{
    const size_t items = (size_t)a.n * c;
    if (items == 0) return;
    hipLaunchKernelGGL(vecchia_umul_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a, c, B, ldb, Y, ldy);
}

// U'W and diag(U'U): wavefront w of the workgroup serves column 4 blockIdx + w.  The columns of W go VECCHIA_UT_COLS at a time
// (up to that many, a list and its coefficients are read once); a column's sums do not know which group they ran in.
constexpr int VECCHIA_UT_COLS = 8;

__global__ void __launch_bounds__(256)
vecchia_ut_kernel(VecchiaTArgs a, int c, const double *W, size_t ldw, double *out, size_t ldo, double *qdiag)
{
    const int lane = threadIdx.x & 63;
    const size_t j = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= (size_t)a.n) return;
    const int kb = a.m + 1, beg = a.ptr[j], end = a.ptr[j + 1];
    for (int q0 = 0; q0 < c; q0 += VECCHIA_UT_COLS) {
        const int nq = min(VECCHIA_UT_COLS, c - q0);
        double acc[VECCHIA_UT_COLS], qd = 0.0;
#pragma unroll
        for (int q = 0; q < VECCHIA_UT_COLS; ++q) acc[q] = 0.0;
        if (lane == 0) {
            const double u = a.coef[j * kb + a.m];
            qd = u * u;
#pragma unroll
            for (int q = 0; q < VECCHIA_UT_COLS; ++q)
                if (q < nq) acc[q] = u * W[j + (size_t)(q0 + q) * ldw];
        }
        for (int e = beg + lane; e < end; e += 64) {
            const size_t k = (size_t)a.rows[e];
            const double u = a.coef[k * kb + a.place[e]];
            qd += u * u;
#pragma unroll
            for (int q = 0; q < VECCHIA_UT_COLS; ++q)
                if (q < nq) acc[q] += u * W[k + (size_t)(q0 + q) * ldw];
        }
        for (int d = 32; d > 0; d >>= 1) {
            qd += __shfl_xor(qd, d);
#pragma unroll
            for (int q = 0; q < VECCHIA_UT_COLS; ++q) acc[q] += __shfl_xor(acc[q], d);
        }
        if (lane == 0) {
            if (q0 == 0 && qdiag) qdiag[j] = qd;
#pragma unroll
            for (int q = 0; q < VECCHIA_UT_COLS; ++q)
                if (q < nq) out[j + (size_t)(q0 + q) * ldo] = acc[q];
        }
    }
}

void launch_vecchia_ut(const VecchiaTArgs &a, int c, const double *W, size_t ldw, double *out, size_t ldo, double *qdiag,
                       hipStream_t s)
{
    if (a.n <= 0) return;
    hipLaunchKernelGGL(vecchia_ut_kernel, dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, s, a, c, W, ldw, out, ldo, qdiag);
}

// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
vecchia_cv_single_kernel(const double *qdiag, const double *uty, size_t ldu, int nr, const int *idx, const int *lab, int count,
                         double *var, double *res, size_t ldr, int *fail)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int i = idx ? idx[t] : t;
    const double k = qdiag[i];
    if (!(k > 0.0) || !isfinite(k)) atomicMin(fail, lab ? lab[t] : t);
    const double v = 1.0 / k;
    var[i] = v;
    for (int c = 0; c < nr; ++c) res[(size_t)i + (size_t)c * ldr] = uty[(size_t)i + (size_t)c * ldu] * v;
}

void launch_vecchia_cv_single(const double *qdiag, const double *uty, size_t ldu, int nr, const int *idx, const int *lab,
                              int count, double *var, double *res, size_t ldr, int *fail, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(vecchia_cv_single_kernel, dim3((count + 255) / 256), dim3(256), 0, s, qdiag, uty, ldu, nr, idx, lab, count,
                       var, res, ldr, fail);
}

// cv_fold_kernel's LDS layout (cv.hip) with the gather replaced: wavefront w owns the members w, w + 4, .. of the fold.  For
// member a it walks a's own row and then list(a) in ascending order; lane t < m + 1 takes place t of the row k at hand (place
// m: k itself), and where that column b is a member of the same fold at or behind a, adds U(k, a) U(k, b) to M(rank b, rank a).
// The lanes of one step name distinct columns and column `rank a` of M is this wavefront's alone: no conflicts, and every
// entry's sum runs over ascending k, the own row of b first (no row before b holds b).
struct VecchiaCvFoldArgs {
    VecchiaTArgs t;
    const int *inv;
    const double *U; size_t ldu; int nr;
    const int *idx, *off, *flist, *lab;
    double *var, *res; size_t ldr;
    int *fail;
};

template <int BP> __global__ void __launch_bounds__(256)
vecchia_cv_fold_kernel(VecchiaCvFoldArgs a)
{
    extern __shared__ double vecchia_cv_lds[];
    constexpr int LD = BP + 1;
    double *M = vecchia_cv_lds, *dinv = M + (size_t)LD * BP, *ub = dinv + BP, *yb = ub + 256;
    const int f = a.flist[blockIdx.x];
    const int base = a.off[f];
    const int *pos = a.idx + base;
    const int b = a.off[f + 1] - base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (b < 1 || b > BP) return;                       // (the host's size classes: never)
    for (int e = tid; e < b * b; e += 256) M[e % b + (e / b) * LD] = 0.0;
    __syncthreads();
    const int m = a.t.m, kb = m + 1;
    for (int ra = wave; ra < b; ra += 4) {
        const int ia = pos[ra], beg = a.t.ptr[ia], len = a.t.ptr[ia + 1] - beg;
        for (int s = -1; s < len; ++s) {
            const size_t k = (size_t)(s < 0 ? ia : a.t.rows[beg + s]);
            const int ta = s < 0 ? m : (int)a.t.place[beg + s];
            const double uka = a.t.coef[k * kb + ta];
            if (lane < kb) {
                const int col = lane < m ? a.t.nbr[k * m + lane] : (int)k;
                if (col >= ia) {
                    const int rb = a.inv[col] - base;
                    if (rb >= 0 && rb < b) M[rb + ra * LD] += uka * a.t.coef[k * kb + lane];
                }
            }
        }
    }
    const bool bad = cv_fold_tail<BP>(M, dinv, ub, yb, b, pos, a.U, a.ldu, a.nr, a.var, a.res, a.ldr);
    if (bad && tid == 0) atomicMin(a.fail, a.lab[f]);
}

template <int BP> static hipError_t vecchia_cv_fold_launch(const VecchiaCvFoldArgs &a, int nfolds, hipStream_t s)
{
    const size_t shm = ((size_t)(BP + 1) * BP + BP + 512) * sizeof(double);
    // more than 64 KB of dynamic LDS needs the kernel's attribute, once per device (cv_fold_launch's handling)
    static std::atomic<unsigned long long> attr_done{0};
    if (shm > 64 * 1024) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (!(dev >= 0 && dev < 64 && ((attr_done.load(std::memory_order_relaxed) >> dev) & 1ull))) {
            if (hipError_t e = hipFuncSetAttribute((const void *)vecchia_cv_fold_kernel<BP>,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm))
                return e;
            if (dev >= 0 && dev < 64) attr_done.fetch_or(1ull << dev, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL(vecchia_cv_fold_kernel<BP>, dim3(nfolds), dim3(256), shm, s, a);
    return hipSuccess;
}

hipError_t launch_vecchia_cv_folds(int cls, const VecchiaTArgs &t, const int *inv, const double *uty, size_t ldu, int nr,
                                   const int *idx, const int *off, const int *flist, const int *lab, int nfolds, double *var,
                                   double *res, size_t ldr, int *fail, hipStream_t s)
{
    if (nfolds <= 0) return hipSuccess;
    VecchiaCvFoldArgs a{t, inv, uty, ldu, nr, idx, off, flist, lab, var, res, ldr, fail};
    switch (cls) {
    case 16: return vecchia_cv_fold_launch<16>(a, nfolds, s);
    case 32: return vecchia_cv_fold_launch<32>(a, nfolds, s);
    case 64: return vecchia_cv_fold_launch<64>(a, nfolds, s);
    case 128: return vecchia_cv_fold_launch<128>(a, nfolds, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace cocons
