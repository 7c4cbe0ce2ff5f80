// vecchia_block.hpp -- the phases of a Vecchia block in LDS: what every block kernel of vecchia.hip (one
// wavefront per observation, T = 64 threads) and of vecchia_group.hip (one workgroup per block of rows, T =
// VECCHIA_GROUP_THREADS) is a sequence of, the LDS layouts of those kernels, and the host's way from `mode` to an instantiation.
// A kernel that calls a phase runs that phase's code, so what two launches are said to share to the bit they share by
// construction.  Every phase states the order of its sums; none depends on T but through the deal of independent elements.
//
// Compile with -ffp-contract=off (see matern_device.hpp): the products and sums stand as written.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <type_traits>
#include "kernels.h"
#include "matern_device.hpp"
#include "grad_pair.hpp"

namespace cocons {

// element (r, c), r >= c, of the packed lower triangle (row after row)
__host__ __device__ __forceinline__ int tri_at(int r, int c) { return r * (r + 1) / 2 + c; }

// pair t = r (r - 1) / 2 + c of the packed strict lower triangle, r > c
__device__ __forceinline__ void tri_pair(int t, int &r, int &c)
{
    r = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)t)) * 0.5f);
    while (r * (r - 1) / 2 > t) --r;
    while ((r + 1) * r / 2 <= t) ++r;
    c = t - r * (r - 1) / 2;
}

// a fixed butterfly over the 64 lanes of a wavefront
__device__ __forceinline__ double vecchia_wave_sum(double v)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------
// The LDS layouts: offsets in doubles from the start of the dynamic LDS, written once -- the kernel carves its pointers from
// the struct, the host's *_lds_bytes function returns its end.  kb: the rows the launch is sized by.
//   par   LOCP_FIELDS x kb   the block's parameters as an SoA of stride kb -- what pair_value_idx reads;
//   par2  LOCP_FIELDS x kb   prediction only: the same rows in the prediction branch's parameters, the prediction site last;
//   tri   kb (kb + 1) / 2    the block, then its factor (the pivots stay in registers: lane r keeps C(r, r));
//   nb    kb ints            the rows' locations, behind everything else.
struct VecchiaValueLds { int par, par2, tri, nb; size_t bytes; };
__host__ __device__ inline VecchiaValueLds vecchia_value_lds(int kb, bool pred)
{
    VecchiaValueLds l;
    l.par = 0; l.par2 = pred ? LOCP_FIELDS * kb : 0; l.tri = l.par2 + LOCP_FIELDS * kb;
    l.nb = l.tri + kb * (kb + 1) / 2;
    l.bytes = (size_t)l.nb * sizeof(double) + (size_t)kb * sizeof(int);
    return l;
}

// The gradient keeps tri at `stg` doubles or more -- once the backward solves are done the factor is dead and the pair walk
// stages a pass there -- and puts behind it:
//   sm, nm  kb (kb + 1) / 2 each  grouped only: row p is the member's s_p, and N[p, 0..p], then h_p in the places 0 .. p - 1;
//   sp    GSITE_FIELDS x kb  the rows' site derivatives (grad_site_kernel's fields) as an SoA of stride kb;
//   v1, v2  kb each          ungrouped: s = L^-T e_last and h = L^-T v; grouped: sum_c y_pc of the members and u = sum_p ys[p] s_p;
//   gs    2 GFAM x kb        the rows' site sums: the log-determinant's share per family, then the quadratic forms';
//   red   2 x waves          grouped only: the wavefronts' shares of the two global-range sums.
constexpr int VECCHIA_STG = 4 * GFAM * 64;                                   // ungrouped: (ii, jj side) x (two shares) x GFAM a pair
constexpr int VECCHIA_GROUP_STGF = 2 * GFAM + 2;                             // grouped, a staged pair: da, db, 2 W_log, 2 W_quad
constexpr int VECCHIA_GROUP_STG = VECCHIA_GROUP_STGF * VECCHIA_GROUP_THREADS;
constexpr int VECCHIA_GROUP_WAVES = VECCHIA_GROUP_THREADS / 64;
struct VecchiaGradLds { int par, tri, sm, nm, sp, v1, v2, gs, red, nb; size_t bytes; };
__host__ __device__ inline VecchiaGradLds vecchia_grad_lds(int kb, bool grouped)
{
    const int ntri = kb * (kb + 1) / 2, stg = grouped ? VECCHIA_GROUP_STG : VECCHIA_STG;
    VecchiaGradLds l;
    l.par = 0; l.tri = LOCP_FIELDS * kb;
    l.sm = l.tri + (ntri < stg ? stg : ntri); l.nm = l.sm + (grouped ? ntri : 0);
    l.sp = l.nm + (grouped ? ntri : 0); l.v1 = l.sp + GSITE_FIELDS * kb; l.v2 = l.v1 + kb; l.gs = l.v2 + kb;
    l.red = l.gs + 2 * GFAM * kb; l.nb = l.red + (grouped ? 2 * VECCHIA_GROUP_WAVES : 0);
    l.bytes = (size_t)l.nb * sizeof(double) + (size_t)kb * sizeof(int);
    return l;
}

// The information keeps the factor in tri and puts behind it, for groups of gd directions and (grouped) chunks of mc members:
//   sm    kb (kb + 1) / 2    grouped only: row p is the member's s_p;
//   sp    VECCHIA_FX x kb    the rows' site derivatives, then two vectors of kb doubles -- ungrouped: sv = s and one unused;
//                            grouped: the members' positions, ascending (kb ints);
//   wts   gd x GFAM x kb     the rows' site weights w_a[f][row] of the group's directions;
//   stg   gd x T             a pass of T pairs: the entry of C_a per direction (and the sums u of the mean block);
//   gall  mc x ndir x kb     g_a = L^-1 (C_a s) of every direction (grouped: and member of the chunk), what the Gram is formed of.
constexpr int VECCHIA_FX = GSITE_FIELDS + 2;
struct VecchiaFisherLds { int par, tri, sm, sp, sv, wts, stg, gall, nb; size_t bytes; };
__host__ __device__ inline VecchiaFisherLds vecchia_fisher_lds(int kb, int ndir, int gd, int mc, bool grouped)
{
    const int ntri = kb * (kb + 1) / 2;
    VecchiaFisherLds l;
    l.par = 0; l.tri = LOCP_FIELDS * kb; l.sm = l.tri + ntri; l.sp = l.sm + (grouped ? ntri : 0);
    l.sv = l.sp + GSITE_FIELDS * kb; l.wts = l.sp + VECCHIA_FX * kb; l.stg = l.wts + gd * GFAM * kb;
    l.gall = l.stg + gd * (grouped ? VECCHIA_GROUP_THREADS : 64); l.nb = l.gall + ndir * mc * kb;
    l.bytes = (size_t)l.nb * sizeof(double) + (size_t)kb * sizeof(int);
    return l;
}

// ---------------------------------------------------------------------------
// Gather of the parameter records of the rows nb[0 .. nrows) into the SoA par; no sums.
template <int T>
__device__ __forceinline__ void vecchia_gather_params(double *par, int kb, const int *nb, int nrows, const double *aos, int tid)
{
    for (int e = tid; e < nrows * VECCHIA_REC; e += T) {
        const int r = e / VECCHIA_REC, f = e % VECCHIA_REC;
        if (f >= LOCP_FIELDS) continue;
        par[f * kb + r] = aos[(size_t)nb[r] * VECCHIA_REC + f];
    }
}

// Gather of the site records (launch_vecchia_site_rec's) of the rows nb[0 .. nrows) into the SoA sp; no sums.
template <int T>
__device__ __forceinline__ void vecchia_gather_sites(double *sp, int kb, const int *nb, int nrows, const double *aosG, int tid)
{
    for (int e = tid; e < nrows * VECCHIA_GSITE_REC; e += T) {
        const int r = e / VECCHIA_GSITE_REC, f = e % VECCHIA_GSITE_REC;
        sp[f * kb + r] = aosG[(size_t)nb[r] * VECCHIA_GSITE_REC + f];
    }
}

// Assembly of the strict triangle and the diagonal: pair t = r (r - 1) / 2 + c is (r, c), r > c, evaluated with the EARLIER
// row on the `ii` side (the reference's orientation, which the u <= eps rule sees).  PRED, last row: the prediction site on
// the `ii` side, exact coordinate matches give its own diagonal value (cov_rns_pred).  No sums: a pair's value does not
// depend on the thread that evaluates it, on the stride or on the place of its rows in LDS.
template <int MODE, int T, bool PRED = false>
__device__ __forceinline__ void vecchia_assemble(const double *par, const double *par2, double *tri, int kb, int nrows, double gr,
                                                 double nu_fixed, int tid)
{
    const int npairs = nrows * (nrows - 1) / 2;
    for (int t = tid; t < npairs; t += T) {
        int r, c;
        tri_pair(t, r, c);
        double v;
        if (PRED && r == nrows - 1) v = pair_value_idx<MODE_GEOM>(par2, (size_t)kb, r, par2, (size_t)kb, c, gr, 0.0, true);
        else v = pair_value_idx<MODE>(par, (size_t)kb, c, par, (size_t)kb, r, gr, nu_fixed, false);
        tri[tri_at(r, c)] = v;
    }
    if (tid < nrows) tri[tri_at(tid, tid)] = par[11 * kb + tid];
}

// The factorisation K = C C' on the leading nf of nrows rows, right-looking, one column per step, thread = row (a thread at
// or behind nrows passes the barriers with nothing to do).  Element (r, c) is touched in ascending j only, with operands of
// the leading sub-block, so the factor of a leading sub-block is the leading sub-block of the factor.  piv_mine: C(r, r) of
// the thread's row.  Returns the first column whose pivot is not positive and finite (the same in every thread), or -1.
__device__ __forceinline__ int vecchia_factor(double *tri, int nrows, int nf, int tid, double &piv_mine)
{
    const int myrow = tri_at(tid, 0);
    piv_mine = 1.0;
    for (int j = 0; j < nf; ++j) {
        __syncthreads();
        const double d = tri[tri_at(j, j)];
        if (!(d > 0.0) || !isfinite(d)) return j;
        const double piv = sqrt(d);
        if (tid == j) piv_mine = piv;
        double lrj = 0.0;
        if (tid > j && tid < nrows) { lrj = tri[myrow + j] / piv; tri[myrow + j] = lrj; }
        __syncthreads();
        if (tid > j && tid < nrows)
            for (int c = j + 1; c <= tid; ++c) tri[myrow + c] -= lrj * tri[tri_at(c, j)];
    }
    return -1;
}

// gather, assembly and factorisation of the whole block in one: what every launch but the prediction's opens with
template <int MODE, int T, bool SITES>
__device__ __forceinline__ int vecchia_open_block(double *par, double *sp, double *tri, int kb, const int *nb, int nrows,
                                                  const double *aosK, const double *aosG, double gr, double nu_fixed, int tid,
                                                  double &piv_mine)
{
    vecchia_gather_params<T>(par, kb, nb, nrows, aosK, tid);
    if constexpr (SITES) vecchia_gather_sites<T>(sp, kb, nb, nrows, aosG, tid);
    __syncthreads();
    vecchia_assemble<MODE, T>(par, par, tri, kb, nrows, gr, nu_fixed, tid);
    return vecchia_factor(tri, nrows, nrows, tid, piv_mine);
}

// Forward substitution over the rows 0 .. k - 1 for VECCHIA_G right-hand sides in registers, lane = row: lane r ends with
// b_r - sum_{j < r} C(r, j) y_j, j ascending (the numerator of y_r: the steps from r on leave it alone).
__device__ __forceinline__ void vecchia_forward(double (&b)[VECCHIA_G], const double *tri, int myrow, double piv_mine, int lane,
                                                int k, int nrows)
{
    for (int j = 0; j < k; ++j) {
        const double l = (lane > j && lane < nrows) ? tri[myrow + j] : 0.0;
#pragma unroll
        for (int g = 0; g < VECCHIA_G; ++g) {
            const double yj = __shfl(lane == j ? b[g] / piv_mine : 0.0, j);
            b[g] -= l * yj;
        }
    }
}

// The backward solves x_g = L_{0..p_g}^-T r_g for N right-hand sides in registers, lane = row, one column of L' (a row of
// the packed factor) per step from `top` = the largest p_g down; a right-hand side sits out the steps above its p_g.  Lane j
// ends with component j: x_g[j] = (r_g[j] - sum_{i > j} L(i, j) x_g[i]) OVER L(j, j), i descending from p_g.  The two forms of
// "over" are not the same bits, and each caller keeps its own: PIV_DIVIDE divides by the pivot pv (the ungrouped launches and
// the grouped coefficients, whose records are launch_vecchia_coefs'); PIV_RECIPROCAL multiplies by pv = 1 / pivot, formed
// once per lane (the grouped gradient and information, which solve once per member).
enum VecchiaPivot { PIV_DIVIDE, PIV_RECIPROCAL };
template <VecchiaPivot PIV, bool STAGGERED, int N>
__device__ __forceinline__ void vecchia_backward_steps(double (&r)[N], double (&x)[N], const double *tri, double pv, int ln, int top,
                                                       const int (&p)[N])
{
    for (int j = top; j >= 0; --j) {
        const double l = ln < j ? tri[tri_at(j, 0) + ln] : 0.0;
#pragma unroll
        for (int g = 0; g < N; ++g) {
            if (STAGGERED && j > p[g]) continue;                                 // (the same in every lane)
            const double xg = __shfl(PIV == PIV_DIVIDE ? r[g] / pv : r[g] * pv, j);
            if (ln == j) x[g] = xg;
            if (ln < j) r[g] -= l * xg;
        }
    }
}
// ... all N from the one position top
template <VecchiaPivot PIV, int N>
__device__ __forceinline__ void vecchia_backward(double (&r)[N], double (&x)[N], const double *tri, double pv, int ln, int top)
{
    const int none[N] = {};
    vecchia_backward_steps<PIV, false>(r, x, tri, pv, ln, top, none);
}
// ... each from its own position p[g] <= top (p[g] < 0: no right-hand side)
template <VecchiaPivot PIV, int N>
__device__ __forceinline__ void vecchia_backward(double (&r)[N], double (&x)[N], const double *tri, double pv, int ln, int top,
                                                 const int (&p)[N])
{
    vecchia_backward_steps<PIV, true>(r, x, tri, pv, ln, top, p);
}

// The walk's collection rule: the staged pairs of the pass [t0, tend) that belong to row ln, in the order that fixes every
// site sum -- jj(slot, c) for its pairs (ln, c), c < ln ascending (the jj side), then ii(slot, r) for its pairs (r, ln),
// r > ln ascending (the ii side); slot = t - t0 is the pair's place in the staging.
template <class FJ, class FI>
__device__ __forceinline__ void vecchia_row_pairs(int ln, int t0, int tend, FJ &&jj, FI &&ii)
{
    const int mine0 = ln * (ln - 1) / 2;
    for (int u = max(t0, mine0); u < min(tend, mine0 + ln); ++u) jj(u - t0, u - mine0);
    int r_lo, r_hi, c_;
    tri_pair(t0, r_lo, c_);
    tri_pair(tend - 1, r_hi, c_);
    for (int r = max(r_lo, ln + 1); r <= r_hi; ++r) {
        const int u = r * (r - 1) / 2 + ln;
        if (u < t0 || u >= tend) continue;
        ii(u - t0, r);
    }
}

// sum_{rr < nrows} g[rr] X[site(rr), kx], the rows ascending: the contraction of a per-row vector with a column of X
__device__ __forceinline__ double vecchia_dot_x(const double *g, int nrows, const int *nb, const double *X, int ldx, int kx)
{
    double s = 0.0;
    for (int rr = 0; rr < nrows; ++rr) s += g[rr] * X[(size_t)nb[rr] + (size_t)kx * ldx];
    return s;
}

// The information's site weights of the gd directions from d0 on: w_a[f][row] = c_f sum_k X[site(row), k] dirs[a][f, k],
// k ascending; scale: c = 2 over k >= 1 (k = 0 is the global range)
template <int T>
__device__ __forceinline__ void vecchia_site_weights(double *wts, int kb, int nrows, const int *nb, const double *X, int ldx, int p,
                                                     const double *dirs, int d0, int gd, int tid)
{
    for (int e = tid; e < gd * GFAM * nrows; e += T) {
        const int rr = e % nrows, f = (e / nrows) % GFAM, d = e / (nrows * GFAM);
        const double *v = dirs + ((size_t)(d0 + d) * GFAM + f) * p;
        double w = 0.0;
        for (int kx = (f == TH_SCALE_ ? 1 : 0); kx < p; ++kx) w += X[(size_t)nb[rr] + (size_t)kx * ldx] * v[kx];
        wts[(d * GFAM + f) * kb + rr] = f == TH_SCALE_ ? 2.0 * w : w;
    }
}

// The pair walk of the information, one pass: thread tid's pair t (if there is one) evaluated once and its entry of C_a
// staged for the gd directions from d0 on: the global range's share first, then per family the jj side's and the ii side's.
template <int MODE, int T>
__device__ __forceinline__ void vecchia_stage_dir_entries(double *stg, const double *wts, const double *par, const double *sp, int kb,
                                                          double gr, double nu_fixed, int smooth_free, const double *dirs, int p,
                                                          int d0, int gd, int t, int npairs, int tid)
{
    double da[GFAM], db[GFAM], dg = 0.0;
    int r = 0, c = 0;
#pragma unroll
    for (int f = 0; f < GFAM; ++f) { da[f] = 0.0; db[f] = 0.0; }
    if (t < npairs) {
        tri_pair(t, r, c);
        pair_partials<MODE>(par, (size_t)kb, sp, (size_t)kb, gr, nu_fixed, smooth_free, c, r, da, db, dg);
    }
    for (int d = 0; d < gd; ++d) {
        double e = 0.0;
        if (t < npairs) {
            const double *w = wts + d * GFAM * kb;
            e = dg * dirs[((size_t)(d0 + d) * GFAM + TH_SCALE_) * p];
#pragma unroll
            for (int f = 0; f < GFAM; ++f) {
                e += da[f] * w[f * kb + c];
                e += db[f] * w[f * kb + r];
            }
        }
        stg[d * T + tid] = e;
    }
}

// The Gram record's share of one block on its leading p + 1 rows, added to s: sum_{j < p} g_a[j] g_b[j], j ascending, then
// g_a[p] g_b[p] / 2
__device__ __forceinline__ double vecchia_gram_add(double s, const double *ga, const double *gb, int p)
{
    for (int j = 0; j < p; ++j) s += ga[j] * gb[j];
    return s + 0.5 * (ga[p] * gb[p]);
}

// ---------------------------------------------------------------------------
// Host: f(std::integral_constant<int, MODE>) for the smoothness mode of the launch
template <class F> inline void vecchia_with_mode(int mode, F &&f)
{
    switch (mode) {
    case MODE_HALF: f(std::integral_constant<int, MODE_HALF>()); break;
    case MODE_THREEHALF: f(std::integral_constant<int, MODE_THREEHALF>()); break;
    case MODE_FIVEHALF: f(std::integral_constant<int, MODE_FIVEHALF>()); break;
    default: f(std::integral_constant<int, MODE_GEOM>()); break;
    }
}

// one launch of a block kernel; cap: where shm may pass 64 KB, the bytes its attribute is raised to (once per device)
template <class A>
inline void vecchia_launch_kernel(void (*kernel)(A), const A &a, int blocks, int threads, size_t shm, hipStream_t s,
                                  std::atomic<unsigned long long> *attr_done = nullptr, size_t cap = 0)
{
    if (attr_done && shm > 64 * 1024) set_dynamic_lds_once((const void *)kernel, cap, *attr_done);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3((unsigned)threads), shm, s, a);
}

}  // namespace cocons
