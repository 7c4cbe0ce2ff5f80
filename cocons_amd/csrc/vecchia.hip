// vecchia.hip -- the Vecchia approximation's per-observation blocks (gfx950).
//
//   vecchia_aos_kernel    : loc_params_kernel's SoA (LOCP_FIELDS x stride) transposed to one 128-byte record of 16 doubles
//                           per location, so that gathering a neighbour's parameters costs one cache line instead of 13.
//   vecchia_resid_kernel  : z[:, col0 ..] - X mean in rhs_rows_kernel's arithmetic, one column per realisation.
//   vecchia_value_kernel  : ONE WAVEFRONT per observation (a workgroup of 64 lanes): the parameters of the observation and
//                           of its k <= 63 neighbours gathered into LDS, the (k + 1) x (k + 1) covariance block assembled with
//                           pair_value_idx -- the dense assembly's arithmetic -- into a packed lower triangle in LDS, factored
//                           there column by column with lane = row, and the right-hand sides carried through the forward
//                           substitution in registers.  PRED: the last row is a prediction site and stays out of the factor.
//   vecchia_grad_kernel, vecchia_fisher_kernel, vecchia_coef_kernel : the same phases (vecchia_block.hpp), then the block's
//                           share of the gradient, of the expected information (4t), or its row of U (4v).
//   vecchia_sum_kernel    : the totals over the per-observation terms, as a two-stage tree of fixed shape.
//
// Every sum of a block runs in ascending row order of the block, which the host makes the ascending order of the caller's
// indices; nothing a block computes depends on another block, on n or on the launch.  No atomics but the integer atomicMin
// that reports a failing block.
//
// Compile with -ffp-contract=off (see matern_device.hpp).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "kernels.h"
#include "vecchia_block.hpp"

namespace cocons {

// ---------------------------------------------------------------------------
// 64 locations per workgroup through an LDS tile: reads along the SoA's rows, writes along the records
__global__ void __launch_bounds__(256)
vecchia_aos_kernel(const double *soa, size_t stride, int n, double *aos)
{
    __shared__ double tile[LOCP_FIELDS][65];
    const int base = blockIdx.x * 64, t = threadIdx.x;
    for (int e = t; e < LOCP_FIELDS * 64; e += 256) {
        const int f = e >> 6, s = e & 63;
        if (base + s < n) tile[f][s] = soa[(size_t)f * stride + (size_t)(base + s)];
    }
    __syncthreads();
    for (int e = t; e < VECCHIA_REC * 64; e += 256) {
        const int s = e / VECCHIA_REC, f = e % VECCHIA_REC;
        if (base + s < n) aos[(size_t)(base + s) * VECCHIA_REC + f] = f < LOCP_FIELDS ? tile[f][s] : 0.0;
    }
}

void launch_vecchia_aos(const double *soa, size_t stride, int n, double *aos, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(vecchia_aos_kernel, dim3((n + 63) / 64), dim3(256), 0, s, soa, stride, n, aos);
}

// the four site derivatives of grad_site_kernel as one 32-byte record per location: what the gradient launch gathers beside
// the parameters' records
__global__ void __launch_bounds__(256)
vecchia_site_rec_kernel(const double *soa, size_t stride, int n, double *rec)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * VECCHIA_GSITE_REC) return;
    const size_t i = e / VECCHIA_GSITE_REC, f = e % VECCHIA_GSITE_REC;
    rec[e] = soa[f * stride + i];
}

void launch_vecchia_site_rec(const double *soa, size_t stride, int n, double *rec, hipStream_t s)
{
    if (n <= 0) return;
    const size_t total = (size_t)n * VECCHIA_GSITE_REC;
    hipLaunchKernelGGL(vecchia_site_rec_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, soa, stride, n, rec);
}

// out[i + k ldo] = z[i + (col0 + k) ldz] - (X mean)[i]; the trend as rhs_rows_kernel forms it (a plain dot product, i ascending)
struct VecchiaResidArgs {
    int n, p;
    const double *X; int ldx;
    double mean[COCONS_P_MAX];
    const double *z; int ldz; int col0, ncol;
    double *out; size_t ldo;
};

__global__ void __launch_bounds__(256)
vecchia_resid_kernel(VecchiaResidArgs a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n) return;
    double trend = 0.0;
    for (int i = 0; i < a.p; ++i) trend += a.X[c + (size_t)i * a.ldx] * a.mean[i];
    for (int k = 0; k < a.ncol; ++k) a.out[c + (size_t)k * a.ldo] = a.z[c + (size_t)(a.col0 + k) * a.ldz] - trend;
}

void launch_vecchia_resid(int n, int p, const double *X, int ldx, const double *mean, const double *z, int ldz, int col0,
                          int ncol, double *out, size_t ldo, hipStream_t s)
{
    VecchiaResidArgs a;
    a.n = n; a.p = p; a.X = X; a.ldx = ldx;
    for (int i = 0; i < COCONS_P_MAX; ++i) a.mean[i] = i < p ? mean[i] : 0.0;
    a.z = z; a.ldz = ldz; a.col0 = col0; a.ncol = ncol; a.out = out; a.ldo = ldo;
    hipLaunchKernelGGL(vecchia_resid_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------
// The block kernels: ONE WAVEFRONT per observation, lane = row.  The LDS layouts stand in vecchia_block.hpp.

// the row's neighbours -- ascending, the free places (-1) behind them -- and then the row itself (prediction: the prediction
// site) into nb, behind a barrier; returns k, the number of neighbours
__device__ __forceinline__ int vecchia_rows(const VecchiaArgs &a, int row, int lane, int *nb)
{
    const int mine = lane < a.m ? a.nbr[(size_t)row * a.m + lane] : -1;
    const int k = __popcll(__ballot(mine >= 0));
    if (lane < k) nb[lane] = mine;
    if (lane == k) nb[lane] = row;
    __syncthreads();
    return k;
}

__device__ __forceinline__ void vecchia_report(const VecchiaArgs &a, int lane, int row1)
{
    if (lane == 0) atomicMin(a.fail, row1);
}

// The right-hand sides through the forward substitution over the neighbours' rows, VECCHIA_G at a time; lane k ends with
// b_k - sum_j C(k, j) y_j, j ascending, and stores Y[row, c] = that / pivot (PRED: stoch[row] = -that) and log d.
// each(b, c0): the numerators of the columns c0 .. in every lane (lane j: of w_c[j], the steps from j on leave it alone).
template <bool PRED, class F>
__device__ __forceinline__ void vecchia_columns(const VecchiaArgs &a, const double *tri, const int *nb, int row, int lane, int k,
                                                double piv_mine, F &&each)
{
    const int nrows = k + 1, myrow = tri_at(lane, 0), site = lane < nrows ? nb[lane] : 0;
    for (int c0 = 0; c0 < a.nb; c0 += VECCHIA_G) {
        double b[VECCHIA_G];
#pragma unroll
        for (int g = 0; g < VECCHIA_G; ++g)
            b[g] = (lane < nrows && c0 + g < a.nb && !(PRED && lane == k)) ? a.B[(size_t)site + (size_t)(c0 + g) * a.ldb] : 0.0;
        vecchia_forward(b, tri, myrow, piv_mine, lane, k, nrows);
        if (lane == k) {
#pragma unroll
            for (int g = 0; g < VECCHIA_G; ++g) {
                if (c0 + g >= a.nb) break;
                if (PRED) a.stoch[row] = 0.0 - b[g];                  // c' K^-1 resid = (C^-1 c)' (C^-1 resid)
                else a.Y[(size_t)row + (size_t)(c0 + g) * a.ldy] = b[g] / piv_mine;
            }
        }
        each(b, c0);
    }
    if (!PRED && lane == k && a.logd) a.logd[row] = log(piv_mine);
}

// The value.  PRED: the last row is a prediction site (cov_rns_pred's rule) and stays out of the factored block -- K = C C' on
// the k neighbours' rows only, the last row then ends as C^-1 c.
template <int MODE, bool PRED>
__global__ void __launch_bounds__(64)
vecchia_value_kernel(VecchiaArgs a)
{
    extern __shared__ double vecchia_lds[];
    const int lane = threadIdx.x, row = blockIdx.x, kb = a.kb;
    const VecchiaValueLds L = vecchia_value_lds(kb, PRED);
    double *par = vecchia_lds + L.par, *par2 = vecchia_lds + L.par2, *tri = vecchia_lds + L.tri;
    int *nb = (int *)(vecchia_lds + L.nb);
    const int k = vecchia_rows(a, row, lane, nb), nrows = k + 1;
    double piv_mine;
    int bad;
    if constexpr (PRED) {
        // the neighbours in both branches' parameters, the prediction site in its own alone
        vecchia_gather_params<64>(par, kb, nb, k, a.aosK, lane);
        vecchia_gather_params<64>(par2, kb, nb, k, a.aosC, lane);
        if (lane < LOCP_FIELDS) { par[lane * kb + k] = 0.0; par2[lane * kb + k] = a.aosP[(size_t)nb[k] * VECCHIA_REC + lane]; }
        __syncthreads();
        vecchia_assemble<MODE, 64, true>(par, par2, tri, kb, nrows, a.gr, a.nu_fixed, lane);
        bad = vecchia_factor(tri, nrows, k, lane, piv_mine);
    } else
        bad = vecchia_open_block<MODE, 64, false>(par, nullptr, tri, kb, nb, nrows, a.aosK, nullptr, a.gr, a.nu_fixed, lane, piv_mine);
    if (bad >= 0) return vecchia_report(a, lane, a.row0 + (int)blockIdx.x + 1);
    __syncthreads();
    vecchia_columns<PRED>(a, tri, nb, row, lane, k, piv_mine, [](const double (&)[VECCHIA_G], int) {});
    if (PRED && lane == k) {
        double q = 0.0;
        for (int j = 0; j < k; ++j) { const double v = tri[tri_at(lane, 0) + j]; q += v * v; }
        a.quad[row] = q;
    }
}

// The coefficients: s = C^-T e_last as one record of kb = m + 1 doubles at rec[row kb ..] -- places t < k hold
// s_t for the neighbour at place t of the device table, places k .. m - 1 hold 0, place m holds s_last.
template <int MODE>
__global__ void __launch_bounds__(64)
vecchia_coef_kernel(VecchiaArgs a)
{
    extern __shared__ double vecchia_lds[];
    const int lane = threadIdx.x, row = a.obs0 + blockIdx.x, kb = a.kb;
    const VecchiaValueLds L = vecchia_value_lds(kb, false);
    double *par = vecchia_lds + L.par, *tri = vecchia_lds + L.tri;
    int *nb = (int *)(vecchia_lds + L.nb);
    const int k = vecchia_rows(a, row, lane, nb), nrows = k + 1;
    double piv_mine;
    if (vecchia_open_block<MODE, 64, false>(par, nullptr, tri, kb, nb, nrows, a.aosK, nullptr, a.gr, a.nu_fixed, lane, piv_mine) >= 0)
        return vecchia_report(a, lane, row + 1);
    __syncthreads();
    double rs[1] = {lane == k ? 1.0 : 0.0}, s[1] = {0.0};
    vecchia_backward<PIV_DIVIDE>(rs, s, tri, piv_mine, lane, k);
    double *rec = a.rec + (size_t)row * kb;
    if (lane < a.m) rec[lane] = lane < k ? s[0] : 0.0;
    if (lane == k) rec[a.m] = s[0];
}

// The gradient: the value's phases, then the block's share of the gradient.  The block's term
// f = nb 2 log d + sum_c y_c^2 has the derivative <W, dC> with W_log = nb s s' and W_quad = -(sum_c y_c^2) s s' - (h s' + s h'),
// s = L^-T e_last, h = L^-T v: two backward solves, the pair partials contracted with the block's weights, per-site sums in
// one fixed order, and one record per observation.
template <int MODE>
__global__ void __launch_bounds__(64)
vecchia_grad_kernel(VecchiaArgs a)
{
    extern __shared__ double vecchia_lds[];
    const int lane = threadIdx.x, row = a.obs0 + blockIdx.x, kb = a.kb;
    const VecchiaGradLds L = vecchia_grad_lds(kb, false);
    double *par = vecchia_lds + L.par, *tri = vecchia_lds + L.tri, *sp = vecchia_lds + L.sp, *sv = vecchia_lds + L.v1;
    double *hv = vecchia_lds + L.v2, *gs = vecchia_lds + L.gs;
    int *nb = (int *)(vecchia_lds + L.nb);
    const int k = vecchia_rows(a, row, lane, nb), nrows = k + 1, npairs = nrows * (nrows - 1) / 2;
    double piv_mine;
    if (vecchia_open_block<MODE, 64, true>(par, sp, tri, kb, nb, nrows, a.aosK, a.aosG, a.gr, a.nu_fixed, lane, piv_mine) >= 0)
        return vecchia_report(a, lane, a.row0 + (int)blockIdx.x + 1);
    __syncthreads();
    // v = sum_c y_c w_c, sum_c y_c^2 and sum_c y_c are formed on the way, the columns ascending
    double vacc = 0.0, ysq = 0.0, ysum = 0.0;
    vecchia_columns<false>(a, tri, nb, row, lane, k, piv_mine, [&](const double (&b)[VECCHIA_G], int c0) {
#pragma unroll
        for (int g = 0; g < VECCHIA_G; ++g) {
            if (c0 + g >= a.nb) break;
            const double w = b[g] / piv_mine;                         // lane k: the whitened value, as stored
            const double y = __shfl(w, k);
            if (lane < k) vacc += y * w;
            ysq += y * y;
            ysum += y;
        }
    });
    double rsh[2] = {lane == k ? 1.0 : 0.0, lane < k ? vacc : 0.0}, sh[2] = {0.0, 0.0};
    vecchia_backward<PIV_DIVIDE>(rsh, sh, tri, piv_mine, lane, k);
    const double s_mine = sh[0], h_mine = sh[1];
    __syncthreads();                       // the factor is dead from here on, tri is the staging of the pair walk
    if (lane < nrows) { sv[lane] = s_mine; hv[lane] = h_mine; }
    const double cn = (double)a.nb;
    auto w_log = [&](double sa, double sb) { return cn * (sa * sb); };
    auto w_quad = [&](double sa, double ha, double sb, double hb) { return 0.0 - ysq * (sa * sb) - (ha * sb + sa * hb); };
    // a row's site sums in registers: the diagonal first -- W_aa (exp(eta_sd), nugget) --, then its pairs pass by pass
    double acc[2 * GFAM];
#pragma unroll
    for (int f = 0; f < 2 * GFAM; ++f) acc[f] = 0.0;
    if (lane < nrows) {
        const double wl = w_log(s_mine, s_mine), wq = w_quad(s_mine, h_mine, s_mine, h_mine);
        const double dsd = sp[3 * kb + lane], dng = par[12 * kb + lane];
        acc[TH_SD_] = wl * dsd; acc[TH_NG_] = wl * dng;
        acc[GFAM + TH_SD_] = wq * dsd; acc[GFAM + TH_NG_] = wq * dng;
    }
    __syncthreads();
    // The pair walk: 64 pairs a pass, one per lane (the order of the assembly), each pair's partials evaluated once and
    // weighted with 2 W_log and 2 W_quad into the staging; then lane = row a adds what the pass holds for its site by
    // vecchia_row_pairs' rule.  A site's sum is therefore formed in one order that is a function of the block alone.
    double *stg = tri;
    double glob_l = 0.0, glob_q = 0.0;
    for (int t0 = 0; t0 < npairs; t0 += 64) {
        const int t = t0 + lane;
        double da[GFAM], db[GFAM], dg = 0.0, w2l = 0.0, w2q = 0.0;
#pragma unroll
        for (int f = 0; f < GFAM; ++f) { da[f] = 0.0; db[f] = 0.0; }
        if (t < npairs) {
            int r, c;
            tri_pair(t, r, c);
            pair_partials<MODE>(par, (size_t)kb, sp, (size_t)kb, a.gr, a.nu_fixed, a.smooth_free, c, r, da, db, dg);
            const double sa = sv[r], ha = hv[r], sb = sv[c], hb = hv[c];
            w2l = 2.0 * w_log(sa, sb);
            w2q = 2.0 * w_quad(sa, ha, sb, hb);
            glob_l += w2l * dg;
            glob_q += w2q * dg;
        }
#pragma unroll
        for (int f = 0; f < GFAM; ++f) {
            stg[(0 * GFAM + f) * 64 + lane] = w2l * da[f];
            stg[(1 * GFAM + f) * 64 + lane] = w2q * da[f];
            stg[(2 * GFAM + f) * 64 + lane] = w2l * db[f];
            stg[(3 * GFAM + f) * 64 + lane] = w2q * db[f];
        }
        __syncthreads();
        if (lane < nrows) {
            auto add = [&](int side, int slot) {
#pragma unroll
                for (int f = 0; f < GFAM; ++f) {
                    acc[f] += stg[(side * GFAM + f) * 64 + slot];
                    acc[GFAM + f] += stg[((side + 1) * GFAM + f) * 64 + slot];
                }
            };
            vecchia_row_pairs(lane, t0, min(t0 + 64, npairs), [&](int slot, int) { add(2, slot); },
                              [&](int slot, int) { add(0, slot); });
        }
        __syncthreads();
    }
    if (lane < nrows) {
#pragma unroll
        for (int f = 0; f < 2 * GFAM; ++f) gs[f * kb + lane] = acc[f];
    }
    glob_l = vecchia_wave_sum(glob_l);
    glob_q = vecchia_wave_sum(glob_q);
    __syncthreads();
    // the record: the site sums contracted with X over the block's rows, ascending
    const int p = a.p, b = blockIdx.x;
    for (int o = lane; o < (2 * GFAM + 1) * p; o += 64) {
        const int q = o / p, kx = o % p;
        const double s = vecchia_dot_x(q < 2 * GFAM ? gs + q * kb : sv, nrows, nb, a.X, a.ldx, kx);
        if (q < 2 * GFAM) a.rec[(size_t)o * a.ldr + b] = s;
        else a.rec[(size_t)(2 * GFAM * p + 2 + kx) * a.ldr + b] = ysum * s;
    }
    if (lane == 0) {
        a.rec[(size_t)(2 * GFAM * p) * a.ldr + b] = glob_l;
        a.rec[(size_t)(2 * GFAM * p + 1) * a.ldr + b] = glob_q;
    }
}

// The information: no right-hand sides (h = 0), s alone.  With q_a = C_a s and g_a = L^-1 q_a the block's share
// is sum_{j < k} g_a[j] g_b[j] + g_a[k] g_b[k] / 2: C_a s per direction from the pair partials, forward solves against the
// factor that is still in LDS, and the Gram of the results as one record.  Directions in groups of a.gd, so that the weights
// fit the LDS.
template <int MODE>
__global__ void __launch_bounds__(64)
vecchia_fisher_kernel(VecchiaArgs a)
{
    extern __shared__ double vecchia_lds[];
    const int lane = threadIdx.x, row = a.obs0 + blockIdx.x, kb = a.kb;
    const VecchiaFisherLds L = vecchia_fisher_lds(kb, a.ndir, a.gd, 1, false);
    double *par = vecchia_lds + L.par, *tri = vecchia_lds + L.tri, *sp = vecchia_lds + L.sp, *sv = vecchia_lds + L.sv;
    double *wts = vecchia_lds + L.wts, *stg = vecchia_lds + L.stg, *gall = vecchia_lds + L.gall;
    int *nb = (int *)(vecchia_lds + L.nb);
    const int k = vecchia_rows(a, row, lane, nb), nrows = k + 1, npairs = nrows * (nrows - 1) / 2;
    double piv_mine;
    if (vecchia_open_block<MODE, 64, true>(par, sp, tri, kb, nb, nrows, a.aosK, a.aosG, a.gr, a.nu_fixed, lane, piv_mine) >= 0)
        return vecchia_report(a, lane, a.row0 + (int)blockIdx.x + 1);
    __syncthreads();
    double rs[1] = {lane == k ? 1.0 : 0.0}, s1[1] = {0.0};
    vecchia_backward<PIV_DIVIDE>(rs, s1, tri, piv_mine, lane, k);
    const double s_mine = s1[0];
    if (lane < nrows) sv[lane] = s_mine;
    const int p = a.p, ndir = a.ndir, b = blockIdx.x, myrow = tri_at(lane, 0);
    for (int d0 = 0; d0 < ndir; d0 += a.gd) {
        const int gd = min(a.gd, ndir - d0);
        __syncthreads();               // sv is written; the previous group's walk has left wts and stg
        vecchia_site_weights<64>(wts, kb, nrows, nb, a.X, a.ldx, p, a.dirs, d0, gd, lane);
        __syncthreads();
        // q_a[row] in registers: the diagonal first, then the row's pairs pass by pass (the gradient walk's order)
        double qa[VECCHIA_FD];
#pragma unroll
        for (int d = 0; d < VECCHIA_FD; ++d) qa[d] = 0.0;
        if (lane < nrows) {
            const double dsd = sp[3 * kb + lane], dng = par[12 * kb + lane];
#pragma unroll
            for (int d = 0; d < VECCHIA_FD; ++d)
                if (d < gd)
                    qa[d] = (dsd * wts[(d * GFAM + TH_SD_) * kb + lane] + dng * wts[(d * GFAM + TH_NG_) * kb + lane]) * s_mine;
        }
        for (int t0 = 0; t0 < npairs; t0 += 64) {
            vecchia_stage_dir_entries<MODE, 64>(stg, wts, par, sp, kb, a.gr, a.nu_fixed, a.smooth_free, a.dirs, p, d0, gd,
                                                t0 + lane, npairs, lane);
            __syncthreads();
            if (lane < nrows) {
                auto add = [&](int slot, int other) {
                    const double so = sv[other];
#pragma unroll
                    for (int d = 0; d < VECCHIA_FD; ++d)
                        if (d < gd) qa[d] += stg[d * 64 + slot] * so;
                };
                vecchia_row_pairs(lane, t0, min(t0 + 64, npairs), add, add);
            }
            __syncthreads();
        }
        // g_a = L^-1 q_a: the likelihood's substitution with q as the right-hand sides; every lane keeps its component
#pragma unroll
        for (int c0 = 0; c0 < VECCHIA_FD; c0 += VECCHIA_G) {
            if (c0 >= gd) break;
            double bb[VECCHIA_G];
#pragma unroll
            for (int g = 0; g < VECCHIA_G; ++g) bb[g] = qa[c0 + g];
            vecchia_forward(bb, tri, myrow, piv_mine, lane, k, nrows);
#pragma unroll
            for (int g = 0; g < VECCHIA_G; ++g)
                if (c0 + g < gd && lane < nrows) gall[(d0 + c0 + g) * kb + lane] = bb[g] / piv_mine;
        }
    }
    // u = sum_rows s[row] X[site(row), .], the rows ascending (the mean gradient's sum)
    if (lane < p) stg[lane] = vecchia_dot_x(sv, nrows, nb, a.X, a.ldx, lane);
    __syncthreads();
    // the record: the lower triangle of the Gram, entry o = a (a + 1) / 2 + b, then that of u u'
    const int ng = ndir * (ndir + 1) / 2;
    for (int o = lane; o < ng; o += 64) {
        int ra, cb;
        tri_pair(o, ra, cb);           // (the strict triangle's numbering of (a + 1, b))
        a.rec[(size_t)o * a.ldr + b] = vecchia_gram_add(0.0, gall + (ra - 1) * kb, gall + cb * kb, k);
    }
    for (int o = lane; o < p * (p + 1) / 2; o += 64) {
        int ra, cb;
        tri_pair(o, ra, cb);
        a.rec[(size_t)(ng + o) * a.ldr + b] = stg[ra - 1] * stg[cb];
    }
}

size_t vecchia_lds_bytes(int m, bool pred) { return vecchia_value_lds(m + 1, pred).bytes; }
size_t vecchia_grad_lds_bytes(int m) { return vecchia_grad_lds(m + 1, false).bytes; }
size_t vecchia_fisher_lds_bytes(int m, int ndir, int gd) { return vecchia_fisher_lds(m + 1, ndir, gd, 1, false).bytes; }

int vecchia_fisher_group(int m, int ndir)
{
    int gd = VECCHIA_FD;
    while (gd > VECCHIA_G && vecchia_fisher_lds_bytes(m, ndir, gd) > VECCHIA_FISHER_LDS_MAX) gd /= 2;
    return std::min(gd, std::max(ndir, 1));
}

// m <= 63: the value's and the coefficients' LDS is at most 31 KB, the gradient's at most 32 KB -- no attribute needed
void launch_vecchia_blocks(int mode, bool pred, const VecchiaArgs &a, hipStream_t s)
{
    if (a.rows <= 0) return;
    vecchia_with_mode(mode, [&](auto M) {
        constexpr int MODE = decltype(M)::value;
        vecchia_launch_kernel(pred ? vecchia_value_kernel<MODE, true> : vecchia_value_kernel<MODE, false>, a, a.rows, 64,
                              vecchia_lds_bytes(a.m, pred), s);
    });
}

void launch_vecchia_coefs(int mode, const VecchiaArgs &a, hipStream_t s)
{
    if (a.rows <= 0) return;
    vecchia_with_mode(mode, [&](auto M) {
        vecchia_launch_kernel(vecchia_coef_kernel<decltype(M)::value>, a, a.rows, 64, vecchia_lds_bytes(a.m, false), s);
    });
}

void launch_vecchia_grad_blocks(int mode, const VecchiaArgs &a, hipStream_t s)
{
    if (a.rows <= 0) return;
    vecchia_with_mode(mode, [&](auto M) {
        vecchia_launch_kernel(vecchia_grad_kernel<decltype(M)::value>, a, a.rows, 64, vecchia_grad_lds_bytes(a.m), s);
    });
}

void launch_vecchia_fisher_blocks(int mode, const VecchiaArgs &a, hipStream_t s)
{
    if (a.rows <= 0) return;
    vecchia_with_mode(mode, [&](auto M) {
        static std::atomic<unsigned long long> attr_done{0};           // (one per instantiation)
        vecchia_launch_kernel(vecchia_fisher_kernel<decltype(M)::value>, a, a.rows, 64,
                              vecchia_fisher_lds_bytes(a.m, a.ndir, a.gd), s, &attr_done, VECCHIA_FISHER_LDS_MAX);
    });
}

// ---------------------------------------------------------------------------
// Totals: column q of v (n x ncol, leading dimension ldv) summed -- squared first from column 1 on -- in segments of
// VECCHIA_SUM_SEG elements (thread t takes the elements t, t + 256, .. of its segment in that order, then a binary tree over
// the 256 threads), and the segments' sums by the same shape in one workgroup per column.  The shape is a function of n alone.
__device__ __forceinline__ double vecchia_tree(double acc, double *red)
{
    const int t = threadIdx.x;
    red[t] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    return red[0];
}

__global__ void __launch_bounds__(256)
vecchia_sum_kernel(const double *v, size_t ldv, int n, double *part, int squares, int seg0, int nseg)
{
    __shared__ double red[256];
    const int seg = blockIdx.x, q = blockIdx.y, t = threadIdx.x;
    const double *col = v + (size_t)q * ldv;
    double acc = 0.0;
    for (int s = 0; s < VECCHIA_SUM_SEG / 256; ++s) {
        const size_t i = (size_t)seg * VECCHIA_SUM_SEG + (size_t)s * 256 + t;
        if (i < (size_t)n) { const double x = col[i]; acc += (squares && q > 0) ? x * x : x; }
    }
    const double total = vecchia_tree(acc, red);
    if (t == 0) part[(size_t)q * nseg + seg0 + seg] = total;
}

__global__ void __launch_bounds__(256)
vecchia_sum_final_kernel(const double *part, int nseg, double *out)
{
    __shared__ double red[256];
    const int q = blockIdx.x, t = threadIdx.x;
    double acc = 0.0;
    for (int i = t; i < nseg; i += 256) acc += part[(size_t)q * nseg + i];
    const double total = vecchia_tree(acc, red);
    if (t == 0) out[q] = total;
}

size_t vecchia_sum_scratch_doubles(int n, int ncol) { return (size_t)((n + VECCHIA_SUM_SEG - 1) / VECCHIA_SUM_SEG) * (size_t)ncol; }

void launch_vecchia_sums(const double *v, size_t ldv, int n, int ncol, double *part, double *out, hipStream_t s)
{
    const int nseg = (n + VECCHIA_SUM_SEG - 1) / VECCHIA_SUM_SEG;
    hipLaunchKernelGGL(vecchia_sum_kernel, dim3(nseg, ncol), dim3(256), 0, s, v, ldv, n, part, 1, 0, nseg);
    hipLaunchKernelGGL(vecchia_sum_final_kernel, dim3(ncol), dim3(256), 0, s, part, nseg, out);
}

void launch_vecchia_chunk_sums(const double *v, size_t ldv, int rows, int ncol, double *part, int seg0, int nseg, hipStream_t s)
{
    if (rows <= 0) return;
    const int segs = (rows + VECCHIA_SUM_SEG - 1) / VECCHIA_SUM_SEG;
    hipLaunchKernelGGL(vecchia_sum_kernel, dim3(segs, ncol), dim3(256), 0, s, v, ldv, rows, part, 0, seg0, nseg);
}

void launch_vecchia_final_sums(const double *part, int nseg, int ncol, double *out, hipStream_t s)
{
    hipLaunchKernelGGL(vecchia_sum_final_kernel, dim3(ncol), dim3(256), 0, s, part, nseg, out);
}

}  // namespace cocons
