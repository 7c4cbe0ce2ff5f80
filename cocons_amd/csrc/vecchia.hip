// vecchia.hip -- the Vecchia approximation's per-observation blocks (gfx950).
//
//   vecchia_aos_kernel    : loc_params_kernel's SoA (LOCP_FIELDS x stride) transposed to one 128-byte record of 16 doubles
//                           per location, so that gathering a neighbour's parameters costs one cache line instead of 13.
//   vecchia_resid_kernel  : z[:, col0 ..] - X mean in rhs_rows_kernel's arithmetic, one column per realisation.
//   vecchia_block_kernel  : ONE WAVEFRONT per observation (a workgroup of 64 lanes): the parameters of the observation and
//                           of its k <= 63 neighbours gathered into LDS, the (k + 1) x (k + 1) covariance block assembled with
//                           pair_value_idx -- the dense assembly's arithmetic -- into a packed lower triangle in LDS, factored
//                           there column by column with lane = row, and the right-hand sides carried through the forward
//                           substitution in registers.  PRED: the last row is a prediction site (cov_rns_pred's rule) and stays
//                           out of the factored block.
//                           GRAD: the same gather, pair loop, factorisation and substitution, then the block's
//                           share of the gradient: two backward solves, the pair partials contracted with the block's weights,
//                           per-site sums in one fixed order, and one record per observation.
//                           FISH: the same gather, pair loop, factorisation and backward solve for s, then the
//                           block's share of the expected information: C_a s per direction from the pair partials, forward
//                           solves against the factor that is still in LDS, and the Gram of the results as one record.
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
#include "matern_device.hpp"
#include "grad_pair.hpp"
#include "vecchia_tri.hpp"

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
// Dynamic LDS, sized by kb = m + 1 rows (vecchia_lds_bytes):
//   par   LOCP_FIELDS x kb   the block's parameters as an SoA of stride kb -- what pair_value_idx reads;
//   par2  LOCP_FIELDS x kb   PRED only: the same rows in the prediction branch's parameters, the prediction site last;
//   tri   kb (kb + 1) / 2    the block, then its factor (the pivots stay in registers: lane r keeps C(r, r));
//   nb    kb ints            the rows' locations.
// GRAD (vecchia_grad_lds_bytes) keeps tri at VECCHIA_STG doubles or more -- once s and h are known the factor is dead and the
// pair walk stages its contributions there -- and puts VECCHIA_GX x kb doubles between tri and nb:
//   sp    GSITE_FIELDS x kb  the rows' site derivatives (grad_site_kernel's fields) as an SoA of stride kb;
//   sv, hv  kb each          s = L^-T e_last and h = L^-T v;
//   gs    2 GFAM x kb        the rows' site sums: the log-determinant's share per family, then the quadratic forms'.
constexpr int VECCHIA_STG = 4 * GFAM * 64;              // a pass of 64 pairs: (ii side, jj side) x (two shares) x GFAM
constexpr int VECCHIA_GX = GSITE_FIELDS + 2 + 2 * GFAM;
// FISH (vecchia_fisher_lds_bytes) keeps the factor in tri and puts behind sp, sv, hv, for groups of gd <= VECCHIA_FD directions:
//   wts   gd x GFAM x kb     the rows' site weights w_a[f][row] of the group's directions;
//   stg   gd x 64            a pass of 64 pairs: the entry of C_a per direction (then, once, the p sums u of the mean block);
//   gall  ndir x kb          g_a = L^-1 (C_a s) of every direction, what the Gram is formed of.
//   (VECCHIA_FX = GSITE_FIELDS + 2 and vecchia_forward stand in vecchia_tri.hpp: the grouped launch uses them too)

__device__ __forceinline__ double vecchia_wave_sum(double v)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int MODE, bool PRED, bool GRAD, bool FISH = false>
__global__ void __launch_bounds__(64)
vecchia_block_kernel(VecchiaArgs a)
{
    static_assert(!(PRED && (GRAD || FISH)) && !(GRAD && FISH), "the gradient and the information are the likelihood launch's");
    constexpr bool DER = GRAD || FISH;             // the launches that gather the site derivatives and solve for s
    extern __shared__ double vecchia_lds[];
    const int lane = threadIdx.x, row = (DER ? a.obs0 : 0) + blockIdx.x, kb = a.kb;
    double *par = vecchia_lds;
    double *par2 = par + (PRED ? LOCP_FIELDS * kb : 0);
    double *tri = par2 + LOCP_FIELDS * kb;
    const int ntri = kb * (kb + 1) / 2;
    double *gx = tri + ((GRAD && ntri < VECCHIA_STG) ? VECCHIA_STG : ntri);
    int *nb = (int *)(gx + (GRAD ? VECCHIA_GX * kb : FISH ? VECCHIA_FX * kb + a.gd * (GFAM * kb + 64) + a.ndir * kb : 0));

    // the row's neighbours: ascending, the free places (-1) behind them
    const int mine = lane < a.m ? a.nbr[(size_t)row * a.m + lane] : -1;
    const int k = __popcll(__ballot(mine >= 0));
    const int nrows = k + 1;                   // the neighbours, then the observation (PRED: the prediction site)
    if (lane < k) nb[lane] = mine;
    if (lane == k) nb[lane] = row;
    __syncthreads();
    for (int e = lane; e < nrows * VECCHIA_REC; e += 64) {
        const int r = e / VECCHIA_REC, f = e % VECCHIA_REC;
        if (f >= LOCP_FIELDS) continue;
        const size_t at = (size_t)nb[r] * VECCHIA_REC + f;
        if (!PRED) par[f * kb + r] = a.aosK[at];
        else if (r < k) { par[f * kb + r] = a.aosK[at]; par2[f * kb + r] = a.aosC[at]; }
        else { par[f * kb + r] = 0.0; par2[f * kb + r] = a.aosP[at]; }
    }
    if (DER)
        for (int e = lane; e < nrows * VECCHIA_GSITE_REC; e += 64) {
            const int r = e / VECCHIA_GSITE_REC, f = e % VECCHIA_GSITE_REC;
            gx[f * kb + r] = a.aosG[(size_t)nb[r] * VECCHIA_GSITE_REC + f];
        }
    __syncthreads();
    // the block: pair t = r (r - 1) / 2 + c is (r, c), r > c, evaluated with the EARLIER row on the `ii` side (the reference's
    // orientation, which the u <= eps rule sees); PRED, last row: the prediction site on the `ii` side, exact coordinate
    // matches give its own diagonal value (cov_rns_pred)
    const int npairs = nrows * (nrows - 1) / 2;
    for (int t = lane; t < npairs; t += 64) {
        int r, c;
        tri_pair(t, r, c);
        double v;
        if (PRED && r == k) v = pair_value_idx<MODE_GEOM>(par2, (size_t)kb, r, par2, (size_t)kb, c, a.gr, 0.0, true);
        else v = pair_value_idx<MODE>(par, (size_t)kb, c, par, (size_t)kb, r, a.gr, a.nu_fixed, false);
        tri[tri_at(r, c)] = v;
    }
    if (lane < nrows) tri[tri_at(lane, lane)] = par[11 * kb + lane];
    // K = C C', right-looking, one column per step; PRED: the k neighbours' block only -- the last row then ends as C^-1 c
    const int nf = PRED ? k : nrows;
    const int myrow = tri_at(lane, 0);
    double piv_mine = 1.0;
    bool bad = false;
    for (int j = 0; j < nf; ++j) {
        __syncthreads();
        const double d = tri[tri_at(j, j)];
        if (!(d > 0.0) || !isfinite(d)) { bad = true; break; }       // (the same in every lane)
        const double piv = sqrt(d);
        if (lane == j) piv_mine = piv;
        double lrj = 0.0;
        if (lane > j && lane < nrows) { lrj = tri[myrow + j] / piv; tri[myrow + j] = lrj; }
        __syncthreads();
        if (lane > j && lane < nrows)
            for (int c = j + 1; c <= lane; ++c) tri[myrow + c] -= lrj * tri[tri_at(c, j)];
    }
    if (bad) {
        if (lane == 0) atomicMin(a.fail, a.row0 + (int)blockIdx.x + 1);
        return;
    }
    __syncthreads();
    // forward substitution over the neighbours' rows, VECCHIA_G right-hand sides at a time; lane k ends with
    // b_k - sum_j C(k, j) y_j, j ascending.  GRAD: every lane j ends with the numerator of w_c[j] (the steps from j on
    // leave it alone), so v = sum_c y_c w_c, sum_c y_c^2 and sum_c y_c are formed on the way, the columns ascending
    const int site = lane < nrows ? nb[lane] : 0;
    double vacc = 0.0, ysq = 0.0, ysum = 0.0;
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
        if (GRAD) {
#pragma unroll
            for (int g = 0; g < VECCHIA_G; ++g) {
                if (c0 + g >= a.nb) break;
                const double w = b[g] / piv_mine;                     // lane k: the whitened value, as stored above
                const double y = __shfl(w, k);
                if (lane < k) vacc += y * w;
                ysq += y * y;
                ysum += y;
            }
        }
    }
    if (lane == k) {
        if (PRED) {
            double q = 0.0;
            for (int j = 0; j < k; ++j) { const double v = tri[myrow + j]; q += v * v; }
            a.quad[row] = q;
        } else if (a.logd) a.logd[row] = log(piv_mine);
    }
    // The block's term f = nb 2 log d + sum_c y_c^2 has the derivative <W, dC> with W_log = nb s s' and
    // W_quad = -(sum_c y_c^2) s s' - (h s' + s h'), s = L^-T e_last, h = L^-T v.  FISH has no right-hand
    // sides (h = 0) and uses s alone.
    [[maybe_unused]] double *sp = gx, *sv = sp + GSITE_FIELDS * kb, *hv = sv + kb;
    [[maybe_unused]] double s_mine = 0.0, h_mine = 0.0;
    if constexpr (DER) {
        // the two backward solves, one column of L' (a row of the packed factor) per step; lane j ends with component j
        double rs = lane == k ? 1.0 : 0.0, rh = lane < k ? vacc : 0.0;
        for (int j = k; j >= 0; --j) {
            const double xs = __shfl(rs / piv_mine, j), xh = __shfl(rh / piv_mine, j);
            if (lane == j) { s_mine = xs; h_mine = xh; }
            if (lane < j) {
                const double l = tri[tri_at(j, 0) + lane];
                rs -= l * xs;
                rh -= l * xh;
            }
        }
        __syncthreads();                   // GRAD: the factor is dead from here on, tri is the staging of the pair walk
        if (lane < nrows) { sv[lane] = s_mine; hv[lane] = h_mine; }
    }
    if constexpr (GRAD) {
        double *gs = hv + kb;
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
        // The pair walk: 64 pairs a pass, one per lane (the order of the assembly above), each pair's partials evaluated once
        // and weighted with 2 W_log and 2 W_quad into the staging; then lane = row a adds what the pass holds for its site --
        // its pairs (a, c), c < a ascending (the jj side), then its pairs (r, a), r > a ascending (the ii side).  A site's sum
        // is therefore formed in one order that is a function of the block alone.
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
                const int tend = min(t0 + 64, npairs), mine0 = lane * (lane - 1) / 2;
                for (int u = max(t0, mine0); u < min(tend, mine0 + lane); ++u) {
#pragma unroll
                    for (int f = 0; f < GFAM; ++f) {
                        acc[f] += stg[(2 * GFAM + f) * 64 + (u - t0)];
                        acc[GFAM + f] += stg[(3 * GFAM + f) * 64 + (u - t0)];
                    }
                }
                int r_lo, r_hi, c_;
                tri_pair(t0, r_lo, c_);
                tri_pair(tend - 1, r_hi, c_);
                for (int r = max(r_lo, lane + 1); r <= r_hi; ++r) {
                    const int u = r * (r - 1) / 2 + lane;
                    if (u < t0 || u >= tend) continue;
#pragma unroll
                    for (int f = 0; f < GFAM; ++f) {
                        acc[f] += stg[(0 * GFAM + f) * 64 + (u - t0)];
                        acc[GFAM + f] += stg[(1 * GFAM + f) * 64 + (u - t0)];
                    }
                }
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
            const double *g = q < 2 * GFAM ? gs + q * kb : sv;
            double s = 0.0;
            for (int rr = 0; rr < nrows; ++rr) s += g[rr] * a.X[(size_t)nb[rr] + (size_t)kx * a.ldx];
            if (q < 2 * GFAM) a.rec[(size_t)o * a.ldr + b] = s;
            else a.rec[(size_t)(2 * GFAM * p + 2 + kx) * a.ldr + b] = ysum * s;
        }
        if (lane == 0) {
            a.rec[(size_t)(2 * GFAM * p) * a.ldr + b] = glob_l;
            a.rec[(size_t)(2 * GFAM * p + 1) * a.ldr + b] = glob_q;
        }
    }
    if constexpr (FISH) {
        // The block's share of the expected information: with q_a = C_a s and g_a = L^-1 q_a,
        // sum_{j < k} g_a[j] g_b[j] + g_a[k] g_b[k] / 2.  Directions in groups of a.gd, so that the weights fit the LDS.
        const int p = a.p, ndir = a.ndir, b = blockIdx.x;
        double *wts = hv + kb, *stg = wts + a.gd * GFAM * kb, *gall = stg + a.gd * 64;
        for (int d0 = 0; d0 < ndir; d0 += a.gd) {
            const int gd = min(a.gd, ndir - d0);
            __syncthreads();               // sv is written; the previous group's walk has left wts and stg
            // the site weights of the group's directions: w_a[f][row] = c_f sum_k X[site(row), k] dirs[a][f, k], k ascending;
            // scale: c = 2 over k >= 1 (k = 0 is the global range)
            for (int e = lane; e < gd * GFAM * nrows; e += 64) {
                const int rr = e % nrows, f = (e / nrows) % GFAM, d = e / (nrows * GFAM);
                const double *v = a.dirs + ((size_t)(d0 + d) * GFAM + f) * p;
                double w = 0.0;
                for (int kx = (f == TH_SCALE_ ? 1 : 0); kx < p; ++kx) w += a.X[(size_t)nb[rr] + (size_t)kx * a.ldx] * v[kx];
                wts[(d * GFAM + f) * kb + rr] = f == TH_SCALE_ ? 2.0 * w : w;
            }
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
                const int t = t0 + lane;
                double da[GFAM], db[GFAM], dg = 0.0;
                int r = 0, c = 0;
#pragma unroll
                for (int f = 0; f < GFAM; ++f) { da[f] = 0.0; db[f] = 0.0; }
                if (t < npairs) {
                    tri_pair(t, r, c);
                    pair_partials<MODE>(par, (size_t)kb, sp, (size_t)kb, a.gr, a.nu_fixed, a.smooth_free, c, r, da, db, dg);
                }
                for (int d = 0; d < gd; ++d) {
                    double e = 0.0;
                    if (t < npairs) {
                        const double *w = wts + d * GFAM * kb;
                        e = dg * a.dirs[((size_t)(d0 + d) * GFAM + TH_SCALE_) * p];
#pragma unroll
                        for (int f = 0; f < GFAM; ++f) {
                            e += da[f] * w[f * kb + c];
                            e += db[f] * w[f * kb + r];
                        }
                    }
                    stg[d * 64 + lane] = e;
                }
                __syncthreads();
                if (lane < nrows) {
                    const int tend = min(t0 + 64, npairs), mine0 = lane * (lane - 1) / 2;
                    for (int u = max(t0, mine0); u < min(tend, mine0 + lane); ++u) {
                        const double so = sv[u - mine0];
#pragma unroll
                        for (int d = 0; d < VECCHIA_FD; ++d)
                            if (d < gd) qa[d] += stg[d * 64 + (u - t0)] * so;
                    }
                    int r_lo, r_hi, c_;
                    tri_pair(t0, r_lo, c_);
                    tri_pair(tend - 1, r_hi, c_);
                    for (int rr = max(r_lo, lane + 1); rr <= r_hi; ++rr) {
                        const int u = rr * (rr - 1) / 2 + lane;
                        if (u < t0 || u >= tend) continue;
                        const double so = sv[rr];
#pragma unroll
                        for (int d = 0; d < VECCHIA_FD; ++d)
                            if (d < gd) qa[d] += stg[d * 64 + (u - t0)] * so;
                    }
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
        if (lane < p) {
            double s = 0.0;
            for (int rr = 0; rr < nrows; ++rr) s += sv[rr] * a.X[(size_t)nb[rr] + (size_t)lane * a.ldx];
            stg[lane] = s;
        }
        __syncthreads();
        // the record: the lower triangle of the Gram, entry o = a (a + 1) / 2 + b, then that of u u'
        const int ng = ndir * (ndir + 1) / 2;
        for (int o = lane; o < ng; o += 64) {
            int ra, cb;
            tri_pair(o, ra, cb);           // (the strict triangle's numbering of (a + 1, b))
            const double *ga = gall + (ra - 1) * kb, *gb = gall + cb * kb;
            double s = 0.0;
            for (int j = 0; j < k; ++j) s += ga[j] * gb[j];
            s += 0.5 * (ga[k] * gb[k]);
            a.rec[(size_t)o * a.ldr + b] = s;
        }
        for (int o = lane; o < p * (p + 1) / 2; o += 64) {
            int ra, cb;
            tri_pair(o, ra, cb);
            a.rec[(size_t)(ng + o) * a.ldr + b] = stg[ra - 1] * stg[cb];
        }
    }
}

size_t vecchia_lds_bytes(int m, bool pred)
{
    const size_t kb = (size_t)m + 1;
    return ((pred ? 2 : 1) * LOCP_FIELDS * kb + kb * (kb + 1) / 2) * sizeof(double) + kb * sizeof(int);
}

template <bool PRED> static void vecchia_launch(int mode, const VecchiaArgs &a, hipStream_t s)
{
    const size_t shm = vecchia_lds_bytes(a.m, PRED);          // m <= 63: at most 31 KB, no attribute needed
    const dim3 grid((unsigned)a.rows), block(64);
    switch (mode) {
    case MODE_HALF: hipLaunchKernelGGL((vecchia_block_kernel<MODE_HALF, PRED, false>), grid, block, shm, s, a); break;
    case MODE_THREEHALF: hipLaunchKernelGGL((vecchia_block_kernel<MODE_THREEHALF, PRED, false>), grid, block, shm, s, a); break;
    case MODE_FIVEHALF: hipLaunchKernelGGL((vecchia_block_kernel<MODE_FIVEHALF, PRED, false>), grid, block, shm, s, a); break;
    default: hipLaunchKernelGGL((vecchia_block_kernel<MODE_GEOM, PRED, false>), grid, block, shm, s, a); break;
    }
}

size_t vecchia_grad_lds_bytes(int m)
{
    const size_t kb = (size_t)m + 1, ntri = kb * (kb + 1) / 2;
    return (LOCP_FIELDS * kb + (ntri < (size_t)VECCHIA_STG ? (size_t)VECCHIA_STG : ntri) + VECCHIA_GX * kb) * sizeof(double) +
           kb * sizeof(int);
}

void launch_vecchia_grad_blocks(int mode, const VecchiaArgs &a, hipStream_t s)
{
    if (a.rows <= 0) return;
    const size_t shm = vecchia_grad_lds_bytes(a.m);           // m <= 63: at most 32 KB, no attribute needed
    const dim3 grid((unsigned)a.rows), block(64);
    switch (mode) {
    case MODE_HALF: hipLaunchKernelGGL((vecchia_block_kernel<MODE_HALF, false, true>), grid, block, shm, s, a); break;
    case MODE_THREEHALF: hipLaunchKernelGGL((vecchia_block_kernel<MODE_THREEHALF, false, true>), grid, block, shm, s, a); break;
    case MODE_FIVEHALF: hipLaunchKernelGGL((vecchia_block_kernel<MODE_FIVEHALF, false, true>), grid, block, shm, s, a); break;
    default: hipLaunchKernelGGL((vecchia_block_kernel<MODE_GEOM, false, true>), grid, block, shm, s, a); break;
    }
}

size_t vecchia_fisher_lds_bytes(int m, int ndir, int gd)
{
    const size_t kb = (size_t)m + 1;
    return (LOCP_FIELDS * kb + kb * (kb + 1) / 2 + VECCHIA_FX * kb + (size_t)gd * (GFAM * kb + 64) + (size_t)ndir * kb) *
               sizeof(double) + kb * sizeof(int);
}

int vecchia_fisher_group(int m, int ndir)
{
    int gd = VECCHIA_FD;
    while (gd > VECCHIA_G && vecchia_fisher_lds_bytes(m, ndir, gd) > VECCHIA_FISHER_LDS_MAX) gd /= 2;
    return std::min(gd, std::max(ndir, 1));
}

template <int MODE> static void vecchia_fisher_launch(const VecchiaArgs &a, size_t shm, hipStream_t s)
{
    static std::atomic<unsigned long long> attr_done{0};
    if (shm > 64 * 1024)
        set_dynamic_lds_once((const void *)vecchia_block_kernel<MODE, false, false, true>, VECCHIA_FISHER_LDS_MAX, attr_done);
    hipLaunchKernelGGL((vecchia_block_kernel<MODE, false, false, true>), dim3((unsigned)a.rows), dim3(64), shm, s, a);
}

void launch_vecchia_fisher_blocks(int mode, const VecchiaArgs &a, hipStream_t s)
{
    if (a.rows <= 0) return;
    const size_t shm = vecchia_fisher_lds_bytes(a.m, a.ndir, a.gd);
    switch (mode) {
    case MODE_HALF: vecchia_fisher_launch<MODE_HALF>(a, shm, s); break;
    case MODE_THREEHALF: vecchia_fisher_launch<MODE_THREEHALF>(a, shm, s); break;
    case MODE_FIVEHALF: vecchia_fisher_launch<MODE_FIVEHALF>(a, shm, s); break;
    default: vecchia_fisher_launch<MODE_GEOM>(a, shm, s); break;
    }
}

void launch_vecchia_blocks(int mode, bool pred, const VecchiaArgs &a, hipStream_t s)
{
    if (a.rows <= 0) return;
    if (pred) vecchia_launch<true>(mode, a, s);
    else vecchia_launch<false>(mode, a, s);
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
