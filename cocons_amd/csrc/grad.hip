// grad.hip -- analytic gradient of the dense -2 log-likelihood (cocons_neg2loglik_grad_dense), gfx950.
//
//   grad_fill_kernel     : unit rows under the matrix (the bordered factorisation solves L^-T beside the residuals), zeros
//   grad_sigma_r_kernel  : A = Sigma^-1 R = L^-T (L^-1 R) from the solved rows
//   grad_gls_kernel / grad_lowrank_kernel : Profile / REML: beta and chol(Xb' Sigma^-1 Xb) from the border's Gram matrix, then
//                          the low-rank block [Sigma^-1 (Z - Xb beta) | sqrt(r) V chol(W)^-T] the pair kernel takes as its A
//   launch_grad_syrk     : -Sigma^-1 = -L^-T L^-1 (lower tiles) by the trailing-update kernel, 256 columns of L^-T at a time
//   grad_site_kernel     : per-site derivative factors beside loc_params_kernel's SoA (tilt, smoothness, std.dev)
//   grad_pair_kernel     : W = r Sigma^-1 - A A' contracted with dSigma/d(site predictors) over the 64 x 64 lower tiles
//   grad_reduce_kernel / grad_xt_kernel : fixed-order sums per site, then X' g and the mean gradient
//
//   fisher_*_kernel, dsigma_dirs_kernel : the expected information (cocons_fisher_dense): direction matrices from the same pair
//                          partials, Sigma^-1 in full, the traces of the products
//
//   taper_grad_*_kernel : the taper fit's contraction over its CSR pattern (cocons_neg2loglik_grad_taper; selinv.hip gives S^-1)
//
// Every sum has a fixed order (no floating-point atomics): two calls give bit-identical gradients.
// Compile with -ffp-contract=off (matern_device.hpp).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "matern_device.hpp"
#include "grad_pair.hpp"           // matern_pair, matern_dnu, pair_partials (shared with vecchia.hip)

namespace cocons {

constexpr int GTS = 64;            // pair tile edge (as pair_sym_kernel)

// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
matern_grad_points_kernel(int n, const double *nu, const double *u, double *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = nu[i], x = u[i];
    double M, Mu, Mn;
    if (x >= 706.0) { M = matern_bessel(v, x); Mu = 0.0; Mn = 0.0; }      // the reference's stand-in: derivatives round to 0
    else { matern_pair(v, x, M, Mu); Mn = matern_dnu(v, x); }
    out[i] = M;
    out[i + n] = Mu;
    out[i + 2 * (size_t)n] = Mn;
}

void launch_matern_grad_points(int n, const double *nu, const double *u, double *out, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(matern_grad_points_kernel, dim3((n + 63) / 64), dim3(64), 0, s, n, nu, u, out);
}

// ---------------------------------------------------------------------------
// rows [row0, row0 + nrows) x columns [0, ncols) of A: 1 where row - row_id == column, else 0 (row_id < 0: all zero).
// Lanes along the rows: every wave store is 512 contiguous bytes.
__global__ void __launch_bounds__(256)
grad_fill_kernel(double *A, size_t lda, int row0, int nrows, int ncols, int row_id)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    const int c1 = min(ncols, (int)(blockIdx.y + 1) * 64);
    for (int c = blockIdx.y * 64; c < c1; ++c)
        A[(size_t)(row0 + i) + (size_t)c * lda] = (row_id >= 0 && row0 + i - row_id == c) ? 1.0 : 0.0;
}

void launch_grad_fill(double *A, size_t lda, int row0, int nrows, int ncols, int row_id, hipStream_t s)
{
    if (nrows <= 0 || ncols <= 0) return;
    hipLaunchKernelGGL(grad_fill_kernel, dim3((nrows + 255) / 256, (ncols + 63) / 64), dim3(256), 0, s, A, lda, row0, nrows,
                       ncols, row_id);
}

// AR[i + c npad] = sum_k B(i, k) w_c(k): B = L^-T in rows brow0.., w_c = L^-1 r_c in row wrow0 + c.  Stage 1: the 64 rows
// of a block over one of GRAD_KSPLIT column chunks (B is upper triangular: chunks left of the rows are zero and skipped)
// into part; stage 2: the chunks summed in order.
constexpr int GRAD_KSPLIT = 16;
__global__ void __launch_bounds__(64)
grad_sigma_r_kernel(const double *A, size_t lda, int npad, int wrow0, int nr, int brow0, double *part)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int chunk = (npad + GRAD_KSPLIT - 1) / GRAD_KSPLIT;
    const int k0 = blockIdx.y * chunk, k1 = min(npad, k0 + chunk);
    for (int c = 0; c < nr; ++c) {
        double s = 0.0;
        for (int k = max(k0, (int)blockIdx.x * 64); k < k1; ++k)
            s = fma(A[(size_t)(brow0 + i) + (size_t)k * lda], A[(size_t)(wrow0 + c) + (size_t)k * lda], s);
        part[((size_t)blockIdx.y * nr + c) * npad + i] = s;
    }
}

__global__ void __launch_bounds__(256)
grad_sigma_r_sum_kernel(const double *part, int npad, int nr, double *AR)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    for (int c = 0; c < nr; ++c) {
        double s = 0.0;
        for (int q = 0; q < GRAD_KSPLIT; ++q) s += part[((size_t)q * nr + c) * npad + i];
        AR[(size_t)i + (size_t)c * npad] = s;
    }
}

size_t grad_sigma_r_scratch_doubles(int npad, int nr) { return (size_t)GRAD_KSPLIT * nr * npad; }

void launch_grad_sigma_r(const double *A, size_t lda, int npad, int wrow0, int nr, int brow0, double *part, double *AR,
                         hipStream_t s)
{
    hipLaunchKernelGGL(grad_sigma_r_kernel, dim3(npad / 64, GRAD_KSPLIT), dim3(64), 0, s, A, lda, npad, wrow0, nr, brow0, part);
    hipLaunchKernelGGL(grad_sigma_r_sum_kernel, dim3((npad + 255) / 256), dim3(256), 0, s, part, npad, nr, AR);
}

// ---------------------------------------------------------------------------
// Profile / REML: the generalised-least-squares step between Sigma^-1 [Z | Xb] and the pair contraction.
// G = fin + 1 is the (r + q)^2 Gram matrix of the border [Z' ; Xb'] (row-major): W = G[r.., r..] = Xb' Sigma^-1 Xb,
// g_k = G[k, r..] = Xb' Sigma^-1 z_k.  One workgroup; the Cholesky factor and the two triangular solves run in the order of
// the host's solve of the same matrix (profile_tail), so a pivot fails here exactly when it fails there.
// gls[0] = 1 (W positive definite) or 0, gls[2 ..] = chol(W) (q x q column-major, lower), then beta (q x r, column k = beta_k).
constexpr int GLS_L0 = 2;
size_t grad_gls_doubles(int r, int q) { return (size_t)GLS_L0 + (size_t)q * q + (size_t)q * r; }

__global__ void __launch_bounds__(64)
grad_gls_kernel(const double *fin, int r, int q, double *gls)
{
    __shared__ double W[COCONS_P_MAX * COCONS_P_MAX];
    __shared__ int ok;
    const int t = threadIdx.x, nb = r + q;
    const double *G = fin + 1;
    for (int e = t; e < q * q; e += 64) W[e] = G[(size_t)(r + e % q) * nb + (r + e / q)];
    if (t == 0) ok = 1;
    __syncthreads();
    for (int j = 0; j < q; ++j) {
        if (t == 0) {
            double d = W[j + j * q];
            for (int k = 0; k < j; ++k) d -= W[j + k * q] * W[j + k * q];
            if (!(d > 0)) ok = 0;
            else W[j + j * q] = sqrt(d);
        }
        __syncthreads();
        if (!ok) break;
        if (t > j && t < q) {
            double s = W[t + j * q];
            for (int k = 0; k < j; ++k) s -= W[t + k * q] * W[j + k * q];
            W[t + j * q] = s / W[j + j * q];
        }
        __syncthreads();
    }
    double *L = gls + GLS_L0, *beta = L + (size_t)q * q;
    for (int e = t; e < q * q; e += 64) L[e] = (ok && e % q >= e / q) ? W[e] : 0.0;
    for (int c = t; c < r; c += 64) {
        double *b = beta + (size_t)c * q;
        for (int i = 0; i < q; ++i) b[i] = ok ? G[(size_t)c * nb + (r + i)] : 0.0;
        if (!ok) continue;
        for (int i = 0; i < q; ++i) {
            double s = b[i];
            for (int k = 0; k < i; ++k) s -= W[i + k * q] * b[k];
            b[i] = s / W[i + i * q];
        }
        for (int i = q - 1; i >= 0; --i) {
            double s = b[i];
            for (int k = i + 1; k < q; ++k) s -= W[k + i * q] * b[k];
            b[i] = s / W[i + i * q];
        }
    }
    if (t == 0) { gls[0] = ok ? 1.0 : 0.0; gls[1] = 0.0; }
}

// LR(i, k) = A_z(i, k) - sum_a V(i, a) beta(a, k), k < r; with reml LR(i, r + a) = sqrt(r) c_a, L c = V(i, .)' (forward
// substitution per site: C = V L^-T).  One thread per site, fixed order.
__global__ void __launch_bounds__(256)
grad_lowrank_kernel(const double *SX, int npad, int r, int q, int reml, const double *gls, double *LR)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    const bool ok = gls[0] != 0.0;
    const double *L = gls + GLS_L0, *beta = L + (size_t)q * q;
    const double *V = SX + (size_t)r * npad;
    for (int k = 0; k < r; ++k) {
        double s = SX[(size_t)i + (size_t)k * npad];
        for (int a = 0; a < q; ++a) s -= V[(size_t)i + (size_t)a * npad] * beta[a + (size_t)k * q];
        LR[(size_t)i + (size_t)k * npad] = ok ? s : 0.0;
    }
    if (!reml) return;
    double *C = LR + (size_t)r * npad;
    if (!ok) {
        for (int a = 0; a < q; ++a) C[(size_t)i + (size_t)a * npad] = 0.0;
        return;
    }
    for (int a = 0; a < q; ++a) {           // (c_b, b < a, is read back from this thread's own stores)
        double s = V[(size_t)i + (size_t)a * npad];
        for (int b = 0; b < a; ++b) s -= L[a + b * q] * C[(size_t)i + (size_t)b * npad];
        C[(size_t)i + (size_t)a * npad] = s / L[a + a * q];
    }
    const double sr = sqrt((double)r);
    for (int a = 0; a < q; ++a) C[(size_t)i + (size_t)a * npad] *= sr;
}

void launch_grad_lowrank(const double *fin, const double *SX, int npad, int r, int q, int reml, double *gls, double *LR,
                         hipStream_t s)
{
    hipLaunchKernelGGL(grad_gls_kernel, dim3(1), dim3(64), 0, s, fin, r, q, gls);
    hipLaunchKernelGGL(grad_lowrank_kernel, dim3((npad + 255) / 256), dim3(256), 0, s, SX, npad, r, q, reml, gls, LR);
}

// C(i, j) -= sum_k B(i, k) B(j, k) over the lower tiles of the leading npad x npad square (zero beforehand): -Sigma^-1.
// B is upper triangular, so the 256 columns from k0 on only reach the tile rows below k0 + 256: about n^3 / 3 flops.
void launch_grad_syrk(double *A, size_t lda, int npad, int brow0, hipStream_t s)
{
    const int nt = npad / TILE;
    UpdateLaunch u;
    u.C = A; u.ldc = lda; u.ldp = lda; u.lower_only = true;
    for (int t = 0; t < nt; t += 2) {
        const int kw = (t + 2 <= nt) ? 2 : 1;
        u.P = A + brow0 + (size_t)t * TILE * lda; u.K = kw * TILE;      // (rows brow0.. of C's own buffer: kblk stays 0, dense)
        u.ti1 = u.tj1 = t + kw;
        launch_update(u, s);
    }
}

// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
grad_site_kernel(LocArgs a, double *out, size_t stride, int smooth_free)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.n) return;
    double t_tilt = 0, t_sm = 0, t_sd = 0;
    for (int i = 0; i < a.p; ++i) {           // as loc_params_kernel
        const double x = a.X[w + (size_t)i * a.ldx];
        t_tilt = fma(x, a.th.tilt[i], t_tilt);
        t_sm = fma(x, a.th.smooth[i], t_sm);
        t_sd = fma(x, a.th.sd[i], t_sd);
    }
    const double pi = 3.14159265358979323846;
    const double et = exp(-t_tilt), st = 1.0 / (1.0 + et);
    const double tilt = pi * st;
    out[w + 0 * stride] = pi * st * (et * st);                       // dt/deta = pi s (1 - s)
    out[w + 1 * stride] = cos(tilt) / sin(tilt);
    double dnu = 0.0;
    if (smooth_free) {
        const double es = exp(-t_sm), ss = 1.0 / (1.0 + es);
        const double span = a.smooth_max - a.smooth_min;
        const double nu = span * ss + a.smooth_min;
        dnu = span * ss * (es * ss) / (2.0 * nu);                      // dlog(nu_ij)/deta_i = dnu_i / (2 nu_i)
    }
    out[w + 2 * stride] = dnu;
    out[w + 3 * stride] = exp(t_sd);
}

void launch_grad_site(const LocArgs &a, double *out, size_t stride, int smooth_free, hipStream_t s)
{
    if (a.n <= 0) return;
    hipLaunchKernelGGL(grad_site_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a, out, stride, smooth_free);
}


__device__ __forceinline__ double wave_sum(double v)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One workgroup per 64 x 64 tile (bi >= bj) of the lower triangle, lane = row, each wave 16 columns.  Entry (r, c), r > c,
// is the pair ii = c, jj = r.  Outputs per tile: the row sites' sums (over its columns), the column sites' sums (over its
// rows), per family, and the tile's global-range sum.
template <int MODE>
__global__ void __launch_bounds__(256)
grad_pair_kernel(GradArgs g)
{
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bi < bj) return;
    __shared__ double rows[4][GTS][GFAM];
    __shared__ double cols[GTS][GFAM];
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = bi * GTS + lane;
    const bool rin = r >= g.pad0 && r < g.n;
    double racc[GFAM] = {0, 0, 0, 0, 0, 0};
    double gacc = 0.0;
    for (int cc = 0; cc < GTS / 4; ++cc) {
        const int cl = wave * (GTS / 4) + cc;
        const int c = bj * GTS + cl;
        const bool cin = c >= g.pad0 && c < g.n;
        double dcol[GFAM] = {0, 0, 0, 0, 0, 0};
        if (rin && cin && r >= c) {
            double W = -g.coef * g.S[(size_t)r + (size_t)c * g.lds];
            for (int k = 0; k < g.nr; ++k) W -= g.AR[(size_t)r + (size_t)k * g.ldar] * g.AR[(size_t)c + (size_t)k * g.ldar];
            if (r == c) {
                racc[TH_SD_] += W * g.site[3 * g.stride + r];
                racc[TH_NG_] += W * g.loc[12 * g.stride + r];
            } else {
                double da[GFAM], db[GFAM], dg;
                pair_partials<MODE>(g.loc, g.stride, g.site, g.stride, g.gr, g.nu_fixed, g.smooth_free, c, r, da, db, dg);
                const double w2 = 2.0 * W;
                for (int f = 0; f < GFAM; ++f) { racc[f] += w2 * db[f]; dcol[f] = w2 * da[f]; }
                gacc += w2 * dg;
            }
        }
        for (int f = 0; f < GFAM; ++f) {            // (every lane of the wave takes part: the loop is wave-uniform)
            const double s = wave_sum(dcol[f]);
            if (lane == 0) cols[cl][f] = s;
        }
    }
    for (int f = 0; f < GFAM; ++f) rows[wave][lane][f] = racc[f];
    const double gw = wave_sum(gacc);
    if (lane == 0) red[wave] = gw;
    __syncthreads();
    const size_t tile = (size_t)bi * (bi + 1) / 2 + bj;
    double *prow = g.part_row + tile * GFAM * GTS, *pcol = g.part_col + tile * GFAM * GTS;
    for (int e = threadIdx.x; e < GFAM * GTS; e += 256) {
        const int f = e / GTS, l = e % GTS;
        prow[e] = ((rows[0][l][f] + rows[1][l][f]) + rows[2][l][f]) + rows[3][l][f];
        pcol[e] = cols[l][f];
    }
    if (threadIdx.x == 0) g.part_glob[tile] = ((red[0] + red[1]) + red[2]) + red[3];
}

// g[f][i] for every site: its tile row's row sums, then its tile column's column sums, in tile order.  rsum[i] = sum_c A(i, c).
__global__ void __launch_bounds__(256)
grad_reduce_kernel(GradArgs g)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int T = g.npad / GTS;
    if (i >= g.npad) return;
    const int t = i / GTS, l = i % GTS;
    for (int f = 0; f < GFAM; ++f) {
        double s = 0.0;
        for (int bj = 0; bj <= t; ++bj) s += g.part_row[((size_t)t * (t + 1) / 2 + bj) * GFAM * GTS + f * GTS + l];
        for (int bi = t; bi < T; ++bi) s += g.part_col[((size_t)bi * (bi + 1) / 2 + t) * GFAM * GTS + f * GTS + l];
        g.gsite[(size_t)f * g.npad + i] = s;
    }
    double a = 0.0;
    for (int k = 0; k < g.nr; ++k) a += g.AR[(size_t)i + (size_t)k * g.ldar];
    g.gsite[(size_t)GFAM * g.npad + i] = a;
}

__device__ double block_sum256(double v, double *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// out[t p + k] = c_{t,k} sum_i X(i, k) g_t(i)  (t < 6; c = 2 for scale k >= 1, 0 for scale k = 0 which takes the global
// sum instead, 1 otherwise); out[6 p + k] = -2 sum_i X(i, k) rsum(i).  One workgroup per output.
__global__ void __launch_bounds__(256)
grad_xt_kernel(GradArgs g)
{
    __shared__ double red[256];
    const int o = blockIdx.x, p = g.p;
    const int t = o / p, k = o % p;
    double s = 0.0;
    if (t == TH_SCALE_ && k == 0) {
        const int T = g.npad / GTS;
        const size_t ntile = (size_t)T * (T + 1) / 2;
        for (size_t e = threadIdx.x; e < ntile; e += 256) s += g.part_glob[e];
    } else {
        const double *gv = g.gsite + (size_t)(t < GFAM ? t : GFAM) * g.npad;
        for (int i = g.pad0 + threadIdx.x; i < g.n; i += 256) s = fma(g.X[(size_t)i + (size_t)k * g.ldx], gv[i], s);
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) {
        double c = 1.0;
        if (t == TH_SCALE_ && k > 0) c = 2.0;
        if (t == GFAM) c = -2.0;
        g.out[o] = c * s;
    }
}

void launch_grad_pairs(int mode, const GradArgs &g, hipStream_t s)
{
    const int T = g.npad / GTS;
    dim3 grid(T, T), blk(256);
    switch (mode) {
    case MODE_HALF: hipLaunchKernelGGL(grad_pair_kernel<MODE_HALF>, grid, blk, 0, s, g); break;
    case MODE_THREEHALF: hipLaunchKernelGGL(grad_pair_kernel<MODE_THREEHALF>, grid, blk, 0, s, g); break;
    case MODE_FIVEHALF: hipLaunchKernelGGL(grad_pair_kernel<MODE_FIVEHALF>, grid, blk, 0, s, g); break;
    default: hipLaunchKernelGGL(grad_pair_kernel<MODE_GEOM>, grid, blk, 0, s, g); break;
    }
    hipLaunchKernelGGL(grad_reduce_kernel, dim3((g.npad + 255) / 256), dim3(256), 0, s, g);
    hipLaunchKernelGGL(grad_xt_kernel, dim3(7 * g.p), dim3(256), 0, s, g);
}

size_t grad_scratch_doubles(int npad)
{
    const size_t T = (size_t)npad / GTS, ntile = T * (T + 1) / 2;
    return 2 * ntile * GFAM * GTS + ntile + (size_t)(GFAM + 1) * npad;
}

// ---------------------------------------------------------------------------
// Expected (Fisher) information of the dense model (cocons_fisher_dense):
//     I[a, b] = (r / 2) tr(Sigma^-1 Sigma_a Sigma^-1 Sigma_b),   Sigma_a = sum_{t,k} v_a[t, k] dSigma / dtheta[t, k].
//   fisher_weight_kernel : per direction and family, the site weights w_a[f][i] = c_f sum_k X(i, k) v_a[f, k]
//   dsigma_dirs_kernel   : the lower tiles of every Sigma_a from ONE evaluation of pair_partials per pair
//   fisher_mirror_kernel : a lower triangle mirrored into a full symmetric matrix (Sigma_a in place; Sigma^-1 from the
//                          gradient's -Sigma^-1, the sign folded in)
//   fisher_project_kernel: (cocons_fisher_reml) Sigma^-1 -> P = Sigma^-1 - C C' in place, the rank-p downdate
//   (the products Sigma_a Sigma^-1 run on the trailing-update kernel, launch_fisher_products)
//   fisher_trace_kernel / fisher_trace_sum_kernel : sum_ij G_a(i, j) G_b(j, i) per 64 x 64 tile, the transposed tile through
//                          LDS; then the tiles' partial sums in a fixed order
//   fisher_sx_kernel / fisher_xtsx_kernel : Sigma^-1 X and r X' (Sigma^-1 X), the mean block
// The matrices live in ONE tall buffer of npad-row blocks with a common leading dimension: that is the panel shape the
// trailing-update kernel multiplies row tiles of.
__global__ void __launch_bounds__(256)
fisher_weight_kernel(int n, int pad0, int npad, int p, const double *X, int ldx, const double *dirs, double *w)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, a = blockIdx.y;
    if (i >= npad) return;
    const bool in = i >= pad0 && i < n;
    const double *v = dirs + (size_t)a * GFAM * p;
    for (int f = 0; f < GFAM; ++f) {
        double s = 0.0;
        if (in)
            for (int k = (f == TH_SCALE_ ? 1 : 0); k < p; ++k) s = fma(X[(size_t)i + (size_t)k * ldx], v[f * p + k], s);
        w[((size_t)a * GFAM + f) * npad + i] = (f == TH_SCALE_ ? 2.0 : 1.0) * s;
    }
}

// One workgroup per 64 x 64 lower tile, lane = row, each wave 16 columns (as grad_pair_kernel).  Entry (r, c), r >= c, of
// direction a goes to D[a dstride + r + c ldd]: every entry of the lower tiles is written, the padding's with zeros.
template <int MODE>
__global__ void __launch_bounds__(256)
dsigma_dirs_kernel(GradArgs g, int ndir, const double *dirs, const double *w, double *D, size_t ldd, size_t dstride)
{
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bi < bj) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = bi * GTS + lane;
    const bool rin = r >= g.pad0 && r < g.n;
    for (int cc = 0; cc < GTS / 4; ++cc) {
        const int c = bj * GTS + wave * (GTS / 4) + cc;
        const bool cin = c >= g.pad0 && c < g.n;
        const bool live = rin && cin && r >= c;
        double da[GFAM] = {0, 0, 0, 0, 0, 0}, db[GFAM] = {0, 0, 0, 0, 0, 0}, dg = 0.0;
        if (live) {
            if (r == c) {                                   // the diagonal: exp(eta_sd) + nugget
                da[TH_SD_] = g.site[3 * g.stride + r];
                da[TH_NG_] = g.loc[12 * g.stride + r];
            } else pair_partials<MODE>(g.loc, g.stride, g.site, g.stride, g.gr, g.nu_fixed, g.smooth_free, c, r, da, db, dg);
        }
        if (r < c) continue;
        for (int a = 0; a < ndir; ++a) {
            double v = 0.0;
            if (live) {
                const double *wa = w + (size_t)a * GFAM * g.npad;
                for (int f = 0; f < GFAM; ++f) v += da[f] * wa[(size_t)f * g.npad + c] + db[f] * wa[(size_t)f * g.npad + r];
                v += dg * dirs[(size_t)a * GFAM * g.p + TH_SCALE_ * g.p];
            }
            D[(size_t)a * dstride + (size_t)r + (size_t)c * ldd] = v;
        }
    }
}

// Tile pair (bi, bj), bi >= bj, of matrix z: dst(bi, bj) = sign * the lower tile of src (its entries r >= c), dst(bj, bi)
// its transpose through LDS.  dst == src (sign = 1) mirrors in place: a workgroup touches its own two tiles only.
__global__ void __launch_bounds__(256)
fisher_mirror_kernel(double *dst, size_t ldd, size_t dz, const double *src, size_t lds, size_t sz, double sign)
{
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bi < bj) return;
    __shared__ double t[GTS][GTS + 1];
    dst += (size_t)blockIdx.z * dz;
    src += (size_t)blockIdx.z * sz;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int cc = 0; cc < GTS / 4; ++cc) {
        const int cl = wave * (GTS / 4) + cc;
        const int r = bi * GTS + lane, c = bj * GTS + cl;
        double v = 0.0;
        if (r >= c) {
            v = sign * src[(size_t)r + (size_t)c * lds];
            dst[(size_t)r + (size_t)c * ldd] = v;
        }
        t[cl][lane] = v;
    }
    __syncthreads();
    for (int cc = 0; cc < GTS / 4; ++cc) {
        const int cl = wave * (GTS / 4) + cc;
        const int r = bj * GTS + lane, c = bi * GTS + cl;
        if (r < c) dst[(size_t)r + (size_t)c * ldd] = t[lane][cl];
    }
}

// The REML projector in place (cocons_fisher_reml): S(i, j) -= scale sum_k C(i, k) C(j, k) over every 64 x 64
// tile of the full npad x npad matrix S = Sigma^-1, both triangles, C = Sigma^-1 X chol(X' Sigma^-1 X)^-T (npad x q, q <=
// COCONS_P_MAX).  One streaming pass: lane = row, each wave 16 columns (as fisher_mirror_kernel), the tile's two 64-row strips
// of C staged once in LDS, column by column (ci[k][lane]: one bank row per read; cj[k][c]: one address for the wave).  A row
// outside the caller's sites [pad0, n) takes C as 0, so the padding keeps the bits it has.  The sum over k runs in order, and
// entries (i, j) and (j, i) run the same products in the same order: P is symmetric to the bit where S is.
__global__ void __launch_bounds__(256)
fisher_project_kernel(double *S, size_t lds, const double *C, size_t ldc, int q, int pad0, int n, double scale)
{
    __shared__ double ci[COCONS_P_MAX][GTS], cj[COCONS_P_MAX][GTS];
    const int bi = blockIdx.x, bj = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ri = bi * GTS + lane, rj = bj * GTS + lane;
    for (int k = wave; k < q; k += 4) {
        ci[k][lane] = (ri >= pad0 && ri < n) ? C[(size_t)ri + (size_t)k * ldc] : 0.0;
        cj[k][lane] = (rj >= pad0 && rj < n) ? C[(size_t)rj + (size_t)k * ldc] : 0.0;
    }
    __syncthreads();
    double acc[GTS / 4];
    for (int cc = 0; cc < GTS / 4; ++cc) acc[cc] = 0.0;
    for (int k = 0; k < q; ++k) {
        const double a = ci[k][lane];
        for (int cc = 0; cc < GTS / 4; ++cc) acc[cc] = fma(a, cj[k][wave * (GTS / 4) + cc], acc[cc]);
    }
    double *col = S + (size_t)ri + (size_t)(bj * GTS + wave * (GTS / 4)) * lds;
    for (int cc = 0; cc < GTS / 4; ++cc) col[(size_t)cc * lds] -= scale * acc[cc];
}

// Workgroup (bi, bj, a): part[((a ndir + b) T + bj) T + bi] = sum over the tile of G_a(i, j) G_b(j, i) for every b >= a.
// The tile of G_a stays in registers; tile (bj, bi) of each G_b goes through LDS so that both reads are coalesced.
__global__ void __launch_bounds__(256)
fisher_trace_kernel(const double *G, size_t ld, size_t dstride, int ndir, double *part)
{
    __shared__ double t[GTS][GTS + 1];
    __shared__ double red[4];
    const int bi = blockIdx.x, bj = blockIdx.y, a = blockIdx.z, T = gridDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *Ga = G + (size_t)a * dstride;
    double mine[GTS / 4];
    for (int cc = 0; cc < GTS / 4; ++cc)
        mine[cc] = Ga[(size_t)(bi * GTS + lane) + (size_t)(bj * GTS + wave * (GTS / 4) + cc) * ld];
    for (int b = a; b < ndir; ++b) {
        const double *Gb = G + (size_t)b * dstride;
        __syncthreads();
        for (int cc = 0; cc < GTS / 4; ++cc) {
            const int cl = wave * (GTS / 4) + cc;
            t[cl][lane] = Gb[(size_t)(bj * GTS + lane) + (size_t)(bi * GTS + cl) * ld];
        }
        __syncthreads();
        double s = 0.0;
        for (int cc = 0; cc < GTS / 4; ++cc) s += mine[cc] * t[lane][wave * (GTS / 4) + cc];
        s = wave_sum(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) part[(((size_t)a * ndir + b) * T + bj) * T + bi] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// info[a, b] = info[b, a] = coef * (the tiles' partial sums, in a fixed order).  One workgroup per pair a <= b.
__global__ void __launch_bounds__(256)
fisher_trace_sum_kernel(const double *part, size_t ntile, int ndir, double coef, double *info)
{
    __shared__ double red[256];
    const int a = blockIdx.x / ndir, b = blockIdx.x % ndir;
    if (a > b) return;
    const double *pp = part + ((size_t)a * ndir + b) * ntile;
    double s = 0.0;
    for (size_t e = threadIdx.x; e < ntile; e += 256) s += pp[e];
    s = block_sum256(s, red);
    if (threadIdx.x == 0) {
        info[(size_t)a * ndir + b] = coef * s;
        info[(size_t)b * ndir + a] = coef * s;
    }
}

// part[(chunk p + c) npad + i] = sum_{k in chunk, a caller's site} S(i, k) X(k, c): S the full symmetric Sigma^-1
// (grad_sigma_r_sum_kernel adds the chunks in order)
__global__ void __launch_bounds__(64)
fisher_sx_kernel(const double *S, size_t lds, int n, int pad0, int npad, int p, const double *X, int ldx, double *part)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int chunk = (npad + GRAD_KSPLIT - 1) / GRAD_KSPLIT;
    const int k0 = max(pad0, (int)blockIdx.y * chunk), k1 = min(n, ((int)blockIdx.y + 1) * chunk);
    for (int c = 0; c < p; ++c) {
        double s = 0.0;
        for (int k = k0; k < k1; ++k) s = fma(S[(size_t)i + (size_t)k * lds], X[(size_t)k + (size_t)c * ldx], s);
        part[((size_t)blockIdx.y * p + c) * npad + i] = s;
    }
}

// out[k p + l] = out[l p + k] = coef sum_i X(i, k) SX(i, l), k <= l.  One workgroup per output.
__global__ void __launch_bounds__(256)
fisher_xtsx_kernel(int n, int pad0, int npad, int p, const double *X, int ldx, const double *SX, double coef, double *out)
{
    __shared__ double red[256];
    const int k = blockIdx.x / p, l = blockIdx.x % p;
    if (k > l) return;
    double s = 0.0;
    for (int i = pad0 + threadIdx.x; i < n; i += 256) s = fma(X[(size_t)i + (size_t)k * ldx], SX[(size_t)i + (size_t)l * npad], s);
    s = block_sum256(s, red);
    if (threadIdx.x == 0) {
        out[k * p + l] = coef * s;
        out[l * p + k] = coef * s;
    }
}

void launch_fisher_mirror(double *dst, size_t ldd, size_t dz, const double *src, size_t lds, size_t sz, int npad, int count,
                          double sign, hipStream_t s)
{
    const int T = npad / GTS;
    hipLaunchKernelGGL(fisher_mirror_kernel, dim3(T, T, count), dim3(256), 0, s, dst, ldd, dz, src, lds, sz, sign);
}

void launch_fisher_project(double *S, size_t lds, const double *C, size_t ldc, int q, int pad0, int n, int npad, double scale,
                           hipStream_t s)
{
    const int T = npad / GTS;
    hipLaunchKernelGGL(fisher_project_kernel, dim3(T, T), dim3(256), 0, s, S, lds, C, ldc, q, pad0, n, scale);
}

void launch_fisher_dirs(int mode, const GradArgs &g, int ndir, const double *dirs, double *w, double *D, size_t ldd,
                        size_t dstride, hipStream_t s)
{
    const int T = g.npad / GTS;
    dim3 grid(T, T), blk(256);
    hipLaunchKernelGGL(fisher_weight_kernel, dim3((g.npad + 255) / 256, ndir), blk, 0, s, g.n, g.pad0, g.npad, g.p, g.X, g.ldx,
                       dirs, w);
    switch (mode) {
    case MODE_HALF: hipLaunchKernelGGL(dsigma_dirs_kernel<MODE_HALF>, grid, blk, 0, s, g, ndir, dirs, w, D, ldd, dstride); break;
    case MODE_THREEHALF: hipLaunchKernelGGL(dsigma_dirs_kernel<MODE_THREEHALF>, grid, blk, 0, s, g, ndir, dirs, w, D, ldd, dstride); break;
    case MODE_FIVEHALF: hipLaunchKernelGGL(dsigma_dirs_kernel<MODE_FIVEHALF>, grid, blk, 0, s, g, ndir, dirs, w, D, ldd, dstride); break;
    default: hipLaunchKernelGGL(dsigma_dirs_kernel<MODE_GEOM>, grid, blk, 0, s, g, ndir, dirs, w, D, ldd, dstride); break;
    }
    launch_fisher_mirror(D, ldd, dstride, D, ldd, dstride, g.npad, ndir, 1.0, s);
}

// Block a + 2 of the tall buffer Tb (blocks of npad rows, leading dimension ldt) = -Sigma_a Sigma^-1 = -(Sigma^-1 Sigma_a)',
// with Sigma^-1 in block 0 and Sigma_a in block a + 1, from the last direction down: a product lands in the block the one
// before it has consumed (block ndir + 1 is the spare).  The trailing-update kernel forms C(I, J) -= sum_k P(I, k) P(J, k)
// for row tiles of ONE panel buffer: I runs over the rows of Sigma_a, J over those of Sigma^-1, FISHER_KP columns a launch.
constexpr int FISHER_KP = 512;
hipError_t launch_fisher_products(double *Tb, size_t ldt, int npad, int ndir, hipStream_t s)
{
    const int nt = npad / TILE;
    const size_t row = (size_t)npad * sizeof(double), pitch = ldt * sizeof(double);
    hipError_t e = hipMemset2DAsync(Tb + (size_t)(ndir + 1) * npad, pitch, 0, row, npad, s);
    UpdateLaunch u;
    u.C = Tb + npad; u.ldc = ldt; u.ldp = ldt; u.tj1 = nt;
    for (int a = ndir - 1; a >= 0 && e == hipSuccess; --a) {
        u.ti0 = (a + 1) * nt; u.ti1 = (a + 2) * nt;
        for (int k0 = 0; k0 < npad; k0 += FISHER_KP) {
            u.P = Tb + (size_t)k0 * ldt; u.K = min(FISHER_KP, npad - k0);      // (kblk stays 0: a dense buffer)
            launch_update(u, s);
        }
        if (a > 0) e = hipMemset2DAsync(Tb + (size_t)(a + 1) * npad, pitch, 0, row, npad, s);
    }
    return e;
}

size_t fisher_trace_scratch_doubles(int npad, int ndir) { return (size_t)ndir * ndir * (npad / GTS) * (npad / GTS); }

void launch_fisher_trace(const double *G, size_t ld, size_t dstride, int npad, int ndir, double coef, double *part, double *info,
                         hipStream_t s)
{
    const int T = npad / GTS;
    hipLaunchKernelGGL(fisher_trace_kernel, dim3(T, T, ndir), dim3(256), 0, s, G, ld, dstride, ndir, part);
    hipLaunchKernelGGL(fisher_trace_sum_kernel, dim3(ndir * ndir), dim3(256), 0, s, part, (size_t)T * T, ndir, coef, info);
}

void launch_fisher_mean(const double *S, size_t lds, int n, int pad0, int npad, int p, const double *X, int ldx, double coef,
                        double *part, double *SX, double *out, hipStream_t s)
{
    hipLaunchKernelGGL(fisher_sx_kernel, dim3(npad / 64, GRAD_KSPLIT), dim3(64), 0, s, S, lds, n, pad0, npad, p, X, ldx, part);
    hipLaunchKernelGGL(grad_sigma_r_sum_kernel, dim3((npad + 255) / 256), dim3(256), 0, s, part, npad, p, SX);
    hipLaunchKernelGGL(fisher_xtsx_kernel, dim3(p * p), dim3(256), 0, s, n, pad0, npad, p, X, ldx, SX, coef, out);
}

// ---------------------------------------------------------------------------
// Taper fit (cocons_neg2loglik_grad_taper): S = T o C(theta) on a CSR pattern, C = cov_rns_taper (matern_device.hpp
// taper_value_idx: isotropic, rho = e^(2 eta_scale) with the FULL scale vector).  With Z = S^-1 on the pattern (selinv.hip)
// and A = S^-1 R the weight of entry (i, j) is W = r Z_ij - sum_c A_ic A_jc; its two terms -- the log-determinant part and
// the quadratic-form part -- are carried apart.
//   taper_grad_entry_kernel : one thread per stored (lower) entry: W T times (C, U = P u dM/du, P nu dM/dnu + U / 2), the
//                             three numbers both sites' partials are made of; off-diagonal entries count twice
//   taper_grad_site_kernel  : one thread per site: its CSR row (row side), then its column through the transposed index
//                             (column side), in index order
//   taper_grad_xt_kernel    : X' g per part and family, and the mean gradient -2 X' A 1
constexpr int TG_SD = 0, TG_SCALE = 1, TG_SMOOTH = 2, TG_NG = 3, TG_FAM = 4;

// u of the pair (ia = row site, ib = column site) in taper_value_idx's arithmetic: both passes take the same branch
template <int MODE>
__device__ __forceinline__ double taper_u(const TaperGradArgs &g, int ia, int ib, double &nu)
{
    const double *L = g.loc;
    const size_t sl = g.stride;
    const double ax = L[ia], ay = L[sl + ia], bx = L[ib], by = L[sl + ib];
    const double ri = L[2 * sl + ia], rj = L[2 * sl + ib];
    nu = (MODE == MODE_GEOM) ? L[10 * sl + ia] * L[10 * sl + ib] : g.nu_fixed;
    const double global_range = (ri + rj) / 2;
    const double dx = ax - bx, dy = ay - by;
    return sqrt(8 * nu) * sqrt(dx * dx + dy * dy) / sqrt(global_range);
}

template <int MODE>
__global__ void __launch_bounds__(256)
taper_grad_entry_kernel(TaperGradArgs g)
{
    const double eps = 2.220446049250313e-16;
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= g.nnz) return;
    int lo = 0, hi = g.n - 1;                 // largest ii with rp[ii] - 1 <= w (taper_kernel)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (g.rp[mid] - 1 <= w) lo = mid; else hi = mid - 1;
    }
    const int ii = lo, jj = g.ci[w] - 1;
    const double *L = g.loc;
    const size_t sl = g.stride;
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
    const double t = g.tapv[w];
    if (ii == jj) {
        e0 = t * g.site[3 * sl + ii];
        e1 = t * L[12 * sl + ii];
    } else {
        double nu;
        const double u = taper_u<MODE>(g, ii, jj, nu);
        if (u <= eps) {                       // coincident: the row site's diagonal value
            e0 = 2.0 * t * g.site[3 * sl + ii];
            e1 = 2.0 * t * L[12 * sl + ii];
        } else if (!(u >= 706.0)) {           // (beyond: the reference's stand-in, derivatives round to 0)
            double M, Mu, Mn = 0.0;
            if (MODE == MODE_HALF) { M = exp(-u); Mu = -M; }
            else if (MODE == MODE_THREEHALF) { const double e = exp(-u); M = (1.0 + u) * e; Mu = -u * e; }
            else if (MODE == MODE_FIVEHALF) { const double e = exp(-u); M = (1.0 + u + u * u / 3.0) * e; Mu = -(u / 3.0) * (1.0 + u) * e; }
            else {
                matern_pair(nu, u, M, Mu);
                if (g.smooth_free) Mn = matern_dnu(nu, u);
            }
            const double ri = L[2 * sl + ii], rj = L[2 * sl + jj];
            const double P = (2 * sqrt(ri) * sqrt(rj)) / (ri + rj) * L[9 * sl + ii] * L[9 * sl + jj];
            const double U = P * Mu * u;
            e0 = 2.0 * t * (P * M);
            e1 = 2.0 * t * U;
            if (g.smooth_free) e2 = 2.0 * t * (P * Mn * nu + 0.5 * U);
        }
    }
    const double wl = g.coef * g.Z[band_index(ii, jj, g.ldz, g.skew, g.npad)];
    double wq = 0.0;
    for (int c = 0; c < g.nr; ++c) wq -= g.AR[(size_t)ii + (size_t)c * g.npad] * g.AR[(size_t)jj + (size_t)c * g.npad];
    const size_t nz = (size_t)g.nnz;
    g.ent[w] = wl * e0; g.ent[nz + w] = wl * e1; g.ent[2 * nz + w] = wl * e2;
    g.ent[3 * nz + w] = wq * e0; g.ent[4 * nz + w] = wq * e1; g.ent[5 * nz + w] = wq * e2;
}

template <int MODE>
__global__ void __launch_bounds__(256)
taper_grad_site_kernel(TaperGradArgs g)
{
    const double eps = 2.220446049250313e-16;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n) return;
    const size_t nz = (size_t)g.nnz, sl = g.stride;
    const double ri = g.loc[2 * sl + i];
    double acc[2][TG_FAM] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    auto side = [&](size_t w, int other) {        // an ordinary off-diagonal entry, seen from site i
        const double phi = ri / (ri + g.loc[2 * sl + other]);
        for (int q = 0; q < 2; ++q) {
            const double e0 = g.ent[(3 * q) * nz + w], e1 = g.ent[(3 * q + 1) * nz + w], e2 = g.ent[(3 * q + 2) * nz + w];
            acc[q][TG_SD] += 0.5 * e0;
            acc[q][TG_SCALE] += e0 * (1.0 - 2.0 * phi) - e1 * phi;
            acc[q][TG_SMOOTH] += e2;
        }
    };
    for (int w = g.rp[i] - 1; w < g.rp[i + 1] - 1; ++w) {          // row side
        const int j = g.ci[w] - 1;
        double nu;
        if (j == i || taper_u<MODE>(g, i, j, nu) <= eps) {
            for (int q = 0; q < 2; ++q) { acc[q][TG_SD] += g.ent[(3 * q) * nz + w]; acc[q][TG_NG] += g.ent[(3 * q + 1) * nz + w]; }
        } else side((size_t)w, j);
    }
    for (int t = g.tcp[i]; t < g.tcp[i + 1]; ++t) {                 // column side
        const int row = g.trow[t];
        double nu;
        if (row == i || taper_u<MODE>(g, row, i, nu) <= eps) continue;
        side((size_t)g.tidx[t], row);
    }
    const double dl = g.site[2 * sl + i];
    for (int q = 0; q < 2; ++q) {
        acc[q][TG_SMOOTH] *= dl;
        for (int f = 0; f < TG_FAM; ++f) g.gsite[(size_t)(q * TG_FAM + f) * g.npad + i] = acc[q][f];
    }
    double s = 0.0;
    for (int c = 0; c < g.nr; ++c) s += g.AR[(size_t)i + (size_t)c * g.npad];
    g.gsite[(size_t)(2 * TG_FAM) * g.npad + i] = s;
}

// out[(q 4 + f) p + k] = sum_i X(i, k) g_qf(i); out[8 p + k] = -2 sum_i X(i, k) rsum(i).  One workgroup per output.
__global__ void __launch_bounds__(256)
taper_grad_xt_kernel(TaperGradArgs g)
{
    __shared__ double red[256];
    const int o = blockIdx.x, v = o / g.p, k = o % g.p;
    const double *gv = g.gsite + (size_t)v * g.npad;
    double s = 0.0;
    for (int i = threadIdx.x; i < g.n; i += 256) s = fma(g.X[(size_t)i + (size_t)k * g.ldx], gv[i], s);
    s = block_sum256(s, red);
    if (threadIdx.x == 0) g.out[o] = (v == 2 * TG_FAM ? -2.0 : 1.0) * s;
}

void launch_taper_grad(int mode, const TaperGradArgs &g, hipStream_t s)
{
    if (g.nnz <= 0 || g.n <= 0) return;
    dim3 ge((g.nnz + 255) / 256), gs((g.n + 255) / 256), blk(256);
    switch (mode) {
    case MODE_HALF:
        hipLaunchKernelGGL(taper_grad_entry_kernel<MODE_HALF>, ge, blk, 0, s, g);
        hipLaunchKernelGGL(taper_grad_site_kernel<MODE_HALF>, gs, blk, 0, s, g);
        break;
    case MODE_THREEHALF:
        hipLaunchKernelGGL(taper_grad_entry_kernel<MODE_THREEHALF>, ge, blk, 0, s, g);
        hipLaunchKernelGGL(taper_grad_site_kernel<MODE_THREEHALF>, gs, blk, 0, s, g);
        break;
    case MODE_FIVEHALF:
        hipLaunchKernelGGL(taper_grad_entry_kernel<MODE_FIVEHALF>, ge, blk, 0, s, g);
        hipLaunchKernelGGL(taper_grad_site_kernel<MODE_FIVEHALF>, gs, blk, 0, s, g);
        break;
    default:
        hipLaunchKernelGGL(taper_grad_entry_kernel<MODE_GEOM>, ge, blk, 0, s, g);
        hipLaunchKernelGGL(taper_grad_site_kernel<MODE_GEOM>, gs, blk, 0, s, g);
        break;
    }
    hipLaunchKernelGGL(taper_grad_xt_kernel, dim3((2 * TG_FAM + 1) * g.p), blk, 0, s, g);
}

// ---------------------------------------------------------------------------
// Expected information of a tapered fit (cocons_fisher_taper): the direction matrices on the pattern,
//     S_a = T o sum_tk v_a[t, k] dC / dtheta[t, k],
// from the three numbers per entry the gradient forms (C = P M, U = P u dM/du, E = P nu dM/dnu + U / 2) and the site weights
// w_a[f][i] = sum_k X(i, k) v_a[f, k] (FULL scale vector: factor 1, k from 0).
//   taper_dirs_weight_kernel : the weights of the four families that enter the taper model
//   taper_dirs_entry_kernel  : one thread per stored (lower) entry, every direction from one evaluation of the pair
__global__ void __launch_bounds__(256)
taper_dirs_weight_kernel(TaperDirsArgs d)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, a = blockIdx.y;
    if (i >= d.g.npad) return;
    const int fam_row[TG_FAM] = {0, 1, 4, 5};      // std.dev, scale, smooth, nugget rows of the 6 x p table
    const int p = d.g.p;
    const double *v = d.dirs + (size_t)a * 6 * p;
    for (int f = 0; f < TG_FAM; ++f) {
        double s = 0.0;
        if (i < d.g.n)
            for (int k = 0; k < p; ++k) s = fma(d.g.X[(size_t)i + (size_t)k * d.g.ldx], v[fam_row[f] * p + k], s);
        d.wsite[((size_t)a * TG_FAM + f) * d.g.npad + i] = s;
    }
}

template <int MODE>
__global__ void __launch_bounds__(256)
taper_dirs_entry_kernel(TaperDirsArgs d)
{
    const double eps = 2.220446049250313e-16;
    const TaperGradArgs &g = d.g;
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= g.nnz) return;
    int lo = 0, hi = g.n - 1;                 // largest ii with rp[ii] - 1 <= w (taper_grad_entry_kernel)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (g.rp[mid] - 1 <= w) lo = mid; else hi = mid - 1;
    }
    const int ii = lo, jj = g.ci[w] - 1;
    const double *L = g.loc;
    const size_t sl = g.stride, np = (size_t)g.npad, nz = (size_t)g.nnz;
    const double t = g.tapv[w];
    // value = t * (c_sd (w_sd,i + w_sd,j) + c_sci w_sc,i + c_scj w_sc,j + c_smi w_sm,i + c_smj w_sm,j + c_ng w_ng,i)
    double c_sd = 0.0, c_sdj = 0.0, c_sci = 0.0, c_scj = 0.0, c_smi = 0.0, c_smj = 0.0, c_ng = 0.0;
    bool own = ii == jj;
    if (!own) {
        double nu;
        const double u = taper_u<MODE>(g, ii, jj, nu);
        if (u <= eps) own = true;             // coincident: the row site's diagonal value
        else if (!(u >= 706.0)) {             // (beyond: the reference's stand-in, derivatives round to 0)
            double M, Mu, Mn = 0.0;
            if (MODE == MODE_HALF) { M = exp(-u); Mu = -M; }
            else if (MODE == MODE_THREEHALF) { const double e = exp(-u); M = (1.0 + u) * e; Mu = -u * e; }
            else if (MODE == MODE_FIVEHALF) { const double e = exp(-u); M = (1.0 + u + u * u / 3.0) * e; Mu = -(u / 3.0) * (1.0 + u) * e; }
            else {
                matern_pair(nu, u, M, Mu);
                if (g.smooth_free) Mn = matern_dnu(nu, u);
            }
            const double ri = L[2 * sl + ii], rj = L[2 * sl + jj];
            const double P = (2 * sqrt(ri) * sqrt(rj)) / (ri + rj) * L[9 * sl + ii] * L[9 * sl + jj];
            const double C = P * M, U = P * Mu * u;
            const double phi_i = ri / (ri + rj), phi_j = rj / (ri + rj);
            c_sd = 0.5 * C; c_sdj = 0.5 * C;
            c_sci = C * (1.0 - 2.0 * phi_i) - U * phi_i;
            c_scj = C * (1.0 - 2.0 * phi_j) - U * phi_j;
            if (g.smooth_free) {
                const double E = P * Mn * nu + 0.5 * U;
                c_smi = E * g.site[2 * sl + ii];
                c_smj = E * g.site[2 * sl + jj];
            }
        }
    }
    if (own) { c_sd = g.site[3 * sl + ii]; c_ng = L[12 * sl + ii]; }
    for (int a = 0; a < d.ndir; ++a) {
        const double *wa = d.wsite + (size_t)a * TG_FAM * np;
        double v = c_sd * wa[TG_SD * np + ii] + c_sdj * wa[TG_SD * np + jj];
        v += c_sci * wa[TG_SCALE * np + ii] + c_scj * wa[TG_SCALE * np + jj];
        v += c_smi * wa[TG_SMOOTH * np + ii] + c_smj * wa[TG_SMOOTH * np + jj];
        v += c_ng * wa[TG_NG * np + ii];
        d.out[(size_t)a * nz + w] = t * v;
    }
}

void launch_taper_dirs(int mode, const TaperDirsArgs &d, hipStream_t s)
{
    if (d.g.nnz <= 0 || d.g.n <= 0 || d.ndir <= 0) return;
    hipLaunchKernelGGL(taper_dirs_weight_kernel, dim3((d.g.npad + 255) / 256, d.ndir), dim3(256), 0, s, d);
    dim3 ge((d.g.nnz + 255) / 256), blk(256);
    switch (mode) {
    case MODE_HALF: hipLaunchKernelGGL(taper_dirs_entry_kernel<MODE_HALF>, ge, blk, 0, s, d); break;
    case MODE_THREEHALF: hipLaunchKernelGGL(taper_dirs_entry_kernel<MODE_THREEHALF>, ge, blk, 0, s, d); break;
    case MODE_FIVEHALF: hipLaunchKernelGGL(taper_dirs_entry_kernel<MODE_FIVEHALF>, ge, blk, 0, s, d); break;
    default: hipLaunchKernelGGL(taper_dirs_entry_kernel<MODE_GEOM>, ge, blk, 0, s, d); break;
    }
}

}  // namespace cocons
