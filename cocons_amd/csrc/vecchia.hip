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
//   vecchia_sum_kernel    : the totals over the per-observation terms, as a two-stage tree of fixed shape.
//
// Every sum of a block runs in ascending row order of the block, which the host makes the ascending order of the caller's
// indices; nothing a block computes depends on another block, on n or on the launch.  No atomics but the integer atomicMin
// that reports a failing block.
//
// Compile with -ffp-contract=off (see matern_device.hpp).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "matern_device.hpp"

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
// element (r, c), r >= c, of the packed lower triangle (row after row)
__device__ __forceinline__ int tri_at(int r, int c) { return r * (r + 1) / 2 + c; }

// Dynamic LDS, sized by kb = m + 1 rows (vecchia_lds_bytes):
//   par   LOCP_FIELDS x kb   the block's parameters as an SoA of stride kb -- what pair_value_idx reads;
//   par2  LOCP_FIELDS x kb   PRED only: the same rows in the prediction branch's parameters, the prediction site last;
//   tri   kb (kb + 1) / 2    the block, then its factor (the pivots stay in registers: lane r keeps C(r, r));
//   nb    kb ints            the rows' locations.
template <int MODE, bool PRED>
__global__ void __launch_bounds__(64)
vecchia_block_kernel(VecchiaArgs a)
{
    extern __shared__ double vecchia_lds[];
    const int lane = threadIdx.x, row = blockIdx.x, kb = a.kb;
    double *par = vecchia_lds;
    double *par2 = par + (PRED ? LOCP_FIELDS * kb : 0);
    double *tri = par2 + LOCP_FIELDS * kb;
    int *nb = (int *)(tri + kb * (kb + 1) / 2);

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
    __syncthreads();
    // the block: pair t = r (r - 1) / 2 + c is (r, c), r > c, evaluated with the EARLIER row on the `ii` side (the reference's
    // orientation, which the u <= eps rule sees); PRED, last row: the prediction site on the `ii` side, exact coordinate
    // matches give its own diagonal value (cov_rns_pred)
    const int npairs = nrows * (nrows - 1) / 2;
    for (int t = lane; t < npairs; t += 64) {
        int r = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)t)) * 0.5f);
        while (r * (r - 1) / 2 > t) --r;
        while ((r + 1) * r / 2 <= t) ++r;
        const int c = t - r * (r - 1) / 2;
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
        if (lane == 0) atomicMin(a.fail, a.row0 + row + 1);
        return;
    }
    __syncthreads();
    // forward substitution over the neighbours' rows, VECCHIA_G right-hand sides at a time; lane k ends with
    // b_k - sum_j C(k, j) y_j, j ascending
    const int site = lane < nrows ? nb[lane] : 0;
    for (int c0 = 0; c0 < a.nb; c0 += VECCHIA_G) {
        double b[VECCHIA_G];
#pragma unroll
        for (int g = 0; g < VECCHIA_G; ++g)
            b[g] = (lane < nrows && c0 + g < a.nb && !(PRED && lane == k)) ? a.B[(size_t)site + (size_t)(c0 + g) * a.ldb] : 0.0;
        for (int j = 0; j < k; ++j) {
            const double l = (lane > j && lane < nrows) ? tri[myrow + j] : 0.0;
#pragma unroll
            for (int g = 0; g < VECCHIA_G; ++g) {
                const double yj = __shfl(lane == j ? b[g] / piv_mine : 0.0, j);
                b[g] -= l * yj;
            }
        }
        if (lane == k) {
#pragma unroll
            for (int g = 0; g < VECCHIA_G; ++g) {
                if (c0 + g >= a.nb) break;
                if (PRED) a.stoch[row] = 0.0 - b[g];                  // c' K^-1 resid = (C^-1 c)' (C^-1 resid)
                else a.Y[(size_t)row + (size_t)(c0 + g) * a.ldy] = b[g] / piv_mine;
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
    case MODE_HALF: hipLaunchKernelGGL((vecchia_block_kernel<MODE_HALF, PRED>), grid, block, shm, s, a); break;
    case MODE_THREEHALF: hipLaunchKernelGGL((vecchia_block_kernel<MODE_THREEHALF, PRED>), grid, block, shm, s, a); break;
    case MODE_FIVEHALF: hipLaunchKernelGGL((vecchia_block_kernel<MODE_FIVEHALF, PRED>), grid, block, shm, s, a); break;
    default: hipLaunchKernelGGL((vecchia_block_kernel<MODE_GEOM, PRED>), grid, block, shm, s, a); break;
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
vecchia_sum_kernel(const double *v, size_t ldv, int n, double *part)
{
    __shared__ double red[256];
    const int seg = blockIdx.x, q = blockIdx.y, t = threadIdx.x;
    const double *col = v + (size_t)q * ldv;
    double acc = 0.0;
    for (int s = 0; s < VECCHIA_SUM_SEG / 256; ++s) {
        const size_t i = (size_t)seg * VECCHIA_SUM_SEG + (size_t)s * 256 + t;
        if (i < (size_t)n) { const double x = col[i]; acc += q > 0 ? x * x : x; }
    }
    const double total = vecchia_tree(acc, red);
    if (t == 0) part[(size_t)q * gridDim.x + seg] = total;
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
    hipLaunchKernelGGL(vecchia_sum_kernel, dim3(nseg, ncol), dim3(256), 0, s, v, ldv, n, part);
    hipLaunchKernelGGL(vecchia_sum_final_kernel, dim3(ncol), dim3(256), 0, s, part, nseg, out);
}

}  // namespace cocons
