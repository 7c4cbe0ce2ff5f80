// solve.hip -- the kernels that read a FINISHED factor (gfx950, fp64 MFMA): the reductions behind the likelihood and the
// predictions (finalize, row_reduce), the draws Y = L E + trend (trmm_lower, band_trmm, gather_rows) and kriging from a held
// factor, dense and band (krige_*, krige_band_*, krige_schur, sym_mirror; krige_band_gram: the folds' K_BB = V V' of
// cocons_cv_taper_folds), and the band sweeps, sparse product and Gram sums of
// the tapered fit's expected information (band_*).  No hand-offs, no mailboxes: nothing here changes
// when a schedule of the factorisation (chol.hip) does.  Storage and the register "blk layout": chol.hip, tile_ops.hpp.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include "kernels.h"
#include "tile_ops.hpp"

namespace cocons {

__device__ __forceinline__ double block_sum(double v, double *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    __syncthreads();
    return t;    // valid on thread 0
}

// block b < nr*nr: Gram entry (b / nr, b % nr) over columns [c0,c1) and < n;
// block nr*nr: sum of log of the diagonal over the same columns.
__global__ void __launch_bounds__(1024)
finalize_kernel(const double *A, size_t lda, int c0, int c1, int n, int row0, int nr, double *out, int skew, int npad,
                const double *A2, int a2_cols)
{
    // A2 != NULL (dense layout only): the factor of the dependency-driven schedule -- the part of a column BELOW the 256 x 256
    // diagonal block it runs through lives in A2 (columns [256, a2_cols): the panels its tasks formed), everything else in A
    __shared__ double red[16];
    const int b = blockIdx.x;
    const int hi = c1 < n ? c1 : n;
    double s = 0.0;
    // every element sits in a cache line of its own (stride lda): 1024 threads with four loads in flight each -- with 256
    // threads and one load at a time the kernel was 25 us of serial round trips at n = 10^4, on the critical path of
    // every evaluation
    constexpr int U = 4;
    const int step = (int)blockDim.x;
    if (b == nr * nr) {
        for (int c = c0 + (int)threadIdx.x; c < hi; c += U * step) {
            double v[U];
#pragma unroll
            for (int q = 0; q < U; ++q) v[q] = (c + q * step < hi) ? A[band_index(c + q * step, c + q * step, lda, skew, npad)] : 1.0;
#pragma unroll
            for (int q = 0; q < U; ++q) s += log(v[q]);
        }
    } else {
        const int ra = row0 + b / nr, rb = row0 + b % nr;
        for (int c = c0 + (int)threadIdx.x; c < hi; c += U * step) {
            double va[U], vb[U];
#pragma unroll
            for (int q = 0; q < U; ++q) {
                const bool in = c + q * step < hi;
                const int cc = c + q * step;
                int below0 = 2 * TILE * (cc / (2 * TILE) + 1);                // first row below column cc's diagonal block
                if (npad > 0 && below0 > npad) below0 = npad;                 // (a last block of one tile)
                const bool in2 = A2 && cc >= 2 * TILE && cc < a2_cols;
                const double *Sa = (in2 && ra >= below0) ? A2 : A;
                const double *Sb = (in2 && rb >= below0) ? A2 : A;
                va[q] = in ? Sa[band_index(ra, cc, lda, skew, npad)] : 0.0;
                vb[q] = in ? Sb[band_index(rb, cc, lda, skew, npad)] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < U; ++q) s += va[q] * vb[q];
        }
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[b == nr * nr ? 0 : 1 + b] = s;
}

// Per-row reductions for predict, in two deterministic stages (no floating-point atomics, so the
// kriging outputs are bit-reproducible run to run like the reference's crossprod / rowSums):
// stage 1: partial sums over chunks of `cchunk` columns -> scratch[(chunk * 2 + {0,1}) * m + i]
// stage 2: the chunks of one row summed in ascending order.
__global__ void __launch_bounds__(256)
row_reduce_kernel(const double *A, size_t lda, int n, int rowy, int row0, int m,
                  double *scratch, int cchunk, int skew, int npad, const double *A2, int a2_cols)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int cb = blockIdx.y * cchunk;
    const int ce = (cb + cchunk < n) ? cb + cchunk : n;
    if (i >= m) return;
    // (A2: the factor of the dependency-driven schedule -- below the diagonal blocks the columns [256, a2_cols) live in the
    // second buffer, launch_finalize; the rows read here lie under the matrix, and a chunk of 256 columns is one panel)
    if (A2 && cb >= 2 * TILE && cb < a2_cols) A = A2;
    double s = 0.0, q = 0.0;
    for (int c = cb; c < ce; ++c) {
        double v = A[band_index(row0 + i, c, lda, skew, npad)];
        double y = A[band_index(rowy, c, lda, skew, npad)];
        s = fma(v, y, s);
        q = fma(v, v, q);
    }
    scratch[((size_t)blockIdx.y * 2 + 0) * m + i] = s;
    scratch[((size_t)blockIdx.y * 2 + 1) * m + i] = q;
}

__global__ void __launch_bounds__(256)
row_reduce_final_kernel(const double *scratch, int m, int nchunks, double *stoch, double *quad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double s = 0.0, q = 0.0;
    for (int c = 0; c < nchunks; ++c) {
        s += scratch[((size_t)c * 2 + 0) * m + i];
        q += scratch[((size_t)c * 2 + 1) * m + i];
    }
    stoch[i] = s;
    quad[i] = q;
}

void launch_finalize_cols(const double *A, size_t lda, int c0, int c1, int n, int row0, int nr,
                          double *out, hipStream_t s)
{
    hipLaunchKernelGGL(finalize_kernel, dim3(nr * nr + 1), dim3(1024), 0, s, A, lda, c0, c1, n, row0, nr, out, 0, 0,
                       (const double *)nullptr, 0);
}

void launch_finalize(const double *A, size_t lda, int n, int row0, int nr, double *out, hipStream_t s, int skew, int npad,
                     const double *A2, int a2_cols)
{
    hipLaunchKernelGGL(finalize_kernel, dim3(nr * nr + 1), dim3(1024), 0, s, A, lda, 0, n, n, row0, nr, out, skew, npad,
                       skew ? (const double *)nullptr : A2, a2_cols);
}

size_t row_reduce_scratch_doubles(int n, int m)
{
    return (size_t)2 * (size_t)m * (size_t)((n + 255) / 256);
}

void launch_row_reduce(const double *A, size_t lda, int n, int rowy, int row0, int m,
                       double *stoch, double *quad, double *scratch, hipStream_t s, int skew, int npad,
                       const double *A2, int a2_cols)
{
    if (m <= 0) return;
    const int cchunk = 2 * TILE, nchunks = (n + cchunk - 1) / cchunk;
    hipLaunchKernelGGL(row_reduce_kernel, dim3((m + 255) / 256, nchunks), dim3(256), 0, s,
                       A, lda, n, rowy, row0, m, scratch, cchunk, skew, npad, skew ? (const double *)nullptr : A2, a2_cols);
    hipLaunchKernelGGL(row_reduce_final_kernel, dim3((m + 255) / 256), dim3(256), 0, s,
                       scratch, m, nchunks, stoch, quad);
}

// ---------------------------------------------------------------------------
// Y = L E + trend for the lower factor L (marginal simulation: cocoSim's t(iiderrors) %*% cholS,
// R/sim.R:172, is (L E)^T).  One workgroup per 64-row block, lanes along rows (coalesced reads of
// L's columns), the four waves split the k-range and are summed through LDS; E(k, s) is
// wave-uniform.  HBM-bound: the lower triangle of L is read once per group of 8 columns of E.
__global__ void __launch_bounds__(256)
trmm_lower_kernel(const double *A, size_t lda, int n, const double *E, int lde, int nsim,
                  const double *trend, double *Y, int ldy)
{
    __shared__ double red[4][8][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rb = gridDim.x - 1 - blockIdx.x;          // longest rows first
    const int i = rb * 64 + lane;
    const int kend = (rb + 1) * 64 < n ? (rb + 1) * 64 : n;
    for (int s0 = 0; s0 < nsim; s0 += 8) {
        double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = wave; k < kend; k += 4) {
            double l = (i < n && k <= i) ? A[(size_t)i + (size_t)k * lda] : 0.0;
#pragma unroll
            for (int s = 0; s < 8; ++s)
                if (s0 + s < nsim) acc[s] = fma(l, E[(size_t)k + (size_t)(s0 + s) * lde], acc[s]);
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) red[wave][s][lane] = acc[s];
        __syncthreads();
        if (wave == 0 && i < n) {
#pragma unroll
            for (int s = 0; s < 8; ++s)
                if (s0 + s < nsim)
                    Y[(size_t)i + (size_t)(s0 + s) * ldy] =
                        ((red[0][s][lane] + red[1][s][lane]) + (red[2][s][lane] + red[3][s][lane])) + trend[i];
        }
        __syncthreads();
    }
}

void launch_trmm_lower(const double *A, size_t lda, int n, const double *E, int lde, int nsim,
                       const double *trend, double *Y, int ldy, hipStream_t s)
{
    if (n <= 0 || nsim <= 0) return;
    hipLaunchKernelGGL(trmm_lower_kernel, dim3((n + 63) / 64), dim3(256), 0, s, A, lda, n, E, lde, nsim, trend, Y, ldy);
}

// ---------------------------------------------------------------------------
// Y = L E + trend for the factor a band-limited factorisation leaves (taper handles: cocoSim's sparse branch,
// (t(iiderrors) %*% cholS) + trend, R/sim.R:214-216).  One workgroup per (128-row tile row I, block of BT_COLS draws):
// it walks the tile columns c of row I inside the envelope (hi[c] > I, hi monotone: a suffix of [0, I]), stages the
// 128 x 64 block of E that column c multiplies in LDS and multiplies the band tile L(I, c) into it on
// v_mfma_f64_16x16x4_f64, so each band tile is read once per BT_COLS draws.  Wave w owns rows 32 w .. 32 w + 31 of the
// tile row (two 16-row blocks) and all four 16-column draw blocks: eight accumulators in blk layout.  Only the lower
// triangle of the diagonal tile is read; E's rows >= n and columns >= nsim are staged as zeros and never read, rows and
// columns of Y beyond n / nsim are not written.  The sum order of every element is fixed (c ascending, then the 16-column
// k blocks, then the MFMA's own order): two launches give identical bits.
constexpr int BT_COLS = 64;
constexpr size_t BT_LDS_BYTES = (size_t)TILE * BT_COLS * sizeof(double);      // 64 KiB

// E staged for the Q operand of blk_mma: 16 x 16 blocks (k block kb = obs / 16, draw block jb = draw / 16) of 256 doubles,
// element (draw j, obs k) of a block at k * 16 + (j ^ k): the XOR spreads the staging stores (consecutive obs) over the
// banks and leaves every read of lds_blk's shape a permutation of 64 contiguous doubles
__device__ __forceinline__ int bt_lds_index(int k, int j)
{
    return (((k >> 4) * (BT_COLS / 16) + (j >> 4)) << 8) + ((k & 15) << 4) + ((j ^ k) & 15);
}

__global__ void __launch_bounds__(256)
band_trmm_kernel(const double *A, size_t lda, int skew, int npad, const int *hi, int n, const double *E, int lde,
                 int nsim, const double *trend, double *Y, int ldy)
{
    extern __shared__ double Es[];
    const int I = blockIdx.x, s0 = blockIdx.y * BT_COLS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // first tile column whose envelope reaches tile row I (hi[I] > I always)
    int c0 = 0;
    if (hi) {
        int lo = 0, up = I;
        while (lo < up) {
            const int mid = (lo + up) >> 1;
            if (hi[mid] > I) up = mid; else lo = mid + 1;
        }
        c0 = lo;
    }
    d4 acc[2][4];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) acc[rb][jb] = d4{0.0, 0.0, 0.0, 0.0};
    const int row0 = I * TILE + 32 * wave;        // first row of the wave's two 16-row blocks
    for (int c = c0; c <= I; ++c) {
        __syncthreads();                          // every wave is done with the previous block of E
        for (int e = threadIdx.x; e < TILE * BT_COLS; e += 256) {
            const int k = e & (TILE - 1), j = e >> 7;
            const int gk = c * TILE + k, gj = s0 + j;
            Es[bt_lds_index(k, j)] = (gk < n && gj < nsim) ? E[(size_t)gk + (size_t)gj * lde] : 0.0;
        }
        __syncthreads();
        // tile column c addressed by global row and column indices (kernels.h band_index / band_base)
        const double *Ac = skew ? A - (ptrdiff_t)TILE * c : A;
        const bool diag = c == I;
#pragma unroll
        for (int kb = 0; kb < TILE / 16; ++kb) {
            if (diag && kb > 2 * wave + 1) break;          // above the diagonal for both of the wave's row blocks
            d4 P[2];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                const int lb = 2 * wave + rb;              // 16-row block inside the tile
                if (diag && kb > lb) { P[rb] = d4{0.0, 0.0, 0.0, 0.0}; continue; }
                P[rb] = glb_blk(Ac, lda, row0 + 16 * rb, c * TILE + 16 * kb, lane);
                if (diag && kb == lb) {                    // lower triangle of the diagonal block: row lane & 15, col 4 r + lane >> 4
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (4 * r + (lane >> 4) > (lane & 15)) P[rb][r] = 0.0;
                }
            }
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) {
                const double *blk = Es + ((kb * (BT_COLS / 16) + jb) << 8);
                d4 Q;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = (lane >> 4) + 4 * r, j = lane & 15;
                    Q[r] = blk[(k << 4) + ((j ^ k) & 15)];
                }
                blk_mma(acc[0][jb], P[0], Q);
                blk_mma(acc[1][jb], P[1], Q);
            }
        }
    }
    // acc[rb][jb] in blk layout: row (lane & 15) of the 16-row block, draw 4 r + (lane >> 4) of the 16-draw block
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int i = row0 + 16 * rb + (lane & 15);
        if (i >= n) continue;
        const double t = trend[i];
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = s0 + 16 * jb + 4 * r + (lane >> 4);
                if (j < nsim) Y[(size_t)i + (size_t)j * ldy] = acc[rb][jb][r] + t;
            }
    }
}

void launch_band_trmm(const double *A, size_t lda, int skew, int npad, const int *d_hi, int nt, int n, const double *E,
                      int lde, int nsim, const double *trend, double *Y, int ldy, hipStream_t s)
{
    if (n <= 0 || nsim <= 0 || nt <= 0) return;
    static std::atomic<unsigned long long> attr_done{0};
    set_dynamic_lds_once((const void *)band_trmm_kernel, BT_LDS_BYTES, attr_done);
    hipLaunchKernelGGL(band_trmm_kernel, dim3(nt, (nsim + BT_COLS - 1) / BT_COLS), dim3(256), BT_LDS_BYTES, s,
                       A, lda, skew, npad, d_hi, n, E, lde, nsim, trend, Y, ldy);
}

// out[i + s ldo] = Y[pos[i] + s ldy], i < n, s < ncol: rows of Y (the handle's order) back to the caller's order
__global__ void __launch_bounds__(256)
gather_rows_kernel(const double *Y, int ldy, const int *pos, int n, int ncol, double *out, int ldo)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = pos[i];
    for (int s = blockIdx.y; s < ncol; s += gridDim.y) out[(size_t)i + (size_t)s * ldo] = Y[(size_t)k + (size_t)s * ldy];
}

void launch_gather_rows(const double *Y, int ldy, const int *pos, int n, int ncol, double *out, int ldo, hipStream_t s)
{
    if (n <= 0 || ncol <= 0) return;
    const int gy = ncol < 64 ? ncol : 64;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((n + 255) / 256, gy), dim3(256), 0, s, Y, ldy, pos, n, ncol, out, ldo);
}

// ---------------------------------------------------------------------------
// Kriging from a held factor (cocons_krige_*): V = C L^-T for a chunk C of cross-covariance rows (M x npad, column-major,
// ld ldc), with stoch[i] = V(i,:) w and quad[i] = V(i,:) V(i,:)' taken as V is formed; V itself overwrites C.
//
// The factor is held PACKED: lower tile (I, J), I >= J, of 128 x 128 doubles (column-major, ld 128) at tile index
// I (I + 1) / 2 + J, strict upper triangle of the diagonal tiles zero.  Per diagonal tile the solve also keeps the
// 4 x 4 inverse operands of trsm16 (2048 doubles, the layout fetch_factor_tile reads: [16-block j][group s][lane]).
//
// Right-looking over the 128-column tiles J = 0 .. nt-1, two launches per tile:
//   krige_diag_kernel   V_J = R_J L_JJ^-T   one workgroup per 64-row strip (a wave 16 rows): trsm_tile_kernel's block
//                       substitution in registers, then the strip's partial reductions, added to stoch / quad in J order
//   krige_update_kernel R_I -= V_J L_IJ^T  for every I > J: one workgroup per (64-row strip, tile I), K = 128 on
//                       v_mfma_f64_16x16x4_f64; L_IJ streams through LDS in four 32-column slices
// Every element's sum order is fixed by J, the 16-column blocks and the MFMA's own order, and a row never meets another
// row: the outputs of a row do not depend on M, on the chunk split or on the other rows (bit for bit, given the row's
// position modulo 64 -- the caller's chunks are multiples of 64 rows).
// Columns outside [c_lo, c_hi) (the handle's front padding and slots) are zero in V whatever C holds there.

// (I, J) of packed tile t
__device__ __forceinline__ void krige_tile_ij(int t, int &I, int &J)
{
    int i = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    while (i * (i + 1) / 2 > t) --i;
    I = i; J = t - i * (i + 1) / 2;
}

__global__ void __launch_bounds__(256)
krige_pack_kernel(const double *A, size_t lda, double *Lp)
{
    int I, J;
    krige_tile_ij((int)blockIdx.x, I, J);
    const double *src = A + (size_t)I * TILE + (size_t)J * TILE * lda;
    double *dst = Lp + (size_t)blockIdx.x * TILE * TILE;
    for (int e = threadIdx.x; e < TILE * TILE; e += 256) {
        const int r = e & (TILE - 1), c = e >> 7;
        const double v = src[(size_t)r + (size_t)c * lda];
        dst[e] = (I == J && r < c) ? 0.0 : v;
    }
}

// per diagonal tile J: the trsm16 operands (inverse of every 4 x 4 diagonal sub-block, formed as potrf16_step forms it,
// with 1 / l for the pivot reciprocals) and w's 128 entries (row `rowy` of A, zero outside [c_lo, c_hi))
__global__ void __launch_bounds__(256)
krige_qprep_kernel(const double *A, size_t lda, int rowy, int c_lo, int c_hi, double *Qp, double *w)
{
    const int J = blockIdx.x, tid = threadIdx.x;
    if (tid < TILE) {
        const int c = J * TILE + tid;
        w[c] = (c >= c_lo && c < c_hi) ? A[(size_t)rowy + (size_t)c * lda] : 0.0;
    }
    for (int e = tid; e < 8 * 256; e += 256) {
        const int jb = e >> 8, s = (e >> 6) & 3, lane = e & 63;
        const int m = lane & 15, k = lane >> 4, c = m & 3;
        double q = 0.0;
        if ((m >> 2) == s && k <= c) {
            const double *L = A + (size_t)(J * TILE + 16 * jb + 4 * s) * (1 + lda);      // the 4 x 4 diagonal sub-block
            const double l10 = L[1], l20 = L[2], l30 = L[3], l21 = L[2 + lda], l31 = L[3 + lda], l32 = L[3 + 2 * lda];
            const double r0 = 1.0 / L[0], r1 = 1.0 / L[1 + lda], r2 = 1.0 / L[2 + 2 * lda], r3 = 1.0 / L[3 + 3 * lda];
            const double m00 = r0, m11 = r1, m22 = r2, m33 = r3;
            const double m10 = -(l10 * m00) * r1;
            const double m21 = -(l21 * m11) * r2;
            const double m32 = -(l32 * m22) * r3;
            const double m20 = -fma(l21, m10, l20 * m00) * r2;
            const double m31 = -fma(l32, m21, l31 * m11) * r3;
            const double m30 = -fma(l32, m20, fma(l31, m10, l30 * m00)) * r3;
            q = sel_lower4(c, k, m00, m10, m11, m20, m21, m22, m30, m31, m32, m33);
        }
        Qp[(size_t)J * 2048 + e] = q;
    }
}

// LDS 90 KiB (the 36 lower 16 x 16 blocks of L_JJ and its trsm16 operands): one workgroup per CU.  There are only
// M / 64 of them per launch and each is short; the update launches carry the arithmetic.
__global__ void __launch_bounds__(256)
krige_diag_kernel(const double *Lp, const double *Qp, const double *w, double *C, size_t ldc, int J, int c_lo, int c_hi,
                  double *stoch, double *quad)
{
    __shared__ double SL[36 * 256];
    __shared__ double QS[8 * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    fetch_factor_tile<false>(Lp + (size_t)(J * (J + 1) / 2 + J) * TILE * TILE, TILE, 0, Qp + (size_t)J * 2048, SL, QS, tid);
    const int rs = 64 * (int)blockIdx.x + 16 * wave, c0 = J * TILE;
    d4 B[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        B[j] = glb_blk(C, ldc, rs, c0 + 16 * j, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = c0 + 16 * j + 4 * r + (lane >> 4);
            if (c < c_lo || c >= c_hi) B[j][r] = 0.0;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        d4 L = lds_blk(SL + (j * (j + 1) / 2 + j) * 256, lane);
        double Q[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) Q[s] = QS[j * 256 + s * 64 + lane];
        trsm16(B[j], L, Q);
        d4 NX = -B[j];
#pragma unroll
        for (int jj = j + 1; jj < 8; ++jj) {
            d4 Lb = lds_blk(SL + (jj * (jj + 1) / 2 + j) * 256, lane);
            blk_mma(B[jj], NX, Lb);
        }
    }
    // row (lane & 15) of the wave's 16 rows, columns 16 j + 4 r + (lane >> 4): partial sums in (j, r) order, then the four
    // column groups of a row combined in a fixed tree
    double sp = 0.0, qp = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = c0 + 16 * j + 4 * r + (lane >> 4);
            const double v = (c < c_lo || c >= c_hi) ? 0.0 : B[j][r];
            B[j][r] = v;
            sp = fma(v, w[c], sp);
            qp = fma(v, v, qp);
        }
    sp += __shfl_xor(sp, 16);
    qp += __shfl_xor(qp, 16);
    sp += __shfl_xor(sp, 32);
    qp += __shfl_xor(qp, 32);
    if (lane < 16) {
        const int i = rs + lane;
        if (J == 0) { stoch[i] = sp; quad[i] = qp; }
        else { stoch[i] += sp; quad[i] += qp; }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) glb_blk_store(C, ldc, rs, c0 + 16 * j, lane, B[j]);
}

// R_I -= V_J L_IJ^T, I = J + 1 + blockIdx.y, rows 64 blockIdx.x .. + 63 (a wave 16 rows, all 128 columns of tile I in
// eight accumulators).  LDS 32 KiB (a 128 x 32 slice of L_IJ as 16 x 16 blocks in lds_blk layout).  188 VGPRs + 64 AGPRs
// (the register-staged slice included): 2 waves per SIMD, 2 workgroups per CU; no scratch.
constexpr int KU_KC = 32;
__global__ void __launch_bounds__(256)
krige_update_kernel(const double *Lp, double *C, size_t ldc, int J)
{
    __shared__ double LS[TILE * KU_KC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int I = J + 1 + (int)blockIdx.y;
    const double *Lt = Lp + (size_t)(I * (I + 1) / 2 + J) * TILE * TILE;
    const int rs = 64 * (int)blockIdx.x + 16 * wave;
    d4 acc[8];
#pragma unroll
    for (int jb = 0; jb < 8; ++jb) acc[jb] = glb_blk(C, ldc, rs, I * TILE + 16 * jb, lane);
    for (int kc = 0; kc < TILE / KU_KC; ++kc) {
        double v[TILE * KU_KC / 256];
#pragma unroll
        for (int q = 0; q < TILE * KU_KC / 256; ++q) {
            const int e = tid + 256 * q, j = e & (TILE - 1), k = e >> 7;
            v[q] = Lt[(size_t)j + (size_t)(KU_KC * kc + k) * TILE];
        }
        __syncthreads();                  // every wave is done with the previous slice
#pragma unroll
        for (int q = 0; q < TILE * KU_KC / 256; ++q) {
            const int e = tid + 256 * q, j = e & (TILE - 1), k = e >> 7;
            LS[(((j >> 4) * (KU_KC / 16) + (k >> 4)) << 8) + ((k & 15) << 4) + (j & 15)] = v[q];
        }
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < KU_KC / 16; ++kb) {
            const d4 NP = -glb_blk(C, ldc, rs, J * TILE + KU_KC * kc + 16 * kb, lane);
#pragma unroll
            for (int jb = 0; jb < 8; ++jb) {
                const d4 Q = lds_blk(LS + ((jb * (KU_KC / 16) + kb) << 8), lane);
                blk_mma(acc[jb], NP, Q);
            }
        }
    }
#pragma unroll
    for (int jb = 0; jb < 8; ++jb) glb_blk_store(C, ldc, rs, I * TILE + 16 * jb, lane, acc[jb]);
}

void launch_krige_pack(const double *A, size_t lda, int nt, int rowy, int c_lo, int c_hi, double *Lp, double *Qp, double *w,
                       hipStream_t s)
{
    if (nt <= 0) return;
    hipLaunchKernelGGL(krige_pack_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, s, A, lda, Lp);
    hipLaunchKernelGGL(krige_qprep_kernel, dim3(nt), dim3(256), 0, s, A, lda, rowy, c_lo, c_hi, Qp, w);
}

void launch_krige_solve(const double *Lp, const double *Qp, const double *w, int nt, double *C, size_t ldc, int rows,
                        int c_lo, int c_hi, double *stoch, double *quad, hipStream_t s)
{
    if (rows <= 0 || nt <= 0) return;
    const unsigned strips = (unsigned)((rows + 63) / 64);
    for (int J = 0; J < nt; ++J) {
        hipLaunchKernelGGL(krige_diag_kernel, dim3(strips), dim3(256), 0, s, Lp, Qp, w, C, ldc, J, c_lo, c_hi, stoch, quad);
        if (J + 1 < nt)
            hipLaunchKernelGGL(krige_update_kernel, dim3(strips, (unsigned)(nt - 1 - J)), dim3(256), 0, s, Lp, C, ldc, J);
    }
}

// ---------------------------------------------------------------------------
// Kriging from a held BAND factor (cocons_krige_taper_*): the same right-looking solve for a taper handle, whose factor
// fills only the tile envelope J <= I < hi[J] and whose chunk C is sparse.  Tile I of the running right-hand side is
// updated only by tile columns K with I < hi[K] <= K + W (W = max_J (hi[J] - J)), so at step J only the tile columns
// J .. J + W - 1 are live: the chunk buffer is a RING of W slots of 128 columns (rows x W * 128, column-major, ld ldr),
// tile column I in slot I mod W.  Per step J:
//   load    tile column J + W - 1 (step 0: the first min(W, nt)) enters the slot tile J - 1 just left: the slot is zeroed
//           and the chunk's entries of that tile column are scattered into it (krige_band_scatter_kernel; the host has
//           bucketed them by tile column, so every stored entry is touched once)
//   diag    V_J = R_J L_JJ^-T and the strip's partial reductions, as krige_diag_kernel
//   update  R_I -= V_J L_IJ^T for J < I < hi[J], as krige_update_kernel
// The factor is held packed per tile column: tile (I, J) at tile index toff[J] + (I - J), 128 x 128 column-major, the
// strict upper triangle of the diagonal tiles zero; Qp and w as launch_krige_pack leaves them.  The padding columns
// (>= n) of a slot are zero and the padding of the factor is the identity, so V is zero there without a mask.
// Sum orders are those of the dense kernels: a row's outputs depend on the row's entries and its position modulo 64 only.

// grid (W, nt): tile (J + blockIdx.x, J = blockIdx.y) of the factor in A (band_index layout) -> its packed place
__global__ void __launch_bounds__(256)
krige_band_pack_kernel(const double *A, size_t lda, int skew, int npad, const int *hi, int nt, const int *toff, double *Lp)
{
    const int J = blockIdx.y, I = J + (int)blockIdx.x;
    if (I >= (hi ? hi[J] : nt)) return;
    double *dst = Lp + (size_t)(toff[J] + (I - J)) * TILE * TILE;
    for (int e = threadIdx.x; e < TILE * TILE; e += 256) {
        const int r = e & (TILE - 1), c = e >> 7;
        const double v = A[band_index(I * TILE + r, J * TILE + c, lda, skew, npad)];
        dst[e] = (I == J && r < c) ? 0.0 : v;
    }
}

// krige_qprep_kernel's arithmetic with the factor addressed through band_index; w = row `rowy`, zero from column n on
__global__ void __launch_bounds__(256)
krige_band_qprep_kernel(const double *A, size_t lda, int skew, int npad, int rowy, int n, double *Qp, double *w)
{
    const int J = blockIdx.x, tid = threadIdx.x;
    if (tid < TILE) {
        const int c = J * TILE + tid;
        w[c] = c < n ? A[band_index(rowy, c, lda, skew, npad)] : 0.0;
    }
    for (int e = tid; e < 8 * 256; e += 256) {
        const int jb = e >> 8, s = (e >> 6) & 3, lane = e & 63;
        const int m = lane & 15, k = lane >> 4, c = m & 3;
        double q = 0.0;
        if ((m >> 2) == s && k <= c) {
            const int d0 = J * TILE + 16 * jb + 4 * s;                                     // the 4 x 4 diagonal sub-block
            auto L = [&](int i, int j) { return A[band_index(d0 + i, d0 + j, lda, skew, npad)]; };
            const double l10 = L(1, 0), l20 = L(2, 0), l30 = L(3, 0), l21 = L(2, 1), l31 = L(3, 1), l32 = L(3, 2);
            const double r0 = 1.0 / L(0, 0), r1 = 1.0 / L(1, 1), r2 = 1.0 / L(2, 2), r3 = 1.0 / L(3, 3);
            const double m00 = r0, m11 = r1, m22 = r2, m33 = r3;
            const double m10 = -(l10 * m00) * r1;
            const double m21 = -(l21 * m11) * r2;
            const double m32 = -(l32 * m22) * r3;
            const double m20 = -fma(l21, m10, l20 * m00) * r2;
            const double m31 = -fma(l32, m21, l31 * m11) * r3;
            const double m30 = -fma(l32, m20, fma(l31, m10, l30 * m00)) * r3;
            q = sel_lower4(c, k, m00, m10, m11, m20, m21, m22, m30, m31, m32, m33);
        }
        Qp[(size_t)J * 2048 + e] = q;
    }
}

// entries [0, count) of one tile column's bucket: slot[dst[k]] = val[src[k]] * tapv[src[k]] (dst = row + column in the
// tile * ldr; the pattern's columns are strictly increasing within a row, so no two entries share a destination)
__global__ void __launch_bounds__(256)
krige_band_scatter_kernel(double *slot, const int *dst, const int *src, int count, const double *val, const double *tapv)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    const int w = src[k];
    slot[dst[k]] = tapv[w] * val[w];
}

// V_J = R_J L_JJ^-T in the slot S (64 blockIdx.x .. + 63 of its rows, ld ldr), Lt = the packed diagonal tile, Qt / wt its
// operands and the 128 entries of w; first: J == 0 (the sums start here).  LDS as krige_diag_kernel.
__global__ void __launch_bounds__(256)
krige_band_diag_kernel(const double *Lt, const double *Qt, const double *wt, double *S, size_t ldr, int first, double *stoch,
                       double *quad)
{
    __shared__ double SL[36 * 256];
    __shared__ double QS[8 * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    fetch_factor_tile<false>(Lt, TILE, 0, Qt, SL, QS, tid);
    const int rs = 64 * (int)blockIdx.x + 16 * wave;
    d4 B[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) B[j] = glb_blk(S, ldr, rs, 16 * j, lane);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        d4 L = lds_blk(SL + (j * (j + 1) / 2 + j) * 256, lane);
        double Q[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) Q[s] = QS[j * 256 + s * 64 + lane];
        trsm16(B[j], L, Q);
        d4 NX = -B[j];
#pragma unroll
        for (int jj = j + 1; jj < 8; ++jj) {
            d4 Lb = lds_blk(SL + (jj * (jj + 1) / 2 + j) * 256, lane);
            blk_mma(B[jj], NX, Lb);
        }
    }
    // partial sums in (j, r) order, then the four column groups of a row in a fixed tree (krige_diag_kernel)
    double sp = 0.0, qp = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double v = B[j][r];
            sp = fma(v, wt[16 * j + 4 * r + (lane >> 4)], sp);
            qp = fma(v, v, qp);
        }
    sp += __shfl_xor(sp, 16);
    qp += __shfl_xor(qp, 16);
    sp += __shfl_xor(sp, 32);
    qp += __shfl_xor(qp, 32);
    if (lane < 16) {
        const int i = rs + lane;
        if (first) { stoch[i] = sp; quad[i] = qp; }
        else { stoch[i] += sp; quad[i] += qp; }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) glb_blk_store(S, ldr, rs, 16 * j, lane, B[j]);
}

// R_I -= V_J L_IJ^T, I = J + 1 + blockIdx.y: Lcol = the packed tiles of tile column J (tile I at Lcol + (I - J) tiles), ring
// slot I mod W updated from slot jslot = J mod W.  Registers and LDS as krige_update_kernel.
__global__ void __launch_bounds__(256)
krige_band_update_kernel(const double *Lcol, double *ring, size_t ldr, int jslot, int W)
{
    __shared__ double LS[TILE * KU_KC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = 1 + (int)blockIdx.y, islot = jslot + d < W ? jslot + d : jslot + d - W;      // I = J + d, jslot = J mod W
    const double *Lt = Lcol + (size_t)d * TILE * TILE;
    const int cv = jslot * TILE, cr = islot * TILE;         // first ring columns of V_J and of R_I
    const int rs = 64 * (int)blockIdx.x + 16 * wave;
    d4 acc[8];
#pragma unroll
    for (int jb = 0; jb < 8; ++jb) acc[jb] = glb_blk(ring, ldr, rs, cr + 16 * jb, lane);
    for (int kc = 0; kc < TILE / KU_KC; ++kc) {
        double v[TILE * KU_KC / 256];
#pragma unroll
        for (int q = 0; q < TILE * KU_KC / 256; ++q) {
            const int e = tid + 256 * q, j = e & (TILE - 1), k = e >> 7;
            v[q] = Lt[(size_t)j + (size_t)(KU_KC * kc + k) * TILE];
        }
        __syncthreads();                  // every wave is done with the previous slice
#pragma unroll
        for (int q = 0; q < TILE * KU_KC / 256; ++q) {
            const int e = tid + 256 * q, j = e & (TILE - 1), k = e >> 7;
            LS[(((j >> 4) * (KU_KC / 16) + (k >> 4)) << 8) + ((k & 15) << 4) + (j & 15)] = v[q];
        }
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < KU_KC / 16; ++kb) {
            const d4 NP = -glb_blk(ring, ldr, rs, cv + KU_KC * kc + 16 * kb, lane);
#pragma unroll
            for (int jb = 0; jb < 8; ++jb) {
                const d4 Q = lds_blk(LS + ((jb * (KU_KC / 16) + kb) << 8), lane);
                blk_mma(acc[jb], NP, Q);
            }
        }
    }
#pragma unroll
    for (int jb = 0; jb < 8; ++jb) glb_blk_store(ring, ldr, rs, cr + 16 * jb, lane, acc[jb]);
}

void launch_krige_band_pack(const double *A, size_t lda, int skew, int npad, int n, const int *d_hi, int nt, int W,
                            const int *d_toff, double *Lp, double *Qp, double *w, hipStream_t s)
{
    if (nt <= 0 || W <= 0) return;
    hipLaunchKernelGGL(krige_band_pack_kernel, dim3((unsigned)W, (unsigned)nt), dim3(256), 0, s, A, lda, skew, npad, d_hi, nt,
                       d_toff, Lp);
    hipLaunchKernelGGL(krige_band_qprep_kernel, dim3(nt), dim3(256), 0, s, A, lda, skew, npad, npad, n, Qp, w);
}

hipError_t launch_krige_band_load(double *slot, size_t ldr, const int *dst, const int *src, int count, const double *val,
                                  const double *tapv, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(slot, 0, ldr * TILE * sizeof(double), s);
    if (e != hipSuccess || count <= 0) return e;
    hipLaunchKernelGGL(krige_band_scatter_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, slot, dst, src, count,
                       val, tapv);
    return hipSuccess;
}

__global__ void __launch_bounds__(256)
krige_band_schur_kernel(const double *ring, size_t ldr, int Wr, int t0, int t1, double *S, size_t lds);      // (below)
__global__ void __launch_bounds__(256)
krige_band_gram_kernel(const double *ring, size_t ldr, int Wr, int t0, int t1, const KrigeGramTask *tasks, double *blocks);

hipError_t launch_krige_band_solve(const KrigeBandSolve &a, hipStream_t s)
{
    if (a.rows <= 0 || a.nt <= 0) return hipSuccess;
    const unsigned strips = (unsigned)((a.rows + 63) / 64);
    const int nt = a.nt, W = a.W;
    const int Wr = a.Wr > 0 ? a.Wr : W;                 // the ring's modulus; the live window stays W
    const int D = (a.S || a.tasks) ? std::max(a.depth, 1) : 0;
    const unsigned mpad = (unsigned)((a.rows + TILE - 1) / TILE * TILE);
    auto load = [&](int I) {
        const int k0 = a.boff[I], k1 = a.boff[I + 1];
        return launch_krige_band_load(a.ring + (size_t)(I % Wr) * TILE * a.ldr, a.ldr, a.bdst + k0, a.bsrc + k0, k1 - k0, a.val,
                                      a.tapv, s);
    };
    for (int I = 0; I < std::min(W, nt); ++I)
        if (hipError_t e = load(I)) return e;
    for (int J = 0; J < nt; ++J) {
        if (J > 0 && J + W - 1 < nt)
            if (hipError_t e = load(J + W - 1)) return e;
        const double *Lcol = a.Lp + (size_t)a.toff[J] * TILE * TILE;
        hipLaunchKernelGGL(krige_band_diag_kernel, dim3(strips), dim3(256), 0, s, Lcol, a.Qp + (size_t)J * 2048,
                           a.w + (size_t)J * TILE, a.ring + (size_t)(J % Wr) * TILE * a.ldr, a.ldr, J == 0 ? 1 : 0, a.stoch, a.quad);
        // the group [J / D * D, J] is solved and still in the ring: its product leaves for S before a later load takes a slot
        if (D && ((J + 1) % D == 0 || J + 1 == nt)) {
            if (a.tasks) {
                if (a.ntasks > 0)
                    hipLaunchKernelGGL(krige_band_gram_kernel, dim3((unsigned)a.ntasks), dim3(256), 0, s, a.ring, a.ldr, Wr,
                                       J / D * D, J + 1, a.tasks, a.blocks);
            } else
                hipLaunchKernelGGL(krige_band_schur_kernel, dim3(mpad / 64, mpad / TILE), dim3(256), 0, s, a.ring, a.ldr, Wr,
                                   J / D * D, J + 1, a.S, a.lds);
        }
        const int hj = a.hi ? a.hi[J] : nt;
        if (hj - J - 1 > 0)
            hipLaunchKernelGGL(krige_band_update_kernel, dim3(strips, (unsigned)(hj - J - 1)), dim3(256), 0, s, Lcol, a.ring, a.ldr,
                               J % Wr, Wr);
    }
    return hipGetLastError();
}

// Predictive covariance from the solved chunk (cocons_krige_joint): S(I, J) -= V(I, :) V(J, :)' over the lower 128 x 128
// tiles of S.  One workgroup per (64-row strip of tile row I, tile column J <= I): a wave 16 rows, all 128 columns of
// the tile in eight accumulators, as krige_update_kernel.  Both operands are rows of the same V (column-major, ld ldv):
// the strip's 64 x 32 slab and tile J's 128 x 32 slab of a K slice go through registers into LDS as 16 x 16 blocks in
// lds_blk layout, 48 KiB together.  Rows >= m of either slab are read as zero (ldv may end before S's padding does).
// K runs over the columns [k0, k1) in slices of 32, in 16-column blocks, in the MFMA's own order -- the same sequence for
// every element of S, whatever m or the grid: no K split, no atomics, nothing between workgroups.  The strips inside a
// diagonal tile form the whole 64 x 128 block, entries above the diagonal included (launch_sym_mirror overwrites them).
constexpr int KS_KC = 32;
__global__ void __launch_bounds__(256)
krige_schur_kernel(const double *V, size_t ldv, int m, int k0, int k1, double *S, size_t lds)
{
    __shared__ double PS[64 * KS_KC];
    __shared__ double QS[TILE * KS_KC];
    const int strip = blockIdx.x, J = blockIdx.y;
    if (2 * J > strip) return;                      // tile J lies right of the strip's diagonal tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = 64 * strip, c0 = J * TILE, rs = r0 + 16 * wave;
    d4 acc[8];
#pragma unroll
    for (int jb = 0; jb < 8; ++jb) acc[jb] = glb_blk(S, lds, rs, c0 + 16 * jb, lane);
    for (int kc = k0; kc < k1; kc += KS_KC) {
        double vq[TILE * KS_KC / 256], vp[64 * KS_KC / 256];
#pragma unroll
        for (int q = 0; q < TILE * KS_KC / 256; ++q) {
            const int e = tid + 256 * q, j = e & (TILE - 1), k = e >> 7;
            vq[q] = c0 + j < m ? V[(size_t)(c0 + j) + (size_t)(kc + k) * ldv] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 64 * KS_KC / 256; ++q) {
            const int e = tid + 256 * q, i = e & 63, k = e >> 6;
            vp[q] = r0 + i < m ? V[(size_t)(r0 + i) + (size_t)(kc + k) * ldv] : 0.0;
        }
        __syncthreads();                  // every wave is done with the previous slice
#pragma unroll
        for (int q = 0; q < TILE * KS_KC / 256; ++q) {
            const int e = tid + 256 * q, j = e & (TILE - 1), k = e >> 7;
            QS[(((j >> 4) * (KS_KC / 16) + (k >> 4)) << 8) + ((k & 15) << 4) + (j & 15)] = vq[q];
        }
#pragma unroll
        for (int q = 0; q < 64 * KS_KC / 256; ++q) {
            const int e = tid + 256 * q, i = e & 63, k = e >> 6;
            PS[(((i >> 4) * (KS_KC / 16) + (k >> 4)) << 8) + ((k & 15) << 4) + (i & 15)] = vp[q];
        }
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < KS_KC / 16; ++kb) {
            const d4 NP = -lds_blk(PS + ((wave * (KS_KC / 16) + kb) << 8), lane);
#pragma unroll
            for (int jb = 0; jb < 8; ++jb) {
                const d4 Q = lds_blk(QS + ((jb * (KS_KC / 16) + kb) << 8), lane);
                blk_mma(acc[jb], NP, Q);
            }
        }
    }
#pragma unroll
    for (int jb = 0; jb < 8; ++jb) glb_blk_store(S, lds, rs, c0 + 16 * jb, lane, acc[jb]);
}

// The same product with both operands read from the kriging ring of a band factor (cocons_krige_taper_joint): S(I, J) -=
// sum over the tile columns t in [t0, t1) of V_t(I, :) V_t(J, :)', V_t the 128 solved columns at ring column (t mod Wr) * 128.
// krige_schur_kernel's tile scheme, registers and LDS: per tile column the slices of 32, the 16-column blocks and the MFMA
// order are its own, and the tile columns come in ascending order; the accumulators go back to S between launches, which is
// exact -- every element of S sees ONE sequence over the columns whatever the grouping.  The ring has ldr = round_up(m, 64)
// rows (those >= m exactly zero: a slot is zeroed before its entries arrive); rows >= ldr are read as zero.
__global__ void __launch_bounds__(256)
krige_band_schur_kernel(const double *ring, size_t ldr, int Wr, int t0, int t1, double *S, size_t lds)
{
    __shared__ double PS[64 * KS_KC];
    __shared__ double QS[TILE * KS_KC];
    const int strip = blockIdx.x, J = blockIdx.y;
    if (2 * J > strip) return;                      // tile J lies right of the strip's diagonal tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = 64 * strip, c0 = J * TILE, rs = r0 + 16 * wave;
    const int mr = (int)ldr;
    d4 acc[8];
#pragma unroll
    for (int jb = 0; jb < 8; ++jb) acc[jb] = glb_blk(S, lds, rs, c0 + 16 * jb, lane);
    // one loop over the slices of every tile column of the group: slice s of tile column t at ring column (t mod Wr) 128 + 32 s
    for (int sl = t0 * (TILE / KS_KC); sl < t1 * (TILE / KS_KC); ++sl) {
        const int t = sl / (TILE / KS_KC), kc = (sl % (TILE / KS_KC)) * KS_KC;
        const double *V = ring + (size_t)(t % Wr) * TILE * ldr;
        double vq[TILE * KS_KC / 256], vp[64 * KS_KC / 256];
#pragma unroll
        for (int q = 0; q < TILE * KS_KC / 256; ++q) {
            const int e = tid + 256 * q, j = e & (TILE - 1), k = e >> 7;
            vq[q] = c0 + j < mr ? V[(size_t)(c0 + j) + (size_t)(kc + k) * ldr] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 64 * KS_KC / 256; ++q) {
            const int e = tid + 256 * q, i = e & 63, k = e >> 6;
            vp[q] = r0 + i < mr ? V[(size_t)(r0 + i) + (size_t)(kc + k) * ldr] : 0.0;
        }
        __syncthreads();                  // every wave is done with the previous slice
#pragma unroll
        for (int q = 0; q < TILE * KS_KC / 256; ++q) {
            const int e = tid + 256 * q, j = e & (TILE - 1), k = e >> 7;
            QS[(((j >> 4) * (KS_KC / 16) + (k >> 4)) << 8) + ((k & 15) << 4) + (j & 15)] = vq[q];
        }
#pragma unroll
        for (int q = 0; q < 64 * KS_KC / 256; ++q) {
            const int e = tid + 256 * q, i = e & 63, k = e >> 6;
            PS[(((i >> 4) * (KS_KC / 16) + (k >> 4)) << 8) + ((k & 15) << 4) + (i & 15)] = vp[q];
        }
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < KS_KC / 16; ++kb) {
            const d4 NP = -lds_blk(PS + ((wave * (KS_KC / 16) + kb) << 8), lane);
#pragma unroll
            for (int jb = 0; jb < 8; ++jb) {
                const d4 Q = lds_blk(QS + ((jb * (KS_KC / 16) + kb) << 8), lane);
                blk_mma(acc[jb], NP, Q);
            }
        }
    }
#pragma unroll
    for (int jb = 0; jb < 8; ++jb) glb_blk_store(S, lds, rs, c0 + 16 * jb, lane, acc[jb]);
}

// The fold-aware Gram product of cross-validation by folds (cocons_cv_taper_folds): D += V_t(strip, :) V_t(tile, :)' over the
// tile columns t in [t0, t1), one workgroup per task -- a 64-row strip of the ring against a 128-row tile of the ring, both
// inside one fold (or one tile of packed small folds), into the task's own block.  krige_band_schur_kernel's slab staging,
// K order and accumulators-through-memory between groups: every element sees ONE summation sequence whatever the grouping,
// the chunk or the other tasks.  The sign is the only difference (K_BB = V V' is added), the operands are read with the
// same guard (ring rows >= ldr count as zero).
__global__ void __launch_bounds__(256)
krige_band_gram_kernel(const double *ring, size_t ldr, int Wr, int t0, int t1, const KrigeGramTask *tasks, double *blocks)
{
    __shared__ double PS[64 * KS_KC];
    __shared__ double QS[TILE * KS_KC];
    const KrigeGramTask tk = tasks[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = tk.row0, c0 = tk.col0;
    const int mr = (int)ldr;
    double *D = blocks + tk.dst;
    const size_t ldd = (size_t)tk.ld;
    d4 acc[8];
#pragma unroll
    for (int jb = 0; jb < 8; ++jb) acc[jb] = glb_blk(D, ldd, 16 * wave, 16 * jb, lane);
    for (int sl = t0 * (TILE / KS_KC); sl < t1 * (TILE / KS_KC); ++sl) {
        const int t = sl / (TILE / KS_KC), kc = (sl % (TILE / KS_KC)) * KS_KC;
        const double *V = ring + (size_t)(t % Wr) * TILE * ldr;
        double vq[TILE * KS_KC / 256], vp[64 * KS_KC / 256];
#pragma unroll
        for (int q = 0; q < TILE * KS_KC / 256; ++q) {
            const int e = tid + 256 * q, j = e & (TILE - 1), k = e >> 7;
            vq[q] = c0 + j < mr ? V[(size_t)(c0 + j) + (size_t)(kc + k) * ldr] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 64 * KS_KC / 256; ++q) {
            const int e = tid + 256 * q, i = e & 63, k = e >> 6;
            vp[q] = r0 + i < mr ? V[(size_t)(r0 + i) + (size_t)(kc + k) * ldr] : 0.0;
        }
        __syncthreads();                  // every wave is done with the previous slice
#pragma unroll
        for (int q = 0; q < TILE * KS_KC / 256; ++q) {
            const int e = tid + 256 * q, j = e & (TILE - 1), k = e >> 7;
            QS[(((j >> 4) * (KS_KC / 16) + (k >> 4)) << 8) + ((k & 15) << 4) + (j & 15)] = vq[q];
        }
#pragma unroll
        for (int q = 0; q < 64 * KS_KC / 256; ++q) {
            const int e = tid + 256 * q, i = e & 63, k = e >> 6;
            PS[(((i >> 4) * (KS_KC / 16) + (k >> 4)) << 8) + ((k & 15) << 4) + (i & 15)] = vp[q];
        }
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < KS_KC / 16; ++kb) {
            const d4 P = lds_blk(PS + ((wave * (KS_KC / 16) + kb) << 8), lane);
#pragma unroll
            for (int jb = 0; jb < 8; ++jb) {
                const d4 Q = lds_blk(QS + ((jb * (KS_KC / 16) + kb) << 8), lane);
                blk_mma(acc[jb], P, Q);
            }
        }
    }
#pragma unroll
    for (int jb = 0; jb < 8; ++jb) glb_blk_store(D, ldd, 16 * wave, 16 * jb, lane, acc[jb]);
}

void launch_krige_schur(const double *V, size_t ldv, int m, int c_lo, int c_hi, int npad, double *S, size_t lds, hipStream_t s)
{
    if (m <= 0 || c_hi <= c_lo) return;
    const int mpad = (m + TILE - 1) / TILE * TILE;
    hipLaunchKernelGGL(krige_schur_kernel, dim3((unsigned)(mpad / 64), (unsigned)(mpad / TILE)), dim3(256), 0, s, V, ldv, m,
                       c_lo / TILE * TILE, npad, S, lds);
}

// S(j, i) = S(i, j) for i > j, i < n: the upper triangle becomes the mirror of the lower one, in 64 x 64 tiles through LDS
__global__ void __launch_bounds__(256)
sym_mirror_kernel(double *S, size_t lds, int n)
{
    __shared__ double T[64 * 65];
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int cc = w; cc < 64; cc += 4) {
        const int r = 64 * bi + l, c = 64 * bj + cc;
        T[cc * 65 + l] = (r < n && c < n) ? S[(size_t)r + (size_t)c * lds] : 0.0;
    }
    __syncthreads();
    // target (row 64 bj + l, column 64 bi + rr) = source (row 64 bi + rr, column 64 bj + l)
    for (int rr = w; rr < 64; rr += 4) {
        const int tr = 64 * bj + l, tc = 64 * bi + rr;
        if (tr < tc && tc < n) S[(size_t)tr + (size_t)tc * lds] = T[l * 65 + rr];
    }
}

void launch_sym_mirror(double *S, size_t lds, int n, hipStream_t s)
{
    if (n <= 0) return;
    const unsigned t = (unsigned)((n + 63) / 64);
    hipLaunchKernelGGL(sym_mirror_kernel, dim3(t, t), dim3(256), 0, s, S, lds, n);
}

// ---------------------------------------------------------------------------
// Expected information of a tapered fit on the band factor (cocons_fisher_taper).  Rows -- probes, then every
// direction's vectors -- live in full-width buffers (rows x npad, column-major, the row index fastest): the kriging ring at
// W = nt, tile column I in slot I.  Per chunk of probe rows E:
//   back solve   W = E L^-1           the forward pair on the flipped transpose M = F L' F of the factor (band_back_pack),
//                                     the rows' columns flipped: column npad - 1 - c of the buffer holds column c
//   spmm         U_a = W S_a          band_spmm_dirs_kernel, every direction from one gather of W
//   sweep        Q = U L^-T           the forward pair on the factor's own packed tiles (launch_band_sweep)
//   gram         sum Q_a o Q_b        band_gram_kernel per 64-row strip and column segment, then fixed-order sums
// No kernel here meets another row of a buffer, and every sum has one order: a row's contribution depends on its entries and its
// position modulo 64 only.

// grid (W, nt): tile (I' = J' + blockIdx.x, J' = blockIdx.y) of M = F L' F, element (r, c) = L's tile (nt - 1 - J', nt - 1 - I')
// at (127 - c, 127 - r); the strict upper triangle of M's diagonal tiles zero
__global__ void __launch_bounds__(256)
band_back_pack_kernel(const double *A, size_t lda, int skew, int npad, const int *hib, int nt, const int *toffb, double *Mp)
{
    const int Jp = blockIdx.y, Ip = Jp + (int)blockIdx.x;
    if (Ip >= hib[Jp]) return;
    const int Lr = nt - 1 - Jp, Lc = nt - 1 - Ip;          // L's tile row and column
    double *dst = Mp + (size_t)(toffb[Jp] + (Ip - Jp)) * TILE * TILE;
    for (int e = threadIdx.x; e < TILE * TILE; e += 256) {
        const int c = e & (TILE - 1), r = e >> 7;           // (source rows run fastest)
        const double v = A[band_index(Lr * TILE + (TILE - 1 - c), Lc * TILE + (TILE - 1 - r), lda, skew, npad)];
        dst[(size_t)r + (size_t)c * TILE] = (Ip == Jp && r < c) ? 0.0 : v;
    }
}

// krige_band_qprep_kernel's arithmetic on the packed diagonal tiles of M (tile toffb[J'], ld 128)
__global__ void __launch_bounds__(256)
band_back_qprep_kernel(const double *Mp, const int *toffb, double *Qb)
{
    const int J = blockIdx.x, tid = threadIdx.x;
    const double *D = Mp + (size_t)toffb[J] * TILE * TILE;
    for (int e = tid; e < 8 * 256; e += 256) {
        const int jb = e >> 8, s = (e >> 6) & 3, lane = e & 63;
        const int m = lane & 15, k = lane >> 4, c = m & 3;
        double q = 0.0;
        if ((m >> 2) == s && k <= c) {
            const int d0 = 16 * jb + 4 * s;                                                // the 4 x 4 diagonal sub-block
            auto L = [&](int i, int j) { return D[(size_t)(d0 + i) + (size_t)(d0 + j) * TILE]; };
            const double l10 = L(1, 0), l20 = L(2, 0), l30 = L(3, 0), l21 = L(2, 1), l31 = L(3, 1), l32 = L(3, 2);
            const double r0 = 1.0 / L(0, 0), r1 = 1.0 / L(1, 1), r2 = 1.0 / L(2, 2), r3 = 1.0 / L(3, 3);
            const double m00 = r0, m11 = r1, m22 = r2, m33 = r3;
            const double m10 = -(l10 * m00) * r1;
            const double m21 = -(l21 * m11) * r2;
            const double m32 = -(l32 * m22) * r3;
            const double m20 = -fma(l21, m10, l20 * m00) * r2;
            const double m31 = -fma(l32, m21, l31 * m11) * r3;
            const double m30 = -fma(l32, m20, fma(l31, m10, l30 * m00)) * r3;
            q = sel_lower4(c, k, m00, m10, m11, m20, m21, m22, m30, m31, m32, m33);
        }
        Qb[(size_t)J * 2048 + e] = q;
    }
}

void launch_band_back_pack(const double *A, size_t lda, int skew, int npad, const int *d_hib, int nt, int W, const int *d_toffb,
                           double *Mp, double *Qb, hipStream_t s)
{
    if (nt <= 0 || W <= 0) return;
    hipLaunchKernelGGL(band_back_pack_kernel, dim3((unsigned)W, (unsigned)nt), dim3(256), 0, s, A, lda, skew, npad, d_hib, nt,
                       d_toffb, Mp);
    hipLaunchKernelGGL(band_back_qprep_kernel, dim3(nt), dim3(256), 0, s, Mp, d_toffb, Qb);
}

hipError_t launch_band_sweep(const BandSweep &a, hipStream_t s)
{
    if (a.rows <= 0 || a.nt <= 0) return hipSuccess;
    const unsigned strips = (unsigned)((a.rows + 63) / 64);
    for (int J = 0; J < a.nt; ++J) {
        const double *Lcol = a.Lp + (size_t)a.toff[J] * TILE * TILE;
        hipLaunchKernelGGL(krige_band_diag_kernel, dim3(strips), dim3(256), 0, s, Lcol, a.Qp + (size_t)J * 2048, a.zero,
                           a.C + (size_t)J * TILE * a.ldc, a.ldc, J == 0 ? 1 : 0, a.st, a.qd);
        const int hj = a.hi ? a.hi[J] : a.nt;
        if (hj - J - 1 > 0)
            hipLaunchKernelGGL(krige_band_update_kernel, dim3(strips, (unsigned)(hj - J - 1)), dim3(256), 0, s, Lcol, a.C, a.ldc, J,
                               a.nt);
    }
    return hipGetLastError();
}

__global__ void __launch_bounds__(256)
band_unit_rows_kernel(double *E, size_t lde, int npad, int g0, int count)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < count) E[(size_t)k + (size_t)(npad - 1 - (g0 + k)) * lde] = 1.0;
}

void launch_band_unit_rows(double *E, size_t lde, int npad, int g0, int count, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(band_unit_rows_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, E, lde, npad, g0, count);
}

__global__ void __launch_bounds__(256)
band_given_rows_kernel(double *E, size_t lde, int npad, const double *P, int n, const int *pos)
{
    const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (i < n) E[(size_t)k + (size_t)(npad - 1 - pos[i]) * lde] = P[(size_t)i + (size_t)k * n];
}

void launch_band_given_rows(double *E, size_t lde, int npad, const double *P, int n, const int *pos, int count, hipStream_t s)
{
    if (count <= 0 || n <= 0) return;
    hipLaunchKernelGGL(band_given_rows_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)count), dim3(256), 0, s, E, lde, npad,
                       P, n, pos);
}

__global__ void __launch_bounds__(256)
band_x_rows_kernel(double *U, size_t ldu, int row0, const double *X, int n, int p, int npad)
{
    const int r = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j < npad) U[(size_t)(row0 + r) + (size_t)j * ldu] = (r < p && j < n) ? X[(size_t)j + (size_t)r * n] : 0.0;
}

void launch_band_x_rows(double *U, size_t ldu, int row0, const double *X, int n, int p, int npad, hipStream_t s)
{
    hipLaunchKernelGGL(band_x_rows_kernel, dim3((unsigned)((npad + 3) / 4)), dim3(256), 0, s, U, ldu, row0, X, n, p, npad);
}

// One thread per (probe row k, site j): a wave shares j, so the pattern and the directions' entries are uniform loads and the
// gather of W is one coalesced 512-byte row segment per entry, shared by the group's accumulators.
constexpr int BAND_DG = 8;         // directions per register group (spmm) and per side of a group pair (gram)
__global__ void __launch_bounds__(256)
band_spmm_dirs_kernel(BandSpmm a)
{
    const int k = 64 * (int)blockIdx.y + (threadIdx.x & 63), j = 4 * (int)blockIdx.x + (threadIdx.x >> 6);
    if (j >= a.npad) return;
    const int t0 = j < a.n ? a.frp[j] : 0, t1 = j < a.n ? a.frp[j + 1] : 0;
    for (int g0 = 0; g0 < a.ndir; g0 += BAND_DG) {
        const int ng = a.ndir - g0 < BAND_DG ? a.ndir - g0 : BAND_DG;
        double acc[BAND_DG];
#pragma unroll
        for (int x = 0; x < BAND_DG; ++x) acc[x] = 0.0;
        for (int t = t0; t < t1; ++t) {
            const double wv = a.Wf[(size_t)k + (size_t)(a.npad - 1 - a.fci[t]) * a.ldw];
            const double *sd = a.Sd + (size_t)g0 * a.nnz + (size_t)a.fidx[t];
#pragma unroll
            for (int x = 0; x < BAND_DG; ++x)
                if (x < ng) acc[x] = fma(sd[(size_t)x * a.nnz], wv, acc[x]);
        }
#pragma unroll
        for (int x = 0; x < BAND_DG; ++x)
            if (x < ng) a.U[(size_t)(g0 + x) * a.bstride + (size_t)k + (size_t)j * a.ldu] = acc[x];
    }
}

void launch_band_spmm_dirs(const BandSpmm &a, hipStream_t s)
{
    if (a.rows <= 0 || a.npad <= 0 || a.ndir <= 0) return;
    hipLaunchKernelGGL(band_spmm_dirs_kernel, dim3((unsigned)((a.npad + 3) / 4), (unsigned)((a.rows + 63) / 64)), dim3(256), 0, s, a);
}

// grid (strips, segments, group pairs ga <= gb): the thread of row k and column class tid / 64 runs over its columns of the
// segment with BAND_DG x BAND_DG accumulators; then per accumulator a butterfly over the wave and the four waves in order
__global__ void __launch_bounds__(256)
band_gram_kernel(const double *Q, size_t ld, size_t base, size_t bstride, int nrows, int npad, int nd, int ngrp, double *seg)
{
    __shared__ double red[4][BAND_DG * BAND_DG];
    int ga = 0, gb = (int)blockIdx.z;
    while (gb >= ngrp - ga) { gb -= ngrp - ga; ++ga; }
    gb += ga;
    const int tid = threadIdx.x, k = tid & 63, wave = tid >> 6;
    const int c0 = (int)blockIdx.y * BAND_GRAM_SEG, c1 = c0 + BAND_GRAM_SEG < npad ? c0 + BAND_GRAM_SEG : npad;
    const int na = nd - ga * BAND_DG < BAND_DG ? nd - ga * BAND_DG : BAND_DG, nb = nd - gb * BAND_DG < BAND_DG ? nd - gb * BAND_DG : BAND_DG;
    const double *qa = Q + base + (size_t)(ga * BAND_DG) * bstride + 64 * (size_t)blockIdx.x + k;
    const double *qb = Q + base + (size_t)(gb * BAND_DG) * bstride + 64 * (size_t)blockIdx.x + k;
    double acc[BAND_DG][BAND_DG];
#pragma unroll
    for (int x = 0; x < BAND_DG; ++x)
#pragma unroll
        for (int y = 0; y < BAND_DG; ++y) acc[x][y] = 0.0;
    if (k < nrows)
        for (int c = c0 + wave; c < c1; c += 4) {
            double va[BAND_DG], vb[BAND_DG];
#pragma unroll
            for (int x = 0; x < BAND_DG; ++x) {
                va[x] = x < na ? qa[(size_t)x * bstride + (size_t)c * ld] : 0.0;
                vb[x] = x < nb ? qb[(size_t)x * bstride + (size_t)c * ld] : 0.0;
            }
#pragma unroll
            for (int x = 0; x < BAND_DG; ++x)
#pragma unroll
                for (int y = 0; y < BAND_DG; ++y) acc[x][y] = fma(va[x], vb[y], acc[x][y]);
        }
#pragma unroll
    for (int x = 0; x < BAND_DG; ++x)
#pragma unroll
        for (int y = 0; y < BAND_DG; ++y) {
            double v = acc[x][y];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (k == 0) red[wave][x * BAND_DG + y] = v;
        }
    __syncthreads();
    if (tid < BAND_DG * BAND_DG) {
        const int a = ga * BAND_DG + tid / BAND_DG, b = gb * BAND_DG + tid % BAND_DG;
        if (a < nd && b < nd && a <= b)
            seg[(((size_t)blockIdx.x * gridDim.y + blockIdx.y) * nd + a) * nd + b] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
}

// part[(strip0 + s) nd nd + e] = sum over the segments, in index order (entries a <= b; the others stay 0)
__global__ void __launch_bounds__(256)
band_gram_seg_kernel(const double *seg, int nseg, int nd, double *part, int strip0)
{
    const int e = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (e >= nd * nd) return;
    double t = 0.0;
    if (e / nd <= e % nd)
        for (int g = 0; g < nseg; ++g) t += seg[((size_t)s * nseg + g) * nd * nd + e];
    part[(size_t)(strip0 + s) * nd * nd + e] = t;
}

__global__ void __launch_bounds__(256)
band_gram_sum_kernel(const double *part, int nstrips, int nd, double weight, double *out)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nd * nd) return;
    const int a = e / nd, b = e % nd;
    if (a > b) return;
    double t = 0.0;
    for (int s = 0; s < nstrips; ++s) t += part[(size_t)s * nd * nd + e];
    out[a * nd + b] = weight * t;
    out[b * nd + a] = weight * t;
}

static inline int band_gram_segments(int npad) { return (npad + BAND_GRAM_SEG - 1) / BAND_GRAM_SEG; }
size_t band_gram_scratch_doubles(int nstrips, int npad, int nd) { return (size_t)nstrips * band_gram_segments(npad) * nd * nd; }

void launch_band_gram(const double *Q, size_t ld, size_t base, size_t bstride, int nrows, int nstrips, int npad, int nd,
                      double *seg, double *part, int strip0, hipStream_t s)
{
    if (nstrips <= 0 || nd <= 0) return;
    const int ngrp = (nd + BAND_DG - 1) / BAND_DG, nseg = band_gram_segments(npad);
    hipLaunchKernelGGL(band_gram_kernel, dim3((unsigned)nstrips, (unsigned)nseg, (unsigned)(ngrp * (ngrp + 1) / 2)), dim3(256), 0, s,
                       Q, ld, base, bstride, nrows, npad, nd, ngrp, seg);
    hipLaunchKernelGGL(band_gram_seg_kernel, dim3((unsigned)((nd * nd + 255) / 256), (unsigned)nstrips), dim3(256), 0, s, seg, nseg,
                       nd, part, strip0);
}

void launch_band_gram_sum(const double *part, int nstrips, int nd, double weight, double *out, hipStream_t s)
{
    if (nd <= 0) return;
    hipLaunchKernelGGL(band_gram_sum_kernel, dim3((unsigned)((nd * nd + 255) / 256)), dim3(256), 0, s, part, nstrips, nd, weight, out);
}

}  // namespace cocons
