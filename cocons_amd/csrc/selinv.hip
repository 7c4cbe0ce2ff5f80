// selinv.hip -- selected inverse of a tapered covariance on the tile envelope of its band factor (gfx950, fp64 MFMA).
//
// A taper handle's factor L (S = L L') lives in tiles of 128 x 128 inside the monotone envelope hi[c] (one past the last tile
// row of tile column c; null: hi[c] = nt), in the packed band layout or the dense one (kernels.h band_index).  From
// S^-1 L = L^-T, sweeping the tile columns J = nt-1 .. 0 with G_KJ = L_KJ L_JJ^-1 (J < K < hi[J]):
//     Z_IJ = - sum_K Z_IK G_KJ                       (J < I < hi[J]; Z_IK = Z_KI' where K > I)
//     Z_JJ = L_JJ^-T L_JJ^-1 - sum_K Z_KJ' G_KJ
//     a_J  = L_JJ^-T y_J - sum_K G_KJ' a_K            (A = L^-T (L^-1 R): the rows under the factor hold y = (L^-1 R)')
// gives Z = S^-1 exactly on every envelope tile: every Z_IK on the right lies inside the envelope because it is monotone.
//
//   selinv_tri_kernel  : L_JJ <- L_JJ^-1 for every tile column at once (forward substitution per column in LDS)
//   selinv_g_kernel    : L_KJ <- G_KJ for every envelope tile at once (in place: a wave owns whole rows of its tile)
//   selinv_col_kernel  : step J, the b = hi[J] - J - 1 tiles Z_IJ: one wave per 32 x 32 block over the whole sum
//   selinv_diag_kernel : step J, Z_JJ (one wave per 16 x 16 block) and a_J (one wave per four columns)
// Z goes to a second buffer of the band's shape; L is consumed (every operation on the handle assembles its matrix anew).
// Two launches per tile column; every sum has a fixed order and nothing is accumulated atomically: repeated calls agree
// bit for bit.  Blocks are held in the factorisation's register layout (tile_ops.hpp: reg r of lane l <-> (row l & 15,
// column 4 r + (l >> 4))), in which blk_mma(acc, P, Q) is acc(i, j) += sum_k P(i, k) Q(j, k).
#include <hip/hip_runtime.h>
#include <atomic>
#include "kernels.h"
#include "tile_ops.hpp"

namespace cocons {

namespace {

// B(row, col) = T[r0 + col, c0 + row]: the transpose of the 16 x 16 block at (r0, c0)
__device__ __forceinline__ d4 blk_ld_t(const double *T, size_t ld, int r0, int c0, int lane)
{
    const double *p = T + (size_t)(r0 + (lane >> 4)) + (size_t)(c0 + (lane & 15)) * ld;
    d4 v;
    v[0] = p[0]; v[1] = p[4]; v[2] = p[8]; v[3] = p[12];
    return v;
}

__device__ __forceinline__ size_t tile_off(int I, int J, size_t ld, int skew, int npad)
{
    return band_index(I * TILE, J * TILE, ld, skew, npad);
}

__device__ __forceinline__ double wave_sum64(double v)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace

// L_JJ^-1 over L_JJ (full tile: zeros above the diagonal).  Thread j solves L x = e_j by forward substitution; its column
// of X sits in LDS (X(k, j) at k * 128 + j), the entries of L are the same for every lane.
__global__ void __launch_bounds__(128)
selinv_tri_kernel(SelinvArgs a)
{
    extern __shared__ double xs[];
    const int J = blockIdx.x, j = threadIdx.x;
    double *T = a.L + tile_off(J, J, a.ldl, a.skew, a.npad);
    const size_t ld = a.ldl;
    for (int k = 0; k < TILE; ++k) xs[k * TILE + j] = 0.0;
    const int w0 = __builtin_amdgcn_readfirstlane((j >> 6) * 64);      // columns from 64 on have nothing above row 64
    for (int i = w0; i < TILE; ++i) {
        double s = (i == j) ? 1.0 : 0.0;
        for (int k = w0; k < i; ++k) s -= T[(size_t)i + (size_t)k * ld] * xs[k * TILE + j];
        xs[i * TILE + j] = s / T[(size_t)i + (size_t)i * ld];
    }
    __syncthreads();
    for (int c = 0; c < TILE; ++c) T[(size_t)j + (size_t)c * ld] = xs[j * TILE + c];
}

// G_KJ = L_KJ L_JJ^-1 over L_KJ, K = J + 1 + blockIdx.x < hi[J].  Wave w: rows [32 w, 32 w + 32) of the tile, all columns;
// it has read those rows in full before it stores them.
__global__ void __launch_bounds__(256)
selinv_g_kernel(SelinvArgs a)
{
    const int J = blockIdx.y, K = J + 1 + blockIdx.x;
    const int hi = a.d_hi ? a.d_hi[J] : a.nt;
    if (K >= hi) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t ld = a.ldl;
    double *X = a.L + tile_off(K, J, ld, a.skew, a.npad);
    const double *W = a.L + tile_off(J, J, ld, a.skew, a.npad);
    const int r0 = 32 * wave;
    d4 acc[2][8];
    for (int rb = 0; rb < 2; ++rb)
        for (int cb = 0; cb < 8; ++cb) acc[rb][cb] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int kb = 0; kb < 8; ++kb) {
        const d4 P0 = glb_blk(X, ld, r0, kb * 16, lane), P1 = glb_blk(X, ld, r0 + 16, kb * 16, lane);
#pragma unroll
        for (int cb = 0; cb < 8; ++cb) {
            if (cb > kb) continue;                 // W is lower triangular: W(k, j) = 0 for k < j
            const d4 Q = blk_ld_t(W, ld, kb * 16, cb * 16, lane);      // Q(j, k) = W(k, j)
            blk_mma(acc[0][cb], P0, Q);
            blk_mma(acc[1][cb], P1, Q);
        }
    }
    for (int rb = 0; rb < 2; ++rb)
        for (int cb = 0; cb < 8; ++cb) glb_blk_store(X, ld, r0 + 16 * rb, cb * 16, lane, acc[rb][cb]);
}

// Step J: Z_IJ = - sum_{J < K < hi} Zop(I, K) G_KJ for I = J + 1 + blockIdx.y.  blockIdx.x: the 64 x 64 quadrant of the
// tile, wave w its 32 x 32 block.  Zop(I, K) is tile (I, K) as stored for I >= K (diagonal tiles are stored in full) and the
// transpose of tile (K, I) for I < K.
__global__ void __launch_bounds__(256)
selinv_col_kernel(SelinvArgs a, int J, int hi)
{
    const int I = J + 1 + blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ro = 64 * (blockIdx.x & 1) + 32 * (wave & 1), co = 64 * (blockIdx.x >> 1) + 32 * (wave >> 1);
    d4 acc[2][2];
    for (int rb = 0; rb < 2; ++rb)
        for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int K = J + 1; K < hi; ++K) {
        const double *G = a.L + tile_off(K, J, a.ldl, a.skew, a.npad);
        const bool straight = I >= K;
        const double *Zt = a.Z + (straight ? tile_off(I, K, a.ldz, a.skew, a.npad) : tile_off(K, I, a.ldz, a.skew, a.npad));
#pragma unroll 2
        for (int kb = 0; kb < 8; ++kb) {
            d4 P[2], Q[2];
            for (int rb = 0; rb < 2; ++rb)
                P[rb] = straight ? glb_blk(Zt, a.ldz, ro + 16 * rb, kb * 16, lane) : blk_ld_t(Zt, a.ldz, kb * 16, ro + 16 * rb, lane);
            for (int cb = 0; cb < 2; ++cb) Q[cb] = blk_ld_t(G, a.ldl, kb * 16, co + 16 * cb, lane);
            for (int rb = 0; rb < 2; ++rb)
                for (int cb = 0; cb < 2; ++cb) blk_mma(acc[rb][cb], P[rb], Q[cb]);
        }
    }
    double *O = a.Z + tile_off(I, J, a.ldz, a.skew, a.npad);
    for (int rb = 0; rb < 2; ++rb)
        for (int cb = 0; cb < 2; ++cb) glb_blk_store(O, a.ldz, ro + 16 * rb, co + 16 * cb, lane, -acc[rb][cb]);
}

// Step J, behind selinv_col_kernel.  Workgroups 0 .. 15: Z_JJ = W' W - sum_K Z_KJ' G_KJ (W = L_JJ^-1), one wave per
// 16 x 16 block of the lower triangle.  Workgroups 16 .. 23: a_J = W' y_J - sum_K G_KJ' a_K for the nr right-hand sides, one wave per four
// columns of the tile, lanes along the rows.
constexpr int SELINV_DIAG_WG = 16, SELINV_SUB_WG = 8;
__global__ void __launch_bounds__(256)
selinv_diag_kernel(SelinvArgs a, int J, int hi)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *W = a.L + tile_off(J, J, a.ldl, a.skew, a.npad);
    if ((int)blockIdx.x < SELINV_DIAG_WG) {
        // Only the blocks on and below the diagonal are computed; each is the mean of the two mirrored forms of the sum (in
        // exact arithmetic equal) and is stored to both sides, the diagonal blocks mirrored through LDS: Z_JJ is symmetric
        // to the bit.  An antisymmetric part, however small, is a growing mode of the sweep.
        __shared__ double tb[4][256];
        const int wb = blockIdx.x * 4 + wave, rb = wb & 7, cb = wb >> 3;
        if (rb < cb) return;
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0}, sub = (d4){0.0, 0.0, 0.0, 0.0}, sub2 = (d4){0.0, 0.0, 0.0, 0.0};
        for (int kb = rb; kb < 8; ++kb)
            blk_mma(acc, blk_ld_t(W, a.ldl, kb * 16, rb * 16, lane), blk_ld_t(W, a.ldl, kb * 16, cb * 16, lane));
        for (int K = J + 1; K < hi; ++K) {
            const double *G = a.L + tile_off(K, J, a.ldl, a.skew, a.npad);
            const double *Zt = a.Z + tile_off(K, J, a.ldz, a.skew, a.npad);
#pragma unroll 2
            for (int kb = 0; kb < 8; ++kb) {
                const d4 zr = blk_ld_t(Zt, a.ldz, kb * 16, rb * 16, lane), gc = blk_ld_t(G, a.ldl, kb * 16, cb * 16, lane);
                const d4 gr = blk_ld_t(G, a.ldl, kb * 16, rb * 16, lane), zc = blk_ld_t(Zt, a.ldz, kb * 16, cb * 16, lane);
                blk_mma(sub, zr, gc);            // (Z_KJ' G_KJ)(i, j)
                blk_mma(sub2, gr, zc);           // (G_KJ' Z_KJ)(i, j) = (Z_KJ' G_KJ)(j, i)
            }
        }
        d4 out = acc - 0.5 * (sub + sub2);
        double *O = a.Z + tile_off(J, J, a.ldz, a.skew, a.npad);
        if (rb == cb) {
            volatile double *t = tb[wave];
            for (int r = 0; r < 4; ++r) t[(lane & 15) + 16 * (4 * r + (lane >> 4))] = out[r];
            __builtin_amdgcn_wave_barrier();
            for (int r = 0; r < 4; ++r) {
                const int row = lane & 15, col = 4 * r + (lane >> 4);
                if (row < col) out[r] = t[col + 16 * row];
            }
            glb_blk_store(O, a.ldz, rb * 16, cb * 16, lane, out);
        } else {
            glb_blk_store(O, a.ldz, rb * 16, cb * 16, lane, out);
            double *q = O + (size_t)(cb * 16 + (lane >> 4)) + (size_t)(rb * 16 + (lane & 15)) * a.ldz;      // the transpose
            q[0] = out[0]; q[4] = out[1]; q[8] = out[2]; q[12] = out[3];
        }
        return;
    }
    if (a.nr <= 0) return;
    const int t0 = (((int)blockIdx.x - SELINV_DIAG_WG) * 4 + wave) * 4;
    for (int c0 = 0; c0 < a.nr; c0 += 4) {
        const int nc = a.nr - c0 < 4 ? a.nr - c0 : 4;
        for (int tt = 0; tt < 4; ++tt) {
            const int t = t0 + tt;
            double s[4] = {0.0, 0.0, 0.0, 0.0};
            for (int h = 0; h < 2; ++h) {
                const int i = 64 * h + lane;
                const double w = W[(size_t)i + (size_t)t * a.ldl];
                for (int c = 0; c < nc; ++c)
                    s[c] += w * a.L[band_index(a.npad + c0 + c, J * TILE + i, a.ldl, a.skew, a.npad)];
            }
            for (int K = J + 1; K < hi; ++K) {
                const double *G = a.L + tile_off(K, J, a.ldl, a.skew, a.npad);
                for (int h = 0; h < 2; ++h) {
                    const int i = 64 * h + lane;
                    const double g = G[(size_t)i + (size_t)t * a.ldl];
                    for (int c = 0; c < nc; ++c) s[c] -= g * a.AR[(size_t)(K * TILE + i) + (size_t)(c0 + c) * a.npad];
                }
            }
            for (int c = 0; c < nc; ++c) {
                const double v = wave_sum64(s[c]);
                if (lane == 0) a.AR[(size_t)(J * TILE + t) + (size_t)(c0 + c) * a.npad] = v;
            }
        }
    }
}

// out[w] = Z(max(i, j), min(i, j)) for the 0-based pairs ij[2 w], ij[2 w + 1]
__global__ void __launch_bounds__(256)
selinv_gather_kernel(const double *Z, size_t ldz, int skew, int npad, const int *ij, size_t count, double *out)
{
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= count) return;
    const int i = ij[2 * w], j = ij[2 * w + 1];
    out[w] = Z[band_index(i > j ? i : j, i > j ? j : i, ldz, skew, npad)];
}

void launch_selinv(const SelinvArgs &a, const int *h_hi, int maxband, hipStream_t s)
{
    const size_t shm = (size_t)TILE * TILE * sizeof(double);      // 128 KB of dynamic LDS (> the 64 KB default)
    static std::atomic<unsigned long long> attr_done{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!(dev >= 0 && dev < 64 && ((attr_done.load(std::memory_order_relaxed) >> dev) & 1ull))) {
        (void)hipFuncSetAttribute((const void *)selinv_tri_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        if (dev >= 0 && dev < 64) attr_done.fetch_or(1ull << dev, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(selinv_tri_kernel, dim3(a.nt), dim3(128), shm, s, a);
    if (maxband > 1) hipLaunchKernelGGL(selinv_g_kernel, dim3(maxband - 1, a.nt), dim3(256), 0, s, a);
    for (int J = a.nt - 1; J >= 0; --J) {
        const int hi = h_hi ? h_hi[J] : a.nt;
        if (hi - J - 1 > 0) hipLaunchKernelGGL(selinv_col_kernel, dim3(4, hi - J - 1), dim3(256), 0, s, a, J, hi);
        hipLaunchKernelGGL(selinv_diag_kernel, dim3(SELINV_DIAG_WG + SELINV_SUB_WG), dim3(256), 0, s, a, J, hi);
    }
}

void launch_selinv_gather(const double *Z, size_t ldz, int skew, int npad, const int *ij, size_t count, double *out, hipStream_t s)
{
    if (count == 0) return;
    hipLaunchKernelGGL(selinv_gather_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, Z, ldz, skew, npad, ij, count, out);
}

}  // namespace cocons
