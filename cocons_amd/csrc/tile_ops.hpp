// tile_ops.hpp -- the 16 x 16 fp64 block primitives of the device code (gfx950, v_mfma_f64_16x16x4_f64): shared by the
// factorisation (chol.hip), the kernels that read a finished factor (solve.hip) and the selected inverse (selinv.hip).
// Device-only: include it from a .hip source, behind kernels.h.
//
// All matrix products run on v_mfma_f64_16x16x4_f64.  A 16x16 block lives in four
// f64 registers per lane in "blk layout":
//      reg r of lane l  <->  element (row = l & 15, col = 4 r + (l >> 4)).
// With the matrix ROW on the lane (contiguous in memory) this layout is at once
//   * the C/D accumulator layout of D[m][n] with n <-> row, m <-> col, and
//   * the A- or B-operand layout for k-step r,
// so a product's result feeds the next product without any data movement:
//      blk_mma(acc, P, Q):  acc(i,j) += sum_k P(i,k) Q(j,k).
#pragma once
#include <hip/hip_runtime.h>

namespace cocons {

typedef double d4 __attribute__((ext_vector_type(4)));

#define MFMA64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
// the same with the first operand negated: for the fp64 forms the instruction's blgp field holds NEG bits
// (neg:[a,b,c]; bit 0 = first source), so D = C - A B costs no extra instruction
#define MFMA64_NEGA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 1)

__device__ __forceinline__ void blk_mma(d4 &acc, const d4 &P, const d4 &Q)
{
    acc = MFMA64(Q[0], P[0], acc);
    acc = MFMA64(Q[1], P[1], acc);
    acc = MFMA64(Q[2], P[2], acc);
    acc = MFMA64(Q[3], P[3], acc);
}

// block-packed LDS image: 16x16 blocks of 256 doubles, element (i,k) at k*16 + i
__device__ __forceinline__ d4 lds_blk(const double *blk, int lane)
{
    d4 v;
    int o = (lane >> 4) * 16 + (lane & 15);
    v[0] = blk[o];
    v[1] = blk[o + 64];
    v[2] = blk[o + 128];
    v[3] = blk[o + 192];
    return v;
}

__device__ __forceinline__ void lds_blk_store(double *blk, int lane, const d4 &v)
{
    int o = (lane >> 4) * 16 + (lane & 15);
    blk[o] = v[0];
    blk[o + 64] = v[1];
    blk[o + 128] = v[2];
    blk[o + 192] = v[3];
}

__device__ __forceinline__ d4 glb_blk(const double *A, size_t lda, int row0, int col0, int lane)
{
    const double *p = A + (size_t)(row0 + (lane & 15)) + (size_t)(col0 + (lane >> 4)) * lda;
    d4 v;
    v[0] = p[0];
    v[1] = p[4 * lda];
    v[2] = p[8 * lda];
    v[3] = p[12 * lda];
    return v;
}

__device__ __forceinline__ void glb_blk_store(double *A, size_t lda, int row0, int col0, int lane, const d4 &v)
{
    double *p = A + (size_t)(row0 + (lane & 15)) + (size_t)(col0 + (lane >> 4)) * lda;
    p[0] = v[0];
    p[4 * lda] = v[1];
    p[8 * lda] = v[2];
    p[12 * lda] = v[3];
}

// L1-bypassing (sc1) load of data another workgroup published with store_wt: with EVERY load of the
// handed-off bytes of this form the consumer needs no acquire fence (buffer_inv).  (store_wt and the hand-offs live in
// chol.hip; this one is here because fetch_factor_tile<WT> names it.)
__device__ __forceinline__ double load_wt(const double *p)
{
    return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
}

// ---------------------------------------------------------------------------
// 16x16 diagonal block on ONE wave, all in registers (blk layout), MFMA-based:
//   for each 4-column group s: broadcast the 4x4 diagonal sub-block (v_readlane), factor
//   and invert it redundantly on every lane (10 + 10 values), then
//     one MFMA  : columns 4s..4s+3  <-  D(:, group s) * inv(L4)^T        (K = 4)
//     one MFMA  : rank-4 update of the whole 16x16 block
// Outputs: the factor L (blk layout) and Q[s] = per-lane MFMA A-operand of inv(L4_s)
// (row m = lane&15, k = lane>>4; zero outside rows 4s..4s+3), which trsm16() reuses.
__device__ __forceinline__ double rdlane(double v, int lane)
{
    int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// l = sqrt(a), r = 1/sqrt(a) for a normal positive a (pivots of an SPD matrix); both to about 1 ulp.  v_rsq_f64 delivers
// 24 bits (measured: tools/diag/seed_precision.hip, max relative error 2^-24.2), so ONE third-order step
//     y = y0 (1 + t/2 + 3 t^2/8),   t = 1 - a y0^2        (truncation 5/16 t^3 < 2^-70)
// gives r after four dependent operations -- r is what the pivot chain of potrf16_step waits for -- and l = a y with one
// Heron correction follows off the chain.  (Rounds 1-2 ran two Newton steps and two corrections: r came out last, after
// eleven dependent operations, sixteen times per 16 x 16 block on the one wave every diagonal tile waits for.)
__device__ __forceinline__ void rsqrt_pivot(double a, double &l, double &r)
{
    const double y0 = __builtin_amdgcn_rsq(a);
    const double s0 = a * y0;
    const double t = fma(-s0, y0, 1.0);
    const double y = fma(y0 * t, fma(t, 0.375, 0.5), y0);
    double s = a * y;
    s = fma(fma(-s, s, a), 0.5 * y, s);      // s + (a - s^2) / (2 s)
    // A pivot that is not a positive finite number comes out as NaN in both results WITHOUT being asked (like sqrt would):
    // v_rsq_f64 gives NaN for a < 0, +-inf for +-0 (then a y0 = 0 inf = NaN) and 0 for +inf (inf 0 = NaN).  Rounds 1-3
    // selected NaN explicitly: eight v_cndmask per pivot on the one wave every diagonal tile waits for.
    l = s;
    r = y;
}

// select among the lower-triangular 4x4 values by (c = row in group, k = column)
__device__ __forceinline__ double sel_lower4(int c, int k, double v00, double v10, double v11, double v20,
                                             double v21, double v22, double v30, double v31, double v32, double v33)
{
    double r0 = v00;                                   // c == 0 (k == 0)
    double r1 = (k == 0) ? v10 : v11;                  // c == 1
    double r2 = (k == 0) ? v20 : ((k == 1) ? v21 : v22);
    double r3 = (k == 0) ? v30 : ((k == 1) ? v31 : ((k == 2) ? v32 : v33));
    double r = (c == 0) ? r0 : ((c == 1) ? r1 : ((c == 2) ? r2 : r3));
    return (k <= c) ? r : 0.0;
}

template <int S>
__device__ __forceinline__ void potrf16_step(d4 &D, double (&Q)[4], int lane, int &fail)
{
    const int m = lane & 15, k = lane >> 4;
    const double ds = D[S];
    // element (4S+a, 4S+b) sits on lane (4S+a) + 16 b of register S
    double a00 = rdlane(ds, 4 * S + 0), a10 = rdlane(ds, 4 * S + 1), a20 = rdlane(ds, 4 * S + 2),
           a30 = rdlane(ds, 4 * S + 3);
    double a11 = rdlane(ds, 4 * S + 1 + 16), a21 = rdlane(ds, 4 * S + 2 + 16), a31 = rdlane(ds, 4 * S + 3 + 16);
    double a22 = rdlane(ds, 4 * S + 2 + 32), a32 = rdlane(ds, 4 * S + 3 + 32);
    double a33 = rdlane(ds, 4 * S + 3 + 48);
    // 4x4 Cholesky (dpotf2 order) -- identical on every lane.  Pivots through
    // rsqrt_pivot(): l = sqrt(a) and r = 1/l from one v_rsq_f64 seed (short dependent chain;
    // this loop is pure latency).
    double l00, r0;
    rsqrt_pivot(a00, l00, r0);
    double l10 = a10 * r0, l20 = a20 * r0, l30 = a30 * r0;
    double t11 = fma(-l10, l10, a11);
    double l11, r1;
    rsqrt_pivot(t11, l11, r1);
    double l21 = fma(-l20, l10, a21) * r1, l31 = fma(-l30, l10, a31) * r1;
    double t22 = fma(-l21, l21, fma(-l20, l20, a22));
    double l22, r2;
    rsqrt_pivot(t22, l22, r2);
    double l32 = fma(-l31, l21, fma(-l30, l20, a32)) * r2;
    double t33 = fma(-l32, l32, fma(-l31, l31, fma(-l30, l30, a33)));
    double l33, r3;
    rsqrt_pivot(t33, l33, r3);
    // which pivot failed first is asked ONCE per group, behind the chain, and only looked into when the last pivot is not
    // a positive number -- a bad pivot makes every later one NaN (the values are the same on every lane: a scalar branch)
    if (__builtin_amdgcn_ballot_w64(!(t33 > 0.0)) != 0ull && fail == 0)
        fail = 4 * S + (!(a00 > 0.0) ? 1 : (!(t11 > 0.0) ? 2 : (!(t22 > 0.0) ? 3 : 4)));
    // (An outer-product form with reciprocals on the dependent chain and the square roots refined beside it -- 3 x 6 + 12
    // dependent operations instead of 4 x 14 -- was measured in round 3: SLOWER, 4.54 -> 4.72 ms on the taper path, whose
    // time is half tile factorisations: one wave issues in order, and the variant has a quarter more instructions.)
    // inverse of the 4x4 factor
    double m00 = r0, m11 = r1, m22 = r2, m33 = r3;
    double m10 = -(l10 * m00) * r1;
    double m21 = -(l21 * m11) * r2;
    double m32 = -(l32 * m22) * r3;
    double m20 = -fma(l21, m10, l20 * m00) * r2;
    double m31 = -fma(l32, m21, l31 * m11) * r3;
    double m30 = -fma(l32, m20, fma(l31, m10, l30 * m00)) * r3;
    const int c = m & 3;
    const bool ingrp = (m >> 2) == S;
    double q = sel_lower4(c, k, m00, m10, m11, m20, m21, m22, m30, m31, m32, m33);
    q = ingrp ? q : 0.0;
    Q[S] = q;
    // columns of group S:  X = D(:, group S) * inv(L4)^T -- the rows of the diagonal sub-block too (D4 inv(L4)^T = L4: the
    // block arrives SYMMETRIC, potrf_tile_body mirrors the diagonal blocks when it loads the tile and every update keeps
    // them so), with exact zeros above the diagonal.  (Until round 4 those sixteen entries were selected from the scalar
    // factor: a second ten-way select, twenty v_cndmask per group on the wave every diagonal tile waits for.)
    d4 z = {0.0, 0.0, 0.0, 0.0};
    d4 X = MFMA64(q, ds, z);
    (void)l11; (void)l22; (void)l33; (void)l00;
    double xs = (m < 4 * S + k) ? 0.0 : X[S];
    // rank-4 update of the remaining columns (registers r > S)
    if (S < 3) {
        d4 U = MFMA64(xs, -xs, D);
#pragma unroll
        for (int r = S + 1; r < 4; ++r) D[r] = U[r];
    }
    D[S] = xs;
}

__device__ __forceinline__ int potrf16_regs(d4 &D, double (&Q)[4], int lane)
{
    int fail = 0;
    potrf16_step<0>(D, Q, lane, fail);
    potrf16_step<1>(D, Q, lane, fail);
    potrf16_step<2>(D, Q, lane, fail);
    potrf16_step<3>(D, Q, lane, fail);
    return fail;
}

// X = B * L^-T for a 16x16 lower block L (blk layout) with the 4x4 inverse operands Q:
// block forward substitution over the four column groups, 7 MFMAs.
__device__ __forceinline__ void trsm16(d4 &B, const d4 &L, const double (&Q)[4])
{
    const d4 z = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        d4 T = MFMA64(Q[s], B[s], z);
        B[s] = T[s];
        if (s < 3) {
            d4 U = MFMA64(L[s], -B[s], B);
#pragma unroll
            for (int r = s + 1; r < 4; ++r) B[r] = U[r];
        }
    }
}

// The 36 lower blocks of the factored diagonal tile at (c0, c0) and its Q operands into LDS (256 threads): EVERY global load is
// issued before the first LDS store -- one round trip.  (Until round 5 the panel kernels fetched block by block, a load and a
// store at a time: 36 dependent round trips, ~10 of the 14.6 us a panel solve took whatever its number of rows; the kernel
// trace of the tail at n = 4096, tools/r5_tail_timeline.sh.)
// WT: the tile comes from the engine inside this launch's lifetime (write-through stores there): L1-bypassing loads here, and the
// wait in front needs no acquire (the hand-off protocol above potrf_engine_kernel; an acquire is ~1.7 us, three per panel launch)
template <bool WT>
__device__ __forceinline__ void fetch_factor_tile(const double *A, size_t lda, int c0, const double *qin, double *SL, double *QS, int tid)
{
    const int i = tid & 15, k = tid >> 4;
    const double *src = A + (size_t)(c0 + i) + (size_t)(c0 + k) * lda;
    double v[36], q[8];
    {
        int b = 0;
#pragma unroll
        for (int ib = 0; ib < 8; ++ib)
#pragma unroll
            for (int kb = 0; kb <= ib; ++kb, ++b) {
                const double *sp = src + (size_t)(16 * ib) + (size_t)(16 * kb) * lda;
                v[b] = WT ? load_wt(sp) : *sp;
            }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = WT ? load_wt(qin + tid + 256 * e) : qin[tid + 256 * e];
#pragma unroll
    for (int b = 0; b < 36; ++b) SL[b * 256 + k * 16 + i] = v[b];
#pragma unroll
    for (int e = 0; e < 8; ++e) QS[tid + 256 * e] = q[e];
}

}  // namespace cocons
