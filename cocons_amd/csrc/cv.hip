// cv.hip -- cross-validated predictions from the inverse covariance.
//
// With K = Sigma^-1 and U = K R, a held-out set B predicts as  R_B - E[R_B | R_A] = (K_BB)^-1 U_B  with covariance (K_BB)^-1.
// The gradient's factorisation leaves -K in the lower triangle of the leading square and U in a buffer of its own; the kernels
// here read them and write results in the handle's internal order:
//   cv_loo_kernel     one observation per thread: var = 1 / K_ii, resid = U_i var
//   cv_fold_kernel    one workgroup per fold of 2 .. 128 observations, the block in LDS: gather, C C' = K_BB, W = C^-1
//                     (its transpose into the upper triangle the factor does not use), var_i = sum_j W_ji^2,
//                     resid = W' (W U_B) -- every sum in a fixed order, no atomics
//   cv_gather_kernel  a larger fold's bordered matrix [K_BB ; U_B' ; I] for the library's own factorisation
//   cv_scatter_kernel its results back to the observations' positions
//   cv_taper_kernel   leave-one-out from the diagonal of the selected inverse (taper handles), all observations or a list
//   cv_border_kernel  a larger fold's bordered matrix without its top block [0 (+ I on the padding) ; U_B' ; I]: the Gram
//                     product of cocons_cv_taper_folds adds K_BB = V V' into the top (solve.hip krige_band_gram_kernel)
// Taper handles by folds: cv_fold_kernel reads a fold's K_BB from a block of its own (base, + sign) instead of -S.
// The only atomic is the record of a failing fold (atomicMin of its label, as the factorisation's info word).
#include "kernels.h"
#include "cv_fold_tail.hpp"
#include <atomic>

namespace cocons {

__global__ void __launch_bounds__(256)
cv_loo_kernel(const double *S, size_t lds, const double *U, size_t ldu, int nr, const int *idx, const int *lab, int first,
              int count, double *var, double *res, size_t ldr, int *fail)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int i = idx ? idx[t] : first + t;
    const double k = -S[(size_t)i + (size_t)i * lds];
    if (!(k > 0.0) || !isfinite(k)) atomicMin(fail, lab ? lab[t] : t);
    const double v = 1.0 / k;
    var[i] = v;
    for (int c = 0; c < nr; ++c) res[(size_t)i + (size_t)c * ldr] = U[(size_t)i + (size_t)c * ldu] * v;
}

void launch_cv_loo(const double *S, size_t lds, const double *U, size_t ldu, int nr, const int *idx, const int *lab, int first,
                   int count, double *var, double *res, size_t ldr, int *fail, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(cv_loo_kernel, dim3((count + 255) / 256), dim3(256), 0, s, S, lds, U, ldu, nr, idx, lab, first, count, var,
                       res, ldr, fail);
}

// One workgroup of 256 threads per fold; BP = 16, 32, 64, 128 sizes the LDS (the arithmetic runs over the fold's own b and
// does not depend on BP).  LDS: the block with an odd leading dimension BP + 1 (rows and columns both without bank conflicts),
// the inverse pivots, and G = 256 / BP right-hand sides and intermediate vectors at a time.
//   lower triangle  K_BB, then its factor C (the diagonal is not stored: dinv = 1 / C_jj)
//   upper triangle  W' = C^-T: W(k, j), k > j, at (j, k); thread j forms column j of W by forward substitution and reads and
//                   writes row j of the upper triangle only, so the inversion needs no barrier
struct CvFoldArgs {
    const double *S; size_t lds;
    const double *U; size_t ldu; int nr;
    const int *idx, *off, *flist, *lab;
    double *var, *res; size_t ldr;
    int *fail;
    const long long *base;      // non-null: K_BB of fold f is the b x b block at S + base[f], ld lds (lower triangle), as it is
};

template <int BP> __global__ void __launch_bounds__(256)
cv_fold_kernel(CvFoldArgs a)
{
    extern __shared__ double cv_lds[];
    constexpr int LD = BP + 1;
    double *M = cv_lds, *dinv = M + (size_t)LD * BP, *ub = dinv + BP, *yb = ub + 256;
    const int f = a.flist[blockIdx.x];
    const int *pos = a.idx + a.off[f];
    const int b = a.off[f + 1] - a.off[f];
    const int tid = threadIdx.x;
    if (b < 1 || b > BP) return;                       // (the host's size classes: never)
    // gather: K(i, j) = -S(max, min); positions ascend inside a fold, so row >= column is the stored triangle
    for (int e = tid; e < b * b; e += 256) {
        const int rr = e % b, cc = e / b;
        if (rr >= cc)
            M[rr + cc * LD] = a.base ? a.S[(size_t)a.base[f] + (size_t)rr + (size_t)cc * a.lds]
                                     : -a.S[(size_t)pos[rr] + (size_t)pos[cc] * a.lds];
    }
    const bool bad = cv_fold_tail<BP>(M, dinv, ub, yb, b, pos, a.U, a.ldu, a.nr, a.var, a.res, a.ldr);
    if (bad && tid == 0) atomicMin(a.fail, a.lab[f]);
}

template <int BP> static hipError_t cv_fold_launch(const CvFoldArgs &a, int nfolds, hipStream_t s)
{
    const size_t shm = ((size_t)(BP + 1) * BP + BP + 512) * sizeof(double);
    // the attribute that allows more than 64 KB of dynamic LDS is per kernel and device: set once per device, not per launch
    // (the mask is this class's own: a template's static)
    static std::atomic<unsigned long long> attr_done{0};
    if (shm > 64 * 1024) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (!(dev >= 0 && dev < 64 && ((attr_done.load(std::memory_order_relaxed) >> dev) & 1ull))) {
            if (hipError_t e = hipFuncSetAttribute((const void *)cv_fold_kernel<BP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)shm))
                return e;
            if (dev >= 0 && dev < 64) attr_done.fetch_or(1ull << dev, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL(cv_fold_kernel<BP>, dim3(nfolds), dim3(256), shm, s, a);
    return hipSuccess;
}

hipError_t launch_cv_folds(int cls, const double *S, size_t lds, const double *U, size_t ldu, int nr, const int *idx,
                           const int *off, const int *flist, const int *lab, int nfolds, double *var, double *res, size_t ldr,
                           int *fail, hipStream_t s)
{
    if (nfolds <= 0) return hipSuccess;
    return launch_cv_folds_at(cls, S, lds, nullptr, U, ldu, nr, idx, off, flist, lab, nfolds, var, res, ldr, fail, s);
}

hipError_t launch_cv_folds_at(int cls, const double *S, size_t lds, const long long *base, const double *U, size_t ldu, int nr,
                              const int *idx, const int *off, const int *flist, const int *lab, int nfolds, double *var,
                              double *res, size_t ldr, int *fail, hipStream_t s)
{
    if (nfolds <= 0) return hipSuccess;
    CvFoldArgs a{S, lds, U, ldu, nr, idx, off, flist, lab, var, res, ldr, fail, base};
    switch (cls) {
    case 16: return cv_fold_launch<16>(a, nfolds, s);
    case 32: return cv_fold_launch<32>(a, nfolds, s);
    case 64: return cv_fold_launch<64>(a, nfolds, s);
    case 128: return cv_fold_launch<128>(a, nfolds, s);
    }
    return hipErrorInvalidValue;
}

__global__ void __launch_bounds__(256)
cv_gather_kernel(const double *S, size_t lds, const double *U, size_t ldu, int nr, const int *pos, int b, int bpad, int rt,
                 double *out, size_t ldo)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ldo * (size_t)bpad) return;
    const int rr = (int)(e % ldo), c = (int)(e / ldo);
    double v;
    if (rr < bpad) {
        if (rr < b && c < b) {
            const int hi = rr >= c ? pos[rr] : pos[c], lo = rr >= c ? pos[c] : pos[rr];
            v = -S[(size_t)hi + (size_t)lo * lds];
        } else
            v = rr == c ? 1.0 : 0.0;
    } else if (rr < bpad + rt) {
        const int k = rr - bpad;
        v = (k < nr && c < b) ? U[(size_t)pos[c] + (size_t)k * ldu] : 0.0;
    } else
        v = rr - bpad - rt == c ? 1.0 : 0.0;
    out[(size_t)rr + (size_t)c * ldo] = v;
}

void launch_cv_gather(const double *S, size_t lds, const double *U, size_t ldu, int nr, const int *pos, int b, int bpad, int rt,
                      double *out, size_t ldo, hipStream_t s)
{
    hipLaunchKernelGGL(cv_gather_kernel, dim3((unsigned)((ldo * (size_t)bpad + 255) / 256)), dim3(256), 0, s, S, lds, U, ldu, nr, pos, b, bpad,
                       rt, out, ldo);
}

__global__ void __launch_bounds__(256)
cv_scatter_kernel(const int *pos, int b, int nr, const double *v, const double *r, double *var, double *res, size_t ldr)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b) return;
    const int o = pos[i];
    var[o] = v[i];
    for (int k = 0; k < nr; ++k) res[(size_t)o + (size_t)k * ldr] = r[(size_t)i + (size_t)k * b];
}

void launch_cv_scatter(const int *pos, int b, int nr, const double *v, const double *r, double *var, double *res, size_t ldr,
                       hipStream_t s)
{
    if (b <= 0) return;
    hipLaunchKernelGGL(cv_scatter_kernel, dim3((b + 255) / 256), dim3(256), 0, s, pos, b, nr, v, r, var, res, ldr);
}

__global__ void __launch_bounds__(256)
cv_border_kernel(const double *U, size_t ldu, int nr, const int *pos, int b, int bpad, int rt, double *out, size_t ldo)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ldo * (size_t)bpad) return;
    const int rr = (int)(e % ldo), c = (int)(e / ldo);
    double v;
    if (rr < bpad)
        v = (rr == c && rr >= b) ? 1.0 : 0.0;
    else if (rr < bpad + rt) {
        const int k = rr - bpad;
        v = (k < nr && c < b) ? U[(size_t)pos[c] + (size_t)k * ldu] : 0.0;
    } else
        v = rr - bpad - rt == c ? 1.0 : 0.0;
    out[(size_t)rr + (size_t)c * ldo] = v;
}

void launch_cv_border(const double *U, size_t ldu, int nr, const int *pos, int b, int bpad, int rt, double *out, size_t ldo,
                      hipStream_t s)
{
    hipLaunchKernelGGL(cv_border_kernel, dim3((unsigned)((ldo * (size_t)bpad + 255) / 256)), dim3(256), 0, s, U, ldu, nr, pos, b,
                       bpad, rt, out, ldo);
}

__global__ void cv_info_take_kernel(int *info, int clean, int *keep, int *fail, int label)
{
    if (threadIdx.x || blockIdx.x) return;
    const int v = *info;
    if (keep) *keep = v;
    else if (v != clean) atomicMin(fail, label);
    *info = clean;
}

__global__ void cv_info_put_kernel(int *info, const int *keep)
{
    if (threadIdx.x || blockIdx.x) return;
    *info = *keep;
}

void launch_cv_info_take(int *info, int clean, int *keep, int *fail, int label, hipStream_t s)
{
    hipLaunchKernelGGL(cv_info_take_kernel, dim3(1), dim3(64), 0, s, info, clean, keep, fail, label);
}

void launch_cv_info_put(int *info, const int *keep, hipStream_t s)
{
    hipLaunchKernelGGL(cv_info_put_kernel, dim3(1), dim3(64), 0, s, info, keep);
}

__global__ void __launch_bounds__(256)
cv_taper_kernel(const double *Z, size_t ldz, int skew, int npad, int n, const double *U, size_t ldu, int nr, double *var,
                double *res, size_t ldr, int *fail, const int *idx, const int *lab)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int i = idx ? idx[t] : t;
    const double k = Z[band_index(i, i, ldz, skew, npad)];
    if (!(k > 0.0) || !isfinite(k)) atomicMin(fail, lab ? lab[t] : i);
    const double v = 1.0 / k;
    var[i] = v;
    for (int c = 0; c < nr; ++c) res[(size_t)i + (size_t)c * ldr] = U[(size_t)i + (size_t)c * ldu] * v;
}

void launch_cv_taper(const double *Z, size_t ldz, int skew, int npad, int n, const double *U, size_t ldu, int nr, double *var,
                     double *res, size_t ldr, int *fail, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(cv_taper_kernel, dim3((n + 255) / 256), dim3(256), 0, s, Z, ldz, skew, npad, n, U, ldu, nr, var, res, ldr,
                       fail, (const int *)nullptr, (const int *)nullptr);
}

void launch_cv_taper_list(const double *Z, size_t ldz, int skew, int npad, const int *idx, const int *lab, int count,
                          const double *U, size_t ldu, int nr, double *var, double *res, size_t ldr, int *fail, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(cv_taper_kernel, dim3((count + 255) / 256), dim3(256), 0, s, Z, ldz, skew, npad, count, U, ldu, nr, var,
                       res, ldr, fail, idx, lab);
}

}  // namespace cocons
