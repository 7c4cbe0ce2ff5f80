// vecchia_tri.hpp -- the packed lower triangle of a Vecchia block in LDS: what vecchia.hip's block kernel and vecchia_sim.hip's
// coefficient kernel index their blocks with, and the forward substitution on it that vecchia.hip and vecchia_group.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace cocons {

// element (r, c), r >= c, of the packed lower triangle (row after row)
__device__ __forceinline__ int tri_at(int r, int c) { return r * (r + 1) / 2 + c; }

// pair t = r (r - 1) / 2 + c of the packed strict lower triangle, r > c
__device__ __forceinline__ void tri_pair(int t, int &r, int &c)
{
    r = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)t)) * 0.5f);
    while (r * (r - 1) / 2 > t) --r;
    while ((r + 1) * r / 2 <= t) ++r;
    c = t - r * (r - 1) / 2;
}

// the information launches' rows behind the factor: the site derivatives and two vectors of kb doubles
constexpr int VECCHIA_FX = GSITE_FIELDS + 2;

// Forward substitution over the neighbours' rows for VECCHIA_G right-hand sides in registers, lane = row: lane r ends with
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

}  // namespace cocons
