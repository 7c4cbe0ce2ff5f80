// vecchia_tri.hpp -- the packed lower triangle of a Vecchia block in LDS: what vecchia.hip's block kernel and vecchia_sim.hip's
// coefficient kernel index their blocks with.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace cocons
