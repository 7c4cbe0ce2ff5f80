// knn_keys.hpp -- sorted keys across the 64 lanes of a wavefront: what the neighbour search (knn.hip) and the
// re-ranking by model correlation (knn_corr.hip) keep their best 64 candidates in.  A key is 64 bits whose
// integer order is the rule's order, with the index breaking ties; one key per lane, ascending over the lanes.
#pragma once
#include <hip/hip_runtime.h>

namespace cocons {
namespace {

constexpr int WAVE = 64;
constexpr unsigned long long KNN_EMPTY = ~0ull;      // no key has this pattern (knn.hip: d2 >= 0 is never a NaN for finite points)

// d2's bit pattern orders as an integer (d2 >= 0), the index breaks ties
struct Key {
    unsigned long long d;
    int i;
};

__device__ __forceinline__ bool key_less(const Key &a, const Key &b) { return a.d < b.d || (a.d == b.d && a.i < b.i); }

__device__ __forceinline__ Key key_from_lane(const Key &k, int src)
{
    Key o;
    o.d = __shfl(k.d, src);
    o.i = __shfl(k.i, src);
    return o;
}

// compare-exchange with lane ^ j: the smaller (keep_min) or the larger key of the two
__device__ __forceinline__ Key key_exchange(const Key &k, int lane, int j, bool keep_min)
{
    const Key o = key_from_lane(k, lane ^ j);
    return key_less(o, k) == keep_min ? o : k;
}

// 64 keys, one per lane, ascending over the lanes
__device__ __forceinline__ Key wave_sort(Key k, int lane)
{
    for (int s = 2; s <= WAVE; s <<= 1)
        for (int j = s >> 1; j > 0; j >>= 1) k = key_exchange(k, lane, j, ((lane & j) == 0) == ((lane & s) == 0));
    return k;
}

// the 64 smallest of two ascending lists of 64, ascending
__device__ __forceinline__ Key wave_merge(Key best, const Key &cand, int lane)
{
    const Key rev = key_from_lane(cand, WAVE - 1 - lane);
    if (key_less(rev, best)) best = rev;
    for (int j = WAVE / 2; j > 0; j >>= 1) best = key_exchange(best, lane, j, (lane & j) == 0);
    return best;
}

__device__ __forceinline__ int wave_sort_int(int v, int lane)
{
    for (int s = 2; s <= WAVE; s <<= 1)
        for (int j = s >> 1; j > 0; j >>= 1) {
            const int o = __shfl(v, lane ^ j);
            const bool keep_min = ((lane & j) == 0) == ((lane & s) == 0);
            v = (o < v) == keep_min ? o : v;
        }
    return v;
}

}  // namespace
}  // namespace cocons
