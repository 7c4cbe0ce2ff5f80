// knn.hip -- the Vecchia neighbour search on the device: the m candidates of a query with the smallest key
// (d2, index), d2 = fl(fl(dx dx) + fl(dy dy)) in fp64 exactly in that form (this file is compiled without contraction), no
// square root, ties to the lower index.  One wave per query row walks rings r = 0, 1, 2, .. of cells around the query's clamped
// cell in a uniform grid over the candidates (pattern_grid.hpp, binned by launch_pattern_bin), 64 candidates per step.  The
// best 64 keys so far live as one sorted list, one per lane; candidates above the m-th are dropped by a ballot, the others
// are compacted into LDS and merged in 64 at a time by a bitonic sort and a bitonic merge over the lanes.  After a complete
// ring the walk stops when the m-th d2 is below knn_ring_bound (knn_plan.hpp) or the block covers the grid; a row that has
// visited more cells than there are points scans the cell-sorted list instead.  No floating-point atomics: the order inside a
// cell is the binning's, the key order removes it, and the outputs are a function of the inputs.
#include "kernels.h"
#include "knn_plan.hpp"
#include "knn_keys.hpp"
#include <limits.h>

namespace cocons {
namespace {

// The running best of one query: lane j holds the j-th smallest key seen, thr is lane m - 1's (all ones: fewer than m seen).
// Survivors of the ballot wait in LDS (2 WAVE places) until 64 of them are there or the ring ends.
struct Search {
    Key best, thr;
    int m, lane, cnt;
    unsigned long long *bd;
    int *bi;
};

__device__ __forceinline__ void search_reset(Search &S)
{
    S.best.d = KNN_EMPTY; S.best.i = INT_MAX;
    S.thr = S.best;
    S.cnt = 0;
}

// merge the last min(cnt, 64) waiting survivors into the list (cnt is the same in every lane: every lane calls)
__device__ __forceinline__ void search_flush(Search &S)
{
    if (S.cnt == 0) return;
    __syncthreads();
    const int base = S.cnt > WAVE ? S.cnt - WAVE : 0;
    Key c;
    c.d = KNN_EMPTY; c.i = INT_MAX;
    if (base + S.lane < S.cnt) { c.d = S.bd[base + S.lane]; c.i = S.bi[base + S.lane]; }
    __syncthreads();
    S.cnt = base;
    S.best = wave_merge(S.best, wave_sort(c, S.lane), S.lane);
    S.thr = key_from_lane(S.best, S.m - 1);
}

// one candidate per lane (valid: the lane has one); every lane calls
__device__ __forceinline__ void search_offer(Search &S, bool valid, double qx, double qy, double x, double y, int idx)
{
    const double dx = x - qx, dy = y - qy;
    const double d2 = dx * dx + dy * dy;
    Key c;
    c.d = (unsigned long long)__double_as_longlong(d2); c.i = idx;
    const bool acc = valid && key_less(c, S.thr);
    const unsigned long long b = __ballot(acc);
    if (!b) return;
    const int at = S.cnt + (int)__popcll(b & ((1ull << S.lane) - 1ull));
    if (acc) { S.bd[at] = c.d; S.bi[at] = c.i; }
    S.cnt += (int)__popcll(b);
    if (S.cnt >= WAVE) search_flush(S);
}

// places [k0, k1) of a list (idx null: the points as they lie, place = index), 64 per step; candidates with index >= limit
// are masked
__device__ __forceinline__ void search_run(Search &S, double qx, double qy, const double *x, const double *y, const int *idx,
                                           int k0, int k1, int limit)
{
    for (int kb = k0; kb < k1; kb += WAVE) {
        const int k = kb + S.lane < k1 ? kb + S.lane : k0;
        const int id = idx ? idx[k] : k;
        search_offer(S, kb + S.lane < k1 && id < limit, qx, qy, x[k], y[k], id);
    }
}

__global__ __launch_bounds__(WAVE) void knn_query_kernel(KnnArgs a)
{
    __shared__ unsigned long long bd[2 * WAVE];
    __shared__ int bi[2 * WAVE];
    const int lane = threadIdx.x, q = a.row0 + (int)blockIdx.x;
    const double qx = a.qx[q], qy = a.qy[q];
    const PatternTargets &t = a.t;
    const int limit = a.ordered ? (q < t.n ? q : t.n) : t.n;
    Search S;
    S.m = a.m; S.lane = lane; S.bd = bd; S.bi = bi;
    search_reset(S);
    if (a.brute) {
        search_run(S, qx, qy, t.x, t.y, nullptr, 0, limit, limit);
        search_flush(S);
    } else if (limit > 0) {
        const int nx = t.g.nx, ny = t.g.ny;
        const int cx = pattern_cell_x(t.g, qx), cy = pattern_cell_y(t.g, qy);
        long long visited = 0;
        for (int r = 0;; ++r) {
            const int x0 = cx - r, x1 = cx + r, y0 = cy - r, y1 = cy + r;
            const int xa = x0 > 0 ? x0 : 0, xb = x1 < nx - 1 ? x1 : nx - 1;
            const int ya = y0 > 0 ? y0 : 0, yb = y1 < ny - 1 ? y1 : ny - 1;
            for (int yy = ya; yy <= yb; ++yy) {
                if (yy == y0 || yy == y1) {
                    // the ring's bottom and top rows: one contiguous run of the cell-sorted list
                    if (xa <= xb) {
                        search_run(S, qx, qy, t.sx, t.sy, t.sidx, t.cstart[yy * nx + xa], t.cstart[yy * nx + xb + 1], limit);
                        visited += xb - xa + 1;
                    }
                } else {
                    if (x0 >= 0 && x0 < nx) {
                        search_run(S, qx, qy, t.sx, t.sy, t.sidx, t.cstart[yy * nx + x0], t.cstart[yy * nx + x0 + 1], limit);
                        ++visited;
                    }
                    if (x1 >= 0 && x1 < nx) {
                        search_run(S, qx, qy, t.sx, t.sy, t.sidx, t.cstart[yy * nx + x1], t.cstart[yy * nx + x1 + 1], limit);
                        ++visited;
                    }
                }
            }
            search_flush(S);
            if (x0 <= 0 && x1 >= nx - 1 && y0 <= 0 && y1 >= ny - 1) break;      // the block covers the grid
            if (S.thr.d != KNN_EMPTY && __longlong_as_double((long long)S.thr.d) < knn_ring_bound(t.g.edge, r)) break;
            if (visited > (long long)t.n) {
                // more cells than points (early rows in one corner, a query far away): the whole list, from an empty one
                search_reset(S);
                search_run(S, qx, qy, t.sx, t.sy, t.sidx, 0, t.n, limit);
                search_flush(S);
                break;
            }
        }
    }
    const bool have = lane < a.m && S.best.d != KNN_EMPTY;
    if (a.nn && lane < a.m) a.nn[(size_t)q + (size_t)lane * a.ldn] = have ? S.best.i + 1 : 0;
    if (a.tab) {
        const int v = wave_sort_int(have ? S.best.i : INT_MAX, lane);
        if (lane < a.m) a.tab[(size_t)q * a.m + lane] = v == INT_MAX ? -1 : v;
    }
}

}  // namespace

hipError_t launch_knn_query(const KnnArgs &a, int rows, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(knn_query_kernel, dim3((unsigned)rows), dim3(WAVE), 0, s, a);
    return hipGetLastError();
}

}  // namespace cocons
