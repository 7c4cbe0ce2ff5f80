// knn_plan.hpp -- the plan of the Vecchia neighbour search (knn.hip), in ONE place for the kernels, the host
// and the diagnostic entry: the head, the doubling levels, every level's grid (a PatternGrid of pattern_grid.hpp whose edge is
// chosen for a handful of points per cell) and the stopping bound of the ring walk.  Standard headers only.
//
// The stopping bound.  After ring r of cells around the query's clamped cell is complete, a candidate that has not been seen
// lies in a cell whose coordinate differs from the query's by r + 1 at least along one axis.  Along that axis the computed
// quotients (v - origin) / edge then differ by more than r; each carries a relative error of 2^-52 at a magnitude of at most
// PATTERN_CELLS_AXIS_MAX = 2^20, an absolute 2^-32, so the points themselves are more than (r - 2^-31) edge apart.  A query
// clamped to -1 or `count` lies beyond the box on that side (the sign of v - origin is exact), which only adds distance.
// b = fl(edge (r - 2^-20)) is below that, so fl(dx) >= b, fl(dx dx) >= fl(b b) and fl(fl(dx dx) + fl(dy dy)) >= fl(b b) by
// the monotonicity of rounding: knn_ring_bound is a lower bound on the d2 THE KERNEL COMPUTES for anything outside the block.
#pragma once
#include "pattern_grid.hpp"
#include <vector>

namespace cocons {

constexpr int KNN_HEAD = 64;          // rows [0, KNN_HEAD) are searched by brute force: one wave scans all predecessors
constexpr int KNN_CELL_POINTS = 16;   // points per cell the edge of a level's grid aims at
constexpr int KNN_LEVELS_MAX = 32;    // doubling from KNN_HEAD passes INT_MAX before that

// lower bound on the d2 of a candidate outside the (2 r + 1)^2 block of cells around the query's clamped cell
COCONS_HD inline double knn_ring_bound(double edge, int r)
{
    if (r < 1) return 0.0;
    const double b = edge * ((double)r - 0x1p-20);
    return b * b;
}

inline int knn_head(int n) { return n < KNN_HEAD ? n : KNN_HEAD; }

// the grid over the first cnt >= 1 finite points: KNN_CELL_POINTS per cell of the bounding box (per cell of its longer side
// where the box is thinner than such a cell), within the cell caps of pattern_grid_make
inline PatternGrid knn_grid_make(int cnt, const double *x, const double *y)
{
    double x0 = x[0], x1 = x[0], y0 = y[0], y1 = y[0];
    for (int i = 1; i < cnt; ++i) {
        if (x[i] < x0) x0 = x[i];
        if (x[i] > x1) x1 = x[i];
        if (y[i] < y0) y0 = y[i];
        if (y[i] > y1) y1 = y[i];
    }
    const double ex = x1 - x0, ey = y1 - y0, share = (double)KNN_CELL_POINTS / (double)cnt;
    double edge = fmax(sqrt(ex) * sqrt(ey) * sqrt(share), fmax(ex, ey) * share);
    if (!(edge > 0.0 && edge <= 1.0e300)) edge = 1.0;     // all points coincident: one cell
    return pattern_grid_make(cnt, x, y, edge);
}

struct KnnLevel {
    int lo = 0, hi = 0;      // rows [lo, hi), hi <= 2 lo, search the grid over the first hi points
    PatternGrid g;
};

// the levels of the ordered search over n points: they tile [knn_head(n), n)
inline std::vector<KnnLevel> knn_levels(int n, const double *x, const double *y)
{
    std::vector<KnnLevel> out;
    for (long long lo = knn_head(n); lo < n;) {
        const long long hi = 2 * lo < n ? 2 * lo : n;
        KnnLevel l;
        l.lo = (int)lo; l.hi = (int)hi;
        l.g = knn_grid_make(l.hi, x, y);
        out.push_back(l);
        lo = hi;
    }
    return out;
}

}  // namespace cocons
