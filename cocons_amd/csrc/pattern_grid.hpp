// pattern_grid.hpp -- the uniform grid of the taper-pattern builder (pattern.hip), in ONE place for the kernels and the host:
// origin, cell edge, cell counts, the cell of a point and its clamping.  Standard headers only; the functions are
// __host__ __device__ under hipcc and plain inline functions under any C++17 compiler.
//
// The grid covers the bounding box of the TARGETS with nx x ny square cells of edge `edge`, numbered row-major
// (cell = cy * nx + cx).  A point's cell coordinate is floor((v - origin) / edge), clamped to [-1, count]: -1 and `count`
// stand for "outside, on this side", whatever the distance.  The edge is delta * (1 + 2^-20) at least, so two points
// no further apart than delta along an axis have cell coordinates that differ by at most 1 in floating point too: the
// quotients carry a relative rounding error of 2^-52 at a magnitude below PATTERN_CELLS_AXIS_MAX = 2^20 (an absolute
// 2^-32), the slack between them is 2^-20 of a cell.  Every target within delta of a point therefore lies in the 3 x 3 block of
// cells around the point's clamped cell (cells outside [0, count) hold nothing), and with row-major numbering the block
// is three contiguous runs of the cell-sorted target list.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define COCONS_HD __host__ __device__
#else
#define COCONS_HD
#endif

namespace cocons {

constexpr long long PATTERN_CELLS_MAX = 1ll << 20;   // cap on nx * ny: the edge grows until the grid fits
constexpr int PATTERN_CELLS_AXIS_MAX = 1 << 20;      // ... and on either count alone (a collinear set)

struct PatternGrid {
    double x0 = 0.0, y0 = 0.0;   // origin: the targets' minimum per coordinate
    double edge = 1.0;           // cell edge (> delta)
    int nx = 1, ny = 1;          // cells per axis
};

// cell coordinate of v along one axis, clamped to [-1, count]
COCONS_HD inline int pattern_cell_axis(double v, double origin, double edge, int count)
{
    double u = floor((v - origin) / edge);
    if (!(u >= -1.0)) u = -1.0;
    if (u > (double)count) u = (double)count;
    return (int)u;
}

COCONS_HD inline int pattern_cell_x(const PatternGrid &g, double x) { return pattern_cell_axis(x, g.x0, g.edge, g.nx); }
COCONS_HD inline int pattern_cell_y(const PatternGrid &g, double y) { return pattern_cell_axis(y, g.y0, g.edge, g.ny); }

// cells of an axis of extent `ext` (>= 0) at this edge: the point at the far end gets the last cell
inline long long pattern_axis_cells(double ext, double edge)
{
    const double c = floor(ext / edge) + 1.0;
    return c < 4.0e18 ? (long long)c : (long long)4.0e18;
}

// the grid over n >= 1 finite targets for a finite delta > 0
inline PatternGrid pattern_grid_make(int n, const double *x, const double *y, double delta)
{
    PatternGrid g;
    double x1 = x[0], y1 = y[0];
    g.x0 = x[0]; g.y0 = y[0];
    for (int i = 1; i < n; ++i) {
        if (x[i] < g.x0) g.x0 = x[i];
        if (x[i] > x1) x1 = x[i];
        if (y[i] < g.y0) g.y0 = y[i];
        if (y[i] > y1) y1 = y[i];
    }
    const double ex = x1 - g.x0, ey = y1 - g.y0;
    g.edge = delta * (1.0 + 0x1p-20);
    for (;;) {
        const long long cx = pattern_axis_cells(ex, g.edge), cy = pattern_axis_cells(ey, g.edge);
        if (cx <= PATTERN_CELLS_AXIS_MAX && cy <= PATTERN_CELLS_AXIS_MAX && cx * cy <= PATTERN_CELLS_MAX) {
            g.nx = (int)cx; g.ny = (int)cy;
            return g;
        }
        // too many cells: a larger edge (by the shortfall where that is known, by at least a quarter every round)
        double grow = 1.25;
        if (cx <= PATTERN_CELLS_AXIS_MAX && cy <= PATTERN_CELLS_AXIS_MAX)
            grow = fmax(grow, sqrt((double)(cx * cy) / (double)PATTERN_CELLS_MAX));
        else
            grow = fmax(grow, (double)(cx > cy ? cx : cy) / (double)PATTERN_CELLS_AXIS_MAX);
        g.edge *= grow;
    }
}

}  // namespace cocons
