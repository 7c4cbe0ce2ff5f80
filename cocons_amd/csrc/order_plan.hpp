// order_plan.hpp -- the plan of the maxmin ordering by scale-halving nets (order.hip), in ONE place for the
// kernels, the host and the diagnostic entry: the labels, the bounding box with its centre and longer side L, every level's
// radius, the dense grid of a level and the rule that chooses between the dense grid and the binned one.  Standard headers only.
//
// THE RULE.  d2(a, b) = fl(fl(dx dx) + fl(dy dy)) in fp64, no contraction, no square root (knn.hip's d2).
//  1. label(i): with b the smallest integer >= 1 with 2^b >= n, mask = 2^b - 1 and s = (b + 1) / 2, mix(v) is three rounds of
//     v = (v C_j) & mask, v ^= v >> s (64-bit product; C = 0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35), and label(i) is the first of
//     mix(i), mix(mix(i)), .. below n.  Every round is a bijection of the b-bit words, so the labels are a permutation of
//     0 .. n - 1.  A lower label is a higher priority.
//  2. Level 0: the point with the smallest key (d2(point, c), caller's index), c = (x0 + 0.5 (x1 - x0), y0 + 0.5 (y1 - y0)).
//  3. Levels k = 1 .. 64: L = max(x1 - x0, y1 - y0), l_k = ldexp(L, 1 - k), e_k = fl(l_k l_k); two points conflict iff
//     d2 < e_k.  Level k: walk the points not yet ordered in ascending label and take a point iff it conflicts with nothing
//     taken so far, at this level or an earlier one.  Inside a level the points stand in ascending label.
//  4. What is left after level 64 follows in ascending label.
//
// The dense grid of level k has the edge g = fl(0.5 l_k (1 + 2^-20)).  Two points of one cell have |dx|, |dy| < g (1 + 2^-30)
// (the quotients (v - origin) / g carry a relative error of 2^-52 at a magnitude below 2^14), so their d2 is below
// 0.51 l_k^2 < e_k: they conflict, and a cell holds at most ONE ordered point.  Two points with d2 < e_k have
// |dx| < l_k (1 + 2^-52), their quotients differ by less than 2 / (1 + 2^-20) + 2^-36 < 2, and the floors by at most 2: every
// conflict lies in the 5 x 5 block of cells.  The binned grid (pattern_grid.hpp) has an edge of l_k (1 + 2^-20) at least and
// the 3 x 3 block by that header's argument.
#pragma once
#include "pattern_grid.hpp"

namespace cocons {

constexpr int ORDER_LEVELS = 64;                    // levels 1 .. 64; what is left behind them is the rest
constexpr int ORDER_COUNTS = ORDER_LEVELS + 3;      // level_counts: [0], level 0, levels 1 .. 64, the rest
constexpr long long ORDER_DENSE_MIN = 1ll << 12;    // the dense grid's cap on cells: 32 n within these two
constexpr long long ORDER_DENSE_MAX = 1ll << 26;
constexpr double ORDER_SPAN_MAX = 0x1p511;          // a longer side above this is refused: 2 L^2 must be finite

struct OrderLabels {
    unsigned long long mask = 1;
    int n = 1, s = 1;
};

inline OrderLabels order_labels_make(int n)
{
    OrderLabels l;
    int b = 1;
    while ((1ll << b) < (long long)n) ++b;
    l.n = n; l.mask = (1ull << b) - 1ull; l.s = (b + 1) / 2;
    return l;
}

COCONS_HD inline unsigned long long order_mix(const OrderLabels &l, unsigned long long v)
{
    v = (v * 0x9E3779B1ull) & l.mask; v ^= v >> l.s;
    v = (v * 0x85EBCA6Bull) & l.mask; v ^= v >> l.s;
    v = (v * 0xC2B2AE35ull) & l.mask; v ^= v >> l.s;
    return v;
}

// cycle walking: the walk from i < n returns to a word below n after at most 2^b - n + 1 steps (mix is a permutation)
COCONS_HD inline int order_label(const OrderLabels &l, int i)
{
    unsigned long long v = order_mix(l, (unsigned long long)i);
    while (v >= (unsigned long long)l.n) v = order_mix(l, v);
    return (int)v;
}

COCONS_HD inline double order_d2(double ax, double ay, double bx, double by)
{
    const double dx = ax - bx, dy = ay - by;
    return dx * dx + dy * dy;
}

struct OrderBox {
    double x0 = 0.0, y0 = 0.0, x1 = 0.0, y1 = 0.0;
    double cx = 0.0, cy = 0.0, L = 0.0;
};

// the box of n >= 1 finite points
inline OrderBox order_box_make(int n, const double *x, const double *y)
{
    OrderBox b;
    b.x0 = b.x1 = x[0]; b.y0 = b.y1 = y[0];
    for (int i = 1; i < n; ++i) {
        if (x[i] < b.x0) b.x0 = x[i];
        if (x[i] > b.x1) b.x1 = x[i];
        if (y[i] < b.y0) b.y0 = y[i];
        if (y[i] > b.y1) b.y1 = y[i];
    }
    const double ex = b.x1 - b.x0, ey = b.y1 - b.y0;
    b.cx = b.x0 + 0.5 * ex; b.cy = b.y0 + 0.5 * ey;
    b.L = ex > ey ? ex : ey;
    return b;
}

// level 0: the smallest key (d2 to the centre, index)
inline int order_first(const OrderBox &b, int n, const double *x, const double *y)
{
    int best = 0;
    double bd = order_d2(x[0], y[0], b.cx, b.cy);
    for (int i = 1; i < n; ++i) {
        const double d = order_d2(x[i], y[i], b.cx, b.cy);
        if (d < bd) { bd = d; best = i; }
    }
    return best;
}

inline double order_ell(const OrderBox &b, int k) { return ldexp(b.L, 1 - k); }
inline double order_e(const OrderBox &b, int k) { const double l = order_ell(b, k); return l * l; }

inline long long order_dense_cap(int n)
{
    const long long want = 32ll * n;
    return want < ORDER_DENSE_MIN ? ORDER_DENSE_MIN : want > ORDER_DENSE_MAX ? ORDER_DENSE_MAX : want;
}

// The dense grid of level k over the box, edge 0.5 l_k (1 + 2^-20); dense = false (g meaningless) where the level has no
// usable edge or more cells than the cap: the binned grid takes it.
inline bool order_dense_grid(const OrderBox &b, int k, long long cap, PatternGrid &g)
{
    const double edge = 0.5 * order_ell(b, k) * (1.0 + 0x1p-20);
    if (!(edge > 0.0)) return false;                                // L = 0, or an underflow
    const long long cx = pattern_axis_cells(b.x1 - b.x0, edge), cy = pattern_axis_cells(b.y1 - b.y0, edge);
    if (cx > (1ll << 14) || cy > (1ll << 14) || cx * cy > cap) return false;
    g.x0 = b.x0; g.y0 = b.y0; g.edge = edge; g.nx = (int)cx; g.ny = (int)cy;
    return true;
}

// The binned grid for level k: pattern_grid_make's for delta = l_k over the box's corners, edge l_k (1 + 2^-20) at least and
// as much larger as its cell caps ask.  l_k = 0 (L = 0, or an underflow): nothing conflicts, any grid serves.
inline PatternGrid order_binned_grid(const OrderBox &b, int k)
{
    const double xs[2] = {b.x0, b.x1}, ys[2] = {b.y0, b.y1};
    double delta = order_ell(b, k);
    if (!(delta > 0.0)) delta = 1.0;
    return pattern_grid_make(2, xs, ys, delta);
}

}  // namespace cocons
