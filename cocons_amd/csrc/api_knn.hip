// api_knn.hip -- C ABI of the Vecchia neighbour search: the stateless cocons_vecchia_neighbours, the handle
// whose table is searched on the device (cocons_fit_create_vecchia_knn) and local kriging with the neighbours found per chunk
// (cocons_vecchia_predict_knn), over the plan of knn_plan.hpp; the host-only cocons_debug_knn_plan, which computes that plan
// with the header the kernels use, and cocons_debug_knn_phases, which times the search's two phases by events.  The handle
// and the prediction themselves are api_vecchia.hip's.
#include "fit.hpp"
#include "knn_plan.hpp"

int knn_grid_build(const char *who, PatternGridBufs &G, int n, const double *hx, const double *hy, const double *dx,
                   const double *dy, hipStream_t s)
{
    const PatternGrid g = knn_grid_make(n, hx, hy);
    if (int rc = pattern_grid_alloc(who, G, (size_t)n, pattern_cells(g))) return rc;
    return pattern_grid_bin(who, G, g, n, dx, dy, s);
}

// Events on one stream, alternately in front of a stretch of binning and of a stretch of queries (cocons_debug_knn_phases);
// off: nothing is created or recorded
struct KnnMarks {
    bool on;
    hipStream_t s;
    std::vector<hipEvent_t> ev;
    ~KnnMarks() { for (hipEvent_t e : ev) hipEventDestroy(e); }
    hipError_t mark()
    {
        if (!on) return hipSuccess;
        hipEvent_t e = nullptr;
        if (hipError_t rc = hipEventCreate(&e)) return rc;
        ev.push_back(e);
        return hipEventRecord(e, s);
    }
    // after the stream is drained: stretch k lies between marks k and k + 1, even k: queries, odd k: binning
    hipError_t sums(KnnPhases &ph) const
    {
        for (size_t k = 0; k + 1 < ev.size(); ++k) {
            float ms = 0.0f;
            if (hipError_t rc = hipEventElapsedTime(&ms, ev[k], ev[k + 1])) return rc;
            (k % 2 ? ph.build_ms : ph.query_ms) += ms;
        }
        return hipSuccess;
    }
};

int knn_self_search(const char *who, int n, const double *hx, const double *hy, const double *dx, const double *dy, int m,
                    int *d_nn, int *d_tab, hipStream_t s, KnnPhases *phases)
{
    const std::vector<KnnLevel> levels = knn_levels(n, hx, hy);
    KnnMarks marks{phases != nullptr, s, {}};
    KnnArgs a;
    a.qx = dx; a.qy = dy; a.m = m; a.ordered = 1;
    a.nn = d_nn; a.ldn = (size_t)n; a.tab = d_tab;
    a.brute = 1;
    a.t.x = dx; a.t.y = dy; a.t.n = knn_head(n);
    HIPCHK_AT(who, marks.mark());
    HIPCHK_AT(who, launch_knn_query(a, knn_head(n), s));
    a.brute = 0;
    PatternGridBufs G;
    size_t cells = 1;
    for (const KnnLevel &l : levels) cells = std::max(cells, pattern_cells(l.g));
    if (!levels.empty())
        if (int rc = pattern_grid_alloc(who, G, (size_t)n, cells)) return rc;
    for (const KnnLevel &l : levels) {
        HIPCHK_AT(who, marks.mark());
        if (int rc = pattern_grid_bin(who, G, l.g, l.hi, dx, dy, s)) return rc;
        a.t = G.t; a.row0 = l.lo;
        HIPCHK_AT(who, marks.mark());
        HIPCHK_AT(who, launch_knn_query(a, l.hi - l.lo, s));
    }
    HIPCHK_AT(who, marks.mark());
    HIPCHK_AT(who, hipStreamSynchronize(s));          // the levels' buffers go out of scope
    if (phases) HIPCHK_AT(who, marks.sums(*phases));
    return 0;
}

// cocons_vecchia_neighbours under the name of the entry that asks; phases (may be null): the ordered self search is timed by
// events and its table stays on the device (nn is not read)
static int knn_neighbours_impl(const char *who, int n, const double *locs, int mq, const double *locs_query, int m, int device,
                               int *nn, KnnPhases *phases)
{
    if (!locs || (!nn && !phases)) return fail(-1, "%s: null argument", who);
    if (n < 1) return fail(-1, "%s: n = %d (at least one point expected)", who, n);
    if (locs_query && mq < 0) return fail(-1, "%s: mq = %d with a query set", who, mq);
    if (m < 1 || m > VECCHIA_M_MAX) return fail(-1, "%s: m = %d is outside 1 .. %d", who, m, VECCHIA_M_MAX);
    if (int rc = pattern_check_finite(who, "locs", (size_t)n, locs)) return rc;
    if (locs_query && mq > 0)
        if (int rc = pattern_check_finite(who, "locs_query", (size_t)mq, locs_query)) return rc;
    const int rows = locs_query ? mq : n;
    if (rows == 0) return 0;
    HIPCHK_AT(who, hipSetDevice(device < 0 ? 0 : device));
    DevBuf<double> dl, dq;
    DevBuf<int> dnn;
    PatternGridBufs G;
    StreamDrain s{nullptr, true};     // own non-blocking stream (the library never launches on the NULL stream)
    HIPCHK_AT(who, hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking));
    HIPCHK_AT(who, dl.alloc((size_t)2 * n));
    HIPCHK_AT(who, dnn.alloc((size_t)rows * m));
    HIPCHK_AT(who, upload_canon(dl, locs, (size_t)2 * n, s));
    if (!locs_query) {
        if (int rc = knn_self_search(who, n, locs, locs + n, dl, dl + n, m, dnn, nullptr, s, phases)) return rc;
        if (phases) return 0;
    } else {
        HIPCHK_AT(who, dq.alloc((size_t)2 * mq));
        HIPCHK_AT(who, upload_canon(dq, locs_query, (size_t)2 * mq, s));
        if (int rc = knn_grid_build(who, G, n, locs, locs + n, dl, dl + n, s)) return rc;
        KnnArgs a;
        a.t = G.t; a.qx = dq; a.qy = dq + mq; a.m = m;
        a.nn = dnn; a.ldn = (size_t)mq;
        HIPCHK_AT(who, launch_knn_query(a, mq, s));
    }
    HIPCHK_AT(who, hipMemcpyAsync(nn, dnn, (size_t)rows * m * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipStreamSynchronize(s));
    return 0;
}

extern "C" int cocons_vecchia_neighbours(int n, const double *locs, int mq, const double *locs_query, int m, int device, int *nn)
{
    return knn_neighbours_impl("cocons_vecchia_neighbours", n, locs, mq, locs_query, m, device, nn, nullptr);
}

extern "C" int cocons_debug_knn_phases(int n, const double *locs, int m, int device, double *ms2)
{
    const char *who = "cocons_debug_knn_phases";
    if (!ms2) return fail(-1, "%s: null argument", who);
    KnnPhases ph;
    if (int rc = knn_neighbours_impl(who, n, locs, 0, nullptr, m, device, nullptr, &ph)) return rc;
    ms2[0] = ph.build_ms; ms2[1] = ph.query_ms;
    return 0;
}

extern "C" cocons_fit *cocons_fit_create_vecchia_knn(int n, int p, int r, const double *locs, const double *X, const double *z,
                                                     const double *smooth_limits, int device, int m)
{
    return vecchia_create_impl("cocons_fit_create_vecchia_knn", n, p, r, locs, X, z, smooth_limits, device, m, nullptr, true);
}

extern "C" int cocons_vecchia_predict_knn(cocons_fit *f, const double *theta, const double *mean, int z_col, int mp,
                                          const double *locs_pred, const double *X_pred, int m_pred, double *stochastic,
                                          double *quadform)
{
    return vecchia_predict_impl("cocons_vecchia_predict_knn", f, theta, mean, z_col, mp, locs_pred, X_pred, m_pred, nullptr, true,
                                stochastic, quadform);
}

extern "C" int cocons_debug_knn_plan(int n, const double *locs, int level, int m, const double *pts, int rmax, int *plan,
                                     double *geom5, int *cells, double *bounds)
{
    const char *who = "cocons_debug_knn_plan";
    if (!locs || !plan || !geom5 || n < 1 || m < 0 || (m > 0 && (!pts || !cells)) || rmax < -1 || (rmax >= 0 && !bounds))
        return fail(-1, "%s: bad argument", who);
    for (size_t i = 0; i < (size_t)2 * n; ++i)
        if (!std::isfinite(locs[i])) return fail(-1, "%s: a coordinate is not finite", who);
    const std::vector<KnnLevel> levels = knn_levels(n, locs, locs + n);
    const int nl = (int)levels.size();
    if (nl > KNN_LEVELS_MAX) return fail(-1, "%s: %d levels, more than the outputs have room for (%d)", who, nl, KNN_LEVELS_MAX);
    if (level < 0 || level > nl) return fail(-1, "%s: level = %d is outside 0 .. %d", who, level, nl);
    plan[0] = knn_head(n); plan[1] = nl;
    std::vector<PatternGrid> grids;
    for (int l = 0; l < nl; ++l) {
        plan[2 + 2 * l] = levels[l].lo; plan[3 + 2 * l] = levels[l].hi;
        grids.push_back(levels[l].g);
    }
    grids.push_back(knn_grid_make(n, locs, locs + n));       // the prediction side's grid over all n points
    for (int l = 0; l <= nl; ++l) {
        const PatternGrid &g = grids[l];
        double *o = geom5 + 5 * l;
        o[0] = g.x0; o[1] = g.y0; o[2] = g.edge; o[3] = g.nx; o[4] = g.ny;
    }
    const PatternGrid &g = grids[level];
    for (int i = 0; i < m; ++i) {
        cells[2 * i] = pattern_cell_x(g, pts[i]);
        cells[2 * i + 1] = pattern_cell_y(g, pts[i + (size_t)m]);
    }
    for (int r = 0; r <= rmax; ++r) bounds[r] = knn_ring_bound(g.edge, r);
    return 0;
}
