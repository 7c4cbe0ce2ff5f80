// api_knn_corr.hip -- C ABI of the Vecchia neighbours by model correlation (the rule: include/cocons_hip.h):
// cocons_vecchia_neighbours_corr, the table of a Vecchia handle's observations at theta, and cocons_fit_create_vecchia_corr_knn,
// the handle whose table it is.  Both run one chain on the handle's stream -- the ordered Euclidean search of width m_cand
// (knn_self_search), the records at theta (vecchia_records), the re-ranking (launch_knn_corr) -- and neither table reaches
// the host on the way to a handle, plain or grouped (cocons_fit_create_vecchia_grouped_corr_knn: the chain of
// cocons_fit_create_vecchia_grouped_knn with this table in the place of its search); cocons_debug_knn_corr_phases times the
// three by events.  New locations: cocons_vecchia_neighbours_corr_pred and cocons_vecchia_predict_corr_knn
// are vecchia_predict_impl with a third table source, whose per-chunk step (corr_pred_chunk) and handle-held lists
// (corr_pred_prepare) live here.  The scratch (the candidate table,
// the table that goes home) belongs to the call; the records land in the handle's own per-evaluation buffer, which every
// evaluation rewrites.  No existing entry comes here.
#include "fit.hpp"

int corr_check_shape(const char *who, int m_cand, int hops, int m)
{
    if (m_cand < 1 || m_cand > VECCHIA_M_MAX) return fail(-1, "%s: m_cand = %d is outside 1 .. %d", who, m_cand, VECCHIA_M_MAX);
    if (hops < 1 || hops > 2) return fail(-1, "%s: hops = %d is outside 1 .. 2", who, hops);
    if (m < 1 || m > VECCHIA_M_MAX) return fail(-1, "%s: m = %d is outside 1 .. %d", who, m, VECCHIA_M_MAX);
    const int most = std::min(cocons::KNN_CORR_CAND_MAX, m_cand + m_cand * m_cand * (hops - 1));
    if (m > most) return fail(-1, "%s: m = %d, but a row has %d candidates at the most (m_cand = %d, hops = %d)", who, m, most, m_cand, hops);
    return 0;
}

int corr_check_theta(const char *who, const double *theta, int p)
{
    for (int k = 0; k < 6 * p; ++k)
        if (!std::isfinite(theta[k])) return fail(-1, "%s: theta[%d] is not finite", who, k);
    return 0;
}

namespace {

// search -> records at theta -> re-rank on the handle's stream, drained.  d_nn (n x m column-major, 1-based, largest rho
// first; may be null), d_tab (the layout of VecchiaState::nbr; may be null).  0, or the smallest 1-based row with a rho that
// is not finite (the failing-block convention; the tables then hold nothing to be used).  ms3 (may be null: no events are
// made): the device milliseconds of the search, the records and the re-ranking launch, by events on the stream.
int corr_table(const char *who, cocons_fit *f, const double *theta, int m_cand, int hops, int m, int *d_nn, int *d_tab,
               double *ms3 = nullptr)
{
    VecchiaState *V = f->vecchia.get();
    const int n = f->n;
    hipStream_t s = f->stream;
    DevBuf<int> cand;
    StreamDrain drain{s, false};
    struct Marks {
        hipEvent_t ev[4] = {};
        ~Marks() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
    } marks;
    auto mark = [&](int k) { return ms3 ? hipEventRecord(marks.ev[k], s) : hipSuccess; };
    if (ms3) for (hipEvent_t &e : marks.ev) HIPCHK_AT(who, hipEventCreate(&e));
    HIPCHK_AT(who, cand.alloc((size_t)n * m_cand));
    HIPCHK_AT(who, mark(0));
    if (int rc = knn_self_search(who, n, f->h_locs.data(), f->h_locs.data() + n, f->dlocs, f->dlocs + n, m_cand, nullptr, cand, s))
        return rc;
    if (int rc = reset_info(f)) return rc;
    HIPCHK_AT(who, mark(1));
    const ModeSel ms = vecchia_records(f, theta, 0, V->aos);
    HIPCHK_AT(who, mark(2));
    KnnCorrArgs a;
    a.n = n; a.mc = m_cand; a.hops = hops; a.m = m;
    a.cand = cand; a.aos = V->aos; a.gr = ms.gr; a.nu_fixed = ms.nu_fixed;
    a.nn = d_nn; a.ldn = (size_t)n; a.tab = d_tab; a.fail = f->dinfo;
    HIPCHK_AT(who, launch_knn_corr(ms.mode, a, s));
    HIPCHK_AT(who, mark(3));
    HIPCHK_AT(who, hipMemcpyAsync(f->hinfo, f->dinfo, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipStreamSynchronize(s));
    for (int k = 0; ms3 && k < 3; ++k) {
        float t = 0.0f;
        HIPCHK_AT(who, hipEventElapsedTime(&t, marks.ev[k], marks.ev[k + 1]));
        ms3[k] = t;
    }
    if (f->hinfo[0] == 0x7f7f7f7f) return 0;
    return fail(f->hinfo[0], "%s: row %d has a candidate whose correlation is not finite", who, f->hinfo[0]);
}

struct CorrKnnSource : VecchiaTableSource {
    const double *theta = nullptr;
    int m_cand = 0, hops = 0, m = 0;
    int make(const char *who, cocons_fit *f, const double *) override
    {
        VecchiaState *V = f->vecchia.get();
        HIPCHK_AT(who, V->nbr.alloc((size_t)f->n * m));
        V->m = m;
        return corr_table(who, f, theta, m_cand, hops, m, nullptr, V->nbr);
    }
};

// cocons_fit_create_vecchia_grouped_knn's chain with the correlation table at the handle's theta in the place of the search
struct CorrTableStep : GroupedTableStep {
    const double *theta = nullptr;
    int m_cand = 0, hops = 0;
    int table(const char *who, cocons_fit *f, const double *, int m, int *d_tab) override
    {
        return corr_table(who, f, theta, m_cand, hops, m, nullptr, d_tab);
    }
};

}  // namespace

// ---- new locations ------------------------------------------------------------------------------------------
int corr_pred_prepare(const char *who, cocons_fit *f, int m_cand, int hops, hipStream_t s)
{
    VecchiaState *V = f->vecchia.get();
    if (int rc = vecchia_need_grid(who, f, s)) return rc;
    if (hops < 2 || (V->corr_all.get() && V->corr_all_mc == m_cand)) return 0;
    // the second-hop lists: every observation's plain kNN among all observations, the handle's from here on (counted by
    // cocons_vecchia_info, freed with it): n x m_cand ints -- 120 MB at n = 10^6, m_cand = 30
    const int n = f->n;
    V->corr_all_mc = 0;
    if (hipError_t e = V->corr_all.alloc((size_t)n * m_cand)) {
        V->corr_all.reset();
        (void)hipGetLastError();
        return fail(-100 - (int)e, "%s: %s", who, hipGetErrorString(e));
    }
    KnnArgs k;
    k.t = V->knn->t; k.qx = f->dlocs; k.qy = f->dlocs + n; k.m = m_cand; k.tab = V->corr_all;
    hipError_t e = launch_knn_query(k, n, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        V->corr_all.reset();
        (void)hipGetLastError();
        return fail(-100 - (int)e, "%s: %s", who, hipGetErrorString(e));
    }
    V->corr_all_mc = m_cand;
    return 0;
}

int corr_pred_chunk(const char *who, cocons_fit *f, const CorrPredSource &c, int m, int mc, int row0, const double *dlp,
                    const double *drec, const double *aosC, double gr, int *d_first, int *d_tab, int *d_nn, hipStream_t s)
{
    VecchiaState *V = f->vecchia.get();
    KnnArgs k;
    k.t = V->knn->t; k.qx = dlp; k.qy = dlp + mc; k.m = c.m_cand; k.tab = d_first;
    HIPCHK_AT(who, launch_knn_query(k, mc, s));
    KnnCorrPredArgs a;
    a.rows = mc; a.mc = c.m_cand; a.hops = c.hops; a.m = m; a.row0 = row0;
    a.first = d_first; a.all = c.hops > 1 ? V->corr_all.get() : nullptr;
    a.aosC = aosC; a.aosP = drec; a.gr = gr;
    a.nn = d_nn; a.ldn = (size_t)mc; a.tab = d_tab; a.fail = f->dinfo;
    HIPCHK_AT(who, launch_knn_corr_pred(a, s));
    return 0;
}

extern "C" int cocons_vecchia_neighbours_corr_pred(cocons_fit *f, const double *theta, int mp, const double *locs_pred,
                                                   const double *X_pred, int m_cand, int hops, int m, int *nn_out)
{
    const char *who = "cocons_vecchia_neighbours_corr_pred";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (mp > 0 && !nn_out) return fail(-1, "%s: bad argument (mp < 0 or a null pointer)", who);
    int none = 0;
    CorrPredSource c;
    c.m_cand = m_cand; c.hops = hops; c.nn_out = nn_out ? nn_out : &none;      // (mp = 0: nothing is written)
    return vecchia_predict_impl(who, f, theta, nullptr, 0, mp, locs_pred, X_pred, m, nullptr, true, nullptr, nullptr, &c);
}

extern "C" int cocons_vecchia_predict_corr_knn(cocons_fit *f, const double *theta, const double *mean, int z_col, int mp,
                                               const double *locs_pred, const double *X_pred, int m_cand, int hops, int m_pred,
                                               double *stochastic, double *quadform)
{
    CorrPredSource c;
    c.m_cand = m_cand; c.hops = hops;
    return vecchia_predict_impl("cocons_vecchia_predict_corr_knn", f, theta, mean, z_col, mp, locs_pred, X_pred, m_pred, nullptr,
                                true, stochastic, quadform, &c);
}

extern "C" cocons_fit *cocons_fit_create_vecchia_grouped_corr_knn(int n, int p, int r, const double *locs, const double *X,
                                                                  const double *z, const double *smooth_limits, int device,
                                                                  const double *theta, int m_cand, int hops, int m,
                                                                  int max_rows, int max_rounds)
{
    const char *who = "cocons_fit_create_vecchia_grouped_corr_knn";
    if (!theta) { fail(-1, "%s: null argument", who); return nullptr; }
    if (p < 1 || p > COCONS_P_MAX) { fail(-1, "%s: bad argument (p = %d)", who, p); return nullptr; }
    if (corr_check_shape(who, m_cand, hops, m) || corr_check_theta(who, theta, p)) return nullptr;
    CorrTableStep step;
    step.theta = theta; step.m_cand = m_cand; step.hops = hops;
    return vecchia_create_grouped_device(who, n, p, r, locs, X, z, smooth_limits, device, m, max_rows, max_rounds, step);
}

extern "C" int cocons_vecchia_neighbours_corr(cocons_fit *f, const double *theta, int m_cand, int hops, int m, int *nn_out)
{
    const char *who = "cocons_vecchia_neighbours_corr";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !nn_out) return fail(-1, "%s: null argument", who);
    if (int rc = corr_check_shape(who, m_cand, hops, m)) return rc;
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (int rc = corr_check_theta(who, theta, f->p)) return rc;
    const size_t count = (size_t)f->n * m;
    DevBuf<int> dnn;
    HIPCHK_AT(who, dnn.alloc(count));
    if (int rc = corr_table(who, f, theta, m_cand, hops, m, dnn, nullptr)) return rc;
    // (into staging of the call: the caller's table stays untouched on every failure)
    std::vector<int> h(count);
    HIPCHK_AT(who, hipMemcpyAsync(h.data(), dnn, count * sizeof(int), hipMemcpyDeviceToHost, f->stream));
    HIPCHK_AT(who, hipStreamSynchronize(f->stream));
    std::copy(h.begin(), h.end(), nn_out);
    return 0;
}

extern "C" int cocons_debug_knn_corr_phases(cocons_fit *f, const double *theta, int m_cand, int hops, int m, double *ms3)
{
    const char *who = "cocons_debug_knn_corr_phases";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !ms3) return fail(-1, "%s: null argument", who);
    if (int rc = corr_check_shape(who, m_cand, hops, m)) return rc;
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (int rc = corr_check_theta(who, theta, f->p)) return rc;
    DevBuf<int> dnn;
    HIPCHK_AT(who, dnn.alloc((size_t)f->n * m));
    double ms[3] = {0.0, 0.0, 0.0};
    if (int rc = corr_table(who, f, theta, m_cand, hops, m, dnn, nullptr, ms)) return rc;
    std::copy(ms, ms + 3, ms3);
    return 0;
}

extern "C" cocons_fit *cocons_fit_create_vecchia_corr_knn(int n, int p, int r, const double *locs, const double *X, const double *z,
                                                          const double *smooth_limits, int device, const double *theta,
                                                          int m_cand, int hops, int m)
{
    const char *who = "cocons_fit_create_vecchia_corr_knn";
    if (!theta) { fail(-1, "%s: null argument", who); return nullptr; }
    if (p < 1 || p > COCONS_P_MAX) { fail(-1, "%s: bad argument (p = %d)", who, p); return nullptr; }
    if (corr_check_shape(who, m_cand, hops, m) || corr_check_theta(who, theta, p)) return nullptr;
    CorrKnnSource src;
    src.theta = theta; src.m_cand = m_cand; src.hops = hops; src.m = m;
    cocons_fit *f = vecchia_create_impl(who, n, p, r, locs, X, z, smooth_limits, device, m, nullptr, true, &src);
    if (!f) (void)hipGetLastError();             // (a refused device is this call's alone: the next launch must not find it)
    return f;
}
