// api_vecchia_cov.hip -- C ABI of U^-T on a Vecchia fit: cocons_vecchia_unwhiten_t, the inverse of
// cocons_vecchia_whiten_t; cocons_vecchia_cov_mult, the model's own covariance (U_pp' U_pp)^-1 = U_pp^-1 U_pp^-T applied to
// columns; cocons_vecchia_cov_cols, columns of it; cocons_vecchia_schedule_t, the transposed level schedule they run on.  One
// call is: the transposed lists unless the handle holds them, the records for theta and the coefficient launch (per row or per
// block of the plan), the status word home -- a failing block ends the call there --, the transposed schedule of
// (table, n_fixed) unless the handle holds it, the descending solve in place on the columns -- one launch per level and tier
// or per run of small levels, in the order of the handle's stream -- and, for the covariance entries, 4v's forward solve with
// the fixed rows of x at zero.
#include "fit.hpp"

namespace {

bool solve_t_fuse()
{
    const char *e = getenv("COCONS_VECCHIA_SOLVE_T_FUSE");
    return !e || atoi(e) != 0;
}

// The tier threshold: VECCHIA_SOLVE_T_WIDE.  COCONS_VECCHIA_SOLVE_T_WIDE=<rows> moves it for a measurement
// (tools/vecchia_cov_timing.py), read when a schedule is made; a list's sum then follows the rule of the tier it lands in.
int solve_t_wide()
{
    const char *e = getenv("COCONS_VECCHIA_SOLVE_T_WIDE");
    return e && atoi(e) >= 0 ? atoi(e) : VECCHIA_SOLVE_T_WIDE;
}

// The launches of one solve of c columns: {first level, one past the last, kind}.  With the switch on, a run of levels
// without wide rows, of at most VECCHIA_SOLVE_T_FUSE_ITEMS (row, column group) items each and of at most
// VECCHIA_SOLVE_T_FUSE_ROWS rows together is one fused launch; every other level is a launch for its one-wave rows and one for
// its wide rows, whichever it has.
enum { SOLVE_T_FUSED, SOLVE_T_WAVE, SOLVE_T_WIDE };
struct SolveTLaunch { int lv0, lv1, kind; };

std::vector<SolveTLaunch> solve_t_plan(const std::vector<int> &hoff, bool fuse, int c)
{
    std::vector<SolveTLaunch> plan;
    const int depth = hoff.empty() ? 0 : (int)(hoff.size() - 1) / 2;
    const long long groups = (c + VECCHIA_SOLVE_T_COLS - 1) / VECCHIA_SOLVE_T_COLS;
    auto narrow = [&](int lv) { return hoff[2 * lv + 1] - hoff[2 * lv]; };
    auto wide = [&](int lv) { return hoff[2 * lv + 2] - hoff[2 * lv + 1]; };
    for (int lv = 0; lv < depth;) {
        int end = lv;
        while (fuse && end < depth && wide(end) == 0 && narrow(end) * groups <= VECCHIA_SOLVE_T_FUSE_ITEMS &&
               hoff[2 * end + 1] - hoff[2 * lv] <= VECCHIA_SOLVE_T_FUSE_ROWS)
            ++end;
        if (end > lv) { plan.push_back({lv, end, SOLVE_T_FUSED}); lv = end; continue; }
        if (narrow(lv) > 0) plan.push_back({lv, lv + 1, SOLVE_T_WAVE});
        if (wide(lv) > 0) plan.push_back({lv, lv + 1, SOLVE_T_WIDE});
        ++lv;
    }
    return plan;
}

// The transposed schedule of (table, n_fixed) on the handle: levels by push-form sweeps over the forward table, then the rows
// ordered by (level, tier).  The transposed lists are on the handle (the tiers read their lengths).
int solve_t_schedule(cocons_fit *f, const char *who, int n_fixed)
{
    VecchiaState *V = f->vecchia.get();
    if (!V->solve_t) V->solve_t.reset(new VecchiaSolveTState());
    VecchiaSolveTState *S = V->solve_t.get();
    const int wide = solve_t_wide();
    if (S->n_fixed == n_fixed && S->wide == wide) return 0;
    const int n = f->n, rows = n - n_fixed;
    hipStream_t s = f->stream;
    S->n_fixed = -1;
    HIPCHK_AT(who, S->level.reserve((size_t)n, s, nullptr));
    HIPCHK_AT(who, S->key.reserve((size_t)n, s, nullptr));
    HIPCHK_AT(who, S->order.reserve((size_t)n, s, nullptr));
    HIPCHK_AT(who, S->off.reserve(2 * (size_t)n + 2, s, nullptr));
    HIPCHK_AT(who, S->word.reserve(2, s, nullptr));
    launch_vecchia_tlevel_init(n, n_fixed, S->level, s);
    // a level is at most `rows`, and a sweep that changes something raises at least one row: rows + 1 sweeps always suffice
    int hword[2] = {1, 0};
    for (long long done = 0; hword[0] && done <= (long long)rows + VECCHIA_SIM_SWEEPS; done += VECCHIA_SIM_SWEEPS) {
        for (int k = 0; k < VECCHIA_SIM_SWEEPS; ++k) {
            if (k == VECCHIA_SIM_SWEEPS - 1) HIPCHK_AT(who, hipMemsetAsync(S->word, 0, 2 * sizeof(int), s));
            launch_vecchia_tlevel_sweep(V->nbr, V->m, n, n_fixed, S->level, S->word, s);
        }
        HIPCHK_AT(who, hipMemcpyAsync(hword, S->word, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipGetLastError());
        HIPCHK_AT(who, hipStreamSynchronize(s));
    }
    if (hword[0]) return fail(-2, "%s: the transposed levels did not settle in %d sweeps", who, rows + 2 * VECCHIA_SIM_SWEEPS);
    // the keys, their counts into off, the largest key into word[1]; the prefix sum of the counts on the host
    launch_vecchia_tkey(S->level, V->cv->ptr, n, n_fixed, wide, S->key, s);
    HIPCHK_AT(who, hipMemsetAsync(S->off, 0, (2 * (size_t)n + 2) * sizeof(int), s));
    launch_vecchia_level_count(S->key, n, n_fixed, S->off, S->word + 1, s);
    HIPCHK_AT(who, hipMemcpyAsync(hword, S->word, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipGetLastError());
    HIPCHK_AT(who, hipStreamSynchronize(s));
    const int depth = (hword[1] + 1) / 2;
    if (depth < 1 || depth > rows) return fail(-2, "%s: a transposed depth of %d for %d rows", who, depth, rows);
    std::vector<int> cnt(2 * (size_t)depth);
    HIPCHK_AT(who, hipMemcpy(cnt.data(), S->off, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
    S->hoff.assign(2 * (size_t)depth + 1, 0);
    S->widest = 0;
    S->wide_rows = 0;
    for (int l = 0; l < depth; ++l) {
        S->hoff[2 * l + 1] = S->hoff[2 * l] + cnt[2 * l];
        S->hoff[2 * l + 2] = S->hoff[2 * l + 1] + cnt[2 * l + 1];
        S->widest = std::max(S->widest, cnt[2 * l] + cnt[2 * l + 1]);
        S->wide_rows += cnt[2 * l + 1];
    }
    if (S->hoff[2 * depth] != rows) return fail(-2, "%s: the transposed levels hold %d of %d rows", who, S->hoff[2 * depth], rows);
    // the scatter moves its cursors: the offsets go up twice, before it and after it
    HIPCHK_AT(who, hipMemcpyAsync(S->off, S->hoff.data(), S->hoff.size() * sizeof(int), hipMemcpyHostToDevice, s));
    launch_vecchia_level_scatter(S->key, n, n_fixed, S->off, S->order, s);
    HIPCHK_AT(who, hipMemcpyAsync(S->off, S->hoff.data(), S->hoff.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK_AT(who, hipGetLastError());
    HIPCHK_AT(who, hipStreamSynchronize(s));
    S->n_fixed = n_fixed;
    S->wide = wide;
    return 0;
}

// v = U_pp^-T w in place on the columns in V->B (rows n_fixed .. n - 1, leading dimension n - n_fixed)
void solve_t(cocons_fit *f, int n_fixed, int c)
{
    VecchiaState *V = f->vecchia.get();
    VecchiaSolveTState *S = V->solve_t.get();
    VecchiaSolveTArgs a;
    a.m = V->m; a.ptr = V->cv->ptr; a.rows = V->cv->rows; a.place = V->cv->place; a.coef = V->sim->coef;
    a.order = S->order; a.off = S->off;
    a.x = V->B; a.ldx = (size_t)(f->n - n_fixed); a.row0 = n_fixed; a.c = c;
    for (const SolveTLaunch &l : solve_t_plan(S->hoff, solve_t_fuse(), c)) {
        const int lv = l.lv0;
        if (l.kind == SOLVE_T_FUSED) launch_vecchia_solve_t_fused(a, l.lv0, l.lv1, f->stream);
        else if (l.kind == SOLVE_T_WAVE) launch_vecchia_solve_t_level(a, S->hoff[2 * lv], S->hoff[2 * lv + 1] - S->hoff[2 * lv], f->stream);
        else launch_vecchia_solve_t_wide(a, S->hoff[2 * lv + 1], S->hoff[2 * lv + 2] - S->hoff[2 * lv + 1], f->stream);
    }
}

// Events around the three phases (cocons_debug_vecchia_solve_t_phases); off: nothing is created or recorded
struct CovMarks {
    bool on;
    hipStream_t s;
    hipEvent_t ev[6] = {};
    CovMarks(bool on_, hipStream_t s_) : on(on_), s(s_)
    {
        if (on) for (hipEvent_t &e : ev) (void)hipEventCreate(&e);
    }
    ~CovMarks()
    {
        if (on) for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    void mark(int i) { if (on) (void)hipEventRecord(ev[i], s); }
    double ms(int i)
    {
        float t = 0.0f;
        if (on && hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]) != hipSuccess) { (void)hipGetLastError(); t = 0.0f; }
        return (double)t;
    }
};

// The three entries' body behind their own checks.  B: (n - n_fixed) x c host columns, or null with idx0: c 0-based rows of the
// table, the unit columns made on the device.  forward: U_pp^-1 behind U_pp^-T.  ms3 (may be null): the device milliseconds of
// the coefficient phase, of the transposed schedule and of the transposed solve's launches.
int cov_impl(const char *who, cocons_fit *f, const double *theta, bool grouped, int n_fixed, int c, const double *B,
             const std::vector<int> *idx0, bool forward, double *out, double *ms3 = nullptr)
{
    VecchiaState *V = f->vecchia.get();
    const size_t n = (size_t)f->n, rows = n - (size_t)n_fixed;
    hipStream_t s = f->stream;
    if (int rc = vecchia_t_build(f, who)) return rc;
    if (!V->solve_t) V->solve_t.reset(new VecchiaSolveTState());
    HIPCHK_AT(who, V->B.reserve(rows * c, s, nullptr));
    if (forward) HIPCHK_AT(who, V->W.reserve(n * (1 + (size_t)c), s, nullptr));
    if (idx0) HIPCHK_AT(who, V->solve_t->idx.reserve((size_t)c, s, nullptr));
    CovMarks marks(ms3 != nullptr, s);
    marks.mark(0);
    if (int st = vecchia_sim_coefs(f, who, theta, n_fixed, grouped)) return st;     // a failing block: its row, nothing written
    marks.mark(1);
    marks.mark(2);
    if (int rc = solve_t_schedule(f, who, n_fixed)) return rc;
    marks.mark(3);
    if (forward) if (int rc = vecchia_sim_schedule(f, who, n_fixed)) return rc;
    if (idx0) {
        HIPCHK_AT(who, hipMemcpyAsync(V->solve_t->idx, idx0->data(), (size_t)c * sizeof(int), hipMemcpyHostToDevice, s));
        launch_vecchia_unit_cols(V->solve_t->idx, c, (int)rows, n_fixed, V->B, rows, s);
    } else {
        HIPCHK_AT(who, upload_canon(V->B, B, rows * c, s));
    }
    marks.mark(4);
    solve_t(f, n_fixed, c);
    marks.mark(5);
    std::vector<double> h;
    if (forward) {
        // the fixed rows of x at zero: their terms leave the rows behind them as they are
        HIPCHK_AT(who, hipMemsetAsync(V->W, 0, n * c * sizeof(double), s));
        vecchia_sim_solve(f, n_fixed, c);
        h.resize(n * c);
        HIPCHK_AT(who, hipMemcpyAsync(h.data(), V->W, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    } else {
        h.resize(rows * c);
        HIPCHK_AT(who, hipMemcpyAsync(h.data(), V->B, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIPCHK_AT(who, hipGetLastError());
    HIPCHK_AT(who, hipStreamSynchronize(s));
    if (forward) for (int q = 0; q < c; ++q) memcpy(out + (size_t)q * rows, h.data() + (size_t)q * n + n_fixed, rows * sizeof(double));
    else memcpy(out, h.data(), h.size() * sizeof(double));
    if (ms3) for (int i = 0; i < 3; ++i) ms3[i] = marks.ms(i);
    return 0;
}

int check_grouped(const char *who, int grouped)
{
    if (grouped != 0 && grouped != 1) return fail(-1, "%s: grouped = %d (0 or 1 expected)", who, grouped);
    return 0;
}

int check_fixed(cocons_fit *f, const char *who, int n_fixed)
{
    if (n_fixed < 0 || n_fixed >= f->n) return fail(-1, "%s: n_fixed = %d is outside 0 .. %d", who, n_fixed, f->n - 1);
    return 0;
}

}  // namespace

static int unwhiten_t_impl(const char *who, cocons_fit *f, const double *theta, int grouped, int c, const double *W, double *out,
                           bool timed, double *ms3)
{
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !W || !out || (timed && !ms3)) return fail(-1, "%s: null argument", who);
    if (c < 1) return fail(-1, "%s: c = %d (at least one column expected)", who, c);
    if (int rc = check_grouped(who, grouped)) return rc;
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (grouped) if (int rc = vecchia_need_plan(f, who)) return rc;
    return cov_impl(who, f, theta, grouped != 0, 0, c, W, nullptr, false, out, timed ? ms3 : nullptr);
}

extern "C" int cocons_vecchia_unwhiten_t(cocons_fit *f, const double *theta, int grouped, int c, const double *W, double *out)
{
    return unwhiten_t_impl("cocons_vecchia_unwhiten_t", f, theta, grouped, c, W, out, false, nullptr);
}

extern "C" int cocons_debug_vecchia_solve_t_phases(cocons_fit *f, const double *theta, int grouped, int c, const double *W,
                                                   double *out, double *ms3)
{
    return unwhiten_t_impl("cocons_debug_vecchia_solve_t_phases", f, theta, grouped, c, W, out, true, ms3);
}

extern "C" int cocons_vecchia_cov_mult(cocons_fit *f, const double *theta, int grouped, int n_fixed, int c, const double *B,
                                       double *out)
{
    const char *who = "cocons_vecchia_cov_mult";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !B || !out) return fail(-1, "%s: null argument", who);
    if (c < 1) return fail(-1, "%s: c = %d (at least one column expected)", who, c);
    if (int rc = check_grouped(who, grouped)) return rc;
    if (n_fixed < 0) return fail(-1, "%s: n_fixed = %d is outside 0 .. n - 1", who, n_fixed);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (grouped) if (int rc = vecchia_need_plan(f, who)) return rc;
    if (int rc = check_fixed(f, who, n_fixed)) return rc;
    return cov_impl(who, f, theta, grouped != 0, n_fixed, c, B, nullptr, true, out);
}

extern "C" int cocons_vecchia_cov_cols(cocons_fit *f, const double *theta, int grouped, int n_fixed, int nidx, const int *idx,
                                       double *out)
{
    const char *who = "cocons_vecchia_cov_cols";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !idx || !out) return fail(-1, "%s: null argument", who);
    if (nidx < 1) return fail(-1, "%s: nidx = %d (at least one column expected)", who, nidx);
    if (int rc = check_grouped(who, grouped)) return rc;
    if (n_fixed < 0) return fail(-1, "%s: n_fixed = %d is outside 0 .. n - 1", who, n_fixed);
    for (int q = 0; q < nidx; ++q)
        if (idx[q] <= n_fixed) return fail(-1, "%s: idx[%d] = %d is outside n_fixed + 1 .. n (n_fixed = %d)", who, q, idx[q], n_fixed);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (grouped) if (int rc = vecchia_need_plan(f, who)) return rc;
    if (int rc = check_fixed(f, who, n_fixed)) return rc;
    std::vector<int> idx0((size_t)nidx);
    for (int q = 0; q < nidx; ++q) {
        if (idx[q] > f->n) return fail(-1, "%s: idx[%d] = %d is outside %d .. %d", who, q, idx[q], n_fixed + 1, f->n);
        idx0[q] = idx[q] - 1;
    }
    return cov_impl(who, f, theta, grouped != 0, n_fixed, nidx, nullptr, &idx0, true, out);
}

// out4 = {depth, rows of the largest level, launches of one solve of one column under the current switch, device bytes of the
// transposed schedule}
extern "C" int cocons_vecchia_schedule_t(cocons_fit *f, int n_fixed, int *tlevels, long long *out4)
{
    const char *who = "cocons_vecchia_schedule_t";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!out4) return fail(-1, "%s: null argument", who);
    if (n_fixed < 0) return fail(-1, "%s: n_fixed = %d is outside 0 .. n - 1", who, n_fixed);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (int rc = check_fixed(f, who, n_fixed)) return rc;
    if (int rc = vecchia_t_build(f, who)) return rc;
    if (int rc = solve_t_schedule(f, who, n_fixed)) return rc;
    VecchiaSolveTState *S = f->vecchia->solve_t.get();
    if (tlevels) {
        std::vector<int> h((size_t)f->n);
        HIPCHK_AT(who, hipMemcpy(h.data(), S->level, h.size() * sizeof(int), hipMemcpyDeviceToHost));
        memcpy(tlevels, h.data(), h.size() * sizeof(int));
    }
    out4[0] = S->depth(); out4[1] = S->widest;
    out4[2] = (long long)solve_t_plan(S->hoff, solve_t_fuse(), 1).size();
    out4[3] = S->bytes();
    return 0;
}

// out4 = {VECCHIA_SOLVE_T_WIDE, threads of the wide tier's workgroup, VECCHIA_SOLVE_T_COLS, VECCHIA_SOLVE_T_FUSE_ITEMS}
extern "C" int cocons_debug_vecchia_solve_t_tiers(int *out4)
{
    if (!out4) return fail(-1, "cocons_debug_vecchia_solve_t_tiers: null argument");
    out4[0] = VECCHIA_SOLVE_T_WIDE; out4[1] = VECCHIA_SOLVE_T_WIDE_THREADS;
    out4[2] = VECCHIA_SOLVE_T_COLS; out4[3] = VECCHIA_SOLVE_T_FUSE_ITEMS;
    return 0;
}
