// api_vecchia_sim.hip -- C ABI of U^-1 on a Vecchia fit: cocons_vecchia_unwhiten, the inverse of
// cocons_vecchia_whiten; cocons_sim_vecchia, fields and conditional draws of the Vecchia model; cocons_vecchia_schedule, the
// level schedule they run on; and cocons_debug_vecchia_sim_phases, which times a call's three phases by events.  One call is:
// the records for theta and the coefficient launch (one wave per row, no dependency), the status word home -- a failing block
// ends the call there --, the schedule of (table, n_fixed) unless the handle holds it, and the solve: one launch per level or
// per run of small levels, in the order of the handle's stream.  The bodies are shared with the grouped entries of
// api_vecchia_group.hip, whose coefficient launch is one workgroup per block of the handle's plan.
#include "fit.hpp"

// Events around the three phases (cocons_debug_vecchia_sim_phases); off: nothing is created or recorded
struct SimMarks {
    bool on;
    hipStream_t s;
    hipEvent_t ev[6] = {};
    SimMarks(bool on_, hipStream_t s_) : on(on_), s(s_)
    {
        if (on) for (hipEvent_t &e : ev) (void)hipEventCreate(&e);
    }
    ~SimMarks()
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

static bool sim_fuse()
{
    const char *e = getenv("COCONS_VECCHIA_SIM_FUSE");
    return !e || atoi(e) != 0;
}

// The launches of one solve of c columns over the levels' offsets: {first level, one past the last} -- with the switch on, a
// run of levels of at most VECCHIA_SIM_FUSE_ITEMS (row, column) pairs each is a fused launch (one workgroup serves a level in
// one pass); every other level is a launch of its own.
struct SimLaunch { int lv0, lv1; bool fused; };

static std::vector<SimLaunch> sim_plan(const std::vector<int> &hoff, bool fuse, int c)
{
    std::vector<SimLaunch> plan;
    const int depth = hoff.empty() ? 0 : (int)hoff.size() - 1;
    for (int lv = 0; lv < depth;) {
        int end = lv;
        while (fuse && end < depth && end - lv < VECCHIA_SIM_FUSE_LEVELS && (long long)(hoff[end + 1] - hoff[end]) * c <= VECCHIA_SIM_FUSE_ITEMS) ++end;
        if (end > lv) { plan.push_back({lv, end, true}); lv = end; }
        else { plan.push_back({lv, lv + 1, false}); ++lv; }
    }
    return plan;
}

// The schedule of (table, n_fixed) on the handle: levels by relaxation sweeps, then the rows ordered by level.
int vecchia_sim_schedule(cocons_fit *f, const char *who, int n_fixed)
{
    VecchiaState *V = f->vecchia.get();
    if (!V->sim) V->sim.reset(new VecchiaSimState());
    VecchiaSimState *S = V->sim.get();
    if (S->n_fixed == n_fixed) return 0;
    const int n = f->n, rows = n - n_fixed;
    hipStream_t s = f->stream;
    S->n_fixed = -1;
    HIPCHK_AT(who, S->level.reserve((size_t)n, s, nullptr));
    HIPCHK_AT(who, S->order.reserve((size_t)n, s, nullptr));
    HIPCHK_AT(who, S->off.reserve((size_t)n + 2, s, nullptr));
    HIPCHK_AT(who, S->word.reserve(2, s, nullptr));
    HIPCHK_AT(who, hipMemsetAsync(S->level, 0, (size_t)n * sizeof(int), s));
    // a level is at most `rows`, and a sweep that changes something raises at least one row: rows + 1 sweeps always suffice
    int hword[2] = {1, 0};
    for (long long done = 0; hword[0] && done <= (long long)rows + VECCHIA_SIM_SWEEPS; done += VECCHIA_SIM_SWEEPS) {
        for (int k = 0; k < VECCHIA_SIM_SWEEPS; ++k) {
            if (k == VECCHIA_SIM_SWEEPS - 1) HIPCHK_AT(who, hipMemsetAsync(S->word, 0, 2 * sizeof(int), s));
            launch_vecchia_level_sweep(V->nbr, V->m, n, n_fixed, S->level, S->word, s);
        }
        HIPCHK_AT(who, hipMemcpyAsync(hword, S->word, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipGetLastError());
        HIPCHK_AT(who, hipStreamSynchronize(s));
    }
    if (hword[0]) return fail(-2, "%s: the levels did not settle in %d sweeps", who, rows + 2 * VECCHIA_SIM_SWEEPS);
    // the counts per level into off, the depth into word[1]; the prefix sum of the depth counts on the host
    HIPCHK_AT(who, hipMemsetAsync(S->off, 0, ((size_t)n + 2) * sizeof(int), s));
    launch_vecchia_level_count(S->level, n, n_fixed, S->off, S->word + 1, s);
    HIPCHK_AT(who, hipMemcpyAsync(hword, S->word, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipGetLastError());
    HIPCHK_AT(who, hipStreamSynchronize(s));
    const int depth = hword[1];
    if (depth < 1 || depth > rows) return fail(-2, "%s: a depth of %d for %d rows", who, depth, rows);
    std::vector<int> cnt((size_t)depth);
    HIPCHK_AT(who, hipMemcpy(cnt.data(), S->off, (size_t)depth * sizeof(int), hipMemcpyDeviceToHost));
    S->hoff.assign((size_t)depth + 1, 0);
    S->widest = 0;
    for (int l = 0; l < depth; ++l) {
        S->hoff[l + 1] = S->hoff[l] + cnt[l];
        S->widest = std::max(S->widest, cnt[l]);
    }
    if (S->hoff[depth] != rows) return fail(-2, "%s: the levels hold %d of %d rows", who, S->hoff[depth], rows);
    // the scatter moves its cursors: the offsets go up twice, before it and after it
    HIPCHK_AT(who, hipMemcpyAsync(S->off, S->hoff.data(), S->hoff.size() * sizeof(int), hipMemcpyHostToDevice, s));
    launch_vecchia_level_scatter(S->level, n, n_fixed, S->off, S->order, s);
    HIPCHK_AT(who, hipMemcpyAsync(S->off, S->hoff.data(), S->hoff.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK_AT(who, hipGetLastError());
    HIPCHK_AT(who, hipStreamSynchronize(s));
    S->n_fixed = n_fixed;
    return 0;
}

// The coefficients of the rows n_fixed .. n - 1 for theta into S->coef and the status word home: 0, the smallest failing
// 1-based row, or < 0.  grouped: one workgroup per block of the handle's plan instead of one wavefront per row
int vecchia_sim_coefs(cocons_fit *f, const char *who, const double *theta, int n_fixed, bool grouped)
{
    VecchiaState *V = f->vecchia.get();
    if (!V->sim) V->sim.reset(new VecchiaSimState());
    HIPCHK_AT(who, V->sim->coef.reserve((size_t)f->n * (V->m + 1), f->stream, nullptr));
    if (int rc = reset_info(f)) return rc;
    const ModeSel ms = vecchia_records(f, theta, 0, V->aos);
    if (grouped) {
        const VecchiaGroupState *G = V->grp.get();
        VecchiaGroupArgs g;
        g.blocks = G->blocks; g.kb = G->maxrows;
        g.off = G->off; g.rows = G->rows; g.order = G->by_size ? G->order.get() : nullptr; g.mask = G->mask;
        g.aosK = V->aos; g.gr = ms.gr; g.nu_fixed = ms.nu_fixed;
        g.coef = V->sim->coef; g.ldc = (size_t)V->m + 1; g.row0 = n_fixed;
        g.fail = f->dinfo;
        launch_vecchia_group_coefs(ms.mode, g, f->stream);
        return vecchia_status(f, who);
    }
    VecchiaArgs a;
    a.rows = f->n - n_fixed; a.obs0 = n_fixed; a.m = V->m; a.kb = V->m + 1; a.nbr = V->nbr; a.aosK = V->aos;
    a.gr = ms.gr; a.nu_fixed = ms.nu_fixed;
    a.rec = V->sim->coef;
    a.fail = f->dinfo;
    launch_vecchia_coefs(ms.mode, a, f->stream);
    return vecchia_status(f, who);
}

// x (n x c in V->W, leading dimension n) from the columns in V->B (rows n_fixed .. n - 1, leading dimension n - n_fixed); the
// fixed rows of x are in place
void vecchia_sim_solve(cocons_fit *f, int n_fixed, int c)
{
    VecchiaState *V = f->vecchia.get();
    VecchiaSimState *S = V->sim.get();
    VecchiaSimArgs a;
    a.nbr = V->nbr; a.m = V->m; a.coef = S->coef; a.order = S->order; a.off = S->off;
    a.W = V->B; a.ldw = (size_t)(f->n - n_fixed); a.w_row0 = n_fixed;
    a.x = V->W; a.ldx = (size_t)f->n; a.c = c;
    for (const SimLaunch &l : sim_plan(S->hoff, sim_fuse(), c)) {
        if (l.fused) launch_vecchia_sim_fused(a, l.lv0, l.lv1, f->stream);
        else launch_vecchia_sim_level(a, S->hoff[l.lv0], S->hoff[l.lv0 + 1] - S->hoff[l.lv0], f->stream);
    }
}

// mean == NULL: cocons_vecchia_unwhiten (n_fixed = 0, no trend).  E: (n - n_fixed) x c, used as given.
static int sim_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, const double *mean, int n_fixed, int z_col,
                    int c, const double *E, double *out, double *phases)
{
    VecchiaState *V = f->vecchia.get();
    const size_t n = (size_t)f->n, rows = n - (size_t)n_fixed;
    hipStream_t s = f->stream;
    SimMarks marks(phases != nullptr, s);
    HIPCHK_AT(who, V->B.reserve(rows * c, s, nullptr));
    HIPCHK_AT(who, V->W.reserve(n * (1 + c), s, nullptr));
    double hmean[COCONS_P_MAX] = {};
    if (mean) for (int i = 0; i < f->p; ++i) hmean[i] = canon_nan(mean[i]);
    marks.mark(0);
    if (int st = vecchia_sim_coefs(f, who, theta, n_fixed, grouped)) return st;
    marks.mark(1);
    marks.mark(2);
    if (int rc = vecchia_sim_schedule(f, who, n_fixed)) return rc;
    marks.mark(3);
    HIPCHK_AT(who, upload_canon(V->B, E, rows * c, s));
    marks.mark(4);
    if (n_fixed > 0)
        launch_vecchia_sim_ends(true, f->n, f->p, n_fixed, c, f->dX, f->n, hmean, f->dz + (size_t)z_col * n, V->W, n, nullptr, 0, s);
    vecchia_sim_solve(f, n_fixed, c);
    marks.mark(5);
    // the result: x itself, or the trend added into the columns' buffer (they are used up)
    const double *res = V->W;
    if (mean) {
        launch_vecchia_sim_ends(false, f->n, f->p, n_fixed, c, f->dX, f->n, hmean, nullptr, V->W, n, V->B, rows, s);
        res = V->B;
    }
    std::vector<double> h(rows * c);
    HIPCHK_AT(who, hipMemcpyAsync(h.data(), res, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipGetLastError());
    HIPCHK_AT(who, hipStreamSynchronize(s));
    memcpy(out, h.data(), h.size() * sizeof(double));
    if (phases) for (int i = 0; i < 3; ++i) phases[i] = marks.ms(i);
    return 0;
}

// cocons_vecchia_unwhiten and cocons_debug_vecchia_sim_phases (timed), and their grouped twins
int vecchia_unwhiten_impl(const char *who, bool grouped, bool timed, cocons_fit *f, const double *theta, int c, const double *W,
                          double *out, double *ms3)
{
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !W || !out || (timed && !ms3)) return fail(-1, "%s: null argument", who);
    if (c < 1) return fail(-1, "%s: c = %d (at least one column expected)", who, c);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (grouped) if (int rc = vecchia_need_plan(f, who)) return rc;
    return sim_impl(who, grouped, f, theta, nullptr, 0, 0, c, W, out, timed ? ms3 : nullptr);
}

extern "C" int cocons_vecchia_unwhiten(cocons_fit *f, const double *theta, int c, const double *W, double *out)
{
    return vecchia_unwhiten_impl("cocons_vecchia_unwhiten", false, false, f, theta, c, W, out, nullptr);
}

extern "C" int cocons_debug_vecchia_sim_phases(cocons_fit *f, const double *theta, int c, const double *W, double *out,
                                               double *ms3)
{
    return vecchia_unwhiten_impl("cocons_debug_vecchia_sim_phases", false, true, f, theta, c, W, out, ms3);
}

static int sim_check_fixed(cocons_fit *f, const char *who, int n_fixed)
{
    if (n_fixed < 0 || n_fixed >= f->n) return fail(-1, "%s: n_fixed = %d is outside 0 .. %d", who, n_fixed, f->n - 1);
    return 0;
}

// cocons_sim_vecchia and its grouped twin
int vecchia_sim_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, const double *mean, int n_fixed, int z_col,
                     int nsim, const double *iiderrors, double *out)
{
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !mean || !iiderrors || !out) return fail(-1, "%s: null argument", who);
    if (nsim < 1) return fail(-1, "%s: nsim = %d (at least one field expected)", who, nsim);
    if (n_fixed < 0) return fail(-1, "%s: n_fixed = %d is outside 0 .. n - 1", who, n_fixed);
    if (z_col < 0) return fail(-1, "%s: z_col = %d is outside the realisations", who, z_col);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (grouped) if (int rc = vecchia_need_plan(f, who)) return rc;
    if (int rc = sim_check_fixed(f, who, n_fixed)) return rc;
    if (z_col < 0 || z_col >= f->r) return fail(-1, "%s: z_col = %d is outside 0 .. %d", who, z_col, f->r - 1);
    return sim_impl(who, grouped, f, theta, mean, n_fixed, z_col, nsim, iiderrors, out, nullptr);
}

extern "C" int cocons_sim_vecchia(cocons_fit *f, const double *theta, const double *mean, int n_fixed, int z_col, int nsim,
                                  const double *iiderrors, double *out)
{
    return vecchia_sim_impl("cocons_sim_vecchia", false, f, theta, mean, n_fixed, z_col, nsim, iiderrors, out);
}

// out4 = {depth, rows of the largest level, launches of one solve of one column, device bytes of the schedule and of the n (m + 1)
// coefficients a solve holds}
extern "C" int cocons_vecchia_schedule(cocons_fit *f, int n_fixed, int *levels, long long *out4)
{
    const char *who = "cocons_vecchia_schedule";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!out4) return fail(-1, "%s: null argument", who);
    if (n_fixed < 0) return fail(-1, "%s: n_fixed = %d is outside 0 .. n - 1", who, n_fixed);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (int rc = sim_check_fixed(f, who, n_fixed)) return rc;
    if (int rc = vecchia_sim_schedule(f, who, n_fixed)) return rc;
    VecchiaSimState *S = f->vecchia->sim.get();
    if (levels) {
        std::vector<int> h((size_t)f->n);
        HIPCHK_AT(who, hipMemcpy(h.data(), S->level, h.size() * sizeof(int), hipMemcpyDeviceToHost));
        memcpy(levels, h.data(), h.size() * sizeof(int));
    }
    out4[0] = S->depth(); out4[1] = S->widest;
    out4[2] = (long long)sim_plan(S->hoff, sim_fuse(), 1).size();
    out4[3] = S->schedule_bytes() + (long long)((size_t)f->n * (f->vecchia->m + 1) * sizeof(double));
    return 0;
}
