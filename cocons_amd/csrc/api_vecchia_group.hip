// api_vecchia_group.hip -- C ABI of grouped Vecchia blocks: cocons_vecchia_group, the greedy grouping rule on
// the host; cocons_vecchia_group_table, the expanded table of any partition; cocons_vecchia_set_groups, the plan of a
// partition on a Vecchia handle whose table is closed under it; cocons_fit_create_vecchia_grouped, the three in one call; and
// cocons_neg2loglik_vecchia_grouped / cocons_vecchia_whiten_grouped, the value and the whitening with one factorisation per
// block, cocons_neg2loglik_grad_vecchia_grouped, the value and the gradient from it, and
// cocons_fisher_vecchia_grouped, the expected information from it, and cocons_vecchia_unwhiten_grouped,
// cocons_sim_vecchia_grouped, cocons_vecchia_whiten_t_grouped and cocons_cv_vecchia_grouped, U^-1, U' and
// cross-validation with their coefficients from it.  A grouped evaluation
// is the ungrouped one with launch_vecchia_group_blocks in the place of launch_vecchia_blocks: the same records, right-hand
// sides, per-row arrays, totals and status word, and therefore the same bits.
#include "fit.hpp"
#include "group_plan.hpp"

namespace {

// cocons_fit_create_vecchia's table rules on the caller's layout; 0, or -1 with the message
int check_table(const char *who, int n, int m, const int *nn)
{
    if (n < 1) return fail(-1, "%s: n = %d (at least one observation expected)", who, n);
    if (m < 1 || m > VECCHIA_M_MAX) return fail(-1, "%s: m = %d is outside 1 .. %d", who, m, VECCHIA_M_MAX);
    std::vector<int> row((size_t)m);
    for (int i = 0; i < n; ++i) {
        int k = 0;
        for (int j = 0; j < m; ++j) {
            const int v = nn[(size_t)i + (size_t)j * n];
            if (v < 0 || v > i)
                return fail(-1, "%s: row %d of nn names an index outside its range (1-based indices in 1 .. row - 1, 0 = none)",
                            who, i + 1);
            if (v > 0) row[(size_t)k++] = v;
        }
        std::sort(row.begin(), row.begin() + k);
        for (int j = 1; j < k; ++j)
            if (row[(size_t)j] == row[(size_t)j - 1])
                return fail(-1, "%s: row %d of nn names an index twice (1-based indices in 1 .. row - 1, 0 = none)", who, i + 1);
    }
    return 0;
}

cocons::GroupTable caller_table(int n, int m, const int *nn)
{
    cocons::GroupTable t;
    t.p = nn; t.n = (size_t)n; t.m = m; t.device = false;
    return t;
}

// group_plan's return as a refusal
int plan_refusal(const char *who, int st, int n)
{
    if (st < 0) return fail(-1, "%s: group[%d] is outside 0 .. %d", who, -st - 1, n - 1);
    return fail(-1, "%s: the block of row %d spans more than %d rows (its members and all their neighbours)", who, st,
                cocons::GROUP_ROWS_MAX);
}

template <class T> hipError_t to_device(DevBuf<T> &d, const std::vector<T> &h, hipStream_t s)
{
    if (hipError_t e = d.reserve(std::max<size_t>(h.size(), 1), s, nullptr, -1, true)) return e;
    if (h.empty()) return hipSuccess;
    return hipMemcpyAsync(d.get(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s);
}

// the grouped launch over the plan's blocks for nb right-hand sides in V->B: log d and the whitened columns into V->W
void group_blocks(cocons_fit *f, const ModeSel &ms, int nb)
{
    VecchiaState *V = f->vecchia.get();
    const VecchiaGroupState *G = V->grp.get();
    VecchiaGroupArgs a;
    a.blocks = G->blocks; a.kb = G->maxrows;
    a.off = G->off; a.rows = G->rows; a.order = G->by_size ? G->order.get() : nullptr; a.mask = G->mask;
    a.aosK = V->aos; a.gr = ms.gr; a.nu_fixed = ms.nu_fixed;
    a.B = V->B; a.ldb = (size_t)f->n; a.nb = nb;
    a.logd = V->W; a.Y = V->W + f->n; a.ldy = (size_t)f->n;
    a.fail = f->dinfo;
    launch_vecchia_group_blocks(ms.mode, a, f->stream);
}

}  // namespace

int vecchia_need_plan(cocons_fit *f, const char *who)
{
    if (!f->vecchia->grp) return fail(-1, "%s: the handle has no plan of grouped blocks (cocons_vecchia_set_groups attaches one)", who);
    return 0;
}

// The grouped gradient's launches: the blocks by id in chunks of `chunk` records, each chunk summed into its
// segments of blocks.  One chunk: the launch deals the blocks largest first, as the value launch does; more: by id within a
// chunk (the records stand at the blocks' ids either way, so the totals do not depend on it).
void vecchia_group_grad_chunks(cocons_fit *f, const ModeSel &ms, int smooth_free, int nc, int chunk, int nseg)
{
    VecchiaState *V = f->vecchia.get();
    const VecchiaGroupState *G = V->grp.get();
    const int n = f->n, ncol = vecchia_rec_cols(f->p);
    VecchiaGroupArgs a;
    a.kb = G->maxrows;
    a.off = G->off; a.rows = G->rows; a.mask = G->mask;
    a.order = (G->by_size && G->blocks <= chunk) ? G->order.get() : nullptr;
    a.aosK = V->aos; a.aosG = V->gaos; a.gr = ms.gr; a.nu_fixed = ms.nu_fixed; a.smooth_free = smooth_free;
    a.B = V->B; a.ldb = (size_t)n; a.nb = nc;
    a.logd = V->W; a.Y = V->W + n; a.ldy = (size_t)n;
    a.X = f->dX; a.ldx = n; a.p = f->p;
    a.rec = V->grec; a.ldr = (size_t)chunk;
    a.fail = f->dinfo;
    for (int b0 = 0; b0 < G->blocks; b0 += chunk) {
        a.blocks = std::min(chunk, G->blocks - b0); a.blk0 = b0;
        launch_vecchia_group_grad_blocks(ms.mode, a, f->stream);
        launch_vecchia_chunk_sums(V->grec, (size_t)chunk, a.blocks, ncol, V->gpart, b0 / VECCHIA_SUM_SEG, nseg, f->stream);
    }
}

// The grouped information's launches: as vecchia_group_grad_chunks, with the information's records and scratch.
void vecchia_group_fisher_chunks(cocons_fit *f, const ModeSel &ms, int smooth_free, int ndir, int gd, int mc, int chunk, int nseg)
{
    VecchiaState *V = f->vecchia.get();
    const VecchiaGroupState *G = V->grp.get();
    const int n = f->n, ncol = vecchia_fisher_cols(ndir, f->p);
    VecchiaGroupArgs a;
    a.kb = G->maxrows;
    a.off = G->off; a.rows = G->rows; a.mask = G->mask;
    a.order = (G->by_size && G->blocks <= chunk) ? G->order.get() : nullptr;
    a.aosK = V->aos; a.aosG = V->gaos; a.gr = ms.gr; a.nu_fixed = ms.nu_fixed; a.smooth_free = smooth_free;
    a.nb = 0;                                   // no right-hand sides, no log d
    a.X = f->dX; a.ldx = n; a.p = f->p;
    a.ndir = ndir; a.gd = gd; a.mc = mc; a.dirs = V->fdirs;
    a.rec = V->frec; a.ldr = (size_t)chunk;
    a.fail = f->dinfo;
    for (int b0 = 0; b0 < G->blocks; b0 += chunk) {
        a.blocks = std::min(chunk, G->blocks - b0); a.blk0 = b0;
        launch_vecchia_group_fisher_blocks(ms.mode, a, f->stream);
        launch_vecchia_chunk_sums(V->frec, (size_t)chunk, a.blocks, ncol, V->fpart, b0 / VECCHIA_SUM_SEG, nseg, f->stream);
    }
}

extern "C" int cocons_vecchia_group(int n, int m, const int *nn, int max_rows, int *group, long long *out4)
{
    const char *who = "cocons_vecchia_group";
    if (!nn || !group) return fail(-1, "%s: null argument", who);
    if (int rc = check_table(who, n, m, nn)) return rc;
    if (max_rows < 2 || max_rows > cocons::GROUP_ROWS_MAX)
        return fail(-1, "%s: max_rows = %d is outside 2 .. %d", who, max_rows, cocons::GROUP_ROWS_MAX);
    const cocons::GroupTable t = caller_table(n, m, nn);
    cocons::group_greedy(t, max_rows, group);
    if (out4) {
        cocons::GroupPlan pl;
        if (int st = cocons::group_plan(t, group, pl)) return plan_refusal(who, st, n);
        out4[0] = pl.blocks; out4[1] = pl.sum_rows; out4[2] = pl.pairs; out4[3] = cocons::group_pairs_ungrouped(t);
    }
    return 0;
}

extern "C" int cocons_vecchia_group_table(int n, int m, const int *nn, const int *group, int m_out, int *nn_out)
{
    const char *who = "cocons_vecchia_group_table";
    if (!nn || !group || (!nn_out && m_out != 0)) return fail(-1, "%s: null argument", who);
    if (int rc = check_table(who, n, m, nn)) return rc;
    cocons::GroupPlan pl;
    if (int st = cocons::group_plan(caller_table(n, m, nn), group, pl)) return plan_refusal(who, st, n);
    if (!nn_out) return pl.longest;
    if (m_out < 1 || m_out > VECCHIA_M_MAX) return fail(-1, "%s: m_out = %d is outside 1 .. %d", who, m_out, VECCHIA_M_MAX);
    if (m_out < pl.longest)
        return fail(-1, "%s: m_out = %d is smaller than the longest expanded row (%d neighbours)", who, m_out, pl.longest);
    cocons::group_table(pl, (size_t)n, m_out, nn_out);
    return 0;
}

extern "C" int cocons_vecchia_set_groups(cocons_fit *f, const int *group)
{
    const char *who = "cocons_vecchia_set_groups";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!group) return fail(-1, "%s: null argument", who);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    VecchiaState *V = f->vecchia.get();
    const int n = f->n, m = V->m;
    // the handle's table home, once: the check runs on the host, and a table that was searched on the device has no copy there
    std::vector<int> tab((size_t)n * m);
    HIPCHK_AT(who, hipMemcpyAsync(tab.data(), V->nbr, tab.size() * sizeof(int), hipMemcpyDeviceToHost, f->stream));
    HIPCHK_AT(who, hipStreamSynchronize(f->stream));
    cocons::GroupTable t;
    t.p = tab.data(); t.n = (size_t)n; t.m = m; t.device = true;
    cocons::GroupPlan pl;
    if (int st = cocons::group_plan(t, group, pl)) return plan_refusal(who, st, n);
    int have = 0, need = 0;
    if (int row = cocons::group_closed(t, pl, &have, &need))
        return fail(-1, "%s: row %d of the handle's table holds %d neighbours, its block needs the %d rows in front of it (the "
                        "table is not closed under these groups; cocons_vecchia_group_table makes one that is)",
                    who, row, have, need);
    std::unique_ptr<VecchiaGroupState> G(new VecchiaGroupState());
    G->blocks = pl.blocks; G->maxrows = pl.maxrows; G->sum_rows = pl.sum_rows; G->pairs = pl.pairs;
    const char *env = getenv("COCONS_VECCHIA_GROUP_ORDER");
    G->by_size = !(env && env[0] == '0' && !env[1]);
    hipStream_t s = f->stream;
    HIPCHK_AT(who, to_device(G->off, pl.off, s));
    HIPCHK_AT(who, to_device(G->rows, pl.rows, s));
    HIPCHK_AT(who, to_device(G->order, pl.order, s));
    HIPCHK_AT(who, to_device(G->mask, pl.mask, s));
    HIPCHK_AT(who, hipStreamSynchronize(s));           // (the plan's host vectors end with this call)
    V->grp = std::move(G);                             // a former plan is freed here: the stream is drained
    return 0;
}

extern "C" int cocons_vecchia_groups_info(cocons_fit *f, long long *out5)
{
    const char *who = "cocons_vecchia_groups_info";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!out5) return fail(-1, "%s: null argument", who);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (int rc = vecchia_need_plan(f, who)) return rc;
    const VecchiaGroupState *G = f->vecchia->grp.get();
    out5[0] = G->blocks; out5[1] = G->maxrows; out5[2] = G->sum_rows; out5[3] = G->pairs; out5[4] = G->bytes();
    return 0;
}

extern "C" cocons_fit *cocons_fit_create_vecchia_grouped(int n, int p, int r, const double *locs, const double *X, const double *z,
                                                         const double *smooth_limits, int device, int m, const int *nn,
                                                         int max_rows)
{
    const char *who = "cocons_fit_create_vecchia_grouped";
    if (!locs || !X || !z || !smooth_limits || !nn) { fail(-1, "%s: null argument", who); return nullptr; }
    if (check_table(who, n, m, nn)) return nullptr;
    if (max_rows < 2 || max_rows > cocons::GROUP_ROWS_MAX) {
        fail(-1, "%s: max_rows = %d is outside 2 .. %d", who, max_rows, cocons::GROUP_ROWS_MAX);
        return nullptr;
    }
    const cocons::GroupTable t = caller_table(n, m, nn);
    std::vector<int> group((size_t)n);
    cocons::group_greedy(t, max_rows, group.data());
    cocons::GroupPlan pl;
    if (int st = cocons::group_plan(t, group.data(), pl)) { plan_refusal(who, st, n); return nullptr; }
    const int m_out = std::max(pl.longest, 1);
    std::vector<int> wide((size_t)n * m_out);
    cocons::group_table(pl, (size_t)n, m_out, wide.data());
    cocons_fit *f = vecchia_create_impl(who, n, p, r, locs, X, z, smooth_limits, device, m_out, wide.data(), false);
    if (!f) return nullptr;
    if (cocons_vecchia_set_groups(f, group.data())) {
        cocons_fit_destroy(f);
        return nullptr;
    }
    return f;
}

extern "C" int cocons_neg2loglik_vecchia_grouped(cocons_fit *f, const double *theta, const double *mean, double *value,
                                                 double *parts)
{
    const char *who = "cocons_neg2loglik_vecchia_grouped";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !mean || !value) return fail(-1, "%s: null argument", who);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (int rc = vecchia_need_plan(f, who)) return rc;
    VecchiaState *V = f->vecchia.get();
    const int n = f->n, r = f->r;
    double hmean[COCONS_P_MAX];
    for (int i = 0; i < f->p; ++i) hmean[i] = canon_nan(mean[i]);
    // (another entry may have left the scratch of its own column count)
    HIPCHK_AT(who, V->B.reserve((size_t)n * r, f->stream, nullptr));
    HIPCHK_AT(who, V->W.reserve((size_t)n * (1 + r), f->stream, nullptr));
    HIPCHK_AT(who, V->part.reserve(vecchia_sum_scratch_doubles(n, 1 + r), f->stream, nullptr));
    if (int rc = reset_info(f)) return rc;
    const ModeSel ms = vecchia_records(f, theta, 0, V->aos);
    launch_vecchia_resid(n, f->p, f->dX, n, hmean, f->dz, n, 0, r, V->B, (size_t)n, f->stream);
    group_blocks(f, ms, r);
    launch_vecchia_sums(V->W, (size_t)n, n, 1 + r, V->part, f->dout, f->stream);
    HIPCHK_AT(who, hipMemcpyAsync(f->hout, f->dout, (size_t)(1 + r) * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    if (int st = vecchia_status(f, who)) return st;
    double total = 0.0;
    for (int k = 0; k < r; ++k) total += n * LOG_2PI + 2 * f->hout[0] + f->hout[1 + k];
    if (parts) for (int k = 0; k <= r; ++k) parts[k] = f->hout[k];
    *value = total;
    return 0;
}

extern "C" int cocons_vecchia_whiten_grouped(cocons_fit *f, const double *theta, int c, const double *B, double *out, double *logd)
{
    const char *who = "cocons_vecchia_whiten_grouped";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !B || !out) return fail(-1, "%s: null argument", who);
    if (c < 1) return fail(-1, "%s: c = %d (at least one column expected)", who, c);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (int rc = vecchia_need_plan(f, who)) return rc;
    VecchiaState *V = f->vecchia.get();
    const size_t n = (size_t)f->n;
    HIPCHK_AT(who, V->B.reserve(n * c, f->stream, nullptr));
    HIPCHK_AT(who, V->W.reserve(n * (1 + c), f->stream, nullptr));
    if (int rc = reset_info(f)) return rc;
    HIPCHK_AT(who, upload_canon(V->B, B, n * c, f->stream));
    const ModeSel ms = vecchia_records(f, theta, 0, V->aos);
    group_blocks(f, ms, c);
    // (into staging of the call: the caller's arrays stay untouched when a block fails)
    std::vector<double> h(n * (1 + c));
    HIPCHK_AT(who, hipMemcpyAsync(h.data(), V->W, h.size() * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    if (int st = vecchia_status(f, who)) return st;
    if (logd) memcpy(logd, h.data(), n * sizeof(double));
    memcpy(out, h.data() + n, n * c * sizeof(double));
    return 0;
}

extern "C" int cocons_neg2loglik_grad_vecchia_grouped(cocons_fit *f, const double *theta, const double *mean, int c,
                                                      const double *B, double *sum_logliks, double *parts, double *grad_theta,
                                                      double *grad_quad, double *grad_mean)
{
    return vecchia_grad_impl("cocons_neg2loglik_grad_vecchia_grouped", true, f, theta, mean, c, B, sum_logliks, parts,
                             grad_theta, grad_quad, grad_mean);
}

extern "C" int cocons_fisher_vecchia_grouped(cocons_fit *f, const double *theta, int ndir, const double *dirs, double *info,
                                             double *info_mean)
{
    return vecchia_fisher_impl("cocons_fisher_vecchia_grouped", true, f, theta, ndir, dirs, info, info_mean);
}

// the ungrouped entries' bodies with launch_vecchia_group_coefs in the place of launch_vecchia_coefs
extern "C" int cocons_vecchia_unwhiten_grouped(cocons_fit *f, const double *theta, int c, const double *W, double *out)
{
    return vecchia_unwhiten_impl("cocons_vecchia_unwhiten_grouped", true, false, f, theta, c, W, out, nullptr);
}

extern "C" int cocons_debug_vecchia_sim_phases_grouped(cocons_fit *f, const double *theta, int c, const double *W, double *out,
                                                       double *ms3)
{
    return vecchia_unwhiten_impl("cocons_debug_vecchia_sim_phases_grouped", true, true, f, theta, c, W, out, ms3);
}

extern "C" int cocons_sim_vecchia_grouped(cocons_fit *f, const double *theta, const double *mean, int n_fixed, int z_col, int nsim,
                                          const double *iiderrors, double *out)
{
    return vecchia_sim_impl("cocons_sim_vecchia_grouped", true, f, theta, mean, n_fixed, z_col, nsim, iiderrors, out);
}

extern "C" int cocons_vecchia_whiten_t_grouped(cocons_fit *f, const double *theta, int c, const double *W, double *out,
                                               double *qdiag)
{
    return vecchia_whiten_t_impl("cocons_vecchia_whiten_t_grouped", true, f, theta, c, W, out, qdiag);
}

extern "C" int cocons_cv_vecchia_grouped(cocons_fit *f, const double *theta, const double *mean, int nfold, const int *fold,
                                         double *resid, double *var, long long *stats4)
{
    return vecchia_cv_impl("cocons_cv_vecchia_grouped", true, f, theta, mean, nfold, fold, resid, var, stats4);
}
