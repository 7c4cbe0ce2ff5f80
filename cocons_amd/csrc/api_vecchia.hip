// api_vecchia.hip -- C ABI of the Vecchia approximation: the third kind of handle -- data, a neighbour table and
// O(n (m + 16)) bytes of scratch, never an n x n buffer -- and the entries on it: the -2 log-likelihood, its analytic gradient
// (DESIGN.md 4s), its expected information, the whitening of given columns, and local kriging.  One evaluation is: the location parameters for theta (loc_params_kernel, then their
// transpose to one record per location), the right-hand sides, ONE launch of a block kernel of vecchia.hip with a wavefront per
// observation -- or, grouped, of vecchia_group.hip with a workgroup per block of the plan --, and -- for the value -- the totals
// as a tree of fixed shape.  Nothing here factors through api.hip.
#include "fit.hpp"

int vecchia_refuse(const char *who)
{
    return fail(-1, "%s: not available on a Vecchia fit (cocons_neg2loglik_vecchia, cocons_neg2loglik_grad_vecchia, "
                    "cocons_fisher_vecchia, cocons_vecchia_whiten and cocons_vecchia_predict are)", who);
}

int vecchia_only(cocons_fit *f, const char *who)
{
    if (!f->vecchia) return fail(-1, "%s: not a Vecchia fit (cocons_fit_create_vecchia makes one)", who);
    return 0;
}

// Row i of a neighbour table (rows x m column-major, 1-based, 0 = none) into row i of the device layout: 0-based, ascending,
// -1 behind the last.  limit: the largest index row i may name.  0, or the first offence: 1 = out of range, 2 = twice.
static int vecchia_row(const int *nn, size_t rows, int m, size_t i, int limit, int *out)
{
    int k = 0;
    for (int j = 0; j < m; ++j) {
        const int v = nn[i + (size_t)j * rows];
        if (v < 0 || v > limit) return 1;
        if (v > 0) out[k++] = v - 1;
    }
    std::sort(out, out + k);
    for (int j = 1; j < k; ++j) if (out[j] == out[j - 1]) return 2;
    for (int j = k; j < m; ++j) out[j] = -1;
    return 0;
}

static const char *const vecchia_offence[] = {"", "names an index outside its range", "names an index twice"};

cocons_fit *vecchia_create_impl(const char *who, int n, int p, int r, const double *locs, const double *X, const double *z,
                                const double *smooth_limits, int device, int m, const int *nn, bool search,
                                VecchiaTableSource *src)
{
    if (src) search = true;                     // (no table comes in either way)
    if (!locs || !X || !z || !smooth_limits || (!search && !nn)) { fail(-1, "%s: null argument", who); return nullptr; }
    if (n < 1) { fail(-1, "%s: n = %d (at least one observation expected)", who, n); return nullptr; }
    if (p < 1 || p > COCONS_P_MAX || r < 1) { fail(-1, "%s: bad argument (p = %d, r = %d)", who, p, r); return nullptr; }
    if (m < 1 || m > VECCHIA_M_MAX) { fail(-1, "%s: m = %d is outside 1 .. %d", who, m, VECCHIA_M_MAX); return nullptr; }
    if (pattern_check_finite(who, "locs", (size_t)n, locs)) return nullptr;
    // a table that comes in is put into the device layout here, before any device work; search: there is none
    std::vector<int> tab;
    if (!search) {
        tab.resize((size_t)n * m);
        for (int i = 0; i < n; ++i)
            if (int bad = vecchia_row(nn, (size_t)n, m, (size_t)i, i, &tab[(size_t)i * m])) {
                fail(-1, "%s: row %d of nn %s (1-based indices in 1 .. row - 1, 0 = none)", who, i + 1, vecchia_offence[bad]);
                return nullptr;
            }
    }
    // the caller's order is the Vecchia order and the handle keeps it (no Morton sort, no padding in front): neighbour
    // indices and outputs need no mapping, and COCONS_SPATIAL_SORT cannot reach a bit of any output
    cocons_fit *f = fit_create_impl(n, p, r, 0, locs, X, z, nullptr, smooth_limits, device, false, true, false, true);
    if (!f) return nullptr;
    auto drop = [&](hipError_t e) {
        fail(-100 - (int)e, "%s: %s", who, hipGetErrorString(e));
        (void)hipGetLastError();
        f->op_mu.unlock();
        cocons_fit_destroy(f);
        return (cocons_fit *)nullptr;
    };
    f->vecchia.reset(new VecchiaState());
    VecchiaState *V = f->vecchia.get();
    V->m = m;
    if (!src)
        if (hipError_t e = V->nbr.alloc((size_t)n * m)) return drop(e);
    if (hipError_t e = V->aos.alloc((size_t)VECCHIA_REC * n)) return drop(e);
    if (hipError_t e = V->B.alloc((size_t)n * r)) return drop(e);
    if (hipError_t e = V->W.alloc((size_t)n * (1 + r))) return drop(e);
    if (hipError_t e = V->part.alloc(vecchia_sum_scratch_doubles(n, 1 + r))) return drop(e);
    if (src) {
        // the table is made on the device by the caller's source and adopted
        if (src->make(who, f, locs)) {
            (void)hipGetLastError();
            f->op_mu.unlock();
            cocons_fit_destroy(f);
            return nullptr;
        }
    } else if (search) {
        // the table straight into V->nbr: it never exists on the host
        if (knn_self_search(who, n, locs, locs + n, f->dlocs, f->dlocs + n, m, nullptr, V->nbr, f->stream)) {
            (void)hipGetLastError();
            f->op_mu.unlock();
            cocons_fit_destroy(f);
            return nullptr;
        }
    } else {
        if (hipError_t e = hipMemcpyAsync(V->nbr, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, f->stream)) return drop(e);
        if (hipError_t e = hipStreamSynchronize(f->stream)) return drop(e);
    }
    f->op_mu.unlock();
    return f;
}

extern "C" cocons_fit *cocons_fit_create_vecchia(int n, int p, int r, const double *locs, const double *X, const double *z,
                                                 const double *smooth_limits, int device, int m, const int *nn)
{
    return vecchia_create_impl("cocons_fit_create_vecchia", n, p, r, locs, X, z, smooth_limits, device, m, nn, false);
}

// out4 = {n, m, device bytes the handle holds, rows per chunk of cocons_vecchia_predict}
static constexpr int VECCHIA_PRED_ROWS = 16384;

extern "C" int cocons_vecchia_info(cocons_fit *f, long long *out4)
{
    const char *who = "cocons_vecchia_info";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!out4) return fail(-1, "%s: null argument", who);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    out4[0] = f->n; out4[1] = f->vecchia->m;
    out4[2] = f->vecchia->bytes() +
              (long long)((f->dX.count() + f->dlocs.count() + f->dz.count() + f->dloc.count() + f->dinv.count() +
                           f->dinfo_out.count()) * sizeof(double));
    out4[3] = VECCHIA_PRED_ROWS;
    return 0;
}

// the observations' records for theta in the parameters of cov_rns (which = 0) or of cov_rns_pred's branch (which = 2)
ModeSel vecchia_records(cocons_fit *f, const double *theta, int which, double *aos)
{
    ThetaVecs tv;
    make_theta_vecs(theta, f->p, tv);
    const ModeSel ms = select_mode(theta, f->p, f->smooth_limits, which);
    launch_loc_params(loc_args(f->n, f->p, f->dX, f->dlocs, f->dloc, f->npad, tv, ms.smooth_kind, f->smooth_limits), f->stream);
    launch_vecchia_aos(f->dloc, f->npad, f->n, aos, f->stream);
    return ms;
}

// the info words home and the stream drained; 0, or the smallest 1-based row whose block has a pivot that is not positive
int vecchia_status(cocons_fit *f, const char *who)
{
    HIPCHK_AT(who, hipMemcpyAsync(f->hinfo, f->dinfo, 2 * sizeof(int), hipMemcpyDeviceToHost, f->stream));
    HIPCHK_AT(who, hipGetLastError());
    HIPCHK_AT(who, hipStreamSynchronize(f->stream));
    if (f->hinfo[0] == 0x7f7f7f7f) return 0;
    g_err = "a conditional variance is not positive";
    return f->hinfo[0];
}

int vecchia_need_plan(cocons_fit *f, const char *who)
{
    if (!f->vecchia->grp) return fail(-1, "%s: the handle has no plan of grouped blocks (cocons_vecchia_set_groups attaches one)", who);
    return 0;
}

// what the ungrouped and the grouped launches' argument blocks share by name
template <class Args> static void vecchia_common_args(Args &a, cocons_fit *f, const ModeSel &ms)
{
    a.aosK = f->vecchia->aos; a.gr = ms.gr; a.nu_fixed = ms.nu_fixed; a.fail = f->dinfo;
}

// nb right-hand sides in V->B: log d and the whitened columns into V->W
template <class Args> static void vecchia_rhs_args(Args &a, cocons_fit *f, int nb)
{
    VecchiaState *V = f->vecchia.get();
    a.B = V->B; a.ldb = (size_t)f->n; a.nb = nb;
    a.logd = V->W; a.Y = V->W + f->n; a.ldy = (size_t)f->n;
}

template <class Args> static void vecchia_plan_args(Args &a, const VecchiaGroupState *G, bool by_size)
{
    a.kb = G->maxrows; a.off = G->off; a.rows = G->rows; a.mask = G->mask;
    a.order = by_size ? G->order.get() : nullptr;
}

// the likelihood launch for nb right-hand sides in V->B: over all n observations, or (grouped) over the plan's blocks with one
// factorisation per block -- the same records, right-hand sides, per-row arrays and status word, and the same bits
static void vecchia_blocks(cocons_fit *f, bool grouped, const ModeSel &ms, int nb)
{
    VecchiaState *V = f->vecchia.get();
    if (grouped) {
        VecchiaGroupArgs a;
        vecchia_common_args(a, f, ms);
        vecchia_rhs_args(a, f, nb);
        vecchia_plan_args(a, V->grp.get(), V->grp->by_size);
        a.blocks = V->grp->blocks;
        launch_vecchia_group_blocks(ms.mode, a, f->stream);
    } else {
        VecchiaArgs a;
        vecchia_common_args(a, f, ms);
        vecchia_rhs_args(a, f, nb);
        a.rows = f->n; a.m = V->m; a.kb = V->m + 1; a.nbr = V->nbr;
        launch_vecchia_blocks(ms.mode, false, a, f->stream);
    }
}

// cocons_neg2loglik_vecchia and (grouped) cocons_neg2loglik_vecchia_grouped
int vecchia_value_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, const double *mean, double *value,
                       double *parts)
{
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !mean || !value) return fail(-1, "%s: null argument", who);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (grouped) if (int rc = vecchia_need_plan(f, who)) return rc;
    VecchiaState *V = f->vecchia.get();
    const int n = f->n, r = f->r;
    double hmean[COCONS_P_MAX];
    for (int i = 0; i < f->p; ++i) hmean[i] = canon_nan(mean[i]);
    // (never shrinks: a handle's scratch holds r columns from its creation on)
    HIPCHK_AT(who, V->B.reserve((size_t)n * r, f->stream, nullptr));
    HIPCHK_AT(who, V->W.reserve((size_t)n * (1 + r), f->stream, nullptr));
    HIPCHK_AT(who, V->part.reserve(vecchia_sum_scratch_doubles(n, 1 + r), f->stream, nullptr));
    if (int rc = reset_info(f)) return rc;
    const ModeSel ms = vecchia_records(f, theta, 0, V->aos);
    launch_vecchia_resid(n, f->p, f->dX, n, hmean, f->dz, n, 0, r, V->B, (size_t)n, f->stream);
    vecchia_blocks(f, grouped, ms, r);
    launch_vecchia_sums(V->W, (size_t)n, n, 1 + r, V->part, f->dout, f->stream);
    HIPCHK_AT(who, hipMemcpyAsync(f->hout, f->dout, (size_t)(1 + r) * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    if (int st = vecchia_status(f, who)) return st;
    double total = 0.0;
    for (int k = 0; k < r; ++k) total += n * LOG_2PI + 2 * f->hout[0] + f->hout[1 + k];
    if (parts) for (int k = 0; k <= r; ++k) parts[k] = f->hout[k];
    *value = total;
    return 0;
}

extern "C" int cocons_neg2loglik_vecchia(cocons_fit *f, const double *theta, const double *mean, double *value, double *parts)
{
    return vecchia_value_impl("cocons_neg2loglik_vecchia", false, f, theta, mean, value, parts);
}

// The gradient's or (ndir > 0) the information's launches of one evaluation: the records in chunks of `chunk` -- one per
// observation, or (grouped) one per block of the plan, by id --, each chunk summed into its segments.
// Grouped, one chunk: the launch deals the blocks largest first, as the value launch does; more: by id within a chunk (the
// records stand at the blocks' ids either way, so the totals do not depend on it).
static void vecchia_record_chunks(cocons_fit *f, bool grouped, const ModeSel &ms, int smooth_free, int nc, int ndir, int gd, int mc,
                                  int chunk, int nseg)
{
    VecchiaState *V = f->vecchia.get();
    const bool fisher = ndir > 0;
    const int n = f->n, ncol = fisher ? vecchia_fisher_cols(ndir, f->p) : vecchia_rec_cols(f->p);
    double *rec = fisher ? V->frec.get() : V->grec.get(), *part = fisher ? V->fpart.get() : V->gpart.get();
    auto fill = [&](auto &a) {
        vecchia_common_args(a, f, ms);
        if (fisher) { a.nb = 0; a.ndir = ndir; a.gd = gd; a.dirs = V->fdirs; }          // no right-hand sides, no log d
        else vecchia_rhs_args(a, f, nc);
        a.aosG = V->gaos; a.smooth_free = smooth_free;
        a.X = f->dX; a.ldx = n; a.p = f->p;
        a.rec = rec; a.ldr = (size_t)chunk;
    };
    if (grouped) {
        const VecchiaGroupState *G = V->grp.get();
        VecchiaGroupArgs a;
        fill(a);
        vecchia_plan_args(a, G, G->by_size && G->blocks <= chunk);
        a.mc = mc;
        for (int b0 = 0; b0 < G->blocks; b0 += chunk) {
            a.blocks = std::min(chunk, G->blocks - b0); a.blk0 = b0;
            (fisher ? launch_vecchia_group_fisher_blocks : launch_vecchia_group_grad_blocks)(ms.mode, a, f->stream);
            launch_vecchia_chunk_sums(rec, (size_t)chunk, a.blocks, ncol, part, b0 / VECCHIA_SUM_SEG, nseg, f->stream);
        }
    } else {
        VecchiaArgs a;
        fill(a);
        a.m = V->m; a.kb = V->m + 1; a.nbr = V->nbr;
        for (int r0 = 0; r0 < n; r0 += chunk) {
            a.rows = std::min(chunk, n - r0); a.obs0 = r0; a.row0 = r0;
            (fisher ? launch_vecchia_fisher_blocks : launch_vecchia_grad_blocks)(ms.mode, a, f->stream);
            launch_vecchia_chunk_sums(rec, (size_t)chunk, a.rows, ncol, part, r0 / VECCHIA_SUM_SEG, nseg, f->stream);
        }
    }
}

// Value and gradient from one launch per chunk of VECCHIA_GRAD_CHUNK observations.  The value's totals are
// launch_vecchia_sums over log d and the whitened columns of all n rows -- the value entry's tree over the value kernel's
// numbers --, the gradient's the same tree over the per-observation records, its first stage run chunk by chunk.
//
// grouped (cocons_neg2loglik_grad_vecchia_grouped): the same arguments, refusals, scratch, value totals and host
// tail; the launches run over the plan's blocks -- one record per block, chunks and segments of blocks -- instead.
int vecchia_grad_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, const double *mean, int c,
                      const double *B, double *sum_logliks, double *parts, double *grad_theta, double *grad_quad,
                      double *grad_mean)
{
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !sum_logliks || !grad_theta || (!B && (!mean || !grad_mean))) return fail(-1, "%s: null argument", who);
    if (B && (mean || grad_mean))
        return fail(-1, "%s: B is given, so mean and grad_mean must be NULL (the columns are used as they are)", who);
    if (B && c < 1) return fail(-1, "%s: c = %d (at least one column expected)", who, c);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (grouped) if (int rc = vecchia_need_plan(f, who)) return rc;
    VecchiaState *V = f->vecchia.get();
    const int n = f->n, p = f->p, nc = B ? c : f->r, ncol = vecchia_rec_cols(p);
    const int units = grouped ? V->grp->blocks : n;           // what a record stands for: a block, or an observation
    const int nseg = (units + VECCHIA_SUM_SEG - 1) / VECCHIA_SUM_SEG, chunk = std::min(units, VECCHIA_GRAD_CHUNK);
    hipStream_t s = f->stream;
    HIPCHK_AT(who, V->B.reserve((size_t)n * nc, s, nullptr));
    HIPCHK_AT(who, V->W.reserve((size_t)n * (1 + nc), s, nullptr));
    HIPCHK_AT(who, V->part.reserve(vecchia_sum_scratch_doubles(n, 1 + nc), s, nullptr));
    HIPCHK_AT(who, V->gsite.reserve((size_t)GSITE_FIELDS * f->npad, s, nullptr));
    HIPCHK_AT(who, V->gaos.reserve((size_t)VECCHIA_GSITE_REC * n, s, nullptr));
    HIPCHK_AT(who, V->grec.reserve((size_t)chunk * ncol, s, nullptr));
    HIPCHK_AT(who, V->gpart.reserve((size_t)nseg * ncol, s, nullptr));
    HIPCHK_AT(who, V->gout.reserve((size_t)(1 + nc) + ncol, s, nullptr));
    double hmean[COCONS_P_MAX];
    if (!B) for (int i = 0; i < p; ++i) hmean[i] = canon_nan(mean[i]);
    if (int rc = reset_info(f)) return rc;
    if (B) HIPCHK_AT(who, upload_canon(V->B, B, (size_t)n * nc, s));
    const ModeSel ms = vecchia_records(f, theta, 0, V->aos);
    if (!B) launch_vecchia_resid(n, p, f->dX, n, hmean, f->dz, n, 0, nc, V->B, (size_t)n, s);
    // the site derivatives beside the records (grad_site_kernel, as every other gradient here forms them)
    ThetaVecs tv;
    make_theta_vecs(theta, p, tv);
    const int smooth_free = ms.smooth_kind == SMOOTH_LOGISTIC_SQRT && f->smooth_limits[1] != f->smooth_limits[0];
    launch_grad_site(loc_args(n, p, f->dX, f->dlocs, V->gsite, f->npad, tv, ms.smooth_kind, f->smooth_limits), V->gsite,
                     f->npad, smooth_free, s);
    launch_vecchia_site_rec(V->gsite, f->npad, n, V->gaos, s);
    vecchia_record_chunks(f, grouped, ms, smooth_free, nc, 0, 0, 0, chunk, nseg);
    launch_vecchia_sums(V->W, (size_t)n, n, 1 + nc, V->part, V->gout, s);
    launch_vecchia_final_sums(V->gpart, nseg, ncol, V->gout + (1 + nc), s);
    std::vector<double> h((size_t)(1 + nc) + ncol);
    HIPCHK_AT(who, hipMemcpyAsync(h.data(), V->gout, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    if (int st = vecchia_status(f, who)) return st;
    double total = 0.0;
    for (int k = 0; k < nc; ++k) total += n * LOG_2PI + 2 * h[0] + h[1 + k];
    if (parts) for (int k = 0; k <= nc; ++k) parts[k] = h[k];
    *sum_logliks = total;
    // the table in cocons_neg2loglik_grad_dense's conventions: scale[0] takes the global-range sum, scale[k >= 1] the factor 2
    const double *g = h.data() + (1 + nc);
    for (int t = 0; t < 6; ++t)
        for (int k = 0; k < p; ++k) {
            double lg = g[t * p + k], qd = g[6 * p + t * p + k];
            if (t == TH_SCALE) {
                if (k == 0) { lg = g[12 * p]; qd = g[12 * p + 1]; }
                else { lg = 2.0 * lg; qd = 2.0 * qd; }
            }
            grad_theta[t * p + k] = lg + qd;
            if (grad_quad) grad_quad[t * p + k] = qd;
        }
    if (grad_mean) for (int k = 0; k < p; ++k) grad_mean[k] = -2.0 * g[12 * p + 2 + k];
    return 0;
}

extern "C" int cocons_neg2loglik_grad_vecchia(cocons_fit *f, const double *theta, const double *mean, int c, const double *B,
                                              double *sum_logliks, double *parts, double *grad_theta, double *grad_quad,
                                              double *grad_mean)
{
    return vecchia_grad_impl("cocons_neg2loglik_grad_vecchia", false, f, theta, mean, c, B, sum_logliks, parts, grad_theta,
                             grad_quad, grad_mean);
}

// Expected information of the Vecchia likelihood: one launch per chunk of vecchia_fisher_chunk observations,
// one record per observation, and the totals through the gradient's two-stage tree -- a function of n alone, whatever the chunk.
//
// grouped (cocons_fisher_vecchia_grouped): the same arguments, refusals, scratch, totals and host tail; the
// launches run over the plan's blocks -- one record per block, chunks and segments of blocks -- instead.
int vecchia_fisher_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, int ndir, const double *dirs,
                        double *info, double *info_mean)
{
    if (int rc = fisher_check_args(who, f, theta, ndir, dirs, info)) return rc;
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (grouped) if (int rc = vecchia_need_plan(f, who)) return rc;
    VecchiaState *V = f->vecchia.get();
    const int n = f->n, p = f->p, ncol = vecchia_fisher_cols(ndir, p), ng = ndir * (ndir + 1) / 2;
    if (int rc = fisher_check_dirs(who, ndir, dirs, p)) return rc;
    const int units = grouped ? V->grp->blocks : n;           // what a record stands for: a block, or an observation
    const int nseg = (units + VECCHIA_SUM_SEG - 1) / VECCHIA_SUM_SEG, chunk = std::min(units, vecchia_fisher_chunk(ndir, p));
    int gd = 0, mc = 0;
    if (grouped) {
        const int kb = V->grp->maxrows;
        vecchia_group_fisher_shape(kb, ndir, &gd, &mc);
        if (vecchia_group_fisher_lds_bytes(kb, ndir, gd, mc) > VECCHIA_FISHER_LDS_MAX)
            return fail(-1, "%s: %d directions at blocks of %d rows need %zu bytes of LDS a workgroup (%zu at most)", who, ndir,
                        kb, vecchia_group_fisher_lds_bytes(kb, ndir, gd, mc), VECCHIA_FISHER_LDS_MAX);
    } else {
        gd = vecchia_fisher_group(V->m, ndir);
        if (vecchia_fisher_lds_bytes(V->m, ndir, gd) > VECCHIA_FISHER_LDS_MAX)
            return fail(-1, "%s: %d directions at m = %d need %zu bytes of LDS a workgroup (%zu at most)", who, ndir, V->m,
                        vecchia_fisher_lds_bytes(V->m, ndir, gd), VECCHIA_FISHER_LDS_MAX);
    }
    hipStream_t s = f->stream;
    const size_t nd = (size_t)ndir * 6 * p;
    // (the records and their segments are sized by n either way -- blocks <= n --, so the handle holds the same bytes after
    // the grouped call as after the ungrouped one)
    const size_t counts[6] = {(size_t)GSITE_FIELDS * f->npad, (size_t)VECCHIA_GSITE_REC * n, nd,
                              (size_t)std::min(n, vecchia_fisher_chunk(ndir, p)) * ncol,
                              (size_t)((n + VECCHIA_SUM_SEG - 1) / VECCHIA_SUM_SEG) * ncol, (size_t)ncol};
    DevBuf<double> *bufs[6] = {&V->gsite, &V->gaos, &V->fdirs, &V->frec, &V->fpart, &V->fout};
    size_t bytes = 0;
    for (int b = 0; b < 6; ++b) bytes += std::max(counts[b], bufs[b]->count()) * sizeof(double);
    for (int b = 0; b < 6; ++b)
        if (hipError_t e = bufs[b]->reserve(counts[b], s, nullptr)) {
            (void)hipGetLastError();
            return fail(-100 - (int)e, "%s: the device cannot hold the %zu bytes of this call's scratch (%d directions, chunks of "
                                       "%d rows): %s", who, bytes, ndir, chunk, hipGetErrorString(e));
        }
    if (int rc = reset_info(f)) return rc;
    HIPCHK_AT(who, upload_canon(V->fdirs, dirs, nd, s));
    const ModeSel ms = vecchia_records(f, theta, 0, V->aos);
    ThetaVecs tv;
    make_theta_vecs(theta, p, tv);
    const int smooth_free = ms.smooth_kind == SMOOTH_LOGISTIC_SQRT && f->smooth_limits[1] != f->smooth_limits[0];
    launch_grad_site(loc_args(n, p, f->dX, f->dlocs, V->gsite, f->npad, tv, ms.smooth_kind, f->smooth_limits), V->gsite,
                     f->npad, smooth_free, s);
    launch_vecchia_site_rec(V->gsite, f->npad, n, V->gaos, s);
    vecchia_record_chunks(f, grouped, ms, smooth_free, 0, ndir, gd, mc, chunk, nseg);
    launch_vecchia_final_sums(V->fpart, nseg, ncol, V->fout, s);
    std::vector<double> h((size_t)ncol);
    HIPCHK_AT(who, hipMemcpyAsync(h.data(), V->fout, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    if (int st = vecchia_status(f, who)) return st;
    // mirrored from the lower triangles: symmetric to the bit
    const double r = (double)f->r;
    for (int a_ = 0; a_ < ndir; ++a_)
        for (int b = 0; b <= a_; ++b) info[a_ * ndir + b] = info[b * ndir + a_] = r * h[(size_t)a_ * (a_ + 1) / 2 + b];
    if (info_mean)
        for (int k = 0; k < p; ++k)
            for (int l = 0; l <= k; ++l) info_mean[k * p + l] = info_mean[l * p + k] = r * h[(size_t)ng + k * (k + 1) / 2 + l];
    return 0;
}

extern "C" int cocons_fisher_vecchia(cocons_fit *f, const double *theta, int ndir, const double *dirs, double *info,
                                     double *info_mean)
{
    return vecchia_fisher_impl("cocons_fisher_vecchia", false, f, theta, ndir, dirs, info, info_mean);
}

// cocons_vecchia_whiten and (grouped) cocons_vecchia_whiten_grouped
int vecchia_whiten_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, int c, const double *B, double *out,
                        double *logd)
{
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !B || !out) return fail(-1, "%s: null argument", who);
    if (c < 1) return fail(-1, "%s: c = %d (at least one column expected)", who, c);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (grouped) if (int rc = vecchia_need_plan(f, who)) return rc;
    VecchiaState *V = f->vecchia.get();
    const size_t n = (size_t)f->n;
    HIPCHK_AT(who, V->B.reserve(n * c, f->stream, nullptr));
    HIPCHK_AT(who, V->W.reserve(n * (1 + c), f->stream, nullptr));
    if (int rc = reset_info(f)) return rc;
    HIPCHK_AT(who, upload_canon(V->B, B, n * c, f->stream));
    const ModeSel ms = vecchia_records(f, theta, 0, V->aos);
    vecchia_blocks(f, grouped, ms, c);
    // (into staging of the call: the caller's arrays stay untouched when a block fails)
    std::vector<double> h(n * (1 + c));
    HIPCHK_AT(who, hipMemcpyAsync(h.data(), V->W, h.size() * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    if (int st = vecchia_status(f, who)) return st;
    if (logd) memcpy(logd, h.data(), n * sizeof(double));
    memcpy(out, h.data() + n, n * c * sizeof(double));
    return 0;
}

extern "C" int cocons_vecchia_whiten(cocons_fit *f, const double *theta, int c, const double *B, double *out, double *logd)
{
    return vecchia_whiten_impl("cocons_vecchia_whiten", false, f, theta, c, B, out, logd);
}

// cocons_vecchia_predict, or with search (cocons_vecchia_predict_knn) the same with every chunk's table found on
// the device: the neighbours land ascending in the chunk's table buffer, no table is uploaded and none is sorted on the host;
// or with corr the same with the chunk's table re-ranked by model correlation, or that table alone
// (corr->nn_out)
int vecchia_predict_impl(const char *who, cocons_fit *f, const double *theta, const double *mean, int z_col, int mp,
                         const double *locs_pred, const double *X_pred, int m_pred, const int *nn_pred, bool search,
                         double *stochastic, double *quadform, const CorrPredSource *corr)
{
    const bool table_only = corr && corr->nn_out;
    if (corr) search = true;                    // (no table comes in either way)
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || (!table_only && !mean)) return fail(-1, "%s: null argument", who);
    if (mp < 0 || (mp > 0 && (!locs_pred || !X_pred || (!search && !nn_pred) || (!table_only && (!stochastic || !quadform)))))
        return fail(-1, "%s: bad argument (mp < 0 or a null pointer)", who);
    if (corr) {
        if (int rc = corr_check_shape(who, corr->m_cand, corr->hops, m_pred)) return rc;
    } else if (m_pred < 1 || m_pred > VECCHIA_M_MAX)
        return fail(-1, "%s: m_pred = %d is outside 1 .. %d", who, m_pred, VECCHIA_M_MAX);
    if (mp > 0)
        if (int rc = pattern_check_finite(who, "locs_pred", (size_t)mp, locs_pred)) return rc;
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (!table_only && (z_col < 0 || z_col >= f->r)) return fail(-1, "%s: z_col = %d is outside 0 .. %d", who, z_col, f->r - 1);
    if (corr)
        if (int rc = corr_check_theta(who, theta, f->p)) return rc;
    VecchiaState *V = f->vecchia.get();
    const int n = f->n, p = f->p, rows = VECCHIA_PRED_ROWS;
    std::vector<int> tab;
    if (!search) {
        tab.resize((size_t)mp * m_pred);
        for (int i = 0; i < mp; ++i)
            if (int bad = vecchia_row(nn_pred, (size_t)mp, m_pred, (size_t)i, n, &tab[(size_t)i * m_pred]))
                return fail(-1, "%s: row %d of nn_pred %s (1-based indices in 1 .. n, 0 = none)", who, i + 1, vecchia_offence[bad]);
    }
    if (mp == 0) return 0;
    double hmean[COCONS_P_MAX] = {};
    for (int i = 0; i < p && !table_only; ++i) hmean[i] = canon_nan(mean[i]);
    // the chunk's buffers: locals of the call (device memory does not grow with mp)
    DevBuf<double> dXp, dlp, dsoa, drec, dst, dqd;
    DevBuf<int> dnb, dfirst, dnn;
    HIPCHK_AT(who, dXp.alloc((size_t)rows * p));
    HIPCHK_AT(who, dlp.alloc((size_t)rows * 2));
    HIPCHK_AT(who, dsoa.alloc((size_t)rows * LOCP_FIELDS));
    HIPCHK_AT(who, drec.alloc((size_t)rows * VECCHIA_REC));
    HIPCHK_AT(who, dst.alloc((size_t)rows));
    HIPCHK_AT(who, dqd.alloc((size_t)rows));
    HIPCHK_AT(who, dnb.alloc((size_t)rows * m_pred));
    if (corr) HIPCHK_AT(who, dfirst.alloc((size_t)rows * corr->m_cand));
    if (table_only) HIPCHK_AT(who, dnn.alloc((size_t)rows * m_pred));
    StreamDrain s{f->stream, false};
    if (int rc = reset_info(f)) return rc;
    if (corr) {
        if (int rc = corr_pred_prepare(who, f, corr->m_cand, corr->hops, s)) return rc;
    } else if (search) {
        if (int rc = vecchia_need_grid(who, f, s)) return rc;
    }
    // K from cov_rns's records; c from the prediction branch's (always logistic + sqrt, see cocons_predict_dense): a second
    // set of records only where the two differ (a fixed smoothness)
    const ModeSel ms2 = select_mode(theta, p, f->smooth_limits, 2);
    const double *aosC = V->aos;
    if (select_mode(theta, p, f->smooth_limits, 0).smooth_kind != ms2.smooth_kind) {
        HIPCHK_AT(who, V->aos2.reserve((size_t)VECCHIA_REC * n, f->stream, nullptr));
        vecchia_records(f, theta, 2, V->aos2);
        aosC = V->aos2;
    }
    const ModeSel ms = vecchia_records(f, theta, 0, V->aos);
    if (!table_only) launch_vecchia_resid(n, p, f->dX, n, hmean, f->dz, n, z_col, 1, V->B, (size_t)n, s);
    ThetaVecs tv;
    make_theta_vecs(theta, p, tv);
    std::vector<double> hX((size_t)rows * p), hl((size_t)rows * 2), hst(table_only ? 0 : (size_t)mp), hqd(hst.size());
    std::vector<int> hnn(table_only ? (size_t)mp * m_pred : 0), hnc(table_only ? (size_t)rows * m_pred : 0);
    for (int b = 0; b < mp; b += rows) {
        const int mc = std::min(rows, mp - b);
        for (int j = 0; j < p; ++j) memcpy(&hX[(size_t)j * mc], X_pred + b + (size_t)j * mp, (size_t)mc * sizeof(double));
        for (int j = 0; j < 2; ++j) memcpy(&hl[(size_t)j * mc], locs_pred + b + (size_t)j * mp, (size_t)mc * sizeof(double));
        HIPCHK_AT(who, upload_canon(dXp, hX.data(), (size_t)mc * p, s));
        HIPCHK_AT(who, upload_canon(dlp, hl.data(), (size_t)mc * 2, s));
        // the chunk's records in front of the table step: they do not depend on the table, and the third source reads them
        launch_loc_params(loc_args(mc, p, dXp, dlp, dsoa, rows, tv, ms2.smooth_kind, f->smooth_limits), s);
        launch_vecchia_aos(dsoa, rows, mc, drec, s);
        if (corr) {
            if (int rc = corr_pred_chunk(who, f, *corr, m_pred, mc, b, dlp, drec, aosC, ms.gr, dfirst, dnb, dnn, s)) return rc;
            // a rho that is not finite leaves its row of the table unwritten: nothing may read the table then
            HIPCHK_AT(who, hipMemcpyAsync(f->hinfo, f->dinfo, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
            if (table_only)
                HIPCHK_AT(who, hipMemcpyAsync(hnc.data(), dnn, (size_t)mc * m_pred * sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK_AT(who, hipStreamSynchronize(s));
            if (f->hinfo[0] != 0x7f7f7f7f) {
                if (f->hinfo[0] <= b) break;             // (a block of an earlier chunk: vecchia_status names it)
                return fail(f->hinfo[0], "%s: row %d has a candidate whose correlation is not finite", who, f->hinfo[0]);
            }
            if (table_only) {
                for (int j = 0; j < m_pred; ++j) memcpy(&hnn[b + (size_t)j * mp], &hnc[(size_t)j * mc], (size_t)mc * sizeof(int));
                continue;
            }
        } else if (search) {
            KnnArgs k;
            k.t = V->knn->t; k.qx = dlp; k.qy = dlp + mc; k.m = m_pred; k.tab = dnb;
            HIPCHK_AT(who, launch_knn_query(k, mc, s));
        } else {
            HIPCHK_AT(who, hipMemcpyAsync(dnb, &tab[(size_t)b * m_pred], (size_t)mc * m_pred * sizeof(int), hipMemcpyHostToDevice, s));
        }
        VecchiaArgs a;
        a.rows = mc; a.m = m_pred; a.kb = m_pred + 1; a.nbr = dnb;
        a.aosK = V->aos; a.aosC = aosC; a.aosP = drec;
        a.gr = ms.gr; a.nu_fixed = ms.nu_fixed;
        a.B = V->B; a.ldb = (size_t)n; a.nb = 1;
        a.stoch = dst; a.quad = dqd;
        a.fail = f->dinfo; a.row0 = b;
        launch_vecchia_blocks(ms.mode, true, a, s);
        HIPCHK_AT(who, hipMemcpyAsync(&hst[b], dst, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipMemcpyAsync(&hqd[b], dqd, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipGetLastError());
        HIPCHK_AT(who, hipStreamSynchronize(s));         // the staging is used again
    }
    if (int st = vecchia_status(f, who)) return st;
    if (table_only) {
        std::copy(hnn.begin(), hnn.end(), corr->nn_out);
        return 0;
    }
    memcpy(stochastic, hst.data(), (size_t)mp * sizeof(double));
    memcpy(quadform, hqd.data(), (size_t)mp * sizeof(double));
    return 0;
}

int vecchia_need_grid(const char *who, cocons_fit *f, hipStream_t s)
{
    VecchiaState *V = f->vecchia.get();
    if (V->knn) return 0;
    // the grid over the observations: the handle's from here on (counted by cocons_vecchia_info, freed with it)
    const int n = f->n;
    V->knn.reset(new PatternGridBufs());
    if (int rc = knn_grid_build(who, *V->knn, n, f->h_locs.data(), f->h_locs.data() + n, f->dlocs, f->dlocs + n, s)) {
        (void)hipStreamSynchronize(s);
        V->knn.reset();
        return rc;
    }
    return 0;
}

extern "C" int cocons_vecchia_predict(cocons_fit *f, const double *theta, const double *mean, int z_col, int mp,
                                      const double *locs_pred, const double *X_pred, int m_pred, const int *nn_pred,
                                      double *stochastic, double *quadform)
{
    return vecchia_predict_impl("cocons_vecchia_predict", f, theta, mean, z_col, mp, locs_pred, X_pred, m_pred, nn_pred, false,
                                stochastic, quadform);
}
