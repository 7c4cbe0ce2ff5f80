// api_predict.hip -- C ABI, what is made of a factor: the one-shot predictions (cocons_predict_dense / _taper), kriging from a
// held factor -- prepare, apply in chunks and joint prediction (predictive covariance and draws), for dense handles and for the
// band factor of tapered fits, over one set of shared helpers (KrigeHeld's allocation, krige_chunks, the argument builders,
// krige_joint_tail; the bucket sort of a chunk's entries is band_plan.hpp's) --, the marginal and conditional simulations,
// cocons_chol_solve.
#include "fit.hpp"

// row row0 of out: the residual z[:, z_col] - X mean over the columns [0, ncols), then nrows_zero rows cleared.  out is in
// the handle's layout (skew; a dense handle's is 0, the layout of cocons_sim_cond_dense's own buffer too)
static void residual_row(cocons_fit *f, const double *mean, int z_col, double *out, size_t ld, int row0, int nrows_zero,
                         int ncols)
{
    RhsArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.n = f->n; ra.p = f->p; ra.X = f->dX; ra.ldx = f->n; ra.use_trend = 1;
    for (int i = 0; i < f->p; ++i) ra.mean[i] = canon_nan(mean[i]);
    ra.src = f->dz + (size_t)z_col * f->n; ra.lds = f->n;
    ra.out = out; ra.ld = ld; ra.row0 = row0; ra.nrows = 1; ra.nrows_zero = nrows_zero;
    ra.col0 = 0; ra.ncols_out = ncols;
    ra.skew = f->skew; ra.npad = f->npad;
    launch_rhs_rows(ra, f->stream);
}

// no right-hand sides: clear the rows under the matrix
static void clear_border(cocons_fit *f)
{
    RhsArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.n = f->n; ra.p = f->p; ra.X = f->dX; ra.ldx = f->n; ra.src = f->dX; ra.lds = f->n;
    ra.out = f->dA; ra.ld = f->lda; ra.row0 = f->npad; ra.nrows = 0; ra.nrows_zero = f->rhs_act;
    ra.col0 = 0; ra.ncols_out = f->npad;
    ra.skew = f->skew; ra.npad = f->npad;
    launch_rhs_rows(ra, f->stream);
}

// trend X %*% mean of the simulations on the host (O(n p)), as the reference does (R/sim.R:170), in the handle's order
static std::vector<double> host_trend(const cocons_fit *f, const double *mean)
{
    const int n = f->n;
    std::vector<double> tr(n, 0.0);
    for (int j = 0; j < f->p; ++j)
        for (int i = 0; i < n; ++i) tr[i] += f->h_X[(size_t)i + (size_t)j * n] * mean[j];
    return tr;
}

// ---------------------------------------------------------------------------
// the handle's buffers of the prediction entries, grown to m new locations
static int pred_reserve(cocons_fit *f, int m)
{
    HIPCHK(f->dlocp.reserve((size_t)LOCP_FIELDS * m, f->stream, f->stream2));
    HIPCHK(f->dXp.reserve((size_t)m * f->p, f->stream, f->stream2));
    HIPCHK(f->dlocsp.reserve((size_t)m * 2, f->stream, f->stream2));
    HIPCHK(f->dstoch.reserve((size_t)m, f->stream, f->stream2));
    HIPCHK(f->dquad.reserve((size_t)m, f->stream, f->stream2));
    HIPCHK(f->dred.reserve(row_reduce_scratch_doubles(f->n, m), f->stream, f->stream2));
    return 0;
}

// kriging core: rows under the matrix = [ (z - X mean)' ; cov_rns_pred (m x n) ]
extern "C" int cocons_predict_dense(cocons_fit *f, const double *theta, const double *mean, int z_col,
                                    int m, const double *locs_pred, const double *X_pred,
                                    double *stochastic, double *quadform)
{
    const char *who = "cocons_predict_dense";
    FIT_ENTER(f);
    if (int rc = no_taper(f, who)) return rc;
    if (!theta || !mean || m <= 0 || !locs_pred || !X_pred || !stochastic || !quadform || z_col < 0 || z_col >= f->r)
        return fail(-1, "%s: bad argument", who);
    const int p = f->p, n = f->n;
    if (int rc = pred_reserve(f, m)) return rc;
    if (int rc = fit_alloc_matrix(f, m + 1)) return rc;
    hipStream_t s = f->stream;
    HIPCHK_AT(who, upload_canon(f->dXp, X_pred, (size_t)m * p, s));
    HIPCHK_AT(who, upload_canon(f->dlocsp, locs_pred, (size_t)m * 2, s));
    ThetaVecs tv;
    make_theta_vecs(theta, p, tv);
    const ModeSel ms = select_mode(theta, p, f->smooth_limits, 2);
    const ModeSel ms0 = select_mode(theta, p, f->smooth_limits, 0);
    return run_op(f, who, [&]() -> int {
        assemble_sigma(f, theta, 0, 0, f->npad);
        // row npad: residual of realization z_col (also clears padding rows and columns >= n); rows npad+1 .. npad+m:
        // cross-covariance
        residual_row(f, mean, z_col, f->dA, f->lda, f->npad, f->rhs_act - 1, f->npad);
        launch_loc_params(loc_args(m, p, f->dXp, f->dlocsp, f->dlocp, m, tv, ms.smooth_kind, f->smooth_limits), s);
        PairArgs pa;
        memset(&pa, 0, sizeof pa);
        pa.n = n; pa.m = m; pa.rows = f->dlocp; pa.stride_rows = m; pa.cols = f->dloc; pa.stride = f->npad;
        pa.out = f->dA + f->npad + 1; pa.ld = f->lda; pa.nrows_out = m; pa.ncols_out = n;
        pa.gr = ms.gr; pa.nu_fixed = 0.0;
        // Sigma was assembled from dloc above (stream order); rebuild dloc only if cov_rns used a
        // different smoothness vector (fixed-nu branch) than cov_rns_pred does: the observation-side SoA must use the
        // pred-branch smoothness (always logistic+sqrt, :381)
        if (ms0.smooth_kind != ms.smooth_kind)
            launch_loc_params(loc_args(n, p, f->dX, f->dlocs, f->dloc, f->npad, tv, ms.smooth_kind, f->smooth_limits), s);
        launch_pair_rect(MODE_GEOM, pa, s);
        // (the dependency-driven schedule may take the head of this factorisation too -- round 6: the row reductions below read the
        // factor from both buffers like the objectives' do; with m rows under the matrix every step is a long one)
        FactorView pv = main_view(f);
        pv.dag_ok = true;
        if (int rc = factorize(f, pv, nullptr)) return rc;
        launch_row_reduce(f->dA, f->lda, n, f->npad, f->npad + 1, m, f->dstoch, f->dquad, f->dred, s, 0, 0,
                          f->dag_used ? f->dP : nullptr, f->dag_used ? 2 * TILE * f->dag_nsteps : 0);
        HIPCHK_AT(who, hipMemcpyAsync(stochastic, f->dstoch, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipMemcpyAsync(quadform, f->dquad, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
        return 0;
    });
}

// ---------------------------------------------------------------------------
// Kriging from a held factor: cocons_krige_prepare factors Sigma(theta) once (residual row of z_col as the one right-hand
// side) and keeps the factor in the handle's KrigeState; cocons_krige_apply then predicts any number of new locations in
// chunks of `rows` against it -- cross-covariance chunk (pair_rect), V = C L^-T with both reductions fused
// (launch_krige_solve) -- with device memory independent of m.  Outputs as cocons_predict_dense's.
// What these entries share with the tapered ones further down stands here once, over KrigeHeld (fit.hpp: what both states hold).
static constexpr size_t KRIGE_CHUNK_BYTES = (size_t)1 << 30;      // max_rows = 0: the chunk buffers stay within 1 GiB
static constexpr int KRIGE_ROWS_CAP = 16384;                       // ... and within 16384 rows

// bytes of one chunk row: `wide` doubles in the state's own chunk buffer (C: npad, the ring: W * 128), then Xp, lp, locp, st, qd
static size_t krige_row_bytes(const cocons_fit *f, size_t wide) { return (wide + (size_t)f->p + 2 + LOCP_FIELDS + 2) * sizeof(double); }

// rows per chunk: a caller's max_rows, cut at user_cap where the entry has one (0: none), or what the two limits above
// leave; whole 64-row strips (a row's position in its strip never depends on the split), one at least
static int krige_rows(int max_rows, size_t row_bytes, size_t user_cap)
{
    size_t r = max_rows > 0 ? (size_t)max_rows : std::min<size_t>(KRIGE_CHUNK_BYTES / row_bytes, KRIGE_ROWS_CAP);
    if (max_rows > 0 && user_cap) r = std::min(r, user_cap);
    return (int)std::max<size_t>(r / 64 * 64, 64);
}

// theta and mean canonicalised into the state, and KrigeHeld's buffers for a factor of ntile packed tiles and chunks of K->rows
// rows; *bytes: those buffers' and, at row_bytes a row, the chunk buffer's of the state itself, which the caller allocates
static int krige_held_alloc(const cocons_fit *f, const char *who, KrigeHeld *K, const double *theta, const double *mean, size_t ntile,
                            size_t row_bytes, long long *bytes)
{
    const int p = f->p;
    const size_t R = (size_t)K->rows, nt = (size_t)f->nt, npad = (size_t)f->npad;
    K->theta.resize((size_t)6 * p);
    for (int i = 0; i < 6 * p; ++i) K->theta[i] = canon_nan(theta[i]);
    K->mean.resize((size_t)p);
    for (int i = 0; i < p; ++i) K->mean[i] = canon_nan(mean[i]);
    HIPCHK_AT(who, K->L.alloc(ntile * TILE * TILE));
    HIPCHK_AT(who, K->Q.alloc(nt * 2048));
    HIPCHK_AT(who, K->w.alloc(npad));
    HIPCHK_AT(who, K->loc.alloc(LOCP_FIELDS * npad));
    HIPCHK_AT(who, K->Xp.alloc(R * p));
    HIPCHK_AT(who, K->lp.alloc(R * 2));
    HIPCHK_AT(who, K->locp.alloc(R * LOCP_FIELDS));
    HIPCHK_AT(who, K->st.alloc(R));
    HIPCHK_AT(who, K->qd.alloc(R));
    *bytes = (long long)((ntile * TILE * TILE + nt * 2048 + npad * (1 + LOCP_FIELDS)) * sizeof(double) + R * row_bytes);
    return 0;
}

// the end of a prepare, behind the factor's pack launch: the observation-side SoA in the prediction branch's smoothness
// (always logistic + sqrt, see cocons_predict_dense) -- full_scale: with the FULL scale vector, as cocons_cov_rns_taper_pred
// prepares it --, and the stream drained
static int krige_prepare_finish(cocons_fit *f, const char *who, KrigeHeld *K, bool full_scale)
{
    const double *th = K->theta.data();
    ThetaVecs tv;
    make_theta_vecs(th, f->p, tv, full_scale);
    const ModeSel ms = select_mode(th, f->p, f->smooth_limits, 2);
    launch_loc_params(loc_args(f->n, f->p, f->dX, f->dlocs, K->loc, f->npad, tv, ms.smooth_kind, f->smooth_limits), f->stream);
    HIPCHK_AT(who, hipGetLastError());
    HIPCHK_AT(who, hipStreamSynchronize(f->stream));
    return 0;
}

static int krige_no_state(const char *who, const char *prepare)
{
    return fail(-1, "%s: no kriging state on this handle (call %s first)", who, prepare);
}

// The chunk loop of an apply call: rows [b, b + mc) of the caller's column-major X_pred (m x p) and locs_pred (m x 2) into the
// state's staging, their SoA in the prediction branch's parameters (full_scale: as krige_prepare_finish), body(b, mc, global
// range) -- the entry's own launches, which leave the chunk's outputs in K->st and K->qd --, those to the caller's rows, and
// the stream drained before the staging, the host's and the state's, is used again.  before(b, mc) comes behind the uploads
// of the chunk's rows (K->Xp, K->lp) and ahead of every launch of the loop: the entry's step that makes the chunk's pattern --
// host work and uploads of its own (cocons_krige_taper_apply), or the search on the device from K->lp (..._apply_delta).
template <class Before, class Body>
static int krige_chunks(cocons_fit *f, KrigeHeld *K, const char *who, bool full_scale, int m, const double *locs_pred,
                        const double *X_pred, double *stochastic, double *quadform, Before &&before, Body &&body)
{
    const int p = f->p, rows = K->rows;
    ThetaVecs tv;
    make_theta_vecs(K->theta.data(), p, tv, full_scale);
    const ModeSel ms = select_mode(K->theta.data(), p, f->smooth_limits, 2);
    std::vector<double> hX((size_t)rows * p), hl((size_t)rows * 2);
    StreamDrain s{f->stream, false};
    for (int b = 0; b < m; b += rows) {
        const int mc = std::min(rows, m - b);
        for (int j = 0; j < p; ++j) memcpy(&hX[(size_t)j * mc], X_pred + b + (size_t)j * m, (size_t)mc * sizeof(double));
        for (int j = 0; j < 2; ++j) memcpy(&hl[(size_t)j * mc], locs_pred + b + (size_t)j * m, (size_t)mc * sizeof(double));
        HIPCHK_AT(who, upload_canon(K->Xp, hX.data(), (size_t)mc * p, s));
        HIPCHK_AT(who, upload_canon(K->lp, hl.data(), (size_t)mc * 2, s));
        if (int rc = before(b, mc)) return rc;
        launch_loc_params(loc_args(mc, p, K->Xp, K->lp, K->locp, rows, tv, ms.smooth_kind, f->smooth_limits), s);
        if (int rc = body(b, mc, ms.gr)) return rc;
        HIPCHK_AT(who, hipMemcpyAsync(stochastic + b, K->st, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipMemcpyAsync(quadform + b, K->qd, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipGetLastError());
        HIPCHK_AT(who, hipStreamSynchronize(s));
    }
    return 0;
}

// the cross-covariance of m new locations (their SoA in `rows`, stride ld) with the caller's observations only -- columns
// [pad0, n) in the handle's order -- into those columns of V (m x npad, leading dimension ld)
static PairArgs krige_cross_args(const cocons_fit *f, const KrigeHeld *K, int m, const double *rows, double *V, size_t ld, double gr)
{
    PairArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.n = f->n_user; pa.m = m; pa.rows = rows; pa.stride_rows = ld;
    pa.cols = K->loc + f->pad0; pa.stride = f->npad;
    pa.out = V + (size_t)f->pad0 * ld; pa.ld = ld; pa.nrows_out = m; pa.ncols_out = f->n_user;
    pa.gr = gr; pa.nu_fixed = 0.0;
    return pa;
}

static int krige_sharded(cocons_fit *f, const char *who)
{
    if (f->coll_kind && f->coll_world > 1) return fail(-1, "%s: not available on a sharded handle (world > 1)", who);
    return 0;
}

extern "C" int cocons_krige_prepare(cocons_fit *f, const double *theta, const double *mean, int z_col, int max_rows)
{
    const char *who = "cocons_krige_prepare";
    if (!f) return fail(-1, "%s: null fit handle", who);
    FIT_ENTER(f);
    if (int rc = no_taper(f, who)) return rc;
    if (int rc = krige_sharded(f, who)) return rc;
    if (!theta || !mean || z_col < 0 || z_col >= f->r || max_rows < 0) return fail(-1, "%s: bad argument", who);
    f->krige.reset();                   // replaced -- and gone if this prepare fails
    const int n = f->n, npad = f->npad, nt = f->nt;
    std::unique_ptr<KrigeState> K(new KrigeState());
    const size_t row_bytes = krige_row_bytes(f, (size_t)npad), ntile = (size_t)nt * (nt + 1) / 2;
    K->rows = krige_rows(max_rows, row_bytes, 0);
    const size_t R = (size_t)K->rows;
    StreamDrain s{f->stream, false};
    if (int rc = krige_held_alloc(f, who, K.get(), theta, mean, ntile, row_bytes, &K->bytes)) return rc;
    HIPCHK_AT(who, K->C.alloc(R * npad));
    // the padding and slot columns of a chunk are never written by the assembly: zero once
    HIPCHK_AT(who, hipMemsetAsync(K->C, 0, R * npad * sizeof(double), s));
    const double *th = K->theta.data();
    if (int rc = fit_alloc_matrix(f, 1)) return rc;
    const int st = run_op(f, who, [&]() -> int {
        f->nrhs_cur = 1;
        assemble_sigma(f, th, 0, 0, npad);
        // row npad: residual of realization z_col (the rows under it and the columns >= n cleared)
        residual_row(f, mean, z_col, f->dA, f->lda, npad, f->rhs_act - 1, npad);
        // the plain schedules (dag_ok = false): the factor lies whole in dA, with L^-1 r in row npad
        if (int rc = factorize(f, main_view(f), nullptr)) return rc;
        launch_krige_pack(f->dA, f->lda, nt, npad, f->pad0, n, K->L, K->Q, K->w, s);
        return 0;
    });
    if (st) return st;                  // failing minor: no state (K's buffers are freed on the way out)
    if (int rc = krige_prepare_finish(f, who, K.get(), false)) return rc;
    f->krige = std::move(K);
    return 0;
}

extern "C" int cocons_krige_apply(cocons_fit *f, int m, const double *locs_pred, const double *X_pred,
                                  double *stochastic, double *quadform)
{
    const char *who = "cocons_krige_apply";
    if (m < 0 || (m > 0 && (!locs_pred || !X_pred || !stochastic || !quadform)))
        return fail(-1, "%s: bad argument (m < 0 or a null pointer)", who);
    if (!f) return fail(-1, "%s: null fit handle", who);
    FIT_ENTER(f);
    if (int rc = no_taper(f, who)) return rc;
    if (int rc = krige_sharded(f, who)) return rc;
    KrigeState *K = f->krige.get();
    if (!K) return krige_no_state(who, "cocons_krige_prepare");
    hipStream_t s = f->stream;
    auto solve = [&](int, int mc, double gr) -> int {
        launch_pair_rect(MODE_GEOM, krige_cross_args(f, K, mc, K->locp, K->C, (size_t)K->rows, gr), s);
        launch_krige_solve(K->L, K->Q, K->w, f->nt, K->C, K->rows, mc, f->pad0, f->n, K->st, K->qd, s);
        return 0;
    };
    return krige_chunks(f, K, who, false, m, locs_pred, X_pred, stochastic, quadform, [](int, int) { return 0; }, solve);
}

extern "C" int cocons_krige_release(cocons_fit *f)
{
    if (!f) return fail(-1, "cocons_krige_release: null fit handle");
    FIT_ENTER(f);
    f->krige.reset();                   // (every entry point drains the main stream before it returns: nothing in flight uses it)
    return 0;
}

// out4 = { prepared (0 / 1), device bytes held, rows per chunk, n }
extern "C" int cocons_krige_info(cocons_fit *f, long long *out4)
{
    if (!f) return fail(-1, "cocons_krige_info: null fit handle");
    if (!out4) return fail(-1, "cocons_krige_info: null argument");
    FIT_ENTER(f);
    const KrigeState *K = f->krige.get();
    out4[0] = K ? 1 : 0;
    out4[1] = K ? K->bytes : 0;
    out4[2] = K ? K->rows : 0;
    out4[3] = f->n_user;
    return 0;
}

// mu[i] = X_pred[i, ] mean + stv[i]: tmp_mu of the conditional draws on the host, X_pred column-major m x p (this loop order
// and this order of summation: the draws' bits depend on them)
static void add_trend_to(double *mu, const double *X_pred, int m, int p, const double *mean, const double *stv)
{
    for (int i = 0; i < m; ++i) {
        double sys = 0;
        for (int j = 0; j < p; ++j) sys += X_pred[(size_t)i + (size_t)j * m] * mean[j];
        mu[i] = sys + stv[i];
    }
}

// doubles of the twelve buffers both joint entries allocate, in their order: `first` (V, or the ring) | S | Xp, lp, lu |
// locp, locu | st, q | E, Y | mu.  None is zero.
static void krige_joint_counts(const cocons_fit *f, int m, int nsim, size_t first, size_t counts[12])
{
    const size_t mv = (size_t)round_up(m, 64), mpad = (size_t)round_up(m, TILE), ne = (size_t)m * (size_t)nsim;
    const size_t c[12] = {first, mpad * mpad, (size_t)m * f->p, (size_t)m * 2, (size_t)m * 2, (size_t)LOCP_FIELDS * mv,
                          (size_t)LOCP_FIELDS * mpad, mv, mv, ne ? ne : 1, ne ? ne : 1, (size_t)m};
    memcpy(counts, c, sizeof c);
}

// One joint call as krige_joint_tail takes it: the view S (round_up(m, 128) rows and columns, leading dimension lds), the
// solve's stochastic in dst, the uploaded draws dE, room for the fields and their mean, and the caller's outputs.
struct KrigeJointCall {
    const char *who; int m, nsim; size_t lds;
    double *dS, *dst, *dE, *dY, *dmu;
    const double *X_pred, *mean;
    double *stochastic, *cov, *sims;
    bool plain;                      // the view is factored under PlainSchedule (a band handle: DESIGN.md 4p)
};

// What both joint entries do once head() has enqueued everything up to the mirrored predictive covariance in S: stochastic and
// cov home; with draws, tmp_mu on the host, the factorisation of the view -- it does not start with the handle's observations
// (FoldView), and the schedules with dag_ok = false leave the factor whole in it: no second buffer -- and sims = L_S E + tmp_mu.
// Without draws nothing is factored: no info words, nothing to repeat.  The caller's outputs are written only once the whole
// call has succeeded (cov through a staging copy).  The host ends of the copies are locals here: hence the drain of its own.
template <class Head> static int krige_joint_tail(cocons_fit *f, const KrigeJointCall &c, Head &&head)
{
    const char *who = c.who;
    const int m = c.m, nsim = c.nsim;
    const size_t ne = (size_t)m * (size_t)nsim;
    std::vector<double> stv((size_t)m), mu((size_t)m), hY(ne), hcov;
    if (c.cov && nsim > 0) hcov.resize((size_t)m * m);
    double *cov_to = hcov.empty() ? c.cov : hcov.data();
    int raw = 0x7f7f7f7f;                                // the view's own info word (minors counted from the view's first column)
    StreamDrain s{f->stream, false};
    auto enqueue = [&]() -> int {
        if (int rc = head()) return rc;
        HIPCHK_AT(who, hipMemcpyAsync(stv.data(), c.dst, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
        if (c.cov)
            HIPCHK_AT(who, hipMemcpy2DAsync(cov_to, (size_t)m * sizeof(double), c.dS, c.lds * sizeof(double), (size_t)m * sizeof(double),
                                            (size_t)m, hipMemcpyDeviceToHost, s));
        if (nsim == 0) return 0;
        HIPCHK_AT(who, hipStreamSynchronize(s));
        add_trend_to(mu.data(), c.X_pred, m, f->p, c.mean, stv.data());
        HIPCHK_AT(who, upload_canon(c.dmu, mu.data(), (size_t)m, s));
        {
            // a dense view of the call, maybe of more tiles than the handle's nt: factorize() sizes the hand-off words and the
            // mailboxes by the view (flags_reset, mbox_reset), dinv and dinfo do not depend on the order
            std::unique_ptr<PlainSchedule> plain(c.plain ? new PlainSchedule(f) : nullptr);
            FoldView fv(f);
            FactorView v;
            v.A = c.dS; v.lda = c.lds; v.nt = (int)(c.lds / TILE); v.mt = v.nt;
            if (int rc = factorize(f, v, nullptr)) return rc;
        }
        HIPCHK_AT(who, hipMemcpyAsync(&raw, f->dinfo, sizeof(int), hipMemcpyDeviceToHost, s));
        launch_trmm_lower(c.dS, c.lds, m, c.dE, m, nsim, c.dmu, c.dY, m, s);
        HIPCHK_AT(who, hipMemcpyAsync(hY.data(), c.dY, ne * sizeof(double), hipMemcpyDeviceToHost, s));
        return 0;
    };
    if (nsim == 0) {
        if (int rc = enqueue()) return rc;
        HIPCHK_AT(who, hipGetLastError());
        HIPCHK_AT(who, hipStreamSynchronize(s));
    } else {
        f->nrhs_cur = 0;
        const int st = run_op(f, who, enqueue);
        if (st > 0)
            return fail(-5, "%s: the predictive covariance is not positive definite (leading minor %d of %d not positive)", who,
                        raw, m);
        if (st < 0) {
            const std::string why = g_err;
            return why.compare(0, strlen(who), who) == 0 ? st : fail(st, "%s: %s", who, why.c_str());
        }
        memcpy(c.sims, hY.data(), ne * sizeof(double));
        if (!hcov.empty()) memcpy(c.cov, hcov.data(), hcov.size() * sizeof(double));
    }
    memcpy(c.stochastic, stv.data(), (size_t)m * sizeof(double));
    return 0;
}

// Joint prediction from the held factor: the predictive covariance between the new locations and conditional draws,
//   cov  = Sigma_uu - C Sigma^-1 C'                 (R/predict.R:136-183 gives its diagonal only)
//   sims = L_S E + (X_pred mean + stochastic),  L_S L_S' = cov        (R/sim.R:84-127, cocons_sim_cond_dense's output)
// against the theta, realisation and mean of cocons_krige_prepare.  With V = C L^-T as launch_krige_solve leaves it in a
// buffer of the call, cov = Sigma_uu - V V': one symmetric product on the fp64 MFMA (launch_krige_schur) into a view of
// the call that holds Sigma_uu (cov_rns semantics at locs_unobs, as cocons_sim_cond_dense's block), mirrored to the bit;
// the draws then cost a factorisation of m, not of n + m (krige_joint_tail).
// Device memory of the call: round_up(m, 64) x npad + round_up(m, 128)^2 doubles and the small arrays, all released on return.
extern "C" int cocons_krige_joint(cocons_fit *f, int m, const double *locs_pred, const double *X_pred, const double *locs_unobs,
                                  double *stochastic, double *cov, int nsim, const double *iiderrors, double *sims)
{
    const char *who = "cocons_krige_joint";
    if (m < 1) return fail(-1, "%s: m = %d (at least one new location is needed)", who, m);
    if (!locs_pred || !X_pred || !stochastic) return fail(-1, "%s: null locs_pred, X_pred or stochastic", who);
    if (nsim < 0) return fail(-1, "%s: nsim = %d is negative", who, nsim);
    if (nsim > 0 && (!iiderrors || !sims)) return fail(-1, "%s: nsim = %d with a null iiderrors or sims", who, nsim);
    if (!f) return fail(-1, "%s: null fit handle", who);
    FIT_ENTER(f);
    if (int rc = no_taper(f, who)) return rc;
    if (int rc = krige_sharded(f, who)) return rc;
    const KrigeState *K = f->krige.get();
    if (!K) return krige_no_state(who, "cocons_krige_prepare");
    const int p = f->p, npad = f->npad, pad0 = f->pad0;
    if (m > INT_MAX - TILE) return fail(-1, "%s: m = %d is too large", who, m);
    const int mv = round_up(m, 64), mpad = round_up(m, TILE);
    const size_t ldv = (size_t)mv, lds = (size_t)mpad, ne = (size_t)m * (size_t)nsim;
    const double *lu = locs_unobs ? locs_unobs : locs_pred;
    const double *th = K->theta.data();
    DevBuf<double> dV, dS, dXp, dlp, dlu, dlocp, dlocu, dst, dq, dE, dY, dmu;
    StreamDrain s{f->stream, false};
    {
        size_t counts[12], total = 0;
        krige_joint_counts(f, m, nsim, ldv * npad, counts);
        DevBuf<double> *bufs[12] = {&dV, &dS, &dXp, &dlp, &dlu, &dlocp, &dlocu, &dst, &dq, &dE, &dY, &dmu};
        for (int k = 0; k < 12; ++k) total += counts[k];
        if (hipError_t e = alloc_call_buffers(bufs, counts, 12))
            return fail(-100 - (int)e, "%s: the device cannot hold the %zu bytes of the call (m = %d new locations, n = %d): %s",
                        who, total * sizeof(double), m, f->n_user, hipGetErrorString(e));
    }
    // rows >= m, the padding columns and the slot columns of V are never written by the assembly
    HIPCHK_AT(who, hipMemsetAsync(dV, 0, ldv * npad * sizeof(double), s));
    HIPCHK_AT(who, upload_canon(dXp, X_pred, (size_t)m * p, s));
    HIPCHK_AT(who, upload_canon(dlp, locs_pred, (size_t)m * 2, s));
    HIPCHK_AT(who, upload_canon(dlu, lu, (size_t)m * 2, s));
    if (nsim > 0) HIPCHK_AT(who, upload_canon(dE, iiderrors, ne, s));
    ThetaVecs tv;
    make_theta_vecs(th, p, tv);
    const ModeSel ms0 = select_mode(th, p, f->smooth_limits, 0);   // cov_rns semantics (Sigma_uu)
    const ModeSel msp = select_mode(th, p, f->smooth_limits, 2);   // cov_rns_pred semantics (C)
    const KrigeJointCall call = {who, m, nsim, lds, dS, dst, dE, dY, dmu, X_pred, K->mean.data(), stochastic, cov, sims, false};
    return krige_joint_tail(f, call, [&]() -> int {
        launch_loc_params(loc_args(m, p, dXp, dlp, dlocp, ldv, tv, msp.smooth_kind, f->smooth_limits), s);
        launch_loc_params(loc_args(m, p, dXp, dlu, dlocu, lds, tv, ms0.smooth_kind, f->smooth_limits), s);
        launch_pair_rect(MODE_GEOM, krige_cross_args(f, K, m, dlocp, dV, ldv, msp.gr), s);
        launch_krige_solve(K->L, K->Q, K->w, f->nt, dV, ldv, m, pad0, f->n, dst, dq, s);
        // Sigma_uu, identity in the rows and columns [m, mpad)
        PairArgs pa;
        memset(&pa, 0, sizeof pa);
        pa.n = m; pa.m = m; pa.rows = dlocu; pa.cols = dlocu; pa.stride = lds; pa.stride_rows = lds;
        pa.out = dS; pa.ld = lds; pa.nrows_out = mpad; pa.ncols_out = mpad; pa.gr = ms0.gr; pa.nu_fixed = ms0.nu_fixed;
        launch_pair_sym(ms0.mode, false, pa, s);
        launch_krige_schur(dV, ldv, m, pad0, f->n, npad, dS, lds, s);
        launch_sym_mirror(dS, lds, m, s);
        return 0;
    });
}

// Kriging core of the sparse branch of cocoPredict (R/predict.R:216-283) on a taper handle: S = taper o
// cov_rns_taper(theta) as in the objective, C = pred_taper o cov_rns_taper_pred(theta) (m x n, its own pattern);
// one bordered DENSE factorisation replaces  inv_cov <- spam::solve(S, t(C))  ("memory intensive", :244) and gives
//   stochastic[i] = C[i,] S^-1 resid    (:252)      quadform[i] = C[i,] S^-1 C[i,]'    (:267)
extern "C" int cocons_predict_taper(cocons_fit *f, const double *theta, const double *mean, int z_col, int m,
                                    const double *locs_pred, const double *X_pred, int nnz_pred,
                                    const int *colindices_pred, const int *rowpointers_pred,
                                    const double *taper_entries_pred, double *stochastic, double *quadform)
{
    const char *who = "cocons_predict_taper";
    FIT_ENTER(f);
    if (f->taper_nnz <= 0) return fail(-1, "%s: not a taper fit", who);
    if (!theta || !mean || m <= 0 || !locs_pred || !X_pred || !stochastic || !quadform || z_col < 0 || z_col >= f->r ||
        nnz_pred < 0 || !rowpointers_pred || (nnz_pred > 0 && (!colindices_pred || !taper_entries_pred)))
        return fail(-1, "%s: bad argument", who);
    const int p = f->p, n = f->n;
    if (rowpointers_pred[0] != 1 || rowpointers_pred[m] != nnz_pred + 1)
        return fail(-1, "%s: rowpointers do not match nnz (1-based CSR expected)", who);
    for (int w = 0; w < nnz_pred; ++w)
        if (colindices_pred[w] < 1 || colindices_pred[w] > n) return fail(-1, "%s: column index out of range", who);
    if (int rc = pred_reserve(f, m)) return rc;
    if (int rc = fit_alloc_matrix(f, m + 1)) return rc;
    const size_t nz = nnz_pred > 0 ? (size_t)nnz_pred : 1;
    DevBuf<int> dci, drp;
    DevBuf<double> dtv;
    StreamDrain s{f->stream, false};
    HIPCHK_AT(who, dci.alloc(nz));
    HIPCHK_AT(who, drp.alloc((size_t)m + 1));
    HIPCHK_AT(who, dtv.alloc(nz));
    HIPCHK_AT(who, upload_canon(f->dXp, X_pred, (size_t)m * p, s));
    HIPCHK_AT(who, upload_canon(f->dlocsp, locs_pred, (size_t)m * 2, s));
    HIPCHK_AT(who, hipMemcpyAsync(drp, rowpointers_pred, (size_t)(m + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    if (nnz_pred > 0) {
        std::vector<int> mapped(nnz_pred);          // the pattern's columns in the handle's order of the observations
        for (int w = 0; w < nnz_pred; ++w) mapped[w] = f->taper_inv[colindices_pred[w] - 1] + 1;
        HIPCHK_AT(who, hipMemcpy(dci, mapped.data(), (size_t)nnz_pred * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK_AT(who, upload_canon(dtv, taper_entries_pred, (size_t)nnz_pred, s));
    }
    // parameters as cocons_cov_rns_taper_pred prepares them: FULL scale vector, prediction-branch smoothness
    ThetaVecs tv;
    make_theta_vecs(theta, p, tv, true);
    const ModeSel ms = select_mode(theta, p, f->smooth_limits, 2);
    return run_op(f, who, [&]() -> int {
        if (int rc = assemble_sigma_taper(f, theta)) return rc;      // zeroes the whole buffer, border rows included
        residual_row(f, mean, z_col, f->dA, f->lda, f->npad, f->rhs_act - 1, f->npad);
        launch_loc_params(loc_args(m, p, f->dXp, f->dlocsp, f->dlocp, m, tv, ms.smooth_kind, f->smooth_limits), s);
        // (the observation side after the entries of S were computed from it: stream order)
        launch_loc_params(loc_args(n, p, f->dX, f->dlocs, f->dloc, f->npad, tv, ms.smooth_kind, f->smooth_limits), s);
        TaperLaunch t;
        t.mode = MODE_GEOM; t.pred = true; t.nrows = m; t.nnz = nnz_pred; t.ci = dci; t.rp = drp;
        t.rows = f->dlocp; t.stride_rows = m; t.cols = f->dloc; t.stride = f->npad;
        t.tapv = dtv; t.A = f->dA; t.lda = f->lda; t.row0 = f->npad + 1; t.skew = f->skew; t.npad = f->npad;
        launch_taper(t, s);
        if (int rc = factorize(f, main_view(f), nullptr)) return rc;
        launch_row_reduce(f->dA, f->lda, n, f->npad, f->npad + 1, m, f->dstoch, f->dquad, f->dred, s, f->skew, f->npad);
        HIPCHK_AT(who, hipMemcpyAsync(stochastic, f->dstoch, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipMemcpyAsync(quadform, f->dquad, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
        return 0;
    });
}

// ---------------------------------------------------------------------------
// Kriging from a held band factor: cocons_predict_taper in two parts.  cocons_krige_taper_prepare factors
// S(theta) once with the residual row under it and copies the envelope's tiles, the solve operands and w = L^-1 r out of dA
// into the handle's KrigeTaperState; cocons_krige_taper_apply then predicts any number of new locations in chunks against
// it: the chunk's entries from the taper entry kernel, bucketed by tile column on the host, V = C L^-T through a ring of W
// tile columns (launch_krige_band_solve).  No factorisation in apply, device memory independent of m.
static constexpr int KRIGE_TAPER_ROWS_MAX = 1 << 20;               // a caller's max_rows beyond this is cut (slot offsets are ints)

static int krige_taper_handle(cocons_fit *f, const char *who)
{
    if (f->taper_nnz <= 0) return fail(-1, "%s: not a taper fit (cocons_krige_prepare serves a dense handle)", who);
    return krige_sharded(f, who);
}

// the CSR staging holds at least `entries` entries; a new allocation only when it has to grow (the stream is idle then)
static int krige_taper_stage(KrigeTaperState *K, size_t entries, const char *who)
{
    if (entries <= K->ecap) return 0;
    HIPCHK_AT(who, K->ci.alloc(entries));
    HIPCHK_AT(who, K->bdst.alloc(entries));
    HIPCHK_AT(who, K->bsrc.alloc(entries));
    HIPCHK_AT(who, K->tv.alloc(entries));
    HIPCHK_AT(who, K->val.alloc(entries));
    K->ecap = entries;
    return 0;
}

// a caller's m x ncols pattern: 1-based CSR, columns strictly increasing within a row (what: "" or which pattern of the call)
static int krige_taper_csr_check(const char *who, const char *what, int m, int ncols, int nnz, const int *ci, const int *rp)
{
    if (rp[0] != 1 || rp[m] != nnz + 1) return fail(-1, "%s: %srowpointers do not match nnz (1-based CSR expected)", who, what);
    for (int i = 0; i < m; ++i) {
        const int a = rp[i], b = rp[i + 1];
        if (b < a || a < 1 || b > nnz + 1) return fail(-1, "%s: %srowpointers decrease at row %d", who, what, i + 1);
        for (int w = a - 1; w < b - 1; ++w) {
            const int c = ci[w];
            if (c < 1 || c > ncols) return fail(-1, "%s: %scolumn index out of range (row %d)", who, what, i + 1);
            if (w > a - 1 && c <= ci[w - 1])
                return fail(-1, "%s: %scolumn indices of row %d are not strictly increasing", who, what, i + 1);
        }
    }
    return 0;
}

// the entries of a pred pattern (ci / rp on the device, columns in the handle's order) between nrows new locations -- their
// SoA in `rows` -- and the observations, prediction branch, one value per entry into val
static TaperLaunch krige_pred_taper(const cocons_fit *f, const KrigeHeld *K, int nrows, int nnz, const int *ci, const int *rp,
                                    const double *rows, size_t stride_rows, double *val)
{
    TaperLaunch t;
    t.mode = MODE_GEOM; t.pred = true; t.nrows = nrows; t.nnz = nnz; t.ci = ci; t.rp = rp;
    t.rows = rows; t.stride_rows = stride_rows; t.cols = K->loc; t.stride = f->npad;
    t.out = val;
    return t;
}

// the ring solve of `rows` new locations against the held band factor: what apply and joint both set (boff on the host, the
// other arrays on the device); the joint entry adds Wr, depth, S and lds
static KrigeBandSolve krige_band_solve_args(const cocons_fit *f, const KrigeTaperState *K, double *ring, size_t ldr, int rows,
                                            const int *boff, const int *bdst, const int *bsrc, const double *val,
                                            const double *tapv, double *stoch, double *quad)
{
    KrigeBandSolve a;
    a.Lp = K->L; a.Qp = K->Q; a.w = K->w; a.toff = K->plan.toff.data(); a.hi = envelope_or_null(f);
    a.nt = f->nt; a.W = K->plan.W; a.ring = ring; a.ldr = ldr; a.rows = rows;
    a.boff = boff; a.bdst = bdst; a.bsrc = bsrc; a.val = val; a.tapv = tapv;
    a.stoch = stoch; a.quad = quad;
    return a;
}

extern "C" int cocons_krige_taper_prepare(cocons_fit *f, const double *theta, const double *mean, int z_col, int max_rows)
{
    const char *who = "cocons_krige_taper_prepare";
    if (!f) return fail(-1, "%s: null fit handle", who);
    FIT_ENTER(f);
    if (int rc = krige_taper_handle(f, who)) return rc;
    if (!theta || !mean || z_col < 0 || z_col >= f->r || max_rows < 0) return fail(-1, "%s: bad argument", who);
    f->krige_taper.reset();             // replaced -- and gone if this prepare fails
    const int n = f->n, npad = f->npad, nt = f->nt;
    std::unique_ptr<KrigeTaperState> K(new KrigeTaperState());
    const size_t row_bytes = krige_row_bytes(f, (size_t)band_W(f) * TILE);
    K->rows = krige_rows(max_rows, row_bytes, KRIGE_TAPER_ROWS_MAX);
    if (const char *why = band_plan(nt, envelope_or_null(f), f->taper_maxband, K->plan)) return fail(-1, "%s: %s", who, why);
    const size_t R = (size_t)K->rows, ntile = (size_t)K->plan.toff[nt];
    // the staging starts at the densest row of the handle's own pattern for every row of a chunk
    size_t dens = 1;
    for (int i = 0; i < n; ++i) dens = std::max<size_t>(dens, (size_t)(f->h_trp[i + 1] - f->h_trp[i]));
    StreamDrain s{f->stream, false};
    if (int rc = krige_held_alloc(f, who, K.get(), theta, mean, ntile, row_bytes, &K->fixed_bytes)) return rc;
    HIPCHK_AT(who, K->ring.alloc(R * K->plan.W * TILE));
    HIPCHK_AT(who, K->d_toff.alloc((size_t)nt));
    HIPCHK_AT(who, K->rp.alloc(R + 1));
    if (int rc = krige_taper_stage(K.get(), R * dens, who)) return rc;
    K->fixed_bytes += (long long)(((size_t)nt + R + 1) * sizeof(int));
    HIPCHK_AT(who, hipMemcpyAsync(K->d_toff, K->plan.toff.data(), (size_t)nt * sizeof(int), hipMemcpyHostToDevice, s));
    const double *th = K->theta.data();
    if (int rc = fit_alloc_matrix(f, 1)) return rc;
    const int st = run_op(f, who, [&]() -> int {
        f->nrhs_cur = 1;
        if (int rc = factor_on_band_schedule(f, th, K->plan, [&] {
                residual_row(f, mean, z_col, f->dA, f->lda, npad, f->rhs_act - 1, npad);
            })) return rc;
        launch_krige_band_pack(f->dA, f->lda, f->skew, npad, n, f->d_thi, nt, K->plan.W, K->d_toff, K->L, K->Q, K->w, s);
        return 0;
    });
    if (st) return st;                  // failing minor: no state
    if (int rc = krige_prepare_finish(f, who, K.get(), true)) return rc;
    f->krige_taper = std::move(K);
    return 0;
}

extern "C" int cocons_krige_taper_apply(cocons_fit *f, int m, const double *locs_pred, const double *X_pred, int nnz_pred,
                                        const int *colindices_pred, const int *rowpointers_pred,
                                        const double *taper_entries_pred, double *stochastic, double *quadform)
{
    const char *who = "cocons_krige_taper_apply";
    if (m < 0 || nnz_pred < 0 || (m > 0 && (!locs_pred || !X_pred || !rowpointers_pred || !stochastic || !quadform)) ||
        (m > 0 && nnz_pred > 0 && (!colindices_pred || !taper_entries_pred)))
        return fail(-1, "%s: bad argument (m < 0, nnz_pred < 0 or a null pointer)", who);
    if (!f) return fail(-1, "%s: null fit handle", who);
    FIT_ENTER(f);
    if (int rc = krige_taper_handle(f, who)) return rc;
    KrigeTaperState *K = f->krige_taper.get();
    if (!K) return krige_no_state(who, "cocons_krige_taper_prepare");
    if (m == 0) return 0;
    const int nt = f->nt, rows = K->rows;
    // the whole pattern is checked before any device work
    if (int rc = krige_taper_csr_check(who, "", m, f->n, nnz_pred, colindices_pred, rowpointers_pred)) return rc;
    // the CSR staging grows to the call's densest chunk before the first one is enqueued (the stream is idle)
    size_t dens = 0;
    for (int b = 0; b < m; b += rows) dens = std::max<size_t>(dens, (size_t)(rowpointers_pred[std::min(b + rows, m)] - rowpointers_pred[b]));
    if (int rc = krige_taper_stage(K, dens, who)) return rc;
    std::vector<int> hrp((size_t)rows + 1), hci, hdst, hsrc, boff;
    hipStream_t s = f->stream;
    // the chunk's pattern on its way to the staging: row pointers counted from its first entry, columns in the handle's order,
    // buckets per tile column
    auto pattern = [&](int b, int mc) -> int {
        const int e0 = rowpointers_pred[b] - 1, ne = rowpointers_pred[b + mc] - 1 - e0;
        for (int i = 0; i <= mc; ++i) hrp[i] = rowpointers_pred[b + i] - e0;
        band_buckets<TILE>(nt, f->taper_inv.data(), colindices_pred, rowpointers_pred, b, mc, rows, hci, hdst, hsrc, boff);
        HIPCHK_AT(who, hipMemcpyAsync(K->rp, hrp.data(), (size_t)(mc + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        if (ne > 0) {
            HIPCHK_AT(who, hipMemcpyAsync(K->ci, hci.data(), (size_t)ne * sizeof(int), hipMemcpyHostToDevice, s));
            HIPCHK_AT(who, hipMemcpyAsync(K->bdst, hdst.data(), (size_t)ne * sizeof(int), hipMemcpyHostToDevice, s));
            HIPCHK_AT(who, hipMemcpyAsync(K->bsrc, hsrc.data(), (size_t)ne * sizeof(int), hipMemcpyHostToDevice, s));
            HIPCHK_AT(who, upload_canon(K->tv, taper_entries_pred + e0, (size_t)ne, s));
        }
        return 0;
    };
    return krige_chunks(f, K, who, true, m, locs_pred, X_pred, stochastic, quadform, pattern, [&](int b, int mc, double) -> int {
        const int ne = rowpointers_pred[b + mc] - rowpointers_pred[b];
        launch_taper(krige_pred_taper(f, K, mc, ne, K->ci, K->rp, K->locp, (size_t)rows, K->val), s);
        HIPCHK_AT(who, launch_krige_band_solve(krige_band_solve_args(f, K, K->ring, (size_t)rows, mc, boff.data(), K->bdst, K->bsrc,
                                                                     K->val, K->tv, K->st, K->qd), s));
        return 0;
    });
}

// cocons_krige_taper_apply with the pattern found on the device: per chunk, from its locations in K->lp and the
// grid over the observations in the handle's order (f->dlocs: no taper_inv), the count pass with the histogram of the tile
// columns, both scans, the nt + 1 bucket offsets to the host -- the one wait of the step, and what says how many entries the
// chunk holds --, then columns, taper values and buckets straight into the staging.
extern "C" int cocons_krige_taper_apply_delta(cocons_fit *f, int m, const double *locs_pred, const double *X_pred, double delta,
                                              int kind, double *stochastic, double *quadform, long long *nnz_out)
{
    const char *who = "cocons_krige_taper_apply_delta";
    if (m < 0 || (m > 0 && (!locs_pred || !X_pred || !stochastic || !quadform)))
        return fail(-1, "%s: bad argument (m < 0 or a null pointer)", who);
    if (int rc = pattern_check_delta(who, delta, kind)) return rc;
    if (m > 0)
        if (int rc = pattern_check_finite(who, "locs_pred", (size_t)m, locs_pred)) return rc;
    if (!f) return fail(-1, "%s: null fit handle", who);
    FIT_ENTER(f);
    if (int rc = krige_taper_handle(f, who)) return rc;
    KrigeTaperState *K = f->krige_taper.get();
    if (!K) return krige_no_state(who, "cocons_krige_taper_prepare");
    if (m == 0) { if (nnz_out) *nnz_out = 0; return 0; }
    const int nt = f->nt, n = f->n, rows = K->rows;
    hipStream_t s = f->stream;
    // the grid over the observations: made by the first call on this state, and again for another delta
    if (!K->grid || K->grid->delta != delta) {
        HIPCHK_AT(who, hipStreamSynchronize(s));
        K->grid.reset(new PatternGridBufs());
        HIPCHK_AT(who, K->bwork.alloc((size_t)3 * (nt + 1)));
        if (int rc = pattern_grid_build(who, *K->grid, n, f->h_locs.data(), f->h_locs.data() + n, f->dlocs, f->dlocs + n, delta, s)) {
            hipStreamSynchronize(s);
            K->grid.reset();
            return rc;
        }
    }
    const PatternTargets &T = K->grid->t;
    int *hist = K->bwork, *d_boff = hist + (nt + 1), *cursor = d_boff + (nt + 1);
    std::vector<int> boff((size_t)nt + 1);
    long long total = 0;
    int ne = 0;
    auto pattern = [&](int, int mc) -> int {
        const double *qx = K->lp, *qy = K->lp + mc;
        HIPCHK_AT(who, hipMemsetAsync(hist, 0, ((size_t)nt + 1) * sizeof(int), s));
        HIPCHK_AT(who, launch_pattern_count(T, mc, qx, qy, delta, K->rp, hist, TILE, s));
        HIPCHK_AT(who, launch_scan_exclusive(K->rp, K->rp, mc, 1, nullptr, s));
        HIPCHK_AT(who, launch_scan_exclusive(hist, d_boff, nt, 0, nullptr, s));
        HIPCHK_AT(who, hipMemcpyAsync(boff.data(), d_boff, ((size_t)nt + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipStreamSynchronize(s));
        // (a bucket holds at most rows x 128 entries, so the differences are exact even where the offsets wrapped)
        long long cnt = 0;
        for (int I = 0; I < nt; ++I) cnt += (long long)(unsigned)(boff[I + 1] - boff[I]);
        if (cnt > INT_MAX)
            return fail(-1, "%s: a chunk of %d rows holds %lld entries, more than an int counts (prepare with a smaller max_rows)",
                        who, mc, cnt);
        ne = (int)cnt;
        total += cnt;
        if (int rc = krige_taper_stage(K, (size_t)ne, who)) return rc;      // (the stream is idle)
        if (ne > 0) {
            HIPCHK_AT(who, launch_pattern_fill(T, mc, qx, qy, delta, kind, K->rp, K->ci, K->tv, s));
            HIPCHK_AT(who, hipMemcpyAsync(cursor, d_boff, (size_t)nt * sizeof(int), hipMemcpyDeviceToDevice, s));
            HIPCHK_AT(who, launch_pattern_buckets(mc, K->rp, K->ci, TILE, rows, cursor, K->bdst, K->bsrc, s));
        }
        return 0;
    };
    const int rc = krige_chunks(f, K, who, true, m, locs_pred, X_pred, stochastic, quadform, pattern, [&](int, int mc, double) -> int {
        launch_taper(krige_pred_taper(f, K, mc, ne, K->ci, K->rp, K->locp, (size_t)rows, K->val), s);
        HIPCHK_AT(who, launch_krige_band_solve(krige_band_solve_args(f, K, K->ring, (size_t)rows, mc, boff.data(), K->bdst, K->bsrc,
                                                                     K->val, K->tv, K->st, K->qd), s));
        return 0;
    });
    if (rc == 0 && nnz_out) *nnz_out = total;
    return rc;
}

extern "C" int cocons_krige_taper_release(cocons_fit *f)
{
    if (!f) return fail(-1, "cocons_krige_taper_release: null fit handle");
    FIT_ENTER(f);
    f->krige_taper.reset();             // (every entry point drains the main stream before it returns: nothing in flight uses it)
    return 0;
}

// out6 = { prepared (0 / 1), device bytes held, rows per chunk, n, W (slots of the ring), nt (tile columns) }
extern "C" int cocons_krige_taper_info(cocons_fit *f, long long *out6)
{
    const char *who = "cocons_krige_taper_info";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!out6) return fail(-1, "%s: null argument", who);
    FIT_ENTER(f);
    if (int rc = krige_taper_handle(f, who)) return rc;
    const KrigeTaperState *K = f->krige_taper.get();
    out6[0] = K ? 1 : 0;
    out6[1] = K ? K->bytes() : 0;
    out6[2] = K ? K->rows : 0;
    out6[3] = f->n;
    out6[4] = band_W(f);
    out6[5] = f->nt;
    return 0;
}

// Joint prediction of a tapered fit from the held band factor: cocons_krige_joint's outputs,
//   cov  = S_uu - C S^-1 C'         sims = L_S E + (X_pred mean + stochastic),  L_S L_S' = cov,
// against the theta, realisation and mean of cocons_krige_taper_prepare.  C = pred_taper o cov_rns_taper_pred exactly as one
// chunk of cocons_krige_taper_apply forms it; S_uu = taper_uu o cov_rns_taper at locs_unobs (the objective's entry kernel
// straight into the lower triangle of the call's view S, identity on its padding).  V = C L^-T is never held as rows x n:
// the ring solve runs with a ring depth - 1 slots deeper and S -= V_g V_g' leaves for S group by group of `depth` tile
// columns while the window slides (launch_krige_band_solve).  Mirror, copy out; the draws are cocons_krige_joint's tail on
// the plain schedule (a band handle has no resident engine, and every handle of a fit then draws the same bits).
// Everything on the device belongs to the call; the kriging state is read only.
static constexpr int KRIGE_JOINT_DEPTH = 8;                        // tile columns per Schur launch (measured)

// COCONS_KRIGE_JOINT_DEPTH, read per call: 1 .. 16, or refused
static int krige_joint_depth(const char *who, int *depth)
{
    *depth = KRIGE_JOINT_DEPTH;
    const char *e = getenv("COCONS_KRIGE_JOINT_DEPTH");
    if (!e || !*e) return 0;
    char *end = nullptr;
    const long v = strtol(e, &end, 10);
    if (*end || v < 1 || v > 16) return fail(-1, "%s: COCONS_KRIGE_JOINT_DEPTH = \"%s\" (1 .. 16 expected)", who, e);
    *depth = (int)v;
    return 0;
}

// what every refusal of the two entries that needs no device work shares; K out
static int krige_taper_joint_enter(cocons_fit *f, const char *who, int m, int *depth, const KrigeTaperState **K)
{
    if (int rc = krige_taper_handle(f, who)) return rc;
    *K = f->krige_taper.get();
    if (!*K) return krige_no_state(who, "cocons_krige_taper_prepare");
    if (m > KRIGE_TAPER_ROWS_MAX) return fail(-1, "%s: m = %d is too large (at most %d rows in one call)", who, m, KRIGE_TAPER_ROWS_MAX);
    return krige_joint_depth(who, depth);
}

// slots of the joint call's ring: depth - 1 more than the state's, all tile columns at most
static int krige_joint_ring_slots(const cocons_fit *f, const KrigeTaperState *K, int depth)
{
    return std::min(K->plan.W + depth - 1, f->nt);
}

extern "C" int cocons_krige_taper_joint_bytes(cocons_fit *f, int m, int nsim, long long *bytes)
{
    const char *who = "cocons_krige_taper_joint_bytes";
    if (m < 1) return fail(-1, "%s: m = %d (at least one new location is needed)", who, m);
    if (nsim < 0) return fail(-1, "%s: nsim = %d is negative", who, nsim);
    if (!bytes) return fail(-1, "%s: null argument", who);
    if (!f) return fail(-1, "%s: null fit handle", who);
    FIT_ENTER(f);
    int depth = 0;
    const KrigeTaperState *K = nullptr;
    if (int rc = krige_taper_joint_enter(f, who, m, &depth, &K)) return rc;
    size_t counts[12], total = 0;
    krige_joint_counts(f, m, nsim, (size_t)round_up(m, 64) * krige_joint_ring_slots(f, K, depth) * TILE, counts);
    for (int k = 0; k < 12; ++k) total += counts[k];
    *bytes = (long long)(total * sizeof(double) + 2 * ((size_t)m + 1) * sizeof(int));      // ... and the two row-pointer arrays
    return 0;
}

extern "C" int cocons_krige_taper_joint(cocons_fit *f, int m, const double *locs_pred, const double *X_pred, int nnz_pred,
                                        const int *colindices_pred, const int *rowpointers_pred,
                                        const double *taper_entries_pred, const double *locs_unobs, int nnz_uu,
                                        const int *colindices_uu, const int *rowpointers_uu, const double *taper_entries_uu,
                                        double *stochastic, double *cov, int nsim, const double *iiderrors, double *sims)
{
    const char *who = "cocons_krige_taper_joint";
    if (m < 1) return fail(-1, "%s: m = %d (at least one new location is needed)", who, m);
    if (!locs_pred || !X_pred || !stochastic || !rowpointers_pred || !rowpointers_uu)
        return fail(-1, "%s: null locs_pred, X_pred, stochastic or row pointers", who);
    if (nnz_pred < 0 || (nnz_pred > 0 && (!colindices_pred || !taper_entries_pred)))
        return fail(-1, "%s: nnz_pred = %d is negative, or comes with a null colindices_pred or taper_entries_pred", who, nnz_pred);
    if (nnz_uu < 1 || !colindices_uu || !taper_entries_uu)
        return fail(-1, "%s: nnz_uu = %d (every row holds its diagonal), or a null colindices_uu or taper_entries_uu", who, nnz_uu);
    if (nsim < 0) return fail(-1, "%s: nsim = %d is negative", who, nsim);
    if (nsim > 0 && (!iiderrors || !sims)) return fail(-1, "%s: nsim = %d with a null iiderrors or sims", who, nsim);
    if (!f) return fail(-1, "%s: null fit handle", who);
    FIT_ENTER(f);
    int D = 0;
    const KrigeTaperState *K = nullptr;
    if (int rc = krige_taper_joint_enter(f, who, m, &D, &K)) return rc;
    const int p = f->p, n = f->n, nt = f->nt, Wr = krige_joint_ring_slots(f, K, D);
    // both patterns are checked before any device work; a uu row holds its diagonal entry
    if (int rc = krige_taper_csr_check(who, "pred pattern: ", m, n, nnz_pred, colindices_pred, rowpointers_pred)) return rc;
    if (int rc = krige_taper_csr_check(who, "uu pattern: ", m, m, nnz_uu, colindices_uu, rowpointers_uu)) return rc;
    for (int i = 0; i < m; ++i) {
        const int *a = colindices_uu + rowpointers_uu[i] - 1, *b = colindices_uu + rowpointers_uu[i + 1] - 1;
        if (!std::binary_search(a, b, i + 1)) return fail(-1, "%s: uu pattern: row %d does not hold its diagonal entry", who, i + 1);
    }
    const int mv = round_up(m, 64), mpad = round_up(m, TILE);
    const size_t ldr = (size_t)mv, lds = (size_t)mpad, nsm = (size_t)m * (size_t)nsim;
    const size_t ne = (size_t)nnz_pred, nu = (size_t)nnz_uu;
    const double *lu = locs_unobs ? locs_unobs : locs_pred;
    const double *th = K->theta.data();
    // the pred pattern as one chunk of cocons_krige_taper_apply, in slots of mv rows
    std::vector<int> hci, hdst, hsrc, boff;
    band_buckets<TILE>(nt, f->taper_inv.data(), colindices_pred, rowpointers_pred, 0, m, mv, hci, hdst, hsrc, boff);
    DevBuf<double> dring, dS, dXp, dlp, dlu, dlocp, dlocu, dst, dq, dE, dY, dmu, dtvp, dval, dtvu;
    DevBuf<int> dcip, drpp, dbdst, dbsrc, dciu, drpu;
    StreamDrain s{f->stream, false};
    {
        size_t counts[15], total = 0;
        krige_joint_counts(f, m, nsim, ldr * Wr * TILE, counts);
        counts[12] = ne ? ne : 1; counts[13] = ne ? ne : 1; counts[14] = nu;
        DevBuf<double> *bufs[15] = {&dring, &dS, &dXp, &dlp, &dlu, &dlocp, &dlocu, &dst, &dq, &dE, &dY, &dmu, &dtvp, &dval, &dtvu};
        const size_t icounts[6] = {ne ? ne : 1, (size_t)m + 1, ne ? ne : 1, ne ? ne : 1, nu, (size_t)m + 1};
        DevBuf<int> *ibufs[6] = {&dcip, &drpp, &dbdst, &dbsrc, &dciu, &drpu};
        for (int k = 0; k < 15; ++k) total += counts[k] * sizeof(double);
        for (int k = 0; k < 6; ++k) total += icounts[k] * sizeof(int);
        hipError_t e = alloc_call_buffers(bufs, counts, 15);
        for (int k = 0; k < 6 && e == hipSuccess; ++k)
            if ((e = ibufs[k]->alloc(icounts[k])) != hipSuccess) (void)hipGetLastError();
        if (e != hipSuccess)
            return fail(-100 - (int)e, "%s: the device cannot hold the %zu bytes of the call (m = %d new locations, %d ring slots, "
                        "n = %d): %s", who, total, m, Wr, f->n, hipGetErrorString(e));
    }
    HIPCHK_AT(who, upload_canon(dXp, X_pred, (size_t)m * p, s));
    HIPCHK_AT(who, upload_canon(dlp, locs_pred, (size_t)m * 2, s));
    HIPCHK_AT(who, upload_canon(dlu, lu, (size_t)m * 2, s));
    HIPCHK_AT(who, hipMemcpyAsync(drpp, rowpointers_pred, ((size_t)m + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK_AT(who, hipMemcpyAsync(drpu, rowpointers_uu, ((size_t)m + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK_AT(who, hipMemcpyAsync(dciu, colindices_uu, nu * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK_AT(who, upload_canon(dtvu, taper_entries_uu, nu, s));
    if (ne > 0) {
        HIPCHK_AT(who, hipMemcpyAsync(dcip, hci.data(), ne * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK_AT(who, hipMemcpyAsync(dbdst, hdst.data(), ne * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK_AT(who, hipMemcpyAsync(dbsrc, hsrc.data(), ne * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK_AT(who, upload_canon(dtvp, taper_entries_pred, ne, s));
    }
    if (nsim > 0) HIPCHK_AT(who, upload_canon(dE, iiderrors, nsm, s));
    // C: prediction-branch parameters (cocons_krige_taper_apply); S_uu: those of cocons_cov_rns_taper (the objective's)
    ThetaVecs tv;
    make_theta_vecs(th, p, tv, true);
    const ModeSel msp = select_mode(th, p, f->smooth_limits, 2);
    const ModeSel ms0 = select_mode(th, p, f->smooth_limits, 0);
    const KrigeJointCall call = {who, m, nsim, lds, dS, dst, dE, dY, dmu, X_pred, K->mean.data(), stochastic, cov, sims, true};
    return krige_joint_tail(f, call, [&]() -> int {
        launch_loc_params(loc_args(m, p, dXp, dlp, dlocp, ldr, tv, msp.smooth_kind, f->smooth_limits), s);
        launch_loc_params(loc_args(m, p, dXp, dlu, dlocu, lds, tv, ms0.smooth_kind, f->smooth_limits), s);
        launch_taper(krige_pred_taper(f, K, m, nnz_pred, dcip, drpp, dlocp, ldr, dval), s);
        // S_uu: the entries with column <= row times their taper value into the zeroed view, identity on [m, mpad)
        HIPCHK_AT(who, hipMemsetAsync(dS, 0, lds * mpad * sizeof(double), s));
        TaperLaunch u;
        u.mode = ms0.mode; u.nrows = m; u.nnz = nnz_uu; u.ci = dciu; u.rp = drpu; u.nu_fixed = ms0.nu_fixed;
        u.rows = u.cols = dlocu; u.stride_rows = u.stride = lds;
        u.tapv = dtvu; u.A = dS; u.lda = lds;
        launch_taper(u, s);
        launch_pad_identity(dS, lds, m, mpad, s);
        KrigeBandSolve a = krige_band_solve_args(f, K, dring, ldr, m, boff.data(), dbdst, dbsrc, dval, dtvp, dst, dq);
        a.Wr = Wr; a.depth = D; a.S = dS; a.lds = lds;
        HIPCHK_AT(who, launch_krige_band_solve(a, s));
        launch_sym_mirror(dS, lds, m, s);
        return 0;
    });
}

// ---------------------------------------------------------------------------
// Sparse branch of cocoSim (R/sim.R:177-217) on a taper handle: S = taper o cov_rns_taper(theta) assembled and factored as
// the objective does (the band schedule of the handle's envelope), then Y = L E + trend by band_trmm_kernel and the rows
// of Y gathered into the caller's order.  pos[i] = position of the caller's observation i in f's order.  Y in the handle's
// order: (L E)[k, s] + (X mean)[k], k a position of f.
extern "C" int cocons_fit_taper_order(cocons_fit *f, int *pivot_out)
{
    FIT_ENTER(f);
    if (f->taper_nnz <= 0) return fail(-1, "cocons_fit_taper_order: not a taper fit");
    if (!pivot_out) return fail(-1, "cocons_fit_taper_order: null argument");
    const std::vector<int> &inv = f->taper_inv;
    for (int i = 0; i < f->n; ++i) pivot_out[inv[i]] = i + 1;
    return 0;
}

static int sim_taper_run(cocons_fit *f, const double *theta, const double *mean, int nsim, const double *iiderrors,
                         const std::vector<int> &pos, double *out)
{
    const int n = f->n;
    const size_t ne = (size_t)n * nsim;
    const std::vector<double> tr = host_trend(f, mean);
    DevBuf<double> dE, dY, dO, dtr;
    DevBuf<int> dpos;
    StreamDrain s{f->stream, false};
    HIPCHK_AT("cocons_sim_taper", dE.alloc(ne));
    HIPCHK_AT("cocons_sim_taper", dY.alloc(ne));
    HIPCHK_AT("cocons_sim_taper", dO.alloc(ne));
    HIPCHK_AT("cocons_sim_taper", dtr.alloc((size_t)n));
    HIPCHK_AT("cocons_sim_taper", dpos.alloc((size_t)n));
    HIPCHK_AT("cocons_sim_taper", upload_canon(dE, iiderrors, ne, s));
    HIPCHK_AT("cocons_sim_taper", upload_canon(dtr, tr.data(), (size_t)n, s));
    HIPCHK_AT("cocons_sim_taper", hipMemcpyAsync(dpos, pos.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    if (int rc = fit_alloc_matrix(f, 1)) return rc;
    const int st = run_op(f, "cocons_sim_taper", [&]() -> int {
        f->nrhs_cur = 0;
        HIPCHK_AT("cocons_sim_taper", hipEventRecord(f->ev[4], s));
        if (int rc = assemble_sigma_taper(f, theta)) return rc;
        clear_border(f);
        if (int rc = factorize(f, main_view(f), nullptr)) return rc;
        HIPCHK_AT("cocons_sim_taper", hipEventRecord(f->ev[5], s));
        launch_band_trmm(f->dA, f->lda, f->skew, f->npad, f->d_thi, f->nt, n, dE, n, nsim, dtr, dY, n, s);
        HIPCHK_AT("cocons_sim_taper", hipEventRecord(f->ev[6], s));
        launch_gather_rows(dY, n, dpos, n, nsim, dO, n, s);
        HIPCHK_AT("cocons_sim_taper", hipEventRecord(f->ev[7], s));
        HIPCHK_AT("cocons_sim_taper", hipMemcpyAsync(out, dO, ne * sizeof(double), hipMemcpyDeviceToHost, s));
        return 0;
    });
    if (st == 0)
        for (int q = 0; q < 3; ++q) HIPCHK_AT("cocons_sim_taper", hipEventElapsedTime(&f->sim_ms[q], f->ev[4 + q], f->ev[5 + q]));
    return st;
}

extern "C" int cocons_sim_taper(cocons_fit *f, const double *theta, const double *mean, int nsim, const double *iiderrors,
                                const int *pivot, double *out)
{
    FIT_ENTER(f);
    if (f->taper_nnz <= 0) return fail(-1, "cocons_sim_taper: not a taper fit (cocons_sim_dense simulates on a dense handle)");
    if (!theta || !mean || nsim <= 0 || !iiderrors || !out) return fail(-1, "cocons_sim_taper: bad argument");
    const int n = f->n;
    const std::vector<int> &inv = f->taper_inv;          // inv[caller index] = position in f's order
    std::vector<int> tperm;                               // pivot route: twin position k <- position tperm[k] of f
    bool own = true;
    if (pivot) {
        std::vector<char> seen(n, 0);
        tperm.resize(n);
        for (int k = 0; k < n; ++k) {
            const int o = pivot[k] - 1;
            if (o < 0 || o >= n || seen[o]) return fail(-1, "cocons_sim_taper: pivot is not a permutation of 1..n");
            seen[o] = 1;
            tperm[k] = inv[o];
            if (tperm[k] != k) own = false;
        }
    }
    std::vector<int> pos(n);
    if (own) {                                            // the handle's own order: no twin
        for (int i = 0; i < n; ++i) pos[i] = inv[i];
        return sim_taper_run(f, theta, mean, nsim, iiderrors, pos, out);
    }
    // draw-equal route: the factor of S[pivot, pivot] -- a taper handle in that order, built once and kept while the callers
    // pass the same pivot (the fill-reducing order of spam's chol: computed once per coco object)
    if (!f->taper_twin || f->twin_perm != tperm) {
        if (f->taper_twin) { cocons_fit_destroy(f->taper_twin); f->taper_twin = nullptr; }
        f->krige.reset();                                       // (its buffers: the main stream is drained above)
        f->twin_perm.clear();
        cocons_fit *t = taper_create_ordered(n, f->p, f->r, f->h_locs.data(), f->h_X.data(), f->h_z.data(), f->smooth_limits,
                                             f->device, (int)f->h_tci.size(), f->h_tci.data(), f->h_trp.data(),
                                             f->h_tval.data(), tperm, true);
        if (!t) {
            const std::string why = g_err;
            return fail(-4, "cocons_sim_taper: no taper handle in the given pivot order (%s); pivot = NULL simulates in the "
                            "handle's own order (same distribution, another field for the same draws)", why.c_str());
        }
        f->taper_twin = t;
        f->twin_perm = tperm;
    }
    for (int k = 0; k < n; ++k) pos[pivot[k] - 1] = k;
    std::lock_guard<std::recursive_mutex> twin_guard(f->taper_twin->op_mu);
    if (int rc = fit_check(f->taper_twin)) return rc;
    return sim_taper_run(f->taper_twin, theta, mean, nsim, iiderrors, pos, out);
}

// (diagnostics) device times of the last successful cocons_sim_taper on the handle, in ms: assembly + factorisation,
// band product, gather into the caller's order (the twin's, when that call took the pivot route); out4[3] = the 128 x 128
// tiles of the envelope band_trmm_kernel reads per block of 64 draws
extern "C" int cocons_debug_sim_taper_ms(cocons_fit *f, int twin, double *out4)
{
    FIT_ENTER(f);
    if (!out4) return fail(-1, "cocons_debug_sim_taper_ms: null argument");
    const cocons_fit *g = twin ? f->taper_twin : f;
    if (!g) return fail(-1, "cocons_debug_sim_taper_ms: the handle has no twin");
    if (g->taper_nnz <= 0) return fail(-1, "cocons_debug_sim_taper_ms: not a taper fit");
    for (int q = 0; q < 3; ++q) out4[q] = g->sim_ms[q];
    double tiles = 0;
    if (g->taper_hi.empty()) tiles = 0.5 * g->nt * (g->nt + 1.0);
    else for (int c = 0; c < g->nt; ++c) tiles += g->taper_hi[c] - c;
    out4[3] = tiles;
    return 0;
}

// ---------------------------------------------------------------------------
// marginal simulation core: replaces R/sim.R:147-172
//   covmat <- cov_rns[_classic](...); cholS <- chol(covmat); t(sweep(t(iiderrors) %*% cholS, 2, X %*% mean, "+"))
extern "C" int cocons_sim_dense(cocons_fit *f, const double *theta, const double *mean, int classic,
                                int nsim, const double *iiderrors, double *out)
{
    FIT_ENTER(f);
    if (int rc = no_taper(f, "cocons_sim_dense")) return rc;
    if (!theta || !mean || nsim <= 0 || !iiderrors || !out) return fail(-1, "cocons_sim_dense: bad argument");
    if (f->sorted) {
        // L E depends on the ORDER of the observations (the factor of a permuted matrix is not the
        // permuted factor): the field for given draws is only reproduced in the caller's order
        if (!f->unsorted) {
            f->unsorted = fit_create_impl(f->n_user, f->p, f->r, 0, f->h_locs.data(), f->h_X.data(),
                                          f->r > 0 ? f->h_z.data() : nullptr, nullptr, f->smooth_limits,
                                          f->device, false);
            if (!f->unsorted) return -1;
        }
        return cocons_sim_dense(f->unsorted, theta, mean, classic, nsim, iiderrors, out);
    }
    const int n = f->n;
    if (int rc = fit_alloc_matrix(f, 1)) return rc;
    const std::vector<double> tr = host_trend(f, mean);
    DevBuf<double> dE, dY, dtr;
    StreamDrain s{f->stream, false};
    HIPCHK_AT("cocons_sim_dense", dE.alloc((size_t)n * nsim));
    HIPCHK_AT("cocons_sim_dense", dY.alloc((size_t)n * nsim));
    HIPCHK_AT("cocons_sim_dense", dtr.alloc((size_t)n));
    HIPCHK_AT("cocons_sim_dense", upload_canon(dE, iiderrors, (size_t)n * nsim, s));
    HIPCHK_AT("cocons_sim_dense", upload_canon(dtr, tr.data(), (size_t)n, s));
    return run_op(f, "cocons_sim_dense", [&]() -> int {
        f->nrhs_cur = 0;
        assemble_sigma(f, theta, classic ? 1 : 0, 0, f->npad);
        clear_border(f);
        if (int rc = factorize(f, main_view(f), nullptr)) return rc;
        launch_trmm_lower(f->dA, f->lda, n, dE, n, nsim, dtr, dY, n, s);
        HIPCHK_AT("cocons_sim_dense", hipMemcpyAsync(out, dY, (size_t)n * nsim * sizeof(double), hipMemcpyDeviceToHost, s));
        return 0;
    });
}

// ---------------------------------------------------------------------------
// conditional simulation core: replaces R/sim.R:84-127
//   covmat, covmat_pred, covmat_unobs; L <- chol(covmat_unobs - covmat_pred solve(covmat) t(covmat_pred));
//   t(sweep(t(iiderrors) %*% L, 2, systematic + stochastic, "+"))
// One Cholesky of the JOINT covariance of (observed, new) locations: its lower-right block is
// the factor of the Schur complement, and the kriging mean falls out of the border row, so the
// LU solve, the m x n x m product and the second chol of the reference are all this one pass.
extern "C" int cocons_sim_cond_dense(cocons_fit *f, const double *theta, const double *mean, int z_col,
                                     int m, const double *locs_pred, const double *X_pred,
                                     const double *locs_unobs, int nsim, const double *iiderrors, double *out)
{
    FIT_ENTER(f);
    if (int rc = no_taper(f, "cocons_sim_cond_dense")) return rc;
    if (!theta || !mean || m <= 0 || !locs_pred || !X_pred || !locs_unobs || nsim <= 0 || !iiderrors || !out ||
        z_col < 0 || z_col >= f->r)
        return fail(-1, "cocons_sim_cond_dense: bad argument");
    const int n = f->n, p = f->p, npad = f->npad;
    const int mpad = round_up(m, TILE), N = npad + mpad;
    const size_t ldj = (size_t)N + TILE;
    std::vector<double> mu(m), stv(m);
    DevBuf<double> dJ, dXp, dlp, dlu, dlocp, dlocu, dE, dY, dmu, dst, dq, dred;
    StreamDrain s{f->stream, false};
    HIPCHK_AT("cocons_sim_cond_dense", dJ.alloc(ldj * (size_t)N));
    HIPCHK_AT("cocons_sim_cond_dense", dXp.alloc((size_t)m * p));
    HIPCHK_AT("cocons_sim_cond_dense", dlp.alloc((size_t)m * 2));
    HIPCHK_AT("cocons_sim_cond_dense", dlu.alloc((size_t)m * 2));
    HIPCHK_AT("cocons_sim_cond_dense", dlocp.alloc((size_t)LOCP_FIELDS * mpad));
    HIPCHK_AT("cocons_sim_cond_dense", dlocu.alloc((size_t)LOCP_FIELDS * mpad));
    HIPCHK_AT("cocons_sim_cond_dense", dE.alloc((size_t)m * nsim));
    HIPCHK_AT("cocons_sim_cond_dense", dY.alloc((size_t)m * nsim));
    HIPCHK_AT("cocons_sim_cond_dense", dmu.alloc((size_t)m));
    HIPCHK_AT("cocons_sim_cond_dense", dst.alloc((size_t)m));
    HIPCHK_AT("cocons_sim_cond_dense", dq.alloc((size_t)m));
    HIPCHK_AT("cocons_sim_cond_dense", dred.alloc(row_reduce_scratch_doubles(n, m)));
    HIPCHK_AT("cocons_sim_cond_dense", upload_canon(dXp, X_pred, (size_t)m * p, s));
    HIPCHK_AT("cocons_sim_cond_dense", upload_canon(dlp, locs_pred, (size_t)m * 2, s));
    HIPCHK_AT("cocons_sim_cond_dense", upload_canon(dlu, locs_unobs, (size_t)m * 2, s));
    HIPCHK_AT("cocons_sim_cond_dense", upload_canon(dE, iiderrors, (size_t)m * nsim, s));
    ThetaVecs tv;
    make_theta_vecs(theta, p, tv);
    const ModeSel ms0 = select_mode(theta, p, f->smooth_limits, 0);   // cov_rns semantics
    const ModeSel msp = select_mode(theta, p, f->smooth_limits, 2);   // cov_rns_pred semantics
    const int st = run_op(f, "cocons_sim_cond_dense", [&]() -> int {
        f->nrhs_cur = 1;
        // the observed side, then the new locations twice: with the coordinates handed to cov_rns (covmat_unobs) and with
        // newlocs (cov_rns_pred, always logistic + sqrt)
        launch_loc_params(loc_args(n, p, f->dX, f->dlocs, f->dloc, npad, tv, ms0.smooth_kind, f->smooth_limits), s);
        launch_loc_params(loc_args(m, p, dXp, dlu, dlocu, mpad, tv, ms0.smooth_kind, f->smooth_limits), s);
        launch_loc_params(loc_args(m, p, dXp, dlp, dlocp, mpad, tv, msp.smooth_kind, f->smooth_limits), s);
        PairArgs pa;
        // Sigma_oo  (rows/cols [0, npad))
        memset(&pa, 0, sizeof pa);
        pa.n = n; pa.m = n; pa.rows = f->dloc; pa.cols = f->dloc; pa.stride = npad; pa.stride_rows = npad;
        pa.out = dJ; pa.ld = ldj; pa.nrows_out = npad; pa.ncols_out = npad; pa.gr = ms0.gr; pa.nu_fixed = ms0.nu_fixed;
        launch_pair_sym(ms0.mode, false, pa, s);
        // Sigma_uu  (rows/cols [npad, N))
        memset(&pa, 0, sizeof pa);
        pa.n = m; pa.m = m; pa.rows = dlocu; pa.cols = dlocu; pa.stride = mpad; pa.stride_rows = mpad;
        pa.out = dJ + (size_t)npad + (size_t)npad * ldj; pa.ld = ldj; pa.nrows_out = mpad; pa.ncols_out = mpad;
        pa.gr = ms0.gr; pa.nu_fixed = ms0.nu_fixed;
        launch_pair_sym(ms0.mode, false, pa, s);
        // cross block (rows [npad, N) x cols [0, npad)): observed side needs the pred-branch smoothness
        if (ms0.smooth_kind != msp.smooth_kind)
            launch_loc_params(loc_args(n, p, f->dX, f->dlocs, f->dloc, npad, tv, msp.smooth_kind, f->smooth_limits), s);
        memset(&pa, 0, sizeof pa);
        pa.n = n; pa.m = m; pa.rows = dlocp; pa.stride_rows = mpad; pa.cols = f->dloc; pa.stride = npad;
        pa.out = dJ + npad; pa.ld = ldj; pa.nrows_out = mpad; pa.ncols_out = npad; pa.gr = msp.gr;
        launch_pair_rect(MODE_GEOM, pa, s);
        // border row N: residual of realization z_col over the observed columns, zero elsewhere
        residual_row(f, mean, z_col, dJ, ldj, N, TILE - 1, N);
        FactorView v;
        v.A = dJ; v.lda = ldj; v.nt = N / TILE; v.mt = N / TILE + 1;
        if (int rc = factorize(f, v, nullptr)) return rc;
        // kriging mean: stochastic_i = sum_{c<n} J(npad+i, c) J(N, c);  tmp_mu = X_pred mean + stochastic
        launch_row_reduce(dJ, ldj, n, N, npad, m, dst, dq, dred, s);
        HIPCHK_AT("cocons_sim_cond_dense", hipMemcpyAsync(stv.data(), dst, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK_AT("cocons_sim_cond_dense", hipStreamSynchronize(s));
        add_trend_to(mu.data(), X_pred, m, p, mean, stv.data());
        HIPCHK_AT("cocons_sim_cond_dense", upload_canon(dmu, mu.data(), (size_t)m, s));
        // fields = L_S E + tmp_mu with L_S = lower-right block of the joint factor
        launch_trmm_lower(dJ + (size_t)npad + (size_t)npad * ldj, ldj, m, dE, m, nsim, dmu, dY, m, s);
        HIPCHK_AT("cocons_sim_cond_dense", hipMemcpyAsync(out, dY, (size_t)m * nsim * sizeof(double), hipMemcpyDeviceToHost, s));
        return 0;
    });
    return st > n ? n : st;    // a failure inside the Schur block is still "Cholesky error"
}

// ---------------------------------------------------------------------------
extern "C" int cocons_chol_solve(int n, const double *Ain, int nrhs, const double *rhs,
                                 double *L, double *Y, double *logdet_half)
{
    if (n <= 0 || !Ain || nrhs < 0 || (nrhs > 0 && !rhs)) return fail(-1, "cocons_chol_solve: bad argument");
    // reuse the fit machinery with a dummy 1-column design
    std::vector<double> locs((size_t)2 * n, 0.0), X((size_t)n, 1.0);
    double sl[2] = {0.5, 0.5};
    std::unique_ptr<cocons_fit, void (*)(cocons_fit *)> owner(
        fit_create_impl(n, 1, 0, 0, locs.data(), X.data(), nullptr, nullptr, sl, -1, false), cocons_fit_destroy);   // caller's order,
    cocons_fit *f = owner.get();                                                                                   // padding behind
    if (!f) return -1;
    f->engine_ok = false;     // one-shot handle whose input is uploaded once: plain schedule
    if (int rc = fit_alloc_matrix(f, nrhs > 0 ? nrhs : 1)) return rc;
    // identity everywhere in the padded square, zero rhs rows, then copy A and rhs^T in
    std::vector<double> hostA(f->lda * (size_t)f->npad, 0.0);
    for (int c = 0; c < f->npad; ++c) hostA[(size_t)c + (size_t)c * f->lda] = 1.0;
    for (int c = 0; c < n; ++c) {
        for (int r_ = c; r_ < n; ++r_) hostA[(size_t)r_ + (size_t)c * f->lda] = Ain[(size_t)r_ + (size_t)c * n];
        for (int k = 0; k < nrhs; ++k) hostA[(size_t)(f->npad + k) + (size_t)c * f->lda] = rhs[(size_t)c + (size_t)k * n];
    }
    StreamDrain s{f->stream, false};
    hipError_t e = upload_canon(f->dA, hostA.data(), hostA.size(), s);
    if (e != hipSuccess) return fail(-100, "cocons_chol_solve: %s", hipGetErrorString(e));
    if (int rc = reset_info(f)) return rc;
    if (int rc = factorize(f, main_view(f), nullptr)) return rc;
    launch_finalize(f->dA, f->lda, n, f->npad, 0, f->dout, s);
    e = hipMemcpyAsync(hostA.data(), f->dA, hostA.size() * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(f->hout, f->dout, sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(f->hinfo, f->dinfo, 2 * sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(-100, "cocons_chol_solve: %s", hipGetErrorString(e));
    if (int rc = info_status(f)) return rc;
    if (logdet_half) *logdet_half = f->hout[0];
    if (L)
        for (int c = 0; c < n; ++c)
            for (int r_ = 0; r_ < n; ++r_)
                L[(size_t)r_ + (size_t)c * n] = (r_ >= c) ? hostA[(size_t)r_ + (size_t)c * f->lda] : 0.0;
    if (Y)
        for (int k = 0; k < nrhs; ++k)
            for (int c = 0; c < n; ++c) Y[(size_t)c + (size_t)k * n] = hostA[(size_t)(f->npad + k) + (size_t)c * f->lda];
    return 0;
}
