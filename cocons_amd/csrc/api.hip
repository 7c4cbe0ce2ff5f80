// api.hip -- C ABI of the dense hot path (see include/cocons_hip.h for the contract and the reference interface each entry
// point replaces).  This file is the path of ONE objective evaluation on an unsharded handle, and nothing on that path crosses
// a translation unit: errors, theta -> kernel arguments, the assembly, the schedule switches and the factorisation, and the
// dense, batch, Profile and REML entries.  The handle's life is api_handle.hip's, the entries that never factor api_cov.hip's,
// the diagnostics api_diag.hip's; api_shard.hip, api_predict.hip, api_grad.hip and api_cv.hip hold the entries built on top
// (fit.hpp).
#include "fit.hpp"

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char *cocons_last_error(void) { return g_err.c_str(); }
extern "C" int cocons_abi_version(void) { return 1; }

// ---------------------------------------------------------------------------
// theta -> kernel arguments, exactly the host-side preamble of the reference functions

// Host-to-device copy of caller or host-computed doubles through canon_nan.  The normal case is the plain copy; only when an
// all-ones NaN is present is a canonical host copy staged, and the stream drained before that copy goes out of scope.
hipError_t upload_canon(double *dst, const double *src, size_t count, hipStream_t s)
{
    size_t first = 0;
    for (unsigned long long b; first < count; ++first) {
        memcpy(&b, src + first, sizeof b);
        if (b == ~0ull) break;
    }
    if (first == count) return hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyHostToDevice, s);
    std::vector<double> stage(src, src + count);
    for (size_t i = first; i < count; ++i) stage[i] = canon_nan(stage[i]);
    hipError_t e = hipMemcpyAsync(dst, stage.data(), count * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

// full_scale: the taper entries' FULL scale vector in two_scale_je (cocons_taper.cpp:207), the first scale included
void make_theta_vecs(const double *theta_in, int p, ThetaVecs &tv, bool full_scale)
{
    double theta[6 * COCONS_P_MAX];
    for (int i = 0; i < 6 * p; ++i) theta[i] = canon_nan(theta_in[i]);
    memset(&tv, 0, sizeof tv);
    for (int i = 0; i < p; ++i) {
        double sje = (i == 0) ? 0.0 : theta[TH_SCALE * p + i];      // cocons_full.cpp:49,64
        tv.tilt[i] = theta[TH_TILT * p + i];
        tv.two_scale_je[i] = 2 * (full_scale ? theta[TH_SCALE * p + i] : sje);      // :101
        tv.aniso[i] = theta[TH_ANISO * p + i];
        tv.sqrt_vector[i] = 2 * sje + theta[TH_ANISO * p + i];      // :66
        tv.half_sd[i] = 0.5 * theta[TH_SD * p + i];                 // :104
        tv.nugget[i] = theta[TH_NUGGET * p + i];
        tv.smooth[i] = theta[TH_SMOOTH * p + i];
        tv.sd[i] = theta[TH_SD * p + i];
    }
}

// which = 0 cov_rns, 1 cov_rns_classic, 2 cov_rns_pred
ModeSel select_mode(const double *theta, int p, const double *smooth_limits, int which)
{
    ModeSel m;
    m.gr = canon_nan(1 / std::exp(-2 * theta[TH_SCALE * p + 0]));   // :62, :351, :501
    m.nu_fixed = 0.0;
    if (which == 1) { m.mode = MODE_MEAN; m.smooth_kind = SMOOTH_EXP; return m; }
    if (which == 2) { m.mode = MODE_GEOM; m.smooth_kind = SMOOTH_LOGISTIC_SQRT; return m; }
    bool fix = true;                                                // allzeroelements, types.h:56-63
    for (int i = 1; i < p; ++i)
        if (theta[TH_SMOOTH * p + i] != 0) fix = false;
    if (fix && smooth_limits[0] == smooth_limits[1]) {              // :85-88
        double v = smooth_limits[0];
        m.nu_fixed = v;
        m.smooth_kind = SMOOTH_ZERO;
        if (std::fabs(v - 0.5) < 1e-6) m.mode = MODE_HALF;          // types.h:65-70
        else if (std::fabs(v - 1.5) < 1e-6) m.mode = MODE_THREEHALF;
        else if (std::fabs(v - 2.5) < 1e-6) m.mode = MODE_FIVEHALF;
        else m.mode = MODE_GEOM;   // quirk: zero smooth vector -> u = 0 -> every entry = diag_ii
    } else {
        m.mode = MODE_GEOM;
        m.smooth_kind = SMOOTH_LOGISTIC_SQRT;
    }
    return m;
}

// loc_params arguments of n locations: X (n x p) and locs (n x 2) column-major with leading dimension n, the SoA to out
LocArgs loc_args(int n, int p, const double *X, const double *locs, double *out, size_t stride, const ThetaVecs &tv,
                 int smooth_kind, const double *smooth_limits)
{
    LocArgs la;
    la.n = n; la.p = p;
    la.X = X; la.ldx = n;
    la.locs = locs; la.ldl = n;
    la.out = out; la.stride = stride;
    la.smooth_kind = smooth_kind;
    la.smooth_min = smooth_limits[0]; la.smooth_max = smooth_limits[1];
    la.th = tv;
    return la;
}

int fit_check(cocons_fit *f)
{
    if (!f) return fail(-1, "null fit handle");
    if (f->pid != getpid())
        return fail(-2, "fit handle was created in another process (fork); create it in the worker");
    hipError_t e = hipSetDevice(f->device);
    if (e != hipSuccess) return fail(-3, "hipSetDevice: %s", hipGetErrorString(e));
    return 0;
}

// rows under the matrix that an operation with rhs_rows right-hand sides reserves: whole tiles
static int rhs_rows_cap(int rhs_rows) { return round_up(rhs_rows > 0 ? rhs_rows : 1, TILE); }

int fit_alloc_matrix(cocons_fit *f, int rhs_rows)
{
    int cap = rhs_rows_cap(rhs_rows);
    f->rhs_act = cap;        // a buffer grown by an earlier predict call must not slow later evaluations
    border_unknown(f);      // every user of the rows under the matrix comes through here
    if (f->dA && cap <= f->rhs_cap) return 0;
    f->rhs_cap = cap;
    f->lda = (size_t)(f->skew > 0 ? f->skew * TILE : f->npad) + cap;
    // (exactly lda * npad: a buffer that a gradient call had grown goes back to the objective's size with the new shape)
    HIPCHK(f->dA.reserve(f->lda * (size_t)f->npad, f->stream, f->stream2, -1, true));
    // never-written parts must not hold NaN bit patterns: a band-limited factorisation only clears its envelope, and
    // 0 * garbage must stay 0 whatever the allocator hands back (every time the buffer takes a new shape)
    HIPCHK(hipMemsetAsync(f->dA, 0, f->lda * (size_t)f->npad * sizeof(double), f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
    return 0;
}

// ---------------------------------------------------------------------------
// assembly of Sigma (+ identity padding) into the factorisation buffer, lower triangle.
// bj0 / ncols restrict the 64-wide tile columns (sharded path); full range otherwise.
void assemble_sigma(cocons_fit *f, const double *theta, int which, int col0, int col1)
{
    ThetaVecs tv;
    make_theta_vecs(theta, f->p, tv);
    ModeSel ms = select_mode(theta, f->p, f->smooth_limits, which);
    launch_loc_params(loc_args(f->n, f->p, f->dX, f->dlocs, f->dloc, f->npad, tv, ms.smooth_kind, f->smooth_limits), f->stream);
    PairArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.n = f->n; pa.m = f->n;
    pa.rows = f->dloc; pa.cols = f->dloc;
    pa.stride = f->npad; pa.stride_rows = f->npad;
    pa.out = f->dA; pa.ld = f->lda;
    pa.nrows_out = f->npad; pa.ncols_out = col1;
    pa.bj0 = col0 / 64;
    if (pa.bj0 < f->pad0 / 64) pa.bj0 = f->pad0 / 64;      // 64-wide tile rows / columns that are placeholders only: not assembled
    pa.pad_diag = f->nslot > 0 ? 1e300 : 1.0;               // slot columns: a diagonal no right-hand side can turn negative
    pa.gr = ms.gr; pa.nu_fixed = ms.nu_fixed;
    launch_pair_sym(ms.mode, false, pa, f->stream);
}

// Taper fit: Sigma_tap = taper o cov_rns_taper(theta) (R/neg2loglikelihood.R:25-31) as a dense lower triangle.
// Parameters exactly as cocons_cov_rns_taper prepares them (FULL scale vector, src/cocons_taper.cpp:207).
int assemble_sigma_taper(cocons_fit *f, const double *theta)
{
    ThetaVecs tv;
    make_theta_vecs(theta, f->p, tv, true);
    ModeSel ms = select_mode(theta, f->p, f->smooth_limits, 0);
    launch_loc_params(loc_args(f->n, f->p, f->dX, f->dlocs, f->dloc, f->npad, tv, ms.smooth_kind, f->smooth_limits), f->stream);
    // zero what the factorisation will read: the tiles inside the envelope (the rows under the matrix are written in
    // full by the right-hand-side kernel), or the whole buffer when the factorisation is not band-limited
    if (f->d_thi) launch_band_zero(f->dA, f->lda, f->d_thi, f->nt, f->taper_maxband, f->stream, f->skew);
    else HIPCHK(hipMemsetAsync(f->dA, 0, f->lda * (size_t)f->npad * sizeof(double), f->stream));
    TaperLaunch t;
    t.mode = ms.mode; t.nrows = f->n; t.nnz = f->taper_nnz; t.ci = f->d_tci; t.rp = f->d_trp; t.nu_fixed = ms.nu_fixed;
    t.rows = t.cols = f->dloc; t.stride_rows = t.stride = f->npad;
    t.tapv = f->d_tval; t.A = f->dA; t.lda = f->lda; t.skew = f->skew; t.npad = f->npad;
    launch_taper(t, f->stream);
    launch_pad_identity(f->dA, f->lda, f->n, f->npad, f->stream, f->skew);
    return 0;
}

int no_taper(cocons_fit *f, const char *who)
{
    if (f->taper_nnz > 0) return fail(-1, "%s: not available on a taper fit (cocons_neg2loglik_dense is)", who);
    return 0;
}

// right-hand-side rows under the matrix: rows npad.. : z columns (minus trend), then xb columns
void assemble_rhs(cocons_fit *f, const double *mean, bool use_trend, const double *xb, int nxb,
                  int col0, int col1, bool zero_rest, bool slots)
{
    if (slots) { zero_rest = false; col1 = f->n; }      // (the assembly zeroed the slot rows; their own columns are not touched)
    RhsArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.n = f->n; ra.p = f->p; ra.X = f->dX; ra.ldx = f->n;
    ra.use_trend = use_trend ? 1 : 0;
    if (use_trend) for (int i = 0; i < f->p; ++i) ra.mean[i] = canon_nan(mean[i]);
    ra.src = f->dz; ra.lds = f->n;
    ra.out = f->dA; ra.ld = f->lda;
    ra.skew = f->skew; ra.npad = f->npad;
    ra.row0 = slots ? f->n : f->npad; ra.nrows = f->r;
    ra.nrows_zero = (nxb > 0 || !zero_rest) ? 0 : f->rhs_act - f->r;
    ra.col0 = col0; ra.ncols_out = col1;
    launch_rhs_rows(ra, f->stream);
    if (nxb > 0) {
        ra.use_trend = 0;
        ra.src = xb; ra.lds = f->n;
        ra.row0 = (slots ? f->n : f->npad) + f->r; ra.nrows = nxb;
        ra.nrows_zero = zero_rest ? f->rhs_act - f->r - nxb : 0;
        launch_rhs_rows(ra, f->stream);
    }
}

// Bordered right-looking factorisation, outer block = 2 tiles (256 columns).
//   panel(k)  : potrf(k) | trsm(k) | update tile column k+1 (K=128) | potrf(k+1) | trsm(k+1)
//   U1(k)     : update of the NEXT block's two tile columns with panel k (K = 256)
//   U2(k)     : update of everything right of that
// Look-ahead: panel(k+2) runs on a second stream as soon as U1(k) is done, concurrently
// with U2(k) on the main stream; U1(k+2) waits for it.  mt = total tile rows (matrix + rhs
// rows).  Optional per-launch timing of U2 via events (ev_upd): appended (start, stop).
FactorView main_view(cocons_fit *f)
{
    FactorView v;
    v.A = f->dA; v.lda = f->lda; v.nt = f->nt; v.mt = f->nt + f->rhs_act / TILE;
    v.hi = envelope_or_null(f);
    v.skew = f->skew;
    return v;
}

RhsLayout rhs_layout(const cocons_fit *f, int nrhs)
{
    RhsLayout l;
    l.slots = f->nslot >= nrhs && f->nslot > 0;
    const int act = rhs_rows_cap(nrhs);
    l.tile_rows = l.slots ? 0 : act / TILE;
    l.trim = (!l.slots && act - nrhs >= 64) ? 1 : 0;
    return l;
}

// the view of the matrix an evaluation with this layout factors (after fit_alloc_matrix(f, nrhs))
FactorView rhs_view(cocons_fit *f, const RhsLayout &l)
{
    FactorView v = main_view(f);
    v.mt = v.nt + l.tile_rows;
    v.trim = l.trim;
    return v;
}

// one past the last band row tile of the 256-column block starting at tile k (at least the next diagonal block, so
// that the update which the engine's hand-off hangs on always covers it); -1 = dense
static int band_hi(const FactorView &v, int k)
{
    if (!v.hi) return -1;
    int h = v.hi[k];
    if (k + 1 < v.nt && v.hi[k + 1] > h) h = v.hi[k + 1];
    const int need = k + 4 < v.nt ? k + 4 : v.nt;
    if (h < need) h = need;
    return h < v.nt ? h : v.nt;
}

// tile factorisation + the panel solve below it.  (ONE launch for the two -- the solve's workgroups fetch their rows, wait for
// a word the factorising workgroup raises, take L and solve -- was built and measured in round 5: SLOWER, taper path 4.18 -> 4.57
// ms, batch at n = 4096 1066 -> 1031 evaluations/s: the boundary between the two launches costs less than the write-through
// factor and the serialised fetch of L behind the word; removed.)
// (Round 5, later: ONE launch after all -- not behind a word but FOLLOWING the factorisation through the tile's mailbox, the way the
// engine's partner does: potrf_follow_kernel.  The mailboxes are filled by mbox_reset at the start of the factorisation.)
static void potrf_solve(cocons_fit *f, double *A, size_t lda, int tile, const RowRange &rows, double *q, hipStream_t s)
{
    TrsmLaunch l;
    l.A = A; l.lda = lda; l.c0 = tile * TILE; l.rows = rows; l.dinv = q;
    if (tun().potrf_follow != 0 && !f->follow_off && tile_mbox(f, f->nt + 1) && (l.mbox = tile_mbox(f, tile)) != nullptr) {
        f->follow_used = true;
        l.info = f->dinfo; l.abort_word = handoff_words(f).abort;
        launch_potrf_follow(l, s);
        return;
    }
    launch_potrf_tile(A, lda, tile * TILE, q, f->dinfo, s);
    launch_trsm_tile(l, s);
}

void panel_ops(cocons_fit *f, const FactorView &v, int k, hipStream_t s)
{
    double *q0 = f->dinv, *q1 = f->dinv + 8 * 256;
    const int hb = band_hi(v, k);                       // rows [.., hb) of the band, then the rows under the matrix [nt, mt)
    potrf_solve(f, v.A, v.lda, k, v.panel_rows(k + 1, hb), q0, s);
    if (k + 1 < v.nt) {
        UpdateLaunch u = v.update(hb);
        u.panel_in_c(k * TILE); u.K = TILE; u.ti0 = k + 1; u.ti1 = v.mt; u.tj0 = k + 1; u.tj1 = k + 2; u.lower_only = true;
        launch_update(u, s);
        potrf_solve(f, v.A, v.lda, k + 1, v.panel_rows(k + 2, hb), q1, s);
    }
}

// The table of the switches above: tune name (cocons_debug_tune), environment variable (read once, at the first use; nullptr:
// tests and tools only) and the least value the switch takes (a smaller one is raised to it)
struct TuneRow { const char *name, *env; int Tunables::*field; int lo; };
static const TuneRow tune_rows[] = {
    {"engine", "COCONS_ENGINE", &Tunables::engine, INT_MIN},
    {"dag", "COCONS_DAG", &Tunables::dag, INT_MIN},
    {"dag_lead", "COCONS_DAG_LEAD", &Tunables::dag_lead, INT_MIN},
    {"dag_lead2", "COCONS_DAG_LEAD2", &Tunables::dag_lead2, INT_MIN},
    {"dag_lead3", "COCONS_DAG_LEAD3", &Tunables::dag_lead3, INT_MIN},
    {"dag_min_tiles", "COCONS_DAG_MIN_TILES", &Tunables::dag_min_tiles, INT_MIN},
    {"dag_xcc_quota", "COCONS_DAG_XCC_QUOTA", &Tunables::dag_xcc_quota, INT_MIN},
    {"dag_xcd", "COCONS_DAG_XCD", &Tunables::dag_xcd, INT_MIN},
    {"dag_order", "COCONS_DAG_ORDER", &Tunables::dag_order, INT_MIN},
    {"dag_xcd_min_quota", nullptr, &Tunables::dag_xcd_min_quota, INT_MIN},
    {"dag_bw", "COCONS_DAG_BW", &Tunables::dag_bw, 1},        // (0 would make dag_build_far_table loop forever)
    {"dag_bh", "COCONS_DAG_BH", &Tunables::dag_bh, 1},
    {"dag_trace", nullptr, &Tunables::dag_trace, INT_MIN},
    {"engine_pair", "COCONS_ENGINE_PAIR", &Tunables::engine_pair, INT_MIN},
    {"panel_fused", "COCONS_PANEL_FUSED", &Tunables::panel_fused, INT_MIN},
    {"potrf_follow", "COCONS_POTRF_FOLLOW", &Tunables::potrf_follow, INT_MIN},
    {"panel_split", "COCONS_PANEL_SPLIT", &Tunables::panel_split, INT_MIN},
    {"gate_sabotage", nullptr, &Tunables::gate_sabotage, INT_MIN},
    {"host_delay_us", "COCONS_DEBUG_HOST_DELAY_US", &Tunables::host_delay_us, INT_MIN},
    {"host_delay_tile", "COCONS_DEBUG_HOST_DELAY_TILE", &Tunables::host_delay_tile, INT_MIN},
    {"engine_in_wait_ms", nullptr, &Tunables::engine_in_wait_ms, INT_MIN},
};
static void tune_set(Tunables &t, const TuneRow &r, int value) { t.*r.field = value < r.lo ? r.lo : value; }

Tunables &tun()
{
    static Tunables t;
    if (!t.init) {
        for (const TuneRow &r : tune_rows)
            if (const char *e = r.env ? getenv(r.env) : nullptr) tune_set(t, r, atoi(e));
        t.init = true;
    }
    return t;
}

extern "C" int cocons_debug_tune(const char *name, int value)
{
    if (!name) return fail(-1, "cocons_debug_tune: null name");
    Tunables &t = tun();
    std::string k(name);
    for (const TuneRow &r : tune_rows)
        if (k == r.name) { tune_set(t, r, value); return 0; }
    if (k == "upd_waves") set_update_waves(value);
    else if (k == "w8_max_tiles") set_update_w8_max_tiles(value);
    else if (k == "c_wt") set_update_c_wt(value);
    else return fail(-1, "cocons_debug_tune: unknown switch %s", name);
    return 0;
}

// Workgroups of the persistent launch that may take part on the XCD that also hosts the engine.
// Measured there: an XCD that runs kernels of two queues does not hold eight of these workgroups on every CU -- 227 instead of
// 248 beside the engine's CU: seven on most, eight on some -- and the set that fits changes when the driver's save / restore
// moves the engine.  The quota keeps the launch below what fits in ANY placement: seven per CU on the XCD's other CUs, less
// one CU's worth and one: (CUs per XCD - 1) x 7 - 9 = 208 for the 32 CUs per XCD of MI355X (the value of round 4's soak runs:
// 0 time-outs in 40 000 evaluations), from hipDeviceProp instead of a constant; COCONS_DAG_XCC_QUOTA overrides.
static int dag_xcc_quota()
{
    if (tun().dag_xcc_quota >= 0) return tun().dag_xcc_quota;
    static int derived = -1;
    if (derived < 0) {
        const int cus = device_cus();
        const int xcds = 8;                                 // gfx950: eight accelerator dies (no HIP attribute reports it)
        const int cpx = cus % xcds == 0 ? cus / xcds : 32;
        derived = (cpx - 1) * 7 - 9;
        if (derived < 8) derived = 8;
    }
    return derived;
}

// Chunk exponent of the XCD-aware deal of the persistent launch's task list (chol.hip: dag_position; 0 = one counter for all).
// The deal assumes the eight XCDs of the whole chip -- a partitioned device keeps the one counter -- and XCDs that contribute
// comparable numbers of workgroups: a class of list positions whose XCD holds almost none is carried by the others only while
// they are free to draw, and with everybody waiting at that class's tasks the launch crawls at the pace of its few workgroups
// until a bounded wait ends it (tools/diag/quota_stress.py) -- a quota below dag_xcd_min_quota (half an XCD's share), which
// only the tests set, keeps the one counter too.
static int dag_xcd_group()
{
    const int q = dag_xcc_quota();
    return (tun().dag_xcd && device_cus() == 256 && (q == 0 || q >= tun().dag_xcd_min_quota)) ? 5 : 0;
}

// COCONS_ENGINE: 1 (default) = diagonal tiles are factored by the resident engine while the trailing
// update runs; 0 = every kernel in order on one stream
bool engine_enabled() { return tun().engine != 0; }

// one trailing-update launch (tile columns [t0, t1) of the trapezoid below (t0, t0)), optionally
// bracketed by timing events (profile runs): appended as (start, stop)
static void timed_update(cocons_fit *f, const FactorView &v, int k, int kw, int t0, int t1, hipStream_t s,
                         std::vector<hipEvent_t> *ev_upd, unsigned *sig, int sig_tile, unsigned *queue = nullptr,
                         int skip_tiles = 0)      // > 0: the diagonal block at t0 (that many tiles) was updated by the panel's launch
{
    const int mt = v.mt;
    if (t1 <= t0) return;
    const int hb = band_hi(v, k);                       // band-limited: tile columns and rows [t0, hb), plus the rows [nt, mt)
    if (hb >= 0 && hb < t1) t1 = hb;
    if (t1 <= t0) return;
    hipEvent_t a = nullptr, b = nullptr;
    if (ev_upd) {
        hipEventCreate(&a); hipEventCreate(&b);
        hipEventRecord(a, s);
    }
    // the first panel's leading columns are the unit vectors of the front padding (zero below the diagonal): they add
    // nothing to the trailing matrix, so the update starts behind them (whole 16-column chunks; bit-identical)
    const int kskip = (k == 0 && !v.hi) ? (f->pad0 / 16) * 16 : 0;
    UpdateLaunch u = v.update(hb);
    u.panel_in_c(k * TILE + kskip); u.K = kw * TILE - kskip; u.ti0 = t0; u.ti1 = mt; u.tj0 = t0; u.tj1 = t1; u.lower_only = true;
    u.sig = sig; u.sig_tile = sig_tile; u.queue = queue; u.abort_word = sig ? handoff_words(f).abort : nullptr;   // engine schedule: see update_kernel
    if (skip_tiles > 0) { u.skip_lo = 2 * t0; u.skip_hi = 2 * (t0 + skip_tiles); }
    launch_update(u, s);
    if (ev_upd) {
        hipEventRecord(b, s);
        ev_upd->push_back(a); ev_upd->push_back(b);
    }
}

// algorithmic flops of the trailing update of block k (tile columns [t0, nt)): lower triangle of the
// trailing block of order m (real columns only) times K, plus the rhs rows:  K m (m+1) + 2 K r m
void count_update_flops(cocons_fit *f, int kw, int t0)
{
    double m = (double)f->n_user - ((double)t0 * TILE - (double)f->pad0);      // the caller's rows and columns from t0 on
    if (m > (double)f->n_user) m = (double)f->n_user;
    if (m < 0) m = 0;
    const double K = (double)kw * TILE - (t0 == kw ? (double)f->pad0 : 0.0);     // the first panel holds pad0 placeholder columns
    f->upd_flops += K * m * (m + 1.0) + 2.0 * K * (double)f->nrhs_cur * m;
}

// Reset the hand-off words and launch the diagonal-block engine (see factorize) for a factorisation of view
// v on the second stream, ordered behind the reset.  The engine's 8 waves take every VGPR of a CU, so it can
// only be placed on an EMPTY one: enqueue_eval calls this between the covariance assembly and the short
// right-hand-side kernel, and factorize holds the main stream behind a one-lane gate kernel until the engine
// reports itself resident.
// (Launched between the assembly and the first trailing update it could lose that race and then wait for
// a whole update to drain; with workgroups that wait for the engine on every CU it would never be placed.)
static bool engine_wanted(cocons_fit *f, const FactorView &v)
{
    return engine_enabled() && f->engine_ok && f->stream2 != nullptr && f->engine_skip == 0 && v.nt > 4;
}

// the hand-off words and tile counters of one factorisation with nt tiles, zeroed on the main stream
int flags_reset(cocons_fit *f, int nt)
{
    if (f->flags_cap < nt) {
        const int cap = round_up(nt + 8, 64);
        HIPCHK(f->dflags.reserve(handoff_word_count(cap), f->stream, f->stream2));
        f->flags_cap = cap;
    }
    HIPCHK(hipMemsetAsync(f->dflags, 0, handoff_word_count(f->flags_cap) * sizeof(unsigned), f->stream));
    return 0;
}

// the tiles' mailboxes (the engine's pair mode, the panel kernel, potrf_solve's followers) filled with the pattern that means "not
// written yet" (every byte 0xff; potrf_tile_body: mbox) on the main stream: 88 KB each, 7.1 MB at n = 10^4
int mbox_reset(cocons_fit *f, int nt, bool engine_schedule)
{
    // one allocation, one fill: the tiles' mailboxes | the strip mailboxes (0.5 MB per diagonal block) | the exchange mailboxes of
    // the split panel (64 KB per 64-row strip); the one-launch panel follows the pair's tiles
    const MboxLayout l = mbox_layout(nt, tun().panel_fused && tun().engine_pair, tun().panel_split != 0);
    HIPCHK(f->dmbox.reserve(l.total(), f->stream, f->stream2));
    f->mbox = l;
    // (the plain schedule uses the tiles' mailboxes only)
    HIPCHK(hipMemsetAsync(f->dmbox, 0xff, (engine_schedule ? l.total() : l.tiles) * sizeof(double), f->stream));
    return 0;
}

// ---- the dependency-driven schedule (chol.hip: dag_kernel) ---------------------------------------------------------
static bool dag_wanted(cocons_fit *f, const FactorView &v)
{
    return tun().dag != 0 && v.dag_ok && !v.hi && !v.skew && v.nt > 4 && f->world == 1;
}

// buffers, zeroed task words and the step table of the factorisation of view v (on the main stream, before the engine starts)
int dag_prepare(cocons_fit *f, const FactorView &v)
{
    const size_t elems = v.lda * (size_t)f->npad;
    HIPCHK(f->dP.reserve(elems, f->stream, f->stream2, 0, true));       // (the shape of the view exactly; zeroed when new)
    if (!f->dpart) HIPCHK(f->dpart.alloc((size_t)2 * 16 * 64 * 64));
    HIPCHK(f->dWt.reserve((size_t)v.nt * TILE * TILE, f->stream, f->stream2, 0));   // zero above the diagonals, for good
    const int kskip = (f->pad0 / 16) * 16;
    const int xcd_g = dag_xcd_group();
    const int key[12] = {v.nt, v.mt, v.trim, kskip, tun().dag_lead, tun().dag_min_tiles, tun().dag_lead2, tun().dag_lead3,
                         tun().dag_order, xcd_g, tun().dag_bw, tun().dag_bh};
    if (memcmp(key, f->dag_key, sizeof key) != 0 || !f->ddag_steps) {
        std::vector<DagStepHost> steps;
        std::vector<unsigned> ftab;
        const bool want_tab = tun().dag_order != 0 || xcd_g > 0;
        const unsigned ntasks = dag_build_steps(v.nt, v.mt, v.trim, kskip, tun().dag_lead, tun().dag_min_tiles, steps,
                                                tun().dag_lead2, tun().dag_lead3, want_tab ? &ftab : nullptr, xcd_g,
                                                tun().dag_order ? tun().dag_bw : 0, tun().dag_bh);
        HIPCHK(hipStreamSynchronize(f->stream));      // (the table in place may be in use, whether or not a buffer below grows)
        if (f->stream2) HIPCHK(hipStreamSynchronize(f->stream2));
        HIPCHK(f->ddag_steps.reserve(steps.size() + 1, f->stream, f->stream2, -1, true));
        // (on the handle's own stream: the library never touches the NULL stream -- a synchronous hipMemcpy here gave it a
        // hardware queue of its own and shifted every later stream's assignment)
        HIPCHK(hipMemcpyAsync(f->ddag_steps, steps.data(), steps.size() * sizeof(DagStepHost), hipMemcpyHostToDevice, f->stream));
        HIPCHK(f->ddag_ftab.reserve(ftab.size(), f->stream, f->stream2));
        if (!ftab.empty())
            HIPCHK(hipMemcpyAsync(f->ddag_ftab, ftab.data(), ftab.size() * sizeof(unsigned), hipMemcpyHostToDevice, f->stream));
        f->dag_xcd_g = want_tab ? xcd_g : 0;
        f->dag_have_ftab = want_tab && !ftab.empty();
        HIPCHK(hipStreamSynchronize(f->stream));
        f->dag_nsteps = (int)steps.size(); f->dag_ntasks = ntasks;
        memcpy(f->dag_key, key, sizeof key);
        HIPCHK(f->ddag.reserve(dag_words(f, v.mt).total, f->stream, f->stream2));
    }
    HIPCHK(hipMemsetAsync(f->ddag, 0, f->ddag.count() * sizeof(unsigned), f->stream));
    // trace buffer: 4 stamps + one word of hw_where() pairs per task, 8 stamps per tile pair of the engine -- sized by BOTH
    // the task count and the tile count of THIS step table (a later table with fewer tasks and more tiles must not run past it)
    const size_t trace_elems = dag_trace_words(f, v.nt).count;
    if (tun().dag_trace) HIPCHK(f->ddag_trace.reserve(trace_elems, f->stream, f->stream2));
    f->dag_trace_tasks = (tun().dag_trace && f->ddag_trace) ? f->dag_ntasks : 0;      // 0: the buffer does not describe this table
    if (f->dag_trace_tasks)
        HIPCHK(hipMemsetAsync(f->ddag_trace, 0, trace_elems * sizeof(unsigned long long), f->stream));
    return 0;
}

// the persistent launch of view v on the handle's step table, task words and the hand-off words hw (no trace)
DagLaunch dag_launch(cocons_fit *f, const FactorView &v, const HandoffWords &hw, const unsigned *alive)
{
    const DagWords w = dag_words(f, v.mt);
    DagLaunch d;
    d.A = v.A; d.lda = v.lda; d.P = f->dP; d.Wt = f->dWt; d.steps = f->ddag_steps; d.nsteps = f->dag_nsteps; d.ntasks = f->dag_ntasks;
    d.queue = w.queue; d.tdone = w.tdone; d.pdone = w.pdone; d.pstride = w.pstride; d.pall = w.pall; d.dcount = w.dcount; d.xcnt = w.xcnt;
    d.partbuf = f->dpart; d.sig = hw.in; d.out = hw.out; d.xr = hw.xr; d.abort_word = hw.abort;
    d.alive = alive; d.xcc_quota = dag_xcc_quota(); d.xcd_g = f->dag_xcd_g;
    if (f->dag_have_ftab) d.ftab = f->ddag_ftab;
    return d;
}

static int engine_start(cocons_fit *f, const FactorView &v)
{
    if (f->engine_live) return 0;
    const int nt = v.nt;
    hipStream_t M = f->stream;
    if (int rc = flags_reset(f, nt)) return rc;
    f->dag_next = dag_wanted(f, v);
    if (f->dag_next) {
        if (int rc = dag_prepare(f, v)) return rc;
        if (f->dag_nsteps < 2) f->dag_next = false;          // too small a problem for a head worth the launch: classic throughout
    }
    f->engine_pair_live = tun().engine_pair != 0 ? 1 : 0;
    if (f->engine_pair_live || (tun().potrf_follow && !f->follow_off))
        if (int rc = mbox_reset(f, nt > f->nt ? nt : f->nt)) return rc;
    HIPCHK(hipEventRecord(f->ev_eng, M));                    // (behind the resets of the flag and task words, and of W / P when new)
    HIPCHK(hipStreamWaitEvent(f->stream2, f->ev_eng, 0));
    // (from tile 0: the engine factors the first diagonal block too, its input words raised by the gate kernel -- band-limited
    // views, whose first block is not the engine's, never get the engine: fit_create_taper)
    const HandoffWords hw = handoff_words(f);
    EngineLaunch e;
    e.A = v.A; e.lda = v.lda; e.nt = nt; e.dinv = f->dinv; e.info = f->dinfo; e.in_wait_ms = tun().engine_in_wait_ms;
    e.in = hw.in; e.out = hw.out; e.xr = hw.xr; e.abort_word = hw.abort; e.alive = hw.alive;
    if (f->dag_next) { e.wbuf = f->dWt; e.pbuf = f->dP; e.dag_until = 2 * f->dag_nsteps; }
    if (f->dag_next && f->dag_trace_tasks) e.trace = dag_trace_words(f, nt).engine;
    if (f->engine_pair_live) e.mbox = f->dmbox;
    launch_potrf_engine(e, f->stream2);
    f->engine_live = true;
    return 0;
}

// Bordered right-looking factorisation, outer block = 2 tiles (256 columns).
//
// Plain schedule (COCONS_ENGINE=0, or fewer than 5 tiles), everything on the main stream:
//   potrf(t) | trsm(t) | in-panel update of tile column t+1 | potrf(t+1) | trsm(t+1) | trailing update
//
// Engine schedule: the 256 x 256 diagonal blocks from tile 2 on are factored by ONE resident workgroup
// (potrf_engine_kernel, launched once per factorisation on the second stream, on a CU of its own) as
// soon as the trailing update has published them; the main stream runs, per block k with t = k + 2:
//   U(k)      : trailing update with panel k, tile column t first; its workgroups inside the diagonal
//               block raise in[t] / in[t+1]      -> the engine factors tile t, forms X = A(t+1,t) L(t)^-T,
//                                                   updates and factors tile t+1 (all while U(k) runs)
//   trsm(t)   : rows below the diagonal block; waits for out[t]
//   in-panel update of tile column t+1 (rows below the block) with column t; waits for xr[t]
//   trsm(t+1) : waits for out[t+1]
// So the serial part of every panel -- two 30 us single-workgroup factorisations and the tile between
// them -- is off the critical path as long as U(k) lasts ~90 us; the main stream needs no events and
// issues fewer launches than the plain schedule.
int factorize(cocons_fit *f, const FactorView &v, std::vector<hipEvent_t> *ev_upd)
{
    const int nt = v.nt, mt = v.mt;
    hipStream_t M = f->stream;
    // the placeholder observations in front (fit_create_impl): whatever the assembly kernels put into their columns --
    // covariances, right-hand sides, cross-covariance rows -- is replaced by unit vectors, in every view whose first
    // indices are the handle's observations
    launch_front_identity(v.A, v.lda, f->pad0, mt * TILE, M);
    f->follow_used = false;
    if (!engine_wanted(f, v)) {
        f->engine_used = false;
        f->dag_used = false;
        if (int rc = flags_reset(f, nt)) return rc;
        if (tun().potrf_follow && !f->follow_off)
            if (int rc = mbox_reset(f, nt > f->nt ? nt : f->nt, false)) return rc;
        if (v.hi) {
            // band-limited: one tile column per step (factor, solve, update with K = 128) -- inside a narrow envelope
            // the in-panel update of the two-tile block costs more than the second, cheaper trailing update
            // (4.71 -> 4.53 ms at n = 10^4)
            // (row bound = the column's OWN envelope hi[k] -- per 256-block, monotone, >= k + 1 --, not band_hi(): for an
            // odd k that is the NEXT block's bound, beyond what band_zero_kernel clears in column k)
            // (packed band buffer: the kernels that stay inside tile column k address it by global indices through a
            // shifted base, where the rows under the matrix start at row (k + skew) * 128 -- kernels.h band_base)
            for (int k = 0; k < nt; ++k) {
                const int hb = v.hi[k] < nt ? v.hi[k] : nt;
                double *q = f->dinv + (size_t)(k & 1) * 2048;
                double *Ak = band_base(v.A, k, v.skew);
                const int e0 = v.skew ? k + v.skew : nt, e1 = e0 + (mt - nt);      // tile rows under the matrix
                RowRange rows;
                rows.r0 = (k + 1) * TILE; rows.r1 = e1 * TILE - 64 * v.trim; rows.band_r1 = hb * TILE; rows.ext_r0 = e0 * TILE;
                potrf_solve(f, Ak, v.lda, k, rows, q, M);
                if (k + 1 < nt) {
                    UpdateLaunch u = v.update(hb);
                    u.panel_in_c(k * TILE); u.K = TILE; u.ti0 = k + 1; u.ti1 = mt; u.tj0 = k + 1; u.tj1 = hb < nt ? hb : nt; u.lower_only = true;
                    u.skew = v.skew;
                    launch_update(u, M);
                }
            }
            return 0;
        }
        for (int k = 0; k < nt; k += 2) {
            panel_ops(f, v, k, M);
            if (k + 2 < nt) {
                if (ev_upd) count_update_flops(f, 2, k + 2);
                timed_update(f, v, k, 2, k + 2, nt, M, ev_upd, nullptr, -1, handoff_words(f).tile_queue(k));
            }
        }
        return 0;
    }
    if (int rc = engine_start(f, v)) return rc;          // no-op when enqueue_eval started it before the assembly
    f->engine_live = false;
    f->engine_used = true;
    const HandoffWords hw = handoff_words(f);
    unsigned *const in = hw.in, *const out = hw.out, *const xr = hw.xr, *const abort_word = hw.abort;
    unsigned *alive = hw.alive;
    if (tun().gate_sabotage > 0) { --tun().gate_sabotage; alive += 1; }      // (tests: a word that stays zero)
    // (the engine factors the first diagonal block too: the gate raises its input words; the pair partner counts itself)
    launch_start_gate(alive, abort_word, f->engine_ops++ == 0, f->engine_pair_live,
                      (tun().gate_sabotage == 0 && alive == hw.alive) ? in : nullptr, M);
    // the panel of the block at tile t (behind the engine's factorisation of it): one launch whose strips follow the pair's tiles
    // through their mailboxes, or three launches that wait for the tiles; returns the tiles of the NEXT diagonal block that the
    // launch has updated (the update launch behind it then leaves them alone)
    auto panel_for = [&](int t, bool allow_diag) -> int {
        const bool two = t + 1 < nt;                 // the block has a second tile
        const int r0 = two ? t + 2 : t + 1;          // first tile row below the diagonal block
        const int hb = band_hi(v, t);                // rows of block t's panel: [r0, hb) and the rows under the matrix
        const RowRange rows = v.panel_rows(r0, hb);
        if (two && hb < 0 && tun().panel_fused && f->engine_pair_live && f->dmbox != nullptr) {
            // the next diagonal block (tiles t + 2, t + 3), when there is one, is updated inside this launch
            const int next_tiles = t + 2 < nt ? (t + 3 < nt ? 2 : 1) : 0;
            const int nstrips = (rows.r1 - rows.r0) / 64;
            PanelLaunch p;
            p.A = v.A; p.lda = v.lda; p.c0 = t * TILE; p.rows = rows; p.xr = xr + t; p.abort_word = abort_word;
            p.mb0 = tile_mbox(f, t); p.mb1 = tile_mbox(f, t + 1); p.sig = in; p.sig_tile = t + 2;
            if (allow_diag && next_tiles > 0) p.smb = strip_mbox(f, t >> 1);
            if (p.smb) p.ndiag = next_tiles == 2 ? 10 : 3;
            if (tun().panel_split > 0 && nstrips >= tun().panel_split) p.xmb = xchg_mbox(f, nstrips);
            launch_panel_pair(p, M);
            return (p.smb && nstrips >= (next_tiles == 2 ? 4 : 2)) ? next_tiles : 0;
        }
        TrsmLaunch l;
        l.A = v.A; l.lda = v.lda; l.c0 = t * TILE; l.rows = rows; l.dinv = f->dinv + (size_t)(t & 1) * 2048; l.wait_word = out + t; l.abort_word = abort_word;
        launch_trsm_tile(l, M);
        if (two) {
            UpdateLaunch u = v.update(hb);
            u.panel_in_c(t * TILE); u.K = TILE; u.ti0 = r0; u.ti1 = mt; u.tj0 = t + 1; u.tj1 = t + 2; u.wait_word = xr + t; u.abort_word = abort_word;
            launch_update(u, M);
            l.c0 = (t + 1) * TILE; l.dinv = f->dinv + (size_t)((t + 1) & 1) * 2048; l.wait_word = out + t + 1;
            launch_trsm_tile(l, M);
        }
        return 0;
    };
    // tiles of the diagonal block at t that the previous panel's launch has updated (the persistent launch updates its first
    // diagonal block itself)
    int diag_done = panel_for(0, !f->dag_next);
    f->dag_used = f->dag_next;
    int k_first = 0;                 // first block step the classic loop below runs in full
    if (f->dag_next) {
        // the head of the factorisation -- the steps whose update fills the chip several times over -- is ONE persistent
        // launch (dag_kernel): tiles of update k + 1 start as soon as the strips of panel k + 1 they need and their own tile of
        // update k are done, and the panels between them are tile tasks of the same launch (the engine publishes the tile
        // inverses they multiply with).  Behind the head a step is bound by its dependency chain, and there the classic
        // sequence below has the shorter one: it takes over with the panel behind the last DAG step.
        hipEvent_t ea = nullptr, eb = nullptr;
        if (ev_upd) {
            const double before = f->upd_flops;
            for (int s = 0; s < f->dag_nsteps; ++s) count_update_flops(f, 2, 2 * s + 2);
            f->dag_flops = f->upd_flops - before;
            hipEventCreate(&ea); hipEventCreate(&eb);
            hipEventRecord(ea, M);
        }
        DagLaunch d = dag_launch(f, v, hw, alive);
        if (f->dag_trace_tasks) { const DagTraceWords tw = dag_trace_words(f, nt); d.trace = tw.tasks; d.hw = tw.hw; }
        launch_dag(d, M);
        if (ev_upd) { hipEventRecord(eb, M); ev_upd->push_back(ea); ev_upd->push_back(eb); f->dag_events = 1; }
        k_first = 2 * f->dag_nsteps;
    }
    // (Running the panel kernels on a stream of their own behind near-tile flags, so that they start in the tail of the
    // update that feeds them, was built and measured in round 3: slower -- a 90 KB-LDS solve is not placed beside eight
    // update workgroups per CU, the event back to the main stream costs 12 us -- and removed; so were three forms of the
    // panel as products with explicit inverses published by the engine (round 3: +-1 %, deleted in round 4); DESIGN.md
    // section 8.)
    for (int k = k_first > 0 ? k_first - 2 : 0; k + 2 < nt; k += 2) {
        const int t = k + 2;
        // (tests: a late host -- whatever raises in[host_delay_tile], the panel launch of block t or the update launch behind it,
        // is enqueued host_delay_us late, while the engine has everything it needs to get there and wait)
        if (tun().host_delay_us > 0 && t + 2 == tun().host_delay_tile) usleep((useconds_t)tun().host_delay_us);
        if (k >= k_first) {                          // (the update with the last DAG step's panel was that launch's)
            if (ev_upd) count_update_flops(f, 2, t);
            timed_update(f, v, k, 2, t, nt, M, ev_upd, in, t, hw.tile_queue(k), diag_done);
        }
        diag_done = panel_for(t, k + 4 < nt);
    }
    // no rows under the matrix (right-hand sides in the slots of the last tile): nothing on the main stream has waited for
    // the engine's last tile yet -- what follows (the reductions) must
    if (mt == nt) launch_last_tile_gate(out + (nt - 1), abort_word, M);
    return 0;
}

int reset_info(cocons_fit *f)
{
    HIPCHK(hipMemcpyAsync(f->dinfo, f->hinfo_init, 2 * sizeof(int), hipMemcpyHostToDevice, f->stream));
    return 0;
}

// enqueue one full evaluation with nrhs right-hand-side rows; results land in hout/hinfo
static int enqueue_eval_impl(cocons_fit *f, const double *theta, const double *mean, bool use_trend,
                             const double *xb, int nxb, std::vector<hipEvent_t> *ev_upd, bool stage_events)
{
    const int nrhs = f->r + nxb;
    f->nrhs_cur = nrhs;
    // the padding rows under the right-hand sides (a 128-row tile holds them; r + q of its rows are used) only have to
    // be zeroed when they may hold something else: zero rows stay exactly zero through a factorisation that succeeds
    // (10 MB of strided stores, 22 us on the critical path of every evaluation at n = 10^4)
    const int was_clean = f->border_clean;
    const double *was_A = f->dA;
    if (int rc = fit_alloc_matrix(f, nrhs)) return rc;
    const bool zero_rest = !(was_clean == nrhs && was_A == f->dA);
    f->border_pending = nrhs;
    if (stage_events) hipEventRecord(f->ev[0], f->stream);
    if (int rc = reset_info(f)) return rc;
    if (f->taper_nnz > 0) { if (int rc = assemble_sigma_taper(f, theta)) return rc; }
    else assemble_sigma(f, theta, 0, 0, f->npad);
    // the engine becomes resident while the (short) right-hand-side kernel runs: not earlier -- a second
    // queue with a resident kernel cuts the workgroup dispatch rate of every other launch to a quarter
    // (tools/diag/occupancy_probe.hip), which costs the 12,000-workgroup assembly 6 % -- and not later, see engine_start
    const RhsLayout lay = rhs_layout(f, nrhs);
    const bool slots = lay.slots;
    FactorView fv = rhs_view(f, lay);
    fv.dag_ok = true;                                 // (the reductions below read the factor from both buffers)
    if (engine_wanted(f, fv))
        if (int rc = engine_start(f, fv)) return rc;
    assemble_rhs(f, mean, use_trend, xb, nxb, 0, f->npad, zero_rest, slots);
    if (stage_events) hipEventRecord(f->ev[1], f->stream);
    if (int rc = factorize(f, fv, ev_upd)) return rc;
    if (stage_events) hipEventRecord(f->ev[2], f->stream);
    launch_finalize(f->dA, f->lda, f->n, slots ? f->n : f->npad, nrhs, f->dout, f->stream, f->skew, f->npad,
                    f->dag_used ? f->dP : nullptr, f->dag_used ? 2 * TILE * f->dag_nsteps : 0);
    HIPCHK(hipMemcpyAsync(f->hinfo, f->dinfo, (size_t)(2 + nrhs * nrhs) * sizeof(double),       // info words + outputs
                          hipMemcpyDeviceToHost, f->stream));
    if (stage_events) hipEventRecord(f->ev[3], f->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int enqueue_eval(cocons_fit *f, const double *theta, const double *mean, bool use_trend,
                        const double *xb, int nxb, std::vector<hipEvent_t> *ev_upd, bool stage_events)
{
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    const int rc = enqueue_eval_impl(f, theta, mean, use_trend, xb, nxb, ev_upd, stage_events);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    f->enq_host_us += (t1.tv_sec - t0.tv_sec) * 1e6 + (t1.tv_nsec - t0.tv_nsec) * 1e-3;
    f->enq_calls++;
    return rc;
}

int info_status(cocons_fit *f)
{
    if (f->hinfo[1] != 0) {
        if (getenv("COCONS_DEBUG_ABORT")) debug_abort_report(f);
        return fail(ENGINE_ABORT, "hand-off between the diagonal-tile engine and the main stream timed out");
    }
    // the operation ran to its end on the schedule factorize chose: book-keeping of the engine's back-off
    f->engine_active_last = f->engine_used;
    if (f->engine_used) f->engine_fails = 0;
    else if (f->engine_skip > 0) --f->engine_skip;
    int info = f->hinfo[0];
    if (info != 0x7f7f7f7f) {
        info -= f->pad0;                // (minors are counted in the handle's internal order, behind its front padding)
        if (info < 1) info = 1;
        if (info > f->n_user) info = f->n_user;   // failure reported inside the identity padding cannot happen; clamp anyway
        g_err = "leading minor not positive";
        return info;
    }
    f->border_clean = f->border_pending;      // every pivot positive and finite: zero rows are still zero
    f->border_pending = -1;
    return 0;
}

// The engine could not be scheduled in time, or one of its partners could not (another process or stream kept
// every CU busy, or a profiler serialises kernels): the caller repeats THIS operation once on the plain schedule;
// the handle stays on it for a few more operations (2, 4, ... 64 with consecutive time-outs) and then tries the
// engine again.  Every time-out is counted (cocons_fit_engine_state).
bool engine_retry(cocons_fit *f, int st)
{
    if (st != ENGINE_ABORT || !(f->engine_used || f->follow_used)) return false;
    f->engine_retries++;
    f->engine_last_abort = f->hinfo[1];
    if (!f->engine_used || abort_class((unsigned)f->hinfo[1]) == ABORT_FOLLOW) f->follow_off = true;      // a follower of potrf_follow_kernel gave up: two launches from now on
    if (f->engine_fails < 6) f->engine_fails++;
    f->engine_skip = 1 << f->engine_fails;
    f->engine_live = false;
    f->engine_used = false;
    if (f->stream2) hipStreamSynchronize(f->stream2);
    return true;
}

// One evaluation of the objective, repeated after a hand-off time-out.  enqueue_eval brings the info words home together
// with the outputs (one copy); 0, a failing minor or an error.
static int run_eval(cocons_fit *f, const double *theta, const double *mean, bool use_trend, const double *xb, int nxb)
{
    for (;;) {
        if (int rc = enqueue_eval(f, theta, mean, use_trend, xb, nxb, nullptr, false)) return rc;
        HIPCHK(hipStreamSynchronize(f->stream));
        const int st = info_status(f);
        if (!engine_retry(f, st)) return st;
    }
}

// out[0] = 1 if the last completed operation of the handle ran on the engine schedule, out[1] = hand-off time-outs
// so far (each was followed by a repeat on the plain schedule), out[2] = abort code of the last one (0 = none)
extern "C" int cocons_fit_engine_state(cocons_fit *f, int *out)
{
    if (!f || !out) return fail(-1, "cocons_fit_engine_state: null argument");
    out[0] = f->engine_active_last ? 1 : 0;
    out[1] = f->engine_retries;
    out[2] = f->engine_last_abort;
    // (the slots of cocons_neg2loglik_batch are handles of their own: their time-outs count for this handle)
    for (cocons_fit *c : f->slots) {
        out[1] += c->engine_retries;
        if (!out[2]) out[2] = c->engine_last_abort;
    }
    // (so are the twin of cocons_sim_taper's pivot route and the unsorted clone cocons_sim_dense runs on)
    for (cocons_fit *c : {f->taper_twin, f->unsorted})
        if (c) {
            out[1] += c->engine_retries;
            if (!out[2]) out[2] = c->engine_last_abort;
        }
    return 0;
}

extern "C" int cocons_neg2loglik_dense(cocons_fit *f, const double *theta, const double *mean,
                                       double *sum_logliks, double *parts)
{
    FIT_ENTER(f);
    if (!theta || !mean || !sum_logliks) return fail(-1, "cocons_neg2loglik_dense: null argument");
    if (f->r < 1) return fail(-1, "cocons_neg2loglik_dense: fit has no z");
    if (f->coll_kind < 0) return fail(-7, "cocons_neg2loglik_dense: the communicator of this fit was aborted after an error");
    if (f->coll_kind) return sharded_eval(f, theta, mean, sum_logliks, parts);    // (also with one rank: the caller asked for it)
    if (int st = run_eval(f, theta, mean, true, nullptr, 0)) return st;
    dense_collect(f, sum_logliks, parts);
    return 0;
}

void dense_collect(cocons_fit *f, double *sum_logliks, double *parts)
{
    const int nr = f->r;
    double logdet = f->hout[0], total = 0.0;
    for (int k = 0; k < nr; ++k) {                                   // R/neg2loglikelihood.R:212-218
        double quad = f->hout[1 + k * nr + k];
        total += f->n_user * LOG_2PI + 2 * logdet + quad;
        if (parts) parts[1 + k] = quad;
    }
    if (parts) parts[0] = logdet;
    *sum_logliks = total;
}

// Batch of independent evaluations (the 2P finite-difference points of one L-BFGS-B gradient,
// R/optim.R:237-259 + R/profile.R:11-12, or getHessian's 3 P (P+1)/2 points,
// R/getFunctions.R:979-1016): evaluation i runs on slot i mod S, each slot a clone of the fit
// with its own factorisation buffer and stream, so the latency-bound panel chain of one
// evaluation overlaps the MFMA-bound updates and the VALU-bound assembly of the others.
// thetas: nb x (6 p) row-major tables; means: nb x p; values[nb]; status[nb] (0 / k>0 like the
// single call).  Returns 0 unless a HIP / argument error occurred.
extern "C" int cocons_neg2loglik_batch(cocons_fit *f, int nb, const double *thetas, const double *means,
                                       double *values, int *status)
{
    FIT_ENTER(f);
    if (nb < 0 || (nb > 0 && (!thetas || !means || !values || !status)))
        return fail(-1, "cocons_neg2loglik_batch: bad argument");
    if (f->r < 1) return fail(-1, "cocons_neg2loglik_batch: fit has no z");
    // How many evaluations in flight, and on which schedule (round 5, from the kernel trace of a batch,
    // tools/diag/batch_trace.py): a process's streams share FOUR hardware queues, and kernels of streams that share one run one
    // after the other.  A resident engine holds its queue for the whole evaluation, so two engine-schedule evaluations -- 2
    // main + 2 engine streams -- are all that fits; a third runs behind one of them (n = 4096: 862 evaluations/s with two
    // slots, 695 with three).  On the plain schedule a slot needs ONE queue -- once the slots no longer create engine streams
    // they never use, which had put four slots' main streams on two queues (one queue busy 88 % of the time in the trace) --
    // and four evaluations in flight beat two with engines at every size measured: n = 4096 1067 against 862 evaluations/s,
    // n = 10^4 134 against 128 (33-point gradient).  More hardware queues (GPU_MAX_HW_QUEUES = 8, 12) make it WORSE (642 ... 996
    // at n = 4096): four is what the chip runs side by side.  COCONS_BATCH_ENGINE=1 (two engine slots) and COCONS_BATCH_SLOTS override.
    static int nslots_env = -1, batch_engine = -2;
    if (nslots_env < 0) {
        const char *e = getenv("COCONS_BATCH_SLOTS");
        nslots_env = e ? atoi(e) : 0;
        if (nslots_env < 0) nslots_env = 0;
        if (nslots_env > 8) nslots_env = 8;
        const char *e2 = getenv("COCONS_BATCH_ENGINE");
        batch_engine = e2 ? (atoi(e2) ? 1 : 0) : -1;
    }
    const bool eng_mode = batch_engine >= 0 ? batch_engine == 1 : false;
    const int nslots = nslots_env > 0 ? nslots_env : (eng_mode ? 2 : 4);
    int S = nb < nslots ? (nb > 0 ? nb : 1) : nslots;
    // every extra slot is a clone of the handle with its own n x n factorisation buffer
    // (lda * npad * 8 bytes: 0.83 GB at n = 10^4); if one cannot be created (out of memory) the
    // batch runs on the slots that exist -- slot 0 is the fit itself, so it always completes
    // (the slots are handles of their own in the registry: held for the whole call, like the handle itself, so that no other
    // thread's stream self-test launches probe kernels between their evaluations)
    std::vector<std::unique_lock<std::recursive_mutex>> slot_locks;
    for (cocons_fit *c : f->slots) slot_locks.emplace_back(c->op_mu);
    while ((int)f->slots.size() < S - 1) {
        cocons_fit *c = clone_for_slot(f, eng_mode);
        if (!c) { (void)hipGetLastError(); break; }
        slot_locks.emplace_back(c->op_mu);
        f->slots.push_back(c);
    }
    const bool engine_saved = f->engine_ok;
    if (!eng_mode) {
        if (S > 1) f->engine_ok = false;
        for (auto c : f->slots) c->engine_ok = false;
    }
    if (S > (int)f->slots.size() + 1) S = (int)f->slots.size() + 1;
    for (int i = 0; i < nb; ++i) { values[i] = NAN; status[i] = -1; }   // never left unwritten
    std::vector<int> pending(S, -1);
    const int tp = 6 * f->p;
    int rc_all = 0;
    auto slot_of = [&](int s) { return s == 0 ? f : f->slots[s - 1]; };
    auto collect = [&](int s) -> int {
        cocons_fit *c = slot_of(s);
        int i = pending[s];
        if (i < 0) return 0;
        pending[s] = -1;
        HIPCHK(hipStreamSynchronize(c->stream));
        int st = info_status(c);
        if (engine_retry(c, st)) {           // hand-off time-out: this evaluation again, on the plain schedule
            if (int rc = enqueue_eval(c, thetas + (size_t)i * tp, means + (size_t)i * f->p, true, nullptr, 0, nullptr, false))
                return rc;
            HIPCHK(hipStreamSynchronize(c->stream));
            st = info_status(c);
        }
        status[i] = st;
        if (st == 0) dense_collect(c, &values[i], nullptr);
        else values[i] = NAN;
        return 0;
    };
    for (int i = 0; i < nb; ++i) {
        int s = i % S;
        if (int rc = collect(s)) { rc_all = rc; break; }
        cocons_fit *c = slot_of(s);
        if (int rc = enqueue_eval(c, thetas + (size_t)i * tp, means + (size_t)i * f->p, true, nullptr, 0, nullptr, false)) {
            rc_all = rc;
            break;
        }
        pending[s] = i;
    }
    for (int s = 0; s < S; ++s)
        if (int rc = collect(s)) rc_all = rc_all ? rc_all : rc;
    f->engine_ok = engine_saved;
    return rc_all;
}

// small dense SPD solve on the host (q x q, q <= COCONS_P_MAX): W = C C^T, returns
// sum(log(diag(C))) and solves W x = b in place for nb right-hand sides.
static int host_spd_solve(int q, std::vector<double> &W, int nb, std::vector<double> &B, double *logdet_half)
{
    double ld = 0;
    for (int j = 0; j < q; ++j) {
        double d = W[j + j * q];
        for (int k = 0; k < j; ++k) d -= W[j + k * q] * W[j + k * q];
        if (!(d > 0)) return j + 1;
        d = std::sqrt(d);
        W[j + j * q] = d;
        ld += std::log(d);
        for (int i = j + 1; i < q; ++i) {
            double s = W[i + j * q];
            for (int k = 0; k < j; ++k) s -= W[i + k * q] * W[j + k * q];
            W[i + j * q] = s / d;
        }
    }
    for (int c = 0; c < nb; ++c) {
        double *b = &B[(size_t)c * q];
        for (int i = 0; i < q; ++i) {
            double s = b[i];
            for (int k = 0; k < i; ++k) s -= W[i + k * q] * b[k];
            b[i] = s / W[i + i * q];
        }
        for (int i = q - 1; i >= 0; --i) {
            double s = b[i];
            for (int k = i + 1; k < q; ++k) s -= W[k + i * q] * b[k];
            b[i] = s / W[i + i * q];
        }
    }
    *logdet_half = ld;
    return 0;
}

// shared tail of Profile / REML: Gram matrix G of [y_1..y_r, Y] (Y = L^-1 Xb) ->
// quad_k = G_kk - g_k' W^-1 g_k with W = Y'Y, g_k = Y'y_k.
int profile_tail(cocons_fit *f, int nxb, double n_eff, bool reml, double *sum_logliks, double *parts)
{
    const int r = f->r, nr = r + nxb;
    const double *G = f->hout + 1;
    std::vector<double> W((size_t)nxb * nxb), Bv((size_t)nxb * r);
    for (int a = 0; a < nxb; ++a)
        for (int b = 0; b < nxb; ++b) W[a + (size_t)b * nxb] = G[(r + a) * nr + (r + b)];
    for (int k = 0; k < r; ++k)
        for (int a = 0; a < nxb; ++a) Bv[(size_t)k * nxb + a] = G[k * nr + (r + a)];
    std::vector<double> g = Bv;
    double ldW = 0;
    if (host_spd_solve(nxb, W, r, Bv, &ldW)) return fail(-4, "X' Sigma^-1 X is not positive definite");
    double logdet = f->hout[0], total = 0.0;
    for (int k = 0; k < r; ++k) {
        double corr = 0;
        for (int a = 0; a < nxb; ++a) corr += g[(size_t)k * nxb + a] * Bv[(size_t)k * nxb + a];
        double quad = G[k * nr + k] - corr;
        total += n_eff * LOG_2PI + 2 * logdet + (reml ? 2 * ldW : 0.0) + quad;
        if (parts) parts[2 + k] = quad;
    }
    if (parts) {
        parts[0] = logdet; parts[1] = ldW;
        // generalised-least-squares coefficients W^-1 Xb' Sigma^-1 zbar, zbar = rowSums(z)/r -- the
        // "Compute Betas" block of cocoOptim's pml/reml branch (R/optim.R:329-341)
        for (int a = 0; a < nxb; ++a) {
            double s = 0;
            for (int k = 0; k < r; ++k) s += Bv[(size_t)k * nxb + a];
            parts[2 + r + a] = s / r;
        }
    }
    *sum_logliks = total;
    return 0;
}

extern "C" int cocons_neg2loglik_profile(cocons_fit *f, const double *theta, double *sum_logliks, double *parts)
{
    FIT_ENTER(f);
    if (int rc = no_taper(f, "cocons_neg2loglik_profile")) return rc;
    if (!theta || !sum_logliks) return fail(-1, "cocons_neg2loglik_profile: null argument");
    if (f->r < 1 || f->q < 1) return fail(-1, "cocons_neg2loglik_profile: fit needs z and x_betas");
    if (int st = run_eval(f, theta, nullptr, false, f->dxb, f->q)) return st;
    return profile_tail(f, f->q, (double)f->n_user, false, sum_logliks, parts);   // R/neg2loglikelihood.R:155-160
}

extern "C" int cocons_neg2loglik_reml(cocons_fit *f, const double *theta, int rank, double *sum_logliks, double *parts)
{
    FIT_ENTER(f);
    if (int rc = no_taper(f, "cocons_neg2loglik_reml")) return rc;
    if (!theta || !sum_logliks) return fail(-1, "cocons_neg2loglik_reml: null argument");
    if (f->r < 1) return fail(-1, "cocons_neg2loglik_reml: fit has no z");
    if (int st = run_eval(f, theta, nullptr, false, f->dX, f->p)) return st;
    return profile_tail(f, f->p, (double)(f->n_user - rank), true, sum_logliks, parts);   // :283-287
}
