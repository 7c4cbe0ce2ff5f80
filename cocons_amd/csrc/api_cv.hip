// api_cv.hip -- C ABI, cross-validated predictions: cocons_cv_dense, cocons_cv_taper, cocons_cv_taper_folds.
//
// With K = Sigma^-1, U = K R (R = z - X mean) and a held-out set B with complement A,
//     R_B - Sigma_BA Sigma_AA^-1 R_A = (K_BB)^-1 U_B,     Cov(z_B | z_A) = (K_BB)^-1.
// One gradient operation without its contraction (grad_enqueue, full = false) leaves -K in the lower triangle of the leading
// square and U in grad->AR; every fold then costs its own block of K, by size:
//   1          closed form, one thread per observation (launch_cv_loo) -- with fold = NULL the whole call;
//   2 .. 128   one workgroup per fold with the block in LDS, one launch per size class 16 / 32 / 64 / 128 (launch_cv_folds);
//   > 128      one fold after the other through the library's factorisation on a scratch matrix of the call,
//              [K_BB ; U_B' ; I] -> [C ; (C^-1 U_B)' ; C^-T], whose border gives resid and var as the two kriging reductions
//              (launch_row_reduce).  factorize() touches the view it is given and the handle's hand-off scratch only: dA
//              still holds -K when the next fold is gathered.  Its front-identity step belongs to views that start with the
//              handle's observations; a fold's block does not, so pad0 is 0 while it is factored (FoldView).
// The kernels write in the handle's internal order; labels go in and results come out through cocons_fit::obs_pos.
// The info word: Sigma's failing minor is the call's k > 0; a failing minor inside a fold's block is the fold's (-5).  Between
// the factorisations of one operation the word is taken out and put back on the stream (launch_cv_info_take / _put), so the
// whole call stays ONE run_op operation that a hand-off time-out repeats from the assembly.
#include "fit.hpp"

namespace {

constexpr int INFO_CLEAN = 0x7f7f7f7f;      // reset_info's "no failing minor"

// the folds of one call, in the handle's internal order
struct CvPlan {
    std::vector<int> idx, off, lab;         // fold g (only labels somebody carries): positions idx[off[g] .. off[g + 1]), ascending
    std::vector<int> single_idx, single_lab;
    std::vector<int> flist[4];              // folds of 2 .. 16, 17 .. 32, 33 .. 64, 65 .. 128 observations
    std::vector<int> large;
    int bmax = 0;                           // largest fold beyond CV_SMALL_MAX
};

struct CvDevice {
    DevBuf<int> ints, fail;                 // the plan, one upload; fail: [0] failing fold, [1] Sigma's info word while folds factor
    DevBuf<double> var, res;                // npad, npad x r: results in the internal order
    DevBuf<double> scratch, tres, tvar, red;     // large folds
    const int *idx = nullptr, *off = nullptr, *lab = nullptr, *single_idx = nullptr, *single_lab = nullptr;
    const int *flist[4] = {nullptr, nullptr, nullptr, nullptr};
};

int cv_enqueue(cocons_fit *f, const double *theta, const double *mean, const CvPlan *plan, CvDevice &d, double *hvar, double *hres,
               int *hfail)
{
    const int npad = f->npad, nr = f->r;
    hipStream_t s = f->stream;
    HIPCHK(hipMemsetAsync(d.fail, 0x7f, 2 * sizeof(int), s));
    if (int rc = grad_enqueue(f, theta, mean, false, nullptr)) return rc;
    const double *S = f->dA, *U = f->grad->AR;
    const size_t lds = f->lda;
    if (!plan) {
        launch_cv_loo(S, lds, U, (size_t)npad, nr, nullptr, nullptr, f->pad0, f->n_user, d.var, d.res, (size_t)npad, d.fail, s);
    } else {
        launch_cv_loo(S, lds, U, (size_t)npad, nr, d.single_idx, d.single_lab, 0, (int)plan->single_idx.size(), d.var, d.res,
                      (size_t)npad, d.fail, s);
        for (int c = 0; c < 4; ++c)
            HIPCHK(launch_cv_folds(16 << c, S, lds, U, (size_t)npad, nr, d.idx, d.off, d.flist[c], d.lab, (int)plan->flist[c].size(),
                                   d.var, d.res, (size_t)npad, d.fail, s));
        if (!plan->large.empty()) {
            bool eng = f->engine_used, fol = f->follow_used;     // (a time-out of ANY factorisation of the call is repeated)
            const int rt = round_up(nr, TILE);
            launch_cv_info_take(f->dinfo, INFO_CLEAN, d.fail + 1, nullptr, 0, s);
            for (int g : plan->large) {
                const int b = plan->off[g + 1] - plan->off[g], bpad = round_up(b, TILE);
                const size_t ldo = 2 * (size_t)bpad + (size_t)rt;
                const int *pos = d.idx + plan->off[g];
                launch_cv_gather(S, lds, U, (size_t)npad, nr, pos, b, bpad, rt, d.scratch, ldo, s);
                {
                    FoldView fv(f);
                    FactorView v;
                    v.A = d.scratch; v.lda = ldo; v.nt = bpad / TILE; v.mt = (int)(ldo / TILE);
                    if (int rc = factorize(f, v, nullptr)) return rc;
                }
                eng = eng || f->engine_used; fol = fol || f->follow_used;
                // (one call per realisation: the existing reduction, unchanged; each call forms the same quadform again --
                // r - 1 passes over the b x b border more than needed, against the b^3 of the factorisation in front of them)
                for (int k = 0; k < nr; ++k)
                    launch_row_reduce(d.scratch, ldo, b, bpad + k, bpad + rt, b, d.tres + (size_t)k * b, d.tvar, d.red, s);
                launch_cv_scatter(pos, b, nr, d.tvar, d.tres, d.var, d.res, (size_t)npad, s);
                launch_cv_info_take(f->dinfo, INFO_CLEAN, nullptr, d.fail, plan->lab[g], s);
            }
            launch_cv_info_put(f->dinfo, d.fail + 1, s);
            f->engine_used = eng; f->follow_used = fol;
        }
    }
    HIPCHK(hipMemcpyAsync(hvar, d.var, (size_t)npad * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hres, d.res, (size_t)npad * nr * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hfail, d.fail, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int cocons_cv_dense(cocons_fit *f, const double *theta, const double *mean, int nfold, const int *fold, double *resid,
                               double *var)
{
    const char *who = "cocons_cv_dense";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !mean || !resid || !var) return fail(-1, "%s: null argument", who);
    if (nfold < 0) return fail(-1, "%s: nfold = %d is negative", who, nfold);
    if ((fold == nullptr) != (nfold == 0))
        return fail(-1, "%s: fold and nfold disagree (fold = NULL with nfold = 0 is leave-one-out)", who);
    FIT_ENTER(f);
    if (f->taper_nnz > 0) return fail(-1, "%s: not available on a taper fit (cocons_cv_taper is)", who);
    if (f->coll_kind) return fail(-1, "%s: not available on a sharded handle", who);
    if (f->r < 1) return fail(-1, "%s: fit has no z", who);
    const int n = f->n_user, npad = f->npad, nr = f->r;
    if ((int)f->obs_pos.size() != n) return fail(-1, "%s: the handle keeps no order of its observations", who);
    // (leave-one-out of a single observation is answered, as cocons_cv_taper answers it: nothing is left to predict from, and
    // (K_11)^-1 U_1 and (K_11)^-1 are the residual and Sigma_11)
    CvPlan plan;
    if (fold) {
        std::vector<int> cnt((size_t)nfold, 0);
        for (int i = 0; i < n; ++i) {
            if (fold[i] < 0 || fold[i] >= nfold)
                return fail(-1, "%s: label %d of observation %d is outside [0, %d)", who, fold[i], i, nfold);
            ++cnt[fold[i]];
        }
        std::vector<int> start((size_t)nfold, -1);
        plan.off.push_back(0);
        for (int l = 0; l < nfold; ++l) {
            if (cnt[l] == n) return fail(-1, "%s: fold %d holds all %d observations", who, l, n);
            if (cnt[l] == 0) continue;
            start[l] = plan.off.back();
            plan.lab.push_back(l);
            plan.off.push_back(plan.off.back() + cnt[l]);
        }
        plan.idx.resize((size_t)n);
        std::vector<int> fillp(start);
        for (int i = 0; i < n; ++i) plan.idx[fillp[fold[i]]++] = f->obs_pos[i];
        for (size_t g = 0; g + 1 < plan.off.size(); ++g) {
            std::sort(plan.idx.begin() + plan.off[g], plan.idx.begin() + plan.off[g + 1]);
            const int b = plan.off[g + 1] - plan.off[g];
            if (b == 1) { plan.single_idx.push_back(plan.idx[plan.off[g]]); plan.single_lab.push_back(plan.lab[g]); }
            else if (b <= CV_SMALL_MAX) plan.flist[b <= 16 ? 0 : b <= 32 ? 1 : b <= 64 ? 2 : 3].push_back((int)g);
            else { plan.large.push_back((int)g); if (b > plan.bmax) plan.bmax = b; }
        }
    }
    if (int rc = grad_prepare(f, who, nr)) return rc;
    CvDevice d;
    std::vector<double> hvar((size_t)npad), hres((size_t)npad * nr);
    int hfail = INFO_CLEAN;
    std::vector<int> ints;
    StreamDrain drain{f->stream, false};       // (declared behind the buffers: the stream is idle before they are freed)
    HIPCHK_AT(who, d.fail.alloc(2));
    HIPCHK_AT(who, d.var.alloc((size_t)npad));
    HIPCHK_AT(who, d.res.alloc((size_t)npad * nr));
    if (fold) {
        const std::vector<int> *parts[9] = {&plan.idx, &plan.off, &plan.lab, &plan.single_idx, &plan.single_lab, &plan.flist[0],
                                            &plan.flist[1], &plan.flist[2], &plan.flist[3]};
        size_t at[9], tot = 0;
        for (int k = 0; k < 9; ++k) { at[k] = tot; tot += parts[k]->size(); }
        ints.resize(tot + 1);
        for (int k = 0; k < 9; ++k) std::copy(parts[k]->begin(), parts[k]->end(), ints.begin() + at[k]);
        HIPCHK_AT(who, d.ints.alloc(tot + 1));
        HIPCHK_AT(who, hipMemcpyAsync(d.ints, ints.data(), (tot + 1) * sizeof(int), hipMemcpyHostToDevice, f->stream));
        d.idx = d.ints + at[0]; d.off = d.ints + at[1]; d.lab = d.ints + at[2];
        d.single_idx = d.ints + at[3]; d.single_lab = d.ints + at[4];
        for (int c = 0; c < 4; ++c) d.flist[c] = d.ints + at[5 + c];
        if (plan.bmax > 0) {
            const size_t bpad = (size_t)round_up(plan.bmax, TILE), rt = (size_t)round_up(nr, TILE);
            const size_t counts[4] = {(2 * bpad + rt) * bpad, (size_t)plan.bmax * nr, (size_t)plan.bmax,
                                      row_reduce_scratch_doubles(plan.bmax, plan.bmax)};
            DevBuf<double> *bufs[4] = {&d.scratch, &d.tres, &d.tvar, &d.red};
            if (hipError_t e = alloc_call_buffers(bufs, counts, 4))
                return fail(-100 - (int)e, "%s: the device cannot hold the %zu bytes of the largest fold's matrix (%d observations): %s",
                            who, (counts[0] + counts[1] + counts[2] + counts[3]) * sizeof(double), plan.bmax, hipGetErrorString(e));
        }
    }
    GradLayout layout(f, nr);
    const int st = run_op(f, who, [&]() -> int {
        return cv_enqueue(f, theta, mean, fold ? &plan : nullptr, d, hvar.data(), hres.data(), &hfail);
    });
    if (st) return st;                  // failing minor of Sigma: nothing written
    if (hfail != INFO_CLEAN) {
        if (fold) return fail(-5, "%s: the hold-out block of Sigma^-1 of fold %d is not positive definite", who, hfail);
        int obs = -1;
        for (int i = 0; i < n; ++i)
            if (f->obs_pos[i] == f->pad0 + hfail) { obs = i; break; }
        return fail(-5, "%s: the diagonal of Sigma^-1 at observation %d (its own fold) is not positive", who, obs);
    }
    for (int i = 0; i < n; ++i) {
        const size_t pos = (size_t)f->obs_pos[i];
        var[i] = hvar[pos];
        for (int k = 0; k < nr; ++k) resid[(size_t)i + (size_t)k * n] = hres[pos + (size_t)k * npad];
    }
    return 0;
}

// ---- taper handles ---------------------------------------------------------------------------------------------------------
// Leave-one-out from the diagonal of the selected inverse: the whole of cocons_cv_taper, and cocons_cv_taper_folds without
// folds.  bytes (may be null): the device bytes of the call.
static int cv_taper_loo(cocons_fit *f, const char *who, const double *theta, const double *mean, double *resid, double *var,
                        long long *bytes)
{
    const int n = f->n, npad = f->npad, nr = f->r;
    if ((int)f->taper_inv.size() != n) return fail(-1, "%s: the handle keeps no order of its observations", who);
    if (int rc = taper_grad_prepare(f, who)) return rc;
    DevBuf<int> dfail;
    DevBuf<double> dvar, dres;
    std::vector<double> hvar((size_t)npad), hres((size_t)npad * nr);
    int hfail = INFO_CLEAN;
    StreamDrain drain{f->stream, false};
    HIPCHK_AT(who, dfail.alloc(2));
    HIPCHK_AT(who, dvar.alloc((size_t)npad));
    HIPCHK_AT(who, dres.alloc((size_t)npad * nr));
    if (bytes) *bytes = (long long)(2 * sizeof(int) + ((size_t)npad + (size_t)npad * nr) * sizeof(double));
    const int st = run_op(f, who, [&]() -> int {
        hipStream_t s = f->stream;
        HIPCHK(hipMemsetAsync(dfail, 0x7f, 2 * sizeof(int), s));
        if (int rc = taper_grad_enqueue(f, theta, mean, nullptr)) return rc;
        TaperGradState *G = f->tgrad.get();
        launch_cv_taper(G->Z, G->ldz, f->skew, npad, n, G->AR, (size_t)npad, nr, dvar, dres, (size_t)npad, dfail, s);
        HIPCHK(hipMemcpyAsync(hvar.data(), dvar, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hres.data(), dres, (size_t)npad * nr * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&hfail, dfail, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipGetLastError());
        return 0;
    });
    border_unknown(f);
    if (st) return st;                  // failing minor: nothing written
    if (hfail != INFO_CLEAN) {
        int obs = -1;
        for (int i = 0; i < n; ++i)
            if (f->taper_inv[i] == hfail) { obs = i; break; }
        return fail(-5, "%s: the diagonal of S^-1 at observation %d (its own fold) is not positive", who, obs);
    }
    for (int i = 0; i < n; ++i) {
        const size_t pos = (size_t)f->taper_inv[i];
        var[i] = hvar[pos];
        for (int k = 0; k < nr; ++k) resid[(size_t)i + (size_t)k * n] = hres[pos + (size_t)k * npad];
    }
    return 0;
}

extern "C" int cocons_cv_taper(cocons_fit *f, const double *theta, const double *mean, double *resid, double *var)
{
    const char *who = "cocons_cv_taper";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !mean || !resid || !var) return fail(-1, "%s: null argument", who);
    FIT_ENTER(f);
    if (int rc = taper_refuse(f, who, "cocons_cv_dense")) return rc;
    return cv_taper_loo(f, who, theta, mean, resid, var, nullptr);
}

// Folds on the held band factor (continued).  U = S^-1 R and the singletons come from the selected inverse as
// in cocons_cv_taper.  For the folds of two or more, S is factored once more on the band schedule (the sweep consumed the
// factor) and copied into buffers of the call; the folds' observations then go through the sliding-window band solve as
// unit rows, V = E_B' L^-T, in chunks of whole 128-row tiles -- folds of up to 128 rows packed into tiles, a larger fold from
// a tile boundary on --, and K_BB = V V' is accumulated fold by fold while the window slides (krige_band_gram_kernel, one
// task per 64-row strip x 128-column tile inside a fold or a packed tile).  Per chunk the tails of cocons_cv_dense: the LDS
// kernel on a fold's sub-block of its tile, the library's factorisation on a larger fold's bordered scratch matrix, whose
// top block the Gram product has filled in place.  Everything behind the selected inverse runs on the plain schedule.
namespace {

constexpr int CV_TF_DEPTH = 8;                       // tile columns per Gram launch (krige_band_schur_kernel's measured depth)
constexpr int CV_TF_ROWS_AUTO = 16384;               // rows of a chunk with max_rows = 0, at most
constexpr size_t CV_TF_BYTES_AUTO = (size_t)1 << 30; // ... and the ring and the blocks it may take
constexpr int CV_TF_ROWS_MAX = 1 << 20;              // a caller's max_rows beyond this is cut (slot offsets are ints)

// one chunk of the ring solve: whole tiles and whole folds
struct TfChunk {
    int rows = 0, ntile = 0;                 // rows of the ring; the packed small-fold tiles come first
    size_t blk = 0;                          // doubles of its blocks: ntile tiles of 128 x 128, then the large folds' scratch
    std::vector<int> flist[4], large;        // its folds by size class, and beyond CV_SMALL_MAX
    std::vector<int> ci, rp;                 // the unit rows as a 1-based CSR over the caller's observations (padding rows empty)
    std::vector<KrigeGramTask> tasks;
    std::vector<int> boff;                   // band_buckets' bucket offsets (host)
    size_t at_fl[4] = {0, 0, 0, 0}, at_dst = 0, at_src = 0, at_task = 0;      // where its arrays sit in the uploads
};

// COCONS_CV_GRAM_DEPTH, read per call: 1 .. 16, or refused
int cv_gram_depth(const char *who, int *depth)
{
    *depth = CV_TF_DEPTH;
    const char *e = getenv("COCONS_CV_GRAM_DEPTH");
    if (!e || !*e) return 0;
    char *end = nullptr;
    const long v = strtol(e, &end, 10);
    if (*end || v < 1 || v > 16) return fail(-1, "%s: COCONS_CV_GRAM_DEPTH = \"%s\" (1 .. 16 expected)", who, e);
    *depth = (int)v;
    return 0;
}

}  // namespace

extern "C" int cocons_cv_taper_folds(cocons_fit *f, const double *theta, const double *mean, int nfold, const int *fold,
                                     int max_rows, double *resid, double *var, long long *stats5)
{
    const char *who = "cocons_cv_taper_folds";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !mean || !resid || !var) return fail(-1, "%s: null argument", who);
    if (nfold < 0) return fail(-1, "%s: nfold = %d is negative", who, nfold);
    if ((fold == nullptr) != (nfold == 0))
        return fail(-1, "%s: fold and nfold disagree (fold = NULL with nfold = 0 is leave-one-out)", who);
    if (max_rows < 0) return fail(-1, "%s: max_rows = %d is negative", who, max_rows);
    FIT_ENTER(f);
    if (int rc = taper_refuse(f, who, "cocons_cv_dense")) return rc;
    const int n = f->n, npad = f->npad, nr = f->r, nt = f->nt;
    if ((int)f->taper_inv.size() != n) return fail(-1, "%s: the handle keeps no order of its observations", who);
    if (!fold) {
        long long bytes = 0;
        const int rc = cv_taper_loo(f, who, theta, mean, resid, var, &bytes);
        if (rc == 0 && stats5) { stats5[0] = n; stats5[1] = stats5[2] = stats5[3] = 0; stats5[4] = bytes; }
        return rc;
    }
    // ---- the folds in the handle's order (cocons_cv_dense's plan, positions through taper_inv)
    CvPlan plan;
    std::vector<int> multi;                                  // folds of two or more, in label order
    {
        std::vector<int> cnt((size_t)nfold, 0);
        for (int i = 0; i < n; ++i) {
            if (fold[i] < 0 || fold[i] >= nfold)
                return fail(-1, "%s: label %d of observation %d is outside [0, %d)", who, fold[i], i, nfold);
            ++cnt[fold[i]];
        }
        std::vector<int> start((size_t)nfold, -1);
        plan.off.push_back(0);
        for (int l = 0; l < nfold; ++l) {
            if (cnt[l] == n) return fail(-1, "%s: fold %d holds all %d observations", who, l, n);
            if (cnt[l] == 0) continue;
            start[l] = plan.off.back();
            plan.lab.push_back(l);
            plan.off.push_back(plan.off.back() + cnt[l]);
        }
        plan.idx.resize((size_t)n);
        std::vector<int> fillp(start);
        for (int i = 0; i < n; ++i) plan.idx[fillp[fold[i]]++] = f->taper_inv[i];
        for (size_t g = 0; g + 1 < plan.off.size(); ++g) {
            std::sort(plan.idx.begin() + plan.off[g], plan.idx.begin() + plan.off[g + 1]);
            const int b = plan.off[g + 1] - plan.off[g];
            if (b == 1) { plan.single_idx.push_back(plan.idx[plan.off[g]]); plan.single_lab.push_back(plan.lab[g]); continue; }
            multi.push_back((int)g);
            if (b > CV_SMALL_MAX) { plan.large.push_back((int)g); if (b > plan.bmax) plan.bmax = b; }
        }
    }
    int D = 0;
    if (int rc = cv_gram_depth(who, &D)) return rc;
    BandPlan bplan;
    if (const char *why = band_plan(nt, envelope_or_null(f), f->taper_maxband, bplan)) return fail(-1, "%s: %s", who, why);
    const int Wr = std::min(bplan.W + D - 1, nt);
    const int rt = round_up(nr, TILE);
    const size_t nfolds = plan.lab.size();
    // ---- units (a packed tile of small folds, or one large fold) and chunks of whole units
    std::vector<long long> base(nfolds ? nfolds : 1, 0);     // per fold: where its K_BB starts in its chunk's blocks
    std::vector<TfChunk> chunks;
    size_t nsmall = 0;
    if (!multi.empty()) {
        struct Unit { int rows; size_t blk; bool large; std::vector<int> folds; };
        std::vector<Unit> units;
        int used = TILE;                                      // (rows taken in the open tile: none is open)
        for (int g : multi) {
            const int b = plan.off[g + 1] - plan.off[g];
            if (b > CV_SMALL_MAX) continue;
            ++nsmall;
            if (used + b > TILE) { units.push_back(Unit{TILE, (size_t)TILE * TILE, false, {}}); used = 0; }
            units.back().folds.push_back(g);
            used += b;
        }
        for (int g : plan.large) {
            const size_t bpad = (size_t)round_up(plan.off[g + 1] - plan.off[g], TILE);
            units.push_back(Unit{(int)bpad, (2 * bpad + (size_t)rt) * bpad, true, {g}});
        }
        const int rows_max = max_rows > 0 ? round_up(std::min(max_rows, CV_TF_ROWS_MAX), TILE) : CV_TF_ROWS_AUTO;
        const size_t row_bytes = (size_t)Wr * TILE * sizeof(double);
        std::vector<int> posobs((size_t)n);
        for (int i = 0; i < n; ++i) posobs[f->taper_inv[i]] = i;
        std::vector<int> rowobs;                              // per row of the open chunk: the observation (1-based), 0 = padding
        auto close = [&]() {
            TfChunk &c = chunks.back();
            c.rp.assign((size_t)c.rows + 1, 1);
            for (int i = 0; i < c.rows; ++i) {
                c.rp[i + 1] = c.rp[i] + (rowobs[i] ? 1 : 0);
                if (rowobs[i]) c.ci.push_back(rowobs[i]);
            }
        };
        for (const Unit &u : units) {
            bool open = !chunks.empty();
            if (open) {
                const size_t rows = (size_t)chunks.back().rows + u.rows, blk = chunks.back().blk + u.blk;
                if (rows > (size_t)rows_max || (max_rows == 0 && rows * row_bytes + blk * sizeof(double) > CV_TF_BYTES_AUTO)) {
                    close();
                    open = false;
                }
            }
            if (!open) { chunks.emplace_back(); rowobs.clear(); }
            TfChunk &c = chunks.back();
            const int r0 = c.rows;
            rowobs.resize((size_t)r0 + u.rows, 0);
            if (!u.large) {
                int o = 0;
                for (int g : u.folds) {
                    const int b = plan.off[g + 1] - plan.off[g];
                    for (int k = 0; k < b; ++k) rowobs[(size_t)r0 + o + k] = posobs[plan.idx[plan.off[g] + k]] + 1;
                    base[g] = (long long)(c.blk + (size_t)o * (TILE + 1));
                    c.flist[b <= 16 ? 0 : b <= 32 ? 1 : b <= 64 ? 2 : 3].push_back(g);
                    o += b;
                }
                for (int st = 0; st < 2; ++st) c.tasks.push_back(KrigeGramTask{r0 + 64 * st, r0, TILE, 0, (long long)(c.blk + 64 * st)});
                ++c.ntile;
            } else {
                const int g = u.folds[0], b = plan.off[g + 1] - plan.off[g];
                const size_t ldo = 2 * (size_t)u.rows + (size_t)rt;
                for (int k = 0; k < b; ++k) rowobs[(size_t)r0 + k] = posobs[plan.idx[plan.off[g] + k]] + 1;
                base[g] = (long long)c.blk;
                c.large.push_back(g);
                for (int st = 0; st < u.rows / 64; ++st)
                    for (int J = 0; 2 * J <= st; ++J)
                        c.tasks.push_back(KrigeGramTask{r0 + 64 * st, r0 + TILE * J, (int)ldo, 0,
                                                        (long long)(c.blk + 64 * (size_t)st + (size_t)TILE * J * ldo)});
            }
            c.rows += u.rows;
            c.blk += u.blk;
        }
        close();
    }
    if (int rc = taper_grad_prepare(f, who)) return rc;
    // ---- one upload of the plan; the buckets of every chunk
    std::vector<int> ints, hci, hdst, hsrc;
    std::vector<KrigeGramTask> tasks;
    size_t at[5], rows_big = 0, blk_big = 0, ent_big = 1;
    {
        const std::vector<int> *parts[5] = {&plan.idx, &plan.off, &plan.lab, &plan.single_idx, &plan.single_lab};
        for (int k = 0; k < 5; ++k) { at[k] = ints.size(); ints.insert(ints.end(), parts[k]->begin(), parts[k]->end()); }
        for (TfChunk &c : chunks) {
            for (int k = 0; k < 4; ++k) { c.at_fl[k] = ints.size(); ints.insert(ints.end(), c.flist[k].begin(), c.flist[k].end()); }
            band_buckets<TILE>(nt, f->taper_inv.data(), c.ci.data(), c.rp.data(), 0, c.rows, c.rows, hci, hdst, hsrc, c.boff);
            c.at_dst = ints.size(); ints.insert(ints.end(), hdst.begin(), hdst.end());
            c.at_src = ints.size(); ints.insert(ints.end(), hsrc.begin(), hsrc.end());
            c.at_task = tasks.size(); tasks.insert(tasks.end(), c.tasks.begin(), c.tasks.end());
            rows_big = std::max(rows_big, (size_t)c.rows); blk_big = std::max(blk_big, c.blk); ent_big = std::max(ent_big, hdst.size());
        }
        ints.push_back(0);
    }
    DevBuf<int> dints, dfail, dtoff;
    DevBuf<long long> dbase;
    DevBuf<KrigeGramTask> dtasks;
    DevBuf<double> dvar, dres, dL, dQ, dw, dring, dblocks, dones, dst, dq, dtres, dred;
    std::vector<double> hvar((size_t)npad), hres((size_t)npad * nr);
    int hfail = INFO_CLEAN;
    StreamDrain drain{f->stream, false};
    hipStream_t s = f->stream;
    size_t bytes = 0;
    {
        const bool ring = !chunks.empty();
        const size_t bm = (size_t)plan.bmax;
        const size_t counts[12] = {(size_t)npad, (size_t)npad * nr,
                                   ring ? (size_t)bplan.toff[nt] * TILE * TILE : 0, ring ? (size_t)nt * 2048 : 0, ring ? (size_t)npad : 0,
                                   rows_big * Wr * TILE, blk_big, ring ? ent_big : 0, rows_big, rows_big,
                                   bm * nr + bm, bm ? row_reduce_scratch_doubles(plan.bmax, plan.bmax) : 0};
        DevBuf<double> *bufs[12] = {&dvar, &dres, &dL, &dQ, &dw, &dring, &dblocks, &dones, &dst, &dq, &dtres, &dred};
        for (int k = 0; k < 12; ++k) bytes += counts[k] * sizeof(double);
        bytes += (ints.size() + 2 + (ring ? (size_t)nt : 0)) * sizeof(int) + base.size() * sizeof(long long) +
                 tasks.size() * sizeof(KrigeGramTask);
        hipError_t e = alloc_call_buffers(bufs, counts, 12);
        if (e == hipSuccess) e = dints.alloc(ints.size());
        if (e == hipSuccess) e = dfail.alloc(2);
        if (e == hipSuccess) e = dbase.alloc(base.size());
        if (e == hipSuccess && ring) e = dtoff.alloc((size_t)nt);
        if (e == hipSuccess && !tasks.empty()) e = dtasks.alloc(tasks.size());
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(-100 - (int)e, "%s: the device cannot hold the %zu bytes of the call (chunks of up to %zu rows, %d ring slots, "
                        "largest fold %d observations, n = %d): %s", who, bytes, rows_big, Wr, plan.bmax, n, hipGetErrorString(e));
        }
    }
    double *const tres = dtres, *const tvar = plan.bmax ? dtres + (size_t)plan.bmax * nr : nullptr;
    HIPCHK_AT(who, hipMemcpyAsync(dints, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK_AT(who, hipMemcpyAsync(dbase, base.data(), base.size() * sizeof(long long), hipMemcpyHostToDevice, s));
    if (!tasks.empty())
        HIPCHK_AT(who, hipMemcpyAsync(dtasks, tasks.data(), tasks.size() * sizeof(KrigeGramTask), hipMemcpyHostToDevice, s));
    if (!chunks.empty()) {
        HIPCHK_AT(who, hipMemcpyAsync(dtoff, bplan.toff.data(), (size_t)nt * sizeof(int), hipMemcpyHostToDevice, s));
        const std::vector<double> ones(ent_big, 1.0);
        HIPCHK_AT(who, hipMemcpyAsync(dones, ones.data(), ent_big * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK_AT(who, hipStreamSynchronize(s));            // (ones goes out of scope)
    }
    const int *d_idx = dints + at[0], *d_off = dints + at[1], *d_lab = dints + at[2], *d_sidx = dints + at[3], *d_slab = dints + at[4];
    const int st = run_op(f, who, [&]() -> int {
        HIPCHK(hipMemsetAsync(dfail, 0x7f, 2 * sizeof(int), s));
        // 1. U and the singletons: the selected inverse, as cocons_cv_taper
        if (int rc = taper_grad_enqueue(f, theta, mean, nullptr)) return rc;
        TaperGradState *G = f->tgrad.get();
        const double *U = G->AR;
        launch_cv_taper_list(G->Z, G->ldz, f->skew, npad, d_sidx, d_slab, (int)plan.single_idx.size(), U, (size_t)npad, nr, dvar, dres,
                             (size_t)npad, dfail, s);
        if (!chunks.empty()) {
            bool eng = f->engine_used, fol = f->follow_used;     // (a time-out of ANY factorisation of the call is repeated)
            // 2. the band factor once more (the sweep consumed it), into buffers of the call
            if (int rc = factor_on_band_schedule(f, theta, bplan, [&] { assemble_rhs(f, mean, true, nullptr, 0, 0, npad, true, false); }))
                return rc;
            eng = eng || f->engine_used; fol = fol || f->follow_used;
            launch_krige_band_pack(f->dA, f->lda, f->skew, npad, n, f->d_thi, nt, bplan.W, dtoff, dL, dQ, dw, s);
            launch_cv_info_take(f->dinfo, INFO_CLEAN, dfail + 1, nullptr, 0, s);
            for (const TfChunk &c : chunks) {
                // 3. the chunk's blocks: zero tiles for the packed folds, the bordered scratch of the large ones
                if (c.ntile > 0) HIPCHK(hipMemsetAsync(dblocks, 0, (size_t)c.ntile * TILE * TILE * sizeof(double), s));
                for (int g : c.large) {
                    const int b = plan.off[g + 1] - plan.off[g], bpad = round_up(b, TILE);
                    launch_cv_border(U, (size_t)npad, nr, d_idx + plan.off[g], b, bpad, rt, dblocks + base[g], 2 * (size_t)bpad + rt, s);
                }
                // 4. unit rows through the ring, K_BB = V V' group by group
                KrigeBandSolve a;
                a.Lp = dL; a.Qp = dQ; a.w = dw; a.toff = bplan.toff.data(); a.hi = envelope_or_null(f);
                a.nt = nt; a.W = bplan.W; a.ring = dring; a.ldr = (size_t)c.rows; a.rows = c.rows;
                a.boff = c.boff.data(); a.bdst = dints + c.at_dst; a.bsrc = dints + c.at_src; a.val = dones; a.tapv = dones;
                a.stoch = dst; a.quad = dq;
                a.Wr = Wr; a.depth = D; a.tasks = dtasks + c.at_task; a.ntasks = (int)c.tasks.size(); a.blocks = dblocks;
                HIPCHK(launch_krige_band_solve(a, s));
                // 5. the tails of cocons_cv_dense
                for (int k = 0; k < 4; ++k)
                    HIPCHK(launch_cv_folds_at(16 << k, dblocks, (size_t)TILE, dbase, U, (size_t)npad, nr, d_idx, d_off, dints + c.at_fl[k],
                                              d_lab, (int)c.flist[k].size(), dvar, dres, (size_t)npad, dfail, s));
                for (int g : c.large) {
                    const int b = plan.off[g + 1] - plan.off[g], bpad = round_up(b, TILE);
                    const size_t ldo = 2 * (size_t)bpad + (size_t)rt;
                    double *scratch = dblocks + base[g];
                    {
                        PlainSchedule plain(f);
                        FoldView fv(f);
                        FactorView v;
                        v.A = scratch; v.lda = ldo; v.nt = bpad / TILE; v.mt = (int)(ldo / TILE);
                        if (int rc = factorize(f, v, nullptr)) return rc;
                    }
                    eng = eng || f->engine_used; fol = fol || f->follow_used;
                    for (int k = 0; k < nr; ++k)
                        launch_row_reduce(scratch, ldo, b, bpad + k, bpad + rt, b, tres + (size_t)k * b, tvar, dred, s);
                    launch_cv_scatter(d_idx + plan.off[g], b, nr, tvar, tres, dvar, dres, (size_t)npad, s);
                    launch_cv_info_take(f->dinfo, INFO_CLEAN, nullptr, dfail, plan.lab[g], s);
                }
            }
            launch_cv_info_put(f->dinfo, dfail + 1, s);
            f->engine_used = eng; f->follow_used = fol;
        }
        HIPCHK(hipMemcpyAsync(hvar.data(), dvar, (size_t)npad * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hres.data(), dres, (size_t)npad * nr * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&hfail, dfail, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipGetLastError());
        return 0;
    });
    border_unknown(f);
    if (st) return st;                  // failing minor of S: nothing written
    if (hfail != INFO_CLEAN) return fail(-5, "%s: the hold-out block of S^-1 of fold %d is not positive definite", who, hfail);
    if (stats5) {
        stats5[0] = (long long)plan.single_idx.size(); stats5[1] = (long long)nsmall; stats5[2] = (long long)plan.large.size();
        stats5[3] = (long long)chunks.size(); stats5[4] = (long long)bytes;
    }
    for (int i = 0; i < n; ++i) {
        const size_t pos = (size_t)f->taper_inv[i];
        var[i] = hvar[pos];
        for (int k = 0; k < nr; ++k) resid[(size_t)i + (size_t)k * n] = hres[pos + (size_t)k * npad];
    }
    return 0;
}

