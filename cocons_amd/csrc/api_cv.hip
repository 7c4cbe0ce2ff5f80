// api_cv.hip -- C ABI, cross-validated predictions: cocons_cv_dense, cocons_cv_taper.
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

extern "C" int cocons_cv_taper(cocons_fit *f, const double *theta, const double *mean, double *resid, double *var)
{
    const char *who = "cocons_cv_taper";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !mean || !resid || !var) return fail(-1, "%s: null argument", who);
    FIT_ENTER(f);
    if (int rc = taper_refuse(f, who, "cocons_cv_dense")) return rc;
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
