// api_vecchia_cv.hip -- C ABI of U' and of cross-validation on a Vecchia fit: cocons_vecchia_transpose, the
// lists "which rows name me" of the handle's table; cocons_vecchia_whiten_t, U'W and diag(U'U) through them; cocons_cv_vecchia,
// leave-one-out and folds of up to 128 observations from Q = U'U, which is never formed:
//     r_B - E[r_B | r_A] = (Q_BB)^-1 (Q r)_B,      Cov(r_B | r_A) = (Q_BB)^-1.
// One cross-validation call is: the transposed lists unless the handle holds them, the coefficient launch of
// cocons_vecchia_unwhiten and its status word home -- a failing block ends the call there --, y = U R, U'y and diag(Q) for all
// observations, then the closed form for the observations alone in their fold and one workgroup per larger fold, which
// builds its Q_BB in LDS.  Device memory of a call: O(n (r + 1)), whatever the folds.
#include "fit.hpp"

namespace {

constexpr int INFO_CLEAN = 0x7f7f7f7f;

// Events around the four phases of the build (cocons_debug_vecchia_transpose_phases); off: nothing is created or recorded
struct BuildMarks {
    bool on;
    hipStream_t s;
    hipEvent_t ev[5] = {};
    BuildMarks(bool on_, hipStream_t s_) : on(on_), s(s_)
    {
        if (on) for (hipEvent_t &e : ev) (void)hipEventCreate(&e);
    }
    ~BuildMarks()
    {
        if (on) for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    void mark(int i) { if (on) (void)hipEventRecord(ev[i], s); }
    double ms(int i)
    {
        float t = 0.0f;
        if (on && hipEventElapsedTime(&t, ev[i], ev[i + 1]) != hipSuccess) { (void)hipGetLastError(); t = 0.0f; }
        return (double)t;
    }
};

// The transposed lists of the handle's table on the handle; ms4 (may be null): build them anew and time count, scan, fill
// and sort (the sort with the places) by events
int t_build(cocons_fit *f, const char *who, double *ms4)
{
    VecchiaState *V = f->vecchia.get();
    if (V->cv && V->cv->built && !ms4) return 0;
    const int n = f->n, m = V->m;
    if ((long long)n * m > (long long)INT_MAX)
        return fail(-1, "%s: a table of %d x %d entries is beyond the lists' 32-bit offsets", who, n, m);
    if (!V->cv) V->cv.reset(new VecchiaCvState());
    VecchiaCvState *T = V->cv.get();
    T->built = false;
    hipStream_t s = f->stream;
    const size_t cap = (size_t)n * m;
    const int nb = (n + VECCHIA_T_SCAN - 1) / VECCHIA_T_SCAN;
    // scratch of the build: the counts / cursors, the scan's workgroup totals, the four statistics, the columns of the two
    // longer classes (at most cap / 65 + 1 and cap / 4097 + 1 of them)
    const size_t nmid_max = cap / (VECCHIA_T_WAVE + 1) + 1, nbig_max = cap / (VECCHIA_T_LDS + 1) + 1;
    DevBuf<int> scratch;
    StreamDrain drain{s, false};
    HIPCHK_AT(who, T->ptr.reserve((size_t)n + 1, s, nullptr));
    HIPCHK_AT(who, scratch.alloc((size_t)n + nb + 4 + nmid_max + nbig_max));
    int *cnt = scratch, *bsum = cnt + n, *stat = bsum + nb, *mid = stat + 4, *big = mid + nmid_max;
    BuildMarks marks(ms4 != nullptr, s);
    HIPCHK_AT(who, hipMemsetAsync(cnt, 0, ((size_t)n + nb + 4) * sizeof(int), s));
    marks.mark(0);
    launch_vecchia_t_count(V->nbr, m, n, cnt, s);
    marks.mark(1);
    launch_vecchia_t_scan(cnt, n, T->ptr, bsum, stat, mid, big, s);
    marks.mark(2);
    int hstat[4] = {0, 0, 0, 0}, entries = 0;
    HIPCHK_AT(who, hipMemcpyAsync(hstat, stat, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipMemcpyAsync(&entries, T->ptr + n, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipGetLastError());
    HIPCHK_AT(who, hipStreamSynchronize(s));
    if (entries < 0 || (size_t)entries > cap || hstat[0] > n || (size_t)hstat[2] > nmid_max || (size_t)hstat[3] > nbig_max)
        return fail(-2, "%s: the lists hold %d entries, the longest %d (a table of %d x %d)", who, entries, hstat[0], n, m);
    HIPCHK_AT(who, T->rows.reserve(std::max<size_t>((size_t)entries, 1), s, nullptr, -1, true));
    HIPCHK_AT(who, T->place.reserve(std::max<size_t>((size_t)entries, 1), s, nullptr, -1, true));
    launch_vecchia_t_fill(V->nbr, m, n, T->ptr, cnt, T->rows, s);
    marks.mark(3);
    launch_vecchia_t_sort(n, T->ptr, T->rows, mid, hstat[2], big, hstat[3], s);
    launch_vecchia_t_place(V->nbr, m, n, T->ptr, T->rows, T->place, s);
    marks.mark(4);
    HIPCHK_AT(who, hipGetLastError());
    HIPCHK_AT(who, hipStreamSynchronize(s));
    T->entries = entries; T->longest = hstat[0]; T->unnamed = hstat[1];
    T->built = true;
    if (ms4) for (int i = 0; i < 4; ++i) ms4[i] = marks.ms(i);
    return 0;
}

VecchiaTArgs t_args(cocons_fit *f)
{
    VecchiaState *V = f->vecchia.get();
    VecchiaTArgs a;
    a.n = f->n; a.m = V->m; a.nbr = V->nbr;
    a.ptr = V->cv->ptr; a.rows = V->cv->rows; a.place = V->cv->place;
    a.coef = V->sim->coef;
    return a;
}

}  // namespace

int vecchia_t_build(cocons_fit *f, const char *who) { return t_build(f, who, nullptr); }
VecchiaTArgs vecchia_t_args(cocons_fit *f) { return t_args(f); }

extern "C" int cocons_vecchia_transpose(cocons_fit *f, int *ptr, int *rows, long long *out4)
{
    const char *who = "cocons_vecchia_transpose";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!out4) return fail(-1, "%s: null argument", who);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (int rc = t_build(f, who, nullptr)) return rc;
    VecchiaCvState *T = f->vecchia->cv.get();
    const size_t n = (size_t)f->n, ne = (size_t)T->entries;
    std::vector<int> hp(ptr ? n + 1 : 0), hr(rows ? ne : 0);
    if (ptr) HIPCHK_AT(who, hipMemcpy(hp.data(), T->ptr, hp.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (rows && ne) HIPCHK_AT(who, hipMemcpy(hr.data(), T->rows, hr.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (ptr) memcpy(ptr, hp.data(), hp.size() * sizeof(int));
    if (rows) for (size_t e = 0; e < ne; ++e) rows[e] = hr[e] + 1;
    out4[0] = T->entries; out4[1] = T->longest; out4[2] = T->bytes(); out4[3] = T->unnamed;
    return 0;
}

extern "C" int cocons_debug_vecchia_transpose_phases(cocons_fit *f, double *ms4)
{
    const char *who = "cocons_debug_vecchia_transpose_phases";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!ms4) return fail(-1, "%s: null argument", who);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    return t_build(f, who, ms4);
}

// cocons_vecchia_whiten_t and its grouped twin: the coefficient launch over observations or over the plan's blocks
int vecchia_whiten_t_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, int c, const double *W, double *out,
                          double *qdiag)
{
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !W || !out) return fail(-1, "%s: null argument", who);
    if (c < 1) return fail(-1, "%s: c = %d (at least one column expected)", who, c);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (grouped) if (int rc = vecchia_need_plan(f, who)) return rc;
    VecchiaState *V = f->vecchia.get();
    const size_t n = (size_t)f->n;
    hipStream_t s = f->stream;
    if (int rc = t_build(f, who, nullptr)) return rc;
    HIPCHK_AT(who, V->B.reserve(n * c, s, nullptr));
    HIPCHK_AT(who, V->W.reserve(n * (1 + c), s, nullptr));
    if (int st = vecchia_sim_coefs(f, who, theta, 0, grouped)) return st;
    HIPCHK_AT(who, upload_canon(V->B, W, n * c, s));
    launch_vecchia_ut(t_args(f), c, V->B, n, V->W + n, n, V->W, s);
    std::vector<double> h(n * (1 + c));
    HIPCHK_AT(who, hipMemcpyAsync(h.data(), V->W, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipGetLastError());
    HIPCHK_AT(who, hipStreamSynchronize(s));
    if (qdiag) memcpy(qdiag, h.data(), n * sizeof(double));
    memcpy(out, h.data() + n, n * c * sizeof(double));
    return 0;
}

extern "C" int cocons_vecchia_whiten_t(cocons_fit *f, const double *theta, int c, const double *W, double *out, double *qdiag)
{
    return vecchia_whiten_t_impl("cocons_vecchia_whiten_t", false, f, theta, c, W, out, qdiag);
}

// cocons_cv_vecchia and its grouped twin
int vecchia_cv_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, const double *mean, int nfold,
                    const int *fold, double *resid, double *var, long long *stats4)
{
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !mean || !resid || !var) return fail(-1, "%s: null argument", who);
    if (nfold < 0) return fail(-1, "%s: nfold = %d is negative", who, nfold);
    if ((fold == nullptr) != (nfold == 0))
        return fail(-1, "%s: fold and nfold disagree (fold = NULL with nfold = 0 is leave-one-out)", who);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (grouped) if (int rc = vecchia_need_plan(f, who)) return rc;
    VecchiaState *V = f->vecchia.get();
    const int n = f->n, nr = f->r;
    // ---- the folds (cocons_cv_dense's plan; a Vecchia handle keeps the caller's order, so positions are observations)
    std::vector<int> idx, off, lab, single_idx, single_lab, flist[4], inv;
    if (fold) {
        std::vector<int> cnt((size_t)nfold, 0);
        for (int i = 0; i < n; ++i) {
            if (fold[i] < 0 || fold[i] >= nfold)
                return fail(-1, "%s: label %d of observation %d is outside [0, %d)", who, fold[i], i, nfold);
            ++cnt[fold[i]];
        }
        std::vector<int> start((size_t)nfold, -1);
        off.push_back(0);
        for (int l = 0; l < nfold; ++l) {
            if (cnt[l] == n) return fail(-1, "%s: fold %d holds all %d observations", who, l, n);
            if (cnt[l] > CV_SMALL_MAX)
                return fail(-1, "%s: fold %d holds %d observations, more than the %d a hold-out block of U'U may have here; "
                                "for such a fold make a handle over the complement and predict with "
                                "cocons_vecchia_predict_knn", who, l, cnt[l], CV_SMALL_MAX);
            if (cnt[l] == 0) continue;
            start[l] = off.back();
            lab.push_back(l);
            off.push_back(off.back() + cnt[l]);
        }
        // ascending i fills every fold ascending
        idx.resize((size_t)n);
        inv.resize((size_t)n);
        for (int i = 0; i < n; ++i) { inv[i] = start[fold[i]]; idx[start[fold[i]]++] = i; }
        for (size_t g = 0; g + 1 < off.size(); ++g) {
            const int b = off[g + 1] - off[g];
            if (b == 1) { single_idx.push_back(idx[off[g]]); single_lab.push_back(lab[g]); }
            else flist[b <= 16 ? 0 : b <= 32 ? 1 : b <= 64 ? 2 : 3].push_back((int)g);
        }
    }
    hipStream_t s = f->stream;
    if (int rc = t_build(f, who, nullptr)) return rc;
    double hmean[COCONS_P_MAX];
    for (int i = 0; i < f->p; ++i) hmean[i] = canon_nan(mean[i]);
    HIPCHK_AT(who, V->B.reserve((size_t)n * nr, s, nullptr));
    // ---- the call's device memory: y = U R, U'y, diag(Q), the results, the plan
    DevBuf<double> dbuf;
    DevBuf<int> dints;
    StreamDrain drain{s, false};
    const size_t N = (size_t)n, ndbl = N * nr * 3 + 2 * N;
    std::vector<int> ints;
    size_t at[10] = {}, tot = 0;
    const std::vector<int> *parts[10] = {&idx, &off, &lab, &single_idx, &single_lab, &flist[0], &flist[1], &flist[2], &flist[3], &inv};
    for (int k = 0; k < 10; ++k) { at[k] = tot; tot += parts[k]->size(); }
    ints.resize(tot + 1);
    for (int k = 0; k < 10; ++k) std::copy(parts[k]->begin(), parts[k]->end(), ints.begin() + at[k]);
    ints[tot] = INFO_CLEAN;                                   // the failing fold's word
    if (hipError_t e = dbuf.alloc(ndbl)) {
        (void)hipGetLastError();
        return fail(-100 - (int)e, "%s: the device cannot hold the %zu bytes of this call: %s", who, ndbl * sizeof(double),
                    hipGetErrorString(e));
    }
    HIPCHK_AT(who, dints.alloc(tot + 1));
    double *dY = dbuf, *dUty = dY + N * nr, *dres = dUty + N * nr, *dq = dres + N * nr, *dvar = dq + N;
    int *dfail = dints + tot;
    if (int st = vecchia_sim_coefs(f, who, theta, 0, grouped)) return st; // a failing block: its row, nothing written
    HIPCHK_AT(who, hipMemcpyAsync(dints, ints.data(), (tot + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    const VecchiaTArgs ta = t_args(f);
    launch_vecchia_resid(n, f->p, f->dX, n, hmean, f->dz, n, 0, nr, V->B, N, s);
    launch_vecchia_umul(ta, nr, V->B, N, dY, N, s);
    launch_vecchia_ut(ta, nr, dY, N, dUty, N, dq, s);
    if (!fold) {
        launch_vecchia_cv_single(dq, dUty, N, nr, nullptr, nullptr, n, dvar, dres, N, dfail, s);
    } else {
        launch_vecchia_cv_single(dq, dUty, N, nr, dints + at[3], dints + at[4], (int)single_idx.size(), dvar, dres, N, dfail, s);
        for (int c = 0; c < 4; ++c)
            HIPCHK_AT(who, launch_vecchia_cv_folds(16 << c, ta, dints + at[9], dUty, N, nr, dints + at[0], dints + at[1],
                                                   dints + at[5 + c], dints + at[2], (int)flist[c].size(), dvar, dres, N, dfail, s));
    }
    std::vector<double> hvar(N), hres(N * nr);
    int hfail = INFO_CLEAN;
    HIPCHK_AT(who, hipMemcpyAsync(hvar.data(), dvar, N * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipMemcpyAsync(hres.data(), dres, N * nr * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipMemcpyAsync(&hfail, dfail, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipGetLastError());
    HIPCHK_AT(who, hipStreamSynchronize(s));
    if (hfail != INFO_CLEAN) {
        if (fold) return fail(-5, "%s: the hold-out block of U'U of fold %d is not positive definite", who, hfail);
        return fail(-5, "%s: the diagonal of U'U at observation %d (its own fold) is not positive", who, hfail);
    }
    memcpy(var, hvar.data(), N * sizeof(double));
    memcpy(resid, hres.data(), N * nr * sizeof(double));
    if (stats4) {
        size_t multi = 0;
        for (int c = 0; c < 4; ++c) multi += flist[c].size();
        stats4[0] = fold ? (long long)single_idx.size() : n;
        stats4[1] = (long long)multi;
        stats4[2] = V->cv->entries;
        stats4[3] = (long long)(ndbl * sizeof(double) + (tot + 1) * sizeof(int));
    }
    return 0;
}

extern "C" int cocons_cv_vecchia(cocons_fit *f, const double *theta, const double *mean, int nfold, const int *fold,
                                 double *resid, double *var, long long *stats4)
{
    return vecchia_cv_impl("cocons_cv_vecchia", false, f, theta, mean, nfold, fold, resid, var, stats4);
}
