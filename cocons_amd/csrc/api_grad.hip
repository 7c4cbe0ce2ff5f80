// api_grad.hip -- C ABI, derivatives: the analytic gradients of the dense, Profile, REML and tapered -2 log-likelihoods,
// the Fisher information, and the diagnostics that go with them.
#include "fit.hpp"

// ---------------------------------------------------------------------------
// Analytic gradient of the dense -2 log-likelihood.  One bordered factorisation of
//     [ Sigma ; R' ; I ]      (R = z - X mean, the residual rows in the first tile under the matrix, the unit rows behind it)
// on the plain schedules (dag_ok = false: the whole factor stays in dA) leaves L^-1 R and B = L^-T under the factor, by the
// trailing-update kernel itself.  Then the log-determinant and the quadratic forms (launch_finalize, as the objective),
// A = Sigma^-1 R = B L^-1 R, -Sigma^-1 = -B B' into the square the factor held (launch_grad_syrk), and the pair contraction
// (grad.hip).
// Memory: the bordered matrix needs rt + npad rows under the matrix.  It lives in the SAME allocation as every other
// operation's matrix -- dA grows once to hold it (one extra npad^2) -- with a leading dimension of its own for the duration
// of one gradient operation only (GradLayout).  f->lda, and with it the DAG schedule's second buffer (dag_prepare sizes dP
// from the view's lda), keeps the objective's value: a gradient call moves nothing else on the handle.
// leading dimension of the gradient's layout with nb rows (residuals, or Z' and Xb') in front of the unit rows; while nb <= 128
// it does not depend on nb
size_t grad_lda(const cocons_fit *f, int nb)
{
    return (size_t)f->npad + (size_t)round_up(nb > 0 ? nb : 1, TILE) + (size_t)f->npad;
}

// (GradLayout, fit.hpp: f->lda / f->rhs_act in this layout while one gradient operation runs)
static int grad_refuse(cocons_fit *f, const char *who)
{
    if (int rc = no_taper(f, who)) return rc;
    if (f->coll_kind) return fail(-1, "%s: not available on a sharded handle", who);
    return 0;
}

// The pair parameters of theta as every derivative reads them: the site factors beside loc_params_kernel's SoA go to `site`
// (launch_grad_site, on the handle's stream); returns the pair mode with its fixed values, and whether the smoothness is free.
// full_scale: the taper model's FULL scale vector (assemble_sigma_taper).
static std::pair<ModeSel, int> grad_site_params(cocons_fit *f, const double *theta, bool full_scale, double *site)
{
    ThetaVecs tv;
    make_theta_vecs(theta, f->p, tv, full_scale);
    const ModeSel ms = select_mode(theta, f->p, f->smooth_limits, 0);
    const int smooth_free = ms.smooth_kind == SMOOTH_LOGISTIC_SQRT && f->smooth_limits[1] != f->smooth_limits[0];
    launch_grad_site(loc_args(f->n, f->p, f->dX, f->dlocs, site, f->npad, tv, ms.smooth_kind, f->smooth_limits), site, f->npad,
                     smooth_free, f->stream);
    return {ms, smooth_free};
}

// everything the dense pair partials read, into g (the rest of it zero); the pair mode
static int grad_pair_args(cocons_fit *f, const double *theta, GradArgs &g)
{
    const int npad = f->npad, p = f->p;
    GradState *G = f->grad.get();
    const auto [ms, smooth_free] = grad_site_params(f, theta, false, G->site);
    memset(&g, 0, sizeof g);
    g.n = f->n; g.pad0 = f->pad0; g.npad = npad; g.p = p;
    g.S = f->dA; g.lds = f->lda;
    g.loc = f->dloc; g.stride = npad; g.site = G->site;
    g.X = f->dX; g.ldx = f->n;
    g.gr = ms.gr; g.nu_fixed = ms.nu_fixed; g.smooth_free = smooth_free;
    return ms.mode;
}

// the end of every gradient operation: -Sigma^-1 into the leading square (the unit rows, now L^-T, start rt rows under the
// matrix), then -- with hgrad -- the site factors and the contraction of W = coef Sigma^-1 - LR LR' (LR: npad x ncol) with
// dSigma/dtheta; the 7 p results (6 x p table, then the dense gradient's mean row) go to hgrad
static int grad_contract(cocons_fit *f, const double *theta, int rt, const double *LR, int ncol, double coef, double *hgrad)
{
    const int npad = f->npad, p = f->p;
    hipStream_t s = f->stream;
    GradState *G = f->grad.get();
    launch_grad_fill(f->dA, f->lda, 0, npad, npad, -1, s);
    launch_grad_syrk(f->dA, f->lda, npad, npad + rt, s);
    if (!hgrad) return 0;
    GradArgs g;
    const int mode = grad_pair_args(f, theta, g);
    g.AR = LR; g.ldar = npad; g.nr = ncol; g.coef = coef;
    const size_t T = (size_t)npad / 64, ntile = T * (T + 1) / 2;
    g.part_row = G->scratch; g.part_col = g.part_row + ntile * 6 * 64; g.part_glob = g.part_col + ntile * 6 * 64;
    g.gsite = g.part_glob + ntile;
    g.out = G->out;
    launch_grad_pairs(mode, g, s);
    HIPCHK(hipMemcpyAsync(hgrad, G->out, (size_t)7 * p * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipGetLastError());
    return 0;
}

// everything of one gradient operation on the handle's stream (run_op repeats it after a hand-off time-out); full = false
// stops once -Sigma^-1 is in the leading square (cocons_debug_sigma_inverse)
int grad_enqueue(cocons_fit *f, const double *theta, const double *mean, bool full, double *hgrad)
{
    const int npad = f->npad, nr = f->r, rt = round_up(nr > 0 ? nr : 1, TILE), p = f->p;
    hipStream_t s = f->stream;
    GradState *G = f->grad.get();
    f->nrhs_cur = nr;
    assemble_sigma(f, theta, 0, 0, npad);
    // rows npad.. : R' and zeros up to npad + rt; then the unit rows e_i', i < npad
    RhsArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.n = f->n; ra.p = p; ra.X = f->dX; ra.ldx = f->n; ra.use_trend = 1;
    for (int i = 0; i < p; ++i) ra.mean[i] = canon_nan(mean[i]);
    ra.src = f->dz ? f->dz : f->dX; ra.lds = f->n;
    ra.out = f->dA; ra.ld = f->lda; ra.row0 = npad; ra.nrows = nr; ra.nrows_zero = rt - nr;
    ra.col0 = 0; ra.ncols_out = npad;
    launch_rhs_rows(ra, s);
    launch_grad_fill(f->dA, f->lda, npad + rt, npad, npad, npad + rt, s);
    if (int rc = factorize(f, main_view(f), nullptr)) return rc;
    launch_finalize(f->dA, f->lda, f->n, npad, nr, f->dout, s);
    HIPCHK(hipMemcpyAsync(f->hout, f->dout, (size_t)(1 + nr * nr) * sizeof(double), hipMemcpyDeviceToHost, s));
    if (nr > 0) launch_grad_sigma_r(f->dA, f->lda, npad, npad, nr, npad + rt, G->ARpart, G->AR, s);
    return grad_contract(f, theta, rt, G->AR, nr, (double)nr, full ? hgrad : nullptr);
}

// The same operation for the Profile (reml = false, Xb = x_betas) and REML (Xb = x_covariates) objectives: the border is
// [Z' ; Xb'] without a trend (as the value entries' run_eval), its Gram matrix gives value and parts (profile_tail, on the
// host once the operation is complete) and, on the device, beta and chol(Xb' Sigma^-1 Xb); the contraction runs on
//     W = r Sigma^-1 - U U' [- r C C'],   U = Sigma^-1 (Z - Xb beta),  C = Sigma^-1 Xb chol(Xb' Sigma^-1 Xb)^-T.
static int profile_grad_enqueue(cocons_fit *f, const double *theta, const double *dxb, int nxb, bool reml, double *hgrad)
{
    const int npad = f->npad, r = f->r, nb = r + nxb, rt = round_up(nb, TILE), p = f->p;
    hipStream_t s = f->stream;
    GradState *G = f->grad.get();
    f->nrhs_cur = nb;
    assemble_sigma(f, theta, 0, 0, npad);
    RhsArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.n = f->n; ra.p = p; ra.X = f->dX; ra.ldx = f->n; ra.use_trend = 0;
    ra.src = f->dz; ra.lds = f->n;
    ra.out = f->dA; ra.ld = f->lda; ra.row0 = npad; ra.nrows = r; ra.nrows_zero = 0;
    ra.col0 = 0; ra.ncols_out = npad;
    launch_rhs_rows(ra, s);
    ra.src = dxb; ra.row0 = npad + r; ra.nrows = nxb; ra.nrows_zero = rt - nb;
    launch_rhs_rows(ra, s);
    launch_grad_fill(f->dA, f->lda, npad + rt, npad, npad, npad + rt, s);
    if (int rc = factorize(f, main_view(f), nullptr)) return rc;
    launch_finalize(f->dA, f->lda, f->n, npad, nb, f->dout, s);
    HIPCHK(hipMemcpyAsync(f->hout, f->dout, (size_t)(1 + nb * nb) * sizeof(double), hipMemcpyDeviceToHost, s));
    launch_grad_sigma_r(f->dA, f->lda, npad, npad, nb, npad + rt, G->SXpart, G->SX, s);
    launch_grad_lowrank(f->dout, G->SX, npad, r, nxb, reml ? 1 : 0, G->gls, G->LR, s);
    return grad_contract(f, theta, rt, G->LR, reml ? nb : r, (double)r, hgrad);
}

// nb: rows in front of the unit rows (the dense gradient's r); pcols > 0: the Profile / REML buffers for that many columns
int grad_prepare(cocons_fit *f, const char *who, int nb, int pcols)
{
    const int r1 = f->r > 0 ? f->r : 1;
    if (!f->grad) {
        std::unique_ptr<GradState> G(new GradState());
        const size_t sc = grad_scratch_doubles(f->npad), ar = (size_t)f->npad * r1, arp = grad_sigma_r_scratch_doubles(f->npad, r1),
                     si = (size_t)GSITE_FIELDS * f->npad, ou = (size_t)7 * f->p;
        HIPCHK_AT(who, G->scratch.alloc(sc));
        HIPCHK_AT(who, G->AR.alloc(ar));
        HIPCHK_AT(who, G->ARpart.alloc(arp));
        HIPCHK_AT(who, G->site.alloc(si));
        HIPCHK_AT(who, G->out.alloc(ou));
        G->bytes = (long long)((sc + ar + arp + si + ou) * sizeof(double));
        f->grad = std::move(G);
    }
    if (pcols > f->grad->pcols) {
        GradState *G = f->grad.get();
        const size_t sx = (size_t)f->npad * pcols, sxp = grad_sigma_r_scratch_doubles(f->npad, pcols),
                     gl = grad_gls_doubles(f->r, pcols - f->r);
        HIPCHK_AT(who, hipStreamSynchronize(f->stream));
        HIPCHK_AT(who, G->SX.alloc(sx));
        HIPCHK_AT(who, G->SXpart.alloc(sxp));
        HIPCHK_AT(who, G->LR.alloc(sx));
        HIPCHK_AT(who, G->gls.alloc(gl));
        G->bytes += (long long)((2 * sx + sxp + gl) * sizeof(double));
        G->pcols = pcols;
    }
    if (!f->dA) return fail(-1, "%s: the handle has no matrix buffer", who);
    // dA large enough for the gradient's layout: grown once, f->lda unchanged (GradLayout); the contents need not survive
    // (every operation assembles its matrix anew)
    const size_t need = grad_lda(f, nb) * (size_t)f->npad;
    bool grew = false;
    HIPCHK_AT(who, f->dA.reserve(need, f->stream, f->stream2, 0, false, &grew));
    if (grew) {
        HIPCHK_AT(who, hipStreamSynchronize(f->stream));
        border_unknown(f);
    }
    return 0;
}

extern "C" int cocons_neg2loglik_grad_dense(cocons_fit *f, const double *theta, const double *mean, double *sum_logliks,
                                            double *parts, double *grad_theta, double *grad_mean)
{
    const char *who = "cocons_neg2loglik_grad_dense";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !mean || !sum_logliks || !grad_theta || !grad_mean) return fail(-1, "%s: null argument", who);
    FIT_ENTER(f);
    if (int rc = grad_refuse(f, who)) return rc;
    if (f->r < 1) return fail(-1, "%s: fit has no z", who);
    if (int rc = grad_prepare(f, who, f->r)) return rc;
    std::vector<double> hg((size_t)7 * f->p);
    GradLayout layout(f, f->r);
    const int st = run_op(f, who, [&]() -> int { return grad_enqueue(f, theta, mean, true, hg.data()); });
    if (st) return st;                  // failing minor: nothing written
    dense_collect(f, sum_logliks, parts);
    memcpy(grad_theta, hg.data(), (size_t)6 * f->p * sizeof(double));
    memcpy(grad_mean, hg.data() + (size_t)6 * f->p, (size_t)f->p * sizeof(double));
    return 0;
}

// Profile / REML: value and parts from profile_tail (the value entries' own tail, on the Gram matrix of this operation's
// border), the 6 x p table from the contraction.  Nothing is written unless everything succeeded.
static int profile_grad_entry(cocons_fit *f, const char *who, const double *theta, const double *dxb, int nxb, double n_eff,
                              bool reml, double *sum_logliks, double *parts, double *grad_theta)
{
    const int nb = f->r + nxb;
    if (int rc = grad_prepare(f, who, nb, f->r + (f->q > f->p ? f->q : f->p))) return rc;
    std::vector<double> hg((size_t)7 * f->p), pt((size_t)2 + nb);
    double val = 0.0;
    GradLayout layout(f, nb);
    const int st = run_op(f, who, [&]() -> int { return profile_grad_enqueue(f, theta, dxb, nxb, reml, hg.data()); });
    if (st) return st;                  // failing minor: nothing written
    if (profile_tail(f, nxb, n_eff, reml, &val, pt.data()))
        return fail(-4, "%s: X' Sigma^-1 X is not positive definite", who);
    *sum_logliks = val;
    if (parts) memcpy(parts, pt.data(), pt.size() * sizeof(double));
    memcpy(grad_theta, hg.data(), (size_t)6 * f->p * sizeof(double));
    return 0;
}

extern "C" int cocons_neg2loglik_profile_grad(cocons_fit *f, const double *theta, double *sum_logliks, double *parts,
                                              double *grad_theta)
{
    const char *who = "cocons_neg2loglik_profile_grad";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !sum_logliks || !grad_theta) return fail(-1, "%s: null argument", who);
    FIT_ENTER(f);
    if (int rc = grad_refuse(f, who)) return rc;
    if (f->r < 1 || f->q < 1) return fail(-1, "%s: fit needs z and x_betas", who);
    return profile_grad_entry(f, who, theta, f->dxb, f->q, (double)f->n_user, false, sum_logliks, parts, grad_theta);
}

extern "C" int cocons_neg2loglik_reml_grad(cocons_fit *f, const double *theta, int rank, double *sum_logliks, double *parts,
                                           double *grad_theta)
{
    const char *who = "cocons_neg2loglik_reml_grad";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !sum_logliks || !grad_theta) return fail(-1, "%s: null argument", who);
    FIT_ENTER(f);
    if (int rc = grad_refuse(f, who)) return rc;
    if (f->r < 1) return fail(-1, "%s: fit has no z", who);
    return profile_grad_entry(f, who, theta, f->dX, f->p, (double)(f->n_user - rank), true, sum_logliks, parts, grad_theta);
}

extern "C" int cocons_debug_sigma_inverse(cocons_fit *f, const double *theta, double *out)
{
    const char *who = "cocons_debug_sigma_inverse";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !out) return fail(-1, "%s: null argument", who);
    FIT_ENTER(f);
    if (int rc = grad_refuse(f, who)) return rc;
    if (f->sorted) {
        // the caller's observation order: through the clone that keeps it (as cocons_sim_dense)
        if (!f->unsorted) {
            f->unsorted = fit_create_impl(f->n_user, f->p, f->r, 0, f->h_locs.data(), f->h_X.data(),
                                          f->r > 0 ? f->h_z.data() : nullptr, nullptr, f->smooth_limits,
                                          f->device, false);
            if (!f->unsorted) return -1;
        }
        return cocons_debug_sigma_inverse(f->unsorted, theta, out);
    }
    if (int rc = grad_prepare(f, who, f->r)) return rc;
    const std::vector<double> zero((size_t)f->p, 0.0);
    GradLayout layout(f, f->r);
    const int st = run_op(f, who, [&]() -> int { return grad_enqueue(f, theta, zero.data(), false, nullptr); });
    if (st) return st;
    const size_t n = (size_t)f->n_user;
    HIPCHK_AT(who, hipMemcpy2DAsync(out, n * sizeof(double), f->dA, f->lda * sizeof(double), n * sizeof(double), n,
                                    hipMemcpyDeviceToHost, f->stream));
    HIPCHK_AT(who, hipStreamSynchronize(f->stream));
    for (size_t j = 0; j < n; ++j)                  // the square holds -Sigma^-1 below its diagonal, zeros above
        for (size_t i = 0; i < n; ++i) out[i + j * n] = i >= j ? -out[i + j * n] : 0.0;
    return 0;
}

// ---------------------------------------------------------------------------
// Expected (Fisher) information of the dense model.  The gradient's bordered factorisation leaves -Sigma^-1 in
// the leading square (grad_enqueue, full = false); everything else lives in buffers of this call: one tall buffer of ndir + 2
// blocks of npad rows -- Sigma^-1 in full, the direction matrices Sigma_a, and the products, each of which lands in the block
// the product before it has consumed --, the site weights and the traces' per-tile partial sums.
// The information of the REML fit (cocons_fisher_reml) is the same operation on the REML gradient's border
// [Z' ; X' ; I] (profile_grad_enqueue without the contraction), with the projector P = Sigma^-1 - C C' put where Sigma^-1 was
// (launch_fisher_project) before the products run; it has no mean block.
struct FisherCall {
    DevBuf<double> tall, dirs, w, part, sxpart, sx, out;
    int ndir = 0;
    size_t ldt = 0;
    bool reml = false;
};

static int fisher_enqueue(cocons_fit *f, const double *theta, FisherCall &c, double *hinfo, double *hmean)
{
    const int npad = f->npad, p = f->p, ndir = c.ndir;
    hipStream_t s = f->stream;
    if (c.reml) {
        if (int rc = profile_grad_enqueue(f, theta, f->dX, p, true, nullptr)) return rc;
    } else {
        const std::vector<double> zero((size_t)p, 0.0);
        if (int rc = grad_enqueue(f, theta, zero.data(), false, nullptr)) return rc;
    }
    double *Tb = c.tall;
    launch_fisher_mirror(Tb, c.ldt, 0, f->dA, f->lda, 0, npad, 1, -1.0, s);
    if (c.reml)         // (LR = [U | sqrt(r) C]: the factor sqrt(r) of the gradient's block goes out again)
        launch_fisher_project(Tb, c.ldt, f->grad->LR + (size_t)f->r * npad, (size_t)npad, p, f->pad0, f->n, npad, 1.0 / f->r, s);
    GradArgs g;
    const int mode = grad_pair_args(f, theta, g);
    launch_fisher_dirs(mode, g, ndir, c.dirs, c.w, Tb + npad, c.ldt, (size_t)npad, s);
    HIPCHK(launch_fisher_products(Tb, c.ldt, npad, ndir, s));
    launch_fisher_trace(Tb + 2 * (size_t)npad, c.ldt, (size_t)npad, npad, ndir, 0.5 * f->r, c.part, c.out, s);
    HIPCHK(hipMemcpyAsync(hinfo, c.out, (size_t)ndir * ndir * sizeof(double), hipMemcpyDeviceToHost, s));
    if (hmean) {
        double *dmean = c.out + (size_t)ndir * ndir;
        launch_fisher_mean(Tb, c.ldt, f->n, f->pad0, npad, p, f->dX, f->n, (double)f->r, c.sxpart, c.sx, dmean, s);
        HIPCHK(hipMemcpyAsync(hmean, dmean, (size_t)p * p * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// the checks of the arguments that every information entry makes, in two parts: the pointers and the number of directions
// before the handle is entered, the directions' entries (ndir x 6 p, all finite) behind the handle's own checks
int fisher_check_args(const char *who, const cocons_fit *f, const double *theta, int ndir, const double *dirs, const double *info)
{
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !dirs || !info) return fail(-1, "%s: null argument", who);
    return ndir < 1 || ndir > 7 * COCONS_P_MAX ? fail(-1, "%s: ndir = %d is outside [1, %d]", who, ndir, 7 * COCONS_P_MAX) : 0;
}

int fisher_check_dirs(const char *who, int ndir, const double *dirs, int p)
{
    for (size_t e = 0; e < (size_t)ndir * 6 * p; ++e)
        if (!std::isfinite(dirs[e])) return fail(-1, "%s: direction %d has a non-finite entry", who, (int)(e / ((size_t)6 * p)));
    return 0;
}

// both entries; reml: the border is [Z' ; X' ; I] and info_mean is null
static int fisher_entry(cocons_fit *f, const char *who, const double *theta, int ndir, const double *dirs, double *info,
                        double *info_mean, bool reml)
{
    if (int rc = fisher_check_args(who, f, theta, ndir, dirs, info)) return rc;
    FIT_ENTER_AS(f, who);
    if (int rc = grad_refuse(f, who)) return rc;
    if (f->r < 1) return fail(-1, "%s: fit has no z", who);
    const int npad = f->npad, p = f->p, nb = reml ? f->r + p : f->r;
    const size_t nd = (size_t)ndir * 6 * p;
    if (int rc = fisher_check_dirs(who, ndir, dirs, p)) return rc;
    FisherCall c;
    c.ndir = ndir;
    c.ldt = (size_t)(ndir + 2) * npad;
    c.reml = reml;
    if (c.ldt * 64 * sizeof(double) > 0xffffffffull)       // (the product kernel's 32-bit byte offsets inside a tile)
        return fail(-1, "%s: %d directions of order %d are beyond the product kernel's addressing", who, ndir, npad);
    if (int rc = reml ? grad_prepare(f, who, nb, f->r + (f->q > p ? f->q : p)) : grad_prepare(f, who, nb)) return rc;
    const bool mean = info_mean != nullptr;
    const size_t counts[7] = {c.ldt * npad, nd, (size_t)ndir * 6 * npad, fisher_trace_scratch_doubles(npad, ndir),
                              reml ? 0 : grad_sigma_r_scratch_doubles(npad, p), reml ? 0 : (size_t)npad * p,
                              (size_t)ndir * ndir + (reml ? 0 : (size_t)p * p)};
    DevBuf<double> *bufs[7] = {&c.tall, &c.dirs, &c.w, &c.part, &c.sxpart, &c.sx, &c.out};
    size_t bytes = 0;
    for (size_t k : counts) bytes += k * sizeof(double);
    std::vector<double> hinfo((size_t)ndir * ndir), hmean((size_t)p * p);
    StreamDrain drain{f->stream, false};       // (declared behind the buffers: the stream is idle before they are freed)
    if (hipError_t e = alloc_call_buffers(bufs, counts, 7))
        return fail(-100 - (int)e, "%s: the device cannot hold the %zu bytes of this call (%d + 2 matrices of order %d): %s",
                    who, bytes, ndir, npad, hipGetErrorString(e));
    HIPCHK_AT(who, upload_canon(c.dirs, dirs, nd, f->stream));
    GradLayout layout(f, nb);
    const int st = run_op(f, who, [&]() -> int { return fisher_enqueue(f, theta, c, hinfo.data(), mean ? hmean.data() : nullptr); });
    if (st) return st;                  // failing minor: nothing written
    if (reml) {
        // a failing pivot of W leaves C all zero (launch_grad_lowrank) and the result the ML information: the same Gram matrix,
        // factored on the host in the device's order, says so (as the REML gradient's entry)
        double val = 0.0;
        if (profile_tail(f, p, 0.0, true, &val, nullptr)) return fail(-4, "%s: X' Sigma^-1 X is not positive definite", who);
        // n = p with W positive definite: no error contrasts, P = 0 and the information is the zero matrix -- in floating point
        // the projector keeps the rounding error of Sigma^-1 - C C', whose square (1e-32) would come back instead
        if (f->n_user <= p)
            for (double &x : hinfo) x = 0.0;
    }
    memcpy(info, hinfo.data(), hinfo.size() * sizeof(double));
    if (mean) memcpy(info_mean, hmean.data(), hmean.size() * sizeof(double));
    return 0;
}

extern "C" int cocons_fisher_dense(cocons_fit *f, const double *theta, int ndir, const double *dirs, double *info,
                                   double *info_mean)
{
    return fisher_entry(f, "cocons_fisher_dense", theta, ndir, dirs, info, info_mean, false);
}

extern "C" int cocons_fisher_reml(cocons_fit *f, const double *theta, int ndir, const double *dirs, double *info)
{
    return fisher_entry(f, "cocons_fisher_reml", theta, ndir, dirs, info, nullptr, true);
}

// out4 = { bytes allocated for the matrix buffer dA, bytes of the DAG schedule's second buffer dP, bytes of the gradient's
// scratch, the leading dimension the objective uses }
extern "C" int cocons_debug_fit_memory(cocons_fit *f, long long *out4)
{
    if (!f) return fail(-1, "cocons_debug_fit_memory: null fit handle");
    if (!out4) return fail(-1, "cocons_debug_fit_memory: null argument");
    FIT_ENTER(f);
    out4[0] = (long long)(f->dA.count() * sizeof(double));
    out4[1] = (long long)(f->dP.count() * sizeof(double));
    out4[2] = f->grad ? f->grad->bytes : 0;
    out4[3] = (long long)f->lda;
    return 0;
}

extern "C" int cocons_debug_matern_grad(int n, const double *nu, const double *u, double *out)
{
    if (n <= 0 || !nu || !u || !out) return fail(-1, "cocons_debug_matern_grad: bad argument");
    DevBuf<double> d;
    StreamDrain s{nullptr, true};
    HIPCHK_AT("cocons_debug_matern_grad", hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking));
    HIPCHK_AT("cocons_debug_matern_grad", d.alloc((size_t)5 * n));
    HIPCHK_AT("cocons_debug_matern_grad", upload_canon(d, nu, (size_t)n, s));
    HIPCHK_AT("cocons_debug_matern_grad", upload_canon(d + n, u, (size_t)n, s));
    launch_matern_grad_points(n, d, d + n, d + 2 * (size_t)n, s);
    HIPCHK_AT("cocons_debug_matern_grad", hipGetLastError());
    HIPCHK_AT("cocons_debug_matern_grad", hipMemcpyAsync(out, d + 2 * (size_t)n, (size_t)3 * n * sizeof(double),
                                                          hipMemcpyDeviceToHost, s));
    HIPCHK_AT("cocons_debug_matern_grad", hipStreamSynchronize(s));
    return 0;
}

// ---------------------------------------------------------------------------
// diagnostic: the device Matern correlation 2^(1-nu)/Gamma(nu) u^nu K_nu(u) at n points (host in/out)
extern "C" int cocons_debug_matern(int n, const double *nu, const double *u, double *out)
{
    if (n <= 0 || !nu || !u || !out) return fail(-1, "cocons_debug_matern: bad argument");
    DevBuf<double> d;
    StreamDrain s{nullptr, true};
    HIPCHK_AT("cocons_debug_matern", hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking));
    HIPCHK_AT("cocons_debug_matern", d.alloc((size_t)3 * n));
    HIPCHK_AT("cocons_debug_matern", upload_canon(d, nu, (size_t)n, s));
    HIPCHK_AT("cocons_debug_matern", upload_canon(d + n, u, (size_t)n, s));
    launch_matern_points(n, d, d + n, d + 2 * (size_t)n, s);
    HIPCHK_AT("cocons_debug_matern", hipGetLastError());
    HIPCHK_AT("cocons_debug_matern", hipMemcpyAsync(out, d + 2 * (size_t)n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK_AT("cocons_debug_matern", hipStreamSynchronize(s));
    return 0;
}

// ---------------------------------------------------------------------------
// Analytic gradient of the tapered -2 log-likelihood.  One operation: the objective's assembly and band
// factorisation with the residuals under the matrix, the log-determinant and quadratic forms (launch_finalize, as the
// objective), then the selected inverse on the tile envelope with the back-substitution A = L^-T (L^-1 R) in the same
// sweep (selinv.hip), and the contraction over the stored pattern (grad.hip).
int taper_grad_prepare(cocons_fit *f, const char *who)
{
    if (f->tgrad) return 0;
    std::unique_ptr<TaperGradState> G(new TaperGradState());
    const size_t npad = (size_t)f->npad, nnz = (size_t)f->taper_nnz, n = (size_t)f->n;
    G->ldz = f->skew > 0 ? (size_t)f->skew * TILE : npad;
    // transposed index of the device pattern: the lower triangle of the handle's pattern, numbered row by row as
    // taper_create_ordered filters it; column j's entries in ascending row order
    std::vector<int> tcp(n + 1, 0), tidx(nnz), trow(nnz);
    {
        const std::vector<int> &rp = f->h_trp, &ci = f->h_tci;
        if (rp.size() != n + 1) return fail(-1, "%s: the handle keeps no host copy of its pattern", who);
        size_t cnt = 0;
        for (size_t i = 0; i < n; ++i)
            for (int w = rp[i] - 1; w < rp[i + 1] - 1; ++w)
                if (ci[w] - 1 <= (int)i) { ++tcp[ci[w]]; ++cnt; }
        if (cnt != nnz) return fail(-1, "%s: the host copy of the pattern does not match the device's", who);
        for (size_t j = 0; j < n; ++j) tcp[j + 1] += tcp[j];
        std::vector<int> fill(tcp.begin(), tcp.end() - 1);
        int w2 = 0;
        for (size_t i = 0; i < n; ++i)
            for (int w = rp[i] - 1; w < rp[i + 1] - 1; ++w)
                if (ci[w] - 1 <= (int)i) {
                    const int t = fill[ci[w] - 1]++;
                    tidx[t] = w2++; trow[t] = (int)i;
                }
    }
    const size_t zc = G->ldz * npad, ar = npad * (size_t)f->r, en = 6 * nnz, si = (size_t)GSITE_FIELDS * npad, gs = 9 * npad,
                 ou = (size_t)9 * f->p;
    HIPCHK_AT(who, G->Z.alloc(zc));
    HIPCHK_AT(who, G->AR.alloc(ar));
    HIPCHK_AT(who, G->ent.alloc(en));
    HIPCHK_AT(who, G->site.alloc(si));
    HIPCHK_AT(who, G->gsite.alloc(gs));
    HIPCHK_AT(who, G->out.alloc(ou));
    HIPCHK_AT(who, G->tcp.alloc(n + 1));
    HIPCHK_AT(who, G->tidx.alloc(nnz));
    HIPCHK_AT(who, G->trow.alloc(nnz));
    HIPCHK_AT(who, hipMemcpyAsync(G->tcp, tcp.data(), (n + 1) * sizeof(int), hipMemcpyHostToDevice, f->stream));
    HIPCHK_AT(who, hipMemcpyAsync(G->tidx, tidx.data(), nnz * sizeof(int), hipMemcpyHostToDevice, f->stream));
    HIPCHK_AT(who, hipMemcpyAsync(G->trow, trow.data(), nnz * sizeof(int), hipMemcpyHostToDevice, f->stream));
    // (the padding rows of A and of the site sums are read by nothing, the envelope tiles of Z are written before they are
    // read; cleared once all the same, so that no never-written byte is ever a NaN pattern)
    HIPCHK_AT(who, hipMemsetAsync(G->Z, 0, zc * sizeof(double), f->stream));
    HIPCHK_AT(who, hipMemsetAsync(G->AR, 0, ar * sizeof(double), f->stream));
    HIPCHK_AT(who, hipMemsetAsync(G->gsite, 0, gs * sizeof(double), f->stream));
    HIPCHK_AT(who, hipStreamSynchronize(f->stream));      // the staging vectors go out of scope
    G->bytes = (long long)((zc + ar + en + si + gs + ou) * sizeof(double) + (n + 1 + 2 * nnz) * sizeof(int));
    f->tgrad = std::move(G);
    return 0;
}

// everything of one operation on the handle's stream (run_op repeats it after a hand-off time-out); hgrad = null stops once
// Z = S^-1 is complete (cocons_debug_taper_selinv)
int taper_grad_enqueue(cocons_fit *f, const double *theta, const double *mean, double *hgrad)
{
    const int npad = f->npad, nr = f->r, p = f->p;
    hipStream_t s = f->stream;
    TaperGradState *G = f->tgrad.get();
    f->nrhs_cur = nr;
    if (int rc = fit_alloc_matrix(f, nr)) return rc;
    if (int rc = assemble_sigma_taper(f, theta)) return rc;
    assemble_rhs(f, mean, true, nullptr, 0, 0, npad, true, false);
    if (int rc = factorize(f, main_view(f), nullptr)) return rc;      // (dag_ok = false: the whole factor stays in dA)
    launch_finalize(f->dA, f->lda, f->n, npad, nr, f->dout, s, f->skew, npad);
    HIPCHK(hipMemcpyAsync(f->hout, f->dout, (size_t)(1 + nr * nr) * sizeof(double), hipMemcpyDeviceToHost, s));
    SelinvArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.L = f->dA; sa.ldl = f->lda; sa.Z = G->Z; sa.ldz = G->ldz;
    sa.skew = f->skew; sa.npad = npad; sa.nt = f->nt;
    sa.d_hi = f->d_thi; sa.nr = nr; sa.AR = G->AR;
    launch_selinv(sa, envelope_or_null(f), band_W(f), s);
    HIPCHK(hipGetLastError());
    if (!hgrad) return 0;
    const auto [ms, smooth_free] = grad_site_params(f, theta, true, G->site);
    TaperGradArgs g;
    memset(&g, 0, sizeof g);
    g.n = f->n; g.npad = npad; g.p = p; g.nnz = f->taper_nnz; g.nr = nr;
    g.ci = f->d_tci; g.rp = f->d_trp; g.tcp = G->tcp; g.tidx = G->tidx; g.trow = G->trow; g.tapv = f->d_tval;
    g.Z = G->Z; g.ldz = G->ldz; g.skew = f->skew;
    g.AR = G->AR; g.coef = (double)nr;
    g.loc = f->dloc; g.stride = npad; g.site = G->site;
    g.X = f->dX; g.ldx = f->n;
    g.nu_fixed = ms.nu_fixed; g.smooth_free = smooth_free;
    g.ent = G->ent; g.gsite = G->gsite; g.out = G->out;
    launch_taper_grad(ms.mode, g, s);
    HIPCHK(hipMemcpyAsync(hgrad, G->out, (size_t)9 * p * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipGetLastError());
    return 0;
}

// what every entry of the tapered fit beside the objective asks of its handle; dense_entry: who serves a dense handle instead
int taper_refuse(cocons_fit *f, const char *who, const char *dense_entry)
{
    if (f->taper_nnz <= 0) return fail(-1, "%s: not a taper fit (%s serves a dense handle)", who, dense_entry);
    if (f->coll_kind) return fail(-1, "%s: not available on a sharded handle", who);
    if (f->r < 1) return fail(-1, "%s: fit has no z", who);
    return 0;
}

extern "C" int cocons_neg2loglik_grad_taper(cocons_fit *f, const double *theta, const double *mean, double *sum_logliks,
                                            double *parts, double *grad_theta, double *grad_quad, double *grad_mean)
{
    const char *who = "cocons_neg2loglik_grad_taper";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !mean || !sum_logliks || !grad_theta || !grad_mean) return fail(-1, "%s: null argument", who);
    FIT_ENTER(f);
    if (int rc = taper_refuse(f, who, "cocons_neg2loglik_grad_dense")) return rc;
    if (int rc = taper_grad_prepare(f, who)) return rc;
    const int p = f->p;
    std::vector<double> hg((size_t)9 * p);
    const int st = run_op(f, who, [&]() -> int { return taper_grad_enqueue(f, theta, mean, hg.data()); });
    border_unknown(f);
    if (st) return st;                  // failing minor: nothing written
    dense_collect(f, sum_logliks, parts);
    // device rows: part (log-determinant, quadratic form) x family (std.dev, scale, smooth, nugget); aniso and tilt do not
    // enter the taper model: exactly zero
    static const int fam_row[4] = {TH_SD, TH_SCALE, TH_SMOOTH, TH_NUGGET};
    for (int e = 0; e < 6 * p; ++e) { grad_theta[e] = 0.0; if (grad_quad) grad_quad[e] = 0.0; }
    for (int fm = 0; fm < 4; ++fm)
        for (int k = 0; k < p; ++k) {
            const double ld = hg[(size_t)fm * p + k], qd = hg[(size_t)(4 + fm) * p + k];
            grad_theta[fam_row[fm] * p + k] = ld + qd;
            if (grad_quad) grad_quad[fam_row[fm] * p + k] = qd;
        }
    memcpy(grad_mean, hg.data() + (size_t)8 * p, (size_t)p * sizeof(double));
    return 0;
}

// (diagnostics) (S^-1)_ij at every stored entry of the pattern the handle was created with, in the caller's CSR order
// (out_nnz: as many doubles as that pattern has entries), by the gradient's selected inverse; bytes_out (may be null): the
// device bytes the gradient holds on the handle
extern "C" int cocons_debug_taper_selinv(cocons_fit *f, const double *theta, double *out_nnz, long long *bytes_out)
{
    const char *who = "cocons_debug_taper_selinv";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!theta || !out_nnz) return fail(-1, "%s: null argument", who);
    FIT_ENTER(f);
    if (int rc = taper_refuse(f, who, "cocons_neg2loglik_grad_dense")) return rc;
    if (int rc = taper_grad_prepare(f, who)) return rc;
    const std::vector<double> zero((size_t)f->p, 0.0);
    const int st = run_op(f, who, [&]() -> int { return taper_grad_enqueue(f, theta, zero.data(), nullptr); });
    border_unknown(f);
    if (st) return st;
    // the caller's entry w of row o is the entry at the same place of row taper_inv[o] of the handle's pattern
    const int n = f->n;
    const size_t full = f->h_tci.size();
    std::vector<int> ij(2 * full);
    size_t w = 0;
    for (int o = 0; o < n; ++o) {
        const int i = f->taper_inv[o];
        for (int t = f->h_trp[i] - 1; t < f->h_trp[i + 1] - 1; ++t, ++w) { ij[2 * w] = i; ij[2 * w + 1] = f->h_tci[t] - 1; }
    }
    DevBuf<int> dij;
    DevBuf<double> dv;
    HIPCHK_AT(who, dij.alloc(2 * full));
    HIPCHK_AT(who, dv.alloc(full));
    HIPCHK_AT(who, hipMemcpyAsync(dij, ij.data(), 2 * full * sizeof(int), hipMemcpyHostToDevice, f->stream));
    launch_selinv_gather(f->tgrad->Z, f->tgrad->ldz, f->skew, f->npad, dij, full, dv, f->stream);
    HIPCHK_AT(who, hipGetLastError());
    HIPCHK_AT(who, hipMemcpyAsync(out_nnz, dv, full * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    HIPCHK_AT(who, hipStreamSynchronize(f->stream));
    if (bytes_out) *bytes_out = f->tgrad->bytes;
    return 0;
}

// ---------------------------------------------------------------------------
// Expected (Fisher) information of a tapered fit on the band factor.  With S = T o C(theta) = L L' and
// M_a = L^-1 S_a L^-T,  tr(S^-1 S_a S^-1 S_b) = <M_a, M_b>_F, and for probe rows e_k with sum_k e_k e_k' = c I
//     sum_k (e_k' L^-1 S_a L^-T) . (e_k' L^-1 S_b L^-T) = c <M_a, M_b>_F:
// the n unit vectors give it exactly, N random +-1 probes give Hutchinson's estimate.  One operation: the objective's assembly
// and band factorisation (as cocons_krige_taper_prepare runs it: the same bits under every buffer layout), the factor packed
// twice into buffers of the call -- its own tiles for the forward sweep, the flipped transpose for the backward one --, the
// directions' entries on the pattern, then per chunk of probe rows: backward sweep, sparse product, forward sweep of every
// direction's rows at once (with X' riding in the first chunk for the mean block), Gram partial sums per 64-row strip.
// Nothing of it stays on the handle; the kriging and gradient states are neither read nor written.
static constexpr size_t FISHER_TAPER_CHUNK_BYTES = (size_t)1 << 30;
static constexpr int FISHER_TAPER_ROWS_CAP = 16384;

struct FisherTaperCall {
    DevBuf<double> Lp, Qp, Mp, Qb, E, U, Sd, wsite, site, dirs, zero, st, qd, seg, part, partm, out;
    DevBuf<int> itab, pat, pos;        // itab: the plan's toff | toffb | hib (nt each); pat: frp (n + 1) | fci | fidx (full nnz each)
    BandPlan plan;                     // the envelope, its mirror and the packed tiles' offsets of both (band_plan.hpp)
    size_t fnnz = 0;
    int ndir = 0, nprobe = 0, c = 0, total = 0;
};

static int fisher_taper_enqueue(cocons_fit *f, const double *theta, FisherTaperCall &c, const double *probes, double *hinfo,
                                double *hmean)
{
    const int npad = f->npad, n = f->n, p = f->p, nt = f->nt, ndir = c.ndir;
    hipStream_t s = f->stream;
    const std::vector<double> zero((size_t)p, 0.0);
    // 1. the factor
    f->nrhs_cur = f->r;
    if (int rc = fit_alloc_matrix(f, f->r)) return rc;
    if (int rc = factor_on_band_schedule(f, theta, c.plan, [&] { assemble_rhs(f, zero.data(), true, nullptr, 0, 0, npad, true, false); }))
        return rc;
    const int *d_toff = c.itab, *d_toffb = c.itab + nt, *d_hib = c.itab + 2 * (size_t)nt;
    launch_krige_band_pack(f->dA, f->lda, f->skew, npad, n, f->d_thi, nt, c.plan.W, d_toff, c.Lp, c.Qp, c.st /* w: nobody reads it */, s);
    launch_band_back_pack(f->dA, f->lda, f->skew, npad, d_hib, nt, c.plan.W, d_toffb, c.Mp, c.Qb, s);
    // 2. the directions' entries
    const auto [ms, smooth_free] = grad_site_params(f, theta, true, c.site);
    TaperDirsArgs d;
    memset(&d, 0, sizeof d);
    d.g.n = n; d.g.npad = npad; d.g.p = p; d.g.nnz = f->taper_nnz;
    d.g.ci = f->d_tci; d.g.rp = f->d_trp; d.g.tapv = f->d_tval;
    d.g.loc = f->dloc; d.g.stride = npad; d.g.site = c.site;
    d.g.X = f->dX; d.g.ldx = n;
    d.g.nu_fixed = ms.nu_fixed; d.g.smooth_free = smooth_free;
    d.ndir = ndir; d.dirs = c.dirs; d.wsite = c.wsite; d.out = c.Sd;
    launch_taper_dirs(ms.mode, d, s);
    HIPCHK(hipGetLastError());
    // 3 - 6. the chunks
    const size_t ldu = (size_t)ndir * c.c + 64;
    const int *frp = c.pat, *fci = c.pat + (n + 1), *fidx = fci + c.fnnz;
    int strip0 = 0;
    for (int g0 = 0; g0 < c.total; g0 += c.c) {
        const int cc = std::min(c.c, c.total - g0), cs = round_up(cc, 64), nstrips = cs / 64;
        const bool first = g0 == 0;
        HIPCHK(hipMemsetAsync(c.E, 0, (size_t)c.c * npad * sizeof(double), s));
        if (c.nprobe > 0) {
            // the chunk's probes are staged in U, which the sparse product overwrites afterwards
            HIPCHK(upload_canon(c.U, probes + (size_t)g0 * n, (size_t)cc * n, s));
            launch_band_given_rows(c.E, (size_t)c.c, npad, c.U, n, c.pos, cc, s);
        } else launch_band_unit_rows(c.E, (size_t)c.c, npad, g0, cc, s);
        BandSweep b;
        b.Lp = c.Mp; b.Qp = c.Qb; b.toff = c.plan.toffb.data(); b.hi = c.plan.hib.data(); b.nt = nt;
        b.C = c.E; b.ldc = (size_t)c.c; b.rows = cs; b.zero = c.zero; b.st = c.st; b.qd = c.qd;
        HIPCHK(launch_band_back_solve(b, s));
        BandSpmm m;
        m.Wf = c.E; m.ldw = (size_t)c.c; m.rows = cs; m.n = n; m.npad = npad; m.ndir = ndir;
        m.frp = frp; m.fci = fci; m.fidx = fidx; m.Sd = c.Sd; m.nnz = (size_t)f->taper_nnz;
        m.U = c.U; m.ldu = ldu; m.bstride = (size_t)cs;
        launch_band_spmm_dirs(m, s);
        const int urows = ndir * cs + (first && hmean ? 64 : 0);
        if (first && hmean) launch_band_x_rows(c.U, ldu, ndir * cs, f->dX, n, p, npad, s);
        BandSweep q;
        q.Lp = c.Lp; q.Qp = c.Qp; q.toff = c.plan.toff.data(); q.hi = c.plan.hi.data(); q.nt = nt;
        q.C = c.U; q.ldc = ldu; q.rows = urows; q.zero = c.zero; q.st = c.st; q.qd = c.qd;
        HIPCHK(launch_band_sweep(q, s));
        launch_band_gram(c.U, ldu, 0, (size_t)cs, 64, nstrips, npad, ndir, c.seg, c.part, strip0, s);
        if (first && hmean) launch_band_gram(c.U, ldu, (size_t)ndir * cs, 1, 1, 1, npad, p, c.seg, c.partm, 0, s);
        strip0 += nstrips;
    }
    const double weight = c.nprobe > 0 ? 0.5 * f->r / c.nprobe : 0.5 * f->r;
    launch_band_gram_sum(c.part, strip0, ndir, weight, c.out, s);
    HIPCHK(hipMemcpyAsync(hinfo, c.out, (size_t)ndir * ndir * sizeof(double), hipMemcpyDeviceToHost, s));
    if (hmean) {
        double *dmean = c.out + (size_t)ndir * ndir;
        launch_band_gram_sum(c.partm, 1, p, (double)f->r, dmean, s);
        HIPCHK(hipMemcpyAsync(hmean, dmean, (size_t)p * p * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int cocons_fisher_taper(cocons_fit *f, const double *theta, int ndir, const double *dirs, int nprobe,
                                   const double *probes, int max_rows, double *info, double *info_mean)
{
    const char *who = "cocons_fisher_taper";
    if (int rc = fisher_check_args(who, f, theta, ndir, dirs, info)) return rc;
    if (nprobe < 0) return fail(-1, "%s: nprobe = %d is negative", who, nprobe);
    if (nprobe > 0 && !probes) return fail(-1, "%s: nprobe = %d without probes", who, nprobe);
    if (nprobe == 0 && probes) return fail(-1, "%s: probes given with nprobe = 0 (exact mode takes none)", who);
    if (max_rows < 0) return fail(-1, "%s: max_rows = %d is negative", who, max_rows);
    FIT_ENTER(f);
    if (int rc = taper_refuse(f, who, "cocons_fisher_dense")) return rc;
    const int npad = f->npad, n = f->n, p = f->p, nt = f->nt;
    const size_t nd = (size_t)ndir * 6 * p;
    if (int rc = fisher_check_dirs(who, ndir, dirs, p)) return rc;
    for (size_t e = 0; e < (size_t)nprobe * n; ++e)
        if (!std::isfinite(probes[e])) return fail(-1, "%s: probe %d has a non-finite entry", who, (int)(e / (size_t)n));
    FisherTaperCall c;
    c.ndir = ndir; c.nprobe = nprobe; c.total = nprobe > 0 ? nprobe : n;
    {
        size_t rows = std::min<size_t>(FISHER_TAPER_CHUNK_BYTES / ((size_t)(ndir + 1) * npad * sizeof(double)), FISHER_TAPER_ROWS_CAP);
        rows = std::max<size_t>(rows / 64 * 64, 64);
        if (max_rows > 0) rows = std::min<size_t>(rows, std::max<size_t>((size_t)max_rows / 64 * 64, 64));
        c.c = (int)std::min<size_t>(rows, (size_t)round_up(c.total, 64));
    }
    if (const char *why = band_plan(nt, envelope_or_null(f), f->taper_maxband, c.plan)) return fail(-1, "%s: %s", who, why);
    // the full symmetric pattern in the handle's order (0-based) and, per entry, the index of (max, min) among the lower
    // entries as the device pattern numbers them (row by row)
    const std::vector<int> &rp = f->h_trp, &ci = f->h_tci;
    if (rp.size() != (size_t)n + 1) return fail(-1, "%s: the handle keeps no host copy of its pattern", who);
    c.fnnz = ci.size();
    std::vector<int> pat((size_t)n + 1 + 2 * c.fnnz);
    {
        int *frp = pat.data(), *fci = frp + (n + 1), *fidx = fci + c.fnnz;
        std::vector<int> cur((size_t)n);
        for (int i = 0; i < n; ++i) { frp[i] = rp[i] - 1; cur[i] = rp[i] - 1; }
        frp[n] = rp[n] - 1;
        int low = 0;
        for (int i = 0; i < n; ++i)
            for (int t = frp[i]; t < frp[i + 1]; ++t) {
                fci[t] = ci[t] - 1;
                if (fci[t] <= i) fidx[t] = low++;
            }
        if (low != f->taper_nnz) return fail(-1, "%s: the host copy of the pattern does not match the device's", who);
        // the upper entry (j, i), i > j, is the lower entry (i, j): row i's entries in ascending column order meet the rows j
        // in ascending order, so one cursor per row finds them
        for (int j = 0; j < n; ++j)
            for (int t = frp[j]; t < frp[j + 1]; ++t) {
                const int i = fci[t];
                if (i <= j) continue;
                int u = cur[i];
                if (u >= frp[i + 1] || fci[u] != j) {
                    for (u = frp[i]; u < frp[i + 1] && fci[u] != j; ++u) {}
                    if (u >= frp[i + 1]) return fail(-1, "%s: the handle's pattern is not symmetric", who);
                } else cur[i] = u + 1;
                fidx[t] = fidx[u];
            }
    }
    const size_t ntile = (size_t)c.plan.toff[nt], ldu = (size_t)ndir * c.c + 64, nnz = (size_t)f->taper_nnz;
    const int total_strips = (c.total / c.c) * (c.c / 64) + (round_up(c.total % c.c, 64)) / 64;
    const bool mean = info_mean != nullptr;
    const size_t counts[17] = {ntile * TILE * TILE, (size_t)nt * 2048, ntile * TILE * TILE, (size_t)nt * 2048, (size_t)c.c * npad, ldu * npad,
                               (size_t)ndir * nnz, (size_t)ndir * 4 * npad, (size_t)GSITE_FIELDS * npad, nd, (size_t)npad,
                               std::max<size_t>(ldu, (size_t)npad), ldu,
                               std::max(band_gram_scratch_doubles(c.c / 64, npad, ndir), band_gram_scratch_doubles(1, npad, p)),
                               (size_t)total_strips * ndir * ndir, (size_t)p * p, (size_t)ndir * ndir + (size_t)p * p};
    DevBuf<double> *bufs[17] = {&c.Lp, &c.Qp, &c.Mp, &c.Qb, &c.E, &c.U, &c.Sd, &c.wsite, &c.site, &c.dirs, &c.zero, &c.st, &c.qd,
                                &c.seg, &c.part, &c.partm, &c.out};
    size_t bytes = (3 * (size_t)nt + pat.size() + (size_t)n) * sizeof(int);
    for (size_t k : counts) bytes += k * sizeof(double);
    std::vector<double> hinfo((size_t)ndir * ndir), hmean((size_t)p * p);
    StreamDrain drain{f->stream, false};       // (declared behind the buffers: the stream is idle before they are freed)
    hipError_t e = alloc_call_buffers(bufs, counts, 17);
    if (e == hipSuccess) e = c.itab.alloc(3 * (size_t)nt);
    if (e == hipSuccess) e = c.pat.alloc(pat.size());
    if (e == hipSuccess) e = c.pos.alloc((size_t)n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(-100 - (int)e, "%s: the device cannot hold the %zu bytes of this call (%d directions, chunks of %d rows of %d): %s",
                    who, bytes, ndir, c.c, npad, hipGetErrorString(e));
    }
    hipStream_t s = f->stream;
    HIPCHK_AT(who, upload_canon(c.dirs, dirs, nd, s));
    HIPCHK_AT(who, hipMemsetAsync(c.zero, 0, (size_t)npad * sizeof(double), s));
    HIPCHK_AT(who, hipMemcpyAsync(c.itab, c.plan.toff.data(), (size_t)nt * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK_AT(who, hipMemcpyAsync(c.itab + nt, c.plan.toffb.data(), (size_t)nt * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK_AT(who, hipMemcpyAsync(c.itab + 2 * (size_t)nt, c.plan.hib.data(), (size_t)nt * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK_AT(who, hipMemcpyAsync(c.pat, pat.data(), pat.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK_AT(who, hipMemcpyAsync(c.pos, f->taper_inv.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    const int st = run_op(f, who, [&]() -> int {
        return fisher_taper_enqueue(f, theta, c, probes, hinfo.data(), mean ? hmean.data() : nullptr);
    });
    border_unknown(f);
    if (st) return st;                  // failing minor: nothing written
    memcpy(info, hinfo.data(), hinfo.size() * sizeof(double));
    if (mean) memcpy(info_mean, hmean.data(), hmean.size() * sizeof(double));
    return 0;
}
