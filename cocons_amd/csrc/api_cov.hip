// api_cov.hip -- C ABI, the one-shot covariance entries: cocons_cov_rns and its classic, prediction and taper variants,
// cocons_cov_rows, and the host-only cocons_sumsmoothlone.  They allocate their own buffers (cocons_cov_rows borrows the
// handle's stream and host copies) and never factor anything.
#include "fit.hpp"

// src/cocons_full.cpp:12-30 -- O(p) host arithmetic, kept on the host.
extern "C" double cocons_sumsmoothlone(const double *x, int len, double lambda, double alpha)
{
    double sum = 0;
    for (int w = 0; w < len; ++w) {
        if (std::abs(x[w]) > 1e-4)
            sum = sum + std::abs(x[w]);
        else
            sum = sum + std::pow(alpha, -1) * (std::log(1 + std::exp(-alpha * x[w])) + std::log(1 + std::exp(alpha * x[w])));
    }
    return lambda * sum;
}

// ---------------------------------------------------------------------------
// stateless covariance entry points
static int cov_common(int which, int n, int m, int p, const double *theta, const double *locs,
                      const double *locs_pred, const double *X, const double *X_pred,
                      const double *smooth_limits, double *out)
{
    if (n <= 0 || p <= 0 || p > COCONS_P_MAX || !theta || !locs || !X || !out || (which != 1 && !smooth_limits) ||
        (which == 2 && (m <= 0 || !locs_pred || !X_pred)))
        return fail(-1, "cov_rns*: bad argument");
    double sl_dummy[2] = {0.0, 0.0};
    const double *sl = smooth_limits ? smooth_limits : sl_dummy;
    ThetaVecs tv;
    make_theta_vecs(theta, p, tv);
    ModeSel ms = select_mode(theta, p, sl, which);
    const size_t rows = which == 2 ? (size_t)m : (size_t)n;
    DevBuf<double> dX, dl, dloc, dXp, dlp, dlocp, dout;
    StreamDrain s{nullptr, true};     // own non-blocking stream (the library never launches on the NULL stream)
    HIPCHK_AT("cov_rns*", hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking));
    HIPCHK_AT("cov_rns*", dX.alloc((size_t)n * p));
    HIPCHK_AT("cov_rns*", dl.alloc((size_t)n * 2));
    HIPCHK_AT("cov_rns*", dloc.alloc((size_t)LOCP_FIELDS * n));
    HIPCHK_AT("cov_rns*", dout.alloc(rows * (size_t)n));
    HIPCHK_AT("cov_rns*", upload_canon(dX, X, (size_t)n * p, s));
    HIPCHK_AT("cov_rns*", upload_canon(dl, locs, (size_t)n * 2, s));
    launch_loc_params(loc_args(n, p, dX, dl, dloc, n, tv, ms.smooth_kind, sl), s);
    PairArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.n = n; pa.cols = dloc; pa.stride = n; pa.out = dout; pa.gr = ms.gr; pa.nu_fixed = ms.nu_fixed;
    if (which == 2) {
        HIPCHK_AT("cov_rns*", dXp.alloc((size_t)m * p));
        HIPCHK_AT("cov_rns*", dlp.alloc((size_t)m * 2));
        HIPCHK_AT("cov_rns*", dlocp.alloc((size_t)LOCP_FIELDS * m));
        HIPCHK_AT("cov_rns*", upload_canon(dXp, X_pred, (size_t)m * p, s));
        HIPCHK_AT("cov_rns*", upload_canon(dlp, locs_pred, (size_t)m * 2, s));
        launch_loc_params(loc_args(m, p, dXp, dlp, dlocp, m, tv, ms.smooth_kind, sl), s);
        pa.m = m; pa.rows = dlocp; pa.stride_rows = m; pa.ld = m; pa.nrows_out = m; pa.ncols_out = n;
        launch_pair_rect(ms.mode, pa, s);
    } else {
        pa.m = n; pa.rows = dloc; pa.stride_rows = n; pa.ld = n; pa.nrows_out = n; pa.ncols_out = n;
        launch_pair_sym(ms.mode, true, pa, s);
    }
    HIPCHK_AT("cov_rns*", hipGetLastError());
    HIPCHK_AT("cov_rns*", hipMemcpyAsync(out, dout, rows * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK_AT("cov_rns*", hipStreamSynchronize(s));
    return 0;
}

extern "C" int cocons_cov_rns(int n, int p, const double *theta, const double *locs, const double *X,
                              const double *smooth_limits, double *out)
{
    return cov_common(0, n, 0, p, theta, locs, nullptr, X, nullptr, smooth_limits, out);
}

extern "C" int cocons_cov_rns_classic(int n, int p, const double *theta, const double *locs, const double *X, double *out)
{
    return cov_common(1, n, 0, p, theta, locs, nullptr, X, nullptr, nullptr, out);
}

extern "C" int cocons_cov_rns_pred(int n, int m, int p, const double *theta, const double *locs,
                                   const double *locs_pred, const double *X, const double *X_pred,
                                   const double *smooth_limits, double *out)
{
    return cov_common(2, n, m, p, theta, locs, locs_pred, X, X_pred, smooth_limits, out);
}

// ---------------------------------------------------------------------------
// sparse/taper covariance entries (first slice): the assembly only -- the spam
// Cholesky behind R/neg2loglikelihood.R:20-108 stays with the caller.
static int taper_common(bool pred, int n, int m, int p, const double *theta, const double *locs,
                        const double *locs_pred, const double *X, const double *X_pred, const double *smooth_limits,
                        int nnz, const int *colindices, const int *rowpointers, double *out)
{
    if (n <= 0 || p <= 0 || p > COCONS_P_MAX || !theta || !locs || !X || !smooth_limits || nnz < 0 || !colindices ||
        !rowpointers || (nnz > 0 && !out) || (pred && (m <= 0 || !locs_pred || !X_pred)))
        return fail(-1, "cov_rns_taper*: bad argument");
    const int nrows = pred ? m : n;
    if (rowpointers[0] != 1 || rowpointers[nrows] != nnz + 1) return fail(-1, "cov_rns_taper*: rowpointers do not match nnz (1-based CSR expected)");
    for (int w = 0; w < nnz; ++w)
        if (colindices[w] < 1 || colindices[w] > n) return fail(-1, "cov_rns_taper*: column index out of range");
    ThetaVecs tv;
    make_theta_vecs(theta, p, tv, true);                                  // FULL scale vector (cocons_taper.cpp:207)
    // smoothness dispatch of cov_rns_taper (:183-201); the prediction variant always takes the Bessel branch
    ModeSel ms = select_mode(theta, p, smooth_limits, pred ? 2 : 0);
    const size_t nz = nnz > 0 ? (size_t)nnz : 1;
    DevBuf<double> dX, dl, dloc, dXp, dlp, dlocp, dout;
    DevBuf<int> dci, drp;
    StreamDrain s{nullptr, true};
    HIPCHK_AT("cov_rns_taper*", hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking));
    HIPCHK_AT("cov_rns_taper*", dX.alloc((size_t)n * p));
    HIPCHK_AT("cov_rns_taper*", dl.alloc((size_t)n * 2));
    HIPCHK_AT("cov_rns_taper*", dloc.alloc((size_t)LOCP_FIELDS * n));
    HIPCHK_AT("cov_rns_taper*", dout.alloc(nz));
    HIPCHK_AT("cov_rns_taper*", dci.alloc(nz));
    HIPCHK_AT("cov_rns_taper*", drp.alloc((size_t)nrows + 1));
    HIPCHK_AT("cov_rns_taper*", upload_canon(dX, X, (size_t)n * p, s));
    HIPCHK_AT("cov_rns_taper*", upload_canon(dl, locs, (size_t)n * 2, s));
    HIPCHK_AT("cov_rns_taper*", hipMemcpyAsync(dci, colindices, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK_AT("cov_rns_taper*", hipMemcpyAsync(drp, rowpointers, (size_t)(nrows + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    launch_loc_params(loc_args(n, p, dX, dl, dloc, n, tv, ms.smooth_kind, smooth_limits), s);
    if (pred) {
        HIPCHK_AT("cov_rns_taper*", dXp.alloc((size_t)m * p));
        HIPCHK_AT("cov_rns_taper*", dlp.alloc((size_t)m * 2));
        HIPCHK_AT("cov_rns_taper*", dlocp.alloc((size_t)LOCP_FIELDS * m));
        HIPCHK_AT("cov_rns_taper*", upload_canon(dXp, X_pred, (size_t)m * p, s));
        HIPCHK_AT("cov_rns_taper*", upload_canon(dlp, locs_pred, (size_t)m * 2, s));
        launch_loc_params(loc_args(m, p, dXp, dlp, dlocp, m, tv, ms.smooth_kind, smooth_limits), s);
    }
    TaperLaunch t;
    t.mode = pred ? (int)MODE_GEOM : ms.mode; t.pred = pred; t.nrows = pred ? m : n; t.nnz = nnz; t.ci = dci; t.rp = drp; t.out = dout;
    t.rows = pred ? dlocp : dloc; t.stride_rows = pred ? m : n; t.cols = dloc; t.stride = n; t.nu_fixed = pred ? 0.0 : ms.nu_fixed;
    launch_taper(t, s);
    HIPCHK_AT("cov_rns_taper*", hipGetLastError());
    if (nnz > 0) HIPCHK_AT("cov_rns_taper*", hipMemcpyAsync(out, dout, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK_AT("cov_rns_taper*", hipStreamSynchronize(s));
    return 0;
}

extern "C" int cocons_cov_rns_taper(int n, int p, const double *theta, const double *locs, const double *X,
                                    const double *smooth_limits, int nnz, const int *colindices,
                                    const int *rowpointers, double *entries)
{
    return taper_common(false, n, 0, p, theta, locs, nullptr, X, nullptr, smooth_limits, nnz, colindices, rowpointers, entries);
}

extern "C" int cocons_cov_rns_taper_pred(int n, int m, int p, const double *theta, const double *locs,
                                         const double *locs_pred, const double *X, const double *X_pred,
                                         const double *smooth_limits, int nnz, const int *colindices,
                                         const int *rowpointers, double *entries)
{
    return taper_common(true, n, m, p, theta, locs, locs_pred, X, X_pred, smooth_limits, nnz, colindices, rowpointers, entries);
}

// ---------------------------------------------------------------------------
// Rows of the dense covariance / correlation matrix of a fit, without the n x n matrix.
// Works on the fit's ORIGINAL observation order (the reference's orientation rule "ii = the smaller index"
// and its u <= eps rule depend on it), from the host copies the handle keeps: O(n p) bytes go down,
// nidx * n doubles come back.
extern "C" int cocons_cov_rows(cocons_fit *f, const double *theta, int classic, int nidx, const int *idx, int cor,
                               double *out)
{
    FIT_ENTER(f);
    if (int rc = no_taper(f, "cocons_cov_rows")) return rc;
    if (!theta || nidx <= 0 || !idx || !out) return fail(-1, "cocons_cov_rows: bad argument");
    const int n = f->n_user, p = f->p;          // (works on the host copies: the caller's observations in the caller's order)
    for (int b = 0; b < nidx; ++b)
        if (idx[b] < 0 || idx[b] >= n) return fail(-1, "cocons_cov_rows: row index out of range (0-based)");
    ThetaVecs tv;
    make_theta_vecs(theta, p, tv);
    ModeSel ms = select_mode(theta, p, f->smooth_limits, classic ? 1 : 0);
    DevBuf<double> dX, dl, dloc, dout;
    DevBuf<int> didx;
    StreamDrain s{f->stream, false};
    HIPCHK_AT("cocons_cov_rows", dX.alloc((size_t)n * p));
    HIPCHK_AT("cocons_cov_rows", dl.alloc((size_t)n * 2));
    HIPCHK_AT("cocons_cov_rows", dloc.alloc((size_t)LOCP_FIELDS * n));
    HIPCHK_AT("cocons_cov_rows", dout.alloc((size_t)nidx * n));
    HIPCHK_AT("cocons_cov_rows", didx.alloc((size_t)nidx));
    HIPCHK_AT("cocons_cov_rows", upload_canon(dX, f->h_X.data(), (size_t)n * p, s));
    HIPCHK_AT("cocons_cov_rows", upload_canon(dl, f->h_locs.data(), (size_t)n * 2, s));
    HIPCHK_AT("cocons_cov_rows", hipMemcpyAsync(didx, idx, (size_t)nidx * sizeof(int), hipMemcpyHostToDevice, s));
    launch_loc_params(loc_args(n, p, dX, dl, dloc, n, tv, ms.smooth_kind, f->smooth_limits), s);
    launch_cov_rows(ms.mode, n, nidx, didx, dloc, n, ms.gr, ms.nu_fixed, cor, dout, s);
    HIPCHK_AT("cocons_cov_rows", hipGetLastError());
    HIPCHK_AT("cocons_cov_rows", hipMemcpyAsync(out, dout, (size_t)nidx * n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK_AT("cocons_cov_rows", hipStreamSynchronize(s));
    return 0;
}
