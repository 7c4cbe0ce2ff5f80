/*
 * oracle/ref_wrap.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * C entries around the reference's own, unmodified covariance sources, with the signatures of
 * oracle/cocons_oracle.c (theta as the 6 x p row-major table, column-major matrices, 1-based CSR).
 * The two reference sources are pulled in by paths given on the compiler's command line
 *     -DCOCONS_REF_FULL='"<dir>/cocons_full.cpp"'  -DCOCONS_REF_TAPER='"<dir>/cocons_taper.cpp"'
 * and see oracle/ref_shim/ in place of Rcpp and Boost (oracle/Makefile, target `ref`).  No line of the
 * reference stands in this file; the library built from it goes to oracle/_ref/, which git ignores.
 */
#if !defined(COCONS_REF_FULL) || !defined(COCONS_REF_TAPER)
#error "give the reference sources as -DCOCONS_REF_FULL='\"...\"' and -DCOCONS_REF_TAPER='\"...\"'"
#endif

#include COCONS_REF_FULL
#include COCONS_REF_TAPER

namespace {

const char *const kAspects[6] = {"std.dev", "scale", "aniso", "tilt", "smooth", "nugget"};

Rcpp::List theta_list(const double *theta, int p)
{
    Rcpp::List l;
    for (int a = 0; a < 6; ++a)
        l.set(kAspects[a], Rcpp::NumericVector(theta + (std::size_t)a * p, theta + (std::size_t)(a + 1) * p));
    return l;
}

/* the reference shifts its index vectors by -1 in place: it gets private double copies */
Rcpp::NumericVector index_vector(const int *idx, int len)
{
    Rcpp::NumericVector v(len);
    for (int i = 0; i < len; ++i) v[i] = idx[i];
    return v;
}

void copy_out(const Rcpp::NumericMatrix &m, double *out)
{
    const std::size_t len = (std::size_t)m.nrow() * m.ncol();
    for (std::size_t i = 0; i < len; ++i) out[i] = m.begin()[i];
}

}  // namespace

extern "C" {

int ref_cov_rns(int n, int p, const double *theta, const double *locs, const double *X,
                const double *smooth_limits, double *out)
{
    Rcpp::List th = theta_list(theta, p);
    Rcpp::NumericMatrix l(n, 2, locs), x(n, p, X);
    Rcpp::NumericVector sl(smooth_limits, smooth_limits + 2);
    copy_out(cov_rns(th, l, x, sl), out);
    return 0;
}

int ref_cov_rns_classic(int n, int p, const double *theta, const double *locs, const double *X, double *out)
{
    Rcpp::List th = theta_list(theta, p);
    Rcpp::NumericMatrix l(n, 2, locs), x(n, p, X);
    copy_out(cov_rns_classic(th, l, x), out);
    return 0;
}

int ref_cov_rns_pred(int n, int m, int p, const double *theta, const double *locs, const double *locs_pred,
                     const double *X, const double *X_pred, const double *smooth_limits, double *out)
{
    Rcpp::List th = theta_list(theta, p);
    Rcpp::NumericMatrix l(n, 2, locs), lp(m, 2, locs_pred), x(n, p, X), xp(m, p, X_pred);
    Rcpp::NumericVector sl(smooth_limits, smooth_limits + 2);
    copy_out(cov_rns_pred(th, l, lp, x, xp, sl), out);
    return 0;
}

int ref_cov_rns_taper(int n, int p, const double *theta, const double *locs, const double *X,
                      const double *smooth_limits, int nnz, const int *colindices, const int *rowpointers,
                      double *out)
{
    Rcpp::List th = theta_list(theta, p);
    Rcpp::NumericMatrix l(n, 2, locs), x(n, p, X);
    Rcpp::NumericVector sl(smooth_limits, smooth_limits + 2);
    Rcpp::NumericVector ci = index_vector(colindices, nnz), rp = index_vector(rowpointers, n + 1);
    Rcpp::NumericVector v = cov_rns_taper(th, l, x, ci, rp, sl);
    for (int i = 0; i < nnz; ++i) out[i] = v[i];
    return 0;
}

int ref_cov_rns_taper_pred(int n, int m, int p, const double *theta, const double *locs,
                           const double *locs_pred, const double *X, const double *X_pred,
                           const double *smooth_limits, int nnz, const int *colindices,
                           const int *rowpointers, double *out)
{
    Rcpp::List th = theta_list(theta, p);
    Rcpp::NumericMatrix l(n, 2, locs), lp(m, 2, locs_pred), x(n, p, X), xp(m, p, X_pred);
    Rcpp::NumericVector sl(smooth_limits, smooth_limits + 2);
    Rcpp::NumericVector ci = index_vector(colindices, nnz), rp = index_vector(rowpointers, m + 1);
    Rcpp::NumericVector v = cov_rns_taper_pred(th, l, lp, x, xp, ci, rp, sl);
    for (int i = 0; i < nnz; ++i) out[i] = v[i];
    return 0;
}

double ref_sumsmoothlone(const double *x, int len, double lambda, double alpha)
{
    Rcpp::NumericVector v(x, x + len);
    return sumsmoothlone(v, lambda, alpha);
}

/* the reference's own default for alpha */
double ref_sumsmoothlone_default_alpha(const double *x, int len, double lambda)
{
    Rcpp::NumericVector v(x, x + len);
    return sumsmoothlone(v, lambda);
}

}  // extern "C"
