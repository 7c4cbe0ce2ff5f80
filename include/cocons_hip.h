/*
 * cocons_hip.h -- C ABI of the MI355X-native dense hot path of blasif/cocons.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / Rcpp types.
 * Every entry point names the reference interface it replaces (paths relative to
 * the reference tree).  The R-side `.Call` glue a maintainer would add is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - matrices are column-major (R layout); `locs` is n x 2, `X` is n x p.
 *   - `theta` is a 6 x p row-major table in the order of the reference's
 *     dictionary minus "mean" (R/profile.R:5-7): std.dev, scale, aniso, tilt,
 *     smooth, nugget -- i.e. what `theta_list[-1]` carries by name
 *     (src/cocons_full.cpp:47-54).
 *   - return value: 0 ok; k > 0 = leading minor of order k is not positive
 *     (LAPACK dpotrf convention; the glue maps it to the reference's 1e+06
 *     sentinel or stop("Cholesky error"), R/neg2loglikelihood.R:200-206);
 *     < 0 = bad argument or HIP error, text in cocons_last_error().
 *   - nothing throws, aborts or exits; no HIP call happens at load time
 *     (fork-safe: the device context is created lazily per process).
 *   - threads: the reference's callers are single-threaded R interpreters, one per worker process
 *     (R/optim.R:117-121, 234-235), and that is all the drop-in needs.  Beyond it: ONE handle serves one call
 *     at a time (a second thread entering with the same handle waits until the first call has returned -- every
 *     entry point holds the handle's operation lock); DIFFERENT handles may be created, used and destroyed from
 *     different threads concurrently, the stateless entry points likewise; cocons_last_error() is per thread.
 *     A handle must not be destroyed while another thread is inside a call on it, and a stream installed with
 *     cocons_fit_set_stream is the caller's: the creation of ANOTHER handle or of a batch slot never launches the
 *     library's probe kernels on it.  (The one exception is cocons_fit_set_stream itself, see there.)
 */
#ifndef COCONS_HIP_H
#define COCONS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define COCONS_P_MAX 32          /* max columns of the design matrix */

typedef struct cocons_fit cocons_fit;   /* opaque: device-resident data of one model fit */

/* library ------------------------------------------------------------------ */
const char *cocons_last_error(void);
int cocons_abi_version(void);
/* number of visible HIP devices (>=0), or <0 on error */
int cocons_device_count(void);

/* ---- stateless covariance assembly (host buffers in, host buffer out) --------
 * replaces .Call("_cocons_cov_rns", theta, locs, x_covariates, smooth_limits)
 *   src/RcppExports.cpp:29-40 -> cov_rns, src/cocons_full.cpp:40-321          */
int cocons_cov_rns(int n, int p, const double *theta, const double *locs,
                   const double *X, const double *smooth_limits, double *out_nxn);
/* replaces .Call("_cocons_cov_rns_classic", theta, locs, x_covariates)
 *   src/RcppExports.cpp:59-69 -> cov_rns_classic, src/cocons_full.cpp:480-594  */
int cocons_cov_rns_classic(int n, int p, const double *theta, const double *locs,
                           const double *X, double *out_nxn);
/* replaces .Call("_cocons_cov_rns_pred", theta, locs, locs_pred, x_covariates,
 *                x_covariates_pred, smooth_limits)
 *   src/RcppExports.cpp:43-56 -> cov_rns_pred, src/cocons_full.cpp:334-471
 * out is m x n column-major, row = prediction location.                        */
int cocons_cov_rns_pred(int n, int m, int p, const double *theta, const double *locs,
                        const double *locs_pred, const double *X, const double *X_pred,
                        const double *smooth_limits, double *out_mxn);
/* replaces .Call("_cocons_sumsmoothlone", x, lambda, alpha)
 *   src/RcppExports.cpp:16-26 -> sumsmoothlone, src/cocons_full.cpp:12-30 (host, O(p)) */
double cocons_sumsmoothlone(const double *x, int len, double lambda, double alpha);

/* ---- sparse/taper covariance entries (first slice) ---------------
 * replaces .Call("_cocons_cov_rns_taper", theta, locs, x_covariates, colindices, rowpointers, smooth_limits)
 *   src/RcppExports.cpp:88-101 -> cov_rns_taper, src/cocons_taper.cpp:151-433
 * and .Call("_cocons_cov_rns_taper_pred", theta, locs, locs_pred, x_covariates, x_covariates_pred,
 *           colindices, rowpointers, smooth_limits)
 *   src/RcppExports.cpp:72-87 -> cov_rns_taper_pred, src/cocons_taper.cpp:17-139.
 * colindices (nnz) / rowpointers (rows + 1) are the spam CSR pattern, 1-BASED as spam stores them, and are
 * only read: the reference shifts its (coerced copies of the) index vectors by -1 in place (:73-74, :211-212),
 * which a caller never sees because spam's integer slots are copied on coercion to NumericVector.
 * entries[w] receives the covariance of stored entry w (row-wise order).  The tapering itself and the
 * sparse Cholesky (R/neg2loglikelihood.R:20-108) stay with the caller.                              */
int cocons_cov_rns_taper(int n, int p, const double *theta, const double *locs, const double *X,
                         const double *smooth_limits, int nnz, const int *colindices, const int *rowpointers,
                         double *entries);
int cocons_cov_rns_taper_pred(int n, int m, int p, const double *theta, const double *locs,
                              const double *locs_pred, const double *X, const double *X_pred,
                              const double *smooth_limits, int nnz, const int *colindices,
                              const int *rowpointers, double *entries);

/* ---- taper objective through the dense factorisation (second slice) ----------------
 * replaces the body of GetNeg2loglikelihoodTaper (R/neg2loglikelihood.R:20-53): ref_taper@entries *
 * cov_rns_taper(...), update.spam.chol.NgPeyton, determinant, forwardsolve.  The handle takes what is constant
 * over the optimisation -- locs, x_covariates, z (n x r), smooth.limits and ref_taper's pattern (colindices /
 * rowpointers, 1-based, symmetric, diagonal stored) with its entries -- and cocons_neg2loglik_dense on it
 * returns  sum_k [ n log 2 pi + 2 sum log diag chol(S) + resid_k' S^-1 resid_k ],  S = taper o cov_rns_taper(theta):
 * spam's value, from a DENSE factorisation of S (zeros stored) -- for n^2 doubles within the device's memory.
 * `parts` as for the dense handle (log-det half, quadratic forms), from which the caller forms
 * GetNeg2loglikelihoodTaperProfile (:73-108, with theta$std.dev[1] = 0).  cocons_neg2loglik_batch pipelines its
 * points over clones of such a handle as for a dense one, cocons_predict_taper is its prediction core; every other
 * fit entry point refuses it.  NULL + cocons_last_error() on failure.                                                */
cocons_fit *cocons_fit_create_taper(int n, int p, int r, const double *locs, const double *X, const double *z,
                                    const double *smooth_limits, int device, int nnz, const int *colindices,
                                    const int *rowpointers, const double *taper_entries);

/* ---- taper patterns from delta: neighbour search and taper values on the device -----------------------------------
 * What spam::nearest.dist and the taper function build in R (R/predict.R:219-235, R/optim.R:377, R/sim.R:194).  The taper of a
 * pair at distance d, with h = d / delta -- spam's cov.wend1, cov.wend2 and cov.sph with theta = c(delta, 1):          */
#define COCONS_TAPER_WEND1 1   /* (1 - h)^4 (4 h + 1)                    */
#define COCONS_TAPER_WEND2 2   /* (1 - h)^6 (35 h^2 + 18 h + 3) / 3      */
#define COCONS_TAPER_SPH   3   /* 1 - 1.5 h + 0.5 h^3                    */

/* cocons_taper_pattern: every pair of a query point (locs_query, m x 2; NULL: the n points of locs themselves, m is then
 * ignored) and a point of locs (n x 2, both column-major) with d = sqrt(dx dx + dy dy) <= delta in fp64, as spam stores it:
 * 1-based CSR, rows = queries, columns = indices into locs, strictly increasing within a row, `entries` the taper `kind` of
 * every pair.  Pairs at d = 0 are stored (the diagonal of the self pattern, coincident points).  Stateless: host buffers in
 * and out, device memory of the call only.  The arrays are a function of the inputs alone (two calls agree bit for bit), and
 * the self pattern with its entries is symmetric to the bit.
 * colindices == NULL: the count call -- *nnz and rowpointers (rows + 1) are written, entries is not read.  Otherwise `cap`
 * (the room in colindices / entries) must be >= the pattern's nnz: if it is not, -1, the message names the nnz needed and
 * nothing is written.  A pattern of more than INT_MAX - 1 entries is refused, naming the count.
 * -1, with a message starting with the entry's name, before any device work and with the outputs untouched: a null locs, nnz
 * or rowpointers, a null entries with colindices given, n < 1, m < 1 with a query set, delta not finite or <= 0, kind
 * outside 1 .. 3, a coordinate that is not finite.                                                                    */
int cocons_taper_pattern(int n, const double *locs, int m, const double *locs_query /* NULL: self */, double delta, int kind,
                         int device, long long cap, long long *nnz, int *rowpointers, int *colindices, double *entries);

/* cocons_fit_create_taper from delta: the self pattern of locs and its taper entries by cocons_taper_pattern's builder, then
 * the handle exactly as cocons_fit_create_taper makes it from those arrays (the same code).  Refusals as above (null
 * pointers, n < 1, delta, kind, coordinates), then cocons_fit_create_taper's.  NULL + cocons_last_error() on failure.   */
cocons_fit *cocons_fit_create_taper_delta(int n, int p, int r, const double *locs, const double *X, const double *z,
                                          const double *smooth_limits, int device, double delta, int kind);

/* Kriging from a held factor: cocoPredict (R/predict.R:136-183) at any number of new locations for one theta.
 * cocons_krige_prepare assembles Sigma(theta), factors it once with (z[:, z_col] - X mean)' as the one right-hand side and
 * keeps, in buffers of its own on the handle: the lower factor in packed 128 x 128 tiles (nt (nt + 1) / 2 of them, not the
 * factorisation buffer), w = L^-1 r, the solve's operands per diagonal tile, the observation side of cov_rns_pred and
 * the chunk buffers.  It replaces any earlier state; on a non-positive pivot it returns the failing minor and leaves no state.
 * cocons_krige_apply then gives, for m >= 0 new locations (locs_pred m x 2, X_pred m x p, column-major),
 *   stochastic[i] = c_i' Sigma^-1 (z - X mean),  quadform[i] = c_i' Sigma^-1 c_i      (as cocons_predict_dense)
 * in chunks of at most `max_rows` rows (rounded down to a multiple of 64, at least 64; 0: as many as keep the chunk
 * buffers within 1 GiB, at most 16384) -- no factorisation, and device memory that does not depend on m.  A row's
 * outputs do not depend on the chunk size or on the other rows (bit for bit).  No other entry point touches the state;
 * cocons_krige_release and cocons_fit_destroy free it.  cocons_krige_info: out4 = {prepared, device bytes held, rows per
 * chunk, n}.  Refused (< 0, with a message) on taper and sharded handles, and apply without a state.                  */
int cocons_krige_prepare(cocons_fit *fit, const double *theta, const double *mean, int z_col, int max_rows);
int cocons_krige_apply(cocons_fit *fit, int m, const double *locs_pred, const double *X_pred,
                       double *stochastic, double *quadform);
int cocons_krige_release(cocons_fit *fit);
int cocons_krige_info(cocons_fit *fit, long long *out4);

/* Joint prediction from the held factor, against the theta, realisation and mean of cocons_krige_prepare: what
 * cocoPredict's dense branch (R/predict.R:136-183) gives per location, between the m new locations, and the conditional
 * draws of cocoSim (R/sim.R:84-127) without the factorisation of the joint (n + m) x (n + m) matrix.
 *   stochastic[i] = c_i' Sigma^-1 (z - X mean)            (the bits of cocons_krige_apply for the same rows)
 *   cov  = Sigma_uu - C Sigma^-1 C'                       m x m column-major, full and symmetric to the bit; NULL: not wanted
 *   sims = L_S E + (X_pred mean + stochastic)             m x nsim, L_S L_S' = cov, E = iiderrors (m x nsim); nsim = 0: no draws
 * with C = cov_rns_pred(theta, locs, locs_pred, X, X_pred) and Sigma_uu = cov_rns(theta, locs_unobs, X_pred) -- nugget on
 * the diagonal, the coincident-pair rule, as cocons_sim_cond_dense's block; locs_unobs = NULL: locs_pred.  With nsim = 0
 * nothing is factored.  Repeated calls agree bit for bit, and the leading block of cov (and the leading entries of
 * stochastic) for the first rows of a request do not depend on the rows behind them.
 * The call takes round_up(m, 64) x npad + round_up(m, 128)^2 doubles of device memory and releases them before it returns;
 * the kriging state is not touched.  Returns 0; -5 when the predictive covariance is not positive definite in floating
 * point (nsim > 0 only; the message names the failing minor); -1 for m < 1, a null locs_pred, X_pred or stochastic,
 * nsim < 0, nsim > 0 with a null iiderrors or sims, a null, taper or sharded handle, or no prepared state; < 0 otherwise
 * (a failed allocation names the bytes needed).  The outputs are written on 0 only.                                     */
int cocons_krige_joint(cocons_fit *fit, int m, const double *locs_pred, const double *X_pred,
                       const double *locs_unobs,           /* m x 2, NULL = locs_pred */
                       double *stochastic,                 /* m */
                       double *cov,                        /* m x m column-major, may be NULL */
                       int nsim, const double *iiderrors,  /* m x nsim, nsim = 0: no draws */
                       double *sims);                      /* m x nsim */

/* Kriging core of the sparse branch of cocoPredict (R/predict.R:216-283) on a taper handle: replaces
 * cov_rns_taper / cov_rns_taper_pred times their tapers, inv_cov <- spam::solve(taper_two, t(pred_taper)) (:244),
 * crossprod(resid, inv_cov) (:252) and rowSums(pred_taper * t(inv_cov)) (:267).  pred_taper's slots go in as they
 * are (m rows, columns = observations, 1-based); theta / mean / z_col as for cocons_predict_dense.
 * stochastic[m], quadform[m] come back; the systematic part and the variance lines (:247-249, :264-272) stay in R. */
int cocons_predict_taper(cocons_fit *fit, const double *theta, const double *mean, int z_col, int m,
                         const double *locs_pred, const double *X_pred, int nnz_pred, const int *colindices_pred,
                         const int *rowpointers_pred, const double *taper_entries_pred,
                         double *stochastic, double *quadform);

/* Kriging from a held BAND factor: cocons_predict_taper in two parts, for any number of new locations at one theta.
 * cocons_krige_taper_prepare (taper handles, every buffer layout) assembles S(theta) as cocons_predict_taper does, factors it
 * once with (z[:, z_col] - X mean)' as the one right-hand side and keeps, in buffers of its own on the handle: the lower
 * 128 x 128 tiles of the factor's envelope packed per tile column, the solve's operands per diagonal tile, w = L^-1 r,
 * the observation side of cov_rns_taper_pred and the chunk buffers.  It replaces any earlier state; on a non-positive
 * pivot it returns the failing minor (> 0) and leaves no state.
 * cocons_krige_taper_apply: for m >= 0 new locations it returns
 *   stochastic[i] = c_i' S^-1 (z - X mean),  quadform[i] = c_i' S^-1 c_i            (the quantities of cocons_predict_taper)
 * from the same inputs: locs_pred m x 2, X_pred m x p (column-major), and pred_taper's CSR slots, 1-based, columns =
 * observations in the caller's order.  Chunks hold at most `max_rows` rows (rounded down to a multiple of 64, at least 64;
 * 0: as many as keep the chunk buffers within 1 GiB, at most 16384).  A chunk's right-hand side lives in a ring of W tile
 * columns (W = the widest tile column of the envelope), never in rows x n.  Apply does no factorisation.  Device memory
 * held does not depend on m: the CSR staging of a chunk belongs to the state, is grown to the densest chunk seen and is
 * counted in the reported bytes.  A row's outputs depend only on that row's data, the state and the row's position modulo
 * 64 in the request -- not on max_rows, on m or on the other rows; repeats agree bit for bit (fixed sum order, no
 * atomics).  A row without neighbours gives exactly 0.0 and 0.0.
 * Refused with -1 and a message starting with the entry's name, before any device work and with the outputs untouched:
 * null arguments or m < 0; a dense or sharded handle; no prepared state; rowpointers_pred[0] != 1, decreasing row
 * pointers or rowpointers_pred[m] != nnz_pred + 1; a column outside [1, n]; column indices not strictly increasing
 * within a row (spam's invariant; the scatter relies on it).
 * No other entry point reads or writes the state; cocons_krige_taper_release and cocons_fit_destroy free it.
 * cocons_krige_taper_info: out6 = {prepared, device bytes held, rows per chunk, n, W, nt (tile columns)}.               */
int cocons_krige_taper_prepare(cocons_fit *fit, const double *theta, const double *mean, int z_col, int max_rows);
int cocons_krige_taper_apply(cocons_fit *fit, int m, const double *locs_pred, const double *X_pred, int nnz_pred,
                             const int *colindices_pred, const int *rowpointers_pred, const double *taper_entries_pred,
                             double *stochastic, double *quadform);
int cocons_krige_taper_release(cocons_fit *fit);
int cocons_krige_taper_info(cocons_fit *fit, long long *out6);

/* cocons_krige_taper_apply without a pattern from the caller: pred_taper is what nearest.dist(locs_pred, locs, delta) and the
 * taper `kind` (COCONS_TAPER_*) give, found per chunk on the device against the observations in the handle's own order --
 * neighbour search, taper values and the buckets per tile column land straight in the state's CSR staging; the nt + 1 bucket
 * offsets are the only thing that comes back to the host, and no per-entry data crosses to the device.  Outputs, chunking
 * and guarantees are cocons_krige_taper_apply's (independence of max_rows bit for bit, exactly 0.0 and 0.0 for a row without
 * neighbours), and so are the bits for the pattern cocons_taper_pattern(locs, locs_pred) exports.  *nnz_out (may be NULL):
 * the pattern's entries over all m rows.  The grid over the observations is built by the first such call on a prepared
 * state, belongs to the state (counted in cocons_krige_taper_info's bytes, dropped with it); the staging grows, with the
 * stream drained, when a chunk needs more entries than it holds.
 * -1, with a message starting with the entry's name, before any device work and with the outputs untouched: m < 0, a null
 * pointer, delta not finite or <= 0, kind outside 1 .. 3, a coordinate of locs_pred that is not finite, a null, dense or
 * sharded handle, no prepared state.                                                                                       */
int cocons_krige_taper_apply_delta(cocons_fit *fit, int m, const double *locs_pred, const double *X_pred, double delta, int kind,
                                   double *stochastic, double *quadform, long long *nnz_out /* may be NULL */);

/* Joint prediction for a tapered fit from the held band factor, against the theta, realisation and mean of
 * cocons_krige_taper_prepare: cocons_krige_joint's outputs for type = "sparse" (the reference's cocoSim has no
 * conditional branch for sparse objects).
 *   stochastic[i] = c_i' S^-1 (z - X mean)                (the bits of cocons_krige_taper_apply for the same rows)
 *   cov  = S_uu - C S^-1 C'                               m x m column-major, full and symmetric to the bit; NULL: not wanted
 *   sims = L_S E + (X_pred mean + stochastic)             m x nsim, L_S L_S' = cov, E = iiderrors (m x nsim); nsim = 0: no draws
 * C = pred_taper o cov_rns_taper_pred(theta, ...) exactly as cocons_krige_taper_apply forms it (same CSR contract, same
 * checks).  S_uu = taper_uu o cov_rns_taper(theta, locs_unobs, X_pred, uu pattern): the objective's entries, variance plus
 * nugget on the diagonal, the kernel's own coincident-pair rule; locs_unobs = NULL: locs_pred.  The uu pattern is what
 * spam::nearest.dist(newlocs, delta, upper = NULL) gives: m x m, 1-based CSR, columns strictly increasing within a row,
 * every row with its diagonal entry.  Only entries with column <= row are read; the upper triangle is their mirror; outside
 * the pattern S_uu is 0.
 * All m rows are one chunk.  The solved rows V = C L^-T are never held as m x n: the ring of cocons_krige_taper_apply is
 * D - 1 slots deeper (min(W + D - 1, nt) slots) and S -= V_g V_g' is accumulated per group of D tile columns while the
 * window slides.  D: COCONS_KRIGE_JOINT_DEPTH, read per call, 1 .. 16 (default 8); cov does not depend on it to the bit.
 * Repeats agree bit for bit, and the leading block of cov and the leading entries of stochastic for the first rows of a
 * request do not depend on the rows behind them.  The draws factor cov on the plain schedule of the dense factorisation.
 * Device memory: round_up(m, 64) x min(W + D - 1, nt) x 128 + round_up(m, 128)^2 doubles, small arrays and the CSR staging
 * (28 bytes per pred entry, 12 per uu entry), all released before the call returns; the kriging state is read, never
 * written.  cocons_krige_taper_joint_bytes: the device bytes the call allocates for (m, nsim) on this handle but the CSR
 * staging, so that a caller can size m; it takes the same refusals.
 * Returns 0; -5 when the predictive covariance is not positive definite in floating point (nsim > 0 only; the message names
 * the failing minor); -1, with a message starting with the entry's name, before any device work and with the outputs
 * untouched, for m < 1, a null locs_pred, X_pred, stochastic or row pointers, nsim < 0, nsim > 0 with a null iiderrors or
 * sims, a null, dense or sharded handle, no prepared state, a malformed pattern (the checks of cocons_krige_taper_apply), a
 * uu row without its diagonal, or a depth outside 1 .. 16; < 0 otherwise (a failed allocation names the bytes needed).
 * The outputs are written on 0 only.                                                                                       */
int cocons_krige_taper_joint(cocons_fit *fit, int m, const double *locs_pred, const double *X_pred,
                             int nnz_pred, const int *colindices_pred, const int *rowpointers_pred,
                             const double *taper_entries_pred,
                             const double *locs_unobs,           /* m x 2, NULL = locs_pred */
                             int nnz_uu, const int *colindices_uu, const int *rowpointers_uu, const double *taper_entries_uu,
                             double *stochastic,                 /* m */
                             double *cov,                        /* m x m column-major, may be NULL */
                             int nsim, const double *iiderrors,  /* m x nsim, nsim = 0: no draws */
                             double *sims);                      /* m x nsim */
int cocons_krige_taper_joint_bytes(cocons_fit *fit, int m, int nsim, long long *bytes);

/* Sparse branch of cocoSim (R/sim.R:177-217) on a taper handle.  S = taper o cov_rns_taper(theta) (the handle's pattern
 * and taper entries), ordered by `pivot` (1-based permutation of 1..n, spam's `ordering(cholS)`; NULL = the handle's own
 * order, see cocons_fit_taper_order).  With L_P L_P' = S[pivot, pivot] and E = iiderrors (n x nsim, column-major, used
 * as given):   out[pivot[k]-1 + s*n] = (L_P E)[k, s] + (X mean)[pivot[k]-1]
 * -- exactly (t(iiderrors) %*% cholS)[, iord] + trend of :216 when pivot is spam's.  0 / k > 0 (failing minor, in the
 * pivoted order) / < 0.  Refused on a dense handle.
 * pivot = NULL (or the handle's own order): the handle's reverse Cuthill-McKee order and narrow envelope -- a field with
 * covariance S, but for the same draws not the reference's field (the factor of a permuted matrix is not the permuted
 * factor).  Any other pivot: a second taper handle in that order, built on first use, kept while calls pass the same
 * pivot and destroyed with this one; an order whose envelope does not fit the device is refused (< 0), never replaced. */
int cocons_sim_taper(cocons_fit *fit, const double *theta, const double *mean, int nsim,
                     const double *iiderrors, const int *pivot, double *out);
/* the handle's own order (RCM unless COCONS_TAPER_RCM=0): pivot_out[k] = 1-based caller index at position k */
int cocons_fit_taper_order(cocons_fit *fit, int *pivot_out);

/* ---- Vecchia approximation: the model's own likelihood from n small blocks -----------------------------
 * What GpGp computes, on the reference's covariance: every observation is conditioned on at most m earlier ones, so
 *   -2 l(theta) ~ sum_k sum_i [ log 2 pi + 2 log d_i + y_ik^2 ],
 * d_i the conditional standard deviation of observation i given its neighbours and y_ik its whitened residual.  It is exact
 * when every observation names all its predecessors, approximates the likelihood of Sigma(theta) itself (not of a tapered
 * covariance), and needs O(n m) memory: the handle holds the data, the table and O(n (m + r + 16)) bytes of scratch, never
 * an n x n buffer.  The caller's order of the observations is the Vecchia order (maxmin, random, by coordinate: the caller's
 * choice), and the handle keeps it.
 * cocons_fit_create_vecchia: locs, X, z, smooth_limits as for cocons_fit_create (r >= 1); nn is n x m column-major, row i
 * (1-based) listing the observations that observation i is conditioned on as 1-based indices in 1 .. i - 1, 0 = none -- zeros
 * anywhere in a row, a row of zeros is an independent observation.  NULL + cocons_last_error(), which names the entry and the
 * first offending row, before any device work: a null pointer, n < 1, m outside 1 .. 63, an index >= its row or < 0, an index
 * twice in a row, a coordinate that is not finite.  This is a third kind of handle: every fit entry above and below refuses
 * it with a message (cocons_fit_destroy, cocons_fit_stream, cocons_fit_set_stream and cocons_fit_sync serve it), and the
 * entries here refuse every other kind.
 * Block of observation i with neighbours j_1 < .. < j_k: K = Sigma(theta)[(j_1 .. j_k, i), (j_1 .. j_k, i)] -- the diagonal and
 * the pair values of cocons_cov_rns for this theta, closed forms at nu = 1/2, 3/2, 5/2 included, a pair evaluated with the
 * observation that comes earlier in the caller's order on the reference's `ii` side -- factored K = C C' in that order of
 * rows.  Every sum has a fixed order: an observation's outputs depend on its own block alone (not on n, on the other rows,
 * or on COCONS_SPATIAL_SORT), the totals are a tree of fixed shape over the per-observation terms, and repeated calls
 * agree bit for bit.  A pivot of any block that is not positive and finite: the entry returns the smallest 1-based index i
 * of such a block (a row of nn_pred for cocons_vecchia_predict) and writes no output; the handle stays usable.
 * Returns: 0, such an index > 0, or < 0 with cocons_last_error().                                                      */
cocons_fit *cocons_fit_create_vecchia(int n, int p, int r, const double *locs, const double *X, const double *z,
                                      const double *smooth_limits, int device, int m, const int *nn);
/* theta (6 x p table) and mean (p) as for cocons_neg2loglik_dense.  parts (1 + r doubles, may be NULL): parts[0] =
 * sum_i log d_i, parts[1 + k] = sum_i y_ik^2 with y_k the whitened z_k - X mean; *value = sum_k [ n log 2 pi +
 * 2 parts[0] + parts[1 + k] ].                                                                                         */
int cocons_neg2loglik_vecchia(cocons_fit *fit, const double *theta, const double *mean, double *value, double *parts);
/* U B for c >= 1 columns: B and out n x c column-major in the caller's order, out[i, :] = the last component of
 * C_i^-1 B[(neighbours of i, i), :]; logd[i] = log d_i (may be NULL).  U'U approximates Sigma^-1: the building block of the
 * forms with covariates in the mean (Profile, REML, GLS), which the caller finishes in O(n c^2).                        */
int cocons_vecchia_whiten(cocons_fit *fit, const double *theta, int c, const double *B, double *out, double *logd);
/* The Vecchia -2 log-likelihood and its analytic gradient in one call: per block two backward solves on the
 * factor the value needs anyway, then the pair partials of the dense gradient contracted with the block's weights.
 * B == NULL: the columns are z - X mean (c is ignored, it is r); sum_logliks and parts (1 + r doubles, may be NULL) are what
 * cocons_neg2loglik_vecchia returns, to the bit; grad_theta is the 6 x p table in theta's layout with the conventions of
 * cocons_neg2loglik_grad_dense (scale[0] takes the global-range sum, scale[k >= 1] carries the factor 2); grad_quad (may be
 * NULL) the same table for the quadratic forms alone, so that the log-determinant's share is grad_theta - grad_quad (as
 * cocons_neg2loglik_grad_taper); grad_mean p doubles.
 * B != NULL: n x c column-major, c >= 1, in the caller's order, used as given -- the forms with the mean profiled out
 * (Profile, REML).  mean and grad_mean must be NULL.  value = sum_k [ n log 2 pi + 2 parts[0] + parts[1 + k] ] over the c
 * columns, parts has 1 + c doubles.
 * Every sum has a fixed order: repeated calls agree bit for bit, and nothing depends on the other rows of n or on the
 * chunks the rows run in.  The first call allocates O(n) doubles plus one chunk of records, kept on the handle and counted by
 * cocons_vecchia_info.  Returns and refusals as the other Vecchia entries; outputs are written on 0 only.                 */
int cocons_neg2loglik_grad_vecchia(cocons_fit *fit, const double *theta, const double *mean, int c, const double *B,
                                   double *sum_logliks, double *parts,
                                   double *grad_theta, double *grad_quad, double *grad_mean);
/* Expected information of the Vecchia likelihood over ndir directions of the table, dirs as for
 * cocons_fisher_dense: ndir tables of 6 x p, ndir in 1 .. 7 * COCONS_P_MAX, under the dense conventions (scale k = 0 is the
 * global range, scale k >= 1 carries the factor 2, a coincident pair takes the earlier row's diagonal partials, a pair with
 * u >= 706 contributes 0).  For observation i with its block C = L L' (neighbours, then i; l the last row), C_a the same
 * block of Sigma_a = sum_tk dirs[a][t p + k] dSigma / dtheta[t p + k], s = L^-T e_l and g_a = L^-1 (C_a s):
 *   info[a * ndir + b] = r sum_i ( sum_{j < l} g_a[j] g_b[j] + g_a[l] g_b[l] / 2 ),
 *   info_mean[k * p + l] = r sum_i u_i[k] u_i[l],  u_i = sum_rows s[row] X[site(row), .]        (p x p, may be NULL).
 * The block's term is (1 / 2) [ tr(C^-1 C_a C^-1 C_b) - tr(C_NN^-1 C_a,NN C_NN^-1 C_b,NN) ], the information of the block less
 * that of its neighbours alone: the expectation under Sigma(theta) of the Hessian of half of cocons_neg2loglik_vecchia,
 * without a penalty.  It is a Gram matrix -- symmetric to the bit (mirrored from its lower triangle) and positive
 * semi-definite --, the block between mean and covariance parameters is 0, and with every predecessor in the table it is
 * cocons_fisher_dense's.  It is NOT the observed Hessian, and NOT the Godambe (sandwich) information of the composite
 * likelihood: only the sensitivity matrix is formed.
 * Every sum has a fixed order: repeated calls agree bit for bit, and nothing depends on the other rows of n or on the chunks
 * the rows run in.  The first call allocates O(n) doubles plus one chunk of records (at most 16 MiB, or 4096 records), kept
 * on the handle and counted by cocons_vecchia_info; a device that cannot hold them gives < 0 with the bytes in the message.
 * Refused (-1) before any device work: null fit, theta, dirs or info, ndir out of range, non-finite dirs, any other kind of
 * handle.  A failing block returns the smallest 1-based row; outputs are written on 0 only.                              */
int cocons_fisher_vecchia(cocons_fit *fit, const double *theta, int ndir, const double *dirs,
                          double *info, double *info_mean);
/* Local kriging at mp >= 0 new locations (locs_pred mp x 2, X_pred mp x p, column-major): nn_pred is mp x m_pred
 * column-major, 1-based indices into the observations, 0 = none, m_pred in 1 .. 63.  For row i with K its neighbours' block
 * (as above) and c the cross-covariance to them by cocons_cov_rns_pred's rule (an exact coordinate match gives the
 * prediction side's diagonal value; the new site is never part of the factored block, so a site on top of an observation is
 * well posed):  stochastic[i] = c' K^-1 (z[nb, z_col] - X[nb] mean),  quadform[i] = c' K^-1 c  -- the two outputs of
 * cocons_predict_dense, for the same host tail.  A row without neighbours gives 0 and 0.  Rows are processed in chunks of
 * 16384 with buffers of the call (device memory does not grow with mp); a row's outputs depend neither on the chunking nor
 * on the other rows, bit for bit.  Refusals (< 0) as for the table of the handle, and a coordinate that is not finite.    */
int cocons_vecchia_predict(cocons_fit *fit, const double *theta, const double *mean, int z_col, int mp,
                           const double *locs_pred, const double *X_pred, int m_pred, const int *nn_pred,
                           double *stochastic, double *quadform);
/* out4 = {n, m, device bytes the handle holds (data, table, scratch), rows per chunk of cocons_vecchia_predict} */
int cocons_vecchia_info(cocons_fit *fit, long long *out4);

/* ---- Vecchia neighbour search on the device ---------------------
 * The rule, here and in every reference: the neighbours of a query q among a set of candidates are the m candidates with the
 * smallest key (d2, index), d2 = fl(fl(dx dx) + fl(dy dy)) with dx = x_c - x_q, dy = y_c - y_q in fp64, no contraction, no
 * square root; ties go to the lower index.  Rows list the nearest first and are zero-padded, so the table for m is the first
 * m columns of the table for any m' > m.  (np.hypot and sqrt round near-ties differently: a table from another rule may
 * differ in such rows.)  The outputs are a function of the inputs, bit for bit, run to run.
 *
 * cocons_vecchia_neighbours: stateless -- host buffers in and out, device memory of the call only.  locs n x 2 column-major.
 * locs_query == NULL: the ordered self search; rows = n, row i (1-based) names the m nearest among rows 1 .. i - 1 in the
 * caller's order, so row 1 is all zeros (mq is ignored).  Otherwise plain kNN: rows = mq >= 0, row i names the m nearest of
 * the n points to query i (locs_query mq x 2 column-major).  nn: rows x m column-major, 1-based, nearest first, 0 = none.
 * Refused (-1) before any HIP call, nn untouched, with a message that starts with the entry's name: null locs or nn, n < 1,
 * mq < 0 with a query set, m outside 1 .. 63, a coordinate that is not finite.  An adversarial order (early rows all in one
 * corner) or a query far from the points is slower, never wrong.                                                          */
int cocons_vecchia_neighbours(int n, const double *locs, int mq, const double *locs_query /* NULL: ordered self search */,
                              int m, int device, int *nn /* rows x m column-major, 1-based, nearest first, 0 = none */);
/* cocons_fit_create_vecchia with the table cocons_vecchia_neighbours(n, locs, 0, NULL, m, ..) returns: the same handle, the
 * same bits from every Vecchia entry.  The table is searched on the device and written straight into the handle; it never
 * exists on the host.  Refusals as cocons_fit_create_vecchia's, under this entry's name.                                  */
cocons_fit *cocons_fit_create_vecchia_knn(int n, int p, int r, const double *locs, const double *X, const double *z,
                                          const double *smooth_limits, int device, int m);
/* cocons_vecchia_predict with the table cocons_vecchia_neighbours(n, locs, mp, locs_pred, m_pred, ..) returns, to the bit:
 * per chunk of 16384 rows the neighbours are found on the device and land in the chunk's table buffer -- no table upload, no
 * host sort.  A row's outputs depend neither on the chunking nor on the other rows.  The grid over the observations is built
 * by the first such call and belongs to the handle: counted by cocons_vecchia_info from then on, freed with the handle.
 * Refusals as cocons_vecchia_predict's, before any device work and with the outputs untouched; a failing block returns its
 * 1-based row.                                                                                                          */
int cocons_vecchia_predict_knn(cocons_fit *fit, const double *theta, const double *mean, int z_col, int mp,
                               const double *locs_pred, const double *X_pred, int m_pred,
                               double *stochastic, double *quadform);

/* ---- Vecchia neighbours by model correlation ----------------------------------------------------------------
 * Under a covariance with local anisotropy the predecessors that matter for row i are those most CORRELATED with it under
 * Sigma(theta), which lie along the long axis of the local kernel and may be far outside its m Euclidean-nearest.  The rule,
 * here and in every reference, for the observations in the caller's order, theta, m_cand in 1 .. 63, hops in {1, 2}, m in
 * 1 .. 63:
 *  1. N(i) is row i of the Euclidean ordered table of width m_cand: cocons_vecchia_neighbours(n, locs, 0, NULL, m_cand, ..).
 *  2. The candidates C(i): N(i) for hops = 1; N(i) and the N(j) of every j in N(i) for hops = 2.  Zeros are dropped, every
 *     member is earlier than i, and an index counts once however many lists name it (at most 63 + 63^2 = 4032 reach the
 *     deduplication).
 *  3. The key of a candidate j is (rho descending, index ascending), rho(i, j) = fl(v / fl(sqrt(fl(d_i d_j)))): v the entry the
 *     Vecchia block of row i holds for (j, i) -- the pair value with the EARLIER row j on the `ii` side, the bits of
 *     cocons_cov_rns's entry --, d the rows' diagonal values (cocons_cov_rns's diagonal); fp64, one rounding per operation,
 *     no contraction.  rho is compared by the total order of its bit patterns, which for rho >= 0 -- every rho of a valid
 *     model -- is the order of its values.
 *  4. Row i lists the m candidates with the largest key, largest rho first, 1-based, zero-padded.
 * So the output is a function of the inputs alone, the same bits from run to run; the table for m is the first m columns of
 * the table for any m' > m at the same m_cand and hops; a row i <= m_cand + 1 ranks all its predecessors; hops = 1 with
 * m = m_cand returns N(i) as a set; and under an isotropic stationary theta every setting returns the Euclidean table's sets
 * (up to ties of rho's rounding).  host.vecchia_neighbours_corr restates the rule in numpy.
 *
 * cocons_vecchia_neighbours_corr: on any Vecchia handle, which supplies locs, X and smooth_limits in its order; the handle's own
 * table is neither read nor changed.  nn_out: n x m column-major.  The Euclidean candidates are searched on the device, the
 * records of theta are those of every Vecchia evaluation.  The scratch -- n (m_cand + m) ints -- belongs to the call and is
 * freed before it returns: cocons_vecchia_info's bytes are the same before and after.  Returns 0; the smallest 1-based row
 * with a rho that is not finite (nn_out untouched: the failing-block convention); -1 before any device work, nn_out
 * untouched, with a message that starts with the entry's name for: a null argument, a handle that is not a Vecchia handle,
 * m_cand, hops or m out of range, m > min(4032, m_cand + m_cand^2 (hops - 1)), a theta that is not finite.
 *
 * cocons_fit_create_vecchia_corr_knn: cocons_fit_create_vecchia with the table cocons_vecchia_neighbours_corr returns for the
 * same data -- the same bits from every Vecchia entry --, made in one chain on the device: search, records at theta, re-rank,
 * adoption.  Neither table reaches the host.  NULL with the refusals above and cocons_fit_create_vecchia's, under this
 * entry's name, or when a rho is not finite.
 *
 * Out of scope: correlation-ranked neighbours inside the joint handle of cocoPredict_vecchia_joint.
 * These entries add to the ABI and change no existing one: cocons_abi_version stays 1.                                    */
int cocons_vecchia_neighbours_corr(cocons_fit *fit, const double *theta, int m_cand, int hops, int m,
                                   int *nn_out /* n x m column-major, 1-based, largest rho first, 0 = none */);
cocons_fit *cocons_fit_create_vecchia_corr_knn(int n, int p, int r, const double *locs, const double *X, const double *z,
                                               const double *smooth_limits, int device, const double *theta, int m_cand,
                                               int hops, int m);

/* ---- ... of NEW locations, and the grouped handle on a correlation table ---------------------------------------
 * Local kriging conditions a new location q on observations; the ones that matter are again the most correlated with q, not
 * the Euclidean-nearest.  The rule, here and in every reference, for a Vecchia handle with n observations, a new location q
 * with its covariates, theta, m_cand in 1 .. 63, hops in {1, 2}, m in 1 .. 63:
 *  1. P(q) is the row cocons_vecchia_neighbours(n, locs, 1, q, m_cand, ..) returns: the plain kNN of q among ALL observations
 *     by the key (d2, index).
 *  2. The candidates C(q): P(q) for hops = 1; P(q) and, for every j in P(q), the row A(j) =
 *     cocons_vecchia_neighbours(n, locs, 1, loc_j, m_cand, ..) for hops = 2 -- the plain kNN of observation j's own
 *     coordinates among all observations, UNORDERED on purpose: a prediction must not depend on the order the observations
 *     were fitted in, and a new location has no predecessors.  j itself (or a coincident twin) may stand in A(j); zeros are
 *     dropped, and an index counts once however many lists name it.
 *  3. The key of a candidate j is (rho descending, index ascending), rho(q, j) = fl(v / fl(sqrt(fl(d_q d_j)))): v the entry the
 *     prediction block of cocons_vecchia_predict holds for (j, q) -- cocons_cov_rns_pred's entry for the new location q and
 *     observation j: the new location on the `ii` side, the prediction branch's parameters (logistic + sqrt smoothness), an
 *     exact coordinate match gives the new location's diagonal value --; d_q the diagonal value of the prediction branch for
 *     q, d_j that for observation j: the bits cocons_cov_rns_pred returns for a new location placed ON an observation with
 *     that observation's covariates (there the coordinates match, and the entry is the diagonal value), so d_q comes from
 *     the new locations predicted "onto themselves" and d_j from the observations predicted onto themselves.  fp64, one
 *     rounding per operation, no contraction; rho is compared by the total order of its bit patterns, as above.
 *  4. Row q lists the m candidates with the largest key, largest rho first, 1-based, zero-padded.
 * So the output is a function of the inputs alone; a row depends on no other row of the query set and on no chunking; the
 * table for m is the first m columns of the table for any m' > m; hops = 1 with m = m_cand returns P(q) as a set; under an
 * isotropic stationary theta every setting returns the Euclidean set (up to ties of rho's rounding); and n <= m_cand ranks
 * every observation.  host.vecchia_neighbours_corr_pred restates the rule in numpy.
 *
 * cocons_vecchia_neighbours_corr_pred: the table of mp new locations (locs_pred mp x 2, X_pred mp x p, column-major) on any
 * Vecchia handle; nn_out mp x m column-major.  The work runs in chunks of cocons_vecchia_info's out4[3] rows with device
 * memory that does not grow with mp.  The handle keeps what later calls use again and cocons_vecchia_info counts it: the grid
 * over the observations (cocons_vecchia_predict_knn's) and, with hops = 2, the table A -- n x m_cand ints, 120 MB at
 * n = 10^6 and m_cand = 30 --, made by the first call with two hops, made again by a call at another m_cand, freed with the
 * handle; hops = 1 never makes it.  Returns 0 (mp = 0: at once); the smallest 1-based row with a rho that is not finite
 * (nn_out untouched); -1 before any device work, nn_out untouched, for: a null argument, mp < 0, a handle that is not a
 * Vecchia handle, m_cand, hops or m out of range, m > min(4032, m_cand + m_cand^2 (hops - 1)), a theta or a coordinate that
 * is not finite.
 *
 * cocons_vecchia_predict_corr_knn: cocons_vecchia_predict with the table cocons_vecchia_neighbours_corr_pred returns, to the
 * bit, every chunk's table made on the device -- the query at m_cand, the chunk's records, the re-ranking, the prediction
 * launch --; no table goes up or down, and a row's outputs depend neither on the chunking nor on the other rows.  Refusals
 * as above and cocons_vecchia_predict_knn's, under this entry's name, outputs untouched; a rho that is not finite or a
 * failing block returns its 1-based row.
 *
 * cocons_fit_create_vecchia_grouped_corr_knn: cocons_fit_create_vecchia_grouped_knn with the table of
 * cocons_vecchia_neighbours_corr(theta, m_cand, hops, m) in the place of the Euclidean search: search, records at theta,
 * re-rank, rounds, plan, expanded table and adoption in one chain on the device.  The handle gives, in every entry grouped or
 * not, the bits of cocons_vecchia_neighbours_corr -> cocons_vecchia_group_rounds -> cocons_vecchia_group_table ->
 * cocons_fit_create_vecchia -> cocons_vecchia_set_groups.  NULL with the refusals of both parents under this entry's name. */
int cocons_vecchia_neighbours_corr_pred(cocons_fit *fit, const double *theta, int mp, const double *locs_pred,
                                        const double *X_pred, int m_cand, int hops, int m,
                                        int *nn_out /* mp x m column-major, 1-based, largest rho first, 0 = none */);
int cocons_vecchia_predict_corr_knn(cocons_fit *fit, const double *theta, const double *mean, int z_col, int mp,
                                    const double *locs_pred, const double *X_pred, int m_cand, int hops, int m_pred,
                                    double *stochastic, double *quadform);
cocons_fit *cocons_fit_create_vecchia_grouped_corr_knn(int n, int p, int r, const double *locs, const double *X,
                                                       const double *z, const double *smooth_limits, int device,
                                                       const double *theta, int m_cand, int hops, int m,
                                                       int max_rows, int max_rounds);

/* ---- Maxmin ordering on the device: scale-halving nets ------------------------------------------------------
 * The order of the observations a Vecchia fit wants: coarse to fine, every point at least half as far from its predecessors
 * as the farthest remaining point is.  The rule, here and in every reference (d2 as above: fl(fl(dx dx) + fl(dy dy)), fp64,
 * no contraction, no square root):
 *  1. Labels, a fixed pseudo-random bijection of the caller's indices 0 .. n - 1 onto 0 .. n - 1: with b the smallest integer
 *     >= 1 with 2^b >= n, mask = 2^b - 1 and s = (b + 1) / 2 (integer division), mix(v) is three rounds of
 *     v = (v C_j) & mask; v ^= v >> s, the product in 64 bits, C = 0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35; label(i) is the
 *     first of mix(i), mix(mix(i)), .. that is below n.  No seed, nothing random at run time.  A lower label is a higher
 *     priority.
 *  2. Level 0 is one point: the smallest key (d2(point, c), caller's index), c = (x0 + 0.5 (x1 - x0), y0 + 0.5 (y1 - y0)) the
 *     centre of the bounding box [x0, x1] x [y0, y1].
 *  3. Levels k = 1 .. 64: L = max(x1 - x0, y1 - y0), l_k = ldexp(L, 1 - k), e_k = fl(l_k l_k).  Two points conflict at level
 *     k iff d2 < e_k (strict).  Walk the points not yet ordered in ascending label and take a point iff it conflicts with
 *     nothing taken so far, at this level or any earlier one.  Inside a level the points stand in ascending label.  A level
 *     may be empty; the levels stop once every point is ordered.
 *  4. The rest: what is unordered after level 64 follows in ascending label (coincident points, pairs closer than L 2^-63).
 * Consequences: order is a permutation; for every position t >= 2 outside the rest, with m_t the smallest d2 from the point at
 * t to the points before it and M_t the largest such minimum over the points at or behind t, M_t < 4 m_t (e_(k-1) = 4 e_k
 * exactly while e_k is a normal number); the output is a function of the inputs alone, bit for bit, run to run.
 *
 * cocons_vecchia_order: stateless -- host buffers in and out, device memory of the call only.  locs n x 2 column-major.
 * order: n ints, 1-based: order[t] is the caller's row at position t + 1.  level_counts (may be NULL; room for 67 ints):
 * [0] = K + 2, the number of records that follow; then the size of level 0 (1), of the levels 1 .. K -- K the last level that
 * was walked, 0 for n = 1 --, and of the rest.
 * Refused (-1) before any HIP call, the outputs untouched, with a message that starts with the entry's name: null locs or
 * order, n < 1, a coordinate that is not finite, and a bounding box whose longer side exceeds 2^511 (d2 and e_1 must not
 * overflow).  Clustered or near-coincident points cost more rounds and larger cells, never a different bit.                */
int cocons_vecchia_order(int n, const double *locs, int device, int *order, int *level_counts /* may be NULL: 67 ints */);

/* ---- U^-1 on a Vecchia fit: fields and conditional draws of the Vecchia model -----------------------------
 * Observation i has the neighbours j_1 < .. < j_k, all earlier rows, and the block K = C C' with its rows in the order
 * (j_1 .. j_k, i), exactly as cocons_neg2loglik_vecchia builds it.  With s = C^-T e_last (the vector the gradient and the
 * information solve for) the whitening is y_i = sum_t s_t b_{j_t} + s_last b_i, and its inverse the recursion, in ascending i,
 *     x_i = ( w_i - sum_{t = 1 .. k} s_t x_{j_t} ) / s_last,
 * the sum over t ascending in one thread, no contraction.  x = U^-1 w has the covariance (U'U)^-1, the Vecchia model's Sigma;
 * with every predecessor in the table U^-1 is the lower Cholesky factor of Sigma(theta).  A row's result is a function of its
 * own coefficients and of its neighbours' results alone: it does not depend on the number of columns, on how the rows are
 * spread over launches (COCONS_VECCHIA_SIM_FUSE=0: one launch per level, no fused runs of small levels) or on the run.
 * The rows are solved level by level: level(i) = 0 for the rows i <= n_fixed, otherwise 1 + the largest level among the row's
 * neighbours (1 without neighbours).  The levels are computed on the device from the handle's table; the handle keeps the
 * schedule of the last n_fixed and n (m + 1) doubles of coefficients, recomputed per call; cocons_vecchia_info counts both.
 * Refused (-1) before any device work, outputs untouched, with a message that starts with the entry's name: a null argument,
 * c < 1, nsim < 1, n_fixed outside 0 .. n - 1, z_col outside the realisations, a handle that is not a Vecchia handle.  A
 * failing block returns its smallest 1-based row; nothing is written and the solve is not launched.  Outputs are written on
 * 0 only.
 * cocons_vecchia_unwhiten: out = U^-1 W, W and out n x c column-major in the caller's order: the inverse of
 * cocons_vecchia_whiten for the same theta.                                                                              */
int cocons_vecchia_unwhiten(cocons_fit *fit, const double *theta, int c, const double *W, double *out);
/* n_fixed = 0: out (n x nsim) = X mean + U^-1 E, cocoSim's marginal branch for a Vecchia handle; E = iiderrors (n x nsim) is
 * used as given.  1 <= n_fixed < n: the rows 1 .. n_fixed are data, x_i = z[i, z_col] - X_i mean, and the rows behind them run
 * the recursion; E and out are (n - n_fixed) x nsim and out_i = X_i mean + x_i.  With E = 0 that is the joint conditional mean
 * of the Vecchia model at the later rows, with N(0, 1) numbers a conditional draw.  The handle is made over (observations,
 * then new locations) with any z in the new rows: they are not read.                                                      */
int cocons_sim_vecchia(cocons_fit *fit, const double *theta, const double *mean, int n_fixed, int z_col,
                       int nsim, const double *iiderrors, double *out);
/* The schedule of (table, n_fixed): levels (n ints, may be NULL) and out4 = {depth, rows of the largest level, launches of one
 * solve of one column under the current COCONS_VECCHIA_SIM_FUSE, device bytes of the schedule and of the coefficients of a solve}.       */
int cocons_vecchia_schedule(cocons_fit *fit, int n_fixed, int *levels /* n, may be NULL */, long long *out4);

/* ---- U' on a Vecchia fit and cross-validation from Q = U'U -------------------------------------------------
 * The Vecchia model's precision is Q = U'U, U the sparse whitening above.  For a held-out set B with complement A and
 * R = z - X mean, the identities of cocons_cv_dense hold with K = Q:
 *     R_B - E[R_B | R_A] = (Q_BB)^-1 (Q R)_B,      Cov(R_B | R_A) = (Q_BB)^-1.
 * Q is never formed.  Definitions every entry below follows:
 *   Coefficients.  Row i of U holds s = C^-T e_last of the row's block: U(i, j_t) = s_t for the neighbour at place t of the
 *     handle's ascending table, U(i, i) = s_last.
 *   Transposed lists.  list(j) = the rows k (all > j) whose table row names j, in ascending k; a row names an index at most
 *     once, so k is unique within a list.  entries = the number of non-zero table entries.  The lists are a function of the
 *     table alone: built once per handle on the device by the first call that needs them, kept on the handle, counted by
 *     cocons_vecchia_info and freed with the handle.
 *   y = U b is formed from the rows' coefficients: y_i = sum_t s_t b_{j_t} + s_last b_i, t ascending, one thread, no
 *     contraction -- the formula of cocons_vecchia_unwhiten's text.  It need not be cocons_vecchia_whiten's bits, which come
 *     from a forward substitution through the block's factor.
 *   (U'w)_j = s_last(j) w_j + sum_{k in list(j)} U(k, j) w_k,     Q_jj = s_last(j)^2 + sum_{k in list(j)} U(k, j)^2.
 *     The order of summation is a fixed function of the list alone: one wavefront serves a column, lane l sums the entries
 *     l, l + 64, .. of the list in ascending order -- lane 0 starts from the own row's term --, and the 64 partial sums meet
 *     in a butterfly of fixed shape.  No floating-point atomics anywhere.
 *   Fold block.  For a fold B with members ascending, Q_BB[a, b] = sum_k U(k, a) U(k, b) over the rows k that hold both
 *     columns, in ascending k, the own row of the later index first.
 * Determinism: repeated calls agree to the bit; a fold's outputs depend on its members alone -- not on the labels, not on how
 * the other observations are grouped; a fold of one returns leave-one-out's bits; the outputs of cocons_vecchia_whiten_t do
 * not depend on c; no other Vecchia entry returns other bits before or after these calls, in any order.
 *
 * cocons_vecchia_transpose: ptr (n + 1 ints, may be NULL) the 0-based offsets of the lists, rows (entries ints, may be NULL)
 * the 1-based rows, ascending inside a list; out4 = {entries, longest list, device bytes of the lists, columns nobody names}.
 * A call with both NULL sizes the buffers.                                                                                */
int cocons_vecchia_transpose(cocons_fit *fit, int *ptr /* n + 1, may be NULL */, int *rows /* entries, may be NULL */,
                             long long *out4);
/* out (n x c) = U'W for W n x c column-major in the caller's order, qdiag (n, may be NULL) = diag(U'U).  Refused (-1) before
 * any device work, outputs untouched, the entry's name in front: a null argument, c < 1, a handle that is not a Vecchia
 * handle.  A failing block returns its smallest 1-based row and nothing is written.                                       */
int cocons_vecchia_whiten_t(cocons_fit *fit, const double *theta, int c, const double *W, double *out /* n x c: U'W */,
                            double *qdiag /* n: diag(U'U), may be NULL */);
/* Cross-validated predictions of the Vecchia model: fold, nfold, resid (n x r), var (n), the return codes and "outputs are
 * written on 0 only" as cocons_cv_dense; fold = NULL with nfold = 0 is leave-one-out; labels nobody carries are allowed;
 * R = z - X mean as cocons_neg2loglik_vecchia forms it.  An observation alone in its fold: var = 1 / Q_jj, resid =
 * (U'U R)_j var.  A fold of 2 .. 128 observations: one workgroup builds Q_BB in LDS and runs cocons_cv_dense's block
 * arithmetic on it.  stats4 (may be NULL) = {folds of one, folds of 2 .. 128, entries, device bytes the call allocated}.
 * Returns 0, the smallest failing 1-based block row (nothing written), -5 when a Q_BB is not positive definite in floating
 * point (the message names the fold), < 0 with cocons_last_error() otherwise.  Refused (-1) before any device work, outputs
 * untouched, the entry's name in front: a null argument, nfold < 0, fold and nfold that disagree, a label outside
 * [0, nfold), a fold that holds all n observations (leave-one-out at n = 1 is answered: resid = z - X mean, var = Sigma_11),
 * a fold of more than 128 observations -- a larger Q_BB is a sparse system of its own; a handle over the complement and
 * cocons_vecchia_predict_knn is the route for such folds --, a handle that is not a Vecchia handle.                       */
int cocons_cv_vecchia(cocons_fit *fit, const double *theta, const double *mean, int nfold, const int *fold,
                      double *resid /* n x r */, double *var /* n */, long long *stats4 /* may be NULL */);

/* ---- grouped Vecchia blocks: one factorisation for a group of rows ------------------------------------------
 * A block B is a set of member rows; S(B) is the union of its members and all their table neighbours, at most 64 rows.  The
 * member at position p of S(B) (ascending) conditions on the positions 0 .. p - 1: a superset of its own neighbours.  The
 * grouped model is therefore an ordinary Vecchia model on the EXPANDED table (m <= 63), and a handle made from that table
 * serves every Vecchia entry; the grouped entries below assemble and factor each block once and return the bits of the
 * ungrouped entries on the same handle.
 *
 * cocons_vecchia_group: the greedy rule on the host (Guinness 2018; GpGp's group_obs).  nn: n x m column-major, 1-based,
 * 0 = none, earlier rows only, m in 1 .. 63 (cocons_fit_create_vecchia's rules, checked); max_rows in 2 .. 64.  Every row
 * starts as a block of its own; the rows are visited in ascending order and, for each neighbour j of row i in the order the
 * row lists them (zeros skipped), the blocks A of i and B of j are merged when A != B, u = |S(A) u S(B)| <= max_rows and
 * u^2 < |S(A)|^2 + |S(B)|^2 -- integers only.  group[n]: 0-based block ids, numbered by their smallest member, ascending.
 * out4 (may be NULL) = {blocks, sum of |S| over the blocks, sum of |S| (|S| - 1) / 2 (the pairs the grouped schedule
 * evaluates), sum over the rows of (k + 1) k / 2 for k neighbours (the pairs of the ungrouped schedule on nn)}.             */
int cocons_vecchia_group(int n, int m, const int *nn, int max_rows, int *group, long long *out4);
/* The ROUND rule: another grouping of the same table, a function of the rows' neighbour SETS alone, stated in
 * synchronous rounds so that a device can run it.  A block's id is its smallest member; at the start every row is a block.
 * One round reads only the state at its start:
 *   1. every live block A looks at its candidates, the blocks B != A that hold a neighbour of a member of A.  With
 *      a = |S(A)|, b = |S(B)|, u = |S(A) u S(B)|, B is eligible when u <= max_rows and u^2 < a^2 + b^2 (the greedy rule's
 *      test); its gain is g = a^2 + b^2 - u^2.  prop(A) is the eligible candidate of the largest gain, ties to the smaller
 *      id, and key(A) = (8192 - g) << 32 | A.  A block without an eligible candidate proposes nothing;
 *   2. best(X) is the smallest key(A) over the proposing blocks A with A = X or prop(A) = X;
 *   3. the edge A -> prop(A) = B is realised when best(A) = best(B) = key(A).  Realised edges share no block; each merges its
 *      two blocks into the smaller id.
 * The rounds end with the first round that has no proposal, or after max_rounds rounds (>= 0; 0 means 256).  Integers only.
 * The partition is NOT the greedy one.  A row with more than max_rows - 1 neighbours never merges; every block a merge made
 * has |S| <= max_rows.  group[n] as cocons_vecchia_group's; out5 (may be NULL) = out4, then the rounds that merged something.
 * cocons_vecchia_group_rounds runs the rule on the host and needs no device.  cocons_vecchia_group_device runs it on the
 * device: one wavefront per live block proposes, 64-bit atomic minima carry the best keys, one wavefront per block merges;
 * the same labels and rounds, integer for integer.  Its scratch, n (4 max_rows + 36) + 8 bytes beside the table's 4 n m, is
 * memory of the call.
 * Refused (-1, the entry's name in front, outputs untouched, before any device work): a null nn or group, a table that
 * breaks cocons_fit_create_vecchia's rules, max_rows outside 2 .. 64, max_rounds < 0; cocons_vecchia_group_device also a
 * device that does not exist.                                                                                               */
int cocons_vecchia_group_rounds(int n, int m, const int *nn, int max_rows, int max_rounds, int *group, long long *out5);
int cocons_vecchia_group_device(int n, int m, const int *nn, int max_rows, int max_rounds, int device, int *group,
                                long long *out5);
/* The expanded table of ANY partition `group` (labels in 0 .. n - 1) of nn's rows: nn_out is n x m_out column-major, 1-based,
 * ascending, zero padded.  m_out = 0 with nn_out = NULL asks for the longest expanded row alone, which is returned (>= 0);
 * otherwise 0.  Refused (-1, the entry's name in front): a table that breaks the rules, a block with |S| > 64 (its smallest
 * member is named), m_out smaller than the longest expanded row or outside 1 .. 63.                                        */
int cocons_vecchia_group_table(int n, int m, const int *nn, const int *group, int m_out, int *nn_out);
/* Attach the plan of the partition `group` (n labels in 0 .. n - 1) to a Vecchia handle.  The handle's table must be CLOSED
 * under it: every member's stored row equals {s in S(block) : s < i}, and |S| <= 64; checked on the host before any device
 * work on the plan -- the table is downloaded once for the check, so a handle of cocons_fit_create_vecchia_knn is served as
 * well.  Refused with -1, the entry's name and the first offending row otherwise.  The plan lives on the handle, counts in
 * cocons_vecchia_info's bytes and is replaced by a second call.  COCONS_VECCHIA_GROUP_ORDER=0 (read here) deals the blocks to
 * the workgroups by block id instead of largest first; no bit of any output depends on it.                                 */
int cocons_vecchia_set_groups(cocons_fit *fit, const int *group);
/* {blocks, rows of the largest block, sum of |S|, pairs, device bytes of the plan} of the handle's plan                    */
int cocons_vecchia_groups_info(cocons_fit *fit, long long *out5);
/* cocons_vecchia_group, cocons_vecchia_group_table, cocons_fit_create_vecchia on the expanded table and
 * cocons_vecchia_set_groups in one call; the other arguments as cocons_fit_create_vecchia.  NULL with cocons_last_error().  */
cocons_fit *cocons_fit_create_vecchia_grouped(int n, int p, int r, const double *locs, const double *X, const double *z,
                                              const double *smooth_limits, int device, int m, const int *nn, int max_rows);
/* The grouped handle made where it is used: the ordered neighbour search (cocons_fit_create_vecchia_knn's),
 * the round rule, the plan and the expanded table, all on the device -- neither the searched table, nor the partition, nor
 * the expanded table reaches the host; home come the rounds' counters and the 65 counts of blocks by size.  The handle is the
 * one that cocons_vecchia_neighbours, cocons_vecchia_group_rounds, cocons_vecchia_group_table (at its longest row),
 * cocons_fit_create_vecchia and cocons_vecchia_set_groups give on the same data: the same table, the same
 * cocons_vecchia_groups_info, the same bits from every entry.  The closure check of cocons_vecchia_set_groups is satisfied by
 * construction and not rerun.  m in 1 .. 63 is the search's; cocons_vecchia_info's m is the expanded table's.  The scratch
 * of the rounds and of the plan is memory of the call.  NULL with cocons_last_error(); refused before any device work:
 * max_rows outside 2 .. 64, max_rounds < 0, and what cocons_fit_create_vecchia_knn refuses.                                 */
cocons_fit *cocons_fit_create_vecchia_grouped_knn(int n, int p, int r, const double *locs, const double *X, const double *z,
                                                  const double *smooth_limits, int device, int m, int max_rows, int max_rounds);
/* The partition and the table of a handle with a plan, read back: block[n] = the 0-based block of every row in the plan's
 * numbering (by smallest member), nn (may be NULL) = the handle's table, n x m column-major with cocons_vecchia_info's m,
 * 1-based, ascending, 0 = none.  Refused (-1): a null handle or block, a handle that is not a Vecchia handle or has no plan.  */
int cocons_vecchia_groups_export(cocons_fit *fit, int *block /* n */, int *nn /* n x m, may be NULL */);
/* cocons_neg2loglik_vecchia and cocons_vecchia_whiten on the grouped schedule: the same arguments, the same return codes --
 * the smallest failing 1-based row included --, outputs written on 0 only, and THE SAME BITS in value, parts, every whitened
 * value and every log d.  Refused (-1): a handle without a plan (cocons_vecchia_set_groups attaches one).                   */
int cocons_neg2loglik_vecchia_grouped(cocons_fit *fit, const double *theta, const double *mean, double *value,
                                      double *parts /* 1 + r, may be NULL */);
int cocons_vecchia_whiten_grouped(cocons_fit *fit, const double *theta, int c, const double *B /* n x c */,
                                  double *out /* n x c */, double *logd /* n, may be NULL */);
/* cocons_neg2loglik_grad_vecchia on the grouped schedule (value and gradient from one factorisation per BLOCK, every pair
 * of a block evaluated once): the same arguments, conventions, return codes and refusals -- B == NULL or given columns,
 * grad_quad and parts may be NULL, outputs written on 0 only, the smallest failing 1-based row.  sum_logliks and parts are
 * cocons_neg2loglik_vecchia_grouped's bits (and so the ungrouped entries'); the gradient is the same model's -- the handle's
 * table is the expanded one -- summed in another order: it agrees with cocons_neg2loglik_grad_vecchia on the same handle to
 * rounding, not to the bit, and repeats to the bit whatever COCONS_VECCHIA_GROUP_ORDER says.  Refused (-1): a handle without
 * a plan.                                                                                                                    */
int cocons_neg2loglik_grad_vecchia_grouped(cocons_fit *fit, const double *theta, const double *mean, int c, const double *B,
                                           double *sum_logliks, double *parts, double *grad_theta, double *grad_quad,
                                           double *grad_mean);
/* cocons_fisher_vecchia on the grouped schedule (one factorisation per BLOCK, every pair of a block evaluated
 * once per walk for all its members): the same arguments, conventions, return codes and refusals -- info_mean may be NULL,
 * info and info_mean symmetric to the bit, outputs written on 0 only, the smallest failing 1-based row, the same scratch on
 * the handle (cocons_vecchia_info reports the same bytes).  With rows S ascending, C = L L' and s_p row p of L^-1, the member
 * at position p gives g_{a,p} = L_{0..p}^-1 (C_a[0..p, 0..p] s_p) and u_p = sum_{row <= p} s_p[row] X[site(row), .]:
 *   info[a * ndir + b] = r sum_blocks sum_members ( sum_{j < p} g_{a,p}[j] g_{b,p}[j] + g_{a,p}[p] g_{b,p}[p] / 2 ),
 *   info_mean[k * p + l] = r sum_blocks sum_members u_p[k] u_p[l].
 * It is the same model's information -- the handle's table is the expanded one -- summed in another order: it agrees with
 * cocons_fisher_vecchia on the same handle to rounding, not to the bit, and repeats to the bit whatever
 * COCONS_VECCHIA_GROUP_ORDER says.  A direction count whose launch cannot fit the LDS is refused (-1) with the bytes in the
 * message.  Refused (-1): a handle without a plan (cocons_vecchia_set_groups attaches one).                                  */
int cocons_fisher_vecchia_grouped(cocons_fit *fit, const double *theta, int ndir, const double *dirs,
                                  double *info, double *info_mean);
/* U^-1, U' and cross-validation on the grouped schedule.  All four entries start from the rows' coefficients
 * s = C^-T e_last; here they come from one factorisation per BLOCK -- the member at position p solves backward on the leading
 * (p + 1) x (p + 1) sub-factor, component j = (e_p[j] - sum_{i > j} L(i, j) s[i]) / L(j, j) with i descending -- into the
 * same records, and everything behind them (the schedule, the level solve, the transposed lists, U'w, the fold blocks) is
 * the ungrouped entry's code.  Each entry has its twin's arguments, conventions, return codes -- the smallest failing 1-based
 * row among the rows that are not fixed included -- and refusals under its own name, writes its outputs on 0 only, and
 * repeats to the bit whatever COCONS_VECCHIA_GROUP_ORDER says.  Refused (-1): a handle without a plan
 * (cocons_vecchia_set_groups attaches one).
 * cocons_vecchia_unwhiten_grouped returns the bits of cocons_vecchia_unwhiten on the same handle.                          */
int cocons_vecchia_unwhiten_grouped(cocons_fit *fit, const double *theta, int c, const double *W, double *out);
/* cocons_sim_vecchia_grouped returns the bits of cocons_sim_vecchia on the same handle; with n_fixed > 0 the blocks whose
 * rows are all fixed do no work and a member row below n_fixed gets no record.                                              */
int cocons_sim_vecchia_grouped(cocons_fit *fit, const double *theta, const double *mean, int n_fixed, int z_col,
                               int nsim, const double *iiderrors, double *out);
/* cocons_vecchia_whiten_t_grouped returns the bits of cocons_vecchia_whiten_t on the same handle.                          */
int cocons_vecchia_whiten_t_grouped(cocons_fit *fit, const double *theta, int c, const double *W, double *out /* n x c: U'W */,
                                    double *qdiag /* n: diag(U'U), may be NULL */);
/* cocons_cv_vecchia_grouped returns the bits of cocons_cv_vecchia on the same handle.                                      */
int cocons_cv_vecchia_grouped(cocons_fit *fit, const double *theta, const double *mean, int nfold, const int *fold,
                              double *resid /* n x r */, double *var /* n */, long long *stats4 /* may be NULL */);

/* U^-T on a Vecchia handle, and the model's own covariance through it (GpGp's L_t_mult).  With the
 * coefficients of cocons_vecchia_unwhiten, U(i, j_t) = s_t and U(i, i) = s_last(i).  For 0 <= n_fixed < n let U_pp be the
 * block of U on the rows and columns >= n_fixed; the rows < n_fixed name nobody behind them, so Q_pp = U_pp' U_pp is the
 * precision of the later rows given the first n_fixed.
 *   THE TRANSPOSED SOLVE.  v = U_pp^-T w is the recursion in DESCENDING j = n - 1 .. n_fixed
 *       v_j = (w_j - sum_{k in list(j)} U(k, j) v_k) / s_last(j),
 * list(j) = the rows that name j (cocons_vecchia_transpose), all > j >= n_fixed: no list is clipped.  THE SUM OF A LIST is a
 * function of the list alone.  A list of at most W = 1024 rows (cocons_debug_vecchia_solve_t_tiers) is summed by one wavefront,
 * T = 64; a longer one by one workgroup, T = 1024.  Thread t adds the products U(k, j) v_k of the entries t, t + T, .. of the
 * ascending list, in that order, to a sum that starts at 0.0; the 64 sums of a wavefront meet in the butterfly
 * s += s(lane xor d), d = 32, 16, .. 1; with T = 1024 the sixteen wavefronts' sums are then added in ascending order, starting
 * from wavefront 0's.  One rounded product, one rounded sum (no contraction); no floating-point atomics; no workgroup waits
 * for another.
 *   THE TRANSPOSED LEVELS.  tlevel(j) = 0 for j < n_fixed, else 1 + the largest tlevel in list(j), 1 for an empty list; made
 * on the device (integer atomics) and kept on the handle next to cocons_vecchia_schedule's, keyed by n_fixed.  The rows are
 * solved level by level in ascending tlevel; runs of narrow levels go as one launch unless COCONS_VECCHIA_SOLVE_T_FUSE=0.
 * A result does not depend on the number of columns, on the group of 8 columns a column ran in, on the launches, on that
 * switch or on n_fixed: row j >= n_fixed of U_pp^-T w has the same bits for every n_fixed <= j when w agrees on the rows >= j.
 *   THE ENTRIES.  `grouped` = 0: the coefficients come from one wavefront per row; 1: from one factorisation per block of the
 * handle's plan (cocons_vecchia_set_groups; refused without one) -- the same records, the same bits behind them.  These
 * entries are new and nothing pins their argument lists, so one flag stands where the older entries have a second name.
 * cocons_vecchia_unwhiten_t: out = U^-T W (n x c, column-major); cocons_vecchia_whiten_t inverts it.
 * cocons_vecchia_cov_mult: out = U_pp^-1 U_pp^-T B -- one coefficient phase, the transposed solve, then
 * cocons_vecchia_unwhiten's forward solve with the fixed rows of x at zero.  n_fixed = 0: Sigma~ B, the covariance of the
 * Vecchia model, Sigma~ = (U'U)^-1; n_fixed > 0 on a handle over (observations, then new locations): Cov(new | data) B.
 * cocons_vecchia_cov_cols: cocons_vecchia_cov_mult on the unit columns e_(idx[q] - n_fixed), made on the device -- its bits
 * for those columns; an index may repeat.
 * cocons_vecchia_schedule_t mirrors cocons_vecchia_schedule: out4 = {depth, rows of the widest level, launches of one solve
 * of one column under the current switch, device bytes of the transposed schedule}; tlevels (may be NULL): tlevel of every row.
 * All: 0, or the smallest failing 1-based row that is not fixed (> 0: nothing written, no solve launched), or < 0 with a
 * message that starts with the entry's name; outputs are written on 0 only.  Refused (-1) before any device work: a null
 * argument, c or nidx < 1, grouped outside 0 / 1, n_fixed outside 0 .. n - 1, an index outside n_fixed + 1 .. n, a handle that
 * is not a Vecchia handle, grouped = 1 without a plan.  No other entry returns other bits before or after these calls.     */
int cocons_vecchia_unwhiten_t(cocons_fit *fit, const double *theta, int grouped, int c,
                              const double *W /* n x c */, double *out /* n x c: U^-T W */);
int cocons_vecchia_cov_mult(cocons_fit *fit, const double *theta, int grouped, int n_fixed, int c,
                            const double *B /* (n - n_fixed) x c */, double *out /* same: U_pp^-1 U_pp^-T B */);
int cocons_vecchia_cov_cols(cocons_fit *fit, const double *theta, int grouped, int n_fixed, int nidx,
                            const int *idx /* 1-based rows, each > n_fixed */, double *out /* (n - n_fixed) x nidx */);
int cocons_vecchia_schedule_t(cocons_fit *fit, int n_fixed, int *tlevels /* n, may be NULL */, long long *out4);

/* ---- fit handle: everything that is constant over an optimisation -------------
 * Created once per cocoOptim / getHessian call from the arguments the reference
 * passes unchanged to every GetNeg2loglikelihood* evaluation
 * (R/optim.R:237-259): locs, x_covariates (= mod_DM), z (n x r), optional
 * x_betas (n x q, Profile only), smooth.limits.  After creation only O(p) bytes
 * cross PCIe per evaluation.  `device` < 0 picks (pid-stable) device 0.
 * `n_extra_rows` reserves room for cocons_predict_dense (0 if unused).          */
cocons_fit *cocons_fit_create(int n, int p, int r, int q, const double *locs,
                              const double *X, const double *z, const double *x_betas,
                              const double *smooth_limits, int device);
void cocons_fit_destroy(cocons_fit *fit);

/* Fused -2 log-likelihood core: replaces the chain
 *   cov_rns -> base::chol (dpotrf) -> sum(log(diag)) -> forwardsolve (dtrsm) -> crossprod
 * of GetNeg2loglikelihood, R/neg2loglikelihood.R:195-218.
 * `mean` (length p) is theta_list$mean.  Outputs:
 *   *sum_logliks = sum_k [ n log(2 pi) + 2 logdet + || R^-T (z_k - X mean) ||^2 ]
 *   parts[0] = sum(log(diag(chol))), parts[1..r] = the r quadratic forms (may be NULL)
 * The penalty (.cocons.getPen, R/checkFunctions.R:474-492) is O(p) host work and
 * stays with the caller.                                                         */
int cocons_neg2loglik_dense(cocons_fit *fit, const double *theta, const double *mean,
                            double *sum_logliks, double *parts);

/* The value of cocons_neg2loglik_dense and its analytic gradient in one call: sum_logliks and parts as
 * there, grad_theta[t * p + k] = d sum_logliks / d theta[t * p + k] (6 x p, the table layout of theta: std.dev, scale,
 * aniso, tilt, smooth, nugget, as the kernels see them) and grad_mean[k] = d sum_logliks / d mean[k].  One factorisation
 * with the identity bordered under Sigma (L^-T beside L^-1 R), Sigma^-1 from it, one pass over the pairs; the sums have
 * a fixed order, so repeated calls agree bit for bit.  0, the failing minor k > 0 (no output written), or < 0 with a
 * message.  Refused (-1) on taper and sharded handles and on a handle without z.  The first call grows the handle's
 * matrix allocation once by n_pad^2 doubles (n_pad = n rounded up to 128), kept for the handle's lifetime; the
 * objective's own layout (its leading dimension, the second buffer of its factorisation schedule) does not change.   */
int cocons_neg2loglik_grad_dense(cocons_fit *fit, const double *theta, const double *mean,
                                 double *sum_logliks, double *parts,
                                 double *grad_theta, double *grad_mean);

/* Batch of nb independent evaluations of the same fit (the 1 + 2P points of one
 * finite-difference gradient, R/optim.R:237-259 with R/profile.R:11-12; getHessian's
 * 3 P (P+1)/2 points, R/getFunctions.R:979-1016).  thetas: nb x (6 p) row-major tables,
 * means: nb x p, values[nb] = sum_logliks of each, status[nb] = 0 or the failing minor k > 0.
 * Evaluations are pipelined over a few internal slots (COCONS_BATCH_SLOTS, default 2, each on the engine schedule) so the
 * latency-bound panel chain of one overlaps the updates and the assembly of the others.    */
int cocons_neg2loglik_batch(cocons_fit *fit, int nb, const double *thetas, const double *means,
                            double *values, int *status);

/* Profile / REML cores: replace R/neg2loglikelihood.R:132-160 and :254-287.
 * Both avoid chol2inv and the n x n P_mat through
 *   z' P z = ||L^-1 z||^2 - (Y'y)' (Y'Y)^-1 (Y'y),  Y = L^-1 Xb, y = L^-1 z.
 * profile: Xb = x_betas given at fit creation (q columns);
 * reml:    Xb = x_covariates (as the reference does, :273-276); `rank` = qr(X)$rank,
 *          computed by the caller.  parts[0] = sum(log(diag(chol))),
 * parts[1] = sum(log(diag(chol(W)))), parts[2 .. 2+r) = quadratic forms,
 * parts[2+r .. 2+r+nxb) = the GLS coefficients W^-1 Xb' Sigma^-1 rowSums(z)/r that cocoOptim
 * recovers after a pml/reml fit (R/optim.R:329-341); nxb = q (profile) or p (reml).
 * `parts` may be NULL, else must hold 2 + r + nxb doubles.                        */
int cocons_neg2loglik_profile(cocons_fit *fit, const double *theta,
                              double *sum_logliks, double *parts);
int cocons_neg2loglik_reml(cocons_fit *fit, const double *theta, int rank,
                           double *sum_logliks, double *parts);

/* The values of cocons_neg2loglik_profile / _reml and their analytic gradients in one call.  sum_logliks and
 * parts (may be NULL; 2 + r + nxb doubles, GLS coefficients included) exactly as the value entries define them; grad_theta is
 * the 6 x p table in theta's layout, as cocons_neg2loglik_grad_dense returns it.  There is no mean gradient: the mean is
 * profiled out.  One factorisation with [Z' ; Xb' ; I] bordered under Sigma; the contraction of the dense gradient runs on
 *   profile:  W = r Sigma^-1 - U U'                  U = Sigma^-1 (Z - Xb beta)
 *   reml:     W = r Sigma^-1 - U U' - r C C'         C = Sigma^-1 Xb chol(Xb' Sigma^-1 Xb)^-T
 * with fixed-order sums: repeated calls agree bit for bit.  0, the failing minor k > 0, -4 when Xb' Sigma^-1 Xb is not
 * positive definite, or < 0 with a message that starts with the entry's name; outputs are written on 0 only.  Refused (-1)
 * on taper and sharded handles, on a handle without z and (profile) without x_betas.  Memory as for
 * cocons_neg2loglik_grad_dense: while r + nxb <= 128 the matrix allocation is the one that entry grows.              */
int cocons_neg2loglik_profile_grad(cocons_fit *fit, const double *theta,
                                   double *sum_logliks, double *parts, double *grad_theta);
int cocons_neg2loglik_reml_grad(cocons_fit *fit, const double *theta, int rank,
                                double *sum_logliks, double *parts, double *grad_theta);

/* The tapered -2 log-likelihood of a taper handle (what cocons_neg2loglik_dense returns on it) and its analytic gradient
 * in one call.  S = T o C(theta) on the handle's pattern; with A = S^-1 R and W = r S^-1 - A A'
 *   d f / d theta_a = sum over the pattern of W_ij T_ij dC_ij / d theta_a,      d f / d mean = -2 X' A 1.
 * S^-1 is formed only where the pattern can be non-zero: a selected inverse on the tile envelope of the band factor, kept in
 * a second buffer of the band's shape (allocated by the first call, kept on the handle, freed with it).
 * sum_logliks and parts (may be NULL; 1 + r doubles) as cocons_neg2loglik_dense gives them on the same handle; grad_theta
 * the 6 x p table of the whole value in theta's layout (the aniso and tilt rows are exactly zero: they do not enter the
 * taper model); grad_quad (may be NULL) the same table for the quadratic forms alone, so that the log-determinant's part is
 * grad_theta - grad_quad (GetNeg2loglikelihoodTaperProfile's gradient is a combination of the two); grad_mean p doubles.
 * Fixed-order sums: repeated calls agree bit for bit.  0, the failing minor k > 0, or < 0 with a message that starts with
 * the entry's name; outputs are written on 0 only.  Refused (-1) on a dense handle, a sharded handle, a handle without z. */
int cocons_neg2loglik_grad_taper(cocons_fit *fit, const double *theta, const double *mean,
                                 double *sum_logliks, double *parts,
                                 double *grad_theta, double *grad_quad, double *grad_mean);

/* Expected (Fisher) information of the dense model at theta, from one factorisation:
 *   info[a * ndir + b] = (r / 2) tr(Sigma^-1 Sigma_a Sigma^-1 Sigma_b),   Sigma_a = sum_{t,k} dirs[a][t * p + k] dSigma / dtheta[t * p + k],
 *   info_mean[k * p + l] = r (X' Sigma^-1 X)[k, l]   (may be NULL; the block between mean and covariance parameters is 0),
 * r the handle's number of realisations.  This is the expected Hessian of -log-likelihood (half the objective
 * cocons_neg2loglik_dense returns) -- what getHessian (R/getFunctions.R:925-1034) estimates by second differences, without
 * the penalty -- positive semi-definite by construction; it is not the observed Hessian.  dirs: ndir tables of 6 x p in
 * theta's layout (row-major, ndir x 6 p), directions in table space under the conventions of grad_theta: scale k = 0 is the
 * global range, scale k >= 1 enters the site predictor with the factor 2, coincident pairs take the first site's diagonal,
 * pairs the reference rounds to 0 contribute 0.  The optimiser's vector maps linearly onto the table, so its P coordinates
 * are P directions.  info is symmetric to the bit; every sum has a fixed order, so repeated calls agree bit for bit.
 * 0, the failing minor k > 0, or < 0 with a message that starts with the entry's name; outputs are written on 0 only.
 * Refused (-1) before any device work: null arguments, ndir outside [1, 7 * COCONS_P_MAX], non-finite entries of dirs,
 * taper and sharded handles, a handle without z.  Memory: (ndir + 2) n_pad^2 doubles (n_pad = n rounded up to 128) and the
 * traces' partial sums are allocated for the call and released before it returns; a device that cannot hold them gives
 * < 0 with the bytes needed in the message.  The handle's matrix allocation is the one cocons_neg2loglik_grad_dense grows. */
int cocons_fisher_dense(cocons_fit *fit, const double *theta, int ndir, const double *dirs,
                        double *info, double *info_mean);

/* Expected information of the REML fit at theta, from one factorisation.  With X = x_covariates, the design
 * cocons_neg2loglik_reml profiles out, V = Sigma^-1 X, W = X' V and P = Sigma^-1 - V W^-1 V' (R/neg2loglikelihood.R:273-278),
 *   info[a * ndir + b] = (r / 2) tr(P Sigma_a P Sigma_b),   Sigma_a and dirs as for cocons_fisher_dense:
 * the expected Hessian of the negative restricted log-likelihood (half the objective cocons_neg2loglik_reml returns), i.e.
 * the Fisher information of the error contrasts K' z with K' X = 0.  Positive semi-definite by construction; no mean block
 * (REML has no mean parameters) and no penalty.  The reference has no counterpart (R/getFunctions.R:930).  info is symmetric
 * to the bit; every sum has a fixed order, so repeated calls agree bit for bit.  With n = p observations there are no error
 * contrasts: info is the zero matrix, exactly.  0, the failing minor k > 0 of Sigma, -4 when
 * X' Sigma^-1 X is not positive definite, or < 0 with a message that starts with the entry's name; info is written on 0 only.
 * Refused (-1) before any device work: null arguments, ndir outside [1, 7 * COCONS_P_MAX], non-finite entries of dirs, taper
 * and sharded handles, a handle without z, sizes beyond the product kernel's addressing.  Memory as for cocons_fisher_dense:
 * (ndir + 2) n_pad^2 doubles and the traces' partial sums belong to the call; the handle keeps what
 * cocons_neg2loglik_reml_grad makes it keep.                                                                              */
int cocons_fisher_reml(cocons_fit *fit, const double *theta, int ndir, const double *dirs, double *info);

/* Expected (Fisher) information of a tapered fit (a handle of cocons_fit_create_taper) at theta, exact or probed, on the band
 * factor the handle's objective produces.  With S = T o C(theta) = L L' in place of Sigma,
 *   info[a * ndir + b] = (r / 2) tr(S^-1 S_a S^-1 S_b),   S_a = T o sum_{t,k} dirs[a][t * p + k] dC / dtheta[t * p + k] (on the pattern),
 *   info_mean[k * p + l] = r (X' S^-1 X)[k, l]   (may be NULL; exact in both modes),
 * computed as the Gram matrix of the whitened rows e_k' L^-1 S_a L^-T over probe rows e_k:
 *   nprobe = 0, probes = NULL   the n unit vectors, in chunks: exact.  Cost O(ndir n^2 bandwidth): meant for n up to ~10^4.
 *   nprobe >= 1                 the caller's probes (n x nprobe, column-major; column k is probe k, its entry i belongs to the
 *                               caller's observation i), used as given with the weight r / (2 nprobe): Hutchinson's estimator
 *                               when E[e e'] = I (random +-1 entries), which is the caller's responsibility.
 * Either way info is a Gram matrix: symmetric to the bit and positive semi-definite by construction; every sum has a fixed
 * order, so the result is repeatable to the bit and does not depend on max_rows (probe rows per chunk, rounded as
 * cocons_krige_taper_prepare rounds it; 0 = the largest multiple of 64 with (ndir + 1) rows n_pad doubles within 1 GiB, at
 * most 16384) nor on the handle's buffer layout.  dirs as for cocons_fisher_dense (ndir tables of 6 x p), under the TAPER
 * gradient's conventions: the full scale vector (rho_i = e^(2 eta_scale,i), no global range, factor 1), a coincident pair
 * takes the diagonal value of the row site of the lower triangle, pairs the reference rounds to 0 contribute 0; the aniso and
 * tilt rows do not enter the taper model, a direction with only those gives an exactly zero row and column.
 * 0, the failing minor k > 0, or < 0 with a message that starts with the entry's name; outputs are written on 0 only.
 * Refused (-1) before any device work: null fit, theta, dirs or info, ndir outside [1, 7 * COCONS_P_MAX], nprobe < 0,
 * nprobe > 0 without probes or probes with nprobe = 0, max_rows < 0, non-finite entries of dirs or probes, a dense handle, a
 * sharded handle, a handle without z.  Memory: two packed copies of the envelope's tiles, ndir values per stored entry and
 * the chunk's (ndir + 1) rows n_pad doubles belong to the call and are released before it returns (a device that cannot
 * hold them gives < 0 with the bytes needed in the message); the kriging and gradient states of the handle are neither read
 * nor written. */
int cocons_fisher_taper(cocons_fit *fit, const double *theta, int ndir, const double *dirs,
                        int nprobe, const double *probes, int max_rows, double *info, double *info_mean);

/* Cross-validated predictions at theta from one factorisation.  With K = Sigma^-1, U = K (z - X mean) and B a
 * held-out set of observations with complement A,
 *   z_B - E[z_B | z_A] = (K_BB)^-1 U_B,   Cov(z_B | z_A) = (K_BB)^-1:
 * every fold costs one block of K, gathered, factored and inverted, behind the one bordered factorisation of
 * cocons_neg2loglik_grad_dense.  fold: n labels in [0, nfold) in the caller's observation order (labels nobody carries are
 * allowed); fold = NULL with nfold = 0: leave-one-out.  resid (n x r, column-major, the caller's order):
 *   resid[i + k n] = z[i, k] - E[z[i, k] | the observations outside i's fold];   var[i] (length n): the predictive variance
 * of observation i (nugget included) given the observations outside its fold, the same for every realisation.
 * Every sum has a fixed order: two calls agree bit for bit, and a fold's outputs depend only on which observations it holds.
 * 0, the failing minor k > 0 of Sigma, -5 when a hold-out block of Sigma^-1 is not positive definite in floating point (the
 * message names the fold), or < 0 with a message that starts with the entry's name; outputs are written on 0 only.
 * Refused (-1) before any device work: null arguments, nfold < 0, fold and nfold that disagree, a label outside [0, nfold),
 * a fold that holds all n observations, taper and sharded handles, a handle without z.  (Leave-one-out of n = 1 is answered:
 * nothing is left to predict from, resid is z - X mean and var is Sigma_11.)  The handle keeps what
 * cocons_neg2loglik_grad_dense makes it keep; everything else belongs to the call.                                        */
int cocons_cv_dense(cocons_fit *fit, const double *theta, const double *mean,
                    int nfold, const int *fold, double *resid, double *var);

/* Leave-one-out for the tapered model S = T o C(theta) on a taper handle, from the selected inverse of
 * cocons_neg2loglik_grad_taper: resid[i + k n] = (S^-1 R)[i, k] / (S^-1)_ii, var[i] = 1 / (S^-1)_ii.  Returns and contracts
 * as cocons_cv_dense; refused (-1) for null arguments, dense and sharded handles and a handle without z.                   */
int cocons_cv_taper(cocons_fit *fit, const double *theta, const double *mean,
                    double *resid, double *var);

/* Cross-validation by folds for the tapered model, from ONE selected inverse and one more band factorisation (DESIGN.md 4l,
 * continued) instead of a refit per fold.  fold, nfold, resid, var, the return codes, the -5 message naming the fold and
 * "outputs are written on 0 only" are cocons_cv_dense's, for S = T o C(theta) on a taper handle; fold = NULL with nfold = 0
 * is leave-one-out and returns the bits of cocons_cv_taper.  Observations alone in their fold take cocons_cv_taper's closed
 * form (its bits).  A fold B of two or more costs K_BB = V V' with V = E_B' L^-T: its observations go through the
 * sliding-window band solve of cocons_krige_taper_apply as unit rows, in chunks of whole 128-row tiles (folds of up to 128
 * packed into tiles, a larger fold from a tile boundary on), and the product is accumulated fold by fold while the window
 * slides -- nothing is formed between different folds.  max_rows: rows per chunk, rounded up to 128; 0 = as many as keep the
 * ring and the blocks of a chunk within 1 GiB, at most 16384 (a fold larger than that gets a chunk of its own size).
 * Every sum has a fixed order: two calls agree bit for bit, and a fold's outputs depend only on which observations it holds
 * -- not on the labels, on how the other observations are grouped, on max_rows or on the depth of the Gram product's groups
 * (COCONS_CV_GRAM_DEPTH, 1 .. 16, default 8).
 * stats5 (may be NULL, written on 0): folds of one observation, folds of 2 .. 128, larger folds, chunks run, device bytes
 * allocated by the call (released before it returns; a device that cannot hold them gives < 0 with the bytes needed in the
 * message).  Refused (-1) before any device work: null arguments, nfold < 0, fold and nfold that disagree, a label outside
 * [0, nfold), a fold that holds all n observations, max_rows < 0, dense and sharded handles, a handle without z.
 * The handle keeps what cocons_neg2loglik_grad_taper makes it keep; a prepared kriging state is neither read nor written. */
int cocons_cv_taper_folds(cocons_fit *fit, const double *theta, const double *mean,
                          int nfold, const int *fold, int max_rows,
                          double *resid, double *var, long long *stats5);

/* Dense kriging core: replaces R/predict.R:136-183
 *   observed_cov <- cov_rns(...); cov_pred <- cov_rns_pred(...);
 *   inv_cov <- solve(observed_cov, t(cov_pred)); crossprod(resid, inv_cov);
 *   rowSums(cov_pred * t(inv_cov))
 * with one bordered Cholesky (Sigma is SPD) instead of LU.  Uses the first
 * realization column `z_col` of the fit's z.  Outputs (length m):
 *   stochastic[i] = c_i' Sigma^-1 (z - X mean),  quadform[i] = c_i' Sigma^-1 c_i     */
int cocons_predict_dense(cocons_fit *fit, const double *theta, const double *mean,
                         int z_col, int m, const double *locs_pred, const double *X_pred,
                         double *stochastic, double *quadform);

/* Rows of the covariance (cor = 0) or correlation (cor != 0, stats::cov2cor) matrix of the fit's
 * locations without forming the n x n matrix: what getCovMatrix's consumers read of it --
 * plot(type = "correlations") uses tmp_cov[ww, ] only (R/methods.R:161-165, :210-214; cov_rns at
 * R/getFunctions.R:44-52).  idx: nidx 0-based row indices in the caller's (original) observation order;
 * classic != 0 selects cov_rns_classic; out: nidx rows of n doubles (row b at out + b * n).
 * O(n p) bytes go down and nidx * n doubles come back instead of the 8 n^2-byte matrix.               */
int cocons_cov_rows(cocons_fit *fit, const double *theta, int classic, int nidx, const int *idx, int cor,
                    double *out);

/* Marginal simulation core: replaces R/sim.R:147-172
 *   covmat <- cov_rns(...) | cov_rns_classic(...); cholS <- chol(covmat);
 *   t(sweep(t(iiderrors) %*% cholS, 2, x %*% mean, "+"))
 * iiderrors and out are n x nsim column-major (the caller draws the N(0,1) numbers, as the
 * reference does with rnorm); classic != 0 selects cov_rns_classic.                        */
int cocons_sim_dense(cocons_fit *fit, const double *theta, const double *mean, int classic,
                     int nsim, const double *iiderrors, double *out);

/* Conditional simulation core: replaces R/sim.R:84-127 (cov_rns, cov_rns_pred, cov_rns on the new
 * locations, solve, chol of the Schur complement, cocoPredict(type = "mean")) by ONE Cholesky of the
 * joint covariance of (observed, new) locations.  locs_pred = newlocs (cross-covariance),
 * locs_unobs = the coordinates the reference hands to cov_rns for covmat_unobs (the first two
 * columns of newdataset, :96-99); iiderrors / out are m x nsim column-major.               */
int cocons_sim_cond_dense(cocons_fit *fit, const double *theta, const double *mean, int z_col,
                          int m, const double *locs_pred, const double *X_pred,
                          const double *locs_unobs, int nsim, const double *iiderrors, double *out);

/* Dense Cholesky of a caller-supplied SPD matrix (host, n x n column-major, lower
 * triangle read) with nrhs right-hand sides: replaces base::chol + forwardsolve
 * (R/neg2loglikelihood.R:200,214) for callers that already hold Sigma.
 * L (optional, n x n) receives the lower factor (= t(chol(Sigma))), Y (optional,
 * n x nrhs) receives L^-1 rhs, logdet_half = sum(log(diag(L))).                   */
int cocons_chol_solve(int n, const double *A, int nrhs, const double *rhs,
                      double *L, double *Y, double *logdet_half);

/* ---- measurement hooks (bench.py / rocprof): device-resident, no host copies ---
 * Runs `reps` complete evaluations of cocons_neg2loglik_dense back to back on the
 * fit's stream with HIP events around each stage.  ms[0]=assembly, ms[1]=Cholesky
 * (+solve, fused), ms[2]=reductions, ms[3]=whole evaluation, ms[4]=average duration
 * of one trailing-update (MFMA) launch, ms[5]=number of such launches per
 * evaluation, ms[6]=sum of trailing-update launch durations per evaluation,
 * ms[7]=algorithmic flops of those launches (K m (m+1) + 2 K r m each; m = trailing order),
 * ms[8]=duration of the ONE persistent launch that runs the head of the factorisation under the
 * dependency-driven schedule (it is also the first of the launches counted in ms[5..7]; 0 when the
 * classic schedule ran), ms[9]=the update flops inside it.  `ms` must hold 10 doubles.           */
int cocons_fit_profile(cocons_fit *fit, const double *theta, const double *mean,
                       int reps, double *ms);

/* State of the resident diagonal-block engine of a dense handle: out[0] = 1 if the last
 * completed operation ran on the engine schedule (0: plain schedule -- small n, a band-limited taper fit, a batch
 * slot, COCONS_ENGINE=0, or the back-off after a time-out), out[1] = hand-off time-outs in the life of the handle
 * (each was answered by ONE repeat of that operation on the plain schedule, then 2, 4 ... 64 further operations
 * stay on it before the engine is tried again), out[2] = the abort code of the last time-out (0 = none).  No
 * reference counterpart: the observability of a mechanism the reference does not have.                       */
int cocons_fit_engine_state(cocons_fit *fit, int *out3);

/* ---- natively sharded evaluation across the GPUs of one node ----------------------
 * Sigma is ROW-BLOCK partitioned (block b = rows 256 b .. 256 b + 255; blocks dealt in groups, see
 * cocons_shard_block_owner below): a rank assembles, solves and updates ITS rows of every column.  Per 256-column
 * block the owner of the diagonal block factors it and the library broadcasts it (0.56 MB, RCCL over xGMI, issued in
 * front of the bulk exchange; COCONS_SHARD_COMM2=1: on a stream -- and communicator -- of its own), every rank solves its rows of
 * the panel, the owner of the NEXT diagonal block updates and factors it from its own rows at once, the solved rows
 * are all-gathered packed by owner (second communication stream), every rank updates its rows of the trailing
 * matrix; the 1 + r^2 partial sums (+ the failing minor) are all-reduced at the end.  No
 * data-path call leaves the library: once a fit has collectives, cocons_neg2loglik_dense on it IS the sharded
 * evaluation and returns the same value on every rank.
 *
 * (a) one process per GPU (torch.distributed.run, MPI, optimParallel workers ...): rank 0 calls
 *     cocons_comm_unique_id, the 128 bytes reach the other ranks by whatever channel the host has, and
 *     every rank calls cocons_fit_comm_init on its own fit (ncclCommInitRank).
 * (b) one process, several GPUs (what a single R session needs, R/optim.R:117-121's single-caller model):
 *     cocons_multi_create takes the device list (ncclCommInitAll), cocons_multi_neg2loglik_dense drives
 *     all of them from the calling thread.
 * (c) tests / other transports: cocons_fit_set_collectives installs caller-provided broadcast and
 *     all-reduce functions (e.g. gloo when several ranks share one GPU, which RCCL refuses).           */
#define COCONS_UNIQUE_ID_BYTES 128
int cocons_comm_unique_id(void *id_out /* COCONS_UNIQUE_ID_BYTES */);
int cocons_fit_comm_init(cocons_fit *fit, int nranks, int rank, const void *id /* COCONS_UNIQUE_ID_BYTES */);
/* broadcast `bytes` at device pointer dev_ptr from rank `root` to every rank; `stream` (hipStream_t) is the
 * library's communication stream for these broadcasts (ordered behind whatever produced / last read the buffer):
 * the function may enqueue on it or block.  Return 0 on success.        */
typedef int (*cocons_bcast_fn)(void *user, void *dev_ptr, long long bytes, int root, void *stream);
/* in-place all-reduce of `count` HOST doubles, op 0 = sum, 1 = min; blocking.                            */
typedef int (*cocons_allreduce_fn)(void *user, double *host_inout, int count, int op);
int cocons_fit_set_collectives(cocons_fit *fit, int rank, int world, cocons_bcast_fn bcast,
                               cocons_allreduce_fn allreduce, void *user);
/* ... and the all-gather of the sharded evaluation: dev_buf holds `world` slots of bytes_per_rank bytes, slot r is
 * rank r's contribution (already in place on rank r); on return every slot is filled on every rank.  `stream`: the
 * stream the library has ordered the buffer's producer on (synchronise it, or enqueue behind it).  0 = ok.        */
typedef int (*cocons_allgather_fn)(void *user, void *dev_buf, long long bytes_per_rank, void *stream);
int cocons_fit_set_allgather(cocons_fit *fit, cocons_allgather_fn allgather);
/* number of ranks the fit is sharded over (1 = not sharded) */
int cocons_fit_world(cocons_fit *fit);

typedef struct cocons_multi cocons_multi;   /* one fit per device + their communicators */
cocons_multi *cocons_multi_create(int n, int p, int r, const double *locs, const double *X, const double *z,
                                  const double *smooth_limits, int ndev, const int *devices);
void cocons_multi_destroy(cocons_multi *m);
/* same outputs as cocons_neg2loglik_dense */
int cocons_multi_neg2loglik_dense(cocons_multi *m, const double *theta, const double *mean,
                                  double *sum_logliks, double *parts);

/* cocoPredict's dense core (cocons_predict_dense) with the m prediction locations split over the devices of
 * the handle: no exchange, slices concatenated on the host (BASELINE config C5).                         */
int cocons_multi_predict_dense(cocons_multi *m, const double *theta, const double *mean, int z_col,
                               int m_pred, const double *locs_pred, const double *X_pred,
                               double *stochastic, double *quadform);
/* Replica mode inside ONE process: the nb independent parameter points of a finite-difference
 * gradient (R/optim.R:256-259, 1 + 2P points) or of getHessian (R/getFunctions.R:979-1016) dealt over the devices
 * of the handle (point i on device i mod ndev), every device running its share through cocons_neg2loglik_batch on its
 * own fit; no collective, so the handle may list a device more than once.  Arguments as cocons_neg2loglik_batch. */
int cocons_multi_neg2loglik_batch(cocons_multi *m, int nb, const double *thetas, const double *means,
                                  double *values, int *status);
/* What the communicators really span: *ndev = devices of the handle, *rccl_count = ncclCommCount of its first
 * communicator (0: no communicator -- a device is listed twice).                                                  */
int cocons_multi_comm_ranks(cocons_multi *m, int *ndev, int *rccl_count);
/* The same for a fit with collectives of its own (cocons_fit_comm_init / cocons_fit_set_collectives): ncclCommCount,
 * ncclCommUserRank, ncclCommCuDevice (or the caller-provided world / rank and the fit's device).  bench.py prints
 * them for every rank.                                                                                            */
int cocons_fit_comm_info(cocons_fit *fit, int *count, int *user_rank, int *device);

/* ---- how the sharded evaluation deals the matrix (no GPU call) ----------------------------------------
 * Sigma is ROW-BLOCK partitioned: block b = rows 256 b ... 256 b + 255 (the reference's chol walks the upper
 * triangle row block by row block, R/neg2loglikelihood.R:200); blocks are dealt in groups of G consecutive
 * blocks, owner(b) = (b / G) mod world (COCONS_SHARD_GROUP, default 4).  Per block: its owner factors the
 * 256 x 256 diagonal block and broadcasts it (0.5 MB), every rank solves ITS rows of the panel, the solved
 * rows are all-gathered, every rank updates its rows.                              */
int cocons_shard_block_owner(int b, int world);
int cocons_shard_num_blocks(cocons_fit *fit);
/* 1 if the handle holds exactly these data (bitwise comparison with the host copies it keeps), else 0.  Host work only.
 * The R glue's handle cache (glue/cocons_hip_glue.c, _cocons_hip_fit_cached) calls it when its O(1) address check
 * misses, so that GetNeg2loglikelihood(theta, par.pos, locs, x_covariates, smooth.limits, z, n, lambda) -- the
 * reference's signature, R/neg2loglikelihood.R:183-191, no handle argument -- finds its handle without hashing the data. */
int cocons_fit_same_data(cocons_fit *fit, int n, int p, int r, int q, const double *locs, const double *X,
                         const double *z, const double *x_betas, const double *smooth_limits);
/* HIP stream the fit launches on (hipStream_t as void*), so the caller can order
 * collectives against it. */
void *cocons_fit_stream(cocons_fit *fit);
/* launch on a caller-owned stream instead (hipStream_t as void*; NULL = default stream).  The call waits until the
 * handle's streams AND the new stream are idle.  A handle that uses the resident diagonal-block engine then tests, inside
 * this call, that its engine stream runs beside the new stream (two one-lane probe kernels, one of them on the caller's
 * stream); on a clash the library redraws its OWN engine stream, and when no draw is clash-free the handle takes the
 * plain schedule (same values to 1e-12, cocons_fit_engine_state reports active = 0) until another stream is installed.
 * The NULL stream is never probed: a handle on it takes the plain schedule.  Results are bit-identical to those on the
 * handle's own stream whenever the schedule is the same.                                                              */
int cocons_fit_set_stream(cocons_fit *fit, void *stream);
int cocons_fit_sync(cocons_fit *fit);

#ifdef __cplusplus
}
#endif
#endif /* COCONS_HIP_H */
