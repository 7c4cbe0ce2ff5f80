# glue/R/cocons_hip.R -- R side of the HIP drop-in: replaces the BODIES of the reference's objective
# closures (R/neg2loglikelihood.R:127-291); names, arguments and return values are unchanged, so
# cocoOptim / getHessian / cocoPredict / cocoSim call them as before.  The thin wrappers of
# R/RcppExports.R (cov_rns, cov_rns_classic, cov_rns_pred, cov_rns_taper*, sumsmoothlone) stay as they
# are: only the native symbols behind them change (glue/cocons_hip_glue.c).
#
# The device-resident data of a fit live in an explicit handle (external pointer).  Callers that hold
# one pass it as `fit = `; otherwise -- cocoOptim calls the closures with the reference's signatures, which have no
# handle -- the native side keeps up to eight handles per process and finds the right one in O(1) by the addresses and
# dimensions of (locs, x_covariates, z, x_betas) and smooth.limits.  An address is a sound key because the cached objects
# are PRESERVED (no other object can get the address) and marked NOT MUTABLE (R code that modifies one must duplicate
# it first: new address, miss, data compared), and a hit is confirmed against the handle's copy of the data; only when
# the addresses miss are the data compared with every cached handle, and only then is a handle created
# (glue/cocons_hip_glue.c, _cocons_hip_fit_cached).  No hash of the data on any path, no package beyond base R.
# cocons_hip_forget() drops the cached handles and releases the objects they key on.

cocons_hip_fit <- function(locs, x_covariates, z, smooth.limits, x_betas = NULL, device = NULL) {
  if (is.null(device)) {
    ndev <- max(1L, .Call(`_cocons_hip_device_count`))
    device <- as.integer(Sys.getenv("COCONS_HIP_DEVICE", Sys.getpid() %% ndev))   # worker -> GPU map
  }
  z <- as.matrix(z)
  storage.mode(locs) <- storage.mode(x_covariates) <- storage.mode(z) <- "double"
  if (!is.null(x_betas)) { x_betas <- as.matrix(x_betas); storage.mode(x_betas) <- "double" }
  .Call(`_cocons_hip_fit_create`, locs, x_covariates, z, x_betas, as.double(smooth.limits), as.integer(device))
}

.cocons.hip.cached <- function(locs, x_covariates, z, smooth.limits, x_betas = NULL) {
  if (!is.matrix(z)) z <- as.matrix(z)                     # (no copy when the caller passes a matrix, as cocoOptim does)
  if (!is.double(locs) || !is.double(x_covariates) || !is.double(z) || (!is.null(x_betas) && !is.double(x_betas)) ||
      !is.double(smooth.limits)) {                           # integer inputs: converted once per call -- the rare path
    storage.mode(locs) <- storage.mode(x_covariates) <- storage.mode(z) <- "double"
    if (!is.null(x_betas)) storage.mode(x_betas) <- "double"
    smooth.limits <- as.double(smooth.limits)
  }
  .Call(`_cocons_hip_fit_cached`, locs, x_covariates, z, x_betas, smooth.limits, -1L)   # -1: worker -> GPU map, natively
}

cocons_hip_forget <- function() invisible(.Call(`_cocons_hip_cache_clear`))

.cocons.hip.result <- function(res, safe) {       # the reference's tryCatch contract, :200-206
  if (res[[1]] > 0L) {
    if (safe) return(NULL) else stop("Cholesky error")
  }
  res[[2]]
}

GetNeg2loglikelihood <- function(theta, par.pos, locs, x_covariates, smooth.limits, z, n, lambda,
                                 safe = TRUE, fit = NULL) {
  theta_list <- cocons::getModelLists(theta = theta, par.pos = par.pos, type = "diff")     # :193
  if (is.null(fit)) fit <- .cocons.hip.cached(locs, x_covariates, z, smooth.limits)
  val <- .cocons.hip.result(.Call(`_cocons_hip_neg2loglik`, fit, theta_list[-1], theta_list$mean), safe)
  if (is.null(val)) return(1e+06)
  val + .cocons.getPen(n * dim(as.matrix(z))[2], lambda, theta_list, smooth.limits)          # :220
}

# value and analytic gradient of the -2 log-likelihood core (no penalty): list(value, table = 6 x p gradient over
# std.dev, scale, aniso, tilt, smooth, nugget as getModelLists(type = "diff") gives them, mean = gradient over theta$mean);
# NULL after a failing Cholesky under safe.  INTEGRATION.md shows the gr = of cocoOptim built on it.
.cocons.hip.neg2loglik.grad <- function(fit, theta_list, safe = TRUE) {
  res <- .cocons.hip.result(.Call(`_cocons_hip_neg2loglik_grad`, fit, theta_list[-1], theta_list$mean), safe)
  if (is.null(res)) return(NULL)
  list(value = res[[1]], table = res[[2]], mean = res[[3]])
}

# expected (Fisher) information of the dense model over theta (the optimiser's vector), P x P in theta's order, from one
# factorisation: E[getHessian] at the model, without the penalty (INTEGRATION.md).  getModelLists(type = "diff") is affine, so
# column a of the Jacobian is getModelLists(theta + e_a) - getModelLists(theta); the table parts go to the device as directions,
# the mean parts give Jm' (r X' Sigma^-1 X) Jm.  NULL after a failing Cholesky under safe.
.cocons.hip.fisher <- function(fit, theta, par.pos, safe = TRUE) {
  aspects <- c("std.dev", "scale", "aniso", "tilt", "smooth", "nugget")
  base <- cocons::getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  p <- length(base$mean)
  flat <- function(tl) c(tl$mean, unlist(tl[aspects], use.names = FALSE))
  J <- vapply(seq_along(theta), function(a) {
    e <- theta
    e[a] <- e[a] + 1
    flat(cocons::getModelLists(theta = e, par.pos = par.pos, type = "diff")) - flat(base)
  }, numeric(7 * p))
  Jm <- J[seq_len(p), , drop = FALSE]
  Jt <- J[-seq_len(p), , drop = FALSE]
  cov <- which(colSums(Jt != 0) > 0)              # (a pure mean parameter costs no product on the device)
  res <- .cocons.hip.result(.Call(`_cocons_hip_fisher`, fit, base[-1], Jt[, if (length(cov)) cov else 1L, drop = FALSE]), safe)
  if (is.null(res)) return(NULL)
  info <- crossprod(Jm, res[[2]] %*% Jm)
  if (length(cov)) info[cov, cov] <- info[cov, cov] + res[[1]]
  info
}

# expected information of the REML fit over theta (cocons_fisher_reml), P x P in theta's order, from one factorisation:
# (r / 2) tr(P Sigma_a P Sigma_b) with the REML projector P (INTEGRATION.md).  solve() of it is the inv.hess of getCIs /
# getModHess for a reml object; the reference has no counterpart.  REML has no mean parameters: par.pos$mean holds no free
# entry.  NULL after a failing Cholesky under safe.
.cocons.hip.fisher_reml <- function(fit, theta, par.pos, safe = TRUE) {
  aspects <- c("std.dev", "scale", "aniso", "tilt", "smooth", "nugget")
  base <- cocons::getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  p <- length(base$mean)
  flat <- function(tl) c(tl$mean, unlist(tl[aspects], use.names = FALSE))
  J <- vapply(seq_along(theta), function(a) {
    e <- theta
    e[a] <- e[a] + 1
    flat(cocons::getModelLists(theta = e, par.pos = par.pos, type = "diff")) - flat(base)
  }, numeric(7 * p))
  if (any(J[seq_len(p), ] != 0)) stop("par.pos has a free mean entry; the REML objective has no mean parameters")
  .cocons.hip.result(.Call(`_cocons_hip_fisher_reml`, fit, base[-1], J[-seq_len(p), , drop = FALSE]), safe)
}

# expected information of a tapered fit (type = "sparse") over theta (cocons_fisher_taper), P x P in theta's order, on the band
# factor of one factorisation: (r / 2) tr(S^-1 S_a S^-1 S_b) with S = T o C(theta), a Gram matrix (symmetric, positive
# semi-definite).  nprobe = 0: exact, O(P n^2 bandwidth); nprobe > 0: Hutchinson's estimate from that many random +-1 probes
# over the n observations (set.seed() beforehand for a repeatable draw); the mean block is exact either way.  fit: a taper handle.  NULL after a
# failing Cholesky under safe.  INTEGRATION.md has the details.
.cocons.hip.fisher.taper <- function(fit, theta, par.pos, nprobe = 0L, n = NULL, max.rows = 0L, safe = TRUE) {
  aspects <- c("std.dev", "scale", "aniso", "tilt", "smooth", "nugget")
  base <- cocons::getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  p <- length(base$mean)
  flat <- function(tl) c(tl$mean, unlist(tl[aspects], use.names = FALSE))
  J <- vapply(seq_along(theta), function(a) {
    e <- theta
    e[a] <- e[a] + 1
    flat(cocons::getModelLists(theta = e, par.pos = par.pos, type = "diff")) - flat(base)
  }, numeric(7 * p))
  Jm <- J[seq_len(p), , drop = FALSE]
  Jt <- J[-seq_len(p), , drop = FALSE]
  cov <- which(colSums(Jt != 0) > 0)
  probes <- NULL
  if (nprobe > 0) {
    if (is.null(n)) stop("nprobe > 0 needs n, the number of observations of the fit")
    probes <- matrix(sample(c(-1, 1), n * nprobe, replace = TRUE), n, nprobe)
  }
  res <- .cocons.hip.result(.Call(`_cocons_hip_fisher_taper`, fit, base[-1], Jt[, if (length(cov)) cov else 1L, drop = FALSE],
                                  probes, as.integer(max.rows)), safe)
  if (is.null(res)) return(NULL)
  info <- crossprod(Jm, res[[2]] %*% Jm)
  if (length(cov)) info[cov, cov] <- info[cov, cov] + res[[1]]
  info
}

# cross-validated predictions at theta_list from ONE factorisation (cocons_cv_dense): every observation predicted from the
# observations outside its fold.  fold: one label of any kind per observation (NULL: leave-one-out).  list(resid = z minus
# its prediction, n x r; var = the predictive variance, nugget included); NULL after a failing Cholesky under safe.
# INTEGRATION.md shows a cross-validated CRPS built on it.
.cocons.hip.cv <- function(fit, theta_list, fold = NULL, safe = TRUE) {
  if (!is.null(fold)) fold <- match(fold, unique(fold)) - 1L
  res <- .cocons.hip.result(.Call(`_cocons_hip_cv`, fit, theta_list[-1], theta_list$mean, fold), safe)
  if (is.null(res)) return(NULL)
  list(resid = res[[1]], var = res[[2]])
}

# the same, leave-one-out, for the tapered model on a taper handle (cocons_cv_taper)
.cocons.hip.cv.taper <- function(fit, theta_list, safe = TRUE) {
  res <- .cocons.hip.result(.Call(`_cocons_hip_cv_taper`, fit, theta_list[-1], theta_list$mean), safe)
  if (is.null(res)) return(NULL)
  list(resid = res[[1]], var = res[[2]])
}

# the same by folds on a taper handle, every fold from the one held band factor (cocons_cv_taper_folds).  fold: one label of
# any kind per observation, normalised as .cocons.hip.cv does (NULL: leave-one-out); max_rows: rows per chunk of the band
# solve (0: the library's choice)
.cocons.hip.cv.taper.folds <- function(fit, theta_list, fold, max_rows = 0L, safe = TRUE) {
  if (!is.null(fold)) fold <- match(fold, unique(fold)) - 1L
  res <- .cocons.hip.result(.Call(`_cocons_hip_cv_taper_folds`, fit, theta_list[-1], theta_list$mean, fold,
                                  as.integer(max_rows)), safe)
  if (is.null(res)) return(NULL)
  list(resid = res[[1]], var = res[[2]])
}

# derivative of sumsmoothlone (src/cocons_full.cpp:12-30) per element: sign(x) off the smooth branch, tanh(alpha x / 2) on it
.cocons.hip.dsumsmoothlone <- function(x, lambda, alpha = 1e6) {
  lambda * ifelse(abs(x) > 1e-4, sign(x), tanh(alpha * x / 2))
}

# d .cocons.getPen / d (entries of theta_list) (R/checkFunctions.R:474-492): a list shaped like theta_list
.cocons.hip.getPen.grad <- function(n, lambda, theta_list, smooth.limits) {
  g <- lapply(theta_list, function(v) numeric(length(v)))
  span <- smooth.limits[2] - smooth.limits[1]
  s <- 1 / (1 + exp(-theta_list$smooth[1]))
  nu0 <- span * s + smooth.limits[1]
  g$scale[1] <- g$scale[1] + lambda[3] * exp(theta_list$scale[1]) * sqrt(nu0)
  g$smooth[1] <- g$smooth[1] + lambda[3] * exp(theta_list$scale[1]) * span * s * (1 - s) / (2 * sqrt(nu0))
  for (ii in 1:6) {                               # names[1] with lambda[2], names[2:6] with lambda[1], as getPen
    v <- theta_list[[ii]]
    if (length(v) > 1)
      g[[ii]][-1] <- g[[ii]][-1] + .cocons.hip.dsumsmoothlone(v[-1], if (ii == 1) lambda[2] else lambda[1])
  }
  lapply(g, function(v) 2 * n * v)
}

# chain rule through getModelLists(type = "diff") (R/getFunctions.R:570-616): gradient over the list entries -> gradient over
# the optimiser's vector (where std.dev and scale are both free: d/d raw_sd = (g_sd + g_sc) / 2, d/d raw_sc = (g_sd - g_sc) / 2)
.cocons.hip.diff.grad <- function(G, par.pos) {
  if (is.logical(par.pos$std.dev) && is.logical(par.pos$scale)) {
    both <- par.pos$std.dev & par.pos$scale
    sd <- G$std.dev; sc <- G$scale
    G$std.dev[both] <- (sd[both] + sc[both]) / 2
    G$scale[both] <- (sd[both] - sc[both]) / 2
  }
  unlist(lapply(names(par.pos), function(k) {
    pp <- par.pos[[k]]
    if (is.logical(pp)) G[[k]][seq_along(pp)][pp] else NULL
  }))
}

# gradient of GetNeg2loglikelihood over theta (the optimiser's vector): what cocoOptim can pass as `gr` (INTEGRATION.md);
# zeros after a failing Cholesky under safe (where GetNeg2loglikelihood returns 1e6)
GetNeg2loglikelihoodGrad <- function(theta, par.pos, locs, x_covariates, smooth.limits, z, n, lambda,
                                     safe = TRUE, fit = NULL) {
  theta_list <- cocons::getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  if (is.null(fit)) fit <- .cocons.hip.cached(locs, x_covariates, z, smooth.limits)
  g <- .cocons.hip.neg2loglik.grad(fit, theta_list, safe)
  if (is.null(g)) return(rep(0, length(theta)))
  G <- .cocons.hip.getPen.grad(n * dim(as.matrix(z))[2], lambda, theta_list, smooth.limits)
  G$mean <- G$mean + g$mean
  aspects <- c("std.dev", "scale", "aniso", "tilt", "smooth", "nugget")
  for (t in seq_along(aspects)) G[[aspects[t]]] <- G[[aspects[t]]] + g$table[t, ]
  .cocons.hip.diff.grad(G, par.pos)
}

# the 1 + 2P points of one finite-difference gradient, or getHessian's 3P(P+1)/2 (R/getFunctions.R:979-1016)
GetNeg2loglikelihoodBatch <- function(thetas, par.pos, locs, x_covariates, smooth.limits, z, n, lambda,
                                      safe = TRUE, fit = NULL) {
  tl <- lapply(thetas, function(t) cocons::getModelLists(theta = t, par.pos = par.pos, type = "diff"))
  if (is.null(fit)) fit <- .cocons.hip.cached(locs, x_covariates, z, smooth.limits)
  res <- .Call(`_cocons_hip_neg2loglik_batch`, fit, lapply(tl, function(x) x[-1]), lapply(tl, function(x) x$mean))
  out <- res[[2]]
  for (i in seq_along(tl)) {
    if (res[[1]][i] > 0L) { if (safe) out[i] <- 1e+06 else stop("Cholesky error") }
    else out[i] <- out[i] + .cocons.getPen(n * dim(as.matrix(z))[2], lambda, tl[[i]], smooth.limits)
  }
  out
}

GetNeg2loglikelihoodProfile <- function(theta, par.pos, locs, x_covariates, smooth.limits, z, n, x_betas,
                                        lambda, safe = TRUE, fit = NULL) {
  theta_list <- cocons::getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  if (is.null(fit)) fit <- .cocons.hip.cached(locs, x_covariates, z, smooth.limits, x_betas)
  v <- .cocons.hip.result(.Call(`_cocons_hip_neg2loglik_profile`, fit, theta_list[-1]), safe)
  if (is.null(v)) return(1e+06)
  v[1] + .cocons.getPen(n * dim(as.matrix(z))[2], lambda, theta_list, smooth.limits)
}

GetNeg2loglikelihoodREML <- function(theta, par.pos, locs, x_covariates, x_betas, smooth.limits, z, n,
                                     lambda, safe = TRUE, fit = NULL) {
  theta_list <- cocons::getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  if (is.null(fit)) fit <- .cocons.hip.cached(locs, x_covariates, z, smooth.limits)
  v <- .cocons.hip.result(.Call(`_cocons_hip_neg2loglik_reml`, fit, theta_list[-1],
                                as.integer(qr(x_covariates)$rank)), safe)                  # :270
  if (is.null(v)) return(1e+06)
  v[1] + .cocons.getPen(n * dim(as.matrix(z))[2], lambda, theta_list, smooth.limits)
}

# gradient over theta (the optimiser's vector) from a Profile / REML value + gradient call: res = list(v, table 6 x p) or
# NULL after a failing Cholesky under safe (zeros, where the value functions return 1e6); N as the value function's getPen
.cocons.hip.profile.grad <- function(res, theta, theta_list, par.pos, N, lambda, smooth.limits) {
  if (is.null(res)) return(rep(0, length(theta)))
  G <- .cocons.hip.getPen.grad(N, lambda, theta_list, smooth.limits)
  aspects <- c("std.dev", "scale", "aniso", "tilt", "smooth", "nugget")
  for (t in seq_along(aspects)) G[[aspects[t]]] <- G[[aspects[t]]] + res[[2]][t, ]
  .cocons.hip.diff.grad(G, par.pos)
}

# gradients of GetNeg2loglikelihoodProfile / GetNeg2loglikelihoodREML over theta, with their signatures: what cocoOptim's
# pml / reml branch can pass as `gr` (INTEGRATION.md).  The mean is profiled out (par.pos$mean all FALSE there).
GetNeg2loglikelihoodProfileGrad <- function(theta, par.pos, locs, x_covariates, smooth.limits, z, n, x_betas,
                                            lambda, safe = TRUE, fit = NULL) {
  theta_list <- cocons::getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  if (is.null(fit)) fit <- .cocons.hip.cached(locs, x_covariates, z, smooth.limits, x_betas)
  res <- .cocons.hip.result(.Call(`_cocons_hip_neg2loglik_profile_grad`, fit, theta_list[-1]), safe)
  .cocons.hip.profile.grad(res, theta, theta_list, par.pos, n * dim(as.matrix(z))[2], lambda, smooth.limits)
}

GetNeg2loglikelihoodREMLGrad <- function(theta, par.pos, locs, x_covariates, x_betas, smooth.limits, z, n,
                                         lambda, safe = TRUE, fit = NULL) {
  theta_list <- cocons::getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  if (is.null(fit)) fit <- .cocons.hip.cached(locs, x_covariates, z, smooth.limits)
  res <- .cocons.hip.result(.Call(`_cocons_hip_neg2loglik_reml_grad`, fit, theta_list[-1],
                                  as.integer(qr(x_covariates)$rank)), safe)
  .cocons.hip.profile.grad(res, theta, theta_list, par.pos, n * dim(as.matrix(z))[2], lambda, smooth.limits)
}

# GLS coefficients after a pml / reml fit (R/optim.R:329-341) without a second chol:
# v = c(sum_logliks, logdet, logdet_W, quad_1..r, beta_1..) as returned by the cores above
.cocons.hip.betas <- function(v, r) v[-seq_len(3 + r)]

# dense kriging core for cocoPredict (R/predict.R:136-183): the four lines cov_rns / cov_rns_pred /
# solve / rowSums become
#   kr <- .cocons.hip.predict(fit, theta_list, newlocs, X_pred_std)
#   stochastic <- kr[, 1];  quadform <- kr[, 2]      # c_i' Sigma^-1 resid,  c_i' Sigma^-1 c_i
.cocons.hip.predict <- function(fit, theta_list, newlocs, X_pred, z_col = 1L) {
  res <- .Call(`_cocons_hip_predict`, fit, theta_list[-1], theta_list$mean, as.integer(z_col), newlocs, X_pred)
  if (res[[1]] > 0L) stop("Cholesky error")
  res[[2]]
}

# the same core at any number of new locations from ONE factorisation (a map grid, several newdatasets, a map in pieces):
#   .cocons.hip.krige.prepare(fit, theta_list)            # Sigma(theta) factored once, the factor kept on the handle
#   kr <- .cocons.hip.krige(fit, newlocs, X_pred_std)     # as often as needed: chunked, device memory independent of m
#   .cocons.hip.krige.release(fit)                        # (or when the handle is closed)
.cocons.hip.krige.prepare <- function(fit, theta_list, z_col = 1L, max_rows = 0L) {
  res <- .Call(`_cocons_hip_krige_prepare`, fit, theta_list[-1], theta_list$mean, as.integer(z_col), as.integer(max_rows))
  if (res[[1]] > 0L) stop("Cholesky error")
  invisible(NULL)
}

.cocons.hip.krige <- function(fit, newlocs, X_pred) {
  res <- .Call(`_cocons_hip_krige`, fit, newlocs, X_pred)
  res[[2]]
}

# joint prediction against the same held factor: the predictive covariance between the new locations (a joint interval, a
# contrast, the variance of an areal mean) and, with iiderrors (m x nsim), cocoSim's conditional draws (R/sim.R:84-127)
# without factoring the joint (n + m) matrix:
#   kj <- .cocons.hip.krige.joint(fit, newlocs, X_pred_std, locs_unobs = as.matrix(newdataset)[, 1:2], iiderrors = E)
#   kj$stochastic;  kj$cov  (m x m, or NULL with cov = FALSE);  kj$sims  (m x nsim, or NULL without iiderrors)
.cocons.hip.krige.joint <- function(fit, newlocs, X_pred, locs_unobs = NULL, iiderrors = NULL, cov = TRUE) {
  res <- .Call(`_cocons_hip_krige_joint`, fit, newlocs, X_pred, locs_unobs, iiderrors, as.logical(cov))
  if (res[[1]] != 0L) stop("Cholesky error")
  list(stochastic = res[[2]], cov = res[[3]], sims = res[[4]])
}

.cocons.hip.krige.release <- function(fit) invisible(.Call(`_cocons_hip_krige_release`, fit))

# rows of cov2cor(cov_rns(...)) for plot(type = "correlations") (R/methods.R:161-165): tmp_cov[ww, ]
.cocons.hip.cor.rows <- function(fit, theta_list, index, classic = FALSE)
  .Call(`_cocons_hip_cov_rows`, fit, theta_list[-1], classic, as.integer(index), TRUE)

# one R process, several GPUs: Sigma row blocks sharded over `devices`, RCCL inside the library
cocons_hip_multi <- function(locs, x_covariates, z, smooth.limits, devices)
  .Call(`_cocons_hip_multi_create`, locs, x_covariates, as.matrix(z), as.double(smooth.limits), as.integer(devices))

# replica mode inside ONE R process: a list of parameter points (the 2p+1 points of a finite-difference gradient,
# R/optim.R:256-259, or getHessian's grid, R/getFunctions.R:979-1016) dealt over the GPUs of a multi handle
cocons_hip_multi_neg2loglik_batch <- function(m, theta_lists) {
  res <- .Call(`_cocons_hip_multi_neg2loglik_batch`, m, lapply(theta_lists, function(th) th[-1]),
               lapply(theta_lists, function(th) th$mean))
  ifelse(res[[1]] > 0L, 1e+06, res[[2]])
}

# c(active, time-outs, last abort code) of the resident diagonal-block engine of a fit handle (diagnostic)
cocons_hip_engine_state <- function(fit) .Call(`_cocons_hip_engine_state`, fit)

# cocoPredict's dense core with the prediction locations split over the GPUs of a multi handle (config C5)
cocons_hip_multi_predict <- function(m, theta_list, newlocs, X_pred, z_col = 1L) {
  res <- .Call(`_cocons_hip_multi_predict`, m, theta_list[-1], theta_list$mean, as.integer(z_col), newlocs, X_pred)
  if (res[[1]] > 0L) stop("Cholesky error")
  res[[2]]
}

# ---- type = "sparse": the taper objective through the dense factorisation on the device --------------------
# handle of one optimisation; ref_taper is the spam object coco() builds (R/cocons.R), n^2 doubles must fit the GPU
cocons_hip_taper_fit <- function(locs, x_covariates, z, smooth.limits, ref_taper, device = -1L)
  .Call(`_cocons_hip_fit_create_taper`, locs, x_covariates, as.matrix(z), as.double(smooth.limits), as.integer(device),
        ref_taper@colindices, ref_taper@rowpointers, as.double(ref_taper@entries))

# body of GetNeg2loglikelihoodTaper (R/neg2loglikelihood.R:20-53); cholS is not used
.cocons.hip.GetNeg2loglikelihoodTaper <- function(theta, par.pos, fit, smooth.limits, z, n, lambda, safe = TRUE) {
  theta_list <- getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  val <- .cocons.hip.result(.Call(`_cocons_hip_neg2loglik`, fit, theta_list[-1], theta_list$mean), safe)
  if (is.null(val)) return(1e+06)
  val + .cocons.getPen(n * dim(z)[2], lambda, theta_list, smooth.limits)
}

# body of GetNeg2loglikelihoodTaperProfile (R/neg2loglikelihood.R:73-108)
.cocons.hip.GetNeg2loglikelihoodTaperProfile <- function(theta, par.pos, fit, smooth.limits, z, n, lambda, safe = TRUE) {
  theta_list <- getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  theta_list$std.dev[1] <- 0
  v <- .cocons.hip.result(.Call(`_cocons_hip_neg2loglik_parts`, fit, theta_list[-1], theta_list$mean), safe)
  if (is.null(v)) return(1e+06)
  r <- dim(z)[2]; logdet <- v[2]; sum_in <- sum(v[-(1:2)])
  r * n * log(2 * pi) + r * n + r * 2 * logdet + r * n * log(sum_in / (r * n)) +
    .cocons.getPen(n * r, lambda, theta_list, smooth.limits)
}

# value, parts and analytic gradient of the tapered -2 log-likelihood core on a taper handle (no penalty):
# list(v = c(sum_logliks, logdet_half, quad_1 .. quad_r), table, quad = 6 x p gradients of the whole value and of the
# quadratic forms alone, mean); NULL after a failing Cholesky under safe
.cocons.hip.neg2loglik.taper.grad <- function(fit, theta_list, safe = TRUE) {
  res <- .cocons.hip.result(.Call(`_cocons_hip_neg2loglik_taper_grad`, fit, theta_list[-1], theta_list$mean), safe)
  if (is.null(res)) return(NULL)
  list(v = res[[1]], table = res[[2]], quad = res[[3]], mean = res[[4]])
}

# gradients of GetNeg2loglikelihoodTaper / GetNeg2loglikelihoodTaperProfile over theta (the optimiser's vector), with the
# bodies' signatures: what cocoOptim's sparse branches can pass as `gr` (INTEGRATION.md); zeros after a failing Cholesky
# under safe (where the value functions return 1e6)
.cocons.hip.GetNeg2loglikelihoodTaperGrad <- function(theta, par.pos, fit, smooth.limits, z, n, lambda, safe = TRUE) {
  theta_list <- getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  g <- .cocons.hip.neg2loglik.taper.grad(fit, theta_list, safe)
  if (is.null(g)) return(rep(0, length(theta)))
  G <- .cocons.hip.getPen.grad(n * dim(z)[2], lambda, theta_list, smooth.limits)
  G$mean <- G$mean + g$mean
  aspects <- c("std.dev", "scale", "aniso", "tilt", "smooth", "nugget")
  for (t in seq_along(aspects)) G[[aspects[t]]] <- G[[aspects[t]]] + g$table[t, ]
  .cocons.hip.diff.grad(G, par.pos)
}

# the Profile form is r 2 logdet + r n log(Q / (r n)) + constants, Q the sum of the quadratic forms: its gradient is the
# log-determinant's share plus r n / Q times the quadratic forms' share; std.dev[1] is overwritten with 0, so its entry is 0
.cocons.hip.GetNeg2loglikelihoodTaperProfileGrad <- function(theta, par.pos, fit, smooth.limits, z, n, lambda, safe = TRUE) {
  theta_list <- getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  theta_list$std.dev[1] <- 0
  g <- .cocons.hip.neg2loglik.taper.grad(fit, theta_list, safe)
  if (is.null(g)) return(rep(0, length(theta)))
  r <- dim(z)[2]; w <- r * n / sum(g$v[-(1:2)])
  G <- .cocons.hip.getPen.grad(n * r, lambda, theta_list, smooth.limits)
  G$mean <- G$mean + w * g$mean
  aspects <- c("std.dev", "scale", "aniso", "tilt", "smooth", "nugget")
  for (t in seq_along(aspects)) G[[aspects[t]]] <- G[[aspects[t]]] + (g$table[t, ] - g$quad[t, ]) + w * g$quad[t, ]
  G$std.dev[1] <- 0
  .cocons.hip.diff.grad(G, par.pos)
}

# sparse branch of cocoPredict (R/predict.R:216-283): the lines from cov_rns_taper to rowSums(pred_taper * t(inv_cov)) become
#   kr <- .cocons.hip.predict.taper(fit, theta_list, newlocs, X_pred_std, pred_taper)   # pred_taper: the spam object of :229-231
#   stochastic_part <- kr[, 1];  uncertainty_some <- uncertainty_some - kr[, 2]
.cocons.hip.predict.taper <- function(fit, theta_list, newlocs, X_pred, pred_taper, z_col = 1L) {
  res <- .Call(`_cocons_hip_predict_taper`, fit, theta_list[-1], theta_list$mean, as.integer(z_col), newlocs, X_pred,
               pred_taper@colindices, pred_taper@rowpointers, as.double(pred_taper@entries))
  if (res[[1]] > 0L) stop("Cholesky error")
  res[[2]]
}

# the same core at any number of new locations from ONE factorisation of the tapered matrix (a map grid, a map in pieces):
#   .cocons.hip.krige.taper.prepare(fit, theta_list)                     # S(theta) factored once, the band factor kept
#   kr <- .cocons.hip.krige.taper(fit, newlocs, X_pred_std, pred_taper)  # as often as needed: chunked, memory independent of m
#   .cocons.hip.krige.taper.release(fit)                                 # (or when the handle is closed)
.cocons.hip.krige.taper.prepare <- function(fit, theta_list, z_col = 1L, max_rows = 0L) {
  res <- .Call(`_cocons_hip_krige_taper_prepare`, fit, theta_list[-1], theta_list$mean, as.integer(z_col), as.integer(max_rows))
  if (res[[1]] > 0L) stop("Cholesky error")
  invisible(NULL)
}

.cocons.hip.krige.taper <- function(fit, newlocs, X_pred, pred_taper) {
  res <- .Call(`_cocons_hip_krige_taper`, fit, newlocs, X_pred, pred_taper@colindices, pred_taper@rowpointers,
               as.double(pred_taper@entries))
  res[[2]]
}

# the taper itself from delta, found on the device: the slots of spam::nearest.dist(newlocs, locs, delta) (newlocs = NULL:
# nearest.dist(locs, delta = delta, upper = NULL)) with cov.wend1 / cov.wend2 / cov.sph at theta = c(delta, 1) as entries
#   tp <- .cocons.hip.taper.pattern(locs, delta, "wend1")   # list(colindices, rowpointers, entries), 1-based
.cocons.hip.taper.kind <- function(kind) {
  k <- match(kind, c("wend1", "wend2", "sph"))
  if (is.na(k)) stop("kind must be one of wend1, wend2, sph")
  as.integer(k)
}

.cocons.hip.taper.pattern <- function(locs, delta, kind = "wend1", newlocs = NULL, device = 0L) {
  res <- .Call(`_cocons_hip_taper_pattern`, locs, newlocs, as.double(delta), .cocons.hip.taper.kind(kind), as.integer(device))
  list(colindices = res[[1]], rowpointers = res[[2]], entries = res[[3]])
}

# .cocons.hip.krige.taper without pred_taper: neighbours and taper values come from delta, chunk by chunk on the device
.cocons.hip.krige.taper.delta <- function(fit, newlocs, X_pred, delta, kind = "wend1") {
  res <- .Call(`_cocons_hip_krige_taper_delta`, fit, newlocs, X_pred, as.double(delta), .cocons.hip.taper.kind(kind))
  res[[2]]
}

# joint prediction against the same held band factor: the predictive covariance between the new locations and, with
# iiderrors (m x nsim), conditional draws of the tapered model (the reference's cocoSim has no conditional branch for
# sparse objects).  uu_taper: the taper between the new locations, spam::nearest.dist(newlocs, delta = delta, upper = NULL)
# with the taper function applied (every row holds its diagonal; the entries with column <= row are read):
#   kj <- .cocons.hip.krige.taper.joint(fit, newlocs, X_pred_std, pred_taper, uu_taper, iiderrors = E)
#   kj$stochastic;  kj$cov  (m x m, or NULL with cov = FALSE);  kj$sims  (m x nsim, or NULL without iiderrors)
.cocons.hip.krige.taper.joint <- function(fit, newlocs, X_pred, pred_taper, uu_taper, locs_unobs = NULL, iiderrors = NULL,
                                          cov = TRUE) {
  res <- .Call(`_cocons_hip_krige_taper_joint`, fit, newlocs, X_pred,
               list(pred_taper@colindices, pred_taper@rowpointers, as.double(pred_taper@entries)),
               list(uu_taper@colindices, uu_taper@rowpointers, as.double(uu_taper@entries)),
               locs_unobs, iiderrors, as.logical(cov))
  if (res[[1]] != 0L) stop("Cholesky error")
  list(stochastic = res[[2]], cov = res[[3]], sims = res[[4]])
}

.cocons.hip.krige.taper.release <- function(fit) invisible(.Call(`_cocons_hip_krige_taper_release`, fit))

# sparse branch of cocoSim (R/sim.R:177-217): the lines from cov_rns_taper to the sweep (:193-216) become
#   fields <- .cocons.hip.sim.taper(fit, theta_list, iiderrors, pivot)     # fit: cocons_hip_taper_fit(...)
# pivot = spam::ordering(spam::chol(ref_taper)) gives the reference's fields to rounding (MMD depends only on the pattern:
# compute it once per coco object); pivot = NULL simulates in the handle's own order -- same distribution, other fields
.cocons.hip.sim.taper <- function(fit, theta_list, iiderrors, pivot = NULL) {
  if (!is.null(pivot)) pivot <- as.integer(pivot)
  res <- .Call(`_cocons_hip_sim_taper`, fit, theta_list[-1], theta_list$mean, as.matrix(iiderrors), pivot)
  if (res[[1]] > 0L) stop("Cholesky error")
  res[[2]]
}

# Vecchia approximation of the model's own likelihood (DESIGN.md 4r): n small blocks instead of one factorisation, O(n m)
# memory, for n up to 10^6.  nn is the n x m matrix of neighbours -- row i names the EARLIER rows (1-based, 0 = none) that
# observation i is conditioned on; the rows' order (maxmin, random, by coordinate) and the neighbour search stay with the caller
# (.cocons.hip.vecchia.order and .cocons.hip.vecchia.neighbours below, or GpGp::order_maxmin and GpGp::find_ordered_nn, give both: nn <- find_ordered_nn(locs[ord, ], m)[, -1]; nn[is.na(nn)] <- 0):
#   fit <- .cocons.hip.vecchia.create(locs[ord, ], x_covariates[ord, ], z[ord, , drop = FALSE], smooth.limits, nn)
#   optim(..., fn = function(theta) .cocons.hip.vecchia.neg2loglik(fit, theta, par.pos, smooth.limits, n, r, lambda))
.cocons.hip.vecchia.create <- function(locs, x_covariates, z, smooth.limits, nn, device = -1L) {
  storage.mode(nn) <- "integer"
  .Call(`_cocons_hip_vecchia_create`, as.matrix(locs), as.matrix(x_covariates), as.matrix(z), as.double(smooth.limits),
        as.integer(device), nn)
}

# GetNeg2loglikelihood with the Vecchia value in place of the dense one: 1e+06 on a failing block under safe (:202-206)
.cocons.hip.vecchia.neg2loglik <- function(fit, theta, par.pos, smooth.limits, n, r, lambda, safe = TRUE) {
  theta_list <- getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  v <- .cocons.hip.result(.Call(`_cocons_hip_vecchia_neg2loglik`, fit, theta_list[-1], theta_list$mean), safe)
  if (is.null(v)) return(1e+06)
  v[1] + .cocons.getPen(n * r, lambda, theta_list, smooth.limits)
}

# value and analytic gradient of the Vecchia -2 log-likelihood core (no penalty; DESIGN.md 4s): list(value, table = 6 x p
# gradient over std.dev, scale, aniso, tilt, smooth, nugget, quad = the quadratic forms' share of it, mean = gradient over
# theta$mean); NULL after a failing block under safe.  The gr = of an optimiser is built on it as on .cocons.hip.neg2loglik.grad
.cocons.hip.vecchia.neg2loglik.grad <- function(fit, theta_list, safe = TRUE) {
  res <- .cocons.hip.result(.Call(`_cocons_hip_vecchia_neg2loglik_grad`, fit, theta_list[-1], theta_list$mean), safe)
  if (is.null(res)) return(NULL)
  list(value = res[[1]], table = res[[2]], quad = res[[3]], mean = res[[4]])
}

# expected information of the Vecchia fit over theta (cocons_fisher_vecchia; DESIGN.md 4t), P x P in theta's order, from one
# pass over the n blocks: the expectation at the model of the Hessian of half of the Vecchia -2 log-likelihood, without the
# penalty -- what GpGp calls info.  Not the observed Hessian, not the Godambe (sandwich) information.  The Jacobian as in
# .cocons.hip.fisher; NULL after a failing block under safe.  grouped: on the grouped schedule (what
# .cocons.hip.vecchia.fisher.grouped passes).
.cocons.hip.vecchia.fisher <- function(fit, theta, par.pos, safe = TRUE, grouped = FALSE) {
  aspects <- c("std.dev", "scale", "aniso", "tilt", "smooth", "nugget")
  base <- cocons::getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  p <- length(base$mean)
  flat <- function(tl) c(tl$mean, unlist(tl[aspects], use.names = FALSE))
  J <- vapply(seq_along(theta), function(a) {
    e <- theta
    e[a] <- e[a] + 1
    flat(cocons::getModelLists(theta = e, par.pos = par.pos, type = "diff")) - flat(base)
  }, numeric(7 * p))
  Jm <- J[seq_len(p), , drop = FALSE]
  Jt <- J[-seq_len(p), , drop = FALSE]
  cov <- which(colSums(Jt != 0) > 0)
  dirs <- Jt[, if (length(cov)) cov else 1L, drop = FALSE]
  res <- .cocons.hip.result(if (grouped) .Call(`_cocons_hip_vecchia_fisher_grouped`, fit, base[-1], dirs)
                            else .Call(`_cocons_hip_vecchia_fisher`, fit, base[-1], dirs), safe)
  if (is.null(res)) return(NULL)
  info <- crossprod(Jm, res[[2]] %*% Jm)
  if (length(cov)) info[cov, cov] <- info[cov, cov] + res[[1]]
  info
}

# local kriging: cbind(stochastic, quadform) for the new locations, each from the observations its row of nn_pred names
# (1-based, 0 = none) -- the two columns cocoPredict's dense branch takes from its solve (R/predict.R:165-173)
.cocons.hip.vecchia.predict <- function(fit, theta_list, newlocs, X_pred, nn_pred, z_col = 1L) {
  storage.mode(nn_pred) <- "integer"
  res <- .Call(`_cocons_hip_vecchia_predict`, fit, theta_list, as.integer(z_col), as.matrix(newlocs), as.matrix(X_pred),
               nn_pred)
  if (res[[1]] > 0L) stop("Cholesky error")
  res[[2]]
}

# the neighbour search on the device (DESIGN.md 4u): no table from another package is needed.  The rule is the key
# (d2, index) with d2 = dx * dx + dy * dy in double, no square root, ties to the lower index; rows list the nearest first and are
# zero-padded, so the table for m is the first m columns of the table for any larger m.
#   nn <- .cocons.hip.vecchia.neighbours(locs[ord, ], m)                 # row i: the m nearest EARLIER rows
#   nn_pred <- .cocons.hip.vecchia.neighbours(locs[ord, ], m, newlocs)   # row i: the m nearest observations of newlocs[i, ]
.cocons.hip.vecchia.neighbours <- function(locs, m, newlocs = NULL, device = 0L) {
  if (!is.null(newlocs)) newlocs <- as.matrix(newlocs)
  .Call(`_cocons_hip_vecchia_neighbours`, as.matrix(locs), newlocs, as.integer(m), as.integer(device))
}

# the maxmin order on the device (DESIGN.md 4w): coarse to fine by nets whose radius halves from level to level, every point
# at least half as far from its predecessors as the farthest remaining point; a function of locs alone, no seed.
#   ord <- .cocons.hip.vecchia.order(locs)        # ord[t]: the row at position t
.cocons.hip.vecchia.order <- function(locs, device = 0L) {
  .Call(`_cocons_hip_vecchia_order`, as.matrix(locs), as.integer(device))
}

# .cocons.hip.vecchia.create without nn: the table of .cocons.hip.vecchia.neighbours(locs, m) is searched on the device and
# stays there; every entry on the handle gives the bits of the handle made from that table
.cocons.hip.vecchia.create.knn <- function(locs, x_covariates, z, smooth.limits, m, device = -1L) {
  .Call(`_cocons_hip_vecchia_create_knn`, as.matrix(locs), as.matrix(x_covariates), as.matrix(z), as.double(smooth.limits),
        as.integer(device), as.integer(m))
}

# the neighbours by MODEL CORRELATION (DESIGN.md 4af): under local anisotropy the predecessors that matter lie along the long
# axis of the local kernel, not inside the Euclidean m-nearest.  Among the m_cand Euclidean-nearest predecessors of a row and
# (hops = 2) theirs, row i lists the m most correlated with it under Sigma(theta), largest first, ties to the lower index.
#   fit0 <- .cocons.hip.vecchia.create.knn(locs[ord, ], X[ord, ], z[ord, , drop = FALSE], smooth.limits, m)   # a first fit
#   nn   <- .cocons.hip.vecchia.neighbours.corr(fit0, theta_list, m)                                          # re-ranked at its optimum
#   fit  <- .cocons.hip.vecchia.create.corr.knn(locs[ord, ], X[ord, ], z[ord, , drop = FALSE], smooth.limits, theta_list, m)
# (the second is .cocons.hip.vecchia.create with nn, made on the device).  A grouped fit on such a table:
# .cocons.hip.vecchia.create.grouped.corr.knn; new locations: .cocons.hip.vecchia.predict.corr.knn (both below).
.cocons.hip.vecchia.neighbours.corr <- function(fit, theta_list, m, m_cand = min(2L * as.integer(m), 63L), hops = 2L) {
  res <- .Call(`_cocons_hip_vecchia_neighbours_corr`, fit, theta_list, as.integer(m_cand), as.integer(hops), as.integer(m))
  if (res[[1]] > 0L) stop("the correlation of row ", res[[1]], " with a candidate is not finite")
  res[[2]]
}

.cocons.hip.vecchia.create.corr.knn <- function(locs, x_covariates, z, smooth.limits, theta_list, m,
                                                m_cand = min(2L * as.integer(m), 63L), hops = 2L, device = -1L) {
  .Call(`_cocons_hip_vecchia_create_corr_knn`, as.matrix(locs), as.matrix(x_covariates), as.matrix(z), as.double(smooth.limits),
        as.integer(device), theta_list, as.integer(m_cand), as.integer(hops), as.integer(m))
}

# .cocons.hip.vecchia.predict without nn_pred: every new location is predicted from its m_pred nearest observations, found
# on the device chunk by chunk
.cocons.hip.vecchia.predict.knn <- function(fit, theta_list, newlocs, X_pred, m_pred, z_col = 1L) {
  res <- .Call(`_cocons_hip_vecchia_predict_knn`, fit, theta_list, as.integer(z_col), as.matrix(newlocs), as.matrix(X_pred),
               as.integer(m_pred))
  if (res[[1]] > 0L) stop("Cholesky error")
  res[[2]]
}

# the neighbours of NEW locations by model correlation (DESIGN.md 4ag): among the m_cand nearest observations of a new
# location and (hops = 2) the m_cand nearest observations of each of those, the m most correlated with it under the
# prediction's covariance at theta, largest first; and local kriging on them, found and ranked on the device chunk by chunk --
# .cocons.hip.vecchia.predict with that table, to the bit.  The fit keeps the grid over the observations and (hops = 2) their
# own neighbour table of width m_cand for later calls
.cocons.hip.vecchia.neighbours.corr.pred <- function(fit, theta_list, newlocs, X_pred, m,
                                                     m_cand = min(2L * as.integer(m), 63L), hops = 2L) {
  res <- .Call(`_cocons_hip_vecchia_neighbours_corr_pred`, fit, theta_list, as.matrix(newlocs), as.matrix(X_pred),
               c(as.integer(m_cand), as.integer(hops), as.integer(m)))
  if (res[[1]] > 0L) stop("the correlation of new location ", res[[1]], " with a candidate is not finite")
  res[[2]]
}

.cocons.hip.vecchia.predict.corr.knn <- function(fit, theta_list, newlocs, X_pred, m_pred,
                                                 m_cand = min(2L * as.integer(m_pred), 63L), hops = 2L, z_col = 1L) {
  res <- .Call(`_cocons_hip_vecchia_predict_corr_knn`, fit, theta_list, as.integer(z_col), as.matrix(newlocs), as.matrix(X_pred),
               c(as.integer(m_cand), as.integer(hops), as.integer(m_pred)))
  if (res[[1]] > 0L) stop("Cholesky error")
  res[[2]]
}

# U^-1 on a Vecchia handle (DESIGN.md 4v): the inverse of the whitening, solved level by level on the device.
# .cocons.hip.vecchia.unwhiten: U^-1 W for the n x c matrix W -- with N(0, 1) columns, fields with the Vecchia model's
# covariance and mean zero, in the rows' (Vecchia) order
.cocons.hip.vecchia.unwhiten <- function(fit, theta_list, W) {
  .cocons.hip.vecchia.unwhiten.by(`_cocons_hip_vecchia_unwhiten`, fit, theta_list, W)
}

# the one body of .cocons.hip.vecchia.unwhiten and .cocons.hip.vecchia.unwhiten.grouped: `shim` switches between them
.cocons.hip.vecchia.unwhiten.by <- function(shim, fit, theta_list, W) {
  W <- as.matrix(W)
  storage.mode(W) <- "double"
  res <- .Call(shim, fit, theta_list[names(theta_list) != "mean"], W)
  if (res[[1]] > 0L) stop("Cholesky error")
  res[[2]]
}

# cocoSim for a Vecchia handle.  n_fixed = 0: X mean + U^-1 iiderrors, the marginal branch (R/sim.R:147-172).  n_fixed >= 1:
# the first n_fixed rows are data (z[, z_col]) and the rows behind them are drawn given them (sim.type = "cond"); the handle
# is made over rbind(locs, newlocs), rbind(X, X_pred) and rbind(z, anything); iiderrors is (n - n_fixed) x nsim, all zero for
# the joint conditional mean
.cocons.hip.vecchia.sim <- function(fit, theta_list, iiderrors, n_fixed = 0L, z_col = 1L) {
  .cocons.hip.vecchia.sim.by(`_cocons_hip_vecchia_sim`, fit, theta_list, iiderrors, n_fixed, z_col)
}

# the one body of .cocons.hip.vecchia.sim and .cocons.hip.vecchia.sim.grouped
.cocons.hip.vecchia.sim.by <- function(shim, fit, theta_list, iiderrors, n_fixed, z_col) {
  iiderrors <- as.matrix(iiderrors)
  storage.mode(iiderrors) <- "double"
  res <- .Call(shim, fit, theta_list, as.integer(n_fixed), as.integer(z_col), iiderrors)
  if (res[[1]] > 0L) stop("Cholesky error")
  res[[2]]
}

# the schedule the two run on: list(levels, info = c(depth, widest level, launches of one solve, device bytes))
.cocons.hip.vecchia.schedule <- function(fit, n_fixed = 0L) {
  res <- .Call(`_cocons_hip_vecchia_schedule`, fit, as.integer(n_fixed))
  list(levels = res[[1]], info = res[[2]])
}

# U' and cross-validation on a Vecchia handle (DESIGN.md 4x): the model's precision is U'U, applied through the transposed
# lists of the table ("which rows name me"), which the handle builds once on the device.
# .cocons.hip.vecchia.transpose: list(ptr, rows, info = c(entries, longest list, device bytes, columns nobody names)) -- the
# rows that name column j are rows[(ptr[j] + 1):ptr[j + 1]], ascending
.cocons.hip.vecchia.transpose <- function(fit) {
  res <- .Call(`_cocons_hip_vecchia_transpose`, fit)
  list(ptr = res[[1]], rows = res[[2]], info = res[[3]])
}

# U'W for the n x c matrix W and diag(U'U): list(out, qdiag)
.cocons.hip.vecchia.whiten.t <- function(fit, theta_list, W) {
  .cocons.hip.vecchia.whiten.t.by(`_cocons_hip_vecchia_whiten_t`, fit, theta_list, W)
}

# the one body of .cocons.hip.vecchia.whiten.t and .cocons.hip.vecchia.whiten.t.grouped
.cocons.hip.vecchia.whiten.t.by <- function(shim, fit, theta_list, W) {
  W <- as.matrix(W)
  storage.mode(W) <- "double"
  res <- .Call(shim, fit, theta_list[names(theta_list) != "mean"], W)
  if (res[[1]] > 0L) stop("Cholesky error")
  list(out = res[[2]][[1]], qdiag = res[[2]][[2]])
}

# U^-T on a Vecchia handle and the model's own covariance through it (DESIGN.md 4ad; GpGp's L_t_mult).  `grouped`: the rows'
# coefficients from one factorisation per block of the handle's plan (.cocons.hip.vecchia.set.groups) -- the same bits.
# .cocons.hip.vecchia.unwhiten.t: U^-T W for the n x c matrix W, the inverse of .cocons.hip.vecchia.whiten.t
.cocons.hip.vecchia.unwhiten.t <- function(fit, theta_list, W, grouped = FALSE) {
  W <- as.matrix(W)
  storage.mode(W) <- "double"
  res <- .Call(`_cocons_hip_vecchia_unwhiten_t`, fit, theta_list[names(theta_list) != "mean"], W, as.integer(grouped))
  if (res[[1]] > 0L) stop("Cholesky error")
  res[[2]]
}

# .cocons.hip.vecchia.cov.mult: (U_pp' U_pp)^-1 B for the (n - n_fixed) x c matrix B.  n_fixed = 0: the covariance of the
# Vecchia model times B; on a handle over rbind(locs, newlocs) with n_fixed = nrow(locs): Cov(new | data) B
.cocons.hip.vecchia.cov.mult <- function(fit, theta_list, B, n_fixed = 0L, grouped = FALSE) {
  B <- as.matrix(B)
  storage.mode(B) <- "double"
  res <- .Call(`_cocons_hip_vecchia_cov_mult`, fit, theta_list[names(theta_list) != "mean"], B, as.integer(n_fixed),
               as.integer(grouped))
  if (res[[1]] > 0L) stop("Cholesky error")
  res[[2]]
}

# .cocons.hip.vecchia.cov.cols: the columns idx (rows of the handle, each > n_fixed; repeats allowed) of that covariance
.cocons.hip.vecchia.cov.cols <- function(fit, theta_list, idx, n_fixed = 0L, grouped = FALSE) {
  res <- .Call(`_cocons_hip_vecchia_cov_cols`, fit, theta_list[names(theta_list) != "mean"], as.integer(idx),
               as.integer(n_fixed), as.integer(grouped))
  if (res[[1]] > 0L) stop("Cholesky error")
  res[[2]]
}

# .cocons.hip.vecchia.schedule.t: list(levels, info = c(depth, rows of the widest level, launches of one solve, device bytes))
# of the transposed schedule the three entries above run on
.cocons.hip.vecchia.schedule.t <- function(fit, n_fixed = 0L) {
  res <- .Call(`_cocons_hip_vecchia_schedule_t`, fit, as.integer(n_fixed))
  list(levels = res[[1]], info = res[[2]])
}

# Grouped Vecchia blocks (DESIGN.md 4y; Guinness 2018, GpGp's group_obs): rows with overlapping neighbour sets share one block,
# which is assembled and factored once.  Every member then conditions on a superset of its own neighbours: the grouped model is
# the Vecchia model of the EXPANDED table, and the grouped entries return the bits of the ungrouped ones on that table's handle.
#   g <- .cocons.hip.vecchia.group(nn)                                   # greedy groups of the table (on the host)
#   wide <- .cocons.hip.vecchia.group.table(nn, g$group)                 # row i: every earlier row of its block
#   fit <- .cocons.hip.vecchia.create(locs, x_covariates, z, smooth.limits, wide)
#   .cocons.hip.vecchia.set.groups(fit, g$group)
#   optim(..., fn = function(theta) .cocons.hip.vecchia.neg2loglik.grouped(fit, theta, par.pos, smooth.limits, n, r, lambda))
# .cocons.hip.vecchia.group: list(group = block ids from 0, numbered by their smallest member, info = c(blocks, rows over the
# blocks, pairs of the grouped schedule, pairs of the ungrouped schedule on nn)); max_rows in 2 .. 64 caps the rows of a block
.cocons.hip.vecchia.group <- function(nn, max_rows = 64L) {
  res <- .Call(`_cocons_hip_vecchia_group`, as.matrix(nn), as.integer(max_rows))
  list(group = res[[1]], info = res[[2]])
}

# the ROUND rule's groups of the table (DESIGN.md 4ac): every round each block proposes the neighbouring block whose merge saves
# the most, and the proposals that are the best of both their blocks are merged; a function of the rows' neighbour sets, not the
# greedy partition.  list(group, info = c(.cocons.hip.vecchia.group's four, the rounds that merged something)); max_rounds = 0:
# at most 256 rounds.  .cocons.hip.vecchia.group.rounds runs on the host, .cocons.hip.vecchia.group.device on the device -- the
# same integers
.cocons.hip.vecchia.group.rounds <- function(nn, max_rows = 64L, max_rounds = 0L) {
  res <- .Call(`_cocons_hip_vecchia_group_rounds`, as.matrix(nn), as.integer(max_rows), as.integer(max_rounds))
  list(group = res[[1]], info = res[[2]])
}

.cocons.hip.vecchia.group.device <- function(nn, max_rows = 64L, max_rounds = 0L, device = 0L) {
  res <- .Call(`_cocons_hip_vecchia_group_device`, as.matrix(nn), as.integer(max_rows), as.integer(max_rounds), as.integer(device))
  list(group = res[[1]], info = res[[2]])
}

# the grouped fit made on the device: the search of .cocons.hip.vecchia.create.knn, the round rule, the plan and the expanded
# table, none of which comes to the host -- the fit of .cocons.hip.vecchia.neighbours, .group.rounds, .group.table, .create and
# .set.groups on the same data, to the bit.  .cocons.hip.vecchia.groups.export reads list(group, nn) back from any fit with a plan
.cocons.hip.vecchia.create.grouped.knn <- function(locs, x_covariates, z, smooth.limits, m, max_rows = 64L, max_rounds = 0L,
                                                   device = -1L) {
  .Call(`_cocons_hip_vecchia_create_grouped_knn`, as.matrix(locs), as.matrix(x_covariates), as.matrix(z), as.double(smooth.limits),
        as.integer(device), as.integer(m), as.integer(max_rows), as.integer(max_rounds))
}

# the same on the table of .cocons.hip.vecchia.neighbours.corr at theta (DESIGN.md 4ag) in the place of the Euclidean search:
# the fit of .neighbours.corr, .group.rounds, .group.table, .create and .set.groups on the same data, to the bit
.cocons.hip.vecchia.create.grouped.corr.knn <- function(locs, x_covariates, z, smooth.limits, theta_list, m,
                                                        m_cand = min(2L * as.integer(m), 63L), hops = 2L, max_rows = 64L,
                                                        max_rounds = 0L, device = -1L) {
  .Call(`_cocons_hip_vecchia_create_grouped_corr_knn`, as.matrix(locs), as.matrix(x_covariates), as.matrix(z),
        as.double(smooth.limits), as.integer(device), theta_list, c(as.integer(m_cand), as.integer(hops), as.integer(m)),
        as.integer(max_rows), as.integer(max_rounds))
}

.cocons.hip.vecchia.groups.export <- function(fit) {
  res <- .Call(`_cocons_hip_vecchia_groups_export`, fit)
  list(group = res[[1]], nn = res[[2]])
}

# the expanded table of ANY partition of nn's rows (labels in 0 .. n - 1): an integer matrix, 1-based, ascending, 0 = none
.cocons.hip.vecchia.group.table <- function(nn, group) {
  .Call(`_cocons_hip_vecchia_group_table`, as.matrix(nn), as.integer(group))
}

# attach the plan of a partition to a Vecchia handle whose table is closed under it (the library checks and names the first
# row that is not): c(blocks, rows of the largest block, rows over the blocks, pairs, device bytes of the plan)
.cocons.hip.vecchia.set.groups <- function(fit, group) {
  .Call(`_cocons_hip_vecchia_set_groups`, fit, as.integer(group))
}

# .cocons.hip.vecchia.neg2loglik on the grouped schedule: the same value to the bit, one factorisation per block
.cocons.hip.vecchia.neg2loglik.grouped <- function(fit, theta, par.pos, smooth.limits, n, r, lambda, safe = TRUE) {
  theta_list <- getModelLists(theta = theta, par.pos = par.pos, type = "diff")
  v <- .cocons.hip.result(.Call(`_cocons_hip_vecchia_neg2loglik_grouped`, fit, theta_list[-1], theta_list$mean), safe)
  if (is.null(v)) return(1e+06)
  v[1] + .cocons.getPen(n * r, lambda, theta_list, smooth.limits)
}

# .cocons.hip.vecchia.neg2loglik.grad on the grouped schedule (DESIGN.md 4z): the same list -- the value to the bit, the gradient
# of the same model to rounding --, from one factorisation per block and every pair of a block evaluated once
.cocons.hip.vecchia.neg2loglik.grad.grouped <- function(fit, theta_list, safe = TRUE) {
  res <- .cocons.hip.result(.Call(`_cocons_hip_vecchia_neg2loglik_grad_grouped`, fit, theta_list[-1], theta_list$mean), safe)
  if (is.null(res)) return(NULL)
  list(value = res[[1]], table = res[[2]], quad = res[[3]], mean = res[[4]])
}

# .cocons.hip.vecchia.fisher on the grouped schedule (cocons_fisher_vecchia_grouped; DESIGN.md 4aa): the same P x P matrix of
# the same model to rounding, from one factorisation per block; the fit needs a plan (.cocons.hip.vecchia.set.groups
# attaches one)
.cocons.hip.vecchia.fisher.grouped <- function(fit, theta, par.pos, safe = TRUE) {
  .cocons.hip.vecchia.fisher(fit, theta, par.pos, safe, grouped = TRUE)
}

# U W for the n x c matrix W and log d on the grouped schedule: list(out, logd)
.cocons.hip.vecchia.whiten.grouped <- function(fit, theta_list, W) {
  W <- as.matrix(W)
  storage.mode(W) <- "double"
  res <- .Call(`_cocons_hip_vecchia_whiten_grouped`, fit, theta_list[names(theta_list) != "mean"], W)
  if (res[[1]] > 0L) stop("Cholesky error")
  list(out = res[[2]][[1]], logd = res[[2]][[2]])
}

# cross-validated predictions of the Vecchia model (cocons_cv_vecchia): what .cocons.hip.cv returns, from U'U -- no refit and
# no n x n matrix.  fold: one label of any kind per observation, every fold of at most 128 observations (NULL: leave-one-out)
.cocons.hip.vecchia.cv <- function(fit, theta_list, fold = NULL, safe = TRUE) {
  .cocons.hip.vecchia.cv.by(`_cocons_hip_vecchia_cv`, fit, theta_list, fold, safe)
}

# the one body of .cocons.hip.vecchia.cv and .cocons.hip.vecchia.cv.grouped
.cocons.hip.vecchia.cv.by <- function(shim, fit, theta_list, fold, safe) {
  if (!is.null(fold)) fold <- match(fold, unique(fold)) - 1L
  res <- .cocons.hip.result(.Call(shim, fit, theta_list, fold), safe)
  if (is.null(res)) return(NULL)
  list(resid = res[[1]], var = res[[2]], stats = res[[3]])
}

# U^-1, U' and cross-validation with the rows' coefficients from one factorisation per block (DESIGN.md 4ab;
# cocons_vecchia_unwhiten_grouped, cocons_sim_vecchia_grouped, cocons_vecchia_whiten_t_grouped, cocons_cv_vecchia_grouped): the
# bits of the ungrouped wrappers on the same fit, through their bodies (the wrappers' own argument lists are part of the layer's
# contract, so the switch is the shim that the shared body calls); the fit needs a plan (.cocons.hip.vecchia.set.groups
# attaches one)
.cocons.hip.vecchia.unwhiten.grouped <- function(fit, theta_list, W) {
  .cocons.hip.vecchia.unwhiten.by(`_cocons_hip_vecchia_unwhiten_grouped`, fit, theta_list, W)
}

.cocons.hip.vecchia.sim.grouped <- function(fit, theta_list, iiderrors, n_fixed = 0L, z_col = 1L) {
  .cocons.hip.vecchia.sim.by(`_cocons_hip_vecchia_sim_grouped`, fit, theta_list, iiderrors, n_fixed, z_col)
}

.cocons.hip.vecchia.whiten.t.grouped <- function(fit, theta_list, W) {
  .cocons.hip.vecchia.whiten.t.by(`_cocons_hip_vecchia_whiten_t_grouped`, fit, theta_list, W)
}

.cocons.hip.vecchia.cv.grouped <- function(fit, theta_list, fold = NULL, safe = TRUE) {
  .cocons.hip.vecchia.cv.by(`_cocons_hip_vecchia_cv_grouped`, fit, theta_list, fold, safe)
}
