/* cocons_hip_diag.h -- diagnostic entry points of libcocons_hip.so.
 *
 * NOT part of the drop-in boundary (include/cocons_hip.h): nothing here replaces a reference interface and no
 * caller of the package needs it: the pointwise evaluation of the device Matern routine that the parity tests pin
 * against mpmath, the run-time schedule switches, the per-task trace and the counter replay of the persistent launch.
 * (The bare-instruction probes of the fp64 pipes live in a library of their own since round 5: cocons_hip_probes.h,
 * libcocons_hip_probes.so -- the product library contains none of their kernels.)  Same conventions as the product
 * header: extern "C", host pointers, int status, no HIP call at load time.
 */
#ifndef COCONS_HIP_DIAG_H
#define COCONS_HIP_DIAG_H

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: the device routine that replaces boost::math::cyl_bessel_k + tgamma + pow at
 * src/cocons_full.cpp:293-297 (:301-305 for u >= 706), evaluated pointwise:
 * out[i] = 2^(1-nu_i)/Gamma(nu_i) * u_i^nu_i * K_nu_i(u_i).  Pinned against the mpmath grid in
 * tests/golden/besselk_grid.json (host arrays in, host array out).                    */
int cocons_debug_matern(int n, const double *nu, const double *u, double *out);

/* Diagnostics of cocons_neg2loglik_grad_dense: the lower triangle of the Sigma(theta)^-1 the gradient uses, in the caller's
 * observation order (n x n column-major host array, zeros above the diagonal; 0, a failing minor k > 0, or < 0), and
 * M, dM/du, dM/dnu of the gradient's device routine at n points (out3n[i], out3n[n + i], out3n[2 n + i]; dM/dnu by a
 * four-point central difference in nu; u >= 706: the reference's stand-in for M, zero derivatives).                */
int cocons_debug_sigma_inverse(struct cocons_fit *fit, const double *theta, double *out_nxn);
int cocons_debug_matern_grad(int n, const double *nu, const double *u, double *out3n);

/* Device memory of a dense handle: out4 = { bytes allocated for the matrix buffer, bytes of the dependency-driven schedule's
 * second buffer, bytes of the gradient's scratch, the leading dimension the objective's matrix uses }.              */
int cocons_debug_fit_memory(struct cocons_fit *fit, long long *out4);

/* Where an operation with r + nxb right-hand sides (nxb = 0: the dense objective, q: Profile, p: REML) carries them through the
 * factorisation on this handle, from the function every evaluation asks: out5 = { pad0 (placeholder observations in front),
 * nslot (slot rows the handle keeps in the matrix's last tile), 1 if these right-hand sides ride in the slots, tile rows of
 * 128 under the matrix it factors (0 with slots), trim (1: the last 64 of those rows hold nothing) }.  Host only: no HIP
 * call.  0, or -1 on a null argument or nxb < 0.                                                                          */
int cocons_debug_rhs_layout(struct cocons_fit *fit, int nxb, int *out5);

/* The grid of the taper-pattern builder (cocons_taper_pattern, cocons_krige_taper_apply_delta) for n targets (locs, n x 2
 * column-major) and delta, and the clamped cell of each of m points (pts, m x 2 column-major), both from the header the
 * kernels use: geom5 = { origin x, origin y, cell edge, cells along x, cells along y }, cells = m pairs (cx, cy), each
 * coordinate in [-1, count] (-1 and count: outside the targets' box on that side).  Host only: no HIP call.  0, or -1 on a
 * null argument, n < 1, m < 0, a delta that is not finite or <= 0, or a target coordinate that is not finite.            */
int cocons_debug_pattern_cells(int n, const double *locs, double delta, int m, const double *pts, double *geom5, int *cells);

/* The plan of the Vecchia neighbour search (cocons_vecchia_neighbours) for n points (locs, n x 2 column-major),
 * from the header the kernels use: plan = { head (rows searched by brute force), L (levels), then L pairs (lo, hi): rows
 * [lo, hi) search the grid over the first hi points } -- room for 2 + 2 * 32 ints; geom5 = L + 1 records { origin x,
 * origin y, cell edge, cells along x, cells along y }, one per level and a last one for the grid over all n points that plain
 * kNN searches (room for 5 * 33 doubles).  For the grid `level` in 0 .. L: cells = m pairs (cx, cy), the clamped cells of the
 * m points pts (m x 2 column-major), each coordinate in [-1, count]; bounds[r], r = 0 .. rmax (rmax = -1: none), the lower
 * bound on the d2 of anything outside the (2 r + 1)^2 block of cells around a query's clamped cell, at which the ring walk
 * stops.  Host only: no HIP call.  0, or -1 with the outputs untouched on a null argument, n < 1, m < 0, rmax < -1, a level
 * outside 0 .. L, or a coordinate of locs that is not finite.                                                              */
int cocons_debug_knn_plan(int n, const double *locs, int level, int m, const double *pts, int rmax, int *plan, double *geom5,
                          int *cells, double *bounds);

/* The two phases of the ordered self search of cocons_vecchia_neighbours(n, locs, 0, NULL, m, device, ..), timed by events on
 * the search's stream: ms2 = { device milliseconds of binning the levels, device milliseconds of the query launches (the
 * head's included) }.  The search runs as it does there, its table stays on the device and is dropped.  For
 * tools/vecchia_knn_timing.py.  0, or < 0 with the refusals of cocons_vecchia_neighbours under this entry's name.        */
int cocons_debug_knn_phases(int n, const double *locs, int m, int device, double *ms2);

/* The three phases of cocons_vecchia_neighbours_corr(fit, theta, m_cand, hops, m, ..), timed by events on the
 * handle's stream: ms3 = { device milliseconds of the Euclidean search of width m_cand, of the records at theta, of the
 * re-ranking launch }.  The call runs as it does there; its table stays on the device and is dropped.  For
 * tools/vecchia_corr_timing.py.  0, or the returns and refusals of cocons_vecchia_neighbours_corr under this entry's name.   */
int cocons_debug_knn_corr_phases(cocons_fit *fit, const double *theta, int m_cand, int hops, int m, double *ms3);

/* The rounds of cocons_vecchia_group_device(n, m, nn, max_rows, max_rounds, device, ..), timed by events on the
 * call's stream: for every round launched -- the one that finds no proposal included --, live[t] = the blocks alive at its
 * start and ms[t] = the device milliseconds of its three launches; at most cap rounds are recorded.  The rounds run as they
 * do there; the labels stay on the device and are dropped.  For tools/vecchia_group_device_timing.py.  Returns the number
 * of rounds recorded (>= 1: live[0 .. return) and ms[0 .. return) are written) -- one more than the rounds that merged when the
 * run ended by itself, exactly max_rounds when the cap ended it --, or < 0 with the refusals of cocons_vecchia_group_device
 * under this entry's name.                                                                                                */
int cocons_debug_group_rounds(int n, int m, const int *nn, int max_rows, int max_rounds, int device, int cap, int *live,
                              double *ms);

/* The plan of the maxmin ordering (cocons_vecchia_order) for n points (locs, n x 2 column-major), from the
 * header the kernels use: labels[i] = label(i) for i = 0 .. n - 1; geom3 = { centre x, centre y, L }; levels2 = 64 pairs
 * (l_k, e_k), k = 1 .. 64.  Host only: no HIP call.  0, or -1 with the outputs untouched on a null argument, n < 1, a
 * coordinate that is not finite or a span above 2^511.                                                                   */
int cocons_debug_order_plan(int n, const double *locs, int *labels, double *geom3, double *levels2);

/* cocons_vecchia_order(n, locs, device, order, level_counts) with its phases timed by events on the call's stream and its
 * work counted: ms4 = device milliseconds of { the upload and the relabelling, the dense levels' rounds, the binned levels'
 * binning and rounds, the levels' ends (counts, scan, scatter, the count's way home) }; stats5 = { levels walked, of them on
 * the dense grid, rounds, kernel launches, host reads of a counter }.  binned_from = 0: the schedule as it is there; k in
 * 1 .. 64: the binned schedule from level k on, whatever the plan says (the bits do not depend on it).  order and
 * level_counts may be NULL.  For tools/vecchia_order_timing.py and the tests.  0, or < 0 with the refusals of
 * cocons_vecchia_order under this entry's name.                                                                          */
int cocons_debug_order_phases(int n, const double *locs, int device, int binned_from, int *order, int *level_counts,
                              double *ms4, long long *stats5);

/* cocons_vecchia_unwhiten(fit, theta, c, W, out) with its three phases timed by events on the handle's stream: ms3 = { the
 * records and the coefficient launch with the status word's way home, the schedule (0 when the handle holds it already), the
 * upload of W and the solve's launches }, device milliseconds.  For tools/vecchia_sim_timing.py.  Returns and refusals as
 * cocons_vecchia_unwhiten's, under this entry's name.                                                                    */
int cocons_debug_vecchia_sim_phases(struct cocons_fit *fit, const double *theta, int c, const double *W, double *out,
                                    double *ms3);
/* cocons_debug_vecchia_sim_phases on the grouped schedule (cocons_vecchia_unwhiten_grouped): the first phase is
 * the records and the grouped coefficient launch.  For tools/vecchia_group_coef_timing.py.  Returns and refusals as
 * cocons_vecchia_unwhiten_grouped's, under this entry's name.                                                            */
int cocons_debug_vecchia_sim_phases_grouped(struct cocons_fit *fit, const double *theta, int c, const double *W, double *out,
                                            double *ms3);

/* The transposed lists of a Vecchia handle's table (cocons_vecchia_transpose) built anew, whether the handle holds them or
 * not, with the build's phases timed by events on the handle's stream: ms4 = { in-degree counts, the scan, the fill, the
 * sorts and the places }, device milliseconds.  For tools/vecchia_cv_timing.py.                                          */
int cocons_debug_vecchia_transpose_phases(struct cocons_fit *fit, double *ms4);

/* The tiers of the transposed Vecchia solve (cocons_vecchia_unwhiten_t), from the header the kernels use:
 * out4 = { VECCHIA_SOLVE_T_WIDE: a list of MORE than this many rows is summed by one workgroup, a shorter one by one
 * wavefront; the threads of that workgroup; the columns of a column group; the (row, column group) items a level may have to
 * join a fused run }.  Host only: no HIP call.  0, or -1 on a null argument.                                              */
int cocons_debug_vecchia_solve_t_tiers(int *out4);
/* cocons_vecchia_unwhiten_t(fit, theta, grouped, c, W, out) with its three phases timed by events on the handle's stream:
 * ms3 = { the records and the coefficient launch with the status word's way home, the transposed schedule (0 when the handle
 * holds it already), the launches of the transposed solve }, device milliseconds.  For tools/vecchia_cov_timing.py, which also
 * moves the tier threshold for a measurement with COCONS_VECCHIA_SOLVE_T_WIDE=<rows> (read when a schedule is made).  Returns
 * and refusals as cocons_vecchia_unwhiten_t's, under this entry's name.                                                   */
int cocons_debug_vecchia_solve_t_phases(struct cocons_fit *fit, const double *theta, int grouped, int c, const double *W,
                                        double *out, double *ms3);

/* Diagnostics of cocons_neg2loglik_grad_taper: (S(theta)^-1)_ij at every stored entry of the pattern the taper handle was
 * created with, in the caller's CSR order (out_nnz: one double per entry of that pattern), by the gradient's selected
 * inverse; bytes_out (may be NULL): the device bytes the gradient holds on the handle.  0, a failing minor k > 0, or < 0. */
int cocons_debug_taper_selinv(struct cocons_fit *fit, const double *theta, double *out_nnz, long long *bytes_out);

/* Schedule switches of the factorisation, settable at run time (the library reads the COCONS_* environment variables
 * of the same meaning once per process; DESIGN.md section 6 lists them): "engine", "engine_pair", "panel_fused", "panel_split",
 * "potrf_follow", "upd_waves", "w8_max_tiles", "dag", "dag_min_tiles", "dag_lead" / "dag_lead2" / "dag_lead3", "dag_xcc_quota",
 * "dag_xcd", "dag_order", "dag_bw", "dag_bh" (both at least 1), "dag_trace" (and, for the tests, "gate_sabotage", "host_delay_us",
 * "host_delay_tile", "engine_in_wait_ms", "dag_xcd_min_quota").  An unknown name returns -1.
 * For timing variants in alternation inside one process (tools/ab_modes.py); results do not depend on them beyond the
 * rounding of a different summation order.                                                                        */
int cocons_debug_tune(const char *name, int value);

/* Per-task time stamps of the last dependency-driven factorisation (cocons_debug_tune("dag", 1) and ("dag_trace", 1)) of a
 * fit handle: steps_out = nsteps x 16 ints (base, near, tpos, nT, H, W, tj0, k0, K, nstrip, two, need, nd_next, split, p2, p3), stamps_out =
 * ntasks x 4 ticks of the 100 MHz clock (drawn, inputs complete, product done, stored).  Returns ntasks; null outputs: sizes only. */
struct cocons_fit;
long long cocons_debug_dag_trace(struct cocons_fit *fit, int *nsteps_out, int *steps_out, unsigned long long *stamps_out,
                                 unsigned long long *engine_out);   /* engine_out (may be null): 8 stamps per pair of tiles, room for 8 (nt + 2) */


/* the first `count` task words of the last dependency-driven factorisation of the handle (host array out): [0] the one task counter,
 * [8..14] the record of a wait that ran out, [16..23] workgroups that took part per XCD, [32..39] the XCDs' own task counters */
int cocons_debug_dag_words(struct cocons_fit *fit, int count, unsigned *out);

/* host time spent ENQUEUEING evaluations on this handle and its batch slots: out2[0] = mean microseconds per evaluation, out2[1] = evaluations */
int cocons_debug_host_enqueue(struct cocons_fit *fit, double *out2);

/* The covariance assembly of an evaluation alone, `reps` times back to back: ms_out[0] = mean milliseconds per assembly
 * (tools/diag/overlap_probe.py: one handle assembling while another thread's handle factorises). */
int cocons_debug_assembly_loop(struct cocons_fit *fit, const double *theta, int reps, double *ms_out);

/* The persistent launch of the dependency-driven schedule replayed ALONE (counter passes: rocprofv3 --pmc serialises kernels,
 * and the real launch waits for the diagonal-block engine on another stream): what the engine would publish is prepared from
 * a plain-schedule factorisation of the same matrix, all hand-off words are raised, and dag_kernel runs the same task list --
 * same products, same C traffic -- between two HIP events, `reps` times.  out[0] = mean duration in ms, out[1] = the update
 * flops of the launch, out[2] = max |panel formed - plain factor| relative to max |factor| (the check), out[3] = tasks,
 * out[4] = steps.  tools/dag_replay.py.  */
int cocons_debug_dag_replay(struct cocons_fit *fit, const double *theta, const double *mean, int reps, double *out5);

/* Device times of the last successful cocons_sim_taper on the handle (twin != 0: on its pivot-order twin), out4[0..2] in ms:
 * assembly + factorisation, the band product (band_trmm_kernel), the gather into the caller's order; out4[3] = the
 * 128 x 128 envelope tiles the product reads per block of 64 draws.  tools/sim_taper_timing.py */
int cocons_debug_sim_taper_ms(struct cocons_fit *fit, int twin, double *out4);

#ifdef __cplusplus
}
#endif
#endif /* COCONS_HIP_DIAG_H */
