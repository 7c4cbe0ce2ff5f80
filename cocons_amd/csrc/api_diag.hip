// api_diag.hip -- C ABI, what only tools and tests call (include/cocons_hip_diag.h): host time per enqueued evaluation, the
// right-hand-side layout, the report of a hand-off time-out (info_status calls it under COCONS_DEBUG_ABORT), the DAG
// schedule's trace and task words, the event-timed profile of an evaluation, the assembly loop, and the persistent launch
// replayed alone.  It reaches into the evaluation path through the block of internals fit.hpp declares for it.
#include "fit.hpp"

// (diagnostics) out[0] = mean host microseconds per enqueued evaluation of this handle and its batch slots, out[1] = evaluations
extern "C" int cocons_debug_host_enqueue(cocons_fit *f, double *out)
{
    if (!f || !out) return fail(-1, "cocons_debug_host_enqueue: null argument");
    double us = f->enq_host_us; long long n = f->enq_calls;
    for (cocons_fit *c : f->slots) { us += c->enq_host_us; n += c->enq_calls; }
    out[0] = n ? us / (double)n : 0.0; out[1] = (double)n;
    return 0;
}

// (diagnostics, no HIP call) where an operation with r + nxb right-hand sides puts them on this handle: rhs_layout itself
// the pattern builder's grid and the clamped cells of given points, from pattern_grid.hpp as the kernels use it (host only)
extern "C" int cocons_debug_pattern_cells(int n, const double *locs, double delta, int m, const double *pts, double *geom5, int *cells)
{
    const char *who = "cocons_debug_pattern_cells";
    if (!locs || !geom5 || n < 1 || m < 0 || (m > 0 && (!pts || !cells))) return fail(-1, "%s: bad argument", who);
    if (!std::isfinite(delta) || delta <= 0.0) return fail(-1, "%s: delta must be finite and > 0", who);
    for (size_t i = 0; i < (size_t)2 * n; ++i)
        if (!std::isfinite(locs[i])) return fail(-1, "%s: a target coordinate is not finite", who);
    const PatternGrid g = pattern_grid_make(n, locs, locs + n, delta);
    geom5[0] = g.x0; geom5[1] = g.y0; geom5[2] = g.edge; geom5[3] = g.nx; geom5[4] = g.ny;
    for (int i = 0; i < m; ++i) {
        cells[2 * i] = pattern_cell_x(g, pts[i]);
        cells[2 * i + 1] = pattern_cell_y(g, pts[i + (size_t)m]);
    }
    return 0;
}

extern "C" int cocons_debug_rhs_layout(cocons_fit *f, int nxb, int *out5)
{
    if (!f || !out5 || nxb < 0) return fail(-1, "cocons_debug_rhs_layout: bad argument");
    const RhsLayout l = rhs_layout(f, f->r + nxb);
    out5[0] = f->pad0; out5[1] = f->nslot; out5[2] = l.slots ? 1 : 0; out5[3] = l.tile_rows; out5[4] = l.trim;
    return 0;
}

// COCONS_DEBUG_ABORT=1: say which wait gave up (0x1tt / 0x2tt engine waiting for tile tt, 0x3tt panel solve waiting for the
// engine's tile tt, 0x5.. in-panel update, 0x600 the gate waiting for the engine to be resident, 0x900 the reductions waiting
// for the engine's last tile: kernels.h, abort_code / abort_class)
void debug_abort_report(cocons_fit *f)
{
    fprintf(stderr, "cocons: hand-off time-out, code 0x%x\n", f->hinfo[1]);
    const unsigned cls = abort_class((unsigned)f->hinfo[1]);
    if (!f->dag_used || !f->ddag || cls < ABORT_DAG_FIRST || cls > ABORT_DAG_LAST) return;
    // a wait of the DAG launch: what it waited for (dag_wait's record) and what the word holds NOW
    unsigned rec[7] = {0, 0, 0, 0, 0, 0, 0}, now = 0, qn = 0;
    const DagWords W = dag_words(f, f->dag_key[1]);       // (the word indices of the record count from the task counter)
    hipMemcpyAsync(rec, W.wait_record, sizeof rec, hipMemcpyDeviceToHost, f->stream);
    hipStreamSynchronize(f->stream);
    if (rec[2] < f->ddag.count()) hipMemcpyAsync(&now, &W.queue[rec[2]], sizeof now, hipMemcpyDeviceToHost, f->stream);
    hipMemcpyAsync(&qn, W.queue, sizeof qn, hipMemcpyDeviceToHost, f->stream);
    hipStreamSynchronize(f->stream);
    fprintf(stderr, "cocons: DAG wait: task %u (of %u, counter now %u) code 0x%x waited for word %u >= %u, saw %u, holds %u now; "
            "%.1f ms, %u polls\n", rec[0], f->dag_ntasks, qn, rec[1], rec[2], rec[3], rec[4], now, rec[5] * 1e-5, rec[6]);
    if (const char *dump = getenv("COCONS_DEBUG_ABORT_DUMP")) {
        // everything an offline look needs (tools/dag_abort.py): header, record, step table, all task words, the engine's
        // flag words, and with tracing on the stamps of every task and of the engine
        static int ndump = 0;
        char path[512];
        snprintf(path, sizeof path, "%s.%d", dump, ndump++);
        if (FILE *fp = fopen(path, "wb")) {
            const unsigned ntr = f->dag_trace_tasks ? 1u : 0u;
            unsigned hdr[16] = {0xDA6D0001u, (unsigned)f->nt, (unsigned)f->dag_nsteps, f->dag_ntasks, (unsigned)f->ddag.count(),
                                (unsigned)f->flags_cap, ntr, (unsigned)f->hinfo[1], qn, now, 0, 0, 0, 0, 0, 0};
            fwrite(hdr, sizeof hdr, 1, fp);
            fwrite(rec, sizeof rec, 1, fp);
            std::vector<DagStepHost> sh((size_t)f->dag_nsteps);
            hipMemcpyAsync(sh.data(), f->ddag_steps, sh.size() * sizeof(DagStepHost), hipMemcpyDeviceToHost, f->stream);
            std::vector<unsigned> w((size_t)f->ddag.count()), fl(handoff_word_count(f->flags_cap));
            hipMemcpyAsync(w.data(), f->ddag, w.size() * sizeof(unsigned), hipMemcpyDeviceToHost, f->stream);
            hipMemcpyAsync(fl.data(), f->dflags, fl.size() * sizeof(unsigned), hipMemcpyDeviceToHost, f->stream);
            hipStreamSynchronize(f->stream);
            fwrite(sh.data(), sizeof(DagStepHost), sh.size(), fp);
            fwrite(w.data(), sizeof(unsigned), w.size(), fp);
            fwrite(fl.data(), sizeof(unsigned), fl.size(), fp);
            if (ntr) {
                std::vector<unsigned long long> st(dag_trace_words(f, f->nt).count);
                hipMemcpyAsync(st.data(), f->ddag_trace, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream);
                hipStreamSynchronize(f->stream);
                fwrite(st.data(), sizeof(unsigned long long), st.size(), fp);
            }
            fclose(fp);
            fprintf(stderr, "cocons: state written to %s\n", path);
        }
    }
    if (f->dag_trace_tasks && !getenv("COCONS_DEBUG_ABORT_DUMP")) {
        // which tasks were drawn and never finished (stamps: drawn, inputs complete, product done, stored)
        std::vector<unsigned long long> st((size_t)f->dag_ntasks * 4);
        hipMemcpyAsync(st.data(), f->ddag_trace, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream);
        hipStreamSynchronize(f->stream);
        unsigned long long tmin = ~0ull;
        for (size_t i = 0; i < st.size(); i += 4) if (st[i] && st[i] < tmin) tmin = st[i];
        int shown = 0;
        for (unsigned L = 0; L < f->dag_ntasks && shown < 40; ++L) {
            const unsigned long long *q = &st[(size_t)L * 4];
            if (q[0] && !q[3]) {
                fprintf(stderr, "   unfinished task %u: drawn %.1f us, inputs %s, product %s\n", L, (q[0] - tmin) * 0.01,
                        q[1] ? "complete" : "WAITING", q[2] ? "done" : "-");
                ++shown;
            }
        }
    }
}

// diagnostics: the step table and the per-task stamps of the last DAG factorisation of the handle (dag_trace = 1).
// steps_out: nsteps x 16 ints (DagStepHost); stamps_out: ntasks x 4 ticks of the 100 MHz clock.  Returns ntasks (or < 0);
// with null outputs only the sizes: *nsteps_out.  engine_out (may be null): 8 stamps per tile pair, (nt + 2) / 2 pairs ... room
// for 8 * (nt + 2) values (see EngineArgs::trace).
extern "C" long long cocons_debug_dag_trace(cocons_fit *f, int *nsteps_out, int *steps_out, unsigned long long *stamps_out,
                                            unsigned long long *engine_out)
{
    FIT_ENTER(f);
    if (!f->ddag_steps) return fail(-1, "cocons_debug_dag_trace: no DAG factorisation on this handle yet");
    if (nsteps_out) *nsteps_out = f->dag_nsteps;
    HIPCHK(hipStreamSynchronize(f->stream));
    // (asynchronous copies on the handle's own stream: a synchronous hipMemcpy runs on the NULL stream, gives it a hardware
    // queue and shifts every later stream's assignment -- the tool would perturb what it observes)
    if (steps_out)
        HIPCHK(hipMemcpyAsync(steps_out, f->ddag_steps, (size_t)f->dag_nsteps * sizeof(DagStepHost), hipMemcpyDeviceToHost, f->stream));
    if (stamps_out) {
        if (!f->ddag_trace || f->dag_trace_tasks != f->dag_ntasks)
            return fail(-1, "cocons_debug_dag_trace: tracing was off (cocons_debug_tune(\"dag_trace\", 1))");
        const DagTraceWords tw = dag_trace_words(f, f->nt);
        HIPCHK(hipMemcpyAsync(stamps_out, tw.tasks, (size_t)f->dag_ntasks * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream));
        if (engine_out)
            HIPCHK(hipMemcpyAsync(engine_out, tw.engine, tw.engine_count * sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream));
    }
    HIPCHK(hipStreamSynchronize(f->stream));
    return (long long)f->dag_ntasks;
}

// (diagnostics) the first `count` task words of the handle's last dependency-driven factorisation: [0] the one task counter,
// [8..14] the record of a wait that ran out, [16..23] workgroups that took part per XCD, [32..39] the XCDs' own task counters
extern "C" int cocons_debug_dag_words(cocons_fit *f, int count, unsigned *out)
{
    FIT_ENTER(f);
    if (!f->ddag || !out || count < 1 || (size_t)count > f->ddag.count()) return fail(-1, "cocons_debug_dag_words: bad argument or no DAG factorisation yet");
    HIPCHK(hipStreamSynchronize(f->stream));
    HIPCHK(hipMemcpyAsync(out, f->ddag, (size_t)count * sizeof(unsigned), hipMemcpyDeviceToHost, f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
    return 0;
}

// ---------------------------------------------------------------------------
extern "C" int cocons_fit_profile(cocons_fit *f, const double *theta, const double *mean, int reps, double *ms)
{
    FIT_ENTER(f);
    if (int rc = no_taper(f, "cocons_fit_profile")) return rc;
    if (!theta || !mean || !ms || reps < 1) return fail(-1, "cocons_fit_profile: bad argument");
    for (;;) {
        double acc[7] = {0, 0, 0, 0, 0, 0, 0};
        double dag_ms = 0.0;
        for (int it = 0; it < reps; ++it) {
            std::vector<hipEvent_t> ev;
            f->upd_flops = 0.0;
            f->dag_flops = 0.0; f->dag_events = 0;
            if (int rc = enqueue_eval(f, theta, mean, true, nullptr, 0, &ev, true)) return rc;
            HIPCHK(hipStreamSynchronize(f->stream));
            float t01, t12, t23, t03;
            HIPCHK(hipEventElapsedTime(&t01, f->ev[0], f->ev[1]));
            HIPCHK(hipEventElapsedTime(&t12, f->ev[1], f->ev[2]));
            HIPCHK(hipEventElapsedTime(&t23, f->ev[2], f->ev[3]));
            HIPCHK(hipEventElapsedTime(&t03, f->ev[0], f->ev[3]));
            acc[0] += t01; acc[1] += t12; acc[2] += t23; acc[3] += t03;
            double sum = 0;
            for (size_t i = 0; i + 1 < ev.size(); i += 2) {
                float t;
                HIPCHK(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
                sum += t;
                if (i == 0 && f->dag_events) dag_ms += t;
            }
            acc[6] += sum;
            acc[5] = (double)(ev.size() / 2);
            for (auto e : ev) hipEventDestroy(e);
        }
        for (int i = 0; i < 4; ++i) ms[i] = acc[i] / reps;
        ms[5] = acc[5];
        ms[6] = acc[6] / reps;
        ms[4] = acc[5] > 0 ? ms[6] / acc[5] : 0.0;
        ms[7] = f->upd_flops;
        ms[8] = dag_ms / reps;
        ms[9] = f->dag_flops;
        int st = info_status(f);
        if (engine_retry(f, st)) continue;
        return st;
    }
}

// (diagnostics) the covariance assembly of an evaluation ALONE, `reps` times back to back on the handle's stream between two
// events: ms_out[0] = mean milliseconds per assembly.  tools/diag/overlap_probe.py runs it on one handle while another thread
// evaluates on a second handle: what the assembly (fp64 vector work) and the factorisation (fp64 matrix work) cost each other
// when they share the chip -- the measurement behind DESIGN.md section 8 "Assembly beside the factorisation".
extern "C" int cocons_debug_assembly_loop(cocons_fit *f, const double *theta, int reps, double *ms_out)
{
    FIT_ENTER(f);
    if (int rc = no_taper(f, "cocons_debug_assembly_loop")) return rc;
    if (!theta || !ms_out || reps < 1) return fail(-1, "cocons_debug_assembly_loop: bad argument");
    if (int rc = fit_alloc_matrix(f, f->r > 0 ? f->r : 1)) return rc;
    hipEventRecord(f->ev[0], f->stream);
    for (int i = 0; i < reps; ++i) assemble_sigma(f, theta, 0, 0, f->npad);
    hipEventRecord(f->ev[1], f->stream);
    HIPCHK(hipStreamSynchronize(f->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, f->ev[0], f->ev[1]));
    ms_out[0] = (double)ms / reps;
    return 0;
}

// ---------------------------------------------------------------------------
// diagnostic: the persistent launch of the dependency-driven schedule (dag_kernel) REPLAYED ALONE -- the same task list, the
// same products, the same C traffic, but nobody to wait for: what the engine would publish while the launch runs (the
// inverses W of the diagonal tiles, the strips X(t+1,t), the raised out[] / xr[] words) is put there beforehand, taken from
// a factorisation of the same matrix on the plain schedule.  This is what makes the launch countable: rocprofv3 --pmc
// serialises kernels, and the real launch waits for the engine on the other stream.
// Sequence: (1) evaluation on the plain schedule -> the complete factor L in the handle's buffer; (2) W(t) = L(t,t)^-1
// (host, 128 x 128 triangular) and L(t+1,t) for every diagonal block of the head into the W buffer / the second buffer P, and
// a copy of L for the check; (3) per repetition: Sigma assembled again, first panel by the classic kernels, task words zeroed,
// in[] / out[] / xr[] raised, dag_kernel launched between two events.  The launch leaves the diagonal blocks updated but
// unfactored (no engine), so no value comes out of a replay; the check is the panels it formed against the plain factor.
// out[0] = mean duration of the launch in ms, out[1] = its update flops (as bench.py counts them), out[2] = max |P - L| over
// the panels the launch formed relative to max |L| there, out[3] = tasks, out[4] = steps.
__global__ void __launch_bounds__(256)
panel_diff_kernel(const double *P, const double *L, size_t lda, int c0, int c1, int rend, unsigned long long *out)
{
    const int c = c0 + (int)blockIdx.x;
    if (c >= c1) return;
    const int r0 = 2 * TILE * (c / (2 * TILE) + 1);          // first row below column c's diagonal block
    double md = 0.0, ml = 0.0;
    for (int r = r0 + (int)threadIdx.x; r < rend; r += (int)blockDim.x) {
        const double l = L[(size_t)r + (size_t)c * lda], d = fabs(P[(size_t)r + (size_t)c * lda] - l);
        md = d > md || d != d ? d : md;
        ml = fabs(l) > ml ? fabs(l) : ml;
    }
    // (non-negative doubles order like their bit patterns; a NaN difference has the largest pattern of all)
    atomicMax(out, (unsigned long long)__double_as_longlong(md));
    atomicMax(out + 1, (unsigned long long)__double_as_longlong(ml));
}

// (3) of cocons_debug_dag_replay: fv is the factor's view, prepared for the DAG schedule
static int dag_replay_run(cocons_fit *f, const FactorView &fv, bool slots, const double *theta, const double *mean, int reps,
                          double *out)
{
    static const char *const tiles_failed = "cocons_debug_dag_replay: copying the diagonal tiles failed";
    const int nrhs = f->r;
    const size_t lda = fv.lda;
    const int nt_head = 2 * f->dag_nsteps + 2;                 // diagonal tiles 2 .. nt_head - 1 belong to the head's blocks
    std::vector<double> tile((size_t)TILE * TILE), W((size_t)TILE * TILE);
    DevBuf<double> Lcopy;
    DevBuf<unsigned long long> dcmp;
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
    } ev;
    StreamDrain M{f->stream, false};
    // (2) what the engine would publish
    HIPCHK_AT("cocons_debug_dag_replay", Lcopy.alloc(lda * (size_t)f->npad));
    HIPCHK_AT("cocons_debug_dag_replay", hipMemcpyAsync(Lcopy, f->dA, lda * (size_t)f->npad * sizeof(double), hipMemcpyDeviceToDevice, M));
    for (int t = 2; t < nt_head && t < fv.nt; ++t) {
        const double *src = f->dA + (size_t)t * TILE + (size_t)t * TILE * lda;
        if (hipMemcpy2DAsync(tile.data(), TILE * sizeof(double), src, lda * sizeof(double), TILE * sizeof(double), TILE,
                             hipMemcpyDeviceToHost, M) != hipSuccess || hipStreamSynchronize(M) != hipSuccess) return fail(-100, tiles_failed);
        std::fill(W.begin(), W.end(), 0.0);
        for (int j = 0; j < TILE; ++j)                     // column j of W = L^-1: forward substitution on e_j
            for (int i = j; i < TILE; ++i) {
                double sacc = i == j ? 1.0 : 0.0;
                for (int k = j; k < i; ++k) sacc -= tile[(size_t)i + (size_t)k * TILE] * W[(size_t)k + (size_t)j * TILE];
                W[(size_t)i + (size_t)j * TILE] = sacc / tile[(size_t)i + (size_t)i * TILE];
            }
        if (hipMemcpyAsync(f->dWt + (size_t)t * TILE * TILE, W.data(), W.size() * sizeof(double), hipMemcpyHostToDevice, M) != hipSuccess ||
            hipStreamSynchronize(M) != hipSuccess) return fail(-100, tiles_failed);
        if ((t & 1) == 0 && t + 1 < fv.nt) {               // X(t+1,t) = L(t+1,t): the engine's second copy, in P
            const size_t off = (size_t)(t + 1) * TILE + (size_t)t * TILE * lda;
            if (hipMemcpy2DAsync(f->dP + off, lda * sizeof(double), f->dA + off, lda * sizeof(double), TILE * sizeof(double), TILE,
                                 hipMemcpyDeviceToDevice, M) != hipSuccess) return fail(-100, tiles_failed);
        }
    }
    HIPCHK_AT("cocons_debug_dag_replay", dcmp.alloc(2));
    // (3) the launch, alone
    const HandoffWords hw = handoff_words(f);
    const DagLaunch d = dag_launch(f, fv, hw, hw.alive);
    f->upd_flops = 0.0;
    f->nrhs_cur = nrhs;
    for (int s2 = 0; s2 < f->dag_nsteps; ++s2) count_update_flops(f, 2, 2 * s2 + 2);
    const double flops = f->upd_flops;
    HIPCHK_AT("cocons_debug_dag_replay", hipEventCreate(&ev.a));
    HIPCHK_AT("cocons_debug_dag_replay", hipEventCreate(&ev.b));
    double ms_sum = 0.0;
    for (int it = 0; it < reps; ++it) {
        if (int rc = reset_info(f)) return rc;
        assemble_sigma(f, theta, 0, 0, f->npad);
        assemble_rhs(f, mean, true, nullptr, 0, 0, f->npad, true, slots);
        launch_front_identity(fv.A, fv.lda, f->pad0, fv.mt * TILE, M);
        panel_ops(f, fv, 0, M);
        HIPCHK_AT("cocons_debug_dag_replay", hipMemsetAsync(f->ddag, 0, f->ddag.count() * sizeof(unsigned), M));
        HIPCHK_AT("cocons_debug_dag_replay", hipMemsetD32Async((hipDeviceptr_t)f->dflags, 0x3fffffff, 3 * (size_t)f->flags_cap, M));   // in / out / xr: all raised
        // (as many workgroups take part as in a real evaluation: the engine and its partner are entered on XCD 0 by hand)
        static const unsigned pair_on_xcd0 = 2u;
        HIPCHK_AT("cocons_debug_dag_replay", hipMemcpyAsync(hw.xcd_arrivals, &pair_on_xcd0, sizeof(unsigned), hipMemcpyHostToDevice, M));
        HIPCHK_AT("cocons_debug_dag_replay", hipEventRecord(ev.a, M));
        launch_dag(d, M);
        HIPCHK_AT("cocons_debug_dag_replay", hipEventRecord(ev.b, M));
        HIPCHK_AT("cocons_debug_dag_replay", hipGetLastError());
        HIPCHK_AT("cocons_debug_dag_replay", hipStreamSynchronize(M));
        float ms = 0;
        HIPCHK_AT("cocons_debug_dag_replay", hipEventElapsedTime(&ms, ev.a, ev.b));
        ms_sum += ms;
    }
    HIPCHK_AT("cocons_debug_dag_replay", hipMemcpyAsync(f->hinfo, f->dinfo, 2 * sizeof(int), hipMemcpyDeviceToHost, M));
    HIPCHK_AT("cocons_debug_dag_replay", hipStreamSynchronize(M));
    if (f->hinfo[1] != 0) return fail(ENGINE_ABORT, "cocons_debug_dag_replay: a wait of the replayed launch ran out");
    // the check: every panel the launch formed (blocks 1 .. nsteps - 1) against the plain factor
    HIPCHK_AT("cocons_debug_dag_replay", hipMemsetAsync(dcmp, 0, 2 * sizeof(unsigned long long), M));
    const int c0 = 2 * TILE, c1 = 2 * TILE * f->dag_nsteps, rend = fv.mt * TILE - 64 * fv.trim;
    hipLaunchKernelGGL(panel_diff_kernel, dim3(c1 - c0), dim3(256), 0, M, (const double *)f->dP, (const double *)Lcopy, lda, c0, c1, rend,
                       dcmp.get());
    unsigned long long h[2] = {0, 0};
    HIPCHK_AT("cocons_debug_dag_replay", hipMemcpyAsync(h, dcmp, sizeof h, hipMemcpyDeviceToHost, M));
    HIPCHK_AT("cocons_debug_dag_replay", hipStreamSynchronize(M));
    double md, ml;
    memcpy(&md, &h[0], 8); memcpy(&ml, &h[1], 8);
    out[0] = ms_sum / reps; out[1] = flops; out[2] = ml > 0 ? md / ml : NAN; out[3] = (double)f->dag_ntasks; out[4] = (double)f->dag_nsteps;
    return 0;
}

extern "C" int cocons_debug_dag_replay(cocons_fit *f, const double *theta, const double *mean, int reps, double *out)
{
    FIT_ENTER(f);
    if (int rc = no_taper(f, "cocons_debug_dag_replay")) return rc;
    if (!theta || !mean || !out || reps < 1) return fail(-1, "cocons_debug_dag_replay: bad argument");
    if (f->r < 1 || f->coll_kind) return fail(-1, "cocons_debug_dag_replay: needs a plain dense fit with z");
    // (1) the factor, on the plain schedule
    const int engine_saved = tun().engine;
    tun().engine = 0;
    int st = enqueue_eval(f, theta, mean, true, nullptr, 0, nullptr, false);
    if (st == 0) { HIPCHK(hipStreamSynchronize(f->stream)); st = info_status(f); }
    tun().engine = engine_saved;
    if (st) return st;
    const int nrhs = f->r;
    const RhsLayout lay = rhs_layout(f, nrhs);
    const bool slots = lay.slots;
    FactorView fv = rhs_view(f, lay);
    fv.dag_ok = true;
    if (!(tun().dag != 0 && !fv.hi && !fv.skew && fv.nt > 4)) return fail(-1, "cocons_debug_dag_replay: the DAG schedule does not apply to this fit");
    if (int rc = flags_reset(f, fv.nt)) return rc;
    if (int prc = dag_prepare(f, fv)) return prc;
    if (f->dag_nsteps < 2) return fail(-1, "cocons_debug_dag_replay: problem too small for a DAG head");
    const int rc = dag_replay_run(f, fv, slots, theta, mean, reps, out);
    border_unknown(f);        // (the buffer holds a half-done factorisation)
    f->dag_used = false;
    return rc;
}
