// api_order.hip -- C ABI of the maxmin ordering by scale-halving nets: the stateless cocons_vecchia_order over
// the plan of order_plan.hpp and the kernels of order.hip; the host-only cocons_debug_order_plan, which computes that plan with
// the header the kernels use; and cocons_debug_order_phases, which runs the ordering with its phases timed by events, counts
// levels, rounds and launches, and can force the binned schedule from a level on (the tests' proof that the bits do not depend
// on the schedule).
#include "fit.hpp"
#include "order_plan.hpp"

namespace {

constexpr int ORDER_BATCH = 4;          // rounds between two looks at the counters (one counter per round of a batch)
constexpr int ORDER_COUNTER_STRIDE = 32;    // ... 128 bytes apart

enum { PH_RELABEL = 0, PH_DENSE = 1, PH_BINNED = 2, PH_EMIT = 3, PH_COUNT = 4 };

struct OrderStats {
    long long levels = 0, dense_levels = 0, rounds = 0, launches = 0, reads = 0;
};

// Events on one stream, one in front of every stretch and its phase (cocons_debug_order_phases); off: nothing is recorded
struct OrderMarks {
    bool on;
    hipStream_t s;
    std::vector<hipEvent_t> ev;
    std::vector<int> phase;
    ~OrderMarks() { for (hipEvent_t e : ev) hipEventDestroy(e); }
    hipError_t mark(int ph)
    {
        if (!on) return hipSuccess;
        hipEvent_t e = nullptr;
        if (hipError_t rc = hipEventCreate(&e)) return rc;
        ev.push_back(e); phase.push_back(ph);
        return hipEventRecord(e, s);
    }
    // after the stream is drained: stretch k lies between marks k and k + 1 and belongs to phase[k]
    hipError_t sums(double *ms) const
    {
        for (size_t k = 0; k + 1 < ev.size(); ++k) {
            float t = 0.0f;
            if (hipError_t rc = hipEventElapsedTime(&t, ev[k], ev[k + 1])) return rc;
            ms[phase[k]] += t;
        }
        return hipSuccess;
    }
};

int order_refusals(const char *who, int n, const double *locs, bool have_out, OrderBox &box)
{
    if (!locs || !have_out) return fail(-1, "%s: null argument", who);
    if (n < 1) return fail(-1, "%s: n = %d (at least one point expected)", who, n);
    if (int rc = pattern_check_finite(who, "locs", (size_t)n, locs)) return rc;
    box = order_box_make(n, locs, locs + n);
    if (!(box.L <= ORDER_SPAN_MAX))
        return fail(-1, "%s: the points span %g, more than 2^511 (the squared distances would overflow)", who, box.L);
    return 0;
}

// rounds of one level until nothing is undecided; counters: ORDER_BATCH slots, host-read after every batch
template <class Round> int order_rounds(const char *who, const OrderArgs &a, unsigned *counters, hipStream_t s, OrderStats &st,
                                        Round &&round)
{
    unsigned host[ORDER_BATCH * ORDER_COUNTER_STRIDE];
    for (long long done = 0;; done += ORDER_BATCH) {
        // every round decides the lowest undecided label at least: R rounds are enough
        if (done > (long long)a.R) return fail(-2, "%s: a level did not end within %d rounds", who, a.R);
        HIPCHK_AT(who, hipMemsetAsync(counters, 0, sizeof host, s));
        for (int b = 0; b < ORDER_BATCH; ++b) {
            OrderArgs r = a;
            r.counter = counters + b * ORDER_COUNTER_STRIDE;
            if (int rc = round(r)) return rc;
        }
        HIPCHK_AT(who, hipMemcpyAsync(host, counters, sizeof host, hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipStreamSynchronize(s));
        ++st.reads;
        for (int b = 0; b < ORDER_BATCH; ++b) {
            ++st.rounds;
            if (host[b * ORDER_COUNTER_STRIDE] == 0) return 0;
        }
    }
}

// the ordering of n points (host: hx, hy; refusals passed) on s; d_order stays on the device.  binned_from: 0, or the first
// level that uses the binned schedule whatever the rule of order_plan.hpp says.  counts: ORDER_COUNTS ints (may be null)
int order_run(const char *who, int n, const double *hx, const double *hy, const OrderBox &box, int binned_from, int *d_order,
              int *counts, hipStream_t s, OrderMarks &marks, OrderStats &st)
{
    DevBuf<double> dxy, pxy;
    DevBuf<int> orig, state, rem, rem2, olab, cellof, cnt, pos, S;
    DevBuf<unsigned> champ, counters;
    DevBuf<long long> total;
    PatternGridBufs G;
    StreamDrain drain{s, false};        // the buffers above are used on s until it is drained
    const size_t N = (size_t)n;
    HIPCHK_AT(who, dxy.alloc(2 * N));
    HIPCHK_AT(who, pxy.alloc(2 * N));
    for (DevBuf<int> *b : {&orig, &state, &rem, &rem2, &olab, &cellof}) HIPCHK_AT(who, b->alloc(N + 1));
    for (DevBuf<int> *b : {&cnt, &pos}) HIPCHK_AT(who, b->alloc(N / 256 + 2));
    HIPCHK_AT(who, counters.alloc((size_t)ORDER_BATCH * ORDER_COUNTER_STRIDE));
    HIPCHK_AT(who, total.alloc(1));
    HIPCHK_AT(who, marks.mark(PH_RELABEL));
    HIPCHK_AT(who, hipMemcpyAsync(dxy, hx, N * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK_AT(who, hipMemcpyAsync(dxy + N, hy, N * sizeof(double), hipMemcpyHostToDevice, s));
    const int first = order_first(box, n, hx, hy);
    HIPCHK_AT(who, launch_order_relabel(n, dxy, dxy + N, first, pxy, pxy + N, orig, state, rem, d_order, olab, s));
    ++st.launches;

    OrderArgs a;
    a.n = n; a.px = pxy; a.py = pxy + N; a.orig = orig; a.state = state;
    a.cellof = cellof;
    int done = 1, nrec = 1;
    if (counts) counts[1] = 1;
    const long long cap = order_dense_cap(n);
    size_t dense_cells = 0;
    bool binned = false;
    int *cur = rem, *nxt = rem2;
    for (int k = 1; k <= ORDER_LEVELS && done < n; ++k) {
        a.rem = cur; a.R = n - done; a.e = order_e(box, k);
        ++st.levels;
        PatternGrid g;
        if ((binned_from < 1 || k < binned_from) && order_dense_grid(box, k, cap, g)) {
            ++st.dense_levels;
            HIPCHK_AT(who, marks.mark(PH_DENSE));
            const size_t cells = pattern_cells(g);
            if (dense_cells == 0) {
                // once, for the largest dense grid the plan allows (the grids grow fourfold from level to level)
                PatternGrid last;
                for (int kk = k; kk <= ORDER_LEVELS && order_dense_grid(box, kk, cap, last); ++kk)
                    dense_cells = std::max(dense_cells, pattern_cells(last));
                HIPCHK_AT(who, S.alloc(dense_cells));
                HIPCHK_AT(who, champ.alloc(dense_cells));
            }
            a.g = g; a.S = S; a.champ = champ;
            HIPCHK_AT(who, hipMemsetAsync(S, 0xff, cells * sizeof(int), s));
            HIPCHK_AT(who, hipMemsetAsync(champ, 0xff, cells * sizeof(unsigned), s));
            HIPCHK_AT(who, launch_order_dense_seed(a, olab, done, s));
            ++st.launches;
            bool opening = true;
            const int rc = order_rounds(who, a, counters, s, st, [&](const OrderArgs &r) {
                if (!opening) {
                    HIPCHK_AT(who, launch_order_dense_champions(r, s));
                    HIPCHK_AT(who, launch_order_dense_take(r, s));
                    st.launches += 2;
                }
                HIPCHK_AT(who, launch_order_dense_check(r, opening, s));
                ++st.launches;
                opening = false;
                return 0;
            });
            if (rc) return rc;
        } else {
            HIPCHK_AT(who, marks.mark(PH_BINNED));
            // a grid binned for an earlier level serves (its edge exceeds this level's radius too) until a finer one is allowed
            const PatternGrid want = order_binned_grid(box, k);
            if (!binned || want.edge < 0.75 * G.t.g.edge) {
                // the buffers once, for the largest grid pattern_grid_make returns; a new binning follows the rounds of the
                // old one on the stream
                if (!binned)
                    if (int rc = pattern_grid_alloc(who, G, N, (size_t)PATTERN_CELLS_MAX)) return rc;
                if (int rc = pattern_grid_bin(who, G, want, n, pxy, pxy + N, s)) return rc;
                st.launches += 3;
                binned = true;
            }
            a.t = G.t;
            const int rc = order_rounds(who, a, counters, s, st, [&](const OrderArgs &r) {
                HIPCHK_AT(who, launch_order_binned_round(r, s));
                ++st.launches;
                return 0;
            });
            if (rc) return rc;
        }
        HIPCHK_AT(who, marks.mark(PH_EMIT));
        long long taken = 0;
        HIPCHK_AT(who, launch_order_emit(a, cnt, pos, total, done, d_order, olab, nxt, s));
        st.launches += 3;
        HIPCHK_AT(who, hipMemcpyAsync(&taken, total, sizeof taken, hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipStreamSynchronize(s));
        ++st.reads;
        if (taken < 0 || taken > (long long)a.R) return fail(-2, "%s: level %d counts %lld of %d points", who, k, taken, a.R);
        done += (int)taken;
        std::swap(cur, nxt);
        nrec = k + 1;
        if (counts) counts[1 + k] = (int)taken;
    }
    HIPCHK_AT(who, marks.mark(PH_EMIT));
    a.rem = cur; a.R = n - done;
    HIPCHK_AT(who, launch_order_rest(a, done, d_order, s));
    if (a.R > 0) ++st.launches;
    if (counts) {
        counts[1 + nrec] = a.R;
        counts[0] = nrec + 1;
    }
    HIPCHK_AT(who, marks.mark(PH_EMIT));
    HIPCHK_AT(who, hipStreamSynchronize(s));
    return 0;
}

int order_impl(const char *who, int n, const double *locs, int device, int binned_from, int *order, int *level_counts, double *ms,
               long long *stats)
{
    OrderBox box;
    if (int rc = order_refusals(who, n, locs, order || ms, box)) return rc;
    HIPCHK_AT(who, hipSetDevice(device < 0 ? 0 : device));
    DevBuf<int> dorder;
    StreamDrain s{nullptr, true};       // own non-blocking stream (the library never launches on the NULL stream)
    HIPCHK_AT(who, hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking));
    HIPCHK_AT(who, dorder.alloc((size_t)n));
    OrderMarks marks{ms != nullptr, s, {}, {}};
    OrderStats st;
    int counts[ORDER_COUNTS] = {0};
    if (int rc = order_run(who, n, locs, locs + n, box, binned_from, dorder, counts, s, marks, st)) return rc;
    if (order) {
        HIPCHK_AT(who, hipMemcpyAsync(order, dorder, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipStreamSynchronize(s));
    }
    if (level_counts) memcpy(level_counts, counts, (size_t)(counts[0] + 1) * sizeof(int));
    if (ms) {
        for (int k = 0; k < PH_COUNT; ++k) ms[k] = 0.0;
        HIPCHK_AT(who, marks.sums(ms));
    }
    if (stats) {
        stats[0] = st.levels; stats[1] = st.dense_levels; stats[2] = st.rounds; stats[3] = st.launches; stats[4] = st.reads;
    }
    return 0;
}

}  // namespace

extern "C" int cocons_vecchia_order(int n, const double *locs, int device, int *order, int *level_counts)
{
    return order_impl("cocons_vecchia_order", n, locs, device, 0, order, level_counts, nullptr, nullptr);
}

extern "C" int cocons_debug_order_phases(int n, const double *locs, int device, int binned_from, int *order, int *level_counts,
                                         double *ms4, long long *stats5)
{
    const char *who = "cocons_debug_order_phases";
    if (!ms4 || !stats5) return fail(-1, "%s: null argument", who);
    if (binned_from < 0 || binned_from > ORDER_LEVELS) return fail(-1, "%s: binned_from = %d is outside 0 .. 64", who, binned_from);
    return order_impl(who, n, locs, device, binned_from, order, level_counts, ms4, stats5);
}

extern "C" int cocons_debug_order_plan(int n, const double *locs, int *labels, double *geom3, double *levels2)
{
    const char *who = "cocons_debug_order_plan";
    if (!locs || !labels || !geom3 || !levels2) return fail(-1, "%s: null argument", who);
    if (n < 1) return fail(-1, "%s: n = %d (at least one point expected)", who, n);
    for (size_t i = 0; i < (size_t)2 * n; ++i)
        if (!std::isfinite(locs[i])) return fail(-1, "%s: a coordinate is not finite", who);
    const OrderBox box = order_box_make(n, locs, locs + n);
    if (!(box.L <= ORDER_SPAN_MAX)) return fail(-1, "%s: the points span %g, more than 2^511", who, box.L);
    const OrderLabels l = order_labels_make(n);
    for (int i = 0; i < n; ++i) labels[i] = order_label(l, i);
    geom3[0] = box.cx; geom3[1] = box.cy; geom3[2] = box.L;
    for (int k = 1; k <= ORDER_LEVELS; ++k) {
        levels2[2 * (k - 1)] = order_ell(box, k);
        levels2[2 * (k - 1) + 1] = order_e(box, k);
    }
    return 0;
}
