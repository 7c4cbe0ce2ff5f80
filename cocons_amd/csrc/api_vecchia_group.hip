// api_vecchia_group.hip -- C ABI of grouped Vecchia blocks: cocons_vecchia_group, the greedy grouping rule on
// the host; cocons_vecchia_group_table, the expanded table of any partition; cocons_vecchia_set_groups, the plan of a
// partition on a Vecchia handle whose table is closed under it; cocons_fit_create_vecchia_grouped, the three in one call; and
// cocons_neg2loglik_vecchia_grouped / cocons_vecchia_whiten_grouped, the value and the whitening with one factorisation per
// block, cocons_neg2loglik_grad_vecchia_grouped, the value and the gradient from it, and
// cocons_fisher_vecchia_grouped, the expected information from it, and cocons_vecchia_unwhiten_grouped,
// cocons_sim_vecchia_grouped, cocons_vecchia_whiten_t_grouped and cocons_cv_vecchia_grouped, U^-1, U' and
// cross-validation with their coefficients from it; and the round rule: cocons_vecchia_group_rounds on the
// host, cocons_vecchia_group_device over the launches of group.hip, cocons_fit_create_vecchia_grouped_knn -- search, rounds,
// plan and expanded table on the device -- and cocons_vecchia_groups_export, the read-back.  A grouped evaluation
// is the ungrouped one's body (the *_impl functions of api_vecchia.hip and its siblings, grouped = true) with
// launch_vecchia_group_blocks in the place of launch_vecchia_blocks: the same records, right-hand sides, per-row arrays, totals
// and status word, and therefore the same bits.
#include "fit.hpp"
#include "group_plan.hpp"
#include <climits>

namespace {

// cocons_fit_create_vecchia's table rules on the caller's layout; 0, or -1 with the message
int check_table(const char *who, int n, int m, const int *nn)
{
    if (n < 1) return fail(-1, "%s: n = %d (at least one observation expected)", who, n);
    if (m < 1 || m > VECCHIA_M_MAX) return fail(-1, "%s: m = %d is outside 1 .. %d", who, m, VECCHIA_M_MAX);
    std::vector<int> row((size_t)m);
    for (int i = 0; i < n; ++i) {
        int k = 0;
        for (int j = 0; j < m; ++j) {
            const int v = nn[(size_t)i + (size_t)j * n];
            if (v < 0 || v > i)
                return fail(-1, "%s: row %d of nn names an index outside its range (1-based indices in 1 .. row - 1, 0 = none)",
                            who, i + 1);
            if (v > 0) row[(size_t)k++] = v;
        }
        std::sort(row.begin(), row.begin() + k);
        for (int j = 1; j < k; ++j)
            if (row[(size_t)j] == row[(size_t)j - 1])
                return fail(-1, "%s: row %d of nn names an index twice (1-based indices in 1 .. row - 1, 0 = none)", who, i + 1);
    }
    return 0;
}

cocons::GroupTable caller_table(int n, int m, const int *nn)
{
    cocons::GroupTable t;
    t.p = nn; t.n = (size_t)n; t.m = m; t.device = false;
    return t;
}

// group_plan's return as a refusal
int plan_refusal(const char *who, int st, int n)
{
    if (st < 0) return fail(-1, "%s: group[%d] is outside 0 .. %d", who, -st - 1, n - 1);
    return fail(-1, "%s: the block of row %d spans more than %d rows (its members and all their neighbours)", who, st,
                cocons::GROUP_ROWS_MAX);
}

template <class T> hipError_t to_device(DevBuf<T> &d, const std::vector<T> &h, hipStream_t s)
{
    if (hipError_t e = d.reserve(std::max<size_t>(h.size(), 1), s, nullptr, -1, true)) return e;
    if (h.empty()) return hipSuccess;
    return hipMemcpyAsync(d.get(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s);
}

}  // namespace

extern "C" int cocons_vecchia_group(int n, int m, const int *nn, int max_rows, int *group, long long *out4)
{
    const char *who = "cocons_vecchia_group";
    if (!nn || !group) return fail(-1, "%s: null argument", who);
    if (int rc = check_table(who, n, m, nn)) return rc;
    if (max_rows < 2 || max_rows > cocons::GROUP_ROWS_MAX)
        return fail(-1, "%s: max_rows = %d is outside 2 .. %d", who, max_rows, cocons::GROUP_ROWS_MAX);
    const cocons::GroupTable t = caller_table(n, m, nn);
    cocons::group_greedy(t, max_rows, group);
    if (out4) {
        cocons::GroupPlan pl;
        if (int st = cocons::group_plan(t, group, pl)) return plan_refusal(who, st, n);
        out4[0] = pl.blocks; out4[1] = pl.sum_rows; out4[2] = pl.pairs; out4[3] = cocons::group_pairs_ungrouped(t);
    }
    return 0;
}

namespace {

// the refusals the two entries of the round rule share, before any device work; 0, or -1 with the message
int check_rounds(const char *who, int n, int m, const int *nn, int max_rows, int max_rounds, const int *group, bool labels = true)
{
    if (!nn || (labels && !group)) return fail(-1, "%s: null argument", who);      // (labels = false: the caller wants none)
    if (int rc = check_table(who, n, m, nn)) return rc;
    if (max_rows < 2 || max_rows > cocons::GROUP_ROWS_MAX)
        return fail(-1, "%s: max_rows = %d is outside 2 .. %d", who, max_rows, cocons::GROUP_ROWS_MAX);
    if (max_rounds < 0) return fail(-1, "%s: max_rounds = %d (0 = %d rounds at the most)", who, max_rounds, cocons::GROUP_ROUNDS_MAX);
    return 0;
}

// out5 of the labels the rule made; the labels themselves go to the caller only with it
int rounds_out(const char *who, int n, int m, const int *nn, const std::vector<int> &lab, int rounds, int *group, long long *out5)
{
    if (out5) {
        const cocons::GroupTable t = caller_table(n, m, nn);
        cocons::GroupPlan pl;
        if (int st = cocons::group_plan(t, lab.data(), pl)) return plan_refusal(who, st, n);
        out5[0] = pl.blocks; out5[1] = pl.sum_rows; out5[2] = pl.pairs; out5[3] = cocons::group_pairs_ungrouped(t);
        out5[4] = rounds;
    }
    std::copy(lab.begin(), lab.end(), group);
    return 0;
}

// The round rule's state on the device: memory of the call that runs the rounds.  n (4 max_rows + 36) bytes.
struct GroupRoundState {
    DevBuf<int> blk, sz, slot, prop, live[2];
    DevBuf<unsigned long long> key, best;
    DevBuf<int> ctr;                   // {somebody proposed, the blocks alive after the round}
    int nlive = 0, cur = 0;
};

// The rounds over the device table d_tab (n x m, the layout of VecchiaState::nbr) on s; the state stays in R, *rounds: the
// rounds that merged something.  The one host traffic of a round is R.ctr, which plans the next round's launches.
// trace (may be null; cocons_debug_group_rounds): per round launched, the blocks alive at its start and its device time by
// events on s -- no event is made without it.
struct GroupTrace {
    int cap = 0, count = 0;
    int *live = nullptr;
    double *ms = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~GroupTrace()
    {
        if (e0) hipEventDestroy(e0);
        if (e1) hipEventDestroy(e1);
    }
};

int group_rounds_device(const char *who, int n, int m, const int *d_tab, int max_rows, int max_rounds, GroupRoundState &R,
                        hipStream_t s, int *rounds, GroupTrace *trace = nullptr)
{
    if (trace) {
        HIPCHK_AT(who, hipEventCreate(&trace->e0));
        HIPCHK_AT(who, hipEventCreate(&trace->e1));
    }
    const size_t N = (size_t)n;
    HIPCHK_AT(who, R.blk.alloc(N));
    HIPCHK_AT(who, R.sz.alloc(N));
    HIPCHK_AT(who, R.slot.alloc(N * (size_t)max_rows));
    HIPCHK_AT(who, R.prop.alloc(N));
    HIPCHK_AT(who, R.live[0].alloc(N));
    HIPCHK_AT(who, R.live[1].alloc(N));
    HIPCHK_AT(who, R.key.alloc(N));
    HIPCHK_AT(who, R.best.alloc(N));
    HIPCHK_AT(who, R.ctr.alloc(2));
    GroupArgs a;
    a.n = n; a.m = m; a.max_rows = max_rows; a.tab = d_tab;
    a.blk = R.blk; a.sz = R.sz; a.slot = R.slot; a.prop = R.prop; a.key = R.key; a.best = R.best;
    a.any = R.ctr; a.count = R.ctr + 1;
    a.next = R.live[0];
    HIPCHK_AT(who, launch_group_init(a, s));
    R.nlive = n; R.cur = 0;
    const int cap = max_rounds > 0 ? max_rounds : cocons::GROUP_ROUNDS_MAX;
    *rounds = 0;
    while (*rounds < cap) {
        a.live = R.live[R.cur]; a.nlive = R.nlive; a.next = R.live[R.cur ^ 1];
        HIPCHK_AT(who, hipMemsetAsync(R.ctr, 0, 2 * sizeof(int), s));
        if (trace) HIPCHK_AT(who, hipEventRecord(trace->e0, s));
        HIPCHK_AT(who, launch_group_propose(a, s));
        HIPCHK_AT(who, launch_group_merge(a, s));
        HIPCHK_AT(who, launch_group_compact(a, s));
        if (trace) HIPCHK_AT(who, hipEventRecord(trace->e1, s));
        int h[2] = {0, 0};
        HIPCHK_AT(who, hipMemcpyAsync(h, R.ctr, sizeof h, hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipStreamSynchronize(s));
        if (trace && trace->count < trace->cap) {
            float ms = 0.0f;
            HIPCHK_AT(who, hipEventElapsedTime(&ms, trace->e0, trace->e1));
            trace->live[trace->count] = R.nlive;
            trace->ms[trace->count++] = ms;
        }
        if (!h[0]) break;                        // nobody proposed: nothing was merged, and the list is as it was
        if (h[1] < 1 || h[1] >= R.nlive) return fail(-1, "%s: a round left %d of %d blocks (internal error)", who, h[1], R.nlive);
        R.nlive = h[1]; R.cur ^= 1;
        ++*rounds;
    }
    return 0;
}

}  // namespace

extern "C" int cocons_vecchia_group_rounds(int n, int m, const int *nn, int max_rows, int max_rounds, int *group, long long *out5)
{
    const char *who = "cocons_vecchia_group_rounds";
    if (int rc = check_rounds(who, n, m, nn, max_rows, max_rounds, group)) return rc;
    std::vector<int> lab((size_t)n);
    int rounds = 0;
    cocons::group_rounds(caller_table(n, m, nn), max_rows, max_rounds, lab.data(), &rounds);
    return rounds_out(who, n, m, nn, lab, rounds, group, out5);
}

// cocons_vecchia_group_device under the name of the entry that asks; trace: the labels stay on the device (group is not read)
static int group_device_impl(const char *who, int n, int m, const int *nn, int max_rows, int max_rounds, int device, int *group,
                             long long *out5, GroupTrace *trace)
{
    if (int rc = check_rounds(who, n, m, nn, max_rows, max_rounds, group, trace == nullptr)) return rc;
    // the table in the device layout: 0-based, ascending, -1 behind the last
    std::vector<int> tab((size_t)n * m);
    for (int i = 0; i < n; ++i) {
        int *row = &tab[(size_t)i * m], k = 0;
        for (int j = 0; j < m; ++j) {
            const int v = nn[(size_t)i + (size_t)j * n];
            if (v > 0) row[k++] = v - 1;
        }
        std::sort(row, row + k);
        std::fill(row + k, row + m, -1);
    }
    if (hipError_t e = hipSetDevice(device < 0 ? 0 : device)) {
        (void)hipGetLastError();                 // (the refusal is this call's alone: the next launch must not find it)
        return fail(-100 - (int)e, "%s: %s", who, hipGetErrorString(e));
    }
    std::vector<int> blk((size_t)n);
    int rounds = 0;
    {
        DevBuf<int> dtab;
        GroupRoundState R;
        StreamDrain s{nullptr, true};
        HIPCHK_AT(who, hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking));
        HIPCHK_AT(who, dtab.alloc(tab.size()));
        HIPCHK_AT(who, hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, s));
        if (int rc = group_rounds_device(who, n, m, dtab, max_rows, max_rounds, R, s, &rounds, trace)) return rc;
        if (trace) return trace->count;
        HIPCHK_AT(who, hipMemcpyAsync(blk.data(), R.blk, blk.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipStreamSynchronize(s));
    }
    // the blocks numbered by their smallest member, on the host: one pass over the n ids that came home
    std::vector<int> id((size_t)n, -1), lab((size_t)n);
    int next = 0;
    for (int i = 0; i < n; ++i) {
        if (blk[(size_t)i] < 0 || blk[(size_t)i] > i) return fail(-1, "%s: row %d came home in block %d (internal error)", who, i + 1, blk[(size_t)i]);
        int &l = id[(size_t)blk[(size_t)i]];
        if (l < 0) l = next++;
        lab[(size_t)i] = l;
    }
    return rounds_out(who, n, m, nn, lab, rounds, group, out5);
}

extern "C" int cocons_vecchia_group_device(int n, int m, const int *nn, int max_rows, int max_rounds, int device, int *group,
                                           long long *out5)
{
    return group_device_impl("cocons_vecchia_group_device", n, m, nn, max_rows, max_rounds, device, group, out5, nullptr);
}

extern "C" int cocons_debug_group_rounds(int n, int m, const int *nn, int max_rows, int max_rounds, int device, int cap, int *live,
                                         double *ms)
{
    const char *who = "cocons_debug_group_rounds";
    if (!live || !ms || cap < 1) return fail(-1, "%s: bad argument", who);
    GroupTrace tr;
    tr.cap = cap; tr.live = live; tr.ms = ms;
    return group_device_impl(who, n, m, nn, max_rows, max_rounds, device, nullptr, nullptr, &tr);
}

extern "C" int cocons_vecchia_group_table(int n, int m, const int *nn, const int *group, int m_out, int *nn_out)
{
    const char *who = "cocons_vecchia_group_table";
    if (!nn || !group || (!nn_out && m_out != 0)) return fail(-1, "%s: null argument", who);
    if (int rc = check_table(who, n, m, nn)) return rc;
    cocons::GroupPlan pl;
    if (int st = cocons::group_plan(caller_table(n, m, nn), group, pl)) return plan_refusal(who, st, n);
    if (!nn_out) return pl.longest;
    if (m_out < 1 || m_out > VECCHIA_M_MAX) return fail(-1, "%s: m_out = %d is outside 1 .. %d", who, m_out, VECCHIA_M_MAX);
    if (m_out < pl.longest)
        return fail(-1, "%s: m_out = %d is smaller than the longest expanded row (%d neighbours)", who, m_out, pl.longest);
    cocons::group_table(pl, (size_t)n, m_out, nn_out);
    return 0;
}

extern "C" int cocons_vecchia_set_groups(cocons_fit *f, const int *group)
{
    const char *who = "cocons_vecchia_set_groups";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!group) return fail(-1, "%s: null argument", who);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    VecchiaState *V = f->vecchia.get();
    const int n = f->n, m = V->m;
    // the handle's table home, once: the check runs on the host, and a table that was searched on the device has no copy there
    std::vector<int> tab((size_t)n * m);
    HIPCHK_AT(who, hipMemcpyAsync(tab.data(), V->nbr, tab.size() * sizeof(int), hipMemcpyDeviceToHost, f->stream));
    HIPCHK_AT(who, hipStreamSynchronize(f->stream));
    cocons::GroupTable t;
    t.p = tab.data(); t.n = (size_t)n; t.m = m; t.device = true;
    cocons::GroupPlan pl;
    if (int st = cocons::group_plan(t, group, pl)) return plan_refusal(who, st, n);
    int have = 0, need = 0;
    if (int row = cocons::group_closed(t, pl, &have, &need))
        return fail(-1, "%s: row %d of the handle's table holds %d neighbours, its block needs the %d rows in front of it (the "
                        "table is not closed under these groups; cocons_vecchia_group_table makes one that is)",
                    who, row, have, need);
    std::unique_ptr<VecchiaGroupState> G(new VecchiaGroupState());
    G->blocks = pl.blocks; G->maxrows = pl.maxrows; G->sum_rows = pl.sum_rows; G->pairs = pl.pairs;
    const char *env = getenv("COCONS_VECCHIA_GROUP_ORDER");
    G->by_size = !(env && env[0] == '0' && !env[1]);
    hipStream_t s = f->stream;
    HIPCHK_AT(who, to_device(G->off, pl.off, s));
    HIPCHK_AT(who, to_device(G->rows, pl.rows, s));
    HIPCHK_AT(who, to_device(G->order, pl.order, s));
    HIPCHK_AT(who, to_device(G->mask, pl.mask, s));
    HIPCHK_AT(who, hipStreamSynchronize(s));           // (the plan's host vectors end with this call)
    V->grp = std::move(G);                             // a former plan is freed here: the stream is drained
    return 0;
}

extern "C" int cocons_vecchia_groups_info(cocons_fit *f, long long *out5)
{
    const char *who = "cocons_vecchia_groups_info";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!out5) return fail(-1, "%s: null argument", who);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (int rc = vecchia_need_plan(f, who)) return rc;
    const VecchiaGroupState *G = f->vecchia->grp.get();
    out5[0] = G->blocks; out5[1] = G->maxrows; out5[2] = G->sum_rows; out5[3] = G->pairs; out5[4] = G->bytes();
    return 0;
}

extern "C" cocons_fit *cocons_fit_create_vecchia_grouped(int n, int p, int r, const double *locs, const double *X, const double *z,
                                                         const double *smooth_limits, int device, int m, const int *nn,
                                                         int max_rows)
{
    const char *who = "cocons_fit_create_vecchia_grouped";
    if (!locs || !X || !z || !smooth_limits || !nn) { fail(-1, "%s: null argument", who); return nullptr; }
    if (check_table(who, n, m, nn)) return nullptr;
    if (max_rows < 2 || max_rows > cocons::GROUP_ROWS_MAX) {
        fail(-1, "%s: max_rows = %d is outside 2 .. %d", who, max_rows, cocons::GROUP_ROWS_MAX);
        return nullptr;
    }
    const cocons::GroupTable t = caller_table(n, m, nn);
    std::vector<int> group((size_t)n);
    cocons::group_greedy(t, max_rows, group.data());
    cocons::GroupPlan pl;
    if (int st = cocons::group_plan(t, group.data(), pl)) { plan_refusal(who, st, n); return nullptr; }
    const int m_out = std::max(pl.longest, 1);
    std::vector<int> wide((size_t)n * m_out);
    cocons::group_table(pl, (size_t)n, m_out, wide.data());
    cocons_fit *f = vecchia_create_impl(who, n, p, r, locs, X, z, smooth_limits, device, m_out, wide.data(), false);
    if (!f) return nullptr;
    if (cocons_vecchia_set_groups(f, group.data())) {
        cocons_fit_destroy(f);
        return nullptr;
    }
    return f;
}

namespace {

// search -> rounds -> plan -> expanded table on the handle's stream: what cocons_vecchia_neighbours,
// cocons_vecchia_group_rounds, cocons_vecchia_group_table and cocons_vecchia_set_groups leave on a handle, made where it is
// used.  Home come the counters of the rounds and the 65 counts of blocks by size -- never a table or a label.  The closure
// check of cocons_vecchia_set_groups needs no rerun: the table is written from the plan's own rows.
// The table step is a parameter (GroupedTableStep): the Euclidean search here, the correlation table in api_knn_corr.hip.
struct GroupedKnnSource : VecchiaTableSource {
    int m = 0, max_rows = 0, max_rounds = 0;
    GroupedTableStep *step = nullptr;
    int make(const char *who, cocons_fit *f, const double *locs) override
    {
        VecchiaState *V = f->vecchia.get();
        const int n = f->n;
        hipStream_t s = f->stream;
        DevBuf<int> tab, num, ids, hist;
        GroupRoundState R;
        std::unique_ptr<VecchiaGroupState> G(new VecchiaGroupState());
        StreamDrain drain{s, false};
        HIPCHK_AT(who, tab.alloc((size_t)n * m));
        if (int rc = step->table(who, f, locs, m, tab)) return rc;
        int rounds = 0;
        if (int rc = group_rounds_device(who, n, m, tab, max_rows, max_rounds, R, s, &rounds)) return rc;
        const int blocks = R.nlive, H = cocons::GROUP_ROWS_MAX + 1;
        GroupPlanArgs a;
        a.n = n; a.m = m; a.max_rows = max_rows; a.blocks = blocks;
        a.tab = tab; a.blk = R.blk; a.sz = R.sz; a.slot = R.slot;
        HIPCHK_AT(who, num.alloc((size_t)n + 1));
        HIPCHK_AT(who, ids.alloc((size_t)blocks));
        HIPCHK_AT(who, hist.alloc((size_t)H));
        HIPCHK_AT(who, G->off.alloc((size_t)blocks + 1));
        a.flag = R.prop; a.num = num; a.ids = ids; a.off = G->off; a.hist = hist;      // (prop: the rounds are over)
        HIPCHK_AT(who, hipMemsetAsync(hist, 0, (size_t)H * sizeof(int), s));
        HIPCHK_AT(who, launch_group_plan_flags(a, s));
        HIPCHK_AT(who, launch_scan_exclusive(a.flag, num, n, 0, nullptr, s));
        HIPCHK_AT(who, launch_group_plan_sizes(a, s));
        HIPCHK_AT(who, launch_scan_exclusive(G->off, G->off, blocks, 0, nullptr, s));
        int h[cocons::GROUP_ROWS_MAX + 1];
        HIPCHK_AT(who, hipMemcpyAsync(h, hist, sizeof h, hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipStreamSynchronize(s));
        long long count = 0;
        for (int k = cocons::GROUP_ROWS_MAX; k >= 1; --k) {          // largest first
            a.start[cocons::GROUP_ROWS_MAX - k] = (int)count;
            count += h[k];
            if (h[k]) {
                G->maxrows = std::max(G->maxrows, k);
                G->sum_rows += (long long)h[k] * k;
                G->pairs += (long long)h[k] * k * (k - 1) / 2;
            }
        }
        a.start[cocons::GROUP_ROWS_MAX] = (int)count;
        if (h[0] || count != blocks) return fail(-1, "%s: %lld blocks by size, %d by the rounds (internal error)", who, count, blocks);
        if (G->sum_rows > INT_MAX) return fail(-1, "%s: the blocks hold %lld rows, more than an offset can count", who, G->sum_rows);
        G->blocks = blocks;
        const char *env = getenv("COCONS_VECCHIA_GROUP_ORDER");
        G->by_size = !(env && env[0] == '0' && !env[1]);
        // the last row of a block is a member, so the longest expanded row belongs to the largest block
        a.m_out = std::max(G->maxrows - 1, 1);
        HIPCHK_AT(who, G->rows.alloc((size_t)G->sum_rows));
        HIPCHK_AT(who, G->order.alloc((size_t)blocks));
        HIPCHK_AT(who, G->mask.alloc((size_t)blocks));
        HIPCHK_AT(who, V->nbr.alloc((size_t)n * a.m_out));
        a.rows = G->rows; a.order = G->order; a.mask = G->mask; a.nbr = V->nbr;
        HIPCHK_AT(who, launch_group_plan_fill(a, s));
        HIPCHK_AT(who, launch_group_plan_order(a, s));
        HIPCHK_AT(who, hipStreamSynchronize(s));
        V->m = a.m_out;
        V->grp = std::move(G);
        return 0;
    }
};

struct EuclideanTableStep : GroupedTableStep {
    int table(const char *who, cocons_fit *f, const double *locs, int m, int *d_tab) override
    {
        const int n = f->n;
        return knn_self_search(who, n, locs, locs + n, f->dlocs, f->dlocs + n, m, nullptr, d_tab, f->stream);
    }
};

}  // namespace

cocons_fit *vecchia_create_grouped_device(const char *who, int n, int p, int r, const double *locs, const double *X,
                                          const double *z, const double *smooth_limits, int device, int m, int max_rows,
                                          int max_rounds, GroupedTableStep &step)
{
    if (max_rows < 2 || max_rows > cocons::GROUP_ROWS_MAX) {
        fail(-1, "%s: max_rows = %d is outside 2 .. %d", who, max_rows, cocons::GROUP_ROWS_MAX);
        return nullptr;
    }
    if (max_rounds < 0) {
        fail(-1, "%s: max_rounds = %d (0 = %d rounds at the most)", who, max_rounds, cocons::GROUP_ROUNDS_MAX);
        return nullptr;
    }
    GroupedKnnSource src;
    src.m = m; src.max_rows = max_rows; src.max_rounds = max_rounds; src.step = &step;
    cocons_fit *f = vecchia_create_impl(who, n, p, r, locs, X, z, smooth_limits, device, m, nullptr, true, &src);
    if (!f) (void)hipGetLastError();             // (a refused device is this call's alone: the next launch must not find it)
    return f;
}

extern "C" cocons_fit *cocons_fit_create_vecchia_grouped_knn(int n, int p, int r, const double *locs, const double *X,
                                                             const double *z, const double *smooth_limits, int device, int m,
                                                             int max_rows, int max_rounds)
{
    EuclideanTableStep step;
    return vecchia_create_grouped_device("cocons_fit_create_vecchia_grouped_knn", n, p, r, locs, X, z, smooth_limits, device, m,
                                         max_rows, max_rounds, step);
}

extern "C" int cocons_vecchia_groups_export(cocons_fit *f, int *block, int *nn)
{
    const char *who = "cocons_vecchia_groups_export";
    if (!f) return fail(-1, "%s: null fit handle", who);
    if (!block) return fail(-1, "%s: null argument", who);
    FIT_ENTER_ANY(f);
    if (int rc = vecchia_only(f, who)) return rc;
    if (int rc = vecchia_need_plan(f, who)) return rc;
    VecchiaState *V = f->vecchia.get();
    const VecchiaGroupState *G = V->grp.get();
    const size_t n = (size_t)f->n, m = (size_t)V->m;
    std::vector<int> off((size_t)G->blocks + 1), rows((size_t)G->sum_rows), tab(nn ? n * m : 0);
    std::vector<unsigned long long> mask((size_t)G->blocks);
    hipStream_t s = f->stream;
    HIPCHK_AT(who, hipMemcpyAsync(off.data(), G->off, off.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipMemcpyAsync(rows.data(), G->rows, rows.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipMemcpyAsync(mask.data(), G->mask, mask.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (nn) HIPCHK_AT(who, hipMemcpyAsync(tab.data(), V->nbr, tab.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipStreamSynchronize(s));
    // (into staging first: the caller's arrays stay untouched when the plan on the device is not one)
    std::vector<int> lab(n, -1);
    for (int b = 0; b < G->blocks; ++b)
        for (int e = off[(size_t)b]; e < off[(size_t)b + 1]; ++e)
            if (mask[(size_t)b] >> (e - off[(size_t)b]) & 1) {
                const int i = rows[(size_t)e];
                if (i < 0 || (size_t)i >= n || lab[(size_t)i] >= 0) return fail(-1, "%s: the plan names row %d twice or not at all (internal error)", who, i + 1);
                lab[(size_t)i] = b;
            }
    for (size_t i = 0; i < n; ++i)
        if (lab[i] < 0) return fail(-1, "%s: the plan names row %d twice or not at all (internal error)", who, (int)i + 1);
    std::copy(lab.begin(), lab.end(), block);
    if (nn)
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0; j < m; ++j) nn[i + j * n] = tab[i * m + j] + 1;          // -1 = none becomes 0
    return 0;
}

extern "C" int cocons_neg2loglik_vecchia_grouped(cocons_fit *f, const double *theta, const double *mean, double *value,
                                                 double *parts)
{
    return vecchia_value_impl("cocons_neg2loglik_vecchia_grouped", true, f, theta, mean, value, parts);
}

extern "C" int cocons_vecchia_whiten_grouped(cocons_fit *f, const double *theta, int c, const double *B, double *out, double *logd)
{
    return vecchia_whiten_impl("cocons_vecchia_whiten_grouped", true, f, theta, c, B, out, logd);
}

extern "C" int cocons_neg2loglik_grad_vecchia_grouped(cocons_fit *f, const double *theta, const double *mean, int c,
                                                      const double *B, double *sum_logliks, double *parts, double *grad_theta,
                                                      double *grad_quad, double *grad_mean)
{
    return vecchia_grad_impl("cocons_neg2loglik_grad_vecchia_grouped", true, f, theta, mean, c, B, sum_logliks, parts,
                             grad_theta, grad_quad, grad_mean);
}

extern "C" int cocons_fisher_vecchia_grouped(cocons_fit *f, const double *theta, int ndir, const double *dirs, double *info,
                                             double *info_mean)
{
    return vecchia_fisher_impl("cocons_fisher_vecchia_grouped", true, f, theta, ndir, dirs, info, info_mean);
}

// the ungrouped entries' bodies with launch_vecchia_group_coefs in the place of launch_vecchia_coefs
extern "C" int cocons_vecchia_unwhiten_grouped(cocons_fit *f, const double *theta, int c, const double *W, double *out)
{
    return vecchia_unwhiten_impl("cocons_vecchia_unwhiten_grouped", true, false, f, theta, c, W, out, nullptr);
}

extern "C" int cocons_debug_vecchia_sim_phases_grouped(cocons_fit *f, const double *theta, int c, const double *W, double *out,
                                                       double *ms3)
{
    return vecchia_unwhiten_impl("cocons_debug_vecchia_sim_phases_grouped", true, true, f, theta, c, W, out, ms3);
}

extern "C" int cocons_sim_vecchia_grouped(cocons_fit *f, const double *theta, const double *mean, int n_fixed, int z_col, int nsim,
                                          const double *iiderrors, double *out)
{
    return vecchia_sim_impl("cocons_sim_vecchia_grouped", true, f, theta, mean, n_fixed, z_col, nsim, iiderrors, out);
}

extern "C" int cocons_vecchia_whiten_t_grouped(cocons_fit *f, const double *theta, int c, const double *W, double *out,
                                               double *qdiag)
{
    return vecchia_whiten_t_impl("cocons_vecchia_whiten_t_grouped", true, f, theta, c, W, out, qdiag);
}

extern "C" int cocons_cv_vecchia_grouped(cocons_fit *f, const double *theta, const double *mean, int nfold, const int *fold,
                                         double *resid, double *var, long long *stats4)
{
    return vecchia_cv_impl("cocons_cv_vecchia_grouped", true, f, theta, mean, nfold, fold, resid, var, stats4);
}
