// api_handle.hip -- C ABI, the handle's life and the placement of its streams: the registry of live handles, creation (dense
// and taper), destruction, the stream accessors, and the self-tests that keep a handle's engine stream and a batch slot's main
// stream on hardware queues of their own (engine_warm, slot_stream_apart).  All of it runs once per handle or per batch slot,
// never inside an evaluation (api.hip).
#include "fit.hpp"

// ---------------------------------------------------------------------------
// Every live handle of the process: engine_warm tests a new handle's streams against the streams of the others (a resident
// engine of one handle must not share a hardware queue with the main stream of another: the batch slots and callers with
// several handles in flight run exactly that combination).
static std::mutex g_reg_mutex;
static std::vector<cocons_fit *> g_registry;
static void registry_add(cocons_fit *f) { std::lock_guard<std::mutex> lk(g_reg_mutex); g_registry.push_back(f); }
static void registry_remove(cocons_fit *f)
{
    std::lock_guard<std::mutex> lk(g_reg_mutex);
    g_registry.erase(std::remove(g_registry.begin(), g_registry.end(), f), g_registry.end());
}

extern "C" int cocons_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { g_err = hipGetErrorString(e); return -1; }
    return n;
}

extern "C" void cocons_fit_destroy(cocons_fit *f)
{
    if (!f) return;
    // out of the registry first (no stream self-test of another thread can find the handle any more), then wait for one that
    // found it earlier and is still launching probe kernels on its streams (engine_warm holds op_mu for that long)
    registry_remove(f);
    f->op_mu.lock(); f->op_mu.unlock();
    // Only the process that created the handle touches the device.  A forked child makes NO HIP call here, on a runtime it
    // does not own: streams, events, the pinned mirror and the clones are left alone, and `delete f` below gives back host
    // memory only -- a DevBuf abandons memory that another process allocated instead of freeing it.
    hipStream_t last[2] = {nullptr, nullptr};
    if (f->pid == getpid()) {
        hipSetDevice(f->device);
        if (f->stream) hipStreamSynchronize(f->stream);
        if (f->stream2) hipStreamSynchronize(f->stream2);
        hipHostFree(f->hinfo);                                  // (hout, hinfo_init: the same allocation)
        for (auto &e : f->ev) if (e) hipEventDestroy(e);
        if (f->ev_eng) hipEventDestroy(f->ev_eng);
        if (f->cstream_l && f->cstream_l != f->cstream) { hipStreamSynchronize(f->cstream_l); hipStreamDestroy(f->cstream_l); }
        if (f->cstream) { hipStreamSynchronize(f->cstream); hipStreamDestroy(f->cstream); }
        shard_events_destroy(f->shard.get());
        if (f->comm_l && f->comm_l_own) rccl_comm_destroy(f->comm_l);
        if (f->comm && f->comm_own) rccl_comm_destroy(f->comm);
        for (auto c : f->slots) cocons_fit_destroy(c);
        if (f->unsorted) cocons_fit_destroy(f->unsorted);
        if (f->taper_twin) cocons_fit_destroy(f->taper_twin);
        last[0] = f->stream2;
        if (f->own_stream) last[1] = f->stream;
    }
    // Every device buffer goes HERE -- the DevBuf members of the handle and of its krige, gradient and shard states --: after
    // every stream that used them was drained (above), before the engine's and the own main stream are destroyed (below, last).
    delete f;
    for (hipStream_t s : last) if (s) hipStreamDestroy(s);
}

static int engine_warm(cocons_fit *f);

cocons_fit *fit_create_impl(int n, int p, int r, int q, const double *locs,
                            const double *X, const double *z, const double *x_betas,
                            const double *smooth_limits, int device, bool allow_sort, bool defer_matrix,
                            bool want_engine, bool return_locked)
{
    if (n <= 0 || p <= 0 || p > COCONS_P_MAX || r < 0 || q < 0 || !locs || !X || !smooth_limits ||
        (r > 0 && !z) || (q > 0 && !x_betas)) {
        fail(-1, "cocons_fit_create: bad argument");
        return nullptr;
    }
    cocons_fit *f = new cocons_fit();
    f->n = n; f->p = p; f->r = r; f->q = q;
    f->device = device < 0 ? 0 : device;
    f->pid = getpid();
    f->npad = round_up(n, TILE);
    f->nt = f->npad / TILE;
    f->smooth_limits[0] = smooth_limits[0];
    f->smooth_limits[1] = smooth_limits[1];
#define CK(expr)                                                                  \
    do {                                                                          \
        hipError_t e__ = (expr);                                                  \
        if (e__ != hipSuccess) {                                                  \
            fail(-100, "cocons_fit_create: %s", hipGetErrorString(e__));          \
            cocons_fit_destroy(f);                                                \
            return nullptr;                                                       \
        }                                                                         \
    } while (0)
    CK(hipSetDevice(f->device));
    // every stream the library creates is non-blocking: nothing here ever joins the NULL stream
    CK(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    f->own_stream = true;
    // Spatial (Morton / Z-order) permutation of the observations.  -2 loglik, the kriging outputs and
    // the simulated fields do not depend on the order of the observed locations (a symmetric
    // permutation of Sigma), but the Bessel kernels run faster when neighbouring indices are
    // neighbouring points (8 x 8 pair patches then see similar distances).  Everything the handle
    // keeps -- locs, X, z, x_betas, host copies -- is stored in the permuted order.
    std::vector<int> perm(n);
    for (int i = 0; i < n; ++i) perm[i] = i;
    {
        const char *e = getenv("COCONS_SPATIAL_SORT");
        if (allow_sort && (e ? atoi(e) : 1) && n > 64) {
            double lo[2] = {locs[0], locs[n]}, hi[2] = {locs[0], locs[n]};
            for (int i = 0; i < n; ++i)
                for (int d = 0; d < 2; ++d) {
                    double v = locs[i + (size_t)d * n];
                    if (v < lo[d]) lo[d] = v;
                    if (v > hi[d]) hi[d] = v;
                }
            std::vector<unsigned long long> key(n);
            bool finite = true;
            for (int i = 0; i < n && finite; ++i) {
                unsigned q[2];
                for (int d = 0; d < 2; ++d) {
                    double span = hi[d] - lo[d];
                    double t = span > 0 ? (locs[i + (size_t)d * n] - lo[d]) / span : 0.0;
                    if (!(t >= 0.0 && t <= 1.0)) { finite = false; t = 0; }
                    q[d] = (unsigned)(t * 65535.0);
                }
                unsigned long long k = 0;
                for (int b = 0; b < 16; ++b)
                    k |= ((unsigned long long)((q[0] >> b) & 1u) << (2 * b)) | ((unsigned long long)((q[1] >> b) & 1u) << (2 * b + 1));
                key[i] = (k << 32) | (unsigned)i;          // ties keep the input order
            }
            if (finite) {
                std::sort(key.begin(), key.end());
                // keep the caller's order when it is already as coherent as the Morton order (e.g. a
                // regular grid listed row by row): compare the path lengths through the points
                auto path = [&](auto idx) {
                    double s = 0;
                    for (int i = 0; i + 1 < n; ++i) {
                        int a = idx(i), b = idx(i + 1);
                        double dx = locs[a] - locs[b], dy = locs[a + (size_t)n] - locs[b + (size_t)n];
                        s += std::sqrt(dx * dx + dy * dy);
                    }
                    return s;
                };
                double p_in = path([&](int i) { return i; });
                double p_mo = path([&](int i) { return (int)(key[i] & 0xffffffffu); });
                if (p_mo < 0.8 * p_in)
                    for (int i = 0; i < n; ++i) perm[i] = (int)(key[i] & 0xffffffffu);
            }
        }
    }
    f->h_locs.assign(locs, locs + (size_t)2 * n);      // host copies: ORIGINAL order
    f->h_X.assign(X, X + (size_t)n * p);
    if (r > 0) f->h_z.assign(z, z + (size_t)n * r);
    if (q > 0) f->h_xb.assign(x_betas, x_betas + (size_t)n * q);
    for (int i = 0; i < n; ++i)
        if (perm[i] != i) { f->sorted = true; break; }
    // Identity padding in FRONT (handles whose internal order is theirs to choose, i.e. allow_sort): pad0 placeholder
    // observations (copies of the first one; their rows and columns are overwritten by unit vectors before every
    // factorisation) precede the caller's, so that the internal problem has exactly npad = n observations and no padding
    // rides through every trailing update.  Order-dependent entry points then go through the unsorted twin, like after a
    // Morton sort.  COCONS_FRONT_PAD=0: padding behind the observations (rounds 1-2).
    f->n_user = n;
    {
        const char *e = getenv("COCONS_FRONT_PAD");
        f->pad0 = (allow_sort && (e ? atoi(e) : 1)) ? f->npad - n : 0;
        // ... except for a few SLOTS kept behind the observations: rows that carry the right-hand sides of an evaluation
        // through the factorisation as part of the matrix's last tile, instead of a tile row of their own under it (one
        // row in use of 64: 1.9 % of the trailing updates' arithmetic at n = 10 000).  COCONS_RHS_SLOTS=0: off.
        const char *e2 = getenv("COCONS_RHS_SLOTS");
        const int need = round_up(r + (q > p ? q : p) > 0 ? r + (q > p ? q : p) : 1, 16);
        f->nslot = (f->pad0 >= need && r > 0 && (e2 ? atoi(e2) : 1)) ? need : 0;
        f->pad0 -= f->nslot;
    }
    const int pad0 = f->pad0, nint = n + pad0;
    if (pad0 > 0) f->sorted = true;
    f->obs_pos.resize(n);
    for (int i = 0; i < n; ++i) f->obs_pos[perm[i]] = pad0 + i;
    auto permute_pad = [&](const double *src, int ncol, bool zero_pad) {
        std::vector<double> out((size_t)nint * ncol);
        for (int c = 0; c < ncol; ++c) {
            // (canon_nan: no all-ones NaN enters the device -- the mailboxes' "not written yet" pattern, see there)
            for (int i = 0; i < pad0; ++i) out[(size_t)i + (size_t)c * nint] = zero_pad ? 0.0 : canon_nan(src[(size_t)perm[0] + (size_t)c * n]);
            for (int i = 0; i < n; ++i) out[(size_t)(pad0 + i) + (size_t)c * nint] = canon_nan(src[(size_t)perm[i] + (size_t)c * n]);
        }
        return out;
    };
    std::vector<double> plocs = permute_pad(locs, 2, false), pX = permute_pad(X, p, false), pz, pxb;
    if (r > 0) pz = permute_pad(z, r, true);
    if (q > 0) pxb = permute_pad(x_betas, q, true);
    locs = plocs.data(); X = pX.data();
    if (r > 0) z = pz.data();
    if (q > 0) x_betas = pxb.data();
    n = nint;                     // from here on: the internal problem
    f->n = n;
    CK(f->dX.alloc((size_t)n * p));
    CK(f->dlocs.alloc((size_t)n * 2));
    CK(hipMemcpyAsync(f->dX, X, (size_t)n * p * sizeof(double), hipMemcpyHostToDevice, f->stream));
    CK(hipMemcpyAsync(f->dlocs, locs, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice, f->stream));
    if (r > 0) {
        CK(f->dz.alloc((size_t)n * r));
        CK(hipMemcpyAsync(f->dz, z, (size_t)n * r * sizeof(double), hipMemcpyHostToDevice, f->stream));
    }
    if (q > 0) {
        CK(f->dxb.alloc((size_t)n * q));
        CK(hipMemcpyAsync(f->dxb, x_betas, (size_t)n * q * sizeof(double), hipMemcpyHostToDevice, f->stream));
    }
    CK(hipStreamSynchronize(f->stream));      // the staging vectors above go out of scope
    CK(f->dloc.alloc((size_t)LOCP_FIELDS * f->npad));
    CK(f->dinv.alloc(2 * 8 * 256));
    // the two info words -- [0] failing minor (atomicMin), [1] abort word of the engine hand-offs -- sit in the 8 bytes in
    // front of the reduction outputs, on the device and in the pinned host mirror: an evaluation brings both home in ONE copy
    int nr_max = r + (q > p ? q : p);
    f->out_cap = (size_t)(1 + nr_max * nr_max) * (size_t)(f->nt + 2);
    {
        double *hbase = nullptr;
        CK(f->dinfo_out.alloc(f->out_cap + 1));
        CK(hipHostMalloc(&hbase, (f->out_cap + 2) * sizeof(double)));
        f->dinfo = (int *)f->dinfo_out.get(); f->dout = f->dinfo_out + 1;
        f->hinfo = (int *)hbase; f->hout = hbase + 1;
        f->hinfo_init = (int *)(hbase + 1 + f->out_cap);      // constant {0x7f7f7f7f, 0}: reset_info's source
        f->hinfo_init[0] = 0x7f7f7f7f; f->hinfo_init[1] = 0;
    }
    for (auto &e : f->ev) CK(hipEventCreate(&e));
    // (the engine's stream is created by engine_warm, and only for handles that may use the engine: every stream a process
    // holds takes a place in the round robin over the few hardware queues -- a batch slot on the plain schedule that created
    // one pushed the NEXT slot's main stream onto a queue already taken, and kernels of streams that share a queue run one
    // after the other: four "concurrent" slots ran on two queues, round 5's kernel trace)
    f->engine_ok = want_engine;
    CK(hipEventCreateWithFlags(&f->ev_eng, hipEventDisableTiming));
    // (two streams per handle and no more: every stream a process holds competes for the few hardware queues -- a third one
    // per handle, for a panel-overlap experiment since removed, halved the throughput of the batch slots)
    // (a taper handle allocates its buffer once the envelope of its pattern is known: packed, it is a fraction of n^2)
    if (!defer_matrix && fit_alloc_matrix(f, nr_max) != 0) { cocons_fit_destroy(f); return nullptr; }
#undef CK
    if (engine_warm(f) != 0) { cocons_fit_destroy(f); return nullptr; }
    // (return_locked: the caller goes on building the handle -- a batch slot, whose main stream may still be redrawn --, so it
    // enters the registry with its operation lock held and no other thread's stream self-test can touch it before it is done)
    if (return_locked) f->op_mu.lock();
    registry_add(f);
    return f;
}

extern "C" cocons_fit *cocons_fit_create(int n, int p, int r, int q, const double *locs,
                                         const double *X, const double *z, const double *x_betas,
                                         const double *smooth_limits, int device)
{
    return fit_create_impl(n, p, r, q, locs, X, z, x_betas, smooth_limits, device, true);
}

// Taper fit: the handle of an optimisation of GetNeg2loglikelihoodTaper (R/neg2loglikelihood.R:20-53).  The
// pattern (colindices / rowpointers, 1-based as spam stores them, symmetric, diagonal stored) and the taper's
// entries are those of `ref_taper`; cocons_neg2loglik_dense on this handle returns
//   sum_k [ n log 2 pi + 2 sum log diag chol(S) + resid_k' S^-1 resid_k ],   S = taper o cov_rns_taper(theta),
// the value spam's sparse Cholesky gives, obtained here through the DENSE factorisation of S (zeros stored):
// valid while n^2 doubles fit the device, and an n = 10^4 evaluation costs what a dense one costs.  The
// observations keep the caller's order (the pattern refers to it).
extern "C" cocons_fit *cocons_fit_create_taper(int n, int p, int r, const double *locs, const double *X, const double *z,
                                               const double *smooth_limits, int device, int nnz, const int *colindices,
                                               const int *rowpointers, const double *taper_entries)
{
    if (n <= 0 || nnz <= 0 || !colindices || !rowpointers || !taper_entries || r < 1) {
        fail(-1, "cocons_fit_create_taper: bad argument");
        return nullptr;
    }
    if (rowpointers[0] != 1 || rowpointers[n] != nnz + 1) {
        fail(-1, "cocons_fit_create_taper: rowpointers do not match nnz (1-based CSR expected)");
        return nullptr;
    }
    for (int i = 0; i < n; ++i) {
        bool diag = false;
        if (rowpointers[i + 1] < rowpointers[i]) { fail(-1, "cocons_fit_create_taper: rowpointers decrease"); return nullptr; }
        for (int w = rowpointers[i] - 1; w < rowpointers[i + 1] - 1; ++w) {
            if (colindices[w] < 1 || colindices[w] > n) { fail(-1, "cocons_fit_create_taper: column index out of range"); return nullptr; }
            if (colindices[w] == i + 1) diag = true;
        }
        if (!diag) {
            char msg[96];
            snprintf(msg, sizeof msg, "row %d stores no diagonal entry", i + 1);
            fail(-1, "cocons_fit_create_taper: %s", msg);
            return nullptr;
        }
    }
    // Order the observations by reverse Cuthill-McKee on the pattern (COCONS_TAPER_RCM=0: keep the caller's order):
    // the value does not depend on the order, the envelope of the factor does, and the factorisation below
    // only touches tiles inside it.
    std::vector<int> perm(n);                    // perm[new] = old
    {
        const char *e = getenv("COCONS_TAPER_RCM");
        const bool rcm = e ? atoi(e) != 0 : true;
        if (!rcm) { for (int i = 0; i < n; ++i) perm[i] = i; }
        else {
            std::vector<int> deg(n), order;
            std::vector<char> seen(n, 0);
            order.reserve(n);
            for (int i = 0; i < n; ++i) deg[i] = rowpointers[i + 1] - rowpointers[i];
            std::vector<int> nb;
            auto bfs = [&](int root, std::vector<int> &out) {        // Cuthill-McKee order of root's component
                const size_t first = out.size();
                out.push_back(root); seen[root] = 1;
                for (size_t h = first; h < out.size(); ++h) {
                    const int u = out[h];
                    nb.clear();
                    for (int w = rowpointers[u] - 1; w < rowpointers[u + 1] - 1; ++w) {
                        const int v2 = colindices[w] - 1;
                        if (!seen[v2]) { seen[v2] = 1; nb.push_back(v2); }
                    }
                    std::sort(nb.begin(), nb.end(), [&](int a2, int b2) { return deg[a2] != deg[b2] ? deg[a2] < deg[b2] : a2 < b2; });
                    for (int v2 : nb) out.push_back(v2);
                }
            };
            std::vector<int> byd(n);
            for (int i = 0; i < n; ++i) byd[i] = i;
            std::sort(byd.begin(), byd.end(), [&](int a2, int b2) { return deg[a2] != deg[b2] ? deg[a2] < deg[b2] : a2 < b2; });
            for (int c = 0; c < n; ++c) {
                const int start = byd[c];
                if (seen[start]) continue;
                // pseudo-peripheral root: the last vertex of a first sweep from the component's minimum-degree vertex
                std::vector<int> probe;
                bfs(start, probe);
                const int root = probe.back();
                for (int u : probe) seen[u] = 0;
                bfs(root, order);
            }
            for (int i = 0; i < n; ++i) perm[i] = order[n - 1 - i];
        }
    }
    return taper_create_ordered(n, p, r, locs, X, z, smooth_limits, device, nnz, colindices, rowpointers, taper_entries, perm,
                                false);
}

// ---------------------------------------------------------------------------
// Taper patterns from delta: what the entries that take (delta, kind) share, and the stateless builder.
int pattern_check_delta(const char *who, double delta, int kind)
{
    if (!std::isfinite(delta) || delta <= 0.0) return fail(-1, "%s: delta must be finite and > 0", who);
    if (kind < COCONS_TAPER_WEND1 || kind > COCONS_TAPER_SPH)
        return fail(-1, "%s: kind = %d is no taper (1 = wend1, 2 = wend2, 3 = sph)", who, kind);
    return 0;
}

int pattern_check_finite(const char *who, const char *what, size_t npts, const double *pts)
{
    for (size_t i = 0; i < 2 * npts; ++i)
        if (!std::isfinite(pts[i])) return fail(-1, "%s: a coordinate of %s is not finite (point %zu)", who, what, i % npts + 1);
    return 0;
}

int pattern_grid_alloc(const char *who, PatternGridBufs &G, size_t pts, size_t cells)
{
    HIPCHK_AT(who, G.cstart.alloc(cells + 1));
    HIPCHK_AT(who, G.cursor.alloc(cells + 1));
    HIPCHK_AT(who, G.sidx.alloc(pts));
    HIPCHK_AT(who, G.sxy.alloc(2 * pts));
    G.bytes = (long long)((2 * (cells + 1) + pts) * sizeof(int) + 2 * pts * sizeof(double));
    return 0;
}

int pattern_grid_bin(const char *who, PatternGridBufs &G, const PatternGrid &g, int cnt, const double *dx, const double *dy,
                     hipStream_t s)
{
    G.t.g = g;
    G.t.n = cnt; G.t.x = dx; G.t.y = dy;
    G.t.cstart = G.cstart; G.t.sidx = G.sidx; G.t.sx = G.sxy; G.t.sy = G.sxy + cnt;
    HIPCHK_AT(who, launch_pattern_bin(G.t, G.cursor, s));
    return 0;
}

int pattern_grid_build(const char *who, PatternGridBufs &G, int n, const double *hx, const double *hy, const double *dx,
                       const double *dy, double delta, hipStream_t s)
{
    const PatternGrid g = pattern_grid_make(n, hx, hy, delta);
    G.delta = delta;
    if (int rc = pattern_grid_alloc(who, G, (size_t)n, pattern_cells(g))) return rc;
    return pattern_grid_bin(who, G, g, n, dx, dy, s);
}

// cocons_taper_pattern under the name of the entry that asks (who)
static int taper_pattern_impl(const char *who, int n, const double *locs, int m, const double *locs_query, double delta, int kind,
                              int device, long long cap, long long *nnz, int *rowpointers, int *colindices, double *entries)
{
    if (!locs || !nnz || !rowpointers || (colindices && !entries)) return fail(-1, "%s: null argument", who);
    if (n < 1) return fail(-1, "%s: n = %d (at least one point expected)", who, n);
    if (locs_query && m < 1) return fail(-1, "%s: m = %d with a query set (at least one query expected)", who, m);
    if (int rc = pattern_check_delta(who, delta, kind)) return rc;
    if (int rc = pattern_check_finite(who, "locs", (size_t)n, locs)) return rc;
    if (locs_query)
        if (int rc = pattern_check_finite(who, "locs_query", (size_t)m, locs_query)) return rc;
    const int rows = locs_query ? m : n;
    HIPCHK_AT(who, hipSetDevice(device < 0 ? 0 : device));
    DevBuf<double> dl, dq, dent;
    DevBuf<int> drp, dci;
    DevBuf<long long> dtot;
    PatternGridBufs G;
    StreamDrain s{nullptr, true};     // own non-blocking stream (the library never launches on the NULL stream)
    HIPCHK_AT(who, hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking));
    HIPCHK_AT(who, dl.alloc((size_t)2 * n));
    HIPCHK_AT(who, drp.alloc((size_t)rows + 1));
    HIPCHK_AT(who, dtot.alloc(1));
    HIPCHK_AT(who, upload_canon(dl, locs, (size_t)2 * n, s));
    const double *qx = dl, *qy = dl + n;
    if (locs_query) {
        HIPCHK_AT(who, dq.alloc((size_t)2 * m));
        HIPCHK_AT(who, upload_canon(dq, locs_query, (size_t)2 * m, s));
        qx = dq; qy = dq + m;
    }
    if (int rc = pattern_grid_build(who, G, n, locs, locs + n, dl, dl + n, delta, s)) return rc;
    HIPCHK_AT(who, launch_pattern_count(G.t, rows, qx, qy, delta, drp, nullptr, 0, s));
    HIPCHK_AT(who, launch_scan_exclusive(drp, drp, rows, 1, dtot, s));
    long long total = 0;
    HIPCHK_AT(who, hipMemcpyAsync(&total, dtot, sizeof total, hipMemcpyDeviceToHost, s));
    HIPCHK_AT(who, hipStreamSynchronize(s));
    if (total > (long long)INT_MAX - 1)
        return fail(-1, "%s: the pattern holds %lld entries, more than an int counts (INT_MAX - 1 at most)", who, total);
    if (!colindices) {                // the count call
        HIPCHK_AT(who, hipMemcpyAsync(rowpointers, drp, ((size_t)rows + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipStreamSynchronize(s));
        *nnz = total;
        return 0;
    }
    if (cap < total) return fail(-1, "%s: cap = %lld is too small, the pattern holds nnz = %lld entries", who, cap, total);
    const size_t nz = total > 0 ? (size_t)total : 1;
    HIPCHK_AT(who, dci.alloc(nz));
    HIPCHK_AT(who, dent.alloc(nz));
    HIPCHK_AT(who, launch_pattern_fill(G.t, rows, qx, qy, delta, kind, drp, dci, dent, s));
    HIPCHK_AT(who, hipMemcpyAsync(rowpointers, drp, ((size_t)rows + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
    if (total > 0) {
        HIPCHK_AT(who, hipMemcpyAsync(colindices, dci, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK_AT(who, hipMemcpyAsync(entries, dent, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIPCHK_AT(who, hipStreamSynchronize(s));
    *nnz = total;
    return 0;
}

extern "C" int cocons_taper_pattern(int n, const double *locs, int m, const double *locs_query, double delta, int kind, int device,
                                    long long cap, long long *nnz, int *rowpointers, int *colindices, double *entries)
{
    return taper_pattern_impl("cocons_taper_pattern", n, locs, m, locs_query, delta, kind, device, cap, nnz, rowpointers, colindices,
                              entries);
}

extern "C" cocons_fit *cocons_fit_create_taper_delta(int n, int p, int r, const double *locs, const double *X, const double *z,
                                                     const double *smooth_limits, int device, double delta, int kind)
{
    const char *who = "cocons_fit_create_taper_delta";
    if (!locs || !X || !z || !smooth_limits) { fail(-1, "%s: null argument", who); return nullptr; }
    if (n < 1) { fail(-1, "%s: n = %d (at least one point expected)", who, n); return nullptr; }
    // the self pattern by the builder (count, then fill), and the handle as cocons_fit_create_taper makes it from the arrays
    std::vector<int> rp((size_t)n + 1), ci;
    std::vector<double> ent;
    long long nnz = 0;
    if (taper_pattern_impl(who, n, locs, n, nullptr, delta, kind, device, 0, &nnz, rp.data(), nullptr, nullptr)) return nullptr;
    ci.resize((size_t)nnz); ent.resize((size_t)nnz);
    if (taper_pattern_impl(who, n, locs, n, nullptr, delta, kind, device, nnz, &nnz, rp.data(), ci.data(), ent.data())) return nullptr;
    return cocons_fit_create_taper(n, p, r, locs, X, z, smooth_limits, device, (int)nnz, ci.data(), rp.data(), ent.data());
}

// Device copies of a taper handle's pattern (lower triangle, nnz entries), taper entries and envelope (hi may be null: none):
// from host vectors (taper_create_ordered) or device to device from another handle (clone_for_slot) on f's stream, drained.
static int taper_pattern_to_device(cocons_fit *f, size_t nnz, const int *ci, const int *rp, const double *val, const int *hi,
                                   bool from_host)
{
    auto copy = [&](void *dst, const void *src, size_t bytes) {
        // (from the host: synchronous copies, i.e. on the NULL stream the library otherwise stays off, DESIGN.md section 4a --
        // kept as it is: which hardware queue a process touches first is behaviour, see dag_prepare)
        return from_host ? hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)
                         : hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, f->stream);
    };
    HIPCHK(f->d_tci.alloc(nnz));
    HIPCHK(f->d_trp.alloc((size_t)f->n + 1));
    HIPCHK(f->d_tval.alloc(nnz));
    HIPCHK(copy(f->d_tci, ci, nnz * sizeof(int)));
    HIPCHK(copy(f->d_trp, rp, ((size_t)f->n + 1) * sizeof(int)));
    HIPCHK(copy(f->d_tval, val, nnz * sizeof(double)));
    if (hi) {
        HIPCHK(f->d_thi.alloc((size_t)f->nt));
        HIPCHK(copy(f->d_thi, hi, (size_t)f->nt * sizeof(int)));
    }
    if (!from_host) HIPCHK(hipStreamSynchronize(f->stream));
    f->taper_nnz = (int)nnz;
    return 0;
}

// The taper handle of a validated pattern with its observations in the order perm (perm[new] = index in the order the
// arguments come in).  check_fit: refuse, with a message that says so, a buffer larger than the device's free memory
// (an order with a wide envelope: cocons_sim_taper's twin) before any allocation is tried.
cocons_fit *taper_create_ordered(int n, int p, int r, const double *locs, const double *X, const double *z,
                                 const double *smooth_limits, int device, int nnz, const int *colindices,
                                 const int *rowpointers, const double *taper_entries, const std::vector<int> &perm,
                                 bool check_fit)
{
    std::vector<int> inv(n);                     // inv[old] = new
    for (int i = 0; i < n; ++i) inv[perm[i]] = i;
    std::vector<double> pl((size_t)2 * n), pX((size_t)p * n), pz((size_t)r * n);
    for (int i = 0; i < n; ++i) {
        const int o = perm[i];
        pl[i] = locs[o]; pl[(size_t)n + i] = locs[(size_t)n + o];
        for (int c = 0; c < p; ++c) pX[(size_t)c * n + i] = X[(size_t)c * n + o];
        for (int c = 0; c < r; ++c) pz[(size_t)c * n + i] = z[(size_t)c * n + o];
    }
    std::vector<int> prp(n + 1), pci(nnz);
    std::vector<double> pte(nnz);
    prp[0] = 1;
    for (int i = 0, w2 = 0; i < n; ++i) {
        const int o = perm[i];
        for (int w = rowpointers[o] - 1; w < rowpointers[o + 1] - 1; ++w, ++w2) {
            pci[w2] = inv[colindices[w] - 1] + 1;
            pte[w2] = taper_entries[w];
        }
        prp[i + 1] = w2 + 1;
    }
    cocons_fit *f = fit_create_impl(n, p, r, 0, pl.data(), pX.data(), pz.data(), nullptr, smooth_limits, device, false, true,
                                    true, true);       // (registered with its operation lock held: it is still being built)
    if (!f) return nullptr;
    f->taper_inv = inv;
    f->h_trp = prp;
    f->h_tci = pci;
    f->h_tval = pte;
    // the envelope per tile column (band_plan.hpp), unless switched off: dense factorisation of the tapered matrix
    const char *e = getenv("COCONS_TAPER_BAND");
    if (!(e && atoi(e) == 0)) {
        BandEnvelope env = band_envelope(n, prp.data(), pci.data(), TILE);
        f->taper_hi = std::move(env.hi); f->taper_maxband = env.maxband;
        // packed band storage unless switched off (COCONS_TAPER_PACKED=0: the dense n x n buffer, only its band used)
        const char *pk = getenv("COCONS_TAPER_PACKED");
        if (!(pk && atoi(pk) == 0) && f->taper_maxband < f->nt) f->skew = f->taper_maxband;
    }
    if (check_fit) {
        const size_t bytes = ((size_t)(f->skew > 0 ? f->skew * TILE : f->npad) + (size_t)round_up(r + p, TILE)) *
                             (size_t)f->npad * sizeof(double);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes > free_b) {
            char msg[192];
            snprintf(msg, sizeof msg, "%.2f GB (envelope of %d tile rows), %.2f GB free", bytes * 1e-9,
                     f->taper_maxband > 0 ? f->taper_maxband : f->nt, free_b * 1e-9);
            fail(-4, "the factor buffer of this order does not fit the device: %s", msg);
            f->op_mu.unlock();
            cocons_fit_destroy(f);
            return nullptr;
        }
    }
    if (fit_alloc_matrix(f, r + p) != 0) { f->op_mu.unlock(); cocons_fit_destroy(f); return nullptr; }
    // the device keeps the lower triangle of the pattern only (the upper half is never evaluated)
    {
        int w2 = 0;
        for (int i = 0; i < n; ++i) {
            const int a0 = prp[i] - 1, a1 = prp[i + 1] - 1;
            prp[i] = w2 + 1;
            for (int w = a0; w < a1; ++w)
                if (pci[w] - 1 <= i) { pci[w2] = pci[w]; pte[w2] = pte[w]; ++w2; }
        }
        prp[n] = w2 + 1;
        nnz = w2;
    }
    if (taper_pattern_to_device(f, nnz, pci.data(), prp.data(), pte.data(), envelope_or_null(f), true) != 0) {
        f->op_mu.unlock();
        cocons_fit_destroy(f);
        return nullptr;
    }
    // inside a narrow envelope the trailing updates are too short to hide the engine's hand-offs behind (4.9 against
    // 4.7 ms at n = 10^4): plain schedule
    if (!f->taper_hi.empty()) f->engine_ok = false;
    f->op_mu.unlock();
    return f;
}

// Does the handle hold exactly these data (bitwise)?  The R glue's handle cache asks on a miss of its address check
// (glue/cocons_hip_glue.c): O(n) host work, no device call.  1 = the same, 0 = different (or a taper handle / bad argument).
extern "C" int cocons_fit_same_data(cocons_fit *f, int n, int p, int r, int q, const double *locs, const double *X,
                                    const double *z, const double *x_betas, const double *smooth_limits)
{
    if (!f || !locs || !X || !smooth_limits || f->taper_nnz > 0 || f->vecchia) return 0;
    if (f->n_user != n || f->p != p || f->r != r || f->q != q) return 0;
    if (f->smooth_limits[0] != smooth_limits[0] || f->smooth_limits[1] != smooth_limits[1]) return 0;
    if (memcmp(f->h_locs.data(), locs, (size_t)2 * n * sizeof(double)) != 0) return 0;
    if (memcmp(f->h_X.data(), X, (size_t)n * p * sizeof(double)) != 0) return 0;
    if (r > 0 && (!z || memcmp(f->h_z.data(), z, (size_t)n * r * sizeof(double)) != 0)) return 0;
    if (q > 0 && (!x_betas || f->h_xb.size() != (size_t)n * q ||
                  memcmp(f->h_xb.data(), x_betas, (size_t)n * q * sizeof(double)) != 0)) return 0;
    return 1;
}

extern "C" void *cocons_fit_stream(cocons_fit *f) { return f ? (void *)f->stream : nullptr; }

static bool redraw_stream(hipStream_t &s, std::vector<hipStream_t> &losers);

// The handle's own pair again, for a main stream the caller has just installed: engine_warm proved at creation that the engine's
// stream runs beside the main stream the library had drawn, which says nothing about this one (a caller's stream that shares
// the engine stream's hardware queue makes every engine-schedule operation run into its bounded wait: correct values from the
// repeat on the plain schedule, 100 ms lost each time).  Only stream2 -- the library's own -- is redrawn, up to engine_warm's 8
// attempts; no clash-free draw, or the NULL stream (never probed): the handle takes the plain schedule until another stream is
// installed.  The caller is inside cocons_fit_set_stream and both streams are idle: the one place where the library launches its
// probe pair on a caller's stream.
static int own_pair_again(cocons_fit *f)
{
    if (f->engine_pair_lost) { f->engine_ok = true; f->engine_pair_lost = false; }
    if (!engine_enabled() || f->nt <= 4 || !f->engine_ok || !f->stream2 || !f->dflags) return 0;
    if (!f->stream) { f->engine_ok = false; f->engine_pair_lost = true; return 0; }
    HIPCHK(hipStreamSynchronize(f->stream));
    unsigned *words = handoff_words(f).selftest;
    std::vector<hipStream_t> losers;
    int ok = 0;
    for (int attempt = 0; attempt < 8; ++attempt) {
        ok = streams_run_concurrently(f->stream2, f->stream, words);
        if (ok != 0) break;
        if (!redraw_stream(f->stream2, losers)) { ok = -1; break; }
    }
    const bool redrawn = !losers.empty();
    for (hipStream_t l : losers) hipStreamDestroy(l);
    if (ok < 0) { (void)hipGetLastError(); return fail(-100, "cocons_fit_set_stream: stream self-test failed"); }
    if (ok == 0) { f->engine_ok = false; f->engine_pair_lost = true; return 0; }
    HIPCHK(hipMemsetAsync(f->dflags, 0, handoff_word_count(f->flags_cap) * sizeof(unsigned), f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
    if (redrawn) {
        // (the first dispatch of the engine kernel on a fresh stream is paid here, as at creation: engine_warm)
        const HandoffWords hw = handoff_words(f);
        EngineLaunch e;
        e.dinv = f->dinv; e.info = f->dinfo; e.in = e.out = e.xr = hw.in; e.abort_word = hw.abort; e.alive = hw.alive;
        launch_potrf_engine_warmup(e, false, f->stream2);
        if (tun().dag) launch_potrf_engine_warmup(e, true, f->stream2);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(f->stream2));
        f->engine_ops = 0;        // (the next engine-schedule operation is the first on this stream: its gate is patient)
    }
    return 0;
}

extern "C" int cocons_fit_set_stream(cocons_fit *f, void *stream)
{
    FIT_ENTER_ANY(f);
    // both streams idle before the swap: no event wait of the panel stream may refer to work on a
    // stream that is about to be destroyed
    HIPCHK(hipStreamSynchronize(f->stream));
    if (f->stream2) HIPCHK(hipStreamSynchronize(f->stream2));
    if (f->own_stream) { HIPCHK(hipStreamDestroy(f->stream)); f->own_stream = false; }
    f->stream = (hipStream_t)stream;
    return own_pair_again(f);
}

extern "C" int cocons_fit_sync(cocons_fit *f)
{
    FIT_ENTER_ANY(f);
    HIPCHK(hipStreamSynchronize(f->stream));
    return 0;
}

// ---------------------------------------------------------------------------
// placement of the streams on the hardware queues

// s shares a hardware queue with a stream it must run beside: it joins `losers` (kept alive until the caller is done, so that
// the next draw lands on another queue) and is drawn again.  false: no stream could be created; s is the old stream again.
static bool redraw_stream(hipStream_t &s, std::vector<hipStream_t> &losers)
{
    hipStream_t fresh = nullptr;
    if (hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking) != hipSuccess) return false;
    losers.push_back(s);
    s = fresh;
    return true;
}

// Warm-up of the engine's stream at handle creation: ONE launch of the engine kernel that raises its alive word and
// leaves (t0 >= nt), with the launch configuration of the real thing (512 threads, the dynamic LDS, the function
// attribute).  The first dispatch of a kernel on a stream that has never run anything makes the runtime set up the
// hardware queue behind it -- and, for a kernel with a private segment, scratch memory: round 3's engine had 88 B per
// lane, and the driver's box recorded a 5 ms gate time-out on the FIRST engine-schedule operation of a fresh process
// (DESIGN.md section 4a).  The kernel is scratch-free now, and what remains of the first-dispatch cost is paid here,
// outside any bounded wait.
static int engine_warm(cocons_fit *f)
{
    if (!engine_enabled() || f->nt <= 4 || !f->engine_ok) { f->engine_ok = f->engine_ok && f->stream2 != nullptr; return 0; }
    if (!f->stream2) HIPCHK(hipStreamCreateWithFlags(&f->stream2, hipStreamNonBlocking));
    if (int rc = flags_reset(f, f->nt)) return rc;
    HIPCHK(hipStreamSynchronize(f->stream));
    // The engine's stream must not share a hardware queue with the main stream (HIP multiplexes streams onto a few queues;
    // which one a stream gets depends on every stream the PROCESS has created): test it, and draw another stream if it
    // does -- the losers stay alive until a winner is found, so that the next draw lands elsewhere.  No luck: this handle
    // stays on the plain schedule.
    {
        std::vector<hipStream_t> losers;
        int ok = 0;
        for (int attempt = 0; attempt < 8; ++attempt) {
            ok = streams_run_concurrently(f->stream2, f->stream, handoff_words(f).selftest);
            if (ok != 0) break;
            if (!redraw_stream(f->stream2, losers)) { ok = -1; break; }
        }
        // ... and across handles: this handle's engine beside every other live handle's main stream, and every other live
        // handle's engine beside this handle's main stream.  (The own-pair test above says nothing about those: with a few
        // more streams in the process -- a batch slot, a second handle of the caller, torch's -- A.main can share a queue
        // with B.engine and B.main with A.engine: each engine then blocks the kernels the OTHER evaluation waits for, and only
        // the bounded waits end it -- correct values, seconds lost.)  Streams of handles that are busy right now are not
        // probed (the probe needs idle streams); a collision redraws THIS handle's stream and repeats all tests.  Only the
        // four most recent other handles are looked at, and a handle that finds no clash-free draw KEEPS its engine: four
        // hardware queues cannot keep a dozen live handles apart, and a clash only matters between handles that work at
        // the same moment (a test that holds twelve idle handles must not lose the engine on four of them).
        // Threads (round 6, the advisor's finding): the probe launches kernels on ANOTHER handle's streams.  It takes that handle's
        // operation lock first -- try_lock, under the registry's lock: a handle some thread is working on is busy and not probed, a
        // handle being destroyed has left the registry, and a handle that IS probed can neither be used nor destroyed until the
        // probe is over (cocons_fit_destroy waits for the lock) --, and it leaves streams the library does not own alone
        // (cocons_fit_set_stream: a caller's stream may carry the caller's own work).  This handle is not in the registry yet and
        // not in anybody's hands: redrawing ITS streams is safe here, and nowhere later.
        unsigned *words = handoff_words(f).selftest;
        for (int round = 0; ok == 1 && round < 8; ++round) {
            std::vector<cocons_fit *> others;
            {
                std::lock_guard<std::mutex> lk(g_reg_mutex);
                for (size_t i = g_registry.size(); i-- > 0 && others.size() < 4;) {      // the four most recent ones
                    cocons_fit *o = g_registry[i];
                    if (o == f || o->pid != f->pid || o->device != f->device || !o->own_stream || !o->stream || !o->stream2 ||
                        !o->engine_ok || !o->op_mu.try_lock())
                        continue;
                    if (hipStreamQuery(o->stream) == hipSuccess && hipStreamQuery(o->stream2) == hipSuccess) others.push_back(o);
                    else o->op_mu.unlock();
                }
            }
            (void)hipGetLastError();
            int clash = 0;                 // 1: this engine stream beside another main stream; 2: this main stream beside another engine
            for (cocons_fit *o : others) {
                int a = streams_run_concurrently(f->stream2, o->stream, words);
                if (a < 0) { ok = -1; break; }
                if (a == 0) { clash = 1; break; }
                if (f->own_stream) {
                    int b = streams_run_concurrently(o->stream2, f->stream, words);
                    if (b < 0) { ok = -1; break; }
                    if (b == 0) { clash = 2; break; }
                }
            }
            for (cocons_fit *o : others) o->op_mu.unlock();      // (streams_run_concurrently drains both streams before it returns)
            if (ok != 1 || clash == 0) break;
            hipStream_t &mine = clash == 1 ? f->stream2 : f->stream;
            if (!redraw_stream(mine, losers)) { ok = -1; break; }
            // the redrawn stream must still pair with this handle's other stream
            int again = streams_run_concurrently(f->stream2, f->stream, words);
            if (again < 0) { ok = -1; break; }
            if (again == 0) {
                // (the redrawn stream shares a queue with this handle's other stream: draw again next round -- the own pair
                // is what must never share)
                bool fixed = false;
                for (int t2 = 0; t2 < 4 && !fixed; ++t2) {
                    if (!redraw_stream(mine, losers)) { ok = -1; break; }
                    const int r2 = streams_run_concurrently(f->stream2, f->stream, words);
                    if (r2 < 0) { ok = -1; break; }
                    fixed = r2 == 1;
                }
                if (ok != 1) break;
                if (!fixed) { ok = 0; break; }
            }
        }
        for (hipStream_t l : losers) hipStreamDestroy(l);
        if (ok < 0) { (void)hipGetLastError(); return fail(-100, "engine_warm: stream self-test failed"); }
        if (ok == 0) { f->engine_ok = false; return 0; }
        HIPCHK(hipMemsetAsync(f->dflags, 0, handoff_word_count(f->flags_cap) * sizeof(unsigned), f->stream));
        HIPCHK(hipStreamSynchronize(f->stream));
    }
    const HandoffWords hw = handoff_words(f);
    EngineLaunch e;
    e.dinv = f->dinv; e.info = f->dinfo; e.in = e.out = e.xr = hw.in; e.abort_word = hw.abort; e.alive = hw.alive;
    launch_potrf_engine_warmup(e, false, f->stream2);
    if (tun().dag) launch_potrf_engine_warmup(e, true, f->stream2);        // the other instantiation of the engine
    HIPCHK(hipGetLastError());
    if (f->stream2) HIPCHK(hipStreamSynchronize(f->stream2));
    return 0;
}

// A second handle over the same data with its own factorisation buffer and streams: one slot of
// cocons_neg2loglik_batch.  A taper handle's clone shares nothing on the device (pattern and taper entries are
// copied device to device) and keeps the order and the envelope of its original.
// A slot's main stream must run BESIDE the main streams of the handle and of its other slots (kernels of streams that share
// a hardware queue run one after the other): tested like the engine's stream, redrawn on a clash.
static void slot_stream_apart(cocons_fit *f, cocons_fit *c)
{
    if (!c->own_stream || !c->dflags) return;
    unsigned *words = handoff_words(c).selftest;
    std::vector<hipStream_t> losers;
    for (int attempt = 0; attempt < 8; ++attempt) {
        bool clash = false;
        std::vector<cocons_fit *> peers{f};
        for (cocons_fit *o : f->slots) if (o != c) peers.push_back(o);
        for (cocons_fit *o : peers) {
            if (!o->own_stream) continue;      // (a caller's stream is never probed for another handle's sake: engine_warm likewise)
            if (hipStreamQuery(o->stream) != hipSuccess) { (void)hipGetLastError(); continue; }      // (busy: not probed)
            const int r = streams_run_concurrently(o->stream, c->stream, words);
            if (r == 0) { clash = true; break; }
            if (r < 0) { (void)hipGetLastError(); break; }
        }
        if (!clash) break;
        if (!redraw_stream(c->stream, losers)) break;
    }
    for (hipStream_t l : losers) hipStreamDestroy(l);
    if (c->stream2 && streams_run_concurrently(c->stream2, c->stream, words) == 0) c->engine_ok = false;     // (its own pair again)
    (void)hipMemsetAsync(c->dflags, 0, handoff_word_count(c->flags_cap) * sizeof(unsigned), c->stream);
    (void)hipStreamSynchronize(c->stream);
}

cocons_fit *clone_for_slot(cocons_fit *f, bool want_engine)
{
    // (a clone enters the registry with its operation lock held -- fit_create_impl(..., return_locked) -- and keeps it until it
    // is complete: its main stream may still be redrawn below, which no other thread's stream self-test may see half done)
    if (f->taper_nnz <= 0) {
        cocons_fit *c = fit_create_impl(f->n_user, f->p, f->r, 0, f->h_locs.data(), f->h_X.data(), f->h_z.data(), nullptr,
                                        f->smooth_limits, f->device, true, false, want_engine, true);
        if (c) {
            if (!c->dflags && flags_reset(c, c->nt) != 0) { c->op_mu.unlock(); cocons_fit_destroy(c); return nullptr; }
            hipStreamSynchronize(c->stream);
            slot_stream_apart(f, c);
            c->engine_ok = c->engine_ok && c->stream2 != nullptr;
            c->op_mu.unlock();
        }
        return c;
    }
    cocons_fit *c = fit_create_impl(f->n_user, f->p, f->r, 0, f->h_locs.data(), f->h_X.data(), f->h_z.data(), nullptr,
                                    f->smooth_limits, f->device, false, true, false, true);      // h_* of a taper handle are in ITS order;
    if (!c) return nullptr;                                                                  // band-limited: never an engine
    struct Unlock { cocons_fit *c; ~Unlock() { if (c) c->op_mu.unlock(); } } unlock{c};
    auto drop = [&]() { unlock.c = nullptr; c->op_mu.unlock(); cocons_fit_destroy(c); return (cocons_fit *)nullptr; };
    if (!c->dflags && flags_reset(c, c->nt) != 0) return drop();
    hipStreamSynchronize(c->stream);
    slot_stream_apart(f, c);
    c->skew = f->skew;                        // the same (packed) buffer layout as the original
    if (fit_alloc_matrix(c, f->r + f->p) != 0) return drop();
    c->taper_hi = f->taper_hi;
    c->taper_inv = f->taper_inv;
    c->taper_maxband = f->taper_maxband;
    // (asynchronous on the clone's own stream: the library makes no call on the NULL stream)
    if (taper_pattern_to_device(c, (size_t)f->taper_nnz, f->d_tci, f->d_trp, f->d_tval, f->d_thi, false) != 0) return drop();
    // a band-limited handle never uses the engine, nor do its clones; a taper handle WITHOUT an envelope (COCONS_TAPER_BAND=0)
    // may -- but this clone was created without an engine stream (want_engine = false), and an engine launched on a null
    // stream would land on the NULL stream the library never touches (round 5's regression, the advisor's finding)
    c->engine_ok = f->engine_ok && c->stream2 != nullptr;
    return c;
}
