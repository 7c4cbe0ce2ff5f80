// api.hip -- C ABI of the dense hot path (see include/cocons_hip.h for the contract and the
// reference interface each entry point replaces).  This file: errors and the handle's life, the schedules and the
// factorisation, the objective entries, the covariance entries and the DAG diagnostics -- everything on the path of one
// objective evaluation.  api_shard.hip, api_predict.hip and api_grad.hip hold the entries built on top of it (fit.hpp).
#include "fit.hpp"

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char *cocons_last_error(void) { return g_err.c_str(); }
extern "C" int cocons_abi_version(void) { return 1; }

extern "C" int cocons_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { g_err = hipGetErrorString(e); return -1; }
    return n;
}

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
// theta -> kernel arguments, exactly the host-side preamble of the reference functions

// Host-to-device copy of caller or host-computed doubles through canon_nan.  The normal case is the plain copy; only when an
// all-ones NaN is present is a canonical host copy staged, and the stream drained before that copy goes out of scope.
hipError_t upload_canon(double *dst, const double *src, size_t count, hipStream_t s)
{
    size_t first = 0;
    for (unsigned long long b; first < count; ++first) {
        memcpy(&b, src + first, sizeof b);
        if (b == ~0ull) break;
    }
    if (first == count) return hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyHostToDevice, s);
    std::vector<double> stage(src, src + count);
    for (size_t i = first; i < count; ++i) stage[i] = canon_nan(stage[i]);
    hipError_t e = hipMemcpyAsync(dst, stage.data(), count * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

// full_scale: the taper entries' FULL scale vector in two_scale_je (cocons_taper.cpp:207), the first scale included
void make_theta_vecs(const double *theta_in, int p, ThetaVecs &tv, bool full_scale)
{
    double theta[6 * COCONS_P_MAX];
    for (int i = 0; i < 6 * p; ++i) theta[i] = canon_nan(theta_in[i]);
    memset(&tv, 0, sizeof tv);
    for (int i = 0; i < p; ++i) {
        double sje = (i == 0) ? 0.0 : theta[TH_SCALE * p + i];      // cocons_full.cpp:49,64
        tv.tilt[i] = theta[TH_TILT * p + i];
        tv.two_scale_je[i] = 2 * (full_scale ? theta[TH_SCALE * p + i] : sje);      // :101
        tv.aniso[i] = theta[TH_ANISO * p + i];
        tv.sqrt_vector[i] = 2 * sje + theta[TH_ANISO * p + i];      // :66
        tv.half_sd[i] = 0.5 * theta[TH_SD * p + i];                 // :104
        tv.nugget[i] = theta[TH_NUGGET * p + i];
        tv.smooth[i] = theta[TH_SMOOTH * p + i];
        tv.sd[i] = theta[TH_SD * p + i];
    }
}

// which = 0 cov_rns, 1 cov_rns_classic, 2 cov_rns_pred
ModeSel select_mode(const double *theta, int p, const double *smooth_limits, int which)
{
    ModeSel m;
    m.gr = canon_nan(1 / std::exp(-2 * theta[TH_SCALE * p + 0]));   // :62, :351, :501
    m.nu_fixed = 0.0;
    if (which == 1) { m.mode = MODE_MEAN; m.smooth_kind = SMOOTH_EXP; return m; }
    if (which == 2) { m.mode = MODE_GEOM; m.smooth_kind = SMOOTH_LOGISTIC_SQRT; return m; }
    bool fix = true;                                                // allzeroelements, types.h:56-63
    for (int i = 1; i < p; ++i)
        if (theta[TH_SMOOTH * p + i] != 0) fix = false;
    if (fix && smooth_limits[0] == smooth_limits[1]) {              // :85-88
        double v = smooth_limits[0];
        m.nu_fixed = v;
        m.smooth_kind = SMOOTH_ZERO;
        if (std::fabs(v - 0.5) < 1e-6) m.mode = MODE_HALF;          // types.h:65-70
        else if (std::fabs(v - 1.5) < 1e-6) m.mode = MODE_THREEHALF;
        else if (std::fabs(v - 2.5) < 1e-6) m.mode = MODE_FIVEHALF;
        else m.mode = MODE_GEOM;   // quirk: zero smooth vector -> u = 0 -> every entry = diag_ii
    } else {
        m.mode = MODE_GEOM;
        m.smooth_kind = SMOOTH_LOGISTIC_SQRT;
    }
    return m;
}

// loc_params arguments of n locations: X (n x p) and locs (n x 2) column-major with leading dimension n, the SoA to out
LocArgs loc_args(int n, int p, const double *X, const double *locs, double *out, size_t stride, const ThetaVecs &tv,
                 int smooth_kind, const double *smooth_limits)
{
    LocArgs la;
    la.n = n; la.p = p;
    la.X = X; la.ldx = n;
    la.locs = locs; la.ldl = n;
    la.out = out; la.stride = stride;
    la.smooth_kind = smooth_kind;
    la.smooth_min = smooth_limits[0]; la.smooth_max = smooth_limits[1];
    la.th = tv;
    return la;
}

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

int fit_check(cocons_fit *f)
{
    if (!f) return fail(-1, "null fit handle");
    if (f->pid != getpid())
        return fail(-2, "fit handle was created in another process (fork); create it in the worker");
    hipError_t e = hipSetDevice(f->device);
    if (e != hipSuccess) return fail(-3, "hipSetDevice: %s", hipGetErrorString(e));
    return 0;
}

// rows under the matrix that an operation with rhs_rows right-hand sides reserves: whole tiles
static int rhs_rows_cap(int rhs_rows) { return round_up(rhs_rows > 0 ? rhs_rows : 1, TILE); }

int fit_alloc_matrix(cocons_fit *f, int rhs_rows)
{
    int cap = rhs_rows_cap(rhs_rows);
    f->rhs_act = cap;        // a buffer grown by an earlier predict call must not slow later evaluations
    border_unknown(f);      // every user of the rows under the matrix comes through here
    if (f->dA && cap <= f->rhs_cap) return 0;
    f->rhs_cap = cap;
    f->lda = (size_t)(f->skew > 0 ? f->skew * TILE : f->npad) + cap;
    // (exactly lda * npad: a buffer that a gradient call had grown goes back to the objective's size with the new shape)
    HIPCHK(f->dA.reserve(f->lda * (size_t)f->npad, f->stream, f->stream2, -1, true));
    // never-written parts must not hold NaN bit patterns: a band-limited factorisation only clears its envelope, and
    // 0 * garbage must stay 0 whatever the allocator hands back (every time the buffer takes a new shape)
    HIPCHK(hipMemsetAsync(f->dA, 0, f->lda * (size_t)f->npad * sizeof(double), f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
    return 0;
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
    if (!f || !locs || !X || !smooth_limits || f->taper_nnz > 0) return 0;
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

extern "C" int cocons_fit_set_stream(cocons_fit *f, void *stream)
{
    FIT_ENTER(f);
    // both streams idle before the swap: no event wait of the panel stream may refer to work on a
    // stream that is about to be destroyed
    HIPCHK(hipStreamSynchronize(f->stream));
    if (f->stream2) HIPCHK(hipStreamSynchronize(f->stream2));
    if (f->own_stream) { HIPCHK(hipStreamDestroy(f->stream)); f->own_stream = false; }
    f->stream = (hipStream_t)stream;
    return 0;
}

extern "C" int cocons_fit_sync(cocons_fit *f)
{
    FIT_ENTER(f);
    HIPCHK(hipStreamSynchronize(f->stream));
    return 0;
}

// ---------------------------------------------------------------------------
// assembly of Sigma (+ identity padding) into the factorisation buffer, lower triangle.
// bj0 / ncols restrict the 64-wide tile columns (sharded path); full range otherwise.
void assemble_sigma(cocons_fit *f, const double *theta, int which, int col0, int col1)
{
    ThetaVecs tv;
    make_theta_vecs(theta, f->p, tv);
    ModeSel ms = select_mode(theta, f->p, f->smooth_limits, which);
    launch_loc_params(loc_args(f->n, f->p, f->dX, f->dlocs, f->dloc, f->npad, tv, ms.smooth_kind, f->smooth_limits), f->stream);
    PairArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.n = f->n; pa.m = f->n;
    pa.rows = f->dloc; pa.cols = f->dloc;
    pa.stride = f->npad; pa.stride_rows = f->npad;
    pa.out = f->dA; pa.ld = f->lda;
    pa.nrows_out = f->npad; pa.ncols_out = col1;
    pa.bj0 = col0 / 64;
    if (pa.bj0 < f->pad0 / 64) pa.bj0 = f->pad0 / 64;      // 64-wide tile rows / columns that are placeholders only: not assembled
    pa.pad_diag = f->nslot > 0 ? 1e300 : 1.0;               // slot columns: a diagonal no right-hand side can turn negative
    pa.gr = ms.gr; pa.nu_fixed = ms.nu_fixed;
    launch_pair_sym(ms.mode, false, pa, f->stream);
}

// Taper fit: Sigma_tap = taper o cov_rns_taper(theta) (R/neg2loglikelihood.R:25-31) as a dense lower triangle.
// Parameters exactly as cocons_cov_rns_taper prepares them (FULL scale vector, src/cocons_taper.cpp:207).
int assemble_sigma_taper(cocons_fit *f, const double *theta)
{
    ThetaVecs tv;
    make_theta_vecs(theta, f->p, tv, true);
    ModeSel ms = select_mode(theta, f->p, f->smooth_limits, 0);
    launch_loc_params(loc_args(f->n, f->p, f->dX, f->dlocs, f->dloc, f->npad, tv, ms.smooth_kind, f->smooth_limits), f->stream);
    // zero what the factorisation will read: the tiles inside the envelope (the rows under the matrix are written in
    // full by the right-hand-side kernel), or the whole buffer when the factorisation is not band-limited
    if (f->d_thi) launch_band_zero(f->dA, f->lda, f->d_thi, f->nt, f->taper_maxband, f->stream, f->skew);
    else HIPCHK(hipMemsetAsync(f->dA, 0, f->lda * (size_t)f->npad * sizeof(double), f->stream));
    TaperLaunch t;
    t.mode = ms.mode; t.nrows = f->n; t.nnz = f->taper_nnz; t.ci = f->d_tci; t.rp = f->d_trp; t.nu_fixed = ms.nu_fixed;
    t.rows = t.cols = f->dloc; t.stride_rows = t.stride = f->npad;
    t.tapv = f->d_tval; t.A = f->dA; t.lda = f->lda; t.skew = f->skew; t.npad = f->npad;
    launch_taper(t, f->stream);
    launch_pad_identity(f->dA, f->lda, f->n, f->npad, f->stream, f->skew);
    return 0;
}

int no_taper(cocons_fit *f, const char *who)
{
    if (f->taper_nnz > 0) return fail(-1, "%s: not available on a taper fit (cocons_neg2loglik_dense is)", who);
    return 0;
}

// right-hand-side rows under the matrix: rows npad.. : z columns (minus trend), then xb columns
void assemble_rhs(cocons_fit *f, const double *mean, bool use_trend, const double *xb, int nxb,
                  int col0, int col1, bool zero_rest, bool slots)
{
    if (slots) { zero_rest = false; col1 = f->n; }      // (the assembly zeroed the slot rows; their own columns are not touched)
    RhsArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.n = f->n; ra.p = f->p; ra.X = f->dX; ra.ldx = f->n;
    ra.use_trend = use_trend ? 1 : 0;
    if (use_trend) for (int i = 0; i < f->p; ++i) ra.mean[i] = canon_nan(mean[i]);
    ra.src = f->dz; ra.lds = f->n;
    ra.out = f->dA; ra.ld = f->lda;
    ra.skew = f->skew; ra.npad = f->npad;
    ra.row0 = slots ? f->n : f->npad; ra.nrows = f->r;
    ra.nrows_zero = (nxb > 0 || !zero_rest) ? 0 : f->rhs_act - f->r;
    ra.col0 = col0; ra.ncols_out = col1;
    launch_rhs_rows(ra, f->stream);
    if (nxb > 0) {
        ra.use_trend = 0;
        ra.src = xb; ra.lds = f->n;
        ra.row0 = (slots ? f->n : f->npad) + f->r; ra.nrows = nxb;
        ra.nrows_zero = zero_rest ? f->rhs_act - f->r - nxb : 0;
        launch_rhs_rows(ra, f->stream);
    }
}

// Bordered right-looking factorisation, outer block = 2 tiles (256 columns).
//   panel(k)  : potrf(k) | trsm(k) | update tile column k+1 (K=128) | potrf(k+1) | trsm(k+1)
//   U1(k)     : update of the NEXT block's two tile columns with panel k (K = 256)
//   U2(k)     : update of everything right of that
// Look-ahead: panel(k+2) runs on a second stream as soon as U1(k) is done, concurrently
// with U2(k) on the main stream; U1(k+2) waits for it.  mt = total tile rows (matrix + rhs
// rows).  Optional per-launch timing of U2 via events (ev_upd): appended (start, stop).
FactorView main_view(cocons_fit *f)
{
    FactorView v;
    v.A = f->dA; v.lda = f->lda; v.nt = f->nt; v.mt = f->nt + f->rhs_act / TILE;
    v.hi = envelope_or_null(f);
    v.skew = f->skew;
    return v;
}

static RhsLayout rhs_layout(const cocons_fit *f, int nrhs)
{
    RhsLayout l;
    l.slots = f->nslot >= nrhs && f->nslot > 0;
    const int act = rhs_rows_cap(nrhs);
    l.tile_rows = l.slots ? 0 : act / TILE;
    l.trim = (!l.slots && act - nrhs >= 64) ? 1 : 0;
    return l;
}

// the view of the matrix an evaluation with this layout factors (after fit_alloc_matrix(f, nrhs))
static FactorView rhs_view(cocons_fit *f, const RhsLayout &l)
{
    FactorView v = main_view(f);
    v.mt = v.nt + l.tile_rows;
    v.trim = l.trim;
    return v;
}

// one past the last band row tile of the 256-column block starting at tile k (at least the next diagonal block, so
// that the update which the engine's hand-off hangs on always covers it); -1 = dense
static int band_hi(const FactorView &v, int k)
{
    if (!v.hi) return -1;
    int h = v.hi[k];
    if (k + 1 < v.nt && v.hi[k + 1] > h) h = v.hi[k + 1];
    const int need = k + 4 < v.nt ? k + 4 : v.nt;
    if (h < need) h = need;
    return h < v.nt ? h : v.nt;
}

// tile factorisation + the panel solve below it.  (ONE launch for the two -- the solve's workgroups fetch their rows, wait for
// a word the factorising workgroup raises, take L and solve -- was built and measured in round 5: SLOWER, taper path 4.18 -> 4.57
// ms, batch at n = 4096 1066 -> 1031 evaluations/s: the boundary between the two launches costs less than the write-through
// factor and the serialised fetch of L behind the word; removed.)
// (Round 5, later: ONE launch after all -- not behind a word but FOLLOWING the factorisation through the tile's mailbox, the way the
// engine's partner does: potrf_follow_kernel.  The mailboxes are filled by mbox_reset at the start of the factorisation.)
static void potrf_solve(cocons_fit *f, double *A, size_t lda, int tile, const RowRange &rows, double *q, hipStream_t s)
{
    TrsmLaunch l;
    l.A = A; l.lda = lda; l.c0 = tile * TILE; l.rows = rows; l.dinv = q;
    if (tun().potrf_follow != 0 && !f->follow_off && tile_mbox(f, f->nt + 1) && (l.mbox = tile_mbox(f, tile)) != nullptr) {
        f->follow_used = true;
        l.info = f->dinfo; l.abort_word = handoff_words(f).abort;
        launch_potrf_follow(l, s);
        return;
    }
    launch_potrf_tile(A, lda, tile * TILE, q, f->dinfo, s);
    launch_trsm_tile(l, s);
}

static void panel_ops(cocons_fit *f, const FactorView &v, int k, hipStream_t s)
{
    double *q0 = f->dinv, *q1 = f->dinv + 8 * 256;
    const int hb = band_hi(v, k);                       // rows [.., hb) of the band, then the rows under the matrix [nt, mt)
    potrf_solve(f, v.A, v.lda, k, v.panel_rows(k + 1, hb), q0, s);
    if (k + 1 < v.nt) {
        UpdateLaunch u = v.update(hb);
        u.panel_in_c(k * TILE); u.K = TILE; u.ti0 = k + 1; u.ti1 = v.mt; u.tj0 = k + 1; u.tj1 = k + 2; u.lower_only = true;
        launch_update(u, s);
        potrf_solve(f, v.A, v.lda, k + 1, v.panel_rows(k + 2, hb), q1, s);
    }
}

// The table of the switches above: tune name (cocons_debug_tune), environment variable (read once, at the first use; nullptr:
// tests and tools only) and the least value the switch takes (a smaller one is raised to it)
struct TuneRow { const char *name, *env; int Tunables::*field; int lo; };
static const TuneRow tune_rows[] = {
    {"engine", "COCONS_ENGINE", &Tunables::engine, INT_MIN},
    {"dag", "COCONS_DAG", &Tunables::dag, INT_MIN},
    {"dag_lead", "COCONS_DAG_LEAD", &Tunables::dag_lead, INT_MIN},
    {"dag_lead2", "COCONS_DAG_LEAD2", &Tunables::dag_lead2, INT_MIN},
    {"dag_lead3", "COCONS_DAG_LEAD3", &Tunables::dag_lead3, INT_MIN},
    {"dag_min_tiles", "COCONS_DAG_MIN_TILES", &Tunables::dag_min_tiles, INT_MIN},
    {"dag_xcc_quota", "COCONS_DAG_XCC_QUOTA", &Tunables::dag_xcc_quota, INT_MIN},
    {"dag_xcd", "COCONS_DAG_XCD", &Tunables::dag_xcd, INT_MIN},
    {"dag_order", "COCONS_DAG_ORDER", &Tunables::dag_order, INT_MIN},
    {"dag_xcd_min_quota", nullptr, &Tunables::dag_xcd_min_quota, INT_MIN},
    {"dag_bw", "COCONS_DAG_BW", &Tunables::dag_bw, 1},        // (0 would make dag_build_far_table loop forever)
    {"dag_bh", "COCONS_DAG_BH", &Tunables::dag_bh, 1},
    {"dag_trace", nullptr, &Tunables::dag_trace, INT_MIN},
    {"engine_pair", "COCONS_ENGINE_PAIR", &Tunables::engine_pair, INT_MIN},
    {"panel_fused", "COCONS_PANEL_FUSED", &Tunables::panel_fused, INT_MIN},
    {"potrf_follow", "COCONS_POTRF_FOLLOW", &Tunables::potrf_follow, INT_MIN},
    {"panel_split", "COCONS_PANEL_SPLIT", &Tunables::panel_split, INT_MIN},
    {"gate_sabotage", nullptr, &Tunables::gate_sabotage, INT_MIN},
    {"host_delay_us", "COCONS_DEBUG_HOST_DELAY_US", &Tunables::host_delay_us, INT_MIN},
    {"host_delay_tile", "COCONS_DEBUG_HOST_DELAY_TILE", &Tunables::host_delay_tile, INT_MIN},
    {"engine_in_wait_ms", nullptr, &Tunables::engine_in_wait_ms, INT_MIN},
};
static void tune_set(Tunables &t, const TuneRow &r, int value) { t.*r.field = value < r.lo ? r.lo : value; }

Tunables &tun()
{
    static Tunables t;
    if (!t.init) {
        for (const TuneRow &r : tune_rows)
            if (const char *e = r.env ? getenv(r.env) : nullptr) tune_set(t, r, atoi(e));
        t.init = true;
    }
    return t;
}

extern "C" int cocons_debug_tune(const char *name, int value)
{
    if (!name) return fail(-1, "cocons_debug_tune: null name");
    Tunables &t = tun();
    std::string k(name);
    for (const TuneRow &r : tune_rows)
        if (k == r.name) { tune_set(t, r, value); return 0; }
    if (k == "upd_waves") set_update_waves(value);
    else if (k == "w8_max_tiles") set_update_w8_max_tiles(value);
    else if (k == "c_wt") set_update_c_wt(value);
    else return fail(-1, "cocons_debug_tune: unknown switch %s", name);
    return 0;
}

// Workgroups of the persistent launch that may take part on the XCD that also hosts the engine.
// Measured there: an XCD that runs kernels of two queues does not hold eight of these workgroups on every CU -- 227 instead of
// 248 beside the engine's CU: seven on most, eight on some -- and the set that fits changes when the driver's save / restore
// moves the engine.  The quota keeps the launch below what fits in ANY placement: seven per CU on the XCD's other CUs, less
// one CU's worth and one: (CUs per XCD - 1) x 7 - 9 = 208 for the 32 CUs per XCD of MI355X (the value of round 4's soak runs:
// 0 time-outs in 40 000 evaluations), from hipDeviceProp instead of a constant; COCONS_DAG_XCC_QUOTA overrides.
static int dag_xcc_quota()
{
    if (tun().dag_xcc_quota >= 0) return tun().dag_xcc_quota;
    static int derived = -1;
    if (derived < 0) {
        const int cus = device_cus();
        const int xcds = 8;                                 // gfx950: eight accelerator dies (no HIP attribute reports it)
        const int cpx = cus % xcds == 0 ? cus / xcds : 32;
        derived = (cpx - 1) * 7 - 9;
        if (derived < 8) derived = 8;
    }
    return derived;
}

// Chunk exponent of the XCD-aware deal of the persistent launch's task list (chol.hip: dag_position; 0 = one counter for all).
// The deal assumes the eight XCDs of the whole chip -- a partitioned device keeps the one counter -- and XCDs that contribute
// comparable numbers of workgroups: a class of list positions whose XCD holds almost none is carried by the others only while
// they are free to draw, and with everybody waiting at that class's tasks the launch crawls at the pace of its few workgroups
// until a bounded wait ends it (tools/diag/quota_stress.py) -- a quota below dag_xcd_min_quota (half an XCD's share), which
// only the tests set, keeps the one counter too.
static int dag_xcd_group()
{
    const int q = dag_xcc_quota();
    return (tun().dag_xcd && device_cus() == 256 && (q == 0 || q >= tun().dag_xcd_min_quota)) ? 5 : 0;
}

// COCONS_ENGINE: 1 (default) = diagonal tiles are factored by the resident engine while the trailing
// update runs; 0 = every kernel in order on one stream
bool engine_enabled() { return tun().engine != 0; }

// one trailing-update launch (tile columns [t0, t1) of the trapezoid below (t0, t0)), optionally
// bracketed by timing events (profile runs): appended as (start, stop)
static void timed_update(cocons_fit *f, const FactorView &v, int k, int kw, int t0, int t1, hipStream_t s,
                         std::vector<hipEvent_t> *ev_upd, unsigned *sig, int sig_tile, unsigned *queue = nullptr,
                         int skip_tiles = 0)      // > 0: the diagonal block at t0 (that many tiles) was updated by the panel's launch
{
    const int mt = v.mt;
    if (t1 <= t0) return;
    const int hb = band_hi(v, k);                       // band-limited: tile columns and rows [t0, hb), plus the rows [nt, mt)
    if (hb >= 0 && hb < t1) t1 = hb;
    if (t1 <= t0) return;
    hipEvent_t a = nullptr, b = nullptr;
    if (ev_upd) {
        hipEventCreate(&a); hipEventCreate(&b);
        hipEventRecord(a, s);
    }
    // the first panel's leading columns are the unit vectors of the front padding (zero below the diagonal): they add
    // nothing to the trailing matrix, so the update starts behind them (whole 16-column chunks; bit-identical)
    const int kskip = (k == 0 && !v.hi) ? (f->pad0 / 16) * 16 : 0;
    UpdateLaunch u = v.update(hb);
    u.panel_in_c(k * TILE + kskip); u.K = kw * TILE - kskip; u.ti0 = t0; u.ti1 = mt; u.tj0 = t0; u.tj1 = t1; u.lower_only = true;
    u.sig = sig; u.sig_tile = sig_tile; u.queue = queue; u.abort_word = sig ? handoff_words(f).abort : nullptr;   // engine schedule: see update_kernel
    if (skip_tiles > 0) { u.skip_lo = 2 * t0; u.skip_hi = 2 * (t0 + skip_tiles); }
    launch_update(u, s);
    if (ev_upd) {
        hipEventRecord(b, s);
        ev_upd->push_back(a); ev_upd->push_back(b);
    }
}

// algorithmic flops of the trailing update of block k (tile columns [t0, nt)): lower triangle of the
// trailing block of order m (real columns only) times K, plus the rhs rows:  K m (m+1) + 2 K r m
static void count_update_flops(cocons_fit *f, int kw, int t0)
{
    double m = (double)f->n_user - ((double)t0 * TILE - (double)f->pad0);      // the caller's rows and columns from t0 on
    if (m > (double)f->n_user) m = (double)f->n_user;
    if (m < 0) m = 0;
    const double K = (double)kw * TILE - (t0 == kw ? (double)f->pad0 : 0.0);     // the first panel holds pad0 placeholder columns
    f->upd_flops += K * m * (m + 1.0) + 2.0 * K * (double)f->nrhs_cur * m;
}

// Reset the hand-off words and launch the diagonal-block engine (see factorize) for a factorisation of view
// v on the second stream, ordered behind the reset.  The engine's 8 waves take every VGPR of a CU, so it can
// only be placed on an EMPTY one: enqueue_eval calls this between the covariance assembly and the short
// right-hand-side kernel, and factorize holds the main stream behind a one-lane gate kernel until the engine
// reports itself resident.
// (Launched between the assembly and the first trailing update it could lose that race and then wait for
// a whole update to drain; with workgroups that wait for the engine on every CU it would never be placed.)
static bool engine_wanted(cocons_fit *f, const FactorView &v)
{
    return engine_enabled() && f->engine_ok && f->stream2 != nullptr && f->engine_skip == 0 && v.nt > 4;
}

// the hand-off words and tile counters of one factorisation with nt tiles, zeroed on the main stream
int flags_reset(cocons_fit *f, int nt)
{
    if (f->flags_cap < nt) {
        const int cap = round_up(nt + 8, 64);
        HIPCHK(f->dflags.reserve(handoff_word_count(cap), f->stream, f->stream2));
        f->flags_cap = cap;
    }
    HIPCHK(hipMemsetAsync(f->dflags, 0, handoff_word_count(f->flags_cap) * sizeof(unsigned), f->stream));
    return 0;
}

// the tiles' mailboxes (the engine's pair mode, the panel kernel, potrf_solve's followers) filled with the pattern that means "not
// written yet" (every byte 0xff; potrf_tile_body: mbox) on the main stream: 88 KB each, 7.1 MB at n = 10^4
int mbox_reset(cocons_fit *f, int nt, bool engine_schedule)
{
    // one allocation, one fill: the tiles' mailboxes | the strip mailboxes (0.5 MB per diagonal block) | the exchange mailboxes of
    // the split panel (64 KB per 64-row strip); the one-launch panel follows the pair's tiles
    const MboxLayout l = mbox_layout(nt, tun().panel_fused && tun().engine_pair, tun().panel_split != 0);
    HIPCHK(f->dmbox.reserve(l.total(), f->stream, f->stream2));
    f->mbox = l;
    // (the plain schedule uses the tiles' mailboxes only)
    HIPCHK(hipMemsetAsync(f->dmbox, 0xff, (engine_schedule ? l.total() : l.tiles) * sizeof(double), f->stream));
    return 0;
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
            losers.push_back(f->stream2);
            f->stream2 = nullptr;
            if (hipStreamCreateWithFlags(&f->stream2, hipStreamNonBlocking) != hipSuccess) { ok = -1; break; }
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
            losers.push_back(mine);
            mine = nullptr;
            if (hipStreamCreateWithFlags(&mine, hipStreamNonBlocking) != hipSuccess) { ok = -1; break; }
            // the redrawn stream must still pair with this handle's other stream
            int again = streams_run_concurrently(f->stream2, f->stream, words);
            if (again < 0) { ok = -1; break; }
            if (again == 0) {
                // (the redrawn stream shares a queue with this handle's other stream: draw again next round -- the own pair
                // is what must never share)
                bool fixed = false;
                for (int t2 = 0; t2 < 4 && !fixed; ++t2) {
                    losers.push_back(mine);
                    mine = nullptr;
                    if (hipStreamCreateWithFlags(&mine, hipStreamNonBlocking) != hipSuccess) { ok = -1; break; }
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

// ---- the dependency-driven schedule (chol.hip: dag_kernel) ---------------------------------------------------------
static bool dag_wanted(cocons_fit *f, const FactorView &v)
{
    return tun().dag != 0 && v.dag_ok && !v.hi && !v.skew && v.nt > 4 && f->world == 1;
}

// buffers, zeroed task words and the step table of the factorisation of view v (on the main stream, before the engine starts)
static int dag_prepare(cocons_fit *f, const FactorView &v)
{
    const size_t elems = v.lda * (size_t)f->npad;
    HIPCHK(f->dP.reserve(elems, f->stream, f->stream2, 0, true));       // (the shape of the view exactly; zeroed when new)
    if (!f->dpart) HIPCHK(f->dpart.alloc((size_t)2 * 16 * 64 * 64));
    HIPCHK(f->dWt.reserve((size_t)v.nt * TILE * TILE, f->stream, f->stream2, 0));   // zero above the diagonals, for good
    const int kskip = (f->pad0 / 16) * 16;
    const int xcd_g = dag_xcd_group();
    const int key[12] = {v.nt, v.mt, v.trim, kskip, tun().dag_lead, tun().dag_min_tiles, tun().dag_lead2, tun().dag_lead3,
                         tun().dag_order, xcd_g, tun().dag_bw, tun().dag_bh};
    if (memcmp(key, f->dag_key, sizeof key) != 0 || !f->ddag_steps) {
        std::vector<DagStepHost> steps;
        std::vector<unsigned> ftab;
        const bool want_tab = tun().dag_order != 0 || xcd_g > 0;
        const unsigned ntasks = dag_build_steps(v.nt, v.mt, v.trim, kskip, tun().dag_lead, tun().dag_min_tiles, steps,
                                                tun().dag_lead2, tun().dag_lead3, want_tab ? &ftab : nullptr, xcd_g,
                                                tun().dag_order ? tun().dag_bw : 0, tun().dag_bh);
        HIPCHK(hipStreamSynchronize(f->stream));      // (the table in place may be in use, whether or not a buffer below grows)
        if (f->stream2) HIPCHK(hipStreamSynchronize(f->stream2));
        HIPCHK(f->ddag_steps.reserve(steps.size() + 1, f->stream, f->stream2, -1, true));
        // (on the handle's own stream: the library never touches the NULL stream -- a synchronous hipMemcpy here gave it a
        // hardware queue of its own and shifted every later stream's assignment)
        HIPCHK(hipMemcpyAsync(f->ddag_steps, steps.data(), steps.size() * sizeof(DagStepHost), hipMemcpyHostToDevice, f->stream));
        HIPCHK(f->ddag_ftab.reserve(ftab.size(), f->stream, f->stream2));
        if (!ftab.empty())
            HIPCHK(hipMemcpyAsync(f->ddag_ftab, ftab.data(), ftab.size() * sizeof(unsigned), hipMemcpyHostToDevice, f->stream));
        f->dag_xcd_g = want_tab ? xcd_g : 0;
        f->dag_have_ftab = want_tab && !ftab.empty();
        HIPCHK(hipStreamSynchronize(f->stream));
        f->dag_nsteps = (int)steps.size(); f->dag_ntasks = ntasks;
        memcpy(f->dag_key, key, sizeof key);
        HIPCHK(f->ddag.reserve(dag_words(f, v.mt).total, f->stream, f->stream2));
    }
    HIPCHK(hipMemsetAsync(f->ddag, 0, f->ddag.count() * sizeof(unsigned), f->stream));
    // trace buffer: 4 stamps + one word of hw_where() pairs per task, 8 stamps per tile pair of the engine -- sized by BOTH
    // the task count and the tile count of THIS step table (a later table with fewer tasks and more tiles must not run past it)
    const size_t trace_elems = dag_trace_words(f, v.nt).count;
    if (tun().dag_trace) HIPCHK(f->ddag_trace.reserve(trace_elems, f->stream, f->stream2));
    f->dag_trace_tasks = (tun().dag_trace && f->ddag_trace) ? f->dag_ntasks : 0;      // 0: the buffer does not describe this table
    if (f->dag_trace_tasks)
        HIPCHK(hipMemsetAsync(f->ddag_trace, 0, trace_elems * sizeof(unsigned long long), f->stream));
    return 0;
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

// the persistent launch of view v on the handle's step table, task words and the hand-off words hw (no trace)
static DagLaunch dag_launch(cocons_fit *f, const FactorView &v, const HandoffWords &hw, const unsigned *alive)
{
    const DagWords w = dag_words(f, v.mt);
    DagLaunch d;
    d.A = v.A; d.lda = v.lda; d.P = f->dP; d.Wt = f->dWt; d.steps = f->ddag_steps; d.nsteps = f->dag_nsteps; d.ntasks = f->dag_ntasks;
    d.queue = w.queue; d.tdone = w.tdone; d.pdone = w.pdone; d.pstride = w.pstride; d.pall = w.pall; d.dcount = w.dcount; d.xcnt = w.xcnt;
    d.partbuf = f->dpart; d.sig = hw.in; d.out = hw.out; d.xr = hw.xr; d.abort_word = hw.abort;
    d.alive = alive; d.xcc_quota = dag_xcc_quota(); d.xcd_g = f->dag_xcd_g;
    if (f->dag_have_ftab) d.ftab = f->ddag_ftab;
    return d;
}

static int engine_start(cocons_fit *f, const FactorView &v)
{
    if (f->engine_live) return 0;
    const int nt = v.nt;
    hipStream_t M = f->stream;
    if (int rc = flags_reset(f, nt)) return rc;
    f->dag_next = dag_wanted(f, v);
    if (f->dag_next) {
        if (int rc = dag_prepare(f, v)) return rc;
        if (f->dag_nsteps < 2) f->dag_next = false;          // too small a problem for a head worth the launch: classic throughout
    }
    f->engine_pair_live = tun().engine_pair != 0 ? 1 : 0;
    if (f->engine_pair_live || (tun().potrf_follow && !f->follow_off))
        if (int rc = mbox_reset(f, nt > f->nt ? nt : f->nt)) return rc;
    HIPCHK(hipEventRecord(f->ev_eng, M));                    // (behind the resets of the flag and task words, and of W / P when new)
    HIPCHK(hipStreamWaitEvent(f->stream2, f->ev_eng, 0));
    // (from tile 0: the engine factors the first diagonal block too, its input words raised by the gate kernel -- band-limited
    // views, whose first block is not the engine's, never get the engine: fit_create_taper)
    const HandoffWords hw = handoff_words(f);
    EngineLaunch e;
    e.A = v.A; e.lda = v.lda; e.nt = nt; e.dinv = f->dinv; e.info = f->dinfo; e.in_wait_ms = tun().engine_in_wait_ms;
    e.in = hw.in; e.out = hw.out; e.xr = hw.xr; e.abort_word = hw.abort; e.alive = hw.alive;
    if (f->dag_next) { e.wbuf = f->dWt; e.pbuf = f->dP; e.dag_until = 2 * f->dag_nsteps; }
    if (f->dag_next && f->dag_trace_tasks) e.trace = dag_trace_words(f, nt).engine;
    if (f->engine_pair_live) e.mbox = f->dmbox;
    launch_potrf_engine(e, f->stream2);
    f->engine_live = true;
    return 0;
}

// Bordered right-looking factorisation, outer block = 2 tiles (256 columns).
//
// Plain schedule (COCONS_ENGINE=0, or fewer than 5 tiles), everything on the main stream:
//   potrf(t) | trsm(t) | in-panel update of tile column t+1 | potrf(t+1) | trsm(t+1) | trailing update
//
// Engine schedule: the 256 x 256 diagonal blocks from tile 2 on are factored by ONE resident workgroup
// (potrf_engine_kernel, launched once per factorisation on the second stream, on a CU of its own) as
// soon as the trailing update has published them; the main stream runs, per block k with t = k + 2:
//   U(k)      : trailing update with panel k, tile column t first; its workgroups inside the diagonal
//               block raise in[t] / in[t+1]      -> the engine factors tile t, forms X = A(t+1,t) L(t)^-T,
//                                                   updates and factors tile t+1 (all while U(k) runs)
//   trsm(t)   : rows below the diagonal block; waits for out[t]
//   in-panel update of tile column t+1 (rows below the block) with column t; waits for xr[t]
//   trsm(t+1) : waits for out[t+1]
// So the serial part of every panel -- two 30 us single-workgroup factorisations and the tile between
// them -- is off the critical path as long as U(k) lasts ~90 us; the main stream needs no events and
// issues fewer launches than the plain schedule.
int factorize(cocons_fit *f, const FactorView &v, std::vector<hipEvent_t> *ev_upd)
{
    const int nt = v.nt, mt = v.mt;
    hipStream_t M = f->stream;
    // the placeholder observations in front (fit_create_impl): whatever the assembly kernels put into their columns --
    // covariances, right-hand sides, cross-covariance rows -- is replaced by unit vectors, in every view whose first
    // indices are the handle's observations
    launch_front_identity(v.A, v.lda, f->pad0, mt * TILE, M);
    f->follow_used = false;
    if (!engine_wanted(f, v)) {
        f->engine_used = false;
        f->dag_used = false;
        if (int rc = flags_reset(f, nt)) return rc;
        if (tun().potrf_follow && !f->follow_off)
            if (int rc = mbox_reset(f, nt > f->nt ? nt : f->nt, false)) return rc;
        if (v.hi) {
            // band-limited: one tile column per step (factor, solve, update with K = 128) -- inside a narrow envelope
            // the in-panel update of the two-tile block costs more than the second, cheaper trailing update
            // (4.71 -> 4.53 ms at n = 10^4)
            // (row bound = the column's OWN envelope hi[k] -- per 256-block, monotone, >= k + 1 --, not band_hi(): for an
            // odd k that is the NEXT block's bound, beyond what band_zero_kernel clears in column k)
            // (packed band buffer: the kernels that stay inside tile column k address it by global indices through a
            // shifted base, where the rows under the matrix start at row (k + skew) * 128 -- kernels.h band_base)
            for (int k = 0; k < nt; ++k) {
                const int hb = v.hi[k] < nt ? v.hi[k] : nt;
                double *q = f->dinv + (size_t)(k & 1) * 2048;
                double *Ak = band_base(v.A, k, v.skew);
                const int e0 = v.skew ? k + v.skew : nt, e1 = e0 + (mt - nt);      // tile rows under the matrix
                RowRange rows;
                rows.r0 = (k + 1) * TILE; rows.r1 = e1 * TILE - 64 * v.trim; rows.band_r1 = hb * TILE; rows.ext_r0 = e0 * TILE;
                potrf_solve(f, Ak, v.lda, k, rows, q, M);
                if (k + 1 < nt) {
                    UpdateLaunch u = v.update(hb);
                    u.panel_in_c(k * TILE); u.K = TILE; u.ti0 = k + 1; u.ti1 = mt; u.tj0 = k + 1; u.tj1 = hb < nt ? hb : nt; u.lower_only = true;
                    u.skew = v.skew;
                    launch_update(u, M);
                }
            }
            return 0;
        }
        for (int k = 0; k < nt; k += 2) {
            panel_ops(f, v, k, M);
            if (k + 2 < nt) {
                if (ev_upd) count_update_flops(f, 2, k + 2);
                timed_update(f, v, k, 2, k + 2, nt, M, ev_upd, nullptr, -1, handoff_words(f).tile_queue(k));
            }
        }
        return 0;
    }
    if (int rc = engine_start(f, v)) return rc;          // no-op when enqueue_eval started it before the assembly
    f->engine_live = false;
    f->engine_used = true;
    const HandoffWords hw = handoff_words(f);
    unsigned *const in = hw.in, *const out = hw.out, *const xr = hw.xr, *const abort_word = hw.abort;
    unsigned *alive = hw.alive;
    if (tun().gate_sabotage > 0) { --tun().gate_sabotage; alive += 1; }      // (tests: a word that stays zero)
    // (the engine factors the first diagonal block too: the gate raises its input words; the pair partner counts itself)
    launch_start_gate(alive, abort_word, f->engine_ops++ == 0, f->engine_pair_live,
                      (tun().gate_sabotage == 0 && alive == hw.alive) ? in : nullptr, M);
    // the panel of the block at tile t (behind the engine's factorisation of it): one launch whose strips follow the pair's tiles
    // through their mailboxes, or three launches that wait for the tiles; returns the tiles of the NEXT diagonal block that the
    // launch has updated (the update launch behind it then leaves them alone)
    auto panel_for = [&](int t, bool allow_diag) -> int {
        const bool two = t + 1 < nt;                 // the block has a second tile
        const int r0 = two ? t + 2 : t + 1;          // first tile row below the diagonal block
        const int hb = band_hi(v, t);                // rows of block t's panel: [r0, hb) and the rows under the matrix
        const RowRange rows = v.panel_rows(r0, hb);
        if (two && hb < 0 && tun().panel_fused && f->engine_pair_live && f->dmbox != nullptr) {
            // the next diagonal block (tiles t + 2, t + 3), when there is one, is updated inside this launch
            const int next_tiles = t + 2 < nt ? (t + 3 < nt ? 2 : 1) : 0;
            const int nstrips = (rows.r1 - rows.r0) / 64;
            PanelLaunch p;
            p.A = v.A; p.lda = v.lda; p.c0 = t * TILE; p.rows = rows; p.xr = xr + t; p.abort_word = abort_word;
            p.mb0 = tile_mbox(f, t); p.mb1 = tile_mbox(f, t + 1); p.sig = in; p.sig_tile = t + 2;
            if (allow_diag && next_tiles > 0) p.smb = strip_mbox(f, t >> 1);
            if (p.smb) p.ndiag = next_tiles == 2 ? 10 : 3;
            if (tun().panel_split > 0 && nstrips >= tun().panel_split) p.xmb = xchg_mbox(f, nstrips);
            launch_panel_pair(p, M);
            return (p.smb && nstrips >= (next_tiles == 2 ? 4 : 2)) ? next_tiles : 0;
        }
        TrsmLaunch l;
        l.A = v.A; l.lda = v.lda; l.c0 = t * TILE; l.rows = rows; l.dinv = f->dinv + (size_t)(t & 1) * 2048; l.wait_word = out + t; l.abort_word = abort_word;
        launch_trsm_tile(l, M);
        if (two) {
            UpdateLaunch u = v.update(hb);
            u.panel_in_c(t * TILE); u.K = TILE; u.ti0 = r0; u.ti1 = mt; u.tj0 = t + 1; u.tj1 = t + 2; u.wait_word = xr + t; u.abort_word = abort_word;
            launch_update(u, M);
            l.c0 = (t + 1) * TILE; l.dinv = f->dinv + (size_t)((t + 1) & 1) * 2048; l.wait_word = out + t + 1;
            launch_trsm_tile(l, M);
        }
        return 0;
    };
    // tiles of the diagonal block at t that the previous panel's launch has updated (the persistent launch updates its first
    // diagonal block itself)
    int diag_done = panel_for(0, !f->dag_next);
    f->dag_used = f->dag_next;
    int k_first = 0;                 // first block step the classic loop below runs in full
    if (f->dag_next) {
        // the head of the factorisation -- the steps whose update fills the chip several times over -- is ONE persistent
        // launch (dag_kernel): tiles of update k + 1 start as soon as the strips of panel k + 1 they need and their own tile of
        // update k are done, and the panels between them are tile tasks of the same launch (the engine publishes the tile
        // inverses they multiply with).  Behind the head a step is bound by its dependency chain, and there the classic
        // sequence below has the shorter one: it takes over with the panel behind the last DAG step.
        hipEvent_t ea = nullptr, eb = nullptr;
        if (ev_upd) {
            const double before = f->upd_flops;
            for (int s = 0; s < f->dag_nsteps; ++s) count_update_flops(f, 2, 2 * s + 2);
            f->dag_flops = f->upd_flops - before;
            hipEventCreate(&ea); hipEventCreate(&eb);
            hipEventRecord(ea, M);
        }
        DagLaunch d = dag_launch(f, v, hw, alive);
        if (f->dag_trace_tasks) { const DagTraceWords tw = dag_trace_words(f, nt); d.trace = tw.tasks; d.hw = tw.hw; }
        launch_dag(d, M);
        if (ev_upd) { hipEventRecord(eb, M); ev_upd->push_back(ea); ev_upd->push_back(eb); f->dag_events = 1; }
        k_first = 2 * f->dag_nsteps;
    }
    // (Running the panel kernels on a stream of their own behind near-tile flags, so that they start in the tail of the
    // update that feeds them, was built and measured in round 3: slower -- a 90 KB-LDS solve is not placed beside eight
    // update workgroups per CU, the event back to the main stream costs 12 us -- and removed; so were three forms of the
    // panel as products with explicit inverses published by the engine (round 3: +-1 %, deleted in round 4); DESIGN.md
    // section 8.)
    for (int k = k_first > 0 ? k_first - 2 : 0; k + 2 < nt; k += 2) {
        const int t = k + 2;
        // (tests: a late host -- whatever raises in[host_delay_tile], the panel launch of block t or the update launch behind it,
        // is enqueued host_delay_us late, while the engine has everything it needs to get there and wait)
        if (tun().host_delay_us > 0 && t + 2 == tun().host_delay_tile) usleep((useconds_t)tun().host_delay_us);
        if (k >= k_first) {                          // (the update with the last DAG step's panel was that launch's)
            if (ev_upd) count_update_flops(f, 2, t);
            timed_update(f, v, k, 2, t, nt, M, ev_upd, in, t, hw.tile_queue(k), diag_done);
        }
        diag_done = panel_for(t, k + 4 < nt);
    }
    // no rows under the matrix (right-hand sides in the slots of the last tile): nothing on the main stream has waited for
    // the engine's last tile yet -- what follows (the reductions) must
    if (mt == nt) launch_last_tile_gate(out + (nt - 1), abort_word, M);
    return 0;
}

int reset_info(cocons_fit *f)
{
    HIPCHK(hipMemcpyAsync(f->dinfo, f->hinfo_init, 2 * sizeof(int), hipMemcpyHostToDevice, f->stream));
    return 0;
}

// enqueue one full evaluation with nrhs right-hand-side rows; results land in hout/hinfo
static int enqueue_eval_impl(cocons_fit *f, const double *theta, const double *mean, bool use_trend,
                             const double *xb, int nxb, std::vector<hipEvent_t> *ev_upd, bool stage_events)
{
    const int nrhs = f->r + nxb;
    f->nrhs_cur = nrhs;
    // the padding rows under the right-hand sides (a 128-row tile holds them; r + q of its rows are used) only have to
    // be zeroed when they may hold something else: zero rows stay exactly zero through a factorisation that succeeds
    // (10 MB of strided stores, 22 us on the critical path of every evaluation at n = 10^4)
    const int was_clean = f->border_clean;
    const double *was_A = f->dA;
    if (int rc = fit_alloc_matrix(f, nrhs)) return rc;
    const bool zero_rest = !(was_clean == nrhs && was_A == f->dA);
    f->border_pending = nrhs;
    if (stage_events) hipEventRecord(f->ev[0], f->stream);
    if (int rc = reset_info(f)) return rc;
    if (f->taper_nnz > 0) { if (int rc = assemble_sigma_taper(f, theta)) return rc; }
    else assemble_sigma(f, theta, 0, 0, f->npad);
    // the engine becomes resident while the (short) right-hand-side kernel runs: not earlier -- a second
    // queue with a resident kernel cuts the workgroup dispatch rate of every other launch to a quarter
    // (tools/diag/occupancy_probe.hip), which costs the 12,000-workgroup assembly 6 % -- and not later, see engine_start
    const RhsLayout lay = rhs_layout(f, nrhs);
    const bool slots = lay.slots;
    FactorView fv = rhs_view(f, lay);
    fv.dag_ok = true;                                 // (the reductions below read the factor from both buffers)
    if (engine_wanted(f, fv))
        if (int rc = engine_start(f, fv)) return rc;
    assemble_rhs(f, mean, use_trend, xb, nxb, 0, f->npad, zero_rest, slots);
    if (stage_events) hipEventRecord(f->ev[1], f->stream);
    if (int rc = factorize(f, fv, ev_upd)) return rc;
    if (stage_events) hipEventRecord(f->ev[2], f->stream);
    launch_finalize(f->dA, f->lda, f->n, slots ? f->n : f->npad, nrhs, f->dout, f->stream, f->skew, f->npad,
                    f->dag_used ? f->dP : nullptr, f->dag_used ? 2 * TILE * f->dag_nsteps : 0);
    HIPCHK(hipMemcpyAsync(f->hinfo, f->dinfo, (size_t)(2 + nrhs * nrhs) * sizeof(double),       // info words + outputs
                          hipMemcpyDeviceToHost, f->stream));
    if (stage_events) hipEventRecord(f->ev[3], f->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

static int enqueue_eval(cocons_fit *f, const double *theta, const double *mean, bool use_trend,
                        const double *xb, int nxb, std::vector<hipEvent_t> *ev_upd, bool stage_events)
{
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    const int rc = enqueue_eval_impl(f, theta, mean, use_trend, xb, nxb, ev_upd, stage_events);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    f->enq_host_us += (t1.tv_sec - t0.tv_sec) * 1e6 + (t1.tv_nsec - t0.tv_nsec) * 1e-3;
    f->enq_calls++;
    return rc;
}

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
static void debug_abort_report(cocons_fit *f)
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

int info_status(cocons_fit *f)
{
    if (f->hinfo[1] != 0) {
        if (getenv("COCONS_DEBUG_ABORT")) debug_abort_report(f);
        return fail(ENGINE_ABORT, "hand-off between the diagonal-tile engine and the main stream timed out");
    }
    // the operation ran to its end on the schedule factorize chose: book-keeping of the engine's back-off
    f->engine_active_last = f->engine_used;
    if (f->engine_used) f->engine_fails = 0;
    else if (f->engine_skip > 0) --f->engine_skip;
    int info = f->hinfo[0];
    if (info != 0x7f7f7f7f) {
        info -= f->pad0;                // (minors are counted in the handle's internal order, behind its front padding)
        if (info < 1) info = 1;
        if (info > f->n_user) info = f->n_user;   // failure reported inside the identity padding cannot happen; clamp anyway
        g_err = "leading minor not positive";
        return info;
    }
    f->border_clean = f->border_pending;      // every pivot positive and finite: zero rows are still zero
    f->border_pending = -1;
    return 0;
}

// The engine could not be scheduled in time, or one of its partners could not (another process or stream kept
// every CU busy, or a profiler serialises kernels): the caller repeats THIS operation once on the plain schedule;
// the handle stays on it for a few more operations (2, 4, ... 64 with consecutive time-outs) and then tries the
// engine again.  Every time-out is counted (cocons_fit_engine_state).
bool engine_retry(cocons_fit *f, int st)
{
    if (st != ENGINE_ABORT || !(f->engine_used || f->follow_used)) return false;
    f->engine_retries++;
    f->engine_last_abort = f->hinfo[1];
    if (!f->engine_used || abort_class((unsigned)f->hinfo[1]) == ABORT_FOLLOW) f->follow_off = true;      // a follower of potrf_follow_kernel gave up: two launches from now on
    if (f->engine_fails < 6) f->engine_fails++;
    f->engine_skip = 1 << f->engine_fails;
    f->engine_live = false;
    f->engine_used = false;
    if (f->stream2) hipStreamSynchronize(f->stream2);
    return true;
}

// One evaluation of the objective, repeated after a hand-off time-out.  enqueue_eval brings the info words home together
// with the outputs (one copy); 0, a failing minor or an error.
static int run_eval(cocons_fit *f, const double *theta, const double *mean, bool use_trend, const double *xb, int nxb)
{
    for (;;) {
        if (int rc = enqueue_eval(f, theta, mean, use_trend, xb, nxb, nullptr, false)) return rc;
        HIPCHK(hipStreamSynchronize(f->stream));
        const int st = info_status(f);
        if (!engine_retry(f, st)) return st;
    }
}

// out[0] = 1 if the last completed operation of the handle ran on the engine schedule, out[1] = hand-off time-outs
// so far (each was followed by a repeat on the plain schedule), out[2] = abort code of the last one (0 = none)
extern "C" int cocons_fit_engine_state(cocons_fit *f, int *out)
{
    if (!f || !out) return fail(-1, "cocons_fit_engine_state: null argument");
    out[0] = f->engine_active_last ? 1 : 0;
    out[1] = f->engine_retries;
    out[2] = f->engine_last_abort;
    // (the slots of cocons_neg2loglik_batch are handles of their own: their time-outs count for this handle)
    for (cocons_fit *c : f->slots) {
        out[1] += c->engine_retries;
        if (!out[2]) out[2] = c->engine_last_abort;
    }
    // (so are the twin of cocons_sim_taper's pivot route and the unsorted clone cocons_sim_dense runs on)
    for (cocons_fit *c : {f->taper_twin, f->unsorted})
        if (c) {
            out[1] += c->engine_retries;
            if (!out[2]) out[2] = c->engine_last_abort;
        }
    return 0;
}

extern "C" int cocons_neg2loglik_dense(cocons_fit *f, const double *theta, const double *mean,
                                       double *sum_logliks, double *parts)
{
    FIT_ENTER(f);
    if (!theta || !mean || !sum_logliks) return fail(-1, "cocons_neg2loglik_dense: null argument");
    if (f->r < 1) return fail(-1, "cocons_neg2loglik_dense: fit has no z");
    if (f->coll_kind < 0) return fail(-7, "cocons_neg2loglik_dense: the communicator of this fit was aborted after an error");
    if (f->coll_kind) return sharded_eval(f, theta, mean, sum_logliks, parts);    // (also with one rank: the caller asked for it)
    if (int st = run_eval(f, theta, mean, true, nullptr, 0)) return st;
    dense_collect(f, sum_logliks, parts);
    return 0;
}

void dense_collect(cocons_fit *f, double *sum_logliks, double *parts)
{
    const int nr = f->r;
    double logdet = f->hout[0], total = 0.0;
    for (int k = 0; k < nr; ++k) {                                   // R/neg2loglikelihood.R:212-218
        double quad = f->hout[1 + k * nr + k];
        total += f->n_user * LOG_2PI + 2 * logdet + quad;
        if (parts) parts[1 + k] = quad;
    }
    if (parts) parts[0] = logdet;
    *sum_logliks = total;
}

// Batch of independent evaluations (the 2P finite-difference points of one L-BFGS-B gradient,
// R/optim.R:237-259 + R/profile.R:11-12, or getHessian's 3 P (P+1)/2 points,
// R/getFunctions.R:979-1016): evaluation i runs on slot i mod S, each slot a clone of the fit
// with its own factorisation buffer and stream, so the latency-bound panel chain of one
// evaluation overlaps the MFMA-bound updates and the VALU-bound assembly of the others.
// thetas: nb x (6 p) row-major tables; means: nb x p; values[nb]; status[nb] (0 / k>0 like the
// single call).  Returns 0 unless a HIP / argument error occurred.
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
            if (hipStreamQuery(o->stream) != hipSuccess) { (void)hipGetLastError(); continue; }      // (busy: not probed)
            const int r = streams_run_concurrently(o->stream, c->stream, words);
            if (r == 0) { clash = true; break; }
            if (r < 0) { (void)hipGetLastError(); break; }
        }
        if (!clash) break;
        losers.push_back(c->stream);
        c->stream = nullptr;
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { c->stream = losers.back(); losers.pop_back(); break; }
    }
    for (hipStream_t l : losers) hipStreamDestroy(l);
    if (c->stream2 && streams_run_concurrently(c->stream2, c->stream, words) == 0) c->engine_ok = false;     // (its own pair again)
    (void)hipMemsetAsync(c->dflags, 0, handoff_word_count(c->flags_cap) * sizeof(unsigned), c->stream);
    (void)hipStreamSynchronize(c->stream);
}

static cocons_fit *clone_for_slot(cocons_fit *f, bool want_engine)
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

extern "C" int cocons_neg2loglik_batch(cocons_fit *f, int nb, const double *thetas, const double *means,
                                       double *values, int *status)
{
    FIT_ENTER(f);
    if (nb < 0 || (nb > 0 && (!thetas || !means || !values || !status)))
        return fail(-1, "cocons_neg2loglik_batch: bad argument");
    if (f->r < 1) return fail(-1, "cocons_neg2loglik_batch: fit has no z");
    // How many evaluations in flight, and on which schedule (round 5, from the kernel trace of a batch,
    // tools/diag/batch_trace.py): a process's streams share FOUR hardware queues, and kernels of streams that share one run one
    // after the other.  A resident engine holds its queue for the whole evaluation, so two engine-schedule evaluations -- 2
    // main + 2 engine streams -- are all that fits; a third runs behind one of them (n = 4096: 862 evaluations/s with two
    // slots, 695 with three).  On the plain schedule a slot needs ONE queue -- once the slots no longer create engine streams
    // they never use, which had put four slots' main streams on two queues (one queue busy 88 % of the time in the trace) --
    // and four evaluations in flight beat two with engines at every size measured: n = 4096 1067 against 862 evaluations/s,
    // n = 10^4 134 against 128 (33-point gradient).  More hardware queues (GPU_MAX_HW_QUEUES = 8, 12) make it WORSE (642 ... 996
    // at n = 4096): four is what the chip runs side by side.  COCONS_BATCH_ENGINE=1 (two engine slots) and COCONS_BATCH_SLOTS override.
    static int nslots_env = -1, batch_engine = -2;
    if (nslots_env < 0) {
        const char *e = getenv("COCONS_BATCH_SLOTS");
        nslots_env = e ? atoi(e) : 0;
        if (nslots_env < 0) nslots_env = 0;
        if (nslots_env > 8) nslots_env = 8;
        const char *e2 = getenv("COCONS_BATCH_ENGINE");
        batch_engine = e2 ? (atoi(e2) ? 1 : 0) : -1;
    }
    const bool eng_mode = batch_engine >= 0 ? batch_engine == 1 : false;
    const int nslots = nslots_env > 0 ? nslots_env : (eng_mode ? 2 : 4);
    int S = nb < nslots ? (nb > 0 ? nb : 1) : nslots;
    // every extra slot is a clone of the handle with its own n x n factorisation buffer
    // (lda * npad * 8 bytes: 0.83 GB at n = 10^4); if one cannot be created (out of memory) the
    // batch runs on the slots that exist -- slot 0 is the fit itself, so it always completes
    // (the slots are handles of their own in the registry: held for the whole call, like the handle itself, so that no other
    // thread's stream self-test launches probe kernels between their evaluations)
    std::vector<std::unique_lock<std::recursive_mutex>> slot_locks;
    for (cocons_fit *c : f->slots) slot_locks.emplace_back(c->op_mu);
    while ((int)f->slots.size() < S - 1) {
        cocons_fit *c = clone_for_slot(f, eng_mode);
        if (!c) { (void)hipGetLastError(); break; }
        slot_locks.emplace_back(c->op_mu);
        f->slots.push_back(c);
    }
    const bool engine_saved = f->engine_ok;
    if (!eng_mode) {
        if (S > 1) f->engine_ok = false;
        for (auto c : f->slots) c->engine_ok = false;
    }
    if (S > (int)f->slots.size() + 1) S = (int)f->slots.size() + 1;
    for (int i = 0; i < nb; ++i) { values[i] = NAN; status[i] = -1; }   // never left unwritten
    std::vector<int> pending(S, -1);
    const int tp = 6 * f->p;
    int rc_all = 0;
    auto slot_of = [&](int s) { return s == 0 ? f : f->slots[s - 1]; };
    auto collect = [&](int s) -> int {
        cocons_fit *c = slot_of(s);
        int i = pending[s];
        if (i < 0) return 0;
        pending[s] = -1;
        HIPCHK(hipStreamSynchronize(c->stream));
        int st = info_status(c);
        if (engine_retry(c, st)) {           // hand-off time-out: this evaluation again, on the plain schedule
            if (int rc = enqueue_eval(c, thetas + (size_t)i * tp, means + (size_t)i * f->p, true, nullptr, 0, nullptr, false))
                return rc;
            HIPCHK(hipStreamSynchronize(c->stream));
            st = info_status(c);
        }
        status[i] = st;
        if (st == 0) dense_collect(c, &values[i], nullptr);
        else values[i] = NAN;
        return 0;
    };
    for (int i = 0; i < nb; ++i) {
        int s = i % S;
        if (int rc = collect(s)) { rc_all = rc; break; }
        cocons_fit *c = slot_of(s);
        if (int rc = enqueue_eval(c, thetas + (size_t)i * tp, means + (size_t)i * f->p, true, nullptr, 0, nullptr, false)) {
            rc_all = rc;
            break;
        }
        pending[s] = i;
    }
    for (int s = 0; s < S; ++s)
        if (int rc = collect(s)) rc_all = rc_all ? rc_all : rc;
    f->engine_ok = engine_saved;
    return rc_all;
}

// small dense SPD solve on the host (q x q, q <= COCONS_P_MAX): W = C C^T, returns
// sum(log(diag(C))) and solves W x = b in place for nb right-hand sides.
static int host_spd_solve(int q, std::vector<double> &W, int nb, std::vector<double> &B, double *logdet_half)
{
    double ld = 0;
    for (int j = 0; j < q; ++j) {
        double d = W[j + j * q];
        for (int k = 0; k < j; ++k) d -= W[j + k * q] * W[j + k * q];
        if (!(d > 0)) return j + 1;
        d = std::sqrt(d);
        W[j + j * q] = d;
        ld += std::log(d);
        for (int i = j + 1; i < q; ++i) {
            double s = W[i + j * q];
            for (int k = 0; k < j; ++k) s -= W[i + k * q] * W[j + k * q];
            W[i + j * q] = s / d;
        }
    }
    for (int c = 0; c < nb; ++c) {
        double *b = &B[(size_t)c * q];
        for (int i = 0; i < q; ++i) {
            double s = b[i];
            for (int k = 0; k < i; ++k) s -= W[i + k * q] * b[k];
            b[i] = s / W[i + i * q];
        }
        for (int i = q - 1; i >= 0; --i) {
            double s = b[i];
            for (int k = i + 1; k < q; ++k) s -= W[k + i * q] * b[k];
            b[i] = s / W[i + i * q];
        }
    }
    *logdet_half = ld;
    return 0;
}

// shared tail of Profile / REML: Gram matrix G of [y_1..y_r, Y] (Y = L^-1 Xb) ->
// quad_k = G_kk - g_k' W^-1 g_k with W = Y'Y, g_k = Y'y_k.
int profile_tail(cocons_fit *f, int nxb, double n_eff, bool reml, double *sum_logliks, double *parts)
{
    const int r = f->r, nr = r + nxb;
    const double *G = f->hout + 1;
    std::vector<double> W((size_t)nxb * nxb), Bv((size_t)nxb * r);
    for (int a = 0; a < nxb; ++a)
        for (int b = 0; b < nxb; ++b) W[a + (size_t)b * nxb] = G[(r + a) * nr + (r + b)];
    for (int k = 0; k < r; ++k)
        for (int a = 0; a < nxb; ++a) Bv[(size_t)k * nxb + a] = G[k * nr + (r + a)];
    std::vector<double> g = Bv;
    double ldW = 0;
    if (host_spd_solve(nxb, W, r, Bv, &ldW)) return fail(-4, "X' Sigma^-1 X is not positive definite");
    double logdet = f->hout[0], total = 0.0;
    for (int k = 0; k < r; ++k) {
        double corr = 0;
        for (int a = 0; a < nxb; ++a) corr += g[(size_t)k * nxb + a] * Bv[(size_t)k * nxb + a];
        double quad = G[k * nr + k] - corr;
        total += n_eff * LOG_2PI + 2 * logdet + (reml ? 2 * ldW : 0.0) + quad;
        if (parts) parts[2 + k] = quad;
    }
    if (parts) {
        parts[0] = logdet; parts[1] = ldW;
        // generalised-least-squares coefficients W^-1 Xb' Sigma^-1 zbar, zbar = rowSums(z)/r -- the
        // "Compute Betas" block of cocoOptim's pml/reml branch (R/optim.R:329-341)
        for (int a = 0; a < nxb; ++a) {
            double s = 0;
            for (int k = 0; k < r; ++k) s += Bv[(size_t)k * nxb + a];
            parts[2 + r + a] = s / r;
        }
    }
    *sum_logliks = total;
    return 0;
}

extern "C" int cocons_neg2loglik_profile(cocons_fit *f, const double *theta, double *sum_logliks, double *parts)
{
    FIT_ENTER(f);
    if (int rc = no_taper(f, "cocons_neg2loglik_profile")) return rc;
    if (!theta || !sum_logliks) return fail(-1, "cocons_neg2loglik_profile: null argument");
    if (f->r < 1 || f->q < 1) return fail(-1, "cocons_neg2loglik_profile: fit needs z and x_betas");
    if (int st = run_eval(f, theta, nullptr, false, f->dxb, f->q)) return st;
    return profile_tail(f, f->q, (double)f->n_user, false, sum_logliks, parts);   // R/neg2loglikelihood.R:155-160
}

extern "C" int cocons_neg2loglik_reml(cocons_fit *f, const double *theta, int rank, double *sum_logliks, double *parts)
{
    FIT_ENTER(f);
    if (int rc = no_taper(f, "cocons_neg2loglik_reml")) return rc;
    if (!theta || !sum_logliks) return fail(-1, "cocons_neg2loglik_reml: null argument");
    if (f->r < 1) return fail(-1, "cocons_neg2loglik_reml: fit has no z");
    if (int st = run_eval(f, theta, nullptr, false, f->dX, f->p)) return st;
    return profile_tail(f, f->p, (double)(f->n_user - rank), true, sum_logliks, parts);   // :283-287
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
