// api_shard.hip -- C ABI, several devices: the RCCL loader, the row-block sharded evaluation of the -2 log-likelihood
// (cocons_neg2loglik_dense on a handle with collectives) and the multi-GPU handle cocons_multi_*.
#include <dlfcn.h>
#include <thread>
#include "fit.hpp"

// ---------------------------------------------------------------------------
// RCCL, loaded on first use (dlopen): the library itself has no load-time dependency on it, and a
// process that never shards never touches it.
struct RcclApi {
    void *h;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *);
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int);
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *);
    ncclResult_t (*CommDestroy)(ncclComm_t);
    ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
    ncclResult_t (*GroupStart)();
    ncclResult_t (*GroupEnd)();
    const char *(*GetErrorString)(ncclResult_t);
    ncclResult_t (*CommCount)(const ncclComm_t, int *);
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *);
    ncclResult_t (*CommCuDevice)(const ncclComm_t, int *);
    ncclResult_t (*CommAbort)(ncclComm_t);
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    ncclResult_t (*CommSplit)(ncclComm_t, int, int, ncclComm_t *, void *);      // optional (RCCL >= 2.18): may be null
};

static RcclApi *rccl_api()
{
    static RcclApi api;
    static int state = 0;      // 0 untried, 1 ok, -1 failed
    if (state == 0) {
        state = -1;
        // RCCL must sit on the SAME HIP / HSA runtime this library runs on.  A process may hold two ROCm
        // stacks (PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64 / librccl): a bare
        // dlopen("librccl.so.1") then returns whichever was loaded first, possibly one whose HSA copy was
        // never initialised ("no ROCm-capable device is detected").  So: look beside the libamdhip64 that
        // hipGetDeviceCount resolves to, and only then fall back to the search path.
        std::vector<std::string> names;
        {
            Dl_info di;
            if (dladdr((void *)&hipGetDeviceCount, &di) && di.dli_fname) {
                std::string dir(di.dli_fname);
                size_t slash = dir.rfind('/');
                if (slash != std::string::npos) {
                    dir.resize(slash + 1);
                    names.push_back(dir + "librccl.so.1");
                    names.push_back(dir + "librccl.so");
                }
            }
        }
        names.push_back("librccl.so.1");
        names.push_back("librccl.so");
        names.push_back("/opt/rocm/lib/librccl.so.1");
        void *h = nullptr;
        for (const std::string &nm : names)
            if ((h = dlopen(nm.c_str(), RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) { g_err = std::string("cannot load RCCL: ") + dlerror(); return nullptr; }
        api.h = h;
#define RSYM(field, name) *(void **)(&api.field) = dlsym(h, name); if (!api.field) { g_err = "RCCL symbol missing: " name; return nullptr; }
        RSYM(GetUniqueId, "ncclGetUniqueId")
        RSYM(CommInitRank, "ncclCommInitRank")
        RSYM(CommInitAll, "ncclCommInitAll")
        RSYM(CommDestroy, "ncclCommDestroy")
        RSYM(Broadcast, "ncclBroadcast")
        RSYM(AllReduce, "ncclAllReduce")
        RSYM(AllGather, "ncclAllGather")
        RSYM(GroupStart, "ncclGroupStart")
        RSYM(GroupEnd, "ncclGroupEnd")
        RSYM(GetErrorString, "ncclGetErrorString")
        RSYM(CommCount, "ncclCommCount")
        RSYM(CommUserRank, "ncclCommUserRank")
        RSYM(CommCuDevice, "ncclCommCuDevice")
        RSYM(CommAbort, "ncclCommAbort")
        RSYM(Send, "ncclSend")
        RSYM(Recv, "ncclRecv")
#undef RSYM
        *(void **)(&api.CommSplit) = dlsym(h, "ncclCommSplit");
        state = 1;
    }
    return state == 1 ? &api : nullptr;
}

void rccl_comm_destroy(ncclComm_t c)
{
    RcclApi *R = rccl_api();
    if (R && c) R->CommDestroy(c);
}

#define NCCLCHK(expr)                                                             \
    do {                                                                          \
        ncclResult_t r__ = (expr);                                                \
        if (r__ != ncclSuccess) {                                                 \
            char b__[512];                                                        \
            snprintf(b__, sizeof b__, "%s failed: %s (%s:%d)", #expr,             \
                     rccl_api() ? rccl_api()->GetErrorString(r__) : "?", __FILE__, __LINE__); \
            g_err = b__;                                                          \
            return -200 - (int)r__;                                               \
        }                                                                         \
    } while (0)

// ---------------------------------------------------------------------------
// Sharded evaluation: Sigma ROW-BLOCK partitioned over the ranks.  Block b = the 256 rows of the
// tiles 2b, 2b+1; blocks are dealt in GROUPS of G consecutive blocks, owner(b) = (b / G) mod world (COCONS_SHARD_GROUP,
// default 4).  A rank assembles, solves and updates ITS rows of every column; per 256-column block k:
//   owner(k)     factors the 256 x 256 diagonal block (all earlier updates of its rows are local)      [0.5 MB]
//   broadcast    L_kk (+ the 4x4-inverse operands of its sixteen 16 x 16 diagonal blocks) from owner(k)
//   every rank   solves ITS rows of the panel, X = B L_kk^-T, in place (solve | in-panel update | solve, row-filtered)
//   owner(k+1)   updates its diagonal block (k+1,k+1) with its own rows of X -- local data -- factors it and starts the
//                broadcast of L_(k+1,k+1): the chain diagonal block -> diagonal block never waits for the bulk exchange
//   all-gather   of the solved rows, packed by owner (every rank contributes B_k / world; on point-to-point links every
//                link then carries B_k / world instead of the whole panel a broadcast would push through each)
//   every rank   updates ITS rows of the trailing matrix with the gathered panel (the column side of a tile belongs to
//                another rank in general: both operands come from the gathered buffer through a per-tile offset table)
// The right-hand sides are rows under the matrix = part of the last block's row block: their owner ends up with
// L^-1 (z - X beta) in place and every rank with every L_kk, so the reductions need no data exchange beyond the usual
// all-reduce of (1 + r^2) doubles and the failing minor.
static const int PT = 2;     // tiles per block

static int shard_group()
{
    static const int g = [] {
        const char *e = getenv("COCONS_SHARD_GROUP");
        int v = e ? atoi(e) : 4;
        return v < 1 ? 1 : v;
    }();
    return g;
}
static inline int shard_owner(int b, int world) { return (b / shard_group()) % world; }

extern "C" int cocons_shard_block_owner(int b, int world) { return (b < 0 || world < 1) ? -1 : shard_owner(b, world); }
extern "C" int cocons_shard_num_blocks(cocons_fit *f) { return f ? (f->nt + PT - 1) / PT : -1; }

static const size_t LKK_DOUBLES = (size_t)PT * TILE * PT * TILE + 2 * 2048;     // diagonal block + Q operands of its two tiles

static void shard_make_plan(ShardPlan &P, int nt, int mt, int world, int group)
{
    P.nt = nt; P.mt = mt; P.world = world; P.group = group;
    const int nb = (nt + PT - 1) / PT, T64 = 2 * mt;
    P.tlo.assign(nb, 0); P.ncols.assign(nb, 0); P.srows.assign(nb, 0);
    P.pmap.assign((size_t)nb * T64, -1); P.cnt.assign((size_t)nb * world, 0);
    P.max_elems = 0;
    for (int k = 0; k < nb; ++k) {
        const int w = (nt - k * PT) < PT ? (nt - k * PT) : PT;
        P.ncols[k] = w * TILE;
        P.tlo[k] = 2 * (k * PT + w);
        int *c = &P.cnt[(size_t)k * world];
        for (int ti = P.tlo[k]; ti < T64; ++ti) c[((ti / 4) / group) % world]++;
        int mx = 0;
        for (int r = 0; r < world; ++r) mx = c[r] > mx ? c[r] : mx;
        P.srows[k] = 64LL * mx;
        std::vector<int> pos(world, 0);
        for (int ti = P.tlo[k]; ti < T64; ++ti) {
            const int o = ((ti / 4) / group) % world;
            P.pmap[(size_t)k * T64 + ti] = (int)((long long)o * P.srows[k] * P.ncols[k] + 64LL * pos[o]++);
        }
        const size_t el = (size_t)world * (size_t)P.srows[k] * (size_t)P.ncols[k];
        if (el > P.max_elems) P.max_elems = el;
    }
}

// (the events only: the buffers go with the state, cocons_fit_destroy)
void shard_events_destroy(ShardState *S)
{
    if (!S) return;
    if (S->ev_main_L) hipEventDestroy(S->ev_main_L);
    for (int b = 0; b < 2; ++b) {
        if (S->ev_comm_L[b]) hipEventDestroy(S->ev_comm_L[b]);
        if (S->ev_main_X[b]) hipEventDestroy(S->ev_main_X[b]);
        if (S->ev_comm_X[b]) hipEventDestroy(S->ev_comm_X[b]);
        if (S->ev_main_U[b]) hipEventDestroy(S->ev_main_U[b]);
    }
}

extern "C" int cocons_fit_world(cocons_fit *f) { return (f && f->coll_kind) ? f->coll_world : 1; }

// buffers, plan and events of the sharded evaluation on this handle (world ranks)
static int shard_prepare(cocons_fit *f, int rank, int world)
{
    f->rank = rank; f->world = world; f->nrhs_cur = f->r;
    if (int rc = fit_alloc_matrix(f, f->r)) return rc;
    const int mt = f->nt + f->rhs_act / TILE;
    if (!f->shard) f->shard.reset(new ShardState());
    ShardState *S = f->shard.get();
    if (S->plan.nt != f->nt || S->plan.mt != mt || S->plan.world != world || S->plan.group != shard_group()) {
        HIPCHK(hipStreamSynchronize(f->stream));
        if (f->cstream) HIPCHK(hipStreamSynchronize(f->cstream));
        shard_make_plan(S->plan, f->nt, mt, world, shard_group());
        HIPCHK(S->d_pmap.alloc(S->plan.pmap.size()));      // (both streams that use the old map were drained just above)
        HIPCHK(hipMemcpyAsync(S->d_pmap, S->plan.pmap.data(), S->plan.pmap.size() * sizeof(int), hipMemcpyHostToDevice, f->stream));
        HIPCHK(hipStreamSynchronize(f->stream));
        for (int b = 0; b < 2; ++b)      // (zeroed when new: slot padding is exchanged too, no NaN patterns)
            HIPCHK(f->xbuf[b].reserve(S->plan.max_elems, f->stream, f->stream2, 0));
    }
    for (int b = 0; b < 2; ++b) {
        if (!S->lkk[b]) HIPCHK(S->lkk[b].alloc(LKK_DOUBLES));
        if (!S->ev_comm_L[b]) HIPCHK(hipEventCreateWithFlags(&S->ev_comm_L[b], hipEventDisableTiming));
        if (!S->ev_main_X[b]) HIPCHK(hipEventCreateWithFlags(&S->ev_main_X[b], hipEventDisableTiming));
        if (!S->ev_comm_X[b]) HIPCHK(hipEventCreateWithFlags(&S->ev_comm_X[b], hipEventDisableTiming));
        if (!S->ev_main_U[b]) HIPCHK(hipEventCreateWithFlags(&S->ev_main_U[b], hipEventDisableTiming));
        S->unpacked[b] = false;
    }
    if (!S->ev_main_L) HIPCHK(hipEventCreateWithFlags(&S->ev_main_L, hipEventDisableTiming));
    return 0;
}

// assemble this rank's rows of Sigma (lower triangle) and, on their owner, the right-hand-side rows under the matrix
static int shard_begin(cocons_fit *f, const double *theta, const double *mean, int rank, int world)
{
    if (int rc = no_taper(f, "sharded evaluation")) return rc;
    if (f->r < 1) return fail(-1, "sharded evaluation: fit has no z");
    if (int rc = shard_prepare(f, rank, world)) return rc;
    if (int rc = reset_info(f)) return rc;
    if (engine_enabled()) {
        if (int rc = flags_reset(f, f->nt)) return rc;     // (the words shard_factor_diag's engine launches read and raise)
        if (tun().engine_pair)
            if (int rc = mbox_reset(f, f->nt)) return rc;  // (... and the mailboxes of their pair mode)
    }
    ThetaVecs tv;
    make_theta_vecs(theta, f->p, tv);
    ModeSel ms = select_mode(theta, f->p, f->smooth_limits, 0);
    launch_loc_params(loc_args(f->n, f->p, f->dX, f->dlocs, f->dloc, f->npad, tv, ms.smooth_kind, f->smooth_limits),
                      f->stream);                      // (replicated: O(n p))
    PairArgs pa;
    pa.n = f->n; pa.m = f->n; pa.rows = f->dloc; pa.cols = f->dloc;
    pa.stride = f->npad; pa.stride_rows = f->npad; pa.out = f->dA; pa.ld = f->lda;
    pa.nrows_out = f->npad; pa.ncols_out = f->npad;
    pa.bj0 = f->pad0 / 64; pa.H = 0; pa.blocked = 0;
    pa.gr = ms.gr; pa.nu_fixed = ms.nu_fixed;
    pa.pad_diag = f->nslot > 0 ? 1e300 : 1.0;
    pa.own_world = world; pa.own_rank = rank; pa.own_group = shard_group();
    launch_pair_sym(ms.mode, false, pa, f->stream);
    const int mt = f->nt + f->rhs_act / TILE;
    if (shard_owner(f->nt / PT, world) == rank)         // the rows under the matrix belong to the block of tile row nt
        assemble_rhs(f, mean, true, nullptr, 0, 0, f->npad);
    launch_front_identity(f->dA, f->lda, f->pad0, mt * TILE, f->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// the owner factors the diagonal block of block k in place and packs it (with the Q operands) for the broadcast
static int shard_factor_diag(cocons_fit *f, int k)
{
    ShardState *S = f->shard.get();
    const int t = k * PT, w = S->plan.ncols[k] / TILE;
    hipStream_t s = f->stream;
    double *A = f->dA, *q0 = f->dinv, *q1 = f->dinv + 2048;
    if (engine_enabled() && f->flags_cap >= t + w) {
        // the whole block in ONE launch of the diagonal-block engine (tile, strip solve, tile update, tile: what the four
        // launches below do, without their three boundaries -- this block is the chain every rank waits for, section 5): its
        // input words are raised beforehand, so it never waits, and it leaves behind the block of its second tile
        const HandoffWords hw = handoff_words(f);
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(hw.in + t), 7, (size_t)w, s));
        EngineLaunch e;
        e.A = A; e.lda = f->lda; e.t0 = t; e.nt = t + w; e.dinv = f->dinv; e.info = f->dinfo;
        e.in = hw.in; e.out = hw.out; e.xr = hw.xr; e.abort_word = hw.abort; e.alive = hw.alive;
        // (pair mode: its two workgroups side by side -- the second tile's factorisation starts ~6 us behind the first's end
        // instead of behind the strip solve and the tile update: 78 -> ~56 us for the block)
        if (w == 2 && tun().engine_pair && tile_mbox(f, f->nt + 1)) e.mbox = tile_mbox(f, 0);
        launch_potrf_engine(e, s);
    } else {
        launch_potrf_tile(A, f->lda, t * TILE, q0, f->dinfo, s);
        if (w == 2) {
            TrsmLaunch l;
            l.A = A; l.lda = f->lda; l.c0 = t * TILE; l.rows.r0 = (t + 1) * TILE; l.rows.r1 = (t + 2) * TILE; l.dinv = q0;
            launch_trsm_tile(l, s);
            UpdateLaunch u;
            u.C = A; u.ldc = f->lda; u.panel_in_c(t * TILE); u.K = TILE; u.ti0 = u.tj0 = t + 1; u.ti1 = u.tj1 = t + 2; u.lower_only = true;
            launch_update(u, s);
            launch_potrf_tile(A, f->lda, (t + 1) * TILE, q1, f->dinfo, s);
        }
    }
    double *L = S->lkk[k & 1];
    HIPCHK(hipMemcpy2DAsync(L, (size_t)PT * TILE * sizeof(double), A + (size_t)t * TILE + (size_t)t * TILE * f->lda,
                            f->lda * sizeof(double), (size_t)w * TILE * sizeof(double), (size_t)w * TILE,
                            hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(L + (size_t)PT * TILE * PT * TILE, f->dinv, 2 * 2048 * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipEventRecord(S->ev_main_L, s));
    return 0;
}

// ---- collectives: RCCL on the communication stream, or the caller's transport ----
// COCONS_SHARD_COMM2 (default 1): the broadcasts of the factored diagonal blocks get a stream -- and, under RCCL, a
// communicator -- of their own, so that the chain from one diagonal block to the next never queues behind the bulk exchange
// COCONS_SHARD_COMM2=1: the broadcasts of the factored diagonal blocks get a stream -- and under RCCL a communicator
// (ncclCommSplit) -- of their own.  OPT-IN since round 6 (the advisor's finding): two RCCL communicators working side by side,
// one of them with receivers that sit resident until their owner has factored, have never run with more than one rank (a GPU
// box of this pool has one GPU) -- default: one communicator, one communication stream, the broadcast still issued IN FRONT
// of the all-gather.  tests/test_gpu_configs.py::test_native_sharded_rccl_two_gpus runs both forms where two devices exist.
static bool shard_comm2()
{
    static const int v = [] { const char *e = getenv("COCONS_SHARD_COMM2"); return e ? atoi(e) : 0; }();
    return v != 0;
}

static int coll_prepare(cocons_fit *f)
{
    if (!f->cstream) HIPCHK(hipStreamCreateWithFlags(&f->cstream, hipStreamNonBlocking));
    if (!f->cstream_l) {
        // RCCL serialises the operations of ONE communicator whatever streams they are given: a second stream only helps
        // with a second communicator (split off by the caller of this function); a caller-provided transport has no such rule
        const bool own = shard_comm2() && (f->coll_kind == 2 || (f->coll_kind == 1 && f->comm_l && f->comm_l != f->comm));
        if (own) HIPCHK(hipStreamCreateWithFlags(&f->cstream_l, hipStreamNonBlocking));
        else f->cstream_l = f->cstream;
    }
    if (!f->dcoll) HIPCHK(f->dcoll.alloc((size_t)(2 + (COCONS_P_MAX + f->r) * (COCONS_P_MAX + f->r))));
    return 0;
}

extern "C" int cocons_comm_unique_id(void *id_out)
{
    if (!id_out) return fail(-1, "cocons_comm_unique_id: null argument");
    RcclApi *R = rccl_api();
    if (!R) return -1;
    ncclUniqueId id;
    NCCLCHK(R->GetUniqueId(&id));
    static_assert(sizeof(ncclUniqueId) == COCONS_UNIQUE_ID_BYTES, "unique id size");
    memcpy(id_out, &id, sizeof id);
    return 0;
}

extern "C" int cocons_fit_comm_init(cocons_fit *f, int nranks, int rank, const void *idp)
{
    FIT_ENTER(f);
    if (int rc = no_taper(f, "cocons_fit_comm_init")) return rc;
    if (!idp || nranks < 1 || rank < 0 || rank >= nranks) return fail(-1, "cocons_fit_comm_init: bad argument");
    if (f->coll_kind) return fail(-1, "cocons_fit_comm_init: the fit already has collectives");
    RcclApi *R = rccl_api();
    if (!R) return -1;
    ncclUniqueId id;
    memcpy(&id, idp, sizeof id);
    // RCCL polls hipGetLastError() after its own launches: a stale (already handled) error code of this
    // process must not be mistaken for a failure of the communicator set-up
    (void)hipGetLastError();
    NCCLCHK(R->CommInitRank(&f->comm, nranks, id, rank));
    f->comm_own = true;
    f->coll_kind = 1; f->coll_rank = rank; f->coll_world = nranks;
    // a second communicator over the same ranks for the small broadcasts on the chain (collective call: every rank is here).
    // Not available / refused: the broadcasts share the one communicator and its stream.
    f->comm_l = nullptr; f->comm_l_own = false;
    if (shard_comm2() && R->CommSplit) {
        ncclComm_t c2 = nullptr;
        if (R->CommSplit(f->comm, 0, rank, &c2, nullptr) == ncclSuccess && c2) { f->comm_l = c2; f->comm_l_own = true; }
        else (void)hipGetLastError();
    }
    return coll_prepare(f);
}

extern "C" int cocons_fit_set_collectives(cocons_fit *f, int rank, int world, cocons_bcast_fn bcast,
                                          cocons_allreduce_fn allreduce, void *user)
{
    FIT_ENTER(f);
    if (int rc = no_taper(f, "cocons_fit_set_collectives")) return rc;
    if (world < 1 || rank < 0 || rank >= world || !bcast || !allreduce)
        return fail(-1, "cocons_fit_set_collectives: bad argument");
    if (f->coll_kind == 1) return fail(-1, "cocons_fit_set_collectives: the fit already has an RCCL communicator");
    f->coll_kind = 2; f->coll_rank = rank; f->coll_world = world;
    f->cb_bcast = bcast; f->cb_allreduce = allreduce; f->cb_user = user;
    return coll_prepare(f);
}

extern "C" int cocons_fit_set_allgather(cocons_fit *f, cocons_allgather_fn allgather)
{
    FIT_ENTER(f);
    if (f->coll_kind != 2) return fail(-1, "cocons_fit_set_allgather: call cocons_fit_set_collectives first");
    f->cb_allgather = allgather;
    return 0;
}

// broadcast of L_kk (packed by shard_factor_diag on its owner) on the communication stream
static int coll_bcast_L(cocons_fit *f, int k, bool in_group)
{
    ShardState *S = f->shard.get();
    const int b = k & 1, owner = shard_owner(k, f->coll_world);
    hipStream_t cs = f->cstream_l;
    // the owner's copy is packed on its main stream; a receiver's buffer was last read by the unpack of L_(k-2) on ITS main
    // stream (the broadcasts have a stream of their own since round 5: nothing else orders the two)
    if (f->coll_rank == owner) HIPCHK(hipStreamWaitEvent(cs, S->ev_main_L, 0));
    else if (S->unpacked[b]) HIPCHK(hipStreamWaitEvent(cs, S->ev_main_U[b], 0));
    if (f->coll_kind == 1) {
        RcclApi *R = rccl_api();
        NCCLCHK(R->Broadcast(S->lkk[b], S->lkk[b], LKK_DOUBLES, ncclDouble, owner, f->comm_l ? f->comm_l : f->comm, cs));
        if (!in_group) HIPCHK(hipEventRecord(S->ev_comm_L[b], cs));
    } else {
        if (f->cb_bcast(f->cb_user, S->lkk[b], (long long)(LKK_DOUBLES * sizeof(double)), owner, (void *)cs) != 0)
            return fail(-6, "caller-provided broadcast failed");
        HIPCHK(hipEventRecord(S->ev_comm_L[b], cs));
    }
    return 0;
}

// all-gather of the solved rows of panel k: every rank's slot of the owner-packed buffer
static int coll_allgather_X(cocons_fit *f, int k, bool in_group)
{
    ShardState *S = f->shard.get();
    const int b = k & 1;
    const size_t cnt = (size_t)S->plan.srows[k] * (size_t)S->plan.ncols[k];
    HIPCHK(hipStreamWaitEvent(f->cstream, S->ev_main_X[b], 0));
    if (f->coll_kind == 1) {
        RcclApi *R = rccl_api();
        NCCLCHK(R->AllGather(f->xbuf[b] + (size_t)f->coll_rank * cnt, f->xbuf[b], cnt, ncclDouble, f->comm, f->cstream));
        if (!in_group) HIPCHK(hipEventRecord(S->ev_comm_X[b], f->cstream));
    } else {
        if (!f->cb_allgather) return fail(-6, "caller-provided transport has no all-gather (cocons_fit_set_allgather)");
        if (f->cb_allgather(f->cb_user, f->xbuf[b], (long long)(cnt * sizeof(double)), (void *)f->cstream) != 0)
            return fail(-6, "caller-provided all-gather failed");
        HIPCHK(hipEventRecord(S->ev_comm_X[b], f->cstream));
    }
    return 0;
}

// One rank's part of step k up to the exchange of the solved rows:
//   L_kk in place (received: unpacked) | solve the own rows below | [owner of block k+1] diagonal block k+1 updated with
//   its own rows, factored, packed | own rows packed into the gathered buffer
static int shard_step_pre(cocons_fit *f, int k, int nb)
{
    ShardState *S = f->shard.get();
    const ShardPlan &P = S->plan;
    const int W = f->coll_world, rank = f->coll_rank, G = shard_group();
    const int t = k * PT, w = P.ncols[k] / TILE, tn = t + w;           // tn: first tile below / right of the block
    const int mt = P.mt;
    hipStream_t s = f->stream;
    double *A = f->dA;
    if (rank != shard_owner(k, W)) {
        HIPCHK(hipStreamWaitEvent(s, S->ev_comm_L[k & 1], 0));
        const double *L = S->lkk[k & 1];
        HIPCHK(hipMemcpy2DAsync(A + (size_t)t * TILE + (size_t)t * TILE * f->lda, f->lda * sizeof(double), L,
                                (size_t)PT * TILE * sizeof(double), (size_t)w * TILE * sizeof(double), (size_t)w * TILE,
                                hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(f->dinv, L + (size_t)PT * TILE * PT * TILE, 2 * 2048 * sizeof(double), hipMemcpyDeviceToDevice, s));
        HIPCHK(hipEventRecord(S->ev_main_U[k & 1], s));
        S->unpacked[k & 1] = true;
    }
    if (tn >= mt) return 0;                                            // nothing below the block
    if (P.cnt[(size_t)k * W + rank] > 0) {
        TrsmLaunch l;
        l.A = A; l.lda = f->lda; l.c0 = t * TILE; l.rows.r0 = tn * TILE; l.rows.r1 = mt * TILE; l.dinv = f->dinv; l.own_world = W; l.own_rank = rank; l.own_group = G;
        launch_trsm_tile(l, s);
        if (w == 2) {
            UpdateLaunch u;
            u.C = A; u.ldc = f->lda; u.P = A + (size_t)t * TILE * f->lda; u.ldp = f->lda;      // (kblk stays 0: a dense buffer)
            u.K = TILE; u.ti0 = tn; u.ti1 = mt; u.tj0 = t + 1; u.tj1 = t + 2; u.group = G; u.world = W; u.rank = rank;
            launch_update(u, s);
            l.c0 = (t + 1) * TILE; l.dinv = f->dinv + 2048;
            launch_trsm_tile(l, s);
        }
    }
    if (tn >= P.nt) return 0;                                          // last block: only right-hand-side rows below, no exchange
    if (k + 1 < nb && rank == shard_owner(k + 1, W)) {
        const int w1 = P.ncols[k + 1] / TILE;
        UpdateLaunch u;                                                                      // own rows of X: local
        u.C = A; u.ldc = f->lda; u.panel_in_c(t * TILE); u.K = w * TILE; u.ti0 = u.tj0 = tn; u.ti1 = u.tj1 = tn + w1; u.lower_only = true;
        launch_update(u, s);
        if (int rc = shard_factor_diag(f, k + 1)) return rc;
    }
    const long long slot = (long long)P.srows[k] * P.ncols[k];
    launch_pack_rows(A, f->lda, t * TILE, w * TILE, f->xbuf[k & 1], (size_t)P.srows[k], S->d_pmap + (size_t)k * 2 * mt, P.tlo[k],
                     2 * mt, slot * rank, slot * (rank + 1), s);
    HIPCHK(hipEventRecord(S->ev_main_X[k & 1], s));
    HIPCHK(hipGetLastError());
    return 0;
}

// ... and behind it: the own rows of the trailing matrix updated with the gathered panel
static int shard_step_post(cocons_fit *f, int k, int nb)
{
    ShardState *S = f->shard.get();
    const ShardPlan &P = S->plan;
    const int W = f->coll_world, rank = f->coll_rank, G = shard_group();
    const int t = k * PT, w = P.ncols[k] / TILE, tn = t + w;
    if (tn >= P.nt) return 0;
    HIPCHK(hipStreamWaitEvent(f->stream, S->ev_comm_X[k & 1], 0));
    if (P.cnt[(size_t)k * W + rank] > 0) {
        // (the owner of block k + 1 has updated that diagonal block with its own rows already: shard_step_pre)
        const bool ahead = k + 1 < nb && rank == shard_owner(k + 1, W);
        UpdateLaunch u;
        u.C = f->dA; u.ldc = f->lda; u.P = f->xbuf[k & 1]; u.ldp = (size_t)P.srows[k]; u.K = w * TILE; u.ti0 = tn; u.ti1 = P.mt; u.tj0 = tn; u.tj1 = P.nt; u.lower_only = true;
        u.group = G; u.world = W; u.rank = rank; u.pmap = S->d_pmap + (size_t)k * 2 * P.mt;
        if (ahead) { u.skip_lo = 2 * tn; u.skip_hi = 2 * (tn + P.ncols[k + 1] / TILE); }
        launch_update(u, f->stream);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// the reductions: the owner of the right-hand-side rows has L^-1 rhs in place and -- like everybody -- every L_kk
static int shard_finish(cocons_fit *f, double *partial, int *info)
{
    const int nr = f->nrhs_cur, len = 1 + nr * nr;
    for (int i = 0; i < len; ++i) partial[i] = 0.0;
    const bool mine = shard_owner(f->nt / PT, f->coll_world) == f->coll_rank;
    if (mine) {
        launch_finalize(f->dA, f->lda, f->n, f->npad, nr, f->dout, f->stream);
        HIPCHK(hipMemcpyAsync(f->hout, f->dout, (size_t)len * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    }
    HIPCHK(hipMemcpyAsync(f->hinfo, f->dinfo, 2 * sizeof(int), hipMemcpyDeviceToHost, f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
    if (mine) for (int i = 0; i < len; ++i) partial[i] = f->hout[i];
    if (info) *info = *f->hinfo;
    return 0;
}

static int sharded_eval_impl(cocons_fit *f, const double *theta, const double *mean, double *sum_logliks, double *parts);

// A rank that fails in the middle of the schedule (HIP or RCCL error: status < 0) must not leave its peers blocked in
// the next collective until a watchdog fires: it aborts its communicator, which makes the peers' pending RCCL calls
// fail, and the handle refuses further sharded evaluations.  (status > 0 -- Sigma not positive definite -- is an
// ordinary result that every rank reaches together.)
int sharded_eval(cocons_fit *f, const double *theta, const double *mean, double *sum_logliks, double *parts)
{
    const int rc = sharded_eval_impl(f, theta, mean, sum_logliks, parts);
    if (rc < 0 && f->coll_kind == 1 && f->comm && f->coll_world > 1) {
        const std::string keep = g_err;
        RcclApi *R = rccl_api();
        if (R && f->comm_l && f->comm_l != f->comm) (void)R->CommAbort(f->comm_l);
        if (R) (void)R->CommAbort(f->comm);
        f->comm = nullptr; f->comm_l = nullptr;
        f->coll_kind = -1;                      // poisoned: see cocons_neg2loglik_dense
        g_err = keep + " (communicator aborted)";
    }
    return rc;
}

static int shard_collect(cocons_fit *f, std::vector<double> &part, double minfo, double *sum_logliks, double *parts)
{
    const int nr = f->r;
    if (minfo != (double)0x7f7f7f7f) {
        int st = (int)minfo;
        st -= f->pad0;
        if (st < 1) st = 1;
        if (st > f->n_user) st = f->n_user;
        g_err = "leading minor not positive";
        return st;
    }
    double total = 0.0;
    for (int c = 0; c < nr; ++c) {
        const double quad = part[1 + c * nr + c];
        total += f->n_user * LOG_2PI + 2 * part[0] + quad;
        if (parts) parts[1 + c] = quad;
    }
    if (parts) parts[0] = part[0];
    *sum_logliks = total;
    return 0;
}

static int sharded_eval_impl(cocons_fit *f, const double *theta, const double *mean, double *sum_logliks, double *parts)
{
    const int rank = f->coll_rank, world = f->coll_world;
    if (int rc = shard_begin(f, theta, mean, rank, world)) return rc;
    const int nb = cocons_shard_num_blocks(f);
    if (rank == shard_owner(0, world))
        if (int rc = shard_factor_diag(f, 0)) return rc;
    if (int rc = coll_bcast_L(f, 0, false)) return rc;
    for (int k = 0; k < nb; ++k) {
        if (int rc = shard_step_pre(f, k, nb)) return rc;
        // (the broadcast of the NEXT diagonal block is issued in FRONT of this block's bulk exchange, in the same order on every
        // rank: it depends on nothing but the owner's own rows -- collectives issued earlier --, so whether the two share a
        // stream, a hardware queue or neither, the chain diagonal block -> diagonal block never waits for an all-gather.
        // Until round 4 it was issued behind the all-gather on the one communication stream, and waited for it.)
        const bool exchange = k * PT + f->shard->plan.ncols[k] / TILE < f->nt;
        if (k + 1 < nb) if (int rc = coll_bcast_L(f, k + 1, false)) return rc;
        if (exchange) if (int rc = coll_allgather_X(f, k, false)) return rc;
        if (int rc = shard_step_post(f, k, nb)) return rc;
    }
    const int nr = f->r, len = 1 + nr * nr;
    std::vector<double> part(len + 1);
    int info = 0;
    if (int rc = shard_finish(f, part.data(), &info)) return rc;
    HIPCHK(hipStreamSynchronize(f->cstream));
    if (f->cstream_l != f->cstream) HIPCHK(hipStreamSynchronize(f->cstream_l));
    double minfo = (double)info;                       // 0x7f7f7f7f = no failing minor (exact in a double)
    if (world > 1) {
        if (f->coll_kind == 1) {
            RcclApi *R = rccl_api();
            HIPCHK(hipMemcpyAsync(f->dcoll, part.data(), (size_t)len * sizeof(double), hipMemcpyHostToDevice, f->cstream));
            HIPCHK(hipMemcpyAsync(f->dcoll + len, &minfo, sizeof(double), hipMemcpyHostToDevice, f->cstream));
            NCCLCHK(R->AllReduce(f->dcoll, f->dcoll, (size_t)len, ncclDouble, ncclSum, f->comm, f->cstream));
            NCCLCHK(R->AllReduce(f->dcoll + len, f->dcoll + len, 1, ncclDouble, ncclMin, f->comm, f->cstream));
            HIPCHK(hipMemcpyAsync(part.data(), f->dcoll, (size_t)(len + 1) * sizeof(double), hipMemcpyDeviceToHost, f->cstream));
            HIPCHK(hipStreamSynchronize(f->cstream));
            minfo = part[len];
        } else {
            if (f->cb_allreduce(f->cb_user, part.data(), len, 0) != 0 || f->cb_allreduce(f->cb_user, &minfo, 1, 1) != 0)
                return fail(-6, "caller-provided all-reduce failed");
        }
    }
    return shard_collect(f, part, minfo, sum_logliks, parts);
}

// ---- one process, several GPUs ---------------------------------------------------------------------
struct cocons_multi {
    int ndev;
    std::vector<cocons_fit *> fits;
    std::vector<ncclComm_t> comms;
};

extern "C" void cocons_multi_destroy(cocons_multi *m)
{
    if (!m) return;
    for (auto f : m->fits) cocons_fit_destroy(f);          // (communicators are not owned by the fits)
    for (auto c : m->comms) rccl_comm_destroy(c);
    delete m;
}

extern "C" cocons_multi *cocons_multi_create(int n, int p, int r, const double *locs, const double *X, const double *z,
                                             const double *smooth_limits, int ndev, const int *devices)
{
    if (ndev < 1 || !devices || r < 1) { fail(-1, "cocons_multi_create: bad argument"); return nullptr; }
    RcclApi *R = rccl_api();
    if (!R) return nullptr;
    cocons_multi *m = new cocons_multi();
    m->ndev = ndev;
    for (int d = 0; d < ndev; ++d) {
        cocons_fit *f = cocons_fit_create(n, p, r, 0, locs, X, z, nullptr, smooth_limits, devices[d]);
        if (!f) { cocons_multi_destroy(m); return nullptr; }
        m->fits.push_back(f);
    }
    // a device listed twice (tests on a one-GPU box) cannot carry an RCCL communicator: such a handle serves
    // the entry points that need no collective (cocons_multi_predict_dense) and refuses the sharded objective
    bool distinct = true;
    for (int a = 0; a < ndev; ++a)
        for (int b = a + 1; b < ndev; ++b)
            if (devices[a] == devices[b]) distinct = false;
    if (!distinct) return m;
    m->comms.assign(ndev, nullptr);
    (void)hipGetLastError();
    ncclResult_t nr = R->CommInitAll(m->comms.data(), ndev, devices);
    if (nr != ncclSuccess) {
        fail(-200, "ncclCommInitAll: %s", R->GetErrorString(nr));
        m->comms.clear();
        cocons_multi_destroy(m);
        return nullptr;
    }
    // second communicators for the chain's broadcasts (one collective call per local rank, inside a group)
    std::vector<ncclComm_t> c2(ndev, nullptr);
    bool split_ok = shard_comm2() && R->CommSplit != nullptr;
    if (split_ok) {
        split_ok = R->GroupStart() == ncclSuccess;
        for (int d = 0; d < ndev && split_ok; ++d) {
            hipSetDevice(devices[d]);
            if (R->CommSplit(m->comms[d], 0, d, &c2[d], nullptr) != ncclSuccess) split_ok = false;
        }
        if (R->GroupEnd() != ncclSuccess) split_ok = false;
        for (int d = 0; d < ndev; ++d) if (!c2[d]) split_ok = false;
        if (!split_ok) { for (auto c : c2) if (c) rccl_comm_destroy(c); (void)hipGetLastError(); }
    }
    for (int d = 0; d < ndev; ++d) {
        cocons_fit *f = m->fits[d];
        f->comm = m->comms[d]; f->comm_own = false;
        f->comm_l = split_ok ? c2[d] : nullptr; f->comm_l_own = split_ok;      // (destroyed with the fit)
        f->coll_kind = 1; f->coll_rank = d; f->coll_world = ndev;
        if (fit_check(f) != 0 || coll_prepare(f) != 0) { cocons_multi_destroy(m); return nullptr; }
    }
    return m;
}

// The calling thread drives every device: each schedule step is enqueued on all devices in turn (all calls
// are asynchronous), the per-panel broadcasts of the ranks are issued inside one RCCL group.
extern "C" int cocons_multi_neg2loglik_dense(cocons_multi *m, const double *theta, const double *mean,
                                             double *sum_logliks, double *parts)
{
    if (!m || !theta || !mean || !sum_logliks) return fail(-1, "cocons_multi_neg2loglik_dense: null argument");
    if (m->comms.empty()) return fail(-1, "cocons_multi_neg2loglik_dense: this handle has no communicator (a device is listed twice)");
    RcclApi *R = rccl_api();
    if (!R) return -1;
    const int W = m->ndev;
    std::vector<std::unique_lock<std::recursive_mutex>> op_locks;       // (this entry point drives the ranks' handles directly)
    for (int d = 0; d < W; ++d) op_locks.emplace_back(m->fits[d]->op_mu);
    for (int d = 0; d < W; ++d) {
        if (int rc = fit_check(m->fits[d])) return rc;
        if (int rc = shard_begin(m->fits[d], theta, mean, d, W)) return rc;
    }
    const int nb = cocons_shard_num_blocks(m->fits[0]);
    auto grouped = [&](int k, bool gather) -> int {
        NCCLCHK(R->GroupStart());
        int rc_in = 0;
        std::string err_in;
        for (int d = 0; d < W && rc_in == 0; ++d) {
            rc_in = fit_check(m->fits[d]);
            if (rc_in == 0) rc_in = gather ? coll_allgather_X(m->fits[d], k, true) : coll_bcast_L(m->fits[d], k, true);
            if (rc_in != 0) err_in = g_err;
        }
        // the group is closed on EVERY path: an error between ncclGroupStart and ncclGroupEnd used to leave it open, and every
        // later RCCL call of the thread inside it
        const ncclResult_t ge = R->GroupEnd();
        if (rc_in != 0) { g_err = err_in; return rc_in; }
        NCCLCHK(ge);
        for (int d = 0; d < W; ++d) {
            if (int rc = fit_check(m->fits[d])) return rc;
            ShardState *S = m->fits[d]->shard.get();
            HIPCHK(hipEventRecord(gather ? S->ev_comm_X[k & 1] : S->ev_comm_L[k & 1],
                                  gather ? m->fits[d]->cstream : m->fits[d]->cstream_l));
        }
        return 0;
    };
    {
        cocons_fit *f0 = m->fits[shard_owner(0, W)];
        if (int rc = fit_check(f0)) return rc;
        if (int rc = shard_factor_diag(f0, 0)) return rc;
    }
    if (int rc = grouped(0, false)) return rc;
    for (int k = 0; k < nb; ++k) {
        for (int d = 0; d < W; ++d) {
            if (int rc = fit_check(m->fits[d])) return rc;
            if (int rc = shard_step_pre(m->fits[d], k, nb)) return rc;
        }
        const bool exchange = k * PT + m->fits[0]->shard->plan.ncols[k] / TILE < m->fits[0]->nt;
        if (k + 1 < nb) if (int rc = grouped(k + 1, false)) return rc;     // (in front of the bulk exchange: see sharded_eval_impl)
        if (exchange) if (int rc = grouped(k, true)) return rc;
        for (int d = 0; d < W; ++d) {
            if (int rc = fit_check(m->fits[d])) return rc;
            if (int rc = shard_step_post(m->fits[d], k, nb)) return rc;
        }
    }
    cocons_fit *f0 = m->fits[0];
    const int nr = f0->r, len = 1 + nr * nr;
    std::vector<double> tot(len, 0.0), part(len);
    int info_min = 0x7f7f7f7f;
    for (int d = 0; d < W; ++d) {
        int info = 0;
        if (int rc = fit_check(m->fits[d])) return rc;
        if (int rc = shard_finish(m->fits[d], part.data(), &info)) return rc;
        HIPCHK(hipStreamSynchronize(m->fits[d]->cstream));
        if (m->fits[d]->cstream_l != m->fits[d]->cstream) HIPCHK(hipStreamSynchronize(m->fits[d]->cstream_l));
        for (int i = 0; i < len; ++i) tot[i] += part[i];
        if (info < info_min) info_min = info;
    }
    return shard_collect(f0, tot, (double)info_min, sum_logliks, parts);
}

// Dense kriging with the m prediction locations split over the devices of the handle (BASELINE config C5:
// the right-hand sides shard): every device factors Sigma with its own slice of the
// cross-covariance rows as border -- no exchange at all -- and the slices are concatenated on the host.
// Outputs as cocons_predict_dense.  One host thread per device issues that device's call.
extern "C" int cocons_multi_predict_dense(cocons_multi *m, const double *theta, const double *mean, int z_col,
                                          int mp, const double *locs_pred, const double *X_pred,
                                          double *stochastic, double *quadform)
{
    if (!m || !theta || !mean || mp <= 0 || !locs_pred || !X_pred || !stochastic || !quadform)
        return fail(-1, "cocons_multi_predict_dense: bad argument");
    const int W = m->ndev, p = m->fits[0]->p;
    std::vector<int> rcs(W, 0);
    std::vector<std::string> errs(W);
    std::vector<std::thread> th;
    for (int d = 0; d < W; ++d) {
        const int lo = (int)((long long)mp * d / W), hi = (int)((long long)mp * (d + 1) / W);
        if (hi <= lo) continue;
        th.emplace_back([=, &rcs, &errs]() {
            const int k = hi - lo;
            std::vector<double> lp((size_t)2 * k), Xp((size_t)p * k);       // column-major slices
            for (int c = 0; c < 2; ++c)
                for (int i = 0; i < k; ++i) lp[(size_t)i + (size_t)c * k] = locs_pred[(size_t)(lo + i) + (size_t)c * mp];
            for (int c = 0; c < p; ++c)
                for (int i = 0; i < k; ++i) Xp[(size_t)i + (size_t)c * k] = X_pred[(size_t)(lo + i) + (size_t)c * mp];
            rcs[d] = cocons_predict_dense(m->fits[d], theta, mean, z_col, k, lp.data(), Xp.data(), stochastic + lo, quadform + lo);
            if (rcs[d] != 0) errs[d] = g_err;          // g_err is thread-local
        });
    }
    for (auto &t : th) t.join();
    for (int d = 0; d < W; ++d)
        if (rcs[d] != 0) { g_err = errs[d]; return rcs[d]; }
    return 0;
}

// Replica mode inside one process: the nb independent parameter points of one finite-difference gradient
// (R/optim.R:256-259, 1 + 2P points) or of getHessian (R/getFunctions.R:979-1016) are dealt over the devices of the
// handle -- point i goes to device i mod ndev -- and every device runs its share through cocons_neg2loglik_batch on
// its own fit (own slots, own streams), driven by one host thread per device.  No collective: the evaluations are
// independent, so the handle may list a device more than once.  thetas / means / values / status as
// cocons_neg2loglik_batch.
extern "C" int cocons_multi_neg2loglik_batch(cocons_multi *m, int nb, const double *thetas, const double *means,
                                             double *values, int *status)
{
    if (!m || nb < 0 || (nb > 0 && (!thetas || !means || !values || !status)))
        return fail(-1, "cocons_multi_neg2loglik_batch: bad argument");
    const int W = m->ndev, p = m->fits[0]->p, tp = 6 * p;
    for (int i = 0; i < nb; ++i) { values[i] = NAN; status[i] = -1; }
    std::vector<int> rcs(W, 0);
    std::vector<std::string> errs(W);
    std::vector<std::thread> th;
    for (int d = 0; d < W; ++d) {
        const int cnt = nb > d ? (nb - d + W - 1) / W : 0;
        if (cnt == 0) continue;
        th.emplace_back([=, &rcs, &errs]() {
            std::vector<double> T((size_t)cnt * tp), M((size_t)cnt * p), V(cnt);
            std::vector<int> S(cnt);
            for (int j = 0; j < cnt; ++j) {
                const int i = d + j * W;
                memcpy(&T[(size_t)j * tp], thetas + (size_t)i * tp, (size_t)tp * sizeof(double));
                memcpy(&M[(size_t)j * p], means + (size_t)i * p, (size_t)p * sizeof(double));
            }
            rcs[d] = cocons_neg2loglik_batch(m->fits[d], cnt, T.data(), M.data(), V.data(), S.data());
            if (rcs[d] != 0) errs[d] = g_err;          // g_err is thread-local
            for (int j = 0; j < cnt; ++j) { values[d + j * W] = V[j]; status[d + j * W] = S[j]; }
        });
    }
    for (auto &t : th) t.join();
    for (int d = 0; d < W; ++d)
        if (rcs[d] != 0) { g_err = errs[d]; return rcs[d]; }
    return 0;
}

// devices the communicators of a multi handle span (0: the handle has none -- a device is listed twice), and the
// size RCCL itself reports for the communicator of the handle's first device (ncclCommCount)
extern "C" int cocons_multi_comm_ranks(cocons_multi *m, int *ndev, int *rccl_count)
{
    if (!m) return fail(-1, "cocons_multi_comm_ranks: null handle");
    if (ndev) *ndev = m->ndev;
    int cnt = 0;
    if (!m->comms.empty()) {
        RcclApi *R = rccl_api();
        if (!R) return -1;
        NCCLCHK(R->CommCount(m->comms[0], &cnt));
    }
    if (rccl_count) *rccl_count = cnt;
    return 0;
}

// the same for a fit that carries a communicator of its own (cocons_fit_comm_init): what ncclCommCount and
// ncclCommUserRank / ncclCommCuDevice say -- the proof bench.py prints that RCCL saw N ranks on N devices
extern "C" int cocons_fit_comm_info(cocons_fit *f, int *count, int *user_rank, int *device)
{
    if (!f) return fail(-1, "cocons_fit_comm_info: null handle");
    int c = 0, u = -1, dv = -1;
    if (f->coll_kind == 1 && f->comm) {
        RcclApi *R = rccl_api();
        if (!R) return -1;
        NCCLCHK(R->CommCount(f->comm, &c));
        NCCLCHK(R->CommUserRank(f->comm, &u));
        NCCLCHK(R->CommCuDevice(f->comm, &dv));
    } else if (f->coll_kind == 2) {
        c = f->coll_world; u = f->coll_rank; dv = f->device;
    }
    if (count) *count = c;
    if (user_rank) *user_rank = u;
    if (device) *device = dv;
    return 0;
}
