// fit.hpp -- internal to the C ABI's translation units (api*.hip): error reporting, the owned device buffer, the fit handle
// with the states it owns, and the declarations of what api.hip -- the path of one objective evaluation, the schedules -- and
// api_handle.hip -- the handle's life -- offer the others.  Not installed, not part of the contract
// (include/cocons_hip.h is).  Everything declared here is hidden from the library's dynamic symbol table; a variable or a
// function-local static lives in exactly one .hip file, never here.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <time.h>
#include <rccl/rccl.h>         // ncclComm_t (members of the handle); the library is loaded on first use, api_shard.hip

#include <algorithm>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.h"
#include "band_plan.hpp"       // the envelope rule and the packed layout of a band factor (host only)
#include "../../include/cocons_hip_diag.h"
#include "matern_device.hpp"   // PairMode, LOCP_FIELDS (host-visible enums)

using namespace cocons;

#pragma GCC visibility push(hidden)

extern thread_local std::string g_err;      // the text cocons_last_error returns (api.hip)
int fail(int code, const char *fmt, ...);

#define HIPCHK(expr)                                                              \
    do {                                                                          \
        hipError_t e__ = (expr);                                                  \
        if (e__ != hipSuccess) {                                                  \
            char b__[512];                                                        \
            snprintf(b__, sizeof b__, "%s failed: %s (%s:%d)", #expr,             \
                     hipGetErrorString(e__), __FILE__, __LINE__);                 \
            g_err = b__;                                                          \
            return -100 - (int)e__;                                               \
        }                                                                         \
    } while (0)

enum { ENGINE_ABORT = -5 };
enum { TH_SD = 0, TH_SCALE = 1, TH_ANISO = 2, TH_TILT = 3, TH_SMOOTH = 4, TH_NUGGET = 5 };

struct ModeSel {
    int mode;          // PairMode
    int smooth_kind;   // SmoothKind
    double nu_fixed;
    double gr;
};

// The mailboxes of the factorisation use the all-ones bit pattern as "not written yet" (chol.hip: the data is its own flag).
// That pattern is a quiet NaN no arithmetic PRODUCES -- the hardware's own NaN is 0x7ff8000000000000 -- but NaN payloads
// PROPAGATE, so an all-ones NaN in the caller's data or parameters could reach a factor block and be waited for until the bounded
// wait gives up (a time-out and a repeat, never a wrong value).  Everything that enters the device is therefore canonicalised:
// an all-ones NaN becomes the standard quiet NaN (R's NA_real_ and NaN are other patterns and pass unchanged).
inline double canon_nan(double v)
{
    unsigned long long b;
    memcpy(&b, &v, sizeof b);
    return b == ~0ull ? std::numeric_limits<double>::quiet_NaN() : v;
}

hipError_t upload_canon(double *dst, const double *src, size_t count, hipStream_t s);

// One owned device allocation and its element count: a local of a one-shot entry point (freed on every way out of it) or a
// member of a handle or of one of its states (freed with it).  Empty: null with count 0 -- also after an allocation failed.
// A buffer frees its memory only in the process that allocated it: a forked child that drops a handle abandons the
// parent's device memory and makes no HIP call on a runtime it does not own (cocons_fit_destroy).
template <class T> class DevBuf {
    T *p_ = nullptr;
    size_t n_ = 0;
    pid_t pid_ = 0;
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_), pid_(o.pid_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); std::swap(pid_, o.pid_); return *this; }
    ~DevBuf() { reset(); }
    void reset()
    {
        if (p_ && pid_ == getpid()) hipFree(p_);
        p_ = nullptr; n_ = 0;
    }
    hipError_t alloc(size_t count)
    {
        reset();
        hipError_t e = hipMalloc(&p_, count * sizeof(T));
        if (e != hipSuccess) { p_ = nullptr; return e; }
        n_ = count; pid_ = getpid();
        return e;
    }
    // Hold at least (exact: exactly) count elements.  Nothing to do: no HIP call at all -- this sits on the path of every
    // evaluation.  Otherwise: drain the handle's main stream s and its engine's stream s2 (may be null) -- work in flight may
    // still use the old memory --, free, allocate and, with fill >= 0, set every byte to fill on s (not waited for).
    // *grew (may be null): whether the buffer is a new allocation.
    hipError_t reserve(size_t count, hipStream_t s, hipStream_t s2, int fill = -1, bool exact = false, bool *grew = nullptr)
    {
        if (grew) *grew = false;
        if (exact ? n_ == count : n_ >= count) return hipSuccess;
        hipError_t e = hipStreamSynchronize(s);
        if (e == hipSuccess && s2) e = hipStreamSynchronize(s2);
        if (e == hipSuccess) e = alloc(count);
        if (e == hipSuccess && fill >= 0) e = hipMemsetAsync(p_, fill, count * sizeof(T), s);
        if (grew) *grew = e == hipSuccess;
        return e;
    }
    size_t count() const { return n_; }
    T *get() const { return p_; }
    operator T *() const { return p_; }
};

// Declared AFTER a function's DevBufs, so that its destructor -- draining the stream the buffers are used on -- runs before
// theirs, on every way out.  own: the stream was created for this call and is destroyed as well.
struct StreamDrain {
    hipStream_t s;
    bool own;
    ~StreamDrain()
    {
        if (!s) return;
        hipStreamSynchronize(s);
        if (own) hipStreamDestroy(s);
    }
    operator hipStream_t() const { return s; }
};

// HIPCHK for the one-shot entry points: the message names the entry point, the code is -100 - hipError_t
#define HIPCHK_AT(who, expr)                                                                        \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess) return fail(-100 - (int)e__, "%s: %s", who, hipGetErrorString(e__)); \
    } while (0)

// theta -> kernel arguments (api.hip)
void make_theta_vecs(const double *theta_in, int p, ThetaVecs &tv, bool full_scale = false);
ModeSel select_mode(const double *theta, int p, const double *smooth_limits, int which);
LocArgs loc_args(int n, int p, const double *X, const double *locs, double *out, size_t stride, const ThetaVecs &tv,
                 int smooth_kind, const double *smooth_limits);
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// What both kriging states hold (KrigeHeld): the packed factor with its solve operands, w, the observation-side SoA, the
// staging and the outputs of one chunk of `rows` new locations, and the prepared theta and mean.  Every buffer is owned by the
// state it is a member of, so no other entry point on the handle -- predict growing dA, the batch slots, engine retries --
// can touch it; the joint entries read it only.
struct KrigeHeld {
    DevBuf<double> L;             // the factor's lower 128 x 128 tiles, packed (dense: all nt (nt + 1) / 2, kernels.h launch_krige_pack;
                                  // taper: the envelope's, tile (I, J) at plan.toff[J] + (I - J), launch_krige_band_pack)
    DevBuf<double> Q;             // nt x 2048: the triangular-solve operands of every diagonal tile
    DevBuf<double> w;             // npad: L^-1 (z[:, z_col] - X mean), zero in the padding and slot columns
    DevBuf<double> loc;           // LOCP_FIELDS x npad: observation-side SoA in the prediction branch's parameters
    DevBuf<double> Xp, lp, locp;  // the chunk's X_pred (rows x p), locations (rows x 2) and SoA (LOCP_FIELDS x rows)
    DevBuf<double> st, qd;        // rows: the chunk's outputs
    std::vector<double> theta;    // 6 p: the prepared theta (canonicalised)
    std::vector<double> mean;     // p: the prepared mean (canonicalised; the joint entries' trend of the draws)
    int rows = 0;                 // rows per chunk (a multiple of 64)
};

// Kriging state of a dense handle (cocons_krige_prepare / _apply / _release)
struct KrigeState : KrigeHeld {
    DevBuf<double> C;             // rows x npad: one chunk of cross-covariance rows, solved in place
    long long bytes = 0;          // device bytes held
};

// The binned targets of a pattern search (pattern.hip), owned: the grid for `delta` over n points whose
// coordinates (t.x, t.y) belong to somebody else, the cell-sorted list and the binning's scratch.
struct PatternGridBufs {
    PatternTargets t;
    double delta = 0.0;
    DevBuf<int> cstart, sidx, cursor;
    DevBuf<double> sxy;
    long long bytes = 0;          // device bytes of the buffers above
};

// Kriging state of a taper handle (cocons_krige_taper_prepare / _apply / _release): the band factor packed
// per tile column and a ring of W tile columns for the chunk.
struct KrigeTaperState : KrigeHeld {
    DevBuf<double> ring;          // rows x plan.W * 128: tile column I of the chunk's right-hand side in slot I mod W
    DevBuf<int> d_toff;           // nt: device copy of plan.toff
    // CSR staging of a chunk, ecap entries (grown to the densest chunk seen): mapped columns, the caller's taper values, the
    // entries' covariance values, the buckets (destination in the slot, entry index), and the chunk's row pointers
    DevBuf<int> ci, rp, bdst, bsrc;
    DevBuf<double> tv, val;
    size_t ecap = 0;
    BandPlan plan;                // first packed tile of every tile column, slots of the ring (band_plan.hpp)
    long long fixed_bytes = 0;    // device bytes of everything but the CSR staging
    // cocons_krige_taper_apply_delta, made by its first call: the grid over the observations in the handle's
    // order, and the bucket histogram, offsets and cursors of a chunk (3 x (nt + 1) ints)
    std::unique_ptr<PatternGridBufs> grid;
    DevBuf<int> bwork;
    long long bytes() const
    {
        return fixed_bytes + (long long)(ecap * (3 * sizeof(int) + 2 * sizeof(double))) +
               (grid ? grid->bytes + (long long)(bwork.count() * sizeof(int)) : 0);
    }
};

// host-side plan of one evaluation's exchange: per block k the rows below it, dealt to their owners and packed
struct ShardPlan {
    int nt = 0, mt = 0, world = 0, group = 0;
    std::vector<int> tlo;            // per block: first 64-row tile below the block
    std::vector<int> ncols;          // per block: its columns (256, or 128 for a last block of one tile)
    std::vector<long long> srows;    // per block: rows per slot S_k (64 x the largest number of tiles any rank owns below)
    std::vector<int> pmap;           // nb x T64: element offset of 64-row tile ti in the gathered buffer of block k (-1: above)
    std::vector<int> cnt;            // nb x world: tiles rank w owns below block k
    size_t max_elems = 0;            // largest gathered buffer
};

// plan, buffers and events of the sharded evaluation on one handle (api_shard.hip)
struct ShardState {
    ShardPlan plan;
    DevBuf<int> d_pmap;
    DevBuf<double> lkk[2];
    hipEvent_t ev_main_L = nullptr, ev_comm_L[2] = {nullptr, nullptr}, ev_main_X[2] = {nullptr, nullptr},
               ev_comm_X[2] = {nullptr, nullptr};
    hipEvent_t ev_main_U[2] = {nullptr, nullptr};    // main stream: the received L_kk in lkk[k & 1] has been unpacked (the buffer may be
    bool unpacked[2] = {false, false};               // overwritten by the broadcast of L_(k+2)); unpacked[b]: recorded this evaluation
};

// Scratch of the dense, Profile and REML gradients and of cocons_fisher_dense (api_grad.hip)
struct GradState {
    DevBuf<double> scratch;       // grad_scratch_doubles(npad)
    DevBuf<double> AR;            // npad x r: Sigma^-1 R
    DevBuf<double> ARpart;        // its partial sums (grad_sigma_r_scratch_doubles)
    DevBuf<double> site;          // GSITE_FIELDS x npad
    DevBuf<double> out;           // 7 p: theta-table gradient, mean gradient
    // Profile / REML gradients only (allocated by their first call, for a border of pcols = r + max(p, q) rows)
    DevBuf<double> SX;            // npad x pcols: Sigma^-1 [Z | Xb]
    DevBuf<double> SXpart;        // its partial sums
    DevBuf<double> LR;            // npad x pcols: the low-rank block [U | sqrt(r) C]
    DevBuf<double> gls;           // chol(Xb' Sigma^-1 Xb) and beta (grad_gls_doubles)
    int pcols = 0;
    long long bytes = 0;          // device bytes of the buffers above
};

// State of cocons_neg2loglik_grad_taper on a taper handle: the selected inverse goes to a second buffer of
// the band's shape, the factor in dA is consumed by the sweep (every operation on the handle assembles its matrix anew).
struct TaperGradState {
    DevBuf<double> Z;             // S^-1 on the tile envelope: ldz x npad, ldz = skew * 128 (packed) or npad
    DevBuf<double> AR;            // npad x r: S^-1 R
    DevBuf<double> ent;           // 6 x nnz: per stored entry, the weighted partials (grad.hip taper_grad_entry_kernel)
    DevBuf<double> site;          // GSITE_FIELDS x npad
    DevBuf<double> gsite;         // 9 x npad
    DevBuf<double> out;           // 9 p
    DevBuf<int> tcp, tidx, trow;  // transposed index of the device pattern (built on the host, once)
    size_t ldz = 0;
    long long bytes = 0;          // device bytes of the buffers above
};

// U^-1 of a Vecchia fit (api_vecchia_sim.hip): the level schedule of (table, n_fixed) -- the last one asked for --
// and the coefficients of one call, n (m + 1) doubles of scratch.
struct VecchiaSimState {
    int n_fixed = -1;             // what the schedule below was made for; -1: none yet
    DevBuf<int> level;            // n: the rows' levels (0: a fixed row)
    DevBuf<int> order;            // n - n_fixed: the rows by level
    DevBuf<int> off;              // depth + 1 offsets into order (allocated n + 2: the counts are formed in it)
    DevBuf<int> word;             // {changed, depth}
    std::vector<int> hoff;        // off on the host: what the launches are planned from
    int widest = 0;               // rows of the largest level
    DevBuf<double> coef;          // n x (m + 1): the rows' s for this theta
    int depth() const { return hoff.empty() ? 0 : (int)hoff.size() - 1; }
    long long schedule_bytes() const { return (long long)((level.count() + order.count() + off.count() + word.count()) * sizeof(int)); }
    long long bytes() const { return schedule_bytes() + (long long)(coef.count() * sizeof(double)); }
};

// U' of a Vecchia fit (api_vecchia_cv.hip): the transposed lists of the table -- a function of the table alone,
// built by the first call that needs them and kept for the handle's life.
struct VecchiaCvState {
    bool built = false;
    DevBuf<int> ptr;              // n + 1 offsets: list(j) = rows[ptr[j] .. ptr[j + 1])
    DevBuf<int> rows;             // entries: the rows that name j, ascending (0-based)
    DevBuf<unsigned char> place;  // entries: the place of j in that row of the table
    long long entries = 0, longest = 0, unnamed = 0;
    long long bytes() const { return (long long)((ptr.count() + rows.count()) * sizeof(int) + place.count()); }
};

// U^-T of a Vecchia fit (api_vecchia_cov.hip): the transposed level schedule of (table, n_fixed, tier threshold)
// -- the last one asked for --, next to the forward one of VecchiaSimState, and the indices of cocons_vecchia_cov_cols.
struct VecchiaSolveTState {
    int n_fixed = -1, wide = -1;  // what the schedule below was made for; -1: none yet
    DevBuf<int> level;            // n: the rows' transposed levels (0: a fixed row)
    DevBuf<int> key;              // n: 2 level - 1 (one-wave tier) or 2 level (wide tier)
    DevBuf<int> order;            // n - n_fixed: the rows by key
    DevBuf<int> off;              // 2 depth + 1 offsets into order (allocated 2 n + 2: the counts are formed in it)
    DevBuf<int> word;             // {changed, largest key}
    DevBuf<int> idx;              // the columns' rows of one cocons_vecchia_cov_cols call
    std::vector<int> hoff;        // off on the host: what the launches are planned from
    int widest = 0;               // rows of the largest level
    long long wide_rows = 0;      // rows of the wide tier
    int depth() const { return hoff.empty() ? 0 : (int)(hoff.size() - 1) / 2; }
    long long bytes() const
    {
        return (long long)((level.count() + key.count() + order.count() + off.count() + word.count() + idx.count()) * sizeof(int));
    }
};

// Grouped blocks of a Vecchia fit (api_vecchia_group.hip): the plan of cocons_vecchia_set_groups on the device --
// group_plan.hpp's GroupPlan --, replaced by a second call.
struct VecchiaGroupState {
    DevBuf<int> off;              // blocks + 1 offsets into rows
    DevBuf<int> rows;             // every block's rows, ascending (0-based)
    DevBuf<int> order;            // the blocks largest first: the sequence a launch deals them in
    DevBuf<unsigned long long> mask;   // per block: bit p = the row at position p is a member
    int blocks = 0, maxrows = 0;
    bool by_size = true;          // deal the blocks in `order` (COCONS_VECCHIA_GROUP_ORDER=0: by block id)
    long long sum_rows = 0, pairs = 0;
    long long bytes() const
    {
        return (long long)((off.count() + rows.count() + order.count()) * sizeof(int) + mask.count() * sizeof(unsigned long long));
    }
};

// What makes a handle a Vecchia handle (cocons_fit_create_vecchia, api_vecchia.hip): the neighbour table and the
// scratch of one evaluation, O(n (m + r + 16)) bytes.  Such a handle has no factorisation buffer at all.
struct VecchiaState {
    int m = 0;                    // columns of the table
    DevBuf<int> nbr;              // n x m, row after row: 0-based neighbours ascending, -1 behind them (kernels.h VecchiaArgs)
    DevBuf<double> aos, aos2;     // VECCHIA_REC x n: the observations' records for this theta (aos2: in the prediction branch's
                                  // parameters, made by the first prediction whose theta needs it)
    DevBuf<double> B;             // n x c: the right-hand sides (the residuals, or cocons_vecchia_whiten's columns)
    DevBuf<double> W;             // n x (1 + c): log d, then the whitened columns
    DevBuf<double> part;          // first-stage sums of the totals
    // cocons_neg2loglik_grad_vecchia, allocated by its first call: O(n) with a small constant, plus one chunk
    DevBuf<double> gsite;         // GSITE_FIELDS x npad: launch_grad_site's SoA
    DevBuf<double> gaos;          // VECCHIA_GSITE_REC x n: the same as one record per location
    DevBuf<double> grec;          // VECCHIA_GRAD_CHUNK x vecchia_rec_cols(p): the per-observation records of one chunk
                                  // (the grouped gradient, DESIGN.md 4z: one record per block; gpart and gout serve it too)
    DevBuf<double> gpart;         // their first-stage sums, all segments of n
    DevBuf<double> gout;          // the totals: 1 + c of the value, then vecchia_rec_cols(p)
    // cocons_fisher_vecchia, allocated by its first call (gsite and gaos above are shared with the gradient)
    DevBuf<double> fdirs;         // ndir x 6 p: the directions
    DevBuf<double> frec;          // vecchia_fisher_chunk x vecchia_fisher_cols: the per-observation records of one chunk
                                  // (the grouped information, DESIGN.md 4aa: one record per block; fpart and fout serve it too)
    DevBuf<double> fpart;         // their first-stage sums, all segments of n
    DevBuf<double> fout;          // the totals: vecchia_fisher_cols
    // cocons_vecchia_predict_knn, made by its first call: the grid over the observations
    std::unique_ptr<PatternGridBufs> knn;
    // cocons_vecchia_predict_corr_knn, cocons_vecchia_neighbours_corr_pred with hops = 2, made by the first
    // such call and made again by a call at another width: the plain kNN of every observation's own coordinates among all
    // observations, n x corr_all_mc in the layout of nbr
    DevBuf<int> corr_all;
    int corr_all_mc = 0;
    // cocons_vecchia_unwhiten, cocons_sim_vecchia, cocons_vecchia_schedule, made by their first call
    std::unique_ptr<VecchiaSimState> sim;
    // cocons_vecchia_transpose, cocons_vecchia_whiten_t, cocons_cv_vecchia, made by their first call
    std::unique_ptr<VecchiaCvState> cv;
    // cocons_vecchia_unwhiten_t, cocons_vecchia_cov_mult, cocons_vecchia_cov_cols, cocons_vecchia_schedule_t
    std::unique_ptr<VecchiaSolveTState> solve_t;
    // cocons_vecchia_set_groups: the plan of the grouped value and whitening
    std::unique_ptr<VecchiaGroupState> grp;
    long long bytes() const
    {
        return (knn ? knn->bytes : 0) + (sim ? sim->bytes() : 0) + (cv ? cv->bytes() : 0) + (solve_t ? solve_t->bytes() : 0) +
               (grp ? grp->bytes() : 0) +
               (long long)((nbr.count() + corr_all.count()) * sizeof(int) +
                           (aos.count() + aos2.count() + B.count() + W.count() + part.count() + gsite.count() + gaos.count() +
                            grec.count() + gpart.count() + gout.count() + fdirs.count() + frec.count() + fpart.count() +
                            fout.count()) * sizeof(double));
    }
};

// elements of the three parts of the mailbox buffer (dmbox; the accessors are below the handle)
struct MboxLayout {
    size_t tiles = 0, smb = 0, xmb = 0;
    size_t total() const { return tiles + smb + xmb; }
};

// ---------------------------------------------------------------------------
// Every device buffer of the handle is a DevBuf member (freed with the handle, cocons_fit_destroy), every host container a
// member by value; a feature that needs another buffer declares one.
struct cocons_fit {
    int n = 0, p = 0, r = 0, q = 0, device = 0;
    pid_t pid = 0;
    int npad = 0, nt = 0;    // padded order, tiles of 128
    int rhs_cap = 0;         // rows reserved under the matrix (multiple of 128)
    int rhs_act = 0;         // rows under the matrix the CURRENT operation uses (multiple of 128, <= rhs_cap)
    size_t lda = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf<double> dX, dlocs, dz, dxb;
    DevBuf<double> dloc;     // LOCP_FIELDS x npad
    DevBuf<double> dA;       // lda * npad doubles, or more once a gradient call has grown it (grad_prepare)
    DevBuf<double> dinv;     // 2 x 8 x 256
    DevBuf<double> dinfo_out;     // ONE allocation: the two info words, then the reductions
    int *dinfo = nullptr;         // (view of dinfo_out)
    double *dout = nullptr;       // reductions (view of dinfo_out)
    double *hout = nullptr;       // pinned mirror (hinfo, hout, hinfo_init: one pinned allocation, freed through hinfo)
    int *hinfo = nullptr, *hinfo_init = nullptr;
    double smooth_limits[2] = {0, 0};
    size_t out_cap = 0;
    // predict scratch (pred_reserve)
    DevBuf<double> dlocp, dXp, dlocsp, dstoch, dquad, dred;
    // sharded state
    int rank = 0, world = 1, nrhs_cur = 0;
    int nslot = 0;                // > 0: the last nslot of the npad rows / columns are SLOTS (npad = n + nslot): columns with a huge
                                  // diagonal and nothing else, rows that hold the right-hand sides of an evaluation (at most nslot
                                  // of them) INSIDE the last tile of the matrix -- no tile row under the matrix (enqueue_eval)
    int n_user = 0, pad0 = 0;     // n = pad0 + n_user: dense handles keep pad0 = npad - n_user placeholder observations IN FRONT
                                  // of the caller's (their columns are made unit vectors before every factorisation,
                                  // launch_front_identity), so that n == npad and no padding sits in the trailing matrix
    DevBuf<double> xbuf[2];       // exchange buffers of the sharded evaluation (shard_prepare)
    hipEvent_t ev[8] = {};
    hipStream_t stream2 = nullptr;     // stream the resident diagonal-tile engine is launched on
    hipEvent_t ev_eng = nullptr;  // orders the engine launch behind the reset of its flag words
    DevBuf<unsigned> dflags;      // the hand-off words: handoff_words() below is their map
    int flags_cap = 0;            // (the stride between in[], out[] and xr[]: not just dflags' count)
    bool engine_ok = false;       // false: this handle never uses the resident engine (batch slots, band-limited taper fits)
    bool engine_pair_lost = false;     // engine_ok went false in cocons_fit_set_stream (the caller's stream shares the engine stream's
                                  // hardware queue, or is the NULL stream): the next stream installed is tested afresh
    bool engine_live = false;     // the engine of the NEXT factorize call is already launched (engine_start)
    bool engine_used = false;     // the factorisation enqueued last runs on the engine schedule
    int border_clean = -1;        // nr >= 0: the rows [nr, rhs_act) under the matrix are known to be exactly zero in every column
                                  // (they were zeroed, and a SUCCESSFUL factorisation keeps zero rows zero): the next
                                  // evaluation with the same nr does not zero them again (-1: unknown)
    int border_pending = -1;      // what border_clean becomes when the operation in flight turns out to have succeeded
    bool engine_active_last = false;   // the last COMPLETED operation ran on the engine schedule (cocons_fit_engine_state)
    int engine_skip = 0;          // operations still to run on the plain schedule after a hand-off timed out (back-off)
    int engine_fails = 0;         // consecutive time-outs (the back-off doubles with each, up to 64 operations)
    int engine_retries = 0;       // time-outs in the life of the handle, each answered by one repeat on the plain schedule
    int engine_last_abort = 0;    // abort word of the last time-out (who gave up: see info_status)
    long long engine_ops = 0;     // operations enqueued on the engine schedule so far (the first one's gate is patient)
    // dependency-driven schedule (factorize_dag): second buffer shaped like dA, tile inverses, task words, step table
    DevBuf<double> dP;
    DevBuf<double> dWt;           // one 128 x 128 tile per tile column
    DevBuf<double> dpart;         // early halves of the split diagonal-block tiles (2 x 16 x 64 x 64 doubles)
    DevBuf<unsigned> ddag;        // the task words: dag_words() below is their map
    DevBuf<DagStepHost> ddag_steps; int dag_nsteps = 0; unsigned dag_ntasks = 0;
    int dag_key[12] = {};         // (nt, mt, trim, kskip, lead, min_tiles, lead2, lead3, order, xcd, bw, bh) the step table was built for
    DevBuf<unsigned> ddag_ftab;   // which tile every far tile task is (dag_build_steps' table), device copy
    int dag_xcd_g = 0;            // chunk exponent of the XCD-aware deal the table was built for (0: one counter)
    bool dag_have_ftab = false;   // the current step table comes with a far-tile table
    DevBuf<unsigned long long> ddag_trace;   // diagnostics (cocons_debug_tune("dag_trace", 1)): dag_trace_words() below
    size_t dag_trace_tasks = 0;              // tasks the buffer describes (0: not this step table)
    bool dag_next = false;        // the engine launched by engine_start is the DAG schedule's (publishes W and the second X)
    int engine_pair_live = 0;     // 1: the engine launched for the next factorisation has a pair partner (it counts itself in alive[2])
    MboxLayout mbox;                     // what dmbox holds (mbox_reset)
    DevBuf<double> dmbox;                // one mailbox per tile (mbox_reset): the engine's pair mode, the panel kernel and potrf_solve's
                                         // followers read a tile's factor from there while it is being formed; tile_mbox() .. below
    bool follow_used = false, follow_off = false;   // the operation being enqueued used launch_potrf_follow; it timed out once on this handle: off
    double enq_host_us = 0; long long enq_calls = 0;   // (diagnostics) host time spent enqueueing evaluations, calls: cocons_debug_host_enqueue
    bool dag_used = false;        // the factorisation enqueued last ran the DAG schedule: its factor is split over dA and dP
    double dag_flops = 0; int dag_events = 0;   // profile runs: update flops inside the DAG launch; 1 = the first event pair is that launch
    // taper fit (cocons_fit_create_taper): the spam pattern (1-based CSR) with the taper's entries; the
    // -2 log-likelihood is then that of the TAPERED covariance, evaluated through the dense factorisation
    int taper_nnz = 0;            // > 0: taper fit
    DevBuf<int> d_tci, d_trp;
    DevBuf<double> d_tval;        // taper entries (constant)
    std::vector<int> taper_hi;    // envelope of the (reordered) pattern per tile column: see FactorView::hi (empty: none)
    DevBuf<int> d_thi; int taper_maxband = 0; // device copy of taper_hi and max_c (hi[c] - c)
    int skew = 0;                 // > 0: the factorisation buffer is PACKED (kernels.h band_index): every tile column keeps
                                  // `skew` (= taper_maxband) tile rows from its diagonal tile down plus the rows under the
                                  // matrix -- O(n x bandwidth) doubles instead of n^2
    std::vector<int> taper_inv;   // position of the caller's observation i in the handle's order (reverse Cuthill-McKee)
    std::vector<int> obs_pos;     // internal position (behind the front padding, in Morton order) of the caller's observation i,
                                  // kept by every handle fit_create_impl makes (n ints); read by cocons_cv_dense, which maps labels
                                  // in and results out through it (a taper handle's order on top of it is taper_inv)
    std::vector<int> h_trp, h_tci;     // host copy of the full (symmetric) pattern and taper entries in the handle's order:
    std::vector<double> h_tval;        // what a twin in another order is built from (O(nnz))
    cocons_fit *taper_twin = nullptr;  // lazily created taper handle in the order of the last pivot cocons_sim_taper was given
    std::vector<int> twin_perm;   // that order: twin position k holds the observation at position twin_perm[k] of this handle
    float sim_ms[3] = {0, 0, 0};  // last cocons_sim_taper: assembly + factorisation, band product, gather (device events)
    // collectives of the natively sharded evaluation (see "native sharded evaluation" below)
    int coll_kind = 0;            // 0 none, 1 RCCL communicator, 2 caller-provided transport
    int coll_rank = 0, coll_world = 0;
    ncclComm_t comm = nullptr;
    bool comm_own = false;        // the communicator was created by cocons_fit_comm_init (destroy it with the fit)
    cocons_bcast_fn cb_bcast = nullptr;
    cocons_allreduce_fn cb_allreduce = nullptr;
    cocons_allgather_fn cb_allgather = nullptr;
    std::unique_ptr<ShardState> shard;   // plan, buffers and events of the sharded evaluation (row-block ownership)
    void *cb_user = nullptr;
    hipStream_t cstream = nullptr;     // stream the bulk exchange (all-gather of the solved rows) is issued on
    hipStream_t cstream_l = nullptr;   // stream the 0.56 MB broadcasts of the factored diagonal blocks are issued on: the chain from one
                                  // diagonal block to the next never queues behind an all-gather (== cstream when the
                                  // broadcasts have no communicator of their own)
    ncclComm_t comm_l = nullptr;  // RCCL: a second communicator over the same ranks (ncclCommSplit) for those broadcasts --
                                  // operations of ONE communicator are serialised whatever stream they are given; null: comm
    bool comm_l_own = false;
    DevBuf<double> dcoll;         // device staging of the final all-reduce (RCCL)
    double upd_flops = 0;         // algorithmic flops of the event-timed trailing updates (profile runs)
    // host copies of the inputs + lazily created clones: the slots of cocons_neg2loglik_batch
    std::vector<double> h_locs, h_X, h_z, h_xb;
    std::vector<cocons_fit *> slots;
    bool sorted = false;          // observations are stored in Morton order (see fit_create_impl)
    cocons_fit *unsorted = nullptr;    // lazily created clone in the ORIGINAL order (marginal simulation)
    std::recursive_mutex op_mu;   // held by every entry point for as long as it works on this handle (FIT_ENTER), and by another
                                  // handle's stream self-test while it launches probe kernels on this handle's streams
                                  // (engine_warm: try_lock under the registry's lock -- a busy handle is not probed, a probed one
                                  // can neither be used nor destroyed until the probe is over)
    std::unique_ptr<KrigeState> krige;   // kriging state (cocons_krige_prepare): one factor of Sigma(theta) held apart from dA
    std::unique_ptr<KrigeTaperState> krige_taper;   // taper fit: kriging state (cocons_krige_taper_prepare); clones and twins carry none
    std::unique_ptr<GradState> grad;     // scratch of cocons_neg2loglik_grad_dense (allocated on first use)
    std::unique_ptr<TaperGradState> tgrad;   // taper fit: state of cocons_neg2loglik_grad_taper (allocated on first use)
    std::unique_ptr<VecchiaState> vecchia;   // non-null: a Vecchia handle (cocons_fit_create_vecchia) -- the third kind
};

// ---- one map per region of device words (every offset in ONE place; the abort dump -- api_diag.hip debug_abort_report, decoded by
// tools/dag_abort.py --, cocons_debug_dag_words and the tests read these indices) ------------------------------------------
// The hand-off words of a factorisation (dflags, zeroed by flags_reset): in[t], out[t], xr[t] (see EngineLaunch), flags_cap
// words each; then 64 words -- the engine's alive word, at + 8 the two words of the stream self-test, at + 16 the
// workgroups that took part per XCD --; then flags_cap tile counters of the trailing updates.  abort: the word behind the
// info word (who gave up, kernels.h abort_code).
struct HandoffWords {
    unsigned *in, *out, *xr, *alive, *selftest, *xcd_arrivals, *abort, *queues;
    unsigned *tile_queue(int k) const { return queues + k / 2; }   // of the update with block k's panel: update_kernel's dynamic tile order
};
inline size_t handoff_word_count(int cap) { return 4 * (size_t)cap + 64; }
inline HandoffWords handoff_words(const cocons_fit *f)
{
    HandoffWords w;
    const size_t cap = (size_t)f->flags_cap;
    unsigned *b = f->dflags;
    w.in = b; w.out = b + cap; w.xr = b + 2 * cap; w.alive = b + 3 * cap;
    w.selftest = w.alive + 8; w.xcd_arrivals = w.alive + 16; w.queues = w.alive + 64;
    w.abort = (unsigned *)(f->dinfo + 1);
    return w;
}

// The task words of the persistent launch (ddag, DagLaunch) for the handle's step table and a view of mt tile rows: the task
// counter, at + 8 the record of a wait that ran out (7 words), at + 64 tdone, then pdone (pstride words per panel), pall,
// dcount and -- eight cache lines behind everything else -- the XCDs' own task counters; total: words in all.
struct DagWords {
    unsigned *queue, *wait_record, *tdone, *pdone, *pall, *dcount, *xcnt;
    int pstride;
    size_t total;
};
inline DagWords dag_words(const cocons_fit *f, int mt)
{
    DagWords w;
    const size_t T64 = 2 * (size_t)mt, ns = (size_t)f->dag_nsteps;
    const size_t tdone = 64, pdone = tdone + T64 * (T64 + 1) / 2, pall = pdone + (ns + 2) * T64, dcount = pall + ns + 64;
    const size_t xcnt = (dcount + 16 * (ns + 2) + 31) / 32 * 32;
    unsigned *b = f->ddag;
    auto at = [b](size_t off) { return b ? b + off : nullptr; };      // (sized before it is allocated: dag_prepare)
    w.queue = b; w.wait_record = at(8); w.tdone = at(tdone); w.pdone = at(pdone); w.pall = at(pall); w.dcount = at(dcount);
    w.xcnt = at(xcnt);
    w.pstride = (int)T64;
    w.total = xcnt + 8 * 32;
    return w;
}

// The trace buffer (ddag_trace) of a step table with the handle's task count on nt tile columns: 4 stamps per task, 8 stamps
// per tile pair of the engine (room for nt + 2 tiles), then one word of hw_where() pairs per task
struct DagTraceWords {
    unsigned long long *tasks, *engine;
    unsigned *hw;
    size_t engine_count, count;      // elements of the engine's part, of everything
};
inline DagTraceWords dag_trace_words(const cocons_fit *f, int nt)
{
    DagTraceWords w;
    unsigned long long *b = f->ddag_trace;
    const size_t ntasks = f->dag_ntasks;
    w.engine_count = 8 * (size_t)(nt + 2); w.count = 5 * ntasks + w.engine_count;
    w.tasks = b; w.engine = b ? b + 4 * ntasks : nullptr; w.hw = b ? (unsigned *)(w.engine + w.engine_count) : nullptr;
    return w;
}

// The mailboxes (dmbox, every byte 0xff = "not written yet", mbox_reset): one per tile for nt + 2 tiles | one strip mailbox per
// diagonal block (the panel launch's next-diagonal-block update) | the exchange mailboxes of the split panel, one per 64-row
// strip of the matrix and the rows under it.  The accessors return null when the buffer does not hold what is asked for.
inline MboxLayout mbox_layout(int nt, bool panel, bool split)
{
    MboxLayout l;
    l.tiles = ((size_t)nt + 2) * ENGINE_MBOX_DOUBLES;
    l.smb = panel ? ((size_t)nt / 2 + 2) * PANEL_SMBOX_DOUBLES : 0;
    l.xmb = panel && split ? (2 * ((size_t)nt + 2) + 4) * PANEL_XMBOX_DOUBLES : 0;
    return l;
}
inline double *tile_mbox(const cocons_fit *f, int t)
{
    return f->dmbox && ((size_t)t + 1) * ENGINE_MBOX_DOUBLES <= f->mbox.tiles ? f->dmbox + (size_t)t * ENGINE_MBOX_DOUBLES : nullptr;
}
inline double *strip_mbox(const cocons_fit *f, int block)
{
    return f->dmbox && ((size_t)block + 1) * PANEL_SMBOX_DOUBLES <= f->mbox.smb
               ? f->dmbox + f->mbox.tiles + (size_t)block * PANEL_SMBOX_DOUBLES : nullptr;
}
inline double *xchg_mbox(const cocons_fit *f, int nstrips)      // for a panel of nstrips 64-row strips
{
    return f->dmbox && (size_t)nstrips * PANEL_XMBOX_DOUBLES <= f->mbox.xmb ? f->dmbox + f->mbox.tiles + f->mbox.smb : nullptr;
}

int fit_check(cocons_fit *f);

// Every public entry point that works on a handle: validate it, then hold its operation lock until the call returns.
// THREADING CONTRACT (include/cocons_hip.h): one handle serves one call at a time -- a second thread that enters with the
// same handle waits here --; different handles may be used, created and destroyed from different threads concurrently.
// FIT_ENTER: the entries of the dense and taper families -- they refuse a Vecchia handle, which has no factorisation buffer,
// under their own name.  FIT_ENTER_ANY: the entries that serve every kind (streams, the Vecchia entries themselves).
int vecchia_refuse(const char *who);
#define FIT_ENTER_ANY(f)                                               \
    if (int rc__ = fit_check(f)) return rc__;                          \
    std::lock_guard<std::recursive_mutex> op_guard__((f)->op_mu)
#define FIT_ENTER_AS(f, who)                                           \
    if (int rc__ = fit_check(f)) return rc__;                          \
    if ((f)->vecchia) return vecchia_refuse(who);                      \
    std::lock_guard<std::recursive_mutex> op_guard__((f)->op_mu)
#define FIT_ENTER(f) FIT_ENTER_AS(f, __func__)      /* (in an entry's own body: __func__ is its name) */

// nothing under the matrix can be relied on: whoever wrote rows there that the objective does not know of says so
inline void border_unknown(cocons_fit *f) { f->border_clean = -1; f->border_pending = -1; }

// a taper handle's envelope as the launchers take it (null: none, they branch on it), and the tile rows a tile column reaches
inline const int *envelope_or_null(const cocons_fit *f) { return f->taper_hi.empty() ? nullptr : f->taper_hi.data(); }
inline int band_W(const cocons_fit *f) { return f->taper_hi.empty() ? f->nt : f->taper_maxband; }

// Allocate the k buffers of one call (a count of zero: none) or say which allocation failed first -- the sticky error is
// cleared, the caller reports how many bytes its call needs.
inline hipError_t alloc_call_buffers(DevBuf<double> *const *bufs, const size_t *counts, int k)
{
    for (int i = 0; i < k; ++i)
        if (hipError_t e = counts[i] ? bufs[i]->alloc(counts[i]) : hipSuccess) { (void)hipGetLastError(); return e; }
    return hipSuccess;
}

// the matrix a factorisation runs on: column tiles nt, row tiles mt (>= nt: rows under the square)
struct FactorView {
    double *A;
    size_t lda;
    int nt, mt;
    const int *hi = nullptr;   // band-limited factorisation (taper handles): hi[c] = one past the last tile row of tile
                               // column c that can be non-zero in the factor (envelope of the pattern); nullptr = dense
    int skew = 0;              // > 0: A is a packed band buffer (kernels.h band_index) of `skew` tile rows per tile column
    int trim = 0;              // 1: the last 64 of the mt * 128 rows hold nothing (the tile of right-hand sides has at most 64
                               // rows in use): no kernel of the factorisation touches them
    bool dag_ok = false;       // the caller reads the factor through launch_finalize(..., A2 = dP) only: the dependency-driven
                               // schedule may be used (its factor is split over two buffers)
    // the rows of a panel from tile row t0 down to the last row any kernel touches; hb = one past the last band tile row of
    // the panel's 256-column block (api.hip band_hi; -1: dense), behind which only the rows under the matrix follow
    RowRange panel_rows(int t0, int hb) const
    {
        RowRange r;
        r.r0 = t0 * TILE; r.r1 = mt * TILE - 64 * trim; r.band_r1 = hb >= 0 ? hb * TILE : -1; r.ext_r0 = nt * TILE;
        return r;
    }
    // an update launch on this matrix with the same band limit and trim (dense indexing: skew stays 0)
    UpdateLaunch update(int hb) const
    {
        UpdateLaunch u;
        u.C = A; u.ldc = lda; u.band_hi = hb; u.ext0 = nt; u.trim64 = trim;
        return u;
    }
};

// pad0 = 0 while a view that does not start with the handle's observations is factored (every way out): factorize()'s
// front-identity step belongs to the other kind (api_cv.hip: a fold's block; api_predict.hip: the predictive covariance)
struct FoldView {
    cocons_fit *f;
    int pad0;
    explicit FoldView(cocons_fit *f_) : f(f_), pad0(f_->pad0) { f->pad0 = 0; }
    ~FoldView() { f->pad0 = pad0; }
};

// Where the nrhs right-hand-side rows of an evaluation sit -- the ONE place that decides it (enqueue_eval_impl, the replay
// diagnostic and cocons_debug_rhs_layout all ask here):
//   slots   they ride in the slot rows of the matrix's last tile (the handle keeps nslot >= nrhs of them): no rows under it;
//   border  otherwise in tile_rows = ceil(nrhs / 128) tile rows under the matrix (what fit_alloc_matrix makes of rhs_act),
//           and trim says that the last 64 of those rows hold nothing: no kernel of the factorisation touches them.
struct RhsLayout {
    bool slots;
    int tile_rows;
    int trim;
};

// Schedule switches: read from the environment once per process, and settable afterwards through cocons_debug_tune (the
// diagnostics header) so that variants can be timed in alternation inside ONE process on ONE device.
struct Tunables {
    int engine = 1;          // COCONS_ENGINE: 1 = diagonal blocks are factored by the resident engine beside the updates
    int dag = 1;             // COCONS_DAG: 1 = the head of the factorisation under the dependency-driven schedule (one persistent
                             // launch for its updates and panels, dag_kernel); 0 = the classic schedule throughout
    // where a step's panel tasks sit in its list: `lead` far tiles, T1 (+ early halves), `lead2` far tiles, T2, `lead3` far
    // tiles, T3 -- each group about where the chip gets to it when the engine publishes what it waits for (the chip draws ~32
    // tasks per us; first tile out ~85 us into a step, strip (t+1, t) ~18 us later, second tile ~60 us after that), so that
    // the workgroups that draw them neither wait with a slot in hand nor come late.  One block at 3600 (round 4's first
    // form): -1.4 %; at 2400: -0.9 %; everything between (800 .. 2000, 400 .. 900, 1800 .. 2400) measures alike.
    int dag_lead = 1600, dag_lead2 = 600, dag_lead3 = 1800;
    int dag_min_tiles = 2000;  // COCONS_DAG_MIN_TILES: the DAG launch covers the leading steps of at least this many update tiles
                             // (n = 10^4: 24 of the 39 steps, 94 % of the flops; below n ~ 4200 no step at all).  3000 until the
                             // engine became a pair (round 5): with the shorter chain the break-even moved back, 1400 .. 2200
                             // measure alike, +0.4 % over 3000)
    int dag_xcd = 1;         // COCONS_DAG_XCD: 1 = XCD-aware task order of the persistent launch (round 6; chol.hip: dag_position) -- list
                             // positions dealt to the XCDs in chunks of 32, the far tiles of a step dealt so that one XCD's tiles in
                             // flight form one block of dag_bw x dag_bh tiles, a class that falls behind helped by the others: fetched
                             // bytes per launch halve, +2 % evaluations/s at n = 10^4; 0 = one counter for all (rounds 4-5).
                             // dag_order (COCONS_DAG_ORDER): 0 = far tiles column-major as in rounds 4-5
    int dag_order = 1, dag_bw = 16, dag_bh = 16;
    int dag_xcd_min_quota = 128;
    int dag_xcc_quota = -1;  // workgroups of the DAG launch that take part on the engine's XCD (of the 255 that land there; 0: all;
                             // -1: derived from the device, dag_xcc_quota() -- 208 on MI355X)
    int engine_pair = 1;     // COCONS_ENGINE_PAIR: 1 = the engine is a PAIR of workgroups -- the second one follows the first tile's
                             // factorisation column block by column block (strip solve, tile update) and factors the second tile
                             // (chol.hip: engine_partner_loop); 0 = one workgroup does the four passes one behind the other
    int panel_fused = 1;     // COCONS_PANEL_FUSED: 1 = the panel of a two-tile block of the engine schedule is ONE launch whose strips
                             // follow the engine pair's tiles through their mailboxes (chol.hip: panel_pair_kernel); 0, or without
                             // the pair: solve | in-panel update | solve, three launches
    int panel_split = 32;    // COCONS_PANEL_SPLIT: a strip of the one-launch panel is TWO workgroups -- the first follows tile t (X0), the second
                             // follows the first through an exchange mailbox (the in-panel product while X0 is being formed), then tile
                             // t+1 -- in panels of at least this many 64-row strips (0: never, 1: always).  It pays where the panel stands
                             // exposed behind a long update launch (n = 4096: +1.9 %, 6400: +1.5 %, 10^4: +0.6 %) and costs where the engine
                             // is the bound anyway (always on: n = 2116 -4.3 %, n = 1024 -2.2 %); an update of 32 strips' trapezoid is ~30 us
    int potrf_follow = 1;    // COCONS_POTRF_FOLLOW: 1 = a tile factorisation and the panel solve below it are ONE launch whose solve
                             // workgroups follow the factorisation through a mailbox (chol.hip: potrf_follow_kernel; the plain and
                             // the band-limited schedule); 0 = two launches
    int dag_trace = 0;       // (diagnostics) time stamps per task, cocons_debug_dag_trace
    int gate_sabotage = 0;   // (tests) the next N engine-schedule factorisations wait at the gate for a word nobody raises:
                             // a genuine 5 ms time-out, abort code 0x600, to exercise the fall-back and its book-keeping
    // (tests) a LATE HOST: the thread that enqueues a factorisation sleeps host_delay_us microseconds in front of the launches that
    // raise the engine's input word in[host_delay_tile] (COCONS_DEBUG_HOST_DELAY_US / _TILE) -- what a host thread throttled in
    // mid-enqueue looks like to the resident engine (round 5's recorded time-out 0x112) --, and
    // engine_in_wait_ms > 0 puts the bound of the engine's input waits back to that many milliseconds (rounds 2-4: 100)
    int host_delay_us = 0, host_delay_tile = -1, engine_in_wait_ms = 0;
    bool init = false;
};

// What api.hip offers the other translation units (defined and described there) ...
Tunables &tun();
bool engine_enabled();
int fit_alloc_matrix(cocons_fit *f, int rhs_rows);
void assemble_sigma(cocons_fit *f, const double *theta, int which, int col0, int col1);
int assemble_sigma_taper(cocons_fit *f, const double *theta);
int no_taper(cocons_fit *f, const char *who);
void assemble_rhs(cocons_fit *f, const double *mean, bool use_trend, const double *xb, int nxb, int col0, int col1,
                  bool zero_rest = true, bool slots = false);
FactorView main_view(cocons_fit *f);
int flags_reset(cocons_fit *f, int nt);
int mbox_reset(cocons_fit *f, int nt, bool engine_schedule = true);
int factorize(cocons_fit *f, const FactorView &v, std::vector<hipEvent_t> *ev_upd);
int reset_info(cocons_fit *f);
// the checks every information entry makes of its arguments (api_grad.hip): the pointers and the number of directions before
// the handle is entered, the directions' entries (ndir x 6 p, all finite) behind the handle's own checks
int fisher_check_args(const char *who, const cocons_fit *f, const double *theta, int ndir, const double *dirs, const double *info);
int fisher_check_dirs(const char *who, int ndir, const double *dirs, int p);
int info_status(cocons_fit *f);
bool engine_retry(cocons_fit *f, int st);
void dense_collect(cocons_fit *f, double *sum_logliks, double *parts);
int profile_tail(cocons_fit *f, int nxb, double n_eff, bool reml, double *sum_logliks, double *parts);
// ... the evaluation path's internals, offered to the diagnostics (api_diag.hip) only: what the replay and the profile run of
// it, and the time-out report info_status asks api_diag.hip for under COCONS_DEBUG_ABORT
RhsLayout rhs_layout(const cocons_fit *f, int nrhs);
FactorView rhs_view(cocons_fit *f, const RhsLayout &l);
void panel_ops(cocons_fit *f, const FactorView &v, int k, hipStream_t s);
void count_update_flops(cocons_fit *f, int kw, int t0);
int dag_prepare(cocons_fit *f, const FactorView &v);
DagLaunch dag_launch(cocons_fit *f, const FactorView &v, const HandoffWords &hw, const unsigned *alive);
int enqueue_eval(cocons_fit *f, const double *theta, const double *mean, bool use_trend, const double *xb, int nxb,
                 std::vector<hipEvent_t> *ev_upd, bool stage_events);
void debug_abort_report(cocons_fit *f);
// ... what api_handle.hip offers: a handle over given data, a taper handle in a given order, a batch slot's clone
cocons_fit *fit_create_impl(int n, int p, int r, int q, const double *locs, const double *X, const double *z, const double *x_betas,
                            const double *smooth_limits, int device, bool allow_sort, bool defer_matrix = false,
                            bool want_engine = true, bool return_locked = false);
cocons_fit *taper_create_ordered(int n, int p, int r, const double *locs, const double *X, const double *z,
                                 const double *smooth_limits, int device, int nnz, const int *colindices, const int *rowpointers,
                                 const double *taper_entries, const std::vector<int> &perm, bool check_fit);
cocons_fit *clone_for_slot(cocons_fit *f, bool want_engine);
// ... the builder of taper patterns: the refusals every entry that takes (delta, kind) and coordinates shares
// (npts points, column-major npts x 2), and the grid over n targets -- hx, hy: their coordinates on the host (the box), dx,
// dy: on the device -- binned on s (not waited for)
int pattern_check_delta(const char *who, double delta, int kind);
int pattern_check_finite(const char *who, const char *what, size_t npts, const double *pts);
int pattern_grid_build(const char *who, PatternGridBufs &G, int n, const double *hx, const double *hy, const double *dx,
                       const double *dy, double delta, hipStream_t s);
// ... its two halves, for grids whose geometry is made elsewhere (the neighbour search's levels): buffers for grids of up to
// pts points and cells cells, and the first cnt points (dx, dy) binned on the grid g into them on s (not waited for)
int pattern_grid_alloc(const char *who, PatternGridBufs &G, size_t pts, size_t cells);
int pattern_grid_bin(const char *who, PatternGridBufs &G, const PatternGrid &g, int cnt, const double *dx, const double *dy,
                     hipStream_t s);
// ... the Vecchia neighbour search (api_knn.hip): the grid over n points for plain kNN, binned on s (not waited
// for), and the ordered self search of n points on s (drained) into d_nn (n x m column-major, 1-based, nearest first; may be
// null) and d_tab (the layout of VecchiaState::nbr; may be null); phases (may be null: no events are made): the device time
// of the binning and of the query launches, by events on s.  And what api_vecchia.hip offers it: the handle and the
// prediction under the name of the entry that asks, search = true: no table comes in, the neighbours are found on the device
struct KnnPhases {
    double build_ms = 0.0, query_ms = 0.0;
};
int knn_grid_build(const char *who, PatternGridBufs &G, int n, const double *hx, const double *hy, const double *dx,
                   const double *dy, hipStream_t s);
int knn_self_search(const char *who, int n, const double *hx, const double *hy, const double *dx, const double *dy, int m,
                    int *d_nn, int *d_tab, hipStream_t s, KnnPhases *phases = nullptr);
// src (may be null; nn and search are then not looked at): the table is made on the device by the caller of
// vecchia_create_impl and adopted -- make() runs with the handle's data on the device and its stream open, leaves V->nbr and
// V->m (and may attach V->grp), and returns 0 or a failure with the message set; m only bounds the search
struct VecchiaTableSource {
    virtual ~VecchiaTableSource() = default;
    virtual int make(const char *who, cocons_fit *f, const double *locs) = 0;
};
cocons_fit *vecchia_create_impl(const char *who, int n, int p, int r, const double *locs, const double *X, const double *z,
                                const double *smooth_limits, int device, int m, const int *nn, bool search,
                                VecchiaTableSource *src = nullptr);
// corr (may be null; nn_pred and search are then not looked at): the third source of a chunk's table, the neighbours of the
// new locations by model correlation (api_knn_corr.hip) -- the query at width m_cand, the chunk's records, the
// re-ranking into the chunk's table.  With nn_out the table of width m_pred goes home instead of a prediction (mp x m_pred
// column-major, 1-based, largest rho first): mean, z_col, stochastic and quadform are then not looked at.
struct CorrPredSource {
    int m_cand = 0, hops = 0;
    int *nn_out = nullptr;
};
int vecchia_predict_impl(const char *who, cocons_fit *f, const double *theta, const double *mean, int z_col, int mp,
                         const double *locs_pred, const double *X_pred, int m_pred, const int *nn_pred, bool search,
                         double *stochastic, double *quadform, const CorrPredSource *corr = nullptr);
// ... and what api_knn_corr.hip offers it: the shape and theta checks of the correlation entries under the name of the entry
// that asks; what a call at (m_cand, hops) needs on the handle -- the grid and, with two hops, the all-observations table --
// made on s where it is missing (drained where something was made); and one chunk's step on s, not waited for: the query of
// the mc rows at (dlp, dlp + mc) into d_first (mc x m_cand), then the re-ranking with the chunk's records drec and the
// observations' aosC into d_tab (mc x m, the layout of VecchiaArgs::nbr) and d_nn (may be null: mc x m column-major, 1-based,
// largest rho first); the failure word gets row0 + the row of a rho that is not finite
int corr_check_shape(const char *who, int m_cand, int hops, int m);
int corr_check_theta(const char *who, const double *theta, int p);
int vecchia_need_grid(const char *who, cocons_fit *f, hipStream_t s);
int corr_pred_prepare(const char *who, cocons_fit *f, int m_cand, int hops, hipStream_t s);
int corr_pred_chunk(const char *who, cocons_fit *f, const CorrPredSource &c, int m, int mc, int row0, const double *dlp,
                    const double *drec, const double *aosC, double gr, int *d_first, int *d_tab, int *d_nn, hipStream_t s);
// ... and what api_vecchia_group.hip offers api_knn_corr.hip: the grouped handle made on the device
// from a table that `table` leaves in d_tab (n x m, the layout of VecchiaState::nbr) on the handle's stream -- the rounds,
// the plan and the expanded table follow it there; table returns 0 or a failure with the message set
struct GroupedTableStep {
    virtual ~GroupedTableStep() = default;
    virtual int table(const char *who, cocons_fit *f, const double *locs, int m, int *d_tab) = 0;
};
cocons_fit *vecchia_create_grouped_device(const char *who, int n, int p, int r, const double *locs, const double *X,
                                          const double *z, const double *smooth_limits, int device, int m, int max_rows,
                                          int max_rounds, GroupedTableStep &step);
// ... and what api_vecchia.hip offers api_vecchia_sim.hip: the refusal of the other kinds of handle, the
// observations' records for theta (which = 0: cov_rns's parameters) and the info words home with the stream drained (0, or the
// smallest 1-based row whose block failed)
int vecchia_only(cocons_fit *f, const char *who);
ModeSel vecchia_records(cocons_fit *f, const double *theta, int which, double *aos);
int vecchia_status(cocons_fit *f, const char *who);
// ... and what api_vecchia.hip offers api_vecchia_group.hip: the bodies of the value, the whitening,
// the gradient and the information with the launches over observations (grouped = false) or over the plan's blocks, and the
// refusal of a handle without a plan
int vecchia_value_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, const double *mean, double *value,
                       double *parts);
int vecchia_whiten_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, int c, const double *B, double *out,
                        double *logd);
int vecchia_grad_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, const double *mean, int c,
                      const double *B, double *sum_logliks, double *parts, double *grad_theta, double *grad_quad,
                      double *grad_mean);
int vecchia_fisher_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, int ndir, const double *dirs,
                        double *info, double *info_mean);
int vecchia_need_plan(cocons_fit *f, const char *who);
// ... and what api_vecchia_sim.hip offers api_vecchia_cv.hip: the coefficients of the rows n_fixed .. n - 1 for
// theta into the handle's sim->coef and the status word home: 0, the smallest failing 1-based row, or < 0
// grouped: launch_vecchia_group_coefs over the plan's blocks -- the caller has asked vecchia_need_plan -- into
// the same records, the same bits
int vecchia_sim_coefs(cocons_fit *f, const char *who, const double *theta, int n_fixed, bool grouped = false);
// ... and what api_vecchia_sim.hip and api_vecchia_cv.hip offer api_vecchia_cov.hip: the forward schedule of
// (table, n_fixed) on the handle and the forward solve of c columns -- x (n x c in V->W, leading dimension n, its fixed rows in
// place) from the columns in V->B (rows n_fixed .. n - 1, leading dimension n - n_fixed) --, and the transposed lists on the
// handle with the arguments the kernels take them in (the coefficients: V->sim->coef)
int vecchia_sim_schedule(cocons_fit *f, const char *who, int n_fixed);
void vecchia_sim_solve(cocons_fit *f, int n_fixed, int c);
int vecchia_t_build(cocons_fit *f, const char *who);
VecchiaTArgs vecchia_t_args(cocons_fit *f);
// ... and what api_vecchia_sim.hip and api_vecchia_cv.hip offer api_vecchia_group.hip: the bodies of
// cocons_vecchia_unwhiten (timed: cocons_debug_vecchia_sim_phases, ms3 required), cocons_sim_vecchia, cocons_vecchia_whiten_t
// and cocons_cv_vecchia with the coefficient launch over observations (grouped = false) or over the plan's blocks
int vecchia_unwhiten_impl(const char *who, bool grouped, bool timed, cocons_fit *f, const double *theta, int c, const double *W,
                          double *out, double *ms3);
int vecchia_sim_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, const double *mean, int n_fixed, int z_col,
                     int nsim, const double *iiderrors, double *out);
int vecchia_whiten_t_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, int c, const double *W, double *out,
                          double *qdiag);
int vecchia_cv_impl(const char *who, bool grouped, cocons_fit *f, const double *theta, const double *mean, int nfold,
                    const int *fold, double *resid, double *var, long long *stats4);
// ... and what they call in api_shard.hip: the sharded cocons_neg2loglik_dense, and cocons_fit_destroy's share
int sharded_eval(cocons_fit *f, const double *theta, const double *mean, double *sum_logliks, double *parts);
void shard_events_destroy(ShardState *S);
void rccl_comm_destroy(ncclComm_t c);

// ... what api_grad.hip offers api_cv.hip (defined and described there): one gradient operation up to -Sigma^-1 in the leading
// square and Sigma^-1 R in grad->AR (grad_enqueue with full = false), S^-1 on the envelope and S^-1 R in tgrad->AR
// (taper_grad_enqueue with hgrad = null), and the buffers and the layout they run in
size_t grad_lda(const cocons_fit *f, int nb);
int grad_prepare(cocons_fit *f, const char *who, int nb, int pcols = 0);
int grad_enqueue(cocons_fit *f, const double *theta, const double *mean, bool full, double *hgrad);
int taper_refuse(cocons_fit *f, const char *who, const char *dense_entry);
int taper_grad_prepare(cocons_fit *f, const char *who);
int taper_grad_enqueue(cocons_fit *f, const double *theta, const double *mean, double *hgrad);

// f->lda / f->rhs_act in the gradient's layout while one gradient operation runs, the objective's afterwards (every way
// out); the rows under the matrix then hold nothing the objective may rely on (border_clean unknown)
struct GradLayout {
    cocons_fit *f;
    size_t lda;
    int rhs_act;
    GradLayout(cocons_fit *f_, int nb) : f(f_), lda(f_->lda), rhs_act(f_->rhs_act)
    {
        f->lda = grad_lda(f, nb);
        f->rhs_act = (int)(f->lda - (size_t)f->npad);
        border_unknown(f);
    }
    ~GradLayout()
    {
        f->lda = lda; f->rhs_act = rhs_act;
        border_unknown(f);
    }
};

// One operation of a one-shot entry that factors on the handle: enqueue() puts everything of it but the info words on the
// handle's stream (assembly, factorisation, the entry's own kernels and result copies; 0 or an error); it is run again after a
// hand-off time-out.  0, a failing minor or an error.
template <class F> int run_op(cocons_fit *f, const char *who, F &&enqueue)
{
    for (;;) {
        if (int rc = reset_info(f)) return rc;
        if (int rc = enqueue()) return rc;
        HIPCHK_AT(who, hipMemcpyAsync(f->hinfo, f->dinfo, 2 * sizeof(int), hipMemcpyDeviceToHost, f->stream));
        HIPCHK_AT(who, hipGetLastError());
        HIPCHK_AT(who, hipStreamSynchronize(f->stream));
        const int st = info_status(f);
        if (!engine_retry(f, st)) return st;
    }
}

// the band schedule is a plain one: no resident engine while one of these is alive
struct PlainSchedule {
    cocons_fit *f; bool ok;
    explicit PlainSchedule(cocons_fit *f_) : f(f_), ok(f_->engine_ok) { f->engine_ok = false; }
    ~PlainSchedule() { f->engine_ok = ok; }
};

// S(theta) of a taper handle assembled, border_rows() -- the caller's rows under the matrix --, and the factorisation on the
// band schedule, which leaves the factor whole in dA for the pack launches that follow (cocons_krige_taper_prepare,
// cocons_fisher_taper).  A handle without an envelope (COCONS_TAPER_BAND=0) takes that schedule too, with the plan's
// hi[c] = nt: the same operations on every tile of the true band as under an envelope -- the tiles outside it only ever
// receive products with exact zeros -- so every layout prepares the same bits.
// (Not for the selected inverse -- taper_grad_enqueue, i.e. the tapered gradient and cocons_cv_taper --: that path factors
// main_view(f) as the objective does, on whatever schedule the handle has, and must stay so.)
template <class F> int factor_on_band_schedule(cocons_fit *f, const double *theta, const BandPlan &pl, F &&border_rows)
{
    PlainSchedule plain(f);
    if (int rc = assemble_sigma_taper(f, theta)) return rc;
    border_rows();
    FactorView v = main_view(f);
    v.hi = pl.hi.data();                // (the handle's own envelope where it has one)
    return factorize(f, v, nullptr);
}

constexpr double LOG_2PI = 1.8378770664093454835606594728112;

#pragma GCC visibility pop
