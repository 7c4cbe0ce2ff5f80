// kernels.h -- argument blocks and launchers shared by the HIP sources and the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <atomic>
#include <vector>
#include "../../include/cocons_hip.h"
#include "pattern_grid.hpp"

namespace cocons {

enum SmoothKind : int {
    SMOOTH_ZERO = 0,           // fixed-smoothness branch: vector stays zero (cocons_full.cpp:83-88)
    SMOOTH_LOGISTIC_SQRT = 1,  // sqrt(Pexpfma_new_smoothness) (:93)
    SMOOTH_EXP = 2             // classic: Pexpfma_new(smooth) (:524)
};

// theta-derived coefficient vectors, formed on the host exactly as the reference forms
// them (2*scale_je, 2*scale_je+aniso, 0.5*std.dev; cocons_full.cpp:64-66,101-104) and
// passed by value in the kernel-argument segment (no per-evaluation H2D copy).
struct ThetaVecs {
    double tilt[COCONS_P_MAX];
    double two_scale_je[COCONS_P_MAX];
    double aniso[COCONS_P_MAX];
    double sqrt_vector[COCONS_P_MAX];
    double half_sd[COCONS_P_MAX];
    double nugget[COCONS_P_MAX];
    double smooth[COCONS_P_MAX];
    double sd[COCONS_P_MAX];
};

struct LocArgs {
    int n, p;
    const double *X; int ldx;       // n x p column-major
    const double *locs; int ldl;    // n x 2 column-major
    double *out; size_t stride;     // LOCP_FIELDS x stride SoA
    int smooth_kind;
    double smooth_min, smooth_max;
    ThetaVecs th;
};

struct PairArgs {
    int n;                 // number of (column-side) locations
    int m;                 // rect only: number of row-side locations
    const double *rows;    // SoA of the row side (== cols for the symmetric kernel)
    const double *cols;    // SoA of the column side
    size_t stride;         // SoA stride of the column side (and rows for sym)
    size_t stride_rows;    // SoA stride of the row side (rect)
    double *out; size_t ld;
    int nrows_out, ncols_out;   // extent to write (>= n pads with identity / zeros)
    int bj0;               // sym: first 64-wide tile column to assemble (sharded path), else 0
    int H;                 // sym: tile rows of the trapezoid (set by the launcher)
    int blocked;           // sym: 8 x 8 pair patches per wave step (set by the launcher, Bessel modes)
    double gr;             // global_range
    double nu_fixed;       // closed-form modes
    double pad_diag;       // sym: diagonal of the identity padding beyond n (0 = the default, 1.0)
    // sym, sharded evaluation: only the tile ROWS of the 256-row blocks this rank owns are assembled -- block b belongs to
    // rank (b / own_group) % own_world (own_world <= 1: every row)
    int own_world = 0, own_rank = 0, own_group = 1;
};

struct RhsArgs {
    int n, p;
    const double *X; int ldx;
    double mean[COCONS_P_MAX];
    int use_trend;
    const double *src; int lds;     // n x nrows column-major (z or x_betas)
    double *out; size_t ld;
    int row0, nrows;       // nrows source rows, written at out rows row0..
    int nrows_zero;        // further rows (row0+nrows ..) cleared to zero
    int col0, ncols_out;   // column range [col0, ncols_out)
    int skew, npad;        // packed band target (band_index): 0 = dense
};

void launch_loc_params(const LocArgs &a, hipStream_t s);
void launch_pair_sym(int mode, bool mirror, const PairArgs &a, hipStream_t s);
void launch_pair_rect(int mode, const PairArgs &a, hipStream_t s);
void launch_rhs_rows(const RhsArgs &a, hipStream_t s);
// entries of the sparse/taper covariance for a CSR pattern (1-based indices, device arrays): see TaperArgs (assemble.hip)
struct TaperLaunch {
    int mode = 0; bool pred = false;             // PairMode; pred: rows = prediction locations (always MODE_GEOM)
    int nrows = 0, nnz = 0; const int *ci = nullptr, *rp = nullptr;
    const double *rows = nullptr; size_t stride_rows = 0;   // SoA of the row side
    const double *cols = nullptr; size_t stride = 0;        // SoA of the column side (observations)
    double nu_fixed = 0.0; double *out = nullptr;           // out: one value per entry, unless A is given:
    const double *tapv = nullptr; double *A = nullptr; size_t lda = 0; int row0 = 0;    // dense target, see TaperArgs
    int skew = 0, npad = 0;                      // packed band target (band_index)
};
void launch_taper(const TaperLaunch &t, hipStream_t s);
// zero the tiles inside the envelope (d_hi: device copy of FactorView::hi; max_band = max over c of hi[c] - c)
void launch_band_zero(double *A, size_t lda, const int *d_hi, int nt, int max_band, hipStream_t s, int skew = 0);
// identity on the padding diagonal of a taper handle's buffer
void launch_front_identity(double *A, size_t lda, int pad0, int rows, hipStream_t s);   // columns [0, pad0): unit vectors
void launch_pad_identity(double *A, size_t lda, int n, int npad, hipStream_t s, int skew = 0);
// rows idx[0..nidx) of the dense covariance (cor != 0: of cov2cor of it); out row b at out + b * n
void launch_cov_rows(int mode, int n, int nidx, const int *idx, const double *loc, size_t stride, double gr,
                     double nu_fixed, int cor, double *out, hipStream_t s);
// out[i] = 2^(1-nu)/Gamma(nu) u^nu K_nu(u) by the device routine of the pair kernels (diagnostic)
void launch_matern_points(int n, const double *nu, const double *x, double *out, hipStream_t s);

// ---- factorisation (chol.hip) -------------------------------------------------
constexpr int TILE = 128;          // tile edge of the blocked factorisation

// Packed band storage of a band-limited factorisation (taper handles): tile column c (128 columns) keeps only the rows
// the factor can touch -- `skew` tile rows from its diagonal tile down, then the rows under the matrix -- so the leading
// dimension is skew * 128 + (rows under the matrix) instead of the matrix order, and element (i, j) sits at
//     i_local + j * ld,   i_local = i - 128 (j / 128)  for a row of the matrix (i < npad),
//                                   skew * 128 + (i - npad)  for a row under it.
// skew = 0: the ordinary dense layout.  Kernels that work inside ONE tile column get a shifted base pointer
// (band_base) and keep their global row indices; the rows under the matrix then start at row (c + skew) * 128.
__host__ __device__ inline size_t band_index(int i, int j, size_t ld, int skew, int npad)
{
    if (skew == 0) return (size_t)i + (size_t)j * ld;
    const int il = i < npad ? i - TILE * (j / TILE) : skew * TILE + (i - npad);
    return (size_t)il + (size_t)j * ld;
}
// base pointer with which tile column c of a packed band buffer is addressed by GLOBAL row and column indices
inline double *band_base(double *A, int c, int skew) { return skew ? A - (ptrdiff_t)TILE * c : A; }

// Factor the 128x128 diagonal tile at (c0,c0) in place (lower), write the inverses of
// its eight 16x16 diagonal blocks to dinv (8*256 doubles).  info: atomicMin of the
// 1-based failing column (initialise to INT_MAX).
void launch_potrf_tile(double *A, size_t lda, int c0, double *dinv, int *info, hipStream_t s);
// Rows [r0, r1) of a panel, or -- band_r1 >= 0, band-limited factorisation -- [r0, band_r1) and [ext_r0, r1); strips(): its
// 64-row strips in the first stretch (the band) and in the second (the rows under the matrix)
struct RowRange {
    int r0 = 0, r1 = 0, band_r1 = -1, ext_r0 = 0;
    void strips(int &nb1, int &nb2) const
    {
        nb1 = ((band_r1 >= 0 ? band_r1 : r1) - r0) / 64; nb2 = band_r1 >= 0 ? (r1 - ext_r0) / 64 : 0;
        if (nb1 < 0) nb1 = 0;
        if (nb2 < 0) nb2 = 0;
    }
};
// Resident diagonal-BLOCK engine (one workgroup on a CU of its own) for the 256 x 256 diagonal blocks
// starting at tile t0 (even): see potrf_engine_kernel.  Flag words, all zero at launch:
//   in[t]    raised by the update kernels (launch_update's sig / sig_tile): 3 = tile (t,t) updated;
//   in[t+1]  7 = tiles (t+1,t) and (t+1,t+1) updated;
//   out[t], out[t+1]  raised to 1 when the factor of that diagonal tile (and its Q operands in
//                     dinv + (tile & 1) * 2048) is published;
//   xr[t]    raised to 1 when X = A(t+1,t) L(t)^-T is published.
// abort_word: set by any party whose bounded wait ran out; everybody leaves when it is non-zero.
//   alive    raised by the engine once it is resident; launch_start_gate(alive, ...) holds a stream until then
// wbuf, pbuf != NULL: the engine of the DAG schedule (launch_dag) -- it also publishes W = L^-1 of every diagonal tile t at
// wbuf + t * 128 * 128 (zeroed once by the caller; complete before out[t]) and a second copy of X in pbuf (shaped like A)
struct EngineLaunch {
    double *A = nullptr; size_t lda = 0; int t0 = 0, nt = 0;
    double *dinv = nullptr; int *info = nullptr; unsigned *in = nullptr, *out = nullptr, *xr = nullptr, *abort_word = nullptr, *alive = nullptr;
    double *wbuf = nullptr, *pbuf = nullptr; int dag_until = 0; unsigned long long *trace = nullptr;
    double *mbox = nullptr;    // pair mode (engine_partner_loop): the tiles' mailboxes (ENGINE_MBOX_DOUBLES each, index = tile), every
                               // byte 0xff at launch; a second workgroup takes the second tile of every block
    int in_wait_ms = 0;        // > 0 (tests): bound of the engine's waits for its input words in milliseconds, not the host-paced 3 s
};
void launch_potrf_engine(const EngineLaunch &e, hipStream_t s);
// the WARM-UP launch (chol.hip): no tile at all, the kernel raises e.alive and leaves; e: dinv, info and the words; dag: which instantiation
void launch_potrf_engine_warmup(EngineLaunch e, bool dag, hipStream_t s);
// Abort codes of the bounded hand-off waits (the abort word behind the info word: who gave up).  CLASS in bits 8..11, an index
// -- the tile or, for the persistent launch, the step -- in the low byte, masked so that no index can spill into another class
// (until round 5 the engine's partner reported 0x700 + tile while the followers used the fixed codes 0x7d0 / 0x7e0 / 0x7f0: from
// tile 208 on a partner's time-out read as a follower's).  One decoder for the host: abort_class().
//   0x100 / 0x200  engine waiting for in[t] / in[t+1] (host-paced)      0x300  panel solve waiting for the engine's tile
//   0x400  split panel's second workgroup waiting in its exchange mailbox   0x500  in-panel update waiting for xr[t]
//   0x600  start-up gate (engine / partner not resident)                 0x700  the engine's partner following tile t
//   0x800  a follower of potrf_follow_kernel (plain / band-limited schedule)  0x900  the reductions waiting for the last tile
//   0xa00 .. 0xe00  waits of the persistent launch (dag_kernel: index = step)  0xf00  next-diagonal-block workgroups of the
//   panel launch waiting in the strip mailbox
constexpr unsigned ABORT_ENGINE_IN0 = 0x100u, ABORT_ENGINE_IN1 = 0x200u, ABORT_PANEL = 0x300u, ABORT_XCHG = 0x400u, ABORT_INPANEL = 0x500u,
                   ABORT_GATE = 0x600u, ABORT_PARTNER = 0x700u, ABORT_FOLLOW = 0x800u, ABORT_LAST_TILE = 0x900u, ABORT_STRIPBOX = 0xf00u,
                   ABORT_DAG_FIRST = 0xa00u, ABORT_DAG_LAST = 0xe00u;      // (the classes of the persistent launch: a range)
__host__ __device__ inline unsigned abort_code(unsigned cls, unsigned index) { return cls | (index & 0xffu); }
inline unsigned abort_class(unsigned code) { return code & 0xf00u; }
constexpr size_t ENGINE_MBOX_DOUBLES = 44 * 256;
// the start-up gate holds the stream until the engine is resident (chol.hip; patient: a handle's first engine-schedule operation)
// nhelp > 0: also waits until that many further workgroups of the engine's launch (the pair partner) are resident
// raise_in != NULL: the gate also raises in[0] = 3, in[1] = 7 (the engine factors the first diagonal block too: launch_potrf_engine t0 = 0)
void launch_start_gate(unsigned *alive, unsigned *abort_word, bool patient, int nhelp, unsigned *raise_in, hipStream_t s);
void launch_last_tile_gate(unsigned *out_word, unsigned *abort_word, hipStream_t s);   // the reductions' wait for the engine's LAST tile
void launch_raise_word(unsigned *word, hipStream_t s);      // *word = 1 (agent scope) by a one-lane kernel: "everything in front of me on this stream is done"
// 1: a kernel on `first` and a kernel launched behind it on `second` overlap (the streams sit on different hardware queues);
// 0: they run one after the other; -1: HIP error.  words: two device words; both streams idle.
int streams_run_concurrently(hipStream_t first, hipStream_t second, unsigned *words);
// rows x cols [c0, c0+128):  X <- X * L(c0)^{-T}, L read from A(c0,c0).
// wait_word != NULL: the tile comes from the engine -- every workgroup first waits for *wait_word >= 1
// own_world > 1 (sharded evaluation): only the 64-row strips inside 256-row blocks b with (b / own_group) % own_world == own_rank
struct TrsmLaunch {
    double *A = nullptr; size_t lda = 0; int c0 = 0; RowRange rows;
    double *dinv = nullptr; unsigned *wait_word = nullptr, *abort_word = nullptr;
    int own_world = 0, own_rank = 0, own_group = 1;
    int *info = nullptr; double *mbox = nullptr;      // launch_potrf_follow only
};
void launch_trsm_tile(const TrsmLaunch &l, hipStream_t s);
// launch_potrf_tile (info) and launch_trsm_tile (dense, unsharded, no wait_word) in ONE launch: the solve workgroups follow the
// factorisation through the tile's mailbox mbox (ENGINE_MBOX_DOUBLES doubles, every byte 0xff beforehand); bit-identical to the two
void launch_potrf_follow(const TrsmLaunch &l, hipStream_t s);
// The panel of a two-tile block of the engine schedule in one launch: rows [r0, r1) of the tile columns at c0 and c0 + 128,
// X0 = B0 L(c0)^-T | B1 -= X0 X(t+1,t)^T | X1 = B1 L(c0+128)^-T (dense, unsharded: rows.band_r1 is not read).  The strips follow
// the two tiles through their mailboxes mb0, mb1 (the engine's pair mode) and the in-panel product waits for xr.  Bit-identical
// to launch_trsm_tile | launch_update (K = 128) | launch_trsm_tile.
struct PanelLaunch {
    double *A = nullptr; size_t lda = 0; int c0 = 0; RowRange rows;
    unsigned *xr = nullptr, *abort_word = nullptr; const double *mb0 = nullptr, *mb1 = nullptr;
    double *smb = nullptr; int ndiag = 0; unsigned *sig = nullptr; int sig_tile = 0;   // see PANEL_SMBOX_DOUBLES
    double *xmb = nullptr;     // split panel: exchange mailboxes, PANEL_XMBOX_DOUBLES per 64-row strip, every byte 0xff (the second
                               // workgroup of a strip puts the pattern back as it reads)
};
void launch_panel_pair(const PanelLaunch &l, hipStream_t s);
constexpr size_t PANEL_XMBOX_DOUBLES = 8 * 4 * 256;
// smb (PANEL_SMBOX_DOUBLES doubles, every byte 0xff beforehand) + ndiag = 10 or 3: the launch also updates the NEXT diagonal
// block (two tiles or one) with this panel and raises sig[sig_tile] (+3) / sig[sig_tile + 1] (+7) like launch_update's tiles
// inside the diagonal block do; the update launch that follows must leave those tiles alone (skip_lo / skip_hi)
constexpr size_t PANEL_SMBOX_DOUBLES = 4 * 16 * 4 * 256;
// C(i,j) -= sum_{k < K} P(i,k) P(j,k) for tiles with tile-row in [ti0,ti1), tile-col in [tj0,tj1); lower_only keeps
// ti >= tj.  All tile indices in units of TILE.
struct UpdateLaunch {
    double *C = nullptr; size_t ldc = 0;
    const double *P = nullptr; size_t ldp = 0; int kblk = 0;   // the panel: element (row, k) at P[row + k * ldp]; packed band: tile column kblk
    void panel_in_c(int k0) { P = C + (size_t)k0 * ldc; ldp = ldc; kblk = k0 / TILE; }   // ... = columns [k0, k0 + K) of C itself
    int K = 0, ti0 = 0, ti1 = 0, tj0 = 0, tj1 = 0; bool lower_only = false;
    int band_hi = -1, ext0 = 0;    // band_hi >= 0: tile rows [ti0, band_hi) and [ext0, ti1)
    int skew = 0;                  // packed band buffer (band_index; with band_hi / ext0): C is its unshifted base
    int trim64 = 0;                // 1: the last 64 rows of the row range hold nothing (a half-used tile of right-hand sides): not updated
    int skip_lo = 0, skip_hi = 0;  // tiles with both 64-row and 64-column index in [skip_lo, skip_hi) are left alone (the next
                                   // diagonal block, when the panel's launch or -- sharded -- its owner has updated it already)
    unsigned *sig = nullptr; int sig_tile = -1;             // hand-off to the engine: its in[] array, even tile of the diagonal block
    unsigned *wait_word = nullptr, *abort_word = nullptr;   // an operand tile comes from the engine: wait for *wait_word >= 1 first
    unsigned *queue = nullptr;     // a device word, ZERO at launch: about as many workgroups as the chip holds then draw the tiles of
                                   // the trapezoid from that counter (lower_only launches)
    // sharded path, world > 1: only tiles whose ROW lies in a 256-row block b with (b / group) % world == rank; pmap (device, one
    // int per 64-row tile, null = global row index): element offset of that tile's rows in the owner-packed panel P (api_shard.hip)
    int group = 1, world = 1, rank = 0; const int *pmap = nullptr;
};
void launch_update(const UpdateLaunch &u, hipStream_t s);
// waves per workgroup of the trailing-update kernel: 4 or 8 (512 threads, KC = 16: half the tile latency; default for
// launches of at most set_update_w8_max_tiles tiles, 0 = every launch)
void set_update_waves(int nw);
void set_update_w8_max_tiles(int ntiles);
void set_update_c_wt(int on);           // (experiment) every C tile through L2-bypassing loads and write-through stores
int device_cus();                                           // CUs of the device (asked once per process)
inline int resident_slots() { return 8 * device_cus(); }    // the chip holds 8 workgroups of the update and DAG kernels on each
// the attribute that allows more than 64 KB of dynamic LDS is per kernel and device: set once, not per launch
inline void set_dynamic_lds_once(const void *kernel, size_t bytes, std::atomic<unsigned long long> &done_mask)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < 64 && ((done_mask.load(std::memory_order_relaxed) >> dev) & 1ull)) return;
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (dev >= 0 && dev < 64) done_mask.fetch_or(1ull << dev, std::memory_order_relaxed);
}
// sharded evaluation: the solved rows this rank owns of the 256-column panel at column col0 (ncols columns), gathered into
// its slot of the owner-packed exchange buffer: for every 64-row tile ti in [ti_lo, ti_hi) with pmap[ti] inside the slot
// [slot_lo, slot_hi): dst[pmap[ti] + rho + c * ldp] = A[(64 ti + rho) + (col0 + c) lda]
void launch_pack_rows(const double *A, size_t lda, int col0, int ncols, double *dst, size_t ldp, const int *pmap, int ti_lo,
                      int ti_hi, long long slot_lo, long long slot_hi, hipStream_t s);

// ---- dependency-driven schedule (chol.hip: dag_kernel) -- ONE persistent launch for every trailing update and every
// panel behind the first one.  DagStepHost mirrors the device record (see DagStep in chol.hip for the meaning).
struct DagStepHost {
    unsigned base, near, tpos, nT;
    int H, W, tj0, k0, K, nstrip, two, need, nd_next, split;
    unsigned p2, p3;
};
// only the leading steps with at least min_tiles update tiles are taken (the head of the factorisation); the last of them has
// no panel tasks: the panel behind it is left to the caller's classic kernels
// the diagonal-block tiles of the steps from 1 on are computed in two halves (nd_next / split, see DagStep)
// lead: far tiles of a step in front of its T1 tasks (and the early halves); lead2 / lead3: far tiles between them and the T2
// tasks, between those and the T3 tasks
unsigned dag_build_steps(int nt, int mt, int trim64, int kskip, int lead, int min_tiles, std::vector<DagStepHost> &out,
                         int lead2 = 0, int lead3 = 0,
                         std::vector<unsigned> *ftab = nullptr,    // out: which tile every FAR tile task is (launch_dag's ftab; chol.hip:
                                                                   // dag_build_far_table) for tasks dealt to the XCDs in chunks of
                         int xcd_g = 0, int bw = 16, int bh = 16); // 2^xcd_g list positions (0: one counter), blocks of bw x bh tiles
// steps: DEVICE copy of the table.  queue, tdone (2 mt (2 mt + 1) / 2 words), pdone ((nsteps + 1) * pstride words,
// pstride >= 2 mt), pall (nsteps + 1 words): zero at launch.  sig / out / xr: the engine's words (EngineLaunch with wbuf = Wt, pbuf = P).
struct DagLaunch {
    double *A = nullptr; size_t lda = 0; double *P = nullptr; const double *Wt = nullptr;
    const DagStepHost *steps = nullptr; int nsteps = 0; unsigned ntasks = 0;
    unsigned *queue = nullptr, *tdone = nullptr, *pdone = nullptr; int pstride = 0; unsigned *pall = nullptr;
    double *partbuf = nullptr; unsigned *dcount = nullptr;   // 2 x 16 x 64 x 64 doubles; 16 words per step (+ 1 step), zero at launch
    unsigned *sig = nullptr, *out = nullptr, *xr = nullptr, *abort_word = nullptr;
    unsigned long long *trace = nullptr; unsigned *hw = nullptr;      // diagnostics (hw only with trace)
    const unsigned *alive = nullptr; int xcc_quota = 0;   // the engine's alive word (1 + its XCD); workgroups that take part on that XCD
    const unsigned *ftab = nullptr; int xcd_g = 0;        // DEVICE copy of dag_build_steps' far-tile table; chunk exponent
    unsigned *xcnt = nullptr;              // the XCDs' task counters: 8 x 32 words (a cache line each), zero at launch
};
void launch_dag(const DagLaunch &d, hipStream_t s);

// ---- what is made of a finished factor (solve.hip): reductions, draws, kriging ---------------------------------------------
// reductions: out[0] = sum_{i<n} log(A(i,i)); out[1 + a*nr + b] = sum_{c<n} A(row0+a,c) A(row0+b,c)
void launch_finalize(const double *A, size_t lda, int n, int row0, int nr, double *out, hipStream_t s,
                     int skew = 0, int npad = 0,           // packed band source (band_index)
                     const double *A2 = nullptr,           // factor of the DAG schedule: below the diagonal blocks the columns
                     int a2_cols = 0);                     // [256, a2_cols) live in A2
// partial version over columns [c0,c1) accumulating into out (atomic adds), sharded path
void launch_finalize_cols(const double *A, size_t lda, int c0, int c1, int n, int row0, int nr,
                          double *out, hipStream_t s);
// per-row reductions for predict: stoch[i] = sum_c A(rowy,c) A(row0+i,c); quad[i] = sum_c A(row0+i,c)^2
// deterministic two-stage reduction; scratch must hold row_reduce_scratch_doubles(n, m) doubles
size_t row_reduce_scratch_doubles(int n, int m);
void launch_row_reduce(const double *A, size_t lda, int n, int rowy, int row0, int m,
                       double *stoch, double *quad, double *scratch, hipStream_t s, int skew = 0, int npad = 0,
                       const double *A2 = nullptr, int a2_cols = 0);   // factor of the DAG schedule, as for launch_finalize

// Y = L E + trend (lower factor L in A), E n x nsim, Y n x nsim
void launch_trmm_lower(const double *A, size_t lda, int n, const double *E, int lde, int nsim,
                       const double *trend, double *Y, int ldy, hipStream_t s);
// the same for the factor of a band-limited factorisation (taper handles): A as the factorisation leaves it -- packed band
// (skew > 0) or dense (skew = 0) --, d_hi the device copy of its envelope (FactorView::hi; nullptr = every tile c <= I),
// nt tile columns; reads only tiles inside the envelope, only the lower triangle of diagonal tiles, only rows < n of E.
// Each band tile is read once per 64 draws; the sum order is fixed (bit-identical launches).
void launch_band_trmm(const double *A, size_t lda, int skew, int npad, const int *d_hi, int nt, int n, const double *E,
                      int lde, int nsim, const double *trend, double *Y, int ldy, hipStream_t s);
// Kriging from a held factor (cocons_krige_*).  pack: the lower tiles of the factor in A (nt x nt tiles) into Lp
// (nt (nt + 1) / 2 tiles of 128 x 128, tile (I, J) at I (I + 1) / 2 + J, diagonal tiles' upper triangle zero), the
// triangular-solve operands of every diagonal tile into Qp (nt x 2048) and w[c] = A(rowy, c) for c in [c_lo, c_hi), else 0
// (npad doubles).  solve: V = C L^-T for rows [0, rows) of C (column-major, ld ldc >= rows rounded up to 64, npad columns;
// V overwrites C), stoch[i] = V(i,:) w, quad[i] = V(i,:) V(i,:)'; columns outside [c_lo, c_hi) count as zero.  Rows are
// independent and every sum order is fixed (bit-identical per row whatever else the chunk holds).
void launch_krige_pack(const double *A, size_t lda, int nt, int rowy, int c_lo, int c_hi, double *Lp, double *Qp, double *w,
                       hipStream_t s);
void launch_krige_solve(const double *Lp, const double *Qp, const double *w, int nt, double *C, size_t ldc, int rows,
                        int c_lo, int c_hi, double *stoch, double *quad, hipStream_t s);
// Kriging from a held band factor (cocons_krige_taper_*).  band_pack: the envelope's lower tiles of the factor in A
// (band_index layout; d_hi: device copy of the envelope, null = hi[c] = nt; W = max_c (hi[c] - c)) into Lp, tile (I, J) at tile
// index d_toff[J] + (I - J) (d_toff: device, nt ints), the operands of every diagonal tile into Qp (nt x 2048) and
// w[c] = A(npad, c) for c < n, else 0 (npad doubles).
void launch_krige_band_pack(const double *A, size_t lda, int skew, int npad, int n, const int *d_hi, int nt, int W,
                            const int *d_toff, double *Lp, double *Qp, double *w, hipStream_t s);
// load: one ring slot (128 columns of ldr rows) zeroed, then slot[dst[k]] = tapv[src[k]] * val[src[k]] for k < count
// (dst = row + column in the tile * ldr, all different)
hipError_t launch_krige_band_load(double *slot, size_t ldr, const int *dst, const int *src, int count, const double *val,
                                  const double *tapv, hipStream_t s);
// band_solve: V = C L^-T for the `rows` rows of a sparse chunk C through a ring of W slots (rows x W * 128 doubles, ld ldr >=
// rows rounded up to 64), stoch[i] = V(i,:) w, quad[i] = V(i,:) V(i,:)'.  The chunk's entries are bucketed by tile column:
// bucket I = the entries boff[I] .. boff[I + 1] of bdst / bsrc (device; boff, toff and hi are HOST arrays, hi null = nt).
// Rows are independent and every sum order is fixed.
// Joint prediction (cocons_krige_taper_joint) sets the last three lines: the ring then has Wr = min(W + depth - 1, nt) slots
// (tile column I in slot I mod Wr; the live window and the loads stay those of W), so a solved tile column survives
// depth - 1 further steps, and behind the diag launch of the last tile column of every group of `depth` consecutive tile
// columns (and of the last, possibly partial, group) one launch does S -= V_g V_g' over the lower tiles of S
// (krige_band_schur_kernel; S: round_up(rows, 128) rows and columns, ld lds; ldr = round_up(rows, 64) exactly).  The slot
// the load of step J takes over held tile J - depth, whose group ended at step <= J - 1.  Every element of S sees the
// tile columns in ascending order whatever the depth: S does not depend on it to the bit.  Unset: the plain ring, no product.
// One 64 x 128 block of a fold-aware Gram product: ring rows [row0, row0 + 64) against ring rows [col0, col0 + 128) -- both
// inside one fold, or one 128-row tile of packed small folds -- added to the block at blocks + dst, leading dimension ld.
struct KrigeGramTask { int row0, col0, ld, pad; long long dst; };
struct KrigeBandSolve {
    const double *Lp = nullptr, *Qp = nullptr, *w = nullptr;
    const int *toff = nullptr, *hi = nullptr; int nt = 0, W = 0;
    double *ring = nullptr; size_t ldr = 0; int rows = 0;
    const int *boff = nullptr, *bdst = nullptr, *bsrc = nullptr;
    const double *val = nullptr, *tapv = nullptr;
    double *stoch = nullptr, *quad = nullptr;
    int Wr = 0;                    // slots of the ring (0: W)
    int depth = 0;                 // tile columns per Schur launch (with S)
    double *S = nullptr; size_t lds = 0;
    // cross-validation by folds (cocons_cv_taper_folds) sets these in place of S: the product of every group goes to the
    // blocks of `tasks` (device, ntasks of them) inside `blocks` instead of one dense S -- D += V_g(strip, :) V_g(tile, :)'
    // (krige_band_gram_kernel), nothing between rows of different tasks' tiles; Wr and depth as with S
    const KrigeGramTask *tasks = nullptr; int ntasks = 0;
    double *blocks = nullptr;
};
hipError_t launch_krige_band_solve(const KrigeBandSolve &a, hipStream_t s);
// schur: S(I, J) -= V(I, :) V(J, :)' over the lower 128 x 128 tiles of S (round_up(m, 128) rows and columns, column-major,
// ld lds), V as launch_krige_solve leaves it (m rows, ld ldv >= round_up(m, 64), npad columns, zero outside [c_lo, c_hi));
// rows >= m of V count as zero.  K runs from c_lo's tile to npad in one fixed order per element: bit-identical launches,
// and the leading block of S does not depend on m.  The upper triangle of S's diagonal tiles is overwritten with values
// nobody may read; launch_sym_mirror then makes the upper triangle of the leading n x n block the mirror of the lower one.
void launch_krige_schur(const double *V, size_t ldv, int m, int c_lo, int c_hi, int npad, double *S, size_t lds, hipStream_t s);
void launch_sym_mirror(double *S, size_t lds, int n, hipStream_t s);
// out[i + s ldo] = Y[pos[i] + s ldy] for i < n, s < ncol
void launch_gather_rows(const double *Y, int ldy, const int *pos, int n, int ncol, double *out, int ldo, hipStream_t s);

// ---- taper patterns from delta (pattern.hip) -----------------------------------------------------------------
// The taper of an entry at distance d, h = d / delta in [0, 1] -- spam's cov.wend1, cov.wend2 and cov.sph with
// theta = c(delta, 1) --, by plain products:
//   COCONS_TAPER_WEND1   (1 - h)^4 (4 h + 1)
//   COCONS_TAPER_WEND2   (1 - h)^6 (35 h^2 + 18 h + 3) / 3
//   COCONS_TAPER_SPH     1 - 1.5 h + 0.5 h^3
__host__ __device__ inline double pattern_taper_value(int kind, double h)
{
    const double u = 1.0 - h, u2 = u * u;
    if (kind == COCONS_TAPER_WEND1) return (u2 * u2) * (4.0 * h + 1.0);
    if (kind == COCONS_TAPER_WEND2) return ((u2 * u2) * u2) * (((35.0 * h) * h + 18.0 * h) + 3.0) / 3.0;
    return (1.0 - 1.5 * h) + (0.5 * h) * (h * h);
}
// The targets of a search, binned (launch_pattern_bin): the grid, the points (x, y: n each), and the cell-sorted list --
// cstart (nx ny + 1: first place of every cell), sidx (n: the point at every place) and its coordinates sx, sy.
struct PatternTargets {
    PatternGrid g;
    int n = 0;
    const double *x = nullptr, *y = nullptr;
    int *cstart = nullptr, *sidx = nullptr;
    double *sx = nullptr, *sy = nullptr;
};
inline size_t pattern_cells(const PatternGrid &g) { return (size_t)g.nx * (size_t)g.ny; }
// out[i] = base + in[0] + .. + in[i - 1] for i <= n (n + 1 outputs; out may be in), *total (device, may be null) = the sum in
// 64 bits -- the outputs are ints and mean nothing when it passes INT_MAX.  One workgroup, a fixed order.
hipError_t launch_scan_exclusive(const int *in, int *out, int n, int base, long long *total, hipStream_t s);
// bin: histogram of the targets' cells, scan, fill of the cell-sorted list.  cursor: nx ny + 1 ints of scratch.  The order
// inside a cell is whatever the atomics give; nothing that leaves the builder depends on it.
hipError_t launch_pattern_bin(const PatternTargets &t, int *cursor, hipStream_t s);
// count: rowcnt[i] = targets within delta of query i (m queries qx, qy), one wave per row.  hist (may be null): nbucket ints,
// zero beforehand; every accepted pair adds one to hist[target / tile].
hipError_t launch_pattern_count(const PatternTargets &t, int m, const double *qx, const double *qy, double delta, int *rowcnt,
                                int *hist, int tile, hipStream_t s);
// fill: for the 1-based row pointers rp of those counts, ci = the accepted targets of every row, 1-based and ascending, and
// ent = their taper values (kind: COCONS_TAPER_*).  Rows of up to PATTERN_SORT_LDS entries are sorted in LDS, longer ones by
// ranks in global memory.
constexpr int PATTERN_SORT_LDS = 512;
hipError_t launch_pattern_fill(const PatternTargets &t, int m, const double *qx, const double *qy, double delta, int kind,
                               const int *rp, int *ci, double *ent, hipStream_t s);
// buckets: band_buckets (band_plan.hpp) on the device for a chunk whose columns are already in the handle's order: entry w
// (row i, 1-based column c + 1) takes a place k of bucket c / tile -- cursor[c / tile]++, cursor starting as a copy of the
// bucket offsets --, bdst[k] = i + (c % tile) * stride, bsrc[k] = w.  Places inside a bucket are dealt by atomics; the ring
// load is a scatter to distinct addresses and does not see their order.
hipError_t launch_pattern_buckets(int m, const int *rp, const int *ci, int tile, int stride, int *cursor, int *bdst, int *bsrc,
                                  hipStream_t s);

// ---- Vecchia neighbour search (knn.hip) ---------------------------------------------------------------------
// One wave per query row: block b of the launch is query q = row0 + b at (qx[q], qy[q]).  Its neighbours are the m candidates
// with the smallest key (d2, index), d2 = fl(fl(dx dx) + fl(dy dy)) -- no square root, ties to the lower index.  The
// candidates are the points of t (binned: launch_pattern_bin) with an index below q (ordered) or all of them; brute: t is not
// binned and the wave scans t.x, t.y[0 .. min(q, t.n)) as they lie (the head of the ordered search).
// nn (may be null): nn[q + j ldn] = the j-th nearest + 1, 0 behind the last.  tab (may be null): tab[q m + j] = the same
// neighbours 0-based and ascending by index, -1 behind the last -- the layout VecchiaArgs::nbr reads.
struct KnnArgs {
    PatternTargets t;
    const double *qx = nullptr, *qy = nullptr;
    int row0 = 0, m = 0;
    int ordered = 0, brute = 0;
    int *nn = nullptr; size_t ldn = 0;
    int *tab = nullptr;
};
hipError_t launch_knn_query(const KnnArgs &a, int rows, hipStream_t s);

// ---- Vecchia neighbours by model correlation (knn_corr.hip; the rule: include/cocons_hip.h) -----------------
// One wave per row: block b of the launch is row i = b of n.  cand: the Euclidean ordered table of width mc in the layout of
// VecchiaArgs::nbr (row after row, 0-based, ascending, -1 behind the last).  The candidates of row i are cand's row i and,
// with hops = 2, the rows of its members, each index once; their key is (rho descending, index ascending), rho = v / sqrt(d_i
// d_j) from the records aos (launch_vecchia_aos) -- v the pair value with the earlier row on the `ii` side, d field 11.
// nn (may be null): nn[i + j ldn] = the candidate with the j-th largest key + 1, 0 behind the last.  tab (may be null):
// tab[i m + j] = the same m candidates 0-based and ascending by index, -1 behind the last.  fail: atomicMin of the 1-based
// rows with a rho that is not finite (such a row writes nothing).
constexpr int KNN_CORR_CAND_MAX = 63 + 63 * 63;       // indices that reach the deduplication of one row
struct KnnCorrArgs {
    int n = 0, mc = 0, hops = 1, m = 0;
    const int *cand = nullptr;
    const double *aos = nullptr;
    double gr = 0.0, nu_fixed = 0.0;
    int *nn = nullptr; size_t ldn = 0;
    int *tab = nullptr;
    int *fail = nullptr;
};
// slots of the row's set of indices in LDS: a power of two above the indices that can reach it, so a free slot always ends
// a probe.  (Neighbouring rows' lists overlap: at m_cand = 60 some 400 of the 3660 are distinct, and the LDS a row holds
// bounds the wavefronts a CU keeps in flight.)
__host__ __device__ inline int knn_corr_slots(int mc, int hops)
{
    int s = 64;
    while (s <= mc + (hops > 1 ? mc * mc : 0)) s <<= 1;
    return s;
}
size_t knn_corr_lds_bytes(int mc, int hops);
hipError_t launch_knn_corr(int mode, const KnnCorrArgs &a, hipStream_t s);

// ... of NEW locations (the rule: include/cocons_hip.h).  One wave per row: block b is row q = b of a chunk of
// `rows` new locations.  first: the chunk's plain kNN table among all n observations, rows x mc in the layout above; all (read
// with hops = 2 only): the same table of the observations' own coordinates, n x mc.  The candidates of row q are first's row
// q and, with hops = 2, the rows of `all` that its members name, each index once; their key is (rho descending, index
// ascending), rho = v / sqrt(d_q d_j) -- v the entry (j, q) of the prediction block (the site on the `ii` side, the prediction
// branch's records aosC of the observations and aosP of the chunk, an exact coordinate match gives the site's field 11), d
// field 11 of those records.  nn, ldn, tab as above with row q of the chunk; fail: atomicMin of row0 + q + 1.
struct KnnCorrPredArgs {
    int rows = 0, mc = 0, hops = 1, m = 0, row0 = 0;
    const int *first = nullptr, *all = nullptr;
    const double *aosC = nullptr, *aosP = nullptr;
    double gr = 0.0;
    int *nn = nullptr; size_t ldn = 0;
    int *tab = nullptr;
    int *fail = nullptr;
};
hipError_t launch_knn_corr_pred(const KnnCorrPredArgs &a, hipStream_t s);

// ---- maxmin ordering by scale-halving nets (order.hip; the rule: order_plan.hpp) -------------------------------
// The points live in LABEL order (px, py, orig: the caller's index), so a lower index is a higher priority.  state[p], by
// label: ORDER_FREE (not ordered, undecided at this level), ORDER_DONE (ordered), ORDER_DROPPED (conflicts with an ordered
// point at this level), ORDER_NEW (the dense schedule: taken in this round, ORDER_DONE after its check kernel).  rem: the R
// labels not ordered before this level, ascending.  A state only ever leaves ORDER_FREE inside a level, so a stale read
// means "undecided" and costs a round, never a bit.
enum : int { ORDER_FREE = 0, ORDER_DONE = 1, ORDER_DROPPED = 2, ORDER_NEW = 3 };
struct OrderArgs {
    int n = 0;
    const double *px = nullptr, *py = nullptr;
    const int *orig = nullptr;
    int *state = nullptr;
    const int *rem = nullptr;
    int R = 0;
    double e = 0.0;                     // e_k: two points conflict iff d2 < e
    // the dense schedule: the level's grid, S (one ordered label per cell, -1: none), the champions (all ones: none) and
    // every rem entry's cell
    PatternGrid g;
    int *S = nullptr;
    unsigned *champ = nullptr;
    int *cellof = nullptr;
    // the binned schedule: all n points (label order) on a grid whose edge exceeds l_k
    PatternTargets t;
    unsigned *counter = nullptr;        // += the points still undecided after the round
};
// relabel: px, py, orig, state from the caller's x, y; rem = every label but first's, ascending; order[0], olab[0]: level 0
hipError_t launch_order_relabel(int n, const double *x, const double *y, int first, double *px, double *py, int *orig, int *state,
                                int *rem, int *order, int *olab, hipStream_t s);
// dense level: S[cell] = label for the `done` ordered labels olab (S is all -1 beforehand)
hipError_t launch_order_dense_seed(const OrderArgs &a, const int *olab, int done, hipStream_t s);
// dense round, three launches: (a) champ[cell] = min of the undecided labels; (b) a champion below the champions of the 24
// surrounding cells is taken (ORDER_NEW, S[cell] = label); (c) check: ORDER_NEW -> ORDER_DONE, the champions of the cells
// touched are cleared, every undecided point looks for a conflict in the 5 x 5 block of S and counts itself if it finds none.
// first: the level's opening check (cellof is computed, champ is all ones already)
hipError_t launch_order_dense_champions(const OrderArgs &a, hipStream_t s);
hipError_t launch_order_dense_take(const OrderArgs &a, hipStream_t s);
hipError_t launch_order_dense_check(const OrderArgs &a, bool first, hipStream_t s);
// binned round, one launch: every undecided point scans the 3 x 3 block; a conflict with an ordered point drops it, else with
// no undecided conflicting point of a lower label it is taken (ORDER_DONE), else it waits and counts itself
hipError_t launch_order_binned_round(const OrderArgs &a, hipStream_t s);
// the end of a level, three launches: cnt[b] = the ordered among places [256 b, 256 b + 256) of rem, first = its exclusive
// scan (launch_scan_exclusive; *total: their number), then order[base + rank] = orig + 1 and olab[..] = label for the
// ordered, rem2[j - rank] = label with the state back to ORDER_FREE for the others.  cnt, first: R / 256 + 2 ints
hipError_t launch_order_emit(const OrderArgs &a, int *cnt, int *first, long long *total, int base, int *order, int *olab,
                             int *rem2, hipStream_t s);
// the rest: order[base + j] = orig[rem[j]] + 1
hipError_t launch_order_rest(const OrderArgs &a, int base, int *order, hipStream_t s);

// ---- grouping Vecchia rows in rounds (group.hip; the rule: group_plan.hpp) ----------------------------------
// The state, by block id (a block's id is its smallest member): blk[row] = the id of the row's block, sz[id] = |S(id)|,
// slot[id max_rows ..] = S(id) ascending -- written only while |S| <= max_rows: a larger S belongs to a row that never
// merges and is never read.  A round is three launches over the live ids: every block proposes (prop, key; the best keys by
// 64-bit atomic minima into best, all ones = none; *any = 1 when somebody proposed), every realised edge merges, and the
// survivors are gathered into next (their best words set to all ones again, *count = their number).  No floating point.
struct GroupArgs {
    int n = 0, m = 0, max_rows = 0;
    const int *tab = nullptr;           // n x m, the layout of VecchiaState::nbr
    int *blk = nullptr, *sz = nullptr, *slot = nullptr, *prop = nullptr;
    unsigned long long *key = nullptr, *best = nullptr;
    const int *live = nullptr; int nlive = 0;
    int *next = nullptr;
    int *any = nullptr, *count = nullptr;
};
// every row a block of its own: blk, sz, slot, best, and live = 0 .. n - 1 written into a.next
hipError_t launch_group_init(const GroupArgs &a, hipStream_t s);
hipError_t launch_group_propose(const GroupArgs &a, hipStream_t s);
hipError_t launch_group_merge(const GroupArgs &a, hipStream_t s);
hipError_t launch_group_compact(const GroupArgs &a, hipStream_t s);

// The plan and the expanded table of the state the rounds left (group_plan.hpp's group_plan and group_table on the same
// partition, integer for integer), four launches: flags (flag[i] = row i is a block's id; its exclusive scan num numbers the
// blocks by smallest member), sizes (ids[b], off[b] = |S(b)| -- scanned in place afterwards -- and hist[k] = the blocks of k
// rows, from which the host takes the statistics and start[]), fill (one wavefront per block: rows, mask, and the expanded
// row of every member into nbr, n x m_out in the layout of VecchiaState::nbr) and order (the blocks largest first, stable in
// the id: one workgroup per size walks the blocks in ascending order, start[64 - k] is where size k begins).
struct GroupPlanArgs {
    int n = 0, m = 0, max_rows = 0, blocks = 0, m_out = 0;
    const int *tab = nullptr, *blk = nullptr, *sz = nullptr, *slot = nullptr;
    int *flag = nullptr;                // n
    const int *num = nullptr;           // n + 1
    int *ids = nullptr;                 // blocks
    int *off = nullptr;                 // blocks + 1
    int *hist = nullptr;                // GROUP_ROWS_MAX + 1
    int *rows = nullptr, *order = nullptr, *nbr = nullptr;
    unsigned long long *mask = nullptr;
    int start[65] = {};
};
hipError_t launch_group_plan_flags(const GroupPlanArgs &a, hipStream_t s);
hipError_t launch_group_plan_sizes(const GroupPlanArgs &a, hipStream_t s);
hipError_t launch_group_plan_fill(const GroupPlanArgs &a, hipStream_t s);
hipError_t launch_group_plan_order(const GroupPlanArgs &a, hipStream_t s);

// ---- analytic gradient of the dense -2 log-likelihood (grad.hip) ----------------------------------------------------------
constexpr int GSITE_FIELDS = 4;    // launch_grad_site: dtilt/deta, cot(tilt), dlog(nu_ij)/deta_smooth, exp(eta_sd)
struct GradArgs {
    int n, pad0, npad, p;          // internal order: sites [pad0, n) are the caller's
    const double *S; size_t lds;   // -Sigma^-1, lower triangle (launch_grad_syrk)
    const double *AR; size_t ldar; int nr;    // the low-rank block, npad x nr: A = Sigma^-1 R (dense), [U | sqrt(r) C] (Profile / REML)
    double coef;                   // W = coef Sigma^-1 - AR AR': nr for the dense gradient, r for Profile / REML
    const double *loc; size_t stride;         // loc_params_kernel's SoA
    const double *site;                       // launch_grad_site's SoA (GSITE_FIELDS x stride)
    const double *X; int ldx;
    double gr, nu_fixed;
    int smooth_free;               // the smoothness varies (logistic branch with hi > lo): the smooth row is formed
    double *part_row, *part_col, *part_glob, *gsite;   // scratch: grad_scratch_doubles(npad), in this order
    double *out;                   // 6 p theta-table gradient (row-major) then p mean gradient
};
// rows [row0, row0 + nrows) x columns [0, ncols) of A: the unit vectors e_(row - row_id)' (row_id < 0: zeros)
void launch_grad_fill(double *A, size_t lda, int row0, int nrows, int ncols, int row_id, hipStream_t s);
// AR (npad x nr) = B W', B = the npad solved rows from brow0 (L^-T), W = the nr solved rows from wrow0 (L^-1 R)';
// part: grad_sigma_r_scratch_doubles(npad, nr) doubles
size_t grad_sigma_r_scratch_doubles(int npad, int nr);
void launch_grad_sigma_r(const double *A, size_t lda, int npad, int wrow0, int nr, int brow0, double *part, double *AR,
                         hipStream_t s);
// the leading npad x npad square of A (lower tiles, zero beforehand) -= B B', B = rows brow0.. (upper triangular)
void launch_grad_syrk(double *A, size_t lda, int npad, int brow0, hipStream_t s);
// Profile / REML: fin = launch_finalize's output of a border [Z' ; Xb'] (log-determinant, then the
// (r + q)^2 Gram matrix), SX (npad x (r + q)) = Sigma^-1 [Z | Xb] = [A_z | V].  W = Xb' Sigma^-1 Xb is factored in one
// workgroup (gls: grad_gls_doubles(r, q) doubles of scratch), then LR (npad x (r [+ q])) = [A_z - V beta | sqrt(r) V chol(W)^-T]
// (the second block with reml only).  A pivot of W that is not positive leaves LR all zero.
size_t grad_gls_doubles(int r, int q);
void launch_grad_lowrank(const double *fin, const double *SX, int npad, int r, int q, int reml, double *gls, double *LR,
                         hipStream_t s);
void launch_grad_site(const LocArgs &a, double *out, size_t stride, int smooth_free, hipStream_t s);
size_t grad_scratch_doubles(int npad);
// pair contraction, per-site sums and X' g into g.out (7 p doubles)
void launch_grad_pairs(int mode, const GradArgs &g, hipStream_t s);
// out[i], out[n + i], out[2 n + i] = M, dM/du, dM/dnu of the gradient's device code
void launch_matern_grad_points(int n, const double *nu, const double *u, double *out, hipStream_t s);

// ---- expected (Fisher) information of the dense model (grad.hip) ---------------------------------------------
// Matrices are blocks of npad rows in one tall buffer with a common leading dimension (the trailing-update kernel's panel shape).
// tile pairs of `count` matrices (dz / sz elements apart): dst = sign * (the lower triangle of src, mirrored); dst may be src
void launch_fisher_mirror(double *dst, size_t ldd, size_t dz, const double *src, size_t lds, size_t sz, int npad, int count,
                          double sign, hipStream_t s);
// (cocons_fisher_reml) S (npad x npad, symmetric in full) -= scale C C' in place, C npad x q (q <=
// COCONS_P_MAX); rows of C outside the caller's sites [pad0, n) count as 0.  Fixed order, symmetric to the bit where S is.
void launch_fisher_project(double *S, size_t lds, const double *C, size_t ldc, int q, int pad0, int n, int npad, double scale,
                           hipStream_t s);
// Sigma_a = sum_tk dirs[a][t, k] dSigma/dtheta[t, k] for the ndir directions (device, ndir x 6 p in theta's table layout), in
// full, at D + a dstride; g: the gradient's site and pair arguments (loc, site, X, gr, nu_fixed, smooth_free); w: ndir x 6 x npad
void launch_fisher_dirs(int mode, const GradArgs &g, int ndir, const double *dirs, double *w, double *D, size_t ldd,
                        size_t dstride, hipStream_t s);
// block a + 2 of Tb = -(Sigma^-1 Sigma_a)' from Sigma^-1 in block 0 and Sigma_a in block a + 1 (ndir + 2 blocks; the
// directions' blocks are consumed)
hipError_t launch_fisher_products(double *Tb, size_t ldt, int npad, int ndir, hipStream_t s);
// info[a, b] = coef sum_ij G_a(i, j) G_b(j, i) (ndir x ndir, symmetric to the bit), G_a at G + a dstride
size_t fisher_trace_scratch_doubles(int npad, int ndir);
void launch_fisher_trace(const double *G, size_t ld, size_t dstride, int npad, int ndir, double coef, double *part, double *info,
                         hipStream_t s);
// out (p x p) = coef X' S X over the caller's sites, S symmetric in full; part: grad_sigma_r_scratch_doubles(npad, p), SX: npad x p
void launch_fisher_mean(const double *S, size_t lds, int n, int pad0, int npad, int p, const double *X, int ldx, double coef,
                        double *part, double *SX, double *out, hipStream_t s);

// ---- analytic gradient of the tapered -2 log-likelihood (selinv.hip, grad.hip) -------------------------------------------
// Selected inverse on the tile envelope of a taper handle's factor.  L: the factorisation's buffer as it leaves it (leading
// dimension ldl, the nr rows under the matrix hold (L^-1 R)'); Z: a buffer of the band's shape without rows under it
// (leading dimension ldz = skew * 128, or npad when skew = 0); both in the layout band_index(., ., ld, skew, npad).
// d_hi: device copy of the envelope (null: hi[c] = nt).  After launch_selinv Z holds S^-1 on every envelope tile (lower
// tiles, diagonal tiles in full), AR (npad x nr, column-major) holds S^-1 R, and L is consumed.
struct SelinvArgs {
    double *L; size_t ldl;
    double *Z; size_t ldz;
    int skew, npad, nt;
    const int *d_hi;
    int nr;
    double *AR;
};
// h_hi: host copy of the envelope (null: none); maxband = max_c (hi[c] - c)
void launch_selinv(const SelinvArgs &a, const int *h_hi, int maxband, hipStream_t s);
// out[w] = Z(max(i, j), min(i, j)) for the 0-based index pairs ij[2 w], ij[2 w + 1]
void launch_selinv_gather(const double *Z, size_t ldz, int skew, int npad, const int *ij, size_t count, double *out, hipStream_t s);
struct TaperGradArgs {
    int n, npad, p, nnz, nr;
    const int *ci, *rp;            // the device pattern: lower triangle, 1-based CSR
    const int *tcp, *tidx, *trow;  // its transposed index: column j's entries tidx[tcp[j] .. tcp[j + 1]) and their rows trow[.]
    const double *tapv;
    const double *Z; size_t ldz; int skew;    // S^-1 (launch_selinv)
    const double *AR;              // S^-1 R, npad x nr
    double coef;                   // W = coef Z - AR AR'
    const double *loc; size_t stride;         // loc_params_kernel's SoA
    const double *site;            // launch_grad_site's SoA
    const double *X; int ldx;
    double nu_fixed;
    int smooth_free;
    double *ent;                   // 6 nnz: per entry, (log-determinant part, quadratic part) x 3
    double *gsite;                 // 9 npad: per site, 2 parts x (std.dev, scale, smooth, nugget), then sum_c A(i, c)
    double *out;                   // 9 p: 2 parts x 4 families x p, then the mean gradient
};
void launch_taper_grad(int mode, const TaperGradArgs &g, hipStream_t s);

// ---- expected (Fisher) information of a tapered fit on the band factor (cocons_fisher_taper) -------------------
// Direction entries (grad.hip): S_a = T o sum_tk v_a[t, k] dC/dtheta[t, k] on the device pattern (lower triangle, 1-based CSR),
// out[a nnz + w] for the ndir directions (dirs: device, ndir x 6 p in theta's table layout); wsite: ndir x 4 x npad scratch
// (the site weights of std.dev, scale, smooth, nugget).  The pair arithmetic is taper_grad_entry_kernel's.
struct TaperDirsArgs {
    TaperGradArgs g;               // n, npad, p, nnz, ci, rp, tapv, loc, stride, site, X, ldx, nu_fixed, smooth_free (the rest unused)
    int ndir;
    const double *dirs;
    double *wsite, *out;
};
void launch_taper_dirs(int mode, const TaperDirsArgs &d, hipStream_t s);
// Rows (probes, directions' vectors) live column-major with the row index fastest: rows x npad, ld a multiple of 64 -- the
// layout of the kriging ring's slots, here at full width (tile column I in slot I).
// back_pack: the operands of the BACKWARD solve W = E L^-1.  With F the flip of all npad indices, W F = (E F) (F L' F)^-T and
// M = F L' F is lower triangular with L's envelope mirrored: the backward solve is the forward pair run on M with the rows'
// columns flipped (column npad - 1 - c of the buffer holds column c).  Tile (I', J') of M, I' >= J', is the flipped transpose of
// L's tile (nt - 1 - J', nt - 1 - I') and goes to tile index d_toffb[J'] + (I' - J') of Mp (d_hib: M's envelope; both device,
// nt ints); Qb (nt x 2048) gets the operands of M's diagonal tiles.
void launch_band_back_pack(const double *A, size_t lda, int skew, int npad, const int *d_hib, int nt, int W, const int *d_toffb,
                           double *Mp, double *Qb, hipStream_t s);
// V = C P^-T for the `rows` rows of a full-width buffer (rows a multiple of 64) on packed tiles P / operands Q as
// launch_krige_band_pack or launch_band_back_pack leave them (toff, hi: HOST arrays of that factor); krige_band_diag_kernel and
// krige_band_update_kernel with the identity ring, no loads.  zero: npad zeros; st, qd: `rows` doubles nobody reads.
struct BandSweep {
    const double *Lp = nullptr, *Qp = nullptr; const int *toff = nullptr, *hi = nullptr; int nt = 0;
    double *C = nullptr; size_t ldc = 0; int rows = 0;
    const double *zero = nullptr; double *st = nullptr, *qd = nullptr;
};
hipError_t launch_band_sweep(const BandSweep &a, hipStream_t s);
inline hipError_t launch_band_back_solve(const BandSweep &a, hipStream_t s) { return launch_band_sweep(a, s); }   // (on back_pack's operands)
// probe rows of a chunk into the flipped buffer E (rows x npad, zero beforehand): unit rows e_(g0 + k), k < count (exact mode) ...
void launch_band_unit_rows(double *E, size_t lde, int npad, int g0, int count, hipStream_t s);
// ... or the caller's probes: E[k, npad - 1 - pos[i]] = P[i + k n] for i < n, k < count (P: n x count, column-major)
void launch_band_given_rows(double *E, size_t lde, int npad, const double *P, int n, const int *pos, int count, hipStream_t s);
// rows [row0, row0 + 64) of U: X' (X: n x p column-major, p <= 64) in its first p rows, zero elsewhere and from column n on
void launch_band_x_rows(double *U, size_t ldu, int row0, const double *X, int n, int p, int npad, hipStream_t s);
// U_a[k, j] = sum_{i in row j of the FULL pattern} S_a[j, i] Wf[k, npad - 1 - i] for k < rows, every direction a at rows
// a bstride + k of U (columns j >= n: zero).  frp / fci: the full symmetric pattern (0-based CSR), fidx: the index of
// entry (max, min) in the lower-triangle order of Sd (ndir x nnz).  Sums in CSR index order.
struct BandSpmm {
    const double *Wf = nullptr; size_t ldw = 0; int rows = 0, n = 0, npad = 0, ndir = 0;
    const int *frp = nullptr, *fci = nullptr, *fidx = nullptr; const double *Sd = nullptr; size_t nnz = 0;
    double *U = nullptr; size_t ldu = 0, bstride = 0;
};
void launch_band_spmm_dirs(const BandSpmm &a, hipStream_t s);
// Gram partial sums of solved rows: part[(strip0 + s) nd nd + a nd + b] = sum over the rows k < nrows (<= 64) of strip s and
// all columns of Q[base + a bstride + 64 s + k, :] o Q[base + b bstride + 64 s + k, :] for a <= b < nd.  Fixed segments of
// BAND_GRAM_SEG columns and a fixed tree inside the workgroup; seg: band_gram_scratch_doubles(nstrips, npad, nd) doubles.
constexpr int BAND_GRAM_SEG = 1024;
size_t band_gram_scratch_doubles(int nstrips, int npad, int nd);
void launch_band_gram(const double *Q, size_t ld, size_t base, size_t bstride, int nrows, int nstrips, int npad, int nd,
                      double *seg, double *part, int strip0, hipStream_t s);
// out[a nd + b] = out[b nd + a] = weight * sum_{s < nstrips} part[s nd nd + a nd + b], in index order
void launch_band_gram_sum(const double *part, int nstrips, int nd, double weight, double *out, hipStream_t s);

// ---- cross-validated predictions (cv.hip)---------------------------------------------------------------------
// S: -Sigma^-1 in the lower triangle (launch_grad_syrk), so K(i, j) = -S(max, min); U = Sigma^-1 R (npad x nr, ld ldu).  Results
// go out in the handle's internal order: var[i], res[i + k ldr].  fail: one word, INT_MAX beforehand, atomicMin of the label of
// a fold whose block has a pivot that is not positive and finite.
constexpr int CV_SMALL_MAX = 128;  // largest fold the LDS kernel takes
// closed form for single observations: positions idx[0 .. count) (idx = null: first + t); the label recorded on failure is
// lab[t] (lab = null: t)
void launch_cv_loo(const double *S, size_t lds, const double *U, size_t ldu, int nr, const int *idx, const int *lab, int first,
                   int count, double *var, double *res, size_t ldr, int *fail, hipStream_t s);
// folds of 2 .. CV_SMALL_MAX observations, one workgroup each: fold flist[g] holds the positions idx[off[f] .. off[f + 1]),
// ascending; cls = 16, 32, 64 or 128 >= the largest of these folds sizes the LDS of the launch
hipError_t launch_cv_folds(int cls, const double *S, size_t lds, const double *U, size_t ldu, int nr, const int *idx,
                           const int *off, const int *flist, const int *lab, int nfolds, double *var, double *res, size_t ldr,
                           int *fail, hipStream_t s);
// the same with K_BB of fold f read as it is from the b x b block at S + base[f], leading dimension lds (lower triangle): the
// blocks the fold-aware Gram product of cocons_cv_taper_folds leaves (base: device, indexed by fold)
hipError_t launch_cv_folds_at(int cls, const double *S, size_t lds, const long long *base, const double *U, size_t ldu, int nr,
                              const int *idx, const int *off, const int *flist, const int *lab, int nfolds, double *var,
                              double *res, size_t ldr, int *fail, hipStream_t s);
// a large fold's bordered matrix (ld ldo = 2 bpad + rt rows, bpad columns): K_BB identity-padded to bpad, under it rt rows with
// U_B' (nr of them, the rest zero), then bpad unit rows
void launch_cv_gather(const double *S, size_t lds, const double *U, size_t ldu, int nr, const int *pos, int b, int bpad, int rt,
                      double *out, size_t ldo, hipStream_t s);
// launch_cv_gather's matrix without K_BB: the top block zero with ones on the padding's diagonal [b, bpad) -- the Gram product
// adds K_BB into it --, U_B' and the unit rows as there
void launch_cv_border(const double *U, size_t ldu, int nr, const int *pos, int b, int bpad, int rt, double *out, size_t ldo,
                      hipStream_t s);
// var[pos[i]] = v[i], res[pos[i] + k ldr] = r[i + k b]
void launch_cv_scatter(const int *pos, int b, int nr, const double *v, const double *r, double *var, double *res, size_t ldr,
                       hipStream_t s);
// between the factorisations of one call: a failing minor in *info (anything but `clean`) is taken out -- into *keep when keep
// is given (Sigma's own), else as atomicMin(*fail, label) -- and *info is `clean` again; put: *info = *keep
void launch_cv_info_take(int *info, int clean, int *keep, int *fail, int label, hipStream_t s);
void launch_cv_info_put(int *info, const int *keep, hipStream_t s);
// taper handles: the diagonal of Z = S^-1 (band_index layout) and AR = S^-1 R
void launch_cv_taper(const double *Z, size_t ldz, int skew, int npad, int n, const double *U, size_t ldu, int nr, double *var,
                     double *res, size_t ldr, int *fail, hipStream_t s);
// the same closed form for the `count` positions idx[t] only; the label recorded on failure is lab[t]
void launch_cv_taper_list(const double *Z, size_t ldz, int skew, int npad, const int *idx, const int *lab, int count,
                          const double *U, size_t ldu, int nr, double *var, double *res, size_t ldr, int *fail, hipStream_t s);

// ---- Vecchia approximation: one small block per observation (vecchia.hip) -------------------------------------
constexpr int VECCHIA_M_MAX = 63;      // neighbours per row: a block of m + 1 rows never exceeds one wavefront
constexpr int VECCHIA_REC = 16;        // doubles per location record: the LOCP_FIELDS parameters padded to one 128-byte line
constexpr int VECCHIA_G = 4;           // right-hand sides carried through one forward substitution
constexpr int VECCHIA_SUM_SEG = 4096;  // elements per first-stage segment of the totals
// aos[i * VECCHIA_REC + f] = soa[i + f * stride] for the n locations of loc_params_kernel's SoA, f < LOCP_FIELDS; the rest 0
void launch_vecchia_aos(const double *soa, size_t stride, int n, double *aos, hipStream_t s);
// out[i + k ldo] = z[i + (col0 + k) ldz] - (X mean)[i] for i < n, k < ncol (mean: p doubles on the host)
void launch_vecchia_resid(int n, int p, const double *X, int ldx, const double *mean, const double *z, int ldz, int col0,
                          int ncol, double *out, size_t ldo, hipStream_t s);
// One block per row.  nbr: rows x m, row after row, the 0-based locations a row is conditioned on in ascending order and -1
// in the places behind them.  Likelihood (pred = false): row i is observation i, its block the neighbours' and its own
// rows of Sigma(theta) from the records aosK; with K = C C', logd[i] = log C(k, k) (logd may be null) and
// Y[i + c ldy] = the last component of C^-1 B[(neighbours, i), c] for the nb columns of B (locations x nb, ld ldb).
// Prediction (pred = true): row i is prediction site i of the chunk (records aosP, prediction branch), K the neighbours'
// block from aosK, c the cross-covariance by cov_rns_pred's rule from aosC (the observations in the prediction branch's
// parameters; may be aosK); stoch[i] = c' K^-1 B[neighbours, 0], quad[i] = c' K^-1 c; a row without neighbours gives 0, 0.
// A pivot that is not positive and finite: atomicMin(*fail, row0 + i + 1), nothing written for that row.
struct VecchiaArgs {
    int rows = 0, m = 0, kb = 0;       // kb = m + 1: what the launch's LDS is sized by
    const int *nbr = nullptr;
    const double *aosK = nullptr, *aosC = nullptr, *aosP = nullptr;
    double gr = 0.0, nu_fixed = 0.0;
    const double *B = nullptr; size_t ldb = 0; int nb = 0;
    double *Y = nullptr; size_t ldy = 0;
    double *logd = nullptr, *stoch = nullptr, *quad = nullptr;
    int *fail = nullptr; int row0 = 0;
    // the gradient launch only (launch_vecchia_grad_blocks): block b of the launch is observation obs0 + b
    int obs0 = 0;
    const double *aosG = nullptr;      // launch_vecchia_site_rec's records
    int smooth_free = 0;
    const double *X = nullptr; int ldx = 0, p = 0;
    double *rec = nullptr; size_t ldr = 0;     // the per-observation records, column q of block b at rec[q ldr + b]
    // the information launch only (launch_vecchia_fisher_blocks); it uses obs0, aosG, smooth_free, X and rec too
    int ndir = 0, gd = 0;              // directions, and how many of them one pair walk serves (vecchia_fisher_group)
    const double *dirs = nullptr;      // ndir tables of 6 x p on the device
};
size_t vecchia_lds_bytes(int m, bool pred);
void launch_vecchia_blocks(int mode, bool pred, const VecchiaArgs &a, hipStream_t s);
// The gradient launch: logd and Y as there (the value kernel's phases, vecchia_block.hpp), and per observation the record of
// vecchia_rec_cols(p) doubles -- with q = f p + k for family f and column k of X: [q] the log-determinant's share of the
// site sums contracted with X, [6 p + q] the quadratic forms' share, [12 p] and [12 p + 1] the two shares of the global-range
// sum, [12 p + 2 + k] = (sum_c y_c) sum_rows s[row] X[site(row), k] (the mean gradient without its factor -2).
constexpr int VECCHIA_GSITE_REC = 4;   // doubles per location of launch_vecchia_site_rec: GSITE_FIELDS
constexpr int VECCHIA_GRAD_CHUNK = 8 * VECCHIA_SUM_SEG;     // observations per gradient launch (a multiple of VECCHIA_SUM_SEG)
inline int vecchia_rec_cols(int p) { return 13 * p + 2; }
// rec[i * VECCHIA_GSITE_REC + f] = soa[i + f * stride] for the n locations of launch_grad_site's SoA
void launch_vecchia_site_rec(const double *soa, size_t stride, int n, double *rec, hipStream_t s);
size_t vecchia_grad_lds_bytes(int m);
void launch_vecchia_grad_blocks(int mode, const VecchiaArgs &a, hipStream_t s);
// The information variant of the likelihood launch (no right-hand sides, logd null): per observation the record of
// vecchia_fisher_cols(ndir, p) doubles -- the lower triangle of the block's Gram over the directions, entry a (a + 1) / 2 + b
// for b <= a, then that of u u' with u = sum_rows s[row] X[site(row), .].  The dynamic LDS grows with m, ndir and the group
// gd = vecchia_fisher_group(m, ndir) <= VECCHIA_FD, the largest that keeps it within VECCHIA_FISHER_LDS_MAX.
constexpr int VECCHIA_FD = 16;         // directions per pair walk at most (a multiple of VECCHIA_G)
constexpr size_t VECCHIA_FISHER_LDS_MAX = 160 * 1024;
constexpr size_t VECCHIA_FISHER_CHUNK_BYTES = (size_t)16 << 20;   // a chunk's records: this many bytes, or one segment's
inline int vecchia_fisher_cols(int ndir, int p) { return ndir * (ndir + 1) / 2 + p * (p + 1) / 2; }
// observations per information launch: a multiple of VECCHIA_SUM_SEG, at most VECCHIA_GRAD_CHUNK
inline int vecchia_fisher_chunk(int ndir, int p)
{
    const size_t segs = VECCHIA_FISHER_CHUNK_BYTES / ((size_t)vecchia_fisher_cols(ndir, p) * sizeof(double) * VECCHIA_SUM_SEG);
    return VECCHIA_SUM_SEG * (int)(segs < 1 ? 1 : segs > VECCHIA_GRAD_CHUNK / VECCHIA_SUM_SEG ? VECCHIA_GRAD_CHUNK / VECCHIA_SUM_SEG : segs);
}
size_t vecchia_fisher_lds_bytes(int m, int ndir, int gd);
int vecchia_fisher_group(int m, int ndir);
void launch_vecchia_fisher_blocks(int mode, const VecchiaArgs &a, hipStream_t s);
// launch_vecchia_sums in two steps for values that arrive in chunks: the first stage over the `rows` values of a chunk that
// starts at segment seg0 of nseg (plain sums in every column), then the second stage over all nseg segments.  The totals are
// the tree launch_vecchia_sums would form over all the values at once, whatever the chunk.
void launch_vecchia_chunk_sums(const double *v, size_t ldv, int rows, int ncol, double *part, int seg0, int nseg, hipStream_t s);
void launch_vecchia_final_sums(const double *part, int nseg, int ncol, double *out, hipStream_t s);
// out[q] = sum_i v[i + q ldv] (q = 0) or of its squares (q >= 1) over i < n, for q < ncol: a tree of fixed shape over values in
// memory; part: vecchia_sum_scratch_doubles(n, ncol) doubles
size_t vecchia_sum_scratch_doubles(int n, int ncol);
void launch_vecchia_sums(const double *v, size_t ldv, int n, int ncol, double *part, double *out, hipStream_t s);

// ---- grouped Vecchia blocks: one factorisation for a group of rows (vecchia_group.hip) -------------------------
// The plan of group_plan.hpp on the device: block b holds the rows rows[off[b] .. off[b + 1]) (at most 64 and at most kb,
// 0-based, ascending), bit p of mask[b] says whether the row at position p is a member; workgroup w of the launch takes block
// order[w] (order null: block w).  Every member i gets logd[i] (logd may be null) and Y[i + c ldy] for the nb columns of B as
// launch_vecchia_blocks gives them on the table whose row i is the block's rows in front of i -- the same bits.  A pivot that
// is not positive and finite at position q: atomicMin(*fail, row + 1) for the first member at a position >= q, nothing written
// for the block.
constexpr int VECCHIA_GROUP_THREADS = 256;     // threads of a block's workgroup: the first 64 are its rows, all evaluate pairs
struct VecchiaGroupArgs {
    int blocks = 0, kb = 0;            // kb: the plan's largest block, what the launch's LDS is sized by
    const int *off = nullptr, *rows = nullptr, *order = nullptr;
    const unsigned long long *mask = nullptr;
    const double *aosK = nullptr;
    double gr = 0.0, nu_fixed = 0.0;
    const double *B = nullptr; size_t ldb = 0; int nb = 0;
    double *Y = nullptr; size_t ldy = 0;
    double *logd = nullptr;
    int *fail = nullptr;
    // the gradient launch only (launch_vecchia_group_grad_blocks): workgroup w of the launch is block
    // blk0 + order[w] (order null: blk0 + w) and writes column q of its record at rec[q ldr + (block - blk0)]
    int blk0 = 0;
    const double *aosG = nullptr;      // launch_vecchia_site_rec's records
    int smooth_free = 0;
    const double *X = nullptr; int ldx = 0, p = 0;
    double *rec = nullptr; size_t ldr = 0;
    // the information launch only (launch_vecchia_group_fisher_blocks); it uses blk0, aosG, smooth_free, X and
    // rec too, and no right-hand sides (nb = 0, logd null)
    int ndir = 0, gd = 0, mc = 0;      // directions, directions a group and members a chunk (vecchia_group_fisher_shape)
    const double *dirs = nullptr;      // ndir tables of 6 x p on the device
    // the coefficient launch only (launch_vecchia_group_coefs): the records of launch_vecchia_coefs, row i at
    // coef[i ldc ..] with ldc = (the handle's table width) + 1 >= kb; the rows below row0 are fixed and get no record
    double *coef = nullptr; size_t ldc = 0; int row0 = 0;
};
void launch_vecchia_group_blocks(int mode, const VecchiaGroupArgs &a, hipStream_t s);
// The coefficient variant of the grouped launch (no right-hand sides, no log d): every member at position p whose row is >= row0
// gets its record as launch_vecchia_coefs documents it -- places t < p hold s_p[t] (the row's neighbours are the block's positions
// 0 .. p - 1), places p .. ldc - 2 hold 0, place ldc - 1 holds s_p[p] -- the same bits, from one factorisation of the block.  A
// pivot that is not positive and finite at position q: atomicMin(*fail, row + 1) for the first member at a position >= q whose row
// is >= row0 (none: no failure), nothing written for the block.  The LDS is launch_vecchia_group_blocks'.
void launch_vecchia_group_coefs(int mode, const VecchiaGroupArgs &a, hipStream_t s);
// The gradient launch over the blocks blk0 .. blk0 + blocks - 1: logd and Y as there (the value kernel's phases),
// and per BLOCK one record of vecchia_rec_cols(p) doubles in launch_vecchia_grad_blocks' layout -- the sum of the records
// its members would give on the expanded table, from one evaluation of every pair of the block.  The dynamic LDS is
// vecchia_group_grad_lds_bytes(kb): 78 144 bytes at kb = 64, above 64 KB from kb = 54 on.
size_t vecchia_group_grad_lds_bytes(int kb);
void launch_vecchia_group_grad_blocks(int mode, const VecchiaGroupArgs &a, hipStream_t s);
// The information variant of the grouped launch (no right-hand sides): per BLOCK one record of vecchia_fisher_cols(ndir, p)
// doubles in launch_vecchia_fisher_blocks' layout -- the sum of the records its members would give on the expanded table, every
// sum in an order that is a function of the block alone.  vecchia_group_fisher_shape gives gd in {4, 8, 16} and mc >= 1 with
// gd mc <= 64; the launch's dynamic LDS is vecchia_group_fisher_lds_bytes(kb, ndir, gd, mc), which the caller holds to
// VECCHIA_FISHER_LDS_MAX (157 952 bytes at kb = 64, ndir = 16: gd = 16, mc = 4).
size_t vecchia_group_fisher_lds_bytes(int kb, int ndir, int gd, int mc);
void vecchia_group_fisher_shape(int kb, int ndir, int *gd, int *mc);
void launch_vecchia_group_fisher_blocks(int mode, const VecchiaGroupArgs &a, hipStream_t s);

// ---- U^-1 of a Vecchia fit: coefficients (vecchia.hip), levels and the level solve (vecchia_sim.hip) ------------
constexpr int VECCHIA_SIM_FUSE_ITEMS = 256;     // a level of at most this many (row, column) pairs may join a fused run
constexpr int VECCHIA_SIM_FUSE_THREADS = 256;   // the one workgroup of a fused run
constexpr int VECCHIA_SIM_FUSE_LEVELS = 2048;   // levels one fused launch walks at most: a chain-shaped table becomes many
                                                // short launches, never one long-running kernel
constexpr int VECCHIA_SIM_SWEEPS = 8;           // relaxation sweeps between two looks at the "changed" word
// The likelihood launch's gather, pair loop and factorisation, then s = C^-T e_last, for the observations a.obs0 ..
// a.obs0 + a.rows - 1 (uses m, kb, nbr, aosK, gr, nu_fixed, fail).  a.rec: n records of kb = m + 1 doubles, row i at
// rec[i kb ..]: place t < k holds s_t of the neighbour at place t of nbr's row, places k .. m - 1 hold 0, place m holds s_last.
// A pivot that is not positive and finite: atomicMin(*fail, row + 1), nothing written for that row.
void launch_vecchia_coefs(int mode, const VecchiaArgs &a, hipStream_t s);
// One relaxation sweep of level[i] = 1 + max_t level[nbr[i m + t]] (1 without neighbours) over the rows n_fixed .. n - 1, in
// place; *changed = 1 where a row's level grew.  level starts as zeros and level[i < n_fixed] stays 0.
void launch_vecchia_level_sweep(const int *nbr, int m, int n, int n_fixed, int *level, int *changed, hipStream_t s);
// count[l - 1] = rows of level l, *depth = the largest level (both zeroed by the caller); then, cursor holding the levels'
// offsets, order[..] = the rows n_fixed .. n - 1 by level (cursor ends as the offsets of the next levels)
void launch_vecchia_level_count(const int *level, int n, int n_fixed, int *count, int *depth, hipStream_t s);
void launch_vecchia_level_scatter(const int *level, int n, int n_fixed, int *cursor, int *order, hipStream_t s);
// x[row + q ldx] = (W[(row - w_row0) + q ldw] - sum_t coef[row (m + 1) + t] x[nbr[row m + t] + q ldx]) / coef[row (m + 1) + m],
// t ascending over the row's neighbours, for q < c.  off: depth + 1 offsets into order, level l (0-based) = order[off[l] ..
// off[l + 1]).
struct VecchiaSimArgs {
    const int *nbr = nullptr; int m = 0;
    const double *coef = nullptr;
    const int *order = nullptr, *off = nullptr;
    const double *W = nullptr; size_t ldw = 0; int w_row0 = 0;
    double *x = nullptr; size_t ldx = 0;
    int c = 0;
};
void launch_vecchia_sim_level(const VecchiaSimArgs &a, int begin, int rows, hipStream_t s);   // one level, the whole chip
void launch_vecchia_sim_fused(const VecchiaSimArgs &a, int lv0, int lv1, hipStream_t s);      // levels lv0 .. lv1 - 1, one workgroup
// cocons_sim_vecchia's ends.  fixed: x[i + q ldx] = z[i] - X_i mean for i < n_fixed, q < c.  Otherwise:
// out[(i - n_fixed) + q ldo] = X_i mean + x[i + q ldx] for n_fixed <= i < n.  The trend as launch_vecchia_resid forms it.
void launch_vecchia_sim_ends(bool fixed, int n, int p, int n_fixed, int c, const double *X, int ldx_design, const double *mean,
                             const double *z, double *x, size_t ldx, double *out, size_t ldo, hipStream_t s);

// ---- U' of a Vecchia fit and cross-validation from Q = U'U (vecchia_cv.hip) -------------------------------------
// The transposed lists: list(j) = the rows k > j whose table row names j, ascending, at rows[ptr[j] .. ptr[j + 1]) (0-based);
// place[e] = the place of j in row rows[e] of the table, so that U(k, j) = coef[k (m + 1) + place[e]].
constexpr int VECCHIA_T_WAVE = 64;      // a list of at most this many rows is sorted by one wavefront in registers
constexpr int VECCHIA_T_LDS = 4096;     // ... of at most this many by one workgroup in LDS; a longer one in memory (bitonic)
constexpr int VECCHIA_T_SCAN = 1024;    // counts per workgroup of the scan's first stage
// cnt[j] += 1 for every entry of the table that names j (cnt zeroed by the caller; integer atomics)
void launch_vecchia_t_count(const int *nbr, int m, int n, int *cnt, hipStream_t s);
// ptr[0 .. n] = the exclusive prefix sums of cnt[0 .. n) in three launches (bsum: (n + VECCHIA_T_SCAN - 1) / VECCHIA_T_SCAN
// ints); the last one also leaves stat = {longest list, columns nobody names, lists of VECCHIA_T_WAVE + 1 .. VECCHIA_T_LDS
// rows, longer lists} (zeroed by the caller) with those lists' columns in mid and big (any order), and cnt zeroed again
void launch_vecchia_t_scan(int *cnt, int n, int *ptr, int *bsum, int *stat, int *mid, int *big, hipStream_t s);
// rows[ptr[j] + cursor[j]++] = i for every entry of row i that names j (cursor zeroed: the order inside a list is the atomics')
void launch_vecchia_t_fill(const int *nbr, int m, int n, const int *ptr, int *cursor, int *rows, hipStream_t s);
// every list ascending: one wavefront per column for the short ones, then nmid and nbig workgroups for the listed columns
void launch_vecchia_t_sort(int n, const int *ptr, int *rows, const int *mid, int nmid, const int *big, int nbig, hipStream_t s);
// place[e] for every entry (a binary search of row i in the sorted list of the column it names)
void launch_vecchia_t_place(const int *nbr, int m, int n, const int *ptr, const int *rows, unsigned char *place, hipStream_t s);
struct VecchiaTArgs {
    int n = 0, m = 0;
    const int *nbr = nullptr, *ptr = nullptr, *rows = nullptr;
    const unsigned char *place = nullptr;
    const double *coef = nullptr;        // launch_vecchia_coefs' records
};
// Y[i + q ldy] = sum_t coef[i (m + 1) + t] B[nbr[i m + t] + q ldb] + coef[i (m + 1) + m] B[i + q ldb], t ascending, one thread
void launch_vecchia_umul(const VecchiaTArgs &a, int c, const double *B, size_t ldb, double *Y, size_t ldy, hipStream_t s);
// out[j + q ldo] = (U'W)(j, q) for q < c and qdiag[j] = (U'U)(j, j) (qdiag may be null): one wavefront per column j; lane l
// sums the entries l, l + 64, .. of list(j) in ascending order -- lane 0 starts from the own row's term --, then the 64
// partial sums meet in a butterfly of fixed shape.  A column's result does not depend on c.
void launch_vecchia_ut(const VecchiaTArgs &a, int c, const double *W, size_t ldw, double *out, size_t ldo, double *qdiag,
                       hipStream_t s);
// observations alone in their fold: var = 1 / qdiag, resid = uty var; idx, lab null: the observations 0 .. count - 1
void launch_vecchia_cv_single(const double *qdiag, const double *uty, size_t ldu, int nr, const int *idx, const int *lab,
                              int count, double *var, double *res, size_t ldr, int *fail, hipStream_t s);
// folds of 2 .. CV_SMALL_MAX observations, one workgroup each (launch_cv_folds' plan and size classes): Q_BB built in LDS
// from the rows of U -- inv[i] = where observation i stands in idx --, then cv_fold_tail with U_B = uty
hipError_t launch_vecchia_cv_folds(int cls, const VecchiaTArgs &a, const int *inv, const double *uty, size_t ldu, int nr,
                                   const int *idx, const int *off, const int *flist, const int *lab, int nfolds, double *var,
                                   double *res, size_t ldr, int *fail, hipStream_t s);

// ---- U^-T of a Vecchia fit: the descending level solve over the transposed lists (vecchia_solve_t.hip) ----------
constexpr int VECCHIA_SOLVE_T_COLS = 8;            // columns that share one reading of a list and its coefficients
constexpr int VECCHIA_SOLVE_T_WIDE = 1024;         // a list of MORE than this many rows is summed by a workgroup, not a wavefront
constexpr int VECCHIA_SOLVE_T_WIDE_THREADS = 1024; // that workgroup
constexpr int VECCHIA_SOLVE_T_FUSE_ITEMS = 16;     // a level of at most this many (row, column group) items, none of them wide,
constexpr int VECCHIA_SOLVE_T_FUSE_THREADS = 1024; // may join a fused run: one workgroup, a wavefront per item of a level
constexpr int VECCHIA_SOLVE_T_FUSE_ROWS = 1024;    // rows (so levels too) of one fused launch at most: their lists' bounds and
                                                   // pivots wait in LDS, and a chain-shaped table becomes many short launches
// tlevel[i] = 1 for n_fixed <= i < n and 0 in front; then one push-form sweep: every row k >= n_fixed raises each neighbour
// j >= n_fixed to at least tlevel[k] + 1 (integer atomicMax), *changed = 1 where something rose.  The fixed point is
// tlevel(j) = 1 + the largest tlevel in list(j), 1 for an empty list.
void launch_vecchia_tlevel_init(int n, int n_fixed, int *tlevel, hipStream_t s);
void launch_vecchia_tlevel_sweep(const int *nbr, int m, int n, int n_fixed, int *tlevel, int *changed, hipStream_t s);
// key[i] = 2 tlevel[i] - 1 where list(i) has at most `wide` rows, 2 tlevel[i] where it has more, 0 for i < n_fixed: what
// launch_vecchia_level_count / _scatter order the rows by -- two offsets per level, the one-wave rows in front of the wide ones
void launch_vecchia_tkey(const int *tlevel, const int *ptr, int n, int n_fixed, int wide, int *key, hipStream_t s);
// In place, for q < c:  x[(j - row0) + q ldx] = (x[(j - row0) + q ldx] - sum_{e in list(j)} coef[rows[e] (m + 1) + place[e]]
// x[(rows[e] - row0) + q ldx]) / coef[j (m + 1) + m].  THE SUM OF A LIST.  With T = 64 (a list of at most VECCHIA_SOLVE_T_WIDE
// rows: one wavefront) or T = VECCHIA_SOLVE_T_WIDE_THREADS (a longer one: one workgroup): thread t adds the products of the
// entries t, t + T, .. of the list, in ascending order, to a sum that starts at 0.0; the 64 sums of a wavefront meet in the
// butterfly s += shfl_xor(s, d), d = 32, 16, .. 1; with T > 64 the wavefronts' sums are then added in ascending order of the
// wavefront, starting from wavefront 0's.  The rule depends on the list's length and on nothing else: not on c, on the group
// of VECCHIA_SOLVE_T_COLS columns a column ran in, on the launch, on the fusing or on row0.
// off: two offsets per level into order -- level l (0-based) = its one-wave rows order[off[2 l] .. off[2 l + 1]), then its wide
// rows order[off[2 l + 1] .. off[2 l + 2]).
struct VecchiaSolveTArgs {
    int m = 0;
    const int *ptr = nullptr, *rows = nullptr;
    const unsigned char *place = nullptr;
    const double *coef = nullptr;
    const int *order = nullptr, *off = nullptr;
    double *x = nullptr; size_t ldx = 0; int row0 = 0;
    int c = 0;
};
void launch_vecchia_solve_t_level(const VecchiaSolveTArgs &a, int begin, int rows, hipStream_t s);  // one-wave rows of a level
void launch_vecchia_solve_t_wide(const VecchiaSolveTArgs &a, int begin, int rows, hipStream_t s);   // wide rows of a level
void launch_vecchia_solve_t_fused(const VecchiaSolveTArgs &a, int lv0, int lv1, hipStream_t s);     // levels lv0 .. lv1 - 1
// B[r + q ldb] = 1 where r + row0 == idx[q], else 0, for r < rows, q < nidx (idx: 0-based rows of the table)
void launch_vecchia_unit_cols(const int *idx, int nidx, int rows, int row0, double *B, size_t ldb, hipStream_t s);

}  // namespace cocons
