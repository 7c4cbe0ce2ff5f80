// knn_corr.hip -- Vecchia neighbours by model correlation (the rule: include/cocons_hip.h): row i conditions on
// the m of its candidates with the largest rho(i, j) under Sigma(theta), not on its m Euclidean-nearest predecessors.  One
// wavefront per row, three phases:
//   1. the candidates -- row i of the Euclidean table and, with two hops, the rows of its members -- go into a set of indices
//      in LDS (open addressing, integer compare-and-swap), so every index is evaluated once however many lists name it, and
//      the set is compacted in place; which slot an index lands in depends on the order of the insertions, which indices the
//      set holds does not;
//   2. the unique candidates 64 at a time, lane = candidate: their records and the row's own are staged as the SoA
//      pair_value_idx reads (vecchia_gather_params), one pair a lane is evaluated with the EARLIER row on the `ii` side -- the
//      entry the block of row i would hold --, rho = v / sqrt(d_i d_j) is rounded once per operation (this file is compiled
//      without contraction) and becomes a 64-bit key whose integer order is the rule's;
//   3. the best 64 keys live one per lane (knn_keys.hpp), every batch is sorted and merged in.
// No floating-point atomics, no wavefront waits for another; the output is a function of the set and the keys alone.
// The phases are device functions, and two kernels are sequences of them: knn_corr_kernel for the observations and
// knn_corr_pred_kernel for new locations, which differ in where the lists come from and in the pair.
#include "kernels.h"
#include "knn_keys.hpp"
#include "vecchia_block.hpp"
#include <limits.h>

namespace cocons {
namespace {

constexpr int CORR_KB = WAVE + 1;                 // a batch of candidates and the row itself: the stride of the staged SoA
constexpr int CORR_NB = WAVE + 4;                 // ints behind the SoA: the batch's indices, the row's, padding
constexpr int CORR_LISTS = 8;                     // lists of a row's members loaded before their indices are inserted

// rho's bits as an integer that ascends as rho DESCENDS (the total order of the bit patterns: for rho >= 0, the order of the
// values); all ones only for a NaN, which never becomes a key
__device__ __forceinline__ unsigned long long corr_key(double rho)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(rho);
    return ~((b >> 63) ? ~b : (b | 0x8000000000000000ull));
}

// v >= 0 into the set (slots: a power of two above the indices that can come; -1 = free)
__device__ __forceinline__ void set_insert(int *set, int lg, int v)
{
    if (v < 0) return;
    const unsigned mask = (1u << lg) - 1u;
    unsigned h = ((unsigned)v * 2654435761u) >> (32 - lg);
    for (;;) {
        const int old = atomicCAS(&set[h], -1, v);
        if (old == -1 || old == v) break;
        h = (h + 1u) & mask;
    }
}

// The carve of the dynamic LDS (knn_corr_lds_bytes): the staged SoA, the batch's indices, the set
struct CorrLds { double *par; int *nb, *set; };
__device__ __forceinline__ CorrLds corr_lds_carve(double *lds)
{
    CorrLds L;
    L.par = lds;
    L.nb = (int *)(L.par + LOCP_FIELDS * CORR_KB);
    L.set = L.nb + CORR_NB;
    return L;
}

// Phase 1: the lanes' indices `mine` (ascending, -1 behind the k1 members) and, with two hops, the rows of `lists` (rows of
// mc ints in the same layout) that they name into the set, each index once, compacted in place.  Returns how many there are;
// ends behind a barrier.
__device__ __forceinline__ int corr_candidates(int *set, int lane, int mc, int hops, int mine, const int *lists)
{
    const int k1 = (int)__popcll(__ballot(mine >= 0));
    int cnt = k1;
    if (hops == 1) {
        set[lane] = mine;                                  // (ascending, the free places behind: already a compact list)
    } else {
        const int slots = knn_corr_slots(mc, 2), lg = __ffs(slots) - 1;
        for (int e = lane; e < slots; e += WAVE) set[e] = -1;
        __syncthreads();
        set_insert(set, lg, mine);
        for (int t0 = 0; t0 < k1; t0 += CORR_LISTS) {      // so many lists in flight
            int v[CORR_LISTS];
#pragma unroll
            for (int g = 0; g < CORR_LISTS; ++g) {
                const int j = __shfl(mine, t0 + g < k1 ? t0 + g : k1 - 1);
                v[g] = (t0 + g < k1 && lane < mc) ? lists[(size_t)j * mc + lane] : -1;
            }
#pragma unroll
            for (int g = 0; g < CORR_LISTS; ++g) set_insert(set, lg, v[g]);
        }
        __syncthreads();
        // compaction in place: the write position never passes the slots already read
        cnt = 0;
        for (int base = 0; base < slots; base += WAVE) {
            const int v = set[base + lane];
            __syncthreads();
            const unsigned long long b = __ballot(v >= 0);
            if (v >= 0) set[cnt + (int)__popcll(b & ((1ull << lane) - 1ull))] = v;
            cnt += (int)__popcll(b);
            __syncthreads();
        }
    }
    __syncthreads();
    return cnt;
}

// Phases 2 and 3: the cnt indices of the set 64 at a time, lane = candidate (a lane without one takes `filler`, whose value
// is dropped).  rho_of(): the batch's indices stand in nb[0 .. 64) behind a barrier; it stages what it needs and returns the
// lane's rho.  The best 64 keys end one per lane; true in every lane: some candidate's rho is not finite.
template <class F>
__device__ __forceinline__ bool corr_rank(const int *set, int cnt, int filler, int *nb, int lane, Key &best, F &&rho_of)
{
    best.d = KNN_EMPTY; best.i = INT_MAX;
    bool bad = false;
    for (int b0 = 0; b0 < cnt; b0 += WAVE) {
        const bool valid = b0 + lane < cnt;
        const int idx = valid ? set[b0 + lane] : filler;
        nb[lane] = idx;
        __syncthreads();
        const double rho = rho_of();
        bad = bad || (valid && !isfinite(rho));
        Key c;
        c.d = valid ? corr_key(rho) : KNN_EMPTY; c.i = valid ? idx : INT_MAX;
        best = wave_merge(best, wave_sort(c, lane), lane);
        __syncthreads();
    }
    return __ballot(bad) != 0;
}

// The row's output: nn (may be null) largest key first, 1-based, 0 behind the last; tab (may be null) ascending by index,
// -1 behind the last
__device__ __forceinline__ void corr_write(const Key &best, int lane, int m, int *nn, size_t ldn, int *tab)
{
    const bool have = lane < m && best.d != KNN_EMPTY;
    if (nn && lane < m) nn[(size_t)lane * ldn] = have ? best.i + 1 : 0;
    if (tab) {
        const int v = wave_sort_int(have ? best.i : INT_MAX, lane);
        if (lane < m) tab[lane] = v == INT_MAX ? -1 : v;
    }
}

template <int MODE>
__global__ void __launch_bounds__(WAVE)
knn_corr_kernel(KnnCorrArgs a)
{
    extern __shared__ double corr_lds[];
    const CorrLds L = corr_lds_carve(corr_lds);
    double *par = L.par;
    const int lane = threadIdx.x, row = (int)blockIdx.x, mc = a.mc;
    const int mine = lane < mc ? a.cand[(size_t)row * mc + lane] : -1;
    if (lane == 0) L.nb[WAVE] = row;
    const int cnt = corr_candidates(L.set, lane, mc, a.hops, mine, a.cand);
    Key best;
    // (a lane without a candidate evaluates the row with itself: u = 0)
    const bool bad = corr_rank(L.set, cnt, row, L.nb, lane, best, [&]() {
        vecchia_gather_params<WAVE>(par, CORR_KB, L.nb, CORR_KB, a.aos, lane);
        __syncthreads();
        const double v = pair_value_idx<MODE>(par, (size_t)CORR_KB, lane, par, (size_t)CORR_KB, WAVE, a.gr, a.nu_fixed, false);
        const double dj = par[11 * CORR_KB + lane], di = par[11 * CORR_KB + WAVE];
        return v / sqrt(di * dj);
    });
    if (bad) {
        if (lane == 0) atomicMin(a.fail, row + 1);
        return;
    }
    corr_write(best, lane, a.m, a.nn ? a.nn + row : nullptr, a.ldn, a.tab ? a.tab + (size_t)row * a.m : nullptr);
}

// New locations: block b is row q = b of the chunk.  The first list is the chunk's plain kNN table, the
// second-hop lists are rows of the all-observations table; the pair is the prediction block's -- the site on the `ii` side
// in the prediction branch's records, an exact coordinate match gives the site's diagonal value -- so the smoothness mode
// of the fit's own records does not come here.
__global__ void __launch_bounds__(WAVE)
knn_corr_pred_kernel(KnnCorrPredArgs a)
{
    extern __shared__ double corr_lds[];
    const CorrLds L = corr_lds_carve(corr_lds);
    double *par = L.par;
    const int lane = threadIdx.x, row = (int)blockIdx.x, mc = a.mc;
    const int mine = lane < mc ? a.first[(size_t)row * mc + lane] : -1;
    if (lane < LOCP_FIELDS) par[lane * CORR_KB + WAVE] = a.aosP[(size_t)row * VECCHIA_REC + lane];
    const int cnt = corr_candidates(L.set, lane, mc, a.hops, mine, a.all);
    Key best;
    // (a lane without a candidate evaluates the first of the set again)
    const bool bad = corr_rank(L.set, cnt, cnt > 0 ? L.set[0] : 0, L.nb, lane, best, [&]() {
        vecchia_gather_params<WAVE>(par, CORR_KB, L.nb, WAVE, a.aosC, lane);
        __syncthreads();
        const double v = pair_value_idx<MODE_GEOM>(par, (size_t)CORR_KB, WAVE, par, (size_t)CORR_KB, lane, a.gr, 0.0, true);
        const double dj = par[11 * CORR_KB + lane], dq = par[11 * CORR_KB + WAVE];
        return v / sqrt(dq * dj);
    });
    if (bad) {
        if (lane == 0) atomicMin(a.fail, a.row0 + row + 1);
        return;
    }
    corr_write(best, lane, a.m, a.nn ? a.nn + row : nullptr, a.ldn, a.tab ? a.tab + (size_t)row * a.m : nullptr);
}

}  // namespace

size_t knn_corr_lds_bytes(int mc, int hops)
{
    return (size_t)LOCP_FIELDS * CORR_KB * sizeof(double) + (size_t)(CORR_NB + knn_corr_slots(mc, hops)) * sizeof(int);
}

hipError_t launch_knn_corr(int mode, const KnnCorrArgs &a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    const size_t shm = knn_corr_lds_bytes(a.mc, a.hops);
    vecchia_with_mode(mode, [&](auto M) {
        vecchia_launch_kernel(knn_corr_kernel<decltype(M)::value>, a, a.n, WAVE, shm, s);
    });
    return hipGetLastError();
}

hipError_t launch_knn_corr_pred(const KnnCorrPredArgs &a, hipStream_t s)
{
    if (a.rows <= 0) return hipSuccess;
    vecchia_launch_kernel(knn_corr_pred_kernel, a, a.rows, WAVE, knn_corr_lds_bytes(a.mc, a.hops), s);
    return hipGetLastError();
}

}  // namespace cocons
