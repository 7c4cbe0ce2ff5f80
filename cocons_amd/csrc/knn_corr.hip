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

template <int MODE>
__global__ void __launch_bounds__(WAVE)
knn_corr_kernel(KnnCorrArgs a)
{
    extern __shared__ double corr_lds[];
    double *par = corr_lds;
    int *nb = (int *)(par + LOCP_FIELDS * CORR_KB), *set = nb + CORR_NB;
    const int lane = threadIdx.x, row = (int)blockIdx.x, mc = a.mc;
    const int mine = lane < mc ? a.cand[(size_t)row * mc + lane] : -1;
    const int k1 = (int)__popcll(__ballot(mine >= 0));
    int cnt = k1;
    if (a.hops == 1) {
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
                v[g] = (t0 + g < k1 && lane < mc) ? a.cand[(size_t)j * mc + lane] : -1;
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
    Key best;
    best.d = KNN_EMPTY; best.i = INT_MAX;
    bool bad = false;
    for (int b0 = 0; b0 < cnt; b0 += WAVE) {
        const bool valid = b0 + lane < cnt;
        const int idx = valid ? set[b0 + lane] : row;      // (a lane without a candidate evaluates the row with itself: u = 0)
        nb[lane] = idx;
        if (lane == 0) nb[WAVE] = row;
        __syncthreads();
        vecchia_gather_params<WAVE>(par, CORR_KB, nb, CORR_KB, a.aos, lane);
        __syncthreads();
        const double v = pair_value_idx<MODE>(par, (size_t)CORR_KB, lane, par, (size_t)CORR_KB, WAVE, a.gr, a.nu_fixed, false);
        const double dj = par[11 * CORR_KB + lane], di = par[11 * CORR_KB + WAVE];
        const double rho = v / sqrt(di * dj);
        bad = bad || (valid && !isfinite(rho));
        Key c;
        c.d = valid ? corr_key(rho) : KNN_EMPTY; c.i = valid ? idx : INT_MAX;
        best = wave_merge(best, wave_sort(c, lane), lane);
        __syncthreads();
    }
    if (__ballot(bad)) {
        if (lane == 0) atomicMin(a.fail, row + 1);
        return;
    }
    const bool have = lane < a.m && best.d != KNN_EMPTY;
    if (a.nn && lane < a.m) a.nn[(size_t)row + (size_t)lane * a.ldn] = have ? best.i + 1 : 0;
    if (a.tab) {
        const int v = wave_sort_int(have ? best.i : INT_MAX, lane);
        if (lane < a.m) a.tab[(size_t)row * a.m + lane] = v == INT_MAX ? -1 : v;
    }
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

}  // namespace cocons
