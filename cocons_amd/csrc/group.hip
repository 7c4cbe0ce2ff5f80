// group.hip -- the round rule of grouped Vecchia blocks on the device (the rule: group_plan.hpp group_rounds).
// The state lives by block id -- a block's id is its smallest member --: blk[row], sz[id] = |S(id)| and S(id) itself, ascending,
// in a slot of max_rows ints.  One round is three launches over the list of live ids, each reading the state the launch before
// it left complete:
//   propose  one wavefront per live block A, lane = position in S(A), S(A) in LDS.  Every row of S(A) that is no member of A is
//            a neighbour of one, so the candidates are the blocks of S(A)'s rows; each distinct one is tested once: lane q
//            binary-searches row q of S(B) in S(A), a ballot counts the intersection, and u, the test and the key follow in
//            integers that are the same in every lane.  Lane 0 stores prop and key and carries key(A) into best[A] and
//            best[prop(A)] by 64-bit atomic minima; best is an array of its own, so those words share no cache line with
//            anything this launch loads.
//   merge    one wavefront per live block A; it goes on only where the edge A -> prop(A) is realised.  Realised edges share
//            no block, so the wave owns both slots: the union by ranks (a binary search per row and a ballot), |S|, and the
//            absorbed block's members relabelled.  Another wave may read blk of such a row while it changes -- it compares it
//            with a third id, and neither the old nor the new value equals that.
//   compact  the surviving ids into the next list (a ballot and one atomic add per wave) and their best words back to "none".
//            The list's order depends on the scheduling; nothing that is computed from it does.
// No floating point, no floating-point atomics, no workgroup waits for another.
#include "kernels.h"
#include "group_plan.hpp"
#include <limits.h>

namespace cocons {
namespace {

constexpr int WAVE = 64;

// the number of entries of the ascending s[0 .. len) below v
__device__ __forceinline__ int lower_bound(const int *s, int len, int v)
{
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void group_init_kernel(GroupArgs a)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= a.n) return;
    const int *row = a.tab + (size_t)i * a.m;
    int k = 0;
    while (k < a.m && row[k] >= 0) ++k;
    a.blk[i] = i;
    a.sz[i] = k + 1;
    a.next[i] = i;
    a.best[i] = GROUP_NO_KEY;
    if (k + 1 <= a.max_rows) {
        int *s = a.slot + (size_t)i * a.max_rows;
        for (int j = 0; j < k; ++j) s[j] = row[j];          // earlier rows, ascending
        s[k] = i;
    }
}

__global__ __launch_bounds__(WAVE) void group_propose_kernel(GroupArgs a)
{
    __shared__ int sa[WAVE], cand[WAVE];
    const int lane = threadIdx.x, A = a.live[blockIdx.x], na = a.sz[A], cap = a.max_rows;
    unsigned long long kb = GROUP_NO_KEY;                    // (8192 - g) << 32 | B: the same in every lane
    if (na <= cap) {
        const int s = lane < na ? a.slot[(size_t)A * cap + lane] : INT_MAX;
        const int c = lane < na ? a.blk[s] : A;
        sa[lane] = s;
        cand[lane] = c;
        __syncthreads();
        bool first = c != A;
        for (int q = 0; first && q < lane; ++q) first = cand[q] != c;
        unsigned long long todo = __ballot(first);
        while (todo) {
            const int B = cand[__ffsll((long long)todo) - 1];
            todo &= todo - 1;
            const int nb = a.sz[B];
            if (nb > cap) continue;
            const bool in = lane < nb;
            const int t = in ? a.slot[(size_t)B * cap + lane] : 0;
            bool both = false;
            if (in) {
                const int at = lower_bound(sa, na, t);
                both = at < na && sa[at] == t;
            }
            const int u = na + nb - __popcll(__ballot(both));
            if (u <= cap && u * u < na * na + nb * nb) {
                const unsigned long long k = group_key(na, nb, u, B);
                kb = k < kb ? k : kb;
            }
        }
    }
    if (lane == 0) {
        if (kb == GROUP_NO_KEY) {
            a.prop[A] = -1;
            a.key[A] = GROUP_NO_KEY;
        } else {
            const int B = (int)(kb & 0xffffffffull);
            const unsigned long long k = (kb >> 32) << 32 | (unsigned)A;
            a.prop[A] = B;
            a.key[A] = k;
            atomicMin(a.best + A, k);
            atomicMin(a.best + B, k);
            *a.any = 1;
        }
    }
}

__global__ __launch_bounds__(WAVE) void group_merge_kernel(GroupArgs a)
{
    __shared__ int sx[WAVE], sy[WAVE];
    const int lane = threadIdx.x, A = a.live[blockIdx.x], B = a.prop[A], cap = a.max_rows;
    if (B < 0) return;
    const unsigned long long k = a.key[A];
    if (a.best[A] != k || a.best[B] != k) return;
    const int lo = A < B ? A : B, hi = A < B ? B : A;
    const int nx = a.sz[lo], ny = a.sz[hi];
    int *out = a.slot + (size_t)lo * cap;
    const int x = lane < nx ? out[lane] : INT_MAX;
    const int y = lane < ny ? a.slot[(size_t)hi * cap + lane] : INT_MAX;
    sx[lane] = x;
    sy[lane] = y;
    __syncthreads();
    // y's rows that S(lo) does not hold; a row's place in the union is the number of the union's rows below it
    int ybelow = 0;
    bool fresh = false;
    if (lane < ny) {
        ybelow = lower_bound(sx, nx, y);
        fresh = !(ybelow < nx && sx[ybelow] == y);
    }
    const unsigned long long fm = __ballot(fresh);
    const int u = nx + __popcll(fm);
    if (u > cap) return;                                     // (the proposal's test has excluded it)
    if (lane < nx) {
        const int below = lower_bound(sy, ny, x);            // below <= 64
        out[lane + __popcll(below < 64 ? fm & ((1ull << below) - 1) : fm)] = x;
    }
    if (fresh) out[ybelow + __popcll(fm & ((1ull << lane) - 1))] = y;
    if (lane < ny && a.blk[y] == hi) a.blk[y] = lo;
    if (lane == 0) a.sz[lo] = u;
}

__global__ __launch_bounds__(256) void group_compact_kernel(GroupArgs a)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x), lane = threadIdx.x & (WAVE - 1);
    int id = -1;
    bool keep = false;
    if (i < a.nlive) {
        id = a.live[i];
        keep = a.blk[id] == id;
    }
    const unsigned long long km = __ballot(keep);
    if (!km) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(a.count, __popcll(km));
    base = __shfl(base, 0);
    if (keep) {
        a.next[base + __popcll(km & ((1ull << lane) - 1))] = id;
        a.best[id] = GROUP_NO_KEY;
    }
}

__global__ __launch_bounds__(256) void group_plan_flags_kernel(GroupPlanArgs a)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < a.n) a.flag[i] = a.blk[i] == i;
}

__global__ __launch_bounds__(256) void group_plan_sizes_kernel(GroupPlanArgs a)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= a.n || a.blk[i] != i) return;
    const int b = a.num[i], k = a.sz[i];
    a.ids[b] = i;
    a.off[b] = k;
    atomicAdd(a.hist + k, 1);                               // (integers: the sums do not depend on the order)
}

__global__ __launch_bounds__(WAVE) void group_plan_fill_kernel(GroupPlanArgs a)
{
    const int lane = threadIdx.x, b = blockIdx.x, id = a.ids[b], k = a.sz[id];
    int r = -1;
    // a block no merge made may exceed max_rows: its slot was never written, and its rows are its table row and itself
    if (lane < k) r = k <= a.max_rows ? a.slot[(size_t)id * a.max_rows + lane] : lane < k - 1 ? a.tab[(size_t)id * a.m + lane] : id;
    const bool member = lane < k && a.blk[r] == id;
    const unsigned long long mm = __ballot(member);
    if (lane < k) a.rows[a.off[b] + lane] = r;
    if (lane == 0) a.mask[b] = mm;
    // the member at position p conditions on the positions 0 .. p - 1: lane j holds the row at position j
    for (unsigned long long todo = mm; todo; todo &= todo - 1) {
        const int p = __ffsll((long long)todo) - 1, row = __shfl(r, p);
        if (lane < a.m_out) a.nbr[(size_t)row * a.m_out + lane] = lane < p ? r : -1;
    }
}

__global__ __launch_bounds__(256) void group_plan_order_kernel(GroupPlanArgs a)
{
    __shared__ int wsum[4];
    const int k = GROUP_ROWS_MAX - (int)blockIdx.x, t = threadIdx.x, lane = t & (WAVE - 1), w = t / WAVE;
    int at = a.start[blockIdx.x];
    if (a.start[blockIdx.x + 1] == at) return;              // no block of this size
    for (int b0 = 0; b0 < a.blocks; b0 += 256) {
        const int b = b0 + t;
        const bool mine = b < a.blocks && a.off[b + 1] - a.off[b] == k;
        const unsigned long long mm = __ballot(mine);
        if (lane == 0) wsum[w] = __popcll(mm);
        __syncthreads();
        int before = 0, all = 0;
        for (int v = 0; v < 4; ++v) {
            before += v < w ? wsum[v] : 0;
            all += wsum[v];
        }
        if (mine) a.order[at + before + __popcll(mm & ((1ull << lane) - 1))] = b;
        at += all;
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_group_init(const GroupArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(group_init_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_propose(const GroupArgs &a, hipStream_t s)
{
    if (a.nlive <= 0) return hipSuccess;
    hipLaunchKernelGGL(group_propose_kernel, dim3((unsigned)a.nlive), dim3(WAVE), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_merge(const GroupArgs &a, hipStream_t s)
{
    if (a.nlive <= 0) return hipSuccess;
    hipLaunchKernelGGL(group_merge_kernel, dim3((unsigned)a.nlive), dim3(WAVE), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_compact(const GroupArgs &a, hipStream_t s)
{
    if (a.nlive <= 0) return hipSuccess;
    hipLaunchKernelGGL(group_compact_kernel, dim3((unsigned)((a.nlive + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_plan_flags(const GroupPlanArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(group_plan_flags_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_plan_sizes(const GroupPlanArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(group_plan_sizes_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_plan_fill(const GroupPlanArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(group_plan_fill_kernel, dim3((unsigned)a.blocks), dim3(WAVE), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_plan_order(const GroupPlanArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(group_plan_order_kernel, dim3((unsigned)GROUP_ROWS_MAX), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace cocons
