// order.hip -- the maxmin ordering by scale-halving nets on the device: the rule of order_plan.hpp, in the
// arithmetic of knn.hip (d2 = fl(fl(dx dx) + fl(dy dy)); this file is compiled without contraction).  The points are scattered
// to position = label once, so that "lower index" is "higher priority"; a level is the lexicographically-first maximal
// independent set of the conflict graph, found in rounds that only ever decide what the sequential walk would decide:
//   dense   a grid of edge l_k / 2: at most one ordered point per cell (a plain int array S), every conflict in the 5 x 5
//           block.  Per round the lowest undecided label of every cell (integer atomicMin), the champions that are below the
//           champions of their 24 surrounding cells are taken, and every undecided point checks S.
//   binned  a cell-sorted list of all points on a grid of edge > l_k (pattern.hip's binning): an undecided point scans its
//           3 x 3 block and is dropped by an ordered conflicting point, taken when no undecided conflicting point has a lower
//           label, and waits otherwise.
// The lowest undecided label is decided in every round, so a level ends after at most R rounds.  Integer atomics only; no
// workgroup waits for another; every kernel is finite.  The outputs are a function of the inputs: the atomics' order decides
// at most how many rounds a level takes.
#include "kernels.h"
#include "order_plan.hpp"

namespace cocons {
namespace {

constexpr int TB = 256;
constexpr unsigned CHAMP_NONE = ~0u;

__device__ __forceinline__ int state_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void state_store(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one atomic per wave: counter += the lanes with `mine`; every lane of the wave calls
__device__ __forceinline__ void count_undecided(unsigned *counter, bool mine)
{
    const unsigned long long b = __ballot(mine);
    if (b && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) atomicAdd(counter, (unsigned)__popcll(b));
}

// a point's cell on the dense grid (inside by construction; clamped all the same, so that no index can leave the arrays)
__device__ __forceinline__ int dense_cell(const PatternGrid &g, double x, double y)
{
    const int cx = min(max(pattern_cell_x(g, x), 0), g.nx - 1), cy = min(max(pattern_cell_y(g, y), 0), g.ny - 1);
    return cy * g.nx + cx;
}

__global__ __launch_bounds__(TB) void order_relabel_kernel(OrderLabels l, const double *x, const double *y, int first, double *px,
                                                           double *py, int *orig, int *state, int *rem, int *order, int *olab)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= l.n) return;
    const int p = order_label(l, i), p0 = order_label(l, first);
    px[p] = x[i]; py[p] = y[i]; orig[p] = i;
    if (p == p0) {
        state[p] = ORDER_DONE;
        order[0] = i + 1; olab[0] = p;
    } else {
        state[p] = ORDER_FREE;
        rem[p < p0 ? p : p - 1] = p;
    }
}

__global__ __launch_bounds__(TB) void order_dense_seed_kernel(OrderArgs a, const int *olab, int done)
{
    const int t = blockIdx.x * TB + threadIdx.x;
    if (t >= done) return;
    const int p = olab[t];
    a.S[dense_cell(a.g, a.px[p], a.py[p])] = p;
}

__global__ __launch_bounds__(TB) void order_dense_champions_kernel(OrderArgs a)
{
    const int j = blockIdx.x * TB + threadIdx.x;
    if (j >= a.R) return;
    const int p = a.rem[j];
    if (a.state[p] != ORDER_FREE) return;
    unsigned *c = a.champ + a.cellof[j];
    // the labels ascend with j: most points find a lower champion there already and make no atomic
    if ((unsigned)p < __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(c, (unsigned)p);
}

__global__ __launch_bounds__(TB) void order_dense_take_kernel(OrderArgs a)
{
    const int j = blockIdx.x * TB + threadIdx.x;
    if (j >= a.R) return;
    const int p = a.rem[j];
    if (a.state[p] != ORDER_FREE) return;
    const int c = a.cellof[j], nx = a.g.nx, ny = a.g.ny;
    if (a.champ[c] != (unsigned)p) return;
    const int cx = c % nx, cy = c / nx;
    for (int yy = max(cy - 2, 0); yy <= min(cy + 2, ny - 1); ++yy)
        for (int xx = max(cx - 2, 0); xx <= min(cx + 2, nx - 1); ++xx)
            if (a.champ[yy * nx + xx] < (unsigned)p) return;
    a.state[p] = ORDER_NEW;
    a.S[c] = p;
}

__global__ __launch_bounds__(TB) void order_dense_check_kernel(OrderArgs a, int first)
{
    const int j = blockIdx.x * TB + threadIdx.x;
    bool undecided = false;
    if (j < a.R) {
        const int p = a.rem[j];
        const double x = a.px[p], y = a.py[p];
        int c;
        if (first) { c = dense_cell(a.g, x, y); a.cellof[j] = c; }
        else c = a.cellof[j];
        const int st = a.state[p];
        if (st == ORDER_NEW) { a.state[p] = ORDER_DONE; a.champ[c] = CHAMP_NONE; }
        if (st == ORDER_FREE) {
            if (!first) a.champ[c] = CHAMP_NONE;
            const int nx = a.g.nx, ny = a.g.ny, cx = c % nx, cy = c / nx;
            bool hit = false;
            for (int yy = max(cy - 2, 0); yy <= min(cy + 2, ny - 1) && !hit; ++yy)
                for (int xx = max(cx - 2, 0); xx <= min(cx + 2, nx - 1); ++xx) {
                    const int q = a.S[yy * nx + xx];
                    if (q >= 0 && order_d2(x, y, a.px[q], a.py[q]) < a.e) { hit = true; break; }
                }
            if (hit) a.state[p] = ORDER_DROPPED;
            undecided = !hit;
        }
    }
    count_undecided(a.counter, undecided);
}

__global__ __launch_bounds__(TB) void order_binned_round_kernel(OrderArgs a)
{
    const int j = blockIdx.x * TB + threadIdx.x;
    bool undecided = false;
    if (j < a.R) {
        const int p = a.rem[j];
        if (state_load(a.state + p) == ORDER_FREE) {
            const PatternTargets &t = a.t;
            const double x = a.px[p], y = a.py[p];
            const int nx = t.g.nx, ny = t.g.ny;
            const int cx = min(max(pattern_cell_x(t.g, x), 0), nx - 1), cy = min(max(pattern_cell_y(t.g, y), 0), ny - 1);
            const int c0 = max(cx - 1, 0), c1 = min(cx + 1, nx - 1);
            bool hit = false, blocked = false;
            for (int yy = max(cy - 1, 0); yy <= min(cy + 1, ny - 1) && !hit; ++yy) {
                const int k0 = t.cstart[yy * nx + c0], k1 = t.cstart[yy * nx + c1 + 1];
                for (int k = k0; k < k1; ++k) {
                    const int q = t.sidx[k];
                    if (q == p || !(order_d2(x, y, t.sx[k], t.sy[k]) < a.e)) continue;
                    const int sq = state_load(a.state + q);
                    if (sq == ORDER_DONE) { hit = true; break; }
                    blocked = blocked || (q < p && sq == ORDER_FREE);
                }
            }
            if (hit) state_store(a.state + p, ORDER_DROPPED);
            else if (!blocked) state_store(a.state + p, ORDER_DONE);
            undecided = !hit && blocked;
        }
    }
    count_undecided(a.counter, undecided);
}

// The end of a level, by workgroups of TB places of rem: cnt[b] = the ordered among workgroup b's places ...
__global__ __launch_bounds__(TB) void order_count_kernel(OrderArgs a, int *cnt)
{
    __shared__ int part[TB / 64];
    const int j = blockIdx.x * TB + threadIdx.x;
    const bool mine = j < a.R && a.state[a.rem[j]] == ORDER_DONE;
    const unsigned long long b = __ballot(mine);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = (int)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int w = 0; w < TB / 64; ++w) sum += part[w];
        cnt[blockIdx.x] = sum;
    }
}

// ... and, with first[b] the exclusive scan of cnt, the scatter: an ordered point goes to the order at base + its rank among
// the ordered of rem, any other to rem2 at its rank among the others, undecided again
__global__ __launch_bounds__(TB) void order_emit_kernel(OrderArgs a, const int *first, int base, int *order, int *olab, int *rem2)
{
    __shared__ int part[TB / 64];
    const int j = blockIdx.x * TB + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = j < a.R ? a.rem[j] : 0;
    const bool mine = j < a.R && a.state[p] == ORDER_DONE;
    const unsigned long long b = __ballot(mine);
    if (lane == 0) part[wave] = (int)__popcll(b);
    __syncthreads();
    if (j >= a.R) return;
    int rank = first[blockIdx.x] + (int)__popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += part[w];
    if (mine) {
        order[base + rank] = a.orig[p] + 1;
        olab[base + rank] = p;
    } else {
        rem2[j - rank] = p;
        a.state[p] = ORDER_FREE;
    }
}

__global__ __launch_bounds__(TB) void order_rest_kernel(OrderArgs a, int base, int *order)
{
    const int j = blockIdx.x * TB + threadIdx.x;
    if (j < a.R) order[base + j] = a.orig[a.rem[j]] + 1;
}

inline unsigned blocks_for(int n) { return (unsigned)((n + TB - 1) / TB); }

}  // namespace

hipError_t launch_order_relabel(int n, const double *x, const double *y, int first, double *px, double *py, int *orig, int *state,
                                int *rem, int *order, int *olab, hipStream_t s)
{
    hipLaunchKernelGGL(order_relabel_kernel, dim3(blocks_for(n)), dim3(TB), 0, s, order_labels_make(n), x, y, first, px, py, orig,
                       state, rem, order, olab);
    return hipGetLastError();
}

hipError_t launch_order_dense_seed(const OrderArgs &a, const int *olab, int done, hipStream_t s)
{
    if (done <= 0) return hipSuccess;
    hipLaunchKernelGGL(order_dense_seed_kernel, dim3(blocks_for(done)), dim3(TB), 0, s, a, olab, done);
    return hipGetLastError();
}

#define ORDER_LAUNCH_OVER_REM(kernel, ...)                                                        \
    do {                                                                                          \
        if (a.R <= 0) return hipSuccess;                                                          \
        hipLaunchKernelGGL(kernel, dim3(blocks_for(a.R)), dim3(TB), 0, s, a, ##__VA_ARGS__);      \
        return hipGetLastError();                                                                 \
    } while (0)

hipError_t launch_order_dense_champions(const OrderArgs &a, hipStream_t s) { ORDER_LAUNCH_OVER_REM(order_dense_champions_kernel); }
hipError_t launch_order_dense_take(const OrderArgs &a, hipStream_t s) { ORDER_LAUNCH_OVER_REM(order_dense_take_kernel); }
hipError_t launch_order_dense_check(const OrderArgs &a, bool first, hipStream_t s)
{
    ORDER_LAUNCH_OVER_REM(order_dense_check_kernel, first ? 1 : 0);
}
hipError_t launch_order_binned_round(const OrderArgs &a, hipStream_t s) { ORDER_LAUNCH_OVER_REM(order_binned_round_kernel); }
hipError_t launch_order_emit(const OrderArgs &a, int *cnt, int *first, long long *total, int base, int *order, int *olab,
                             int *rem2, hipStream_t s)
{
    if (a.R <= 0) return hipSuccess;
    const unsigned blocks = blocks_for(a.R);
    hipLaunchKernelGGL(order_count_kernel, dim3(blocks), dim3(TB), 0, s, a, cnt);
    if (hipError_t e = launch_scan_exclusive(cnt, first, (int)blocks, 0, total, s)) return e;
    hipLaunchKernelGGL(order_emit_kernel, dim3(blocks), dim3(TB), 0, s, a, first, base, order, olab, rem2);
    return hipGetLastError();
}
hipError_t launch_order_rest(const OrderArgs &a, int base, int *order, hipStream_t s)
{
    ORDER_LAUNCH_OVER_REM(order_rest_kernel, base, order);
}

}  // namespace cocons
