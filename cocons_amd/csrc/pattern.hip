// pattern.hip -- taper patterns on the device: every pair (query, target) with d <= delta, d = sqrt(dx dx + dy dy)
// in fp64 exactly in that form (this file is compiled without contraction), as a CSR with ascending columns, and the taper's
// value per entry.  A uniform grid over the targets (pattern_grid.hpp) -- histogram, scan, cell-sorted list --, then one wave
// per query row over the three runs of the 3 x 3 cell block: a count pass, the row pointers by a scan, a fill pass with
// ballot-prefix compaction and a sort of the row.  The atomics of the binning decide the order inside a cell only, and the
// sort removes it: the arrays that leave this file are a function of the inputs.
#include "kernels.h"
#include <limits.h>

namespace cocons {
namespace {

constexpr int SCAN_THREADS = 1024;
constexpr int WAVE = 64;

// thread t sums its own stretch of `in`, the 1024 sums are scanned in LDS, and the stretch is written from its prefix
__global__ __launch_bounds__(SCAN_THREADS) void scan_exclusive_kernel(const int *in, int *out, int n, int base, long long *total)
{
    __shared__ long long part[SCAN_THREADS];
    const int t = threadIdx.x;
    const int per = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    const long long b0 = (long long)t * per;
    const int i0 = (int)(b0 < n ? b0 : n), i1 = (int)(b0 + per < n ? b0 + per : n);
    long long s = 0;
    for (int i = i0; i < i1; ++i) s += in[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {
        const long long v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = base + (t ? part[t - 1] : 0);
    for (int i = i0; i < i1; ++i) {
        const int v = in[i];
        out[i] = (int)run;
        run += v;
    }
    if (t == SCAN_THREADS - 1) {
        out[n] = (int)(base + part[t]);
        if (total) *total = part[t];
    }
}

// a target's cell (inside the grid by construction; clamped all the same, so that no index can leave the arrays)
__device__ inline int target_cell(const PatternGrid &g, double x, double y)
{
    const int cx = min(max(pattern_cell_x(g, x), 0), g.nx - 1), cy = min(max(pattern_cell_y(g, y), 0), g.ny - 1);
    return cy * g.nx + cx;
}

__global__ __launch_bounds__(256) void pattern_cell_count_kernel(PatternTargets t, int *cnt)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < t.n) atomicAdd(&cnt[target_cell(t.g, t.x[i], t.y[i])], 1);
}

__global__ __launch_bounds__(256) void pattern_cell_fill_kernel(PatternTargets t, int *cursor)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= t.n) return;
    const double x = t.x[i], y = t.y[i];
    const int k = atomicAdd(&cursor[target_cell(t.g, x, y)], 1);
    t.sidx[k] = i; t.sx[k] = x; t.sy[k] = y;
}

// The candidates of a query at (x, y): f(k, valid) for every place k of the three runs, 64 places per step -- every lane of
// the wave takes every step, valid says whether its place belongs to the run.
template <class F> __device__ inline void pattern_candidates(const PatternTargets &t, double x, double y, int lane, F &&f)
{
    const int cx = pattern_cell_x(t.g, x), cy = pattern_cell_y(t.g, y);
    const int c0 = max(cx - 1, 0), c1 = min(cx + 1, t.g.nx - 1);
    if (c0 > c1) return;
    for (int yy = max(cy - 1, 0); yy <= min(cy + 1, t.g.ny - 1); ++yy) {
        const int k0 = t.cstart[yy * t.g.nx + c0], k1 = t.cstart[yy * t.g.nx + c1 + 1];
        for (int kb = k0; kb < k1; kb += WAVE) f(kb + lane, kb + lane < k1);
    }
}

__device__ inline bool pattern_within(double x, double y, double tx, double ty, double delta)
{
    const double dx = x - tx, dy = y - ty;
    return sqrt(dx * dx + dy * dy) <= delta;
}

// ctr[key] += (lanes of the wave with this key), one atomic per distinct key; returns the lane's own place (the old value
// plus its rank among the lanes with the same key).  mask = __ballot(active); every lane of the wave calls.
__device__ inline int wave_reserve(int *ctr, int key, bool active, unsigned long long mask, int lane)
{
    int slot = 0;
    while (mask) {
        const int leader = __ffsll((long long)mask) - 1;
        const int lk = __shfl(key, leader);
        const bool mine = active && key == lk;
        const unsigned long long same = __ballot(mine);
        int base = 0;
        if (lane == leader) base = atomicAdd(&ctr[lk], (int)__popcll(same));
        base = __shfl(base, leader);
        if (mine) slot = base + (int)__popcll(same & ((1ull << lane) - 1ull));
        mask &= ~same;
    }
    return slot;
}

__global__ __launch_bounds__(WAVE) void pattern_count_kernel(PatternTargets t, const double *qx, const double *qy, double delta,
                                                             int *rowcnt, int *hist, int tile)
{
    const int row = blockIdx.x, lane = threadIdx.x;
    const double x = qx[row], y = qy[row];
    int count = 0;
    pattern_candidates(t, x, y, lane, [&](int k, bool valid) {
        const bool acc = valid && pattern_within(x, y, t.sx[k], t.sy[k], delta);
        const unsigned long long b = __ballot(acc);
        count += (int)__popcll(b);
        if (hist && b) wave_reserve(hist, acc ? t.sidx[k] / tile : 0, acc, b, lane);
    });
    if (lane == 0) rowcnt[row] = count;
}

__global__ __launch_bounds__(WAVE) void pattern_fill_kernel(PatternTargets t, const double *qx, const double *qy, double delta,
                                                            int kind, const int *rp, int *ci, double *ent)
{
    __shared__ int buf[PATTERN_SORT_LDS];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int e0 = rp[row] - 1, len = rp[row + 1] - 1 - e0;
    if (len <= 0) return;
    const double x = qx[row], y = qy[row];
    const bool in_lds = len <= PATTERN_SORT_LDS;
    // a longer row is staged in the first half of its own stretch of ent (len ints of 2 len), which is written last
    int *stage = in_lds ? buf : reinterpret_cast<int *>(ent + e0);
    int pos = 0;
    pattern_candidates(t, x, y, lane, [&](int k, bool valid) {
        const bool acc = valid && pattern_within(x, y, t.sx[k], t.sy[k], delta);
        const unsigned long long b = __ballot(acc);
        const int at = pos + (int)__popcll(b & ((1ull << lane) - 1ull));
        if (acc && at < len) stage[at] = t.sidx[k];
        pos += (int)__popcll(b);
    });
    if (in_lds) {
        // bitonic sort of the row, padded to a power of two with INT_MAX
        int P = WAVE;
        while (P < len) P <<= 1;
        for (int i = len + lane; i < P; i += WAVE) buf[i] = INT_MAX;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = lane; i < P; i += WAVE) {
                    const int q = i ^ j;
                    if (q > i) {
                        const int a = buf[i], b = buf[q];
                        if ((a > b) == ((i & k) == 0)) { buf[i] = b; buf[q] = a; }
                    }
                }
                __syncthreads();
            }
        for (int k = lane; k < len; k += WAVE) ci[e0 + k] = buf[k] + 1;
    } else {
        // columns are distinct: an entry's place is the number of smaller ones
        __syncthreads();
        for (int k = lane; k < len; k += WAVE) {
            const int c = stage[k];
            int rank = 0;
            for (int j = 0; j < len; ++j) rank += stage[j] < c;
            ci[e0 + rank] = c + 1;
        }
    }
    __syncthreads();
    for (int k = lane; k < len; k += WAVE) {
        const int c = ci[e0 + k] - 1;
        const double dx = x - t.x[c], dy = y - t.y[c];
        const double h = sqrt(dx * dx + dy * dy) / delta;
        ent[e0 + k] = pattern_taper_value(kind, h);
    }
}

__global__ __launch_bounds__(WAVE) void pattern_buckets_kernel(const int *rp, const int *ci, int tile, int stride, int *cursor,
                                                               int *bdst, int *bsrc)
{
    const int row = blockIdx.x, lane = threadIdx.x;
    const int e0 = rp[row] - 1, len = rp[row + 1] - 1 - e0;
    for (int kb = 0; kb < len; kb += WAVE) {
        const int k = kb + lane;
        const bool valid = k < len;
        const int c = valid ? ci[e0 + k] - 1 : 0;
        const int slot = wave_reserve(cursor, c / tile, valid, __ballot(valid), lane);
        if (valid) { bdst[slot] = row + (c % tile) * stride; bsrc[slot] = e0 + k; }
    }
}

}  // namespace

hipError_t launch_scan_exclusive(const int *in, int *out, int n, int base, long long *total, hipStream_t s)
{
    hipLaunchKernelGGL(scan_exclusive_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, in, out, n, base, total);
    return hipGetLastError();
}

hipError_t launch_pattern_bin(const PatternTargets &t, int *cursor, hipStream_t s)
{
    const size_t ncell = pattern_cells(t.g);
    const unsigned blocks = (unsigned)((t.n + 255) / 256);
    if (hipError_t e = hipMemsetAsync(cursor, 0, (ncell + 1) * sizeof(int), s)) return e;
    hipLaunchKernelGGL(pattern_cell_count_kernel, dim3(blocks), dim3(256), 0, s, t, cursor);
    if (hipError_t e = launch_scan_exclusive(cursor, t.cstart, (int)ncell, 0, nullptr, s)) return e;
    if (hipError_t e = hipMemcpyAsync(cursor, t.cstart, ncell * sizeof(int), hipMemcpyDeviceToDevice, s)) return e;
    hipLaunchKernelGGL(pattern_cell_fill_kernel, dim3(blocks), dim3(256), 0, s, t, cursor);
    return hipGetLastError();
}

hipError_t launch_pattern_count(const PatternTargets &t, int m, const double *qx, const double *qy, double delta, int *rowcnt,
                                int *hist, int tile, hipStream_t s)
{
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(pattern_count_kernel, dim3((unsigned)m), dim3(WAVE), 0, s, t, qx, qy, delta, rowcnt, hist, tile);
    return hipGetLastError();
}

hipError_t launch_pattern_fill(const PatternTargets &t, int m, const double *qx, const double *qy, double delta, int kind,
                               const int *rp, int *ci, double *ent, hipStream_t s)
{
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(pattern_fill_kernel, dim3((unsigned)m), dim3(WAVE), 0, s, t, qx, qy, delta, kind, rp, ci, ent);
    return hipGetLastError();
}

hipError_t launch_pattern_buckets(int m, const int *rp, const int *ci, int tile, int stride, int *cursor, int *bdst, int *bsrc,
                                  hipStream_t s)
{
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(pattern_buckets_kernel, dim3((unsigned)m), dim3(WAVE), 0, s, rp, ci, tile, stride, cursor, bdst, bsrc);
    return hipGetLastError();
}

}  // namespace cocons
