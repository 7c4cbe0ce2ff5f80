// vecchia_group.hip -- grouped Vecchia blocks (gfx950): one workgroup per block of up to 64 rows.  Its first
// wavefront factors and solves with lane = row; all VECCHIA_GROUP_THREADS threads gather the records and evaluate the pairs.
//
// A block holds the rows S = (its members and all their neighbours), ascending.  The member at position p conditions on the
// positions 0 .. p - 1, so its term is what vecchia_block_kernel computes on the leading (p + 1) x (p + 1) sub-block:
//   - the pairs are the same pair_value_idx<MODE> calls with the earlier row on the `ii` side (a value does not depend on the
//     stride or on the place of its rows in LDS);
//   - the right-looking factorisation touches element (r, c) in ascending j only, with operands of the leading sub-block;
//   - the forward substitution subtracts in ascending j only, and the steps from p on leave lane p alone.
// The block is therefore assembled and factored ONCE and every member lane writes its own Y[row, c] = b / pivot and
// logd[row] = log(pivot): the bits of the ungrouped launch on the same (expanded) table, from |S| (|S| - 1) / 2 pairs instead
// of one triangle per member.  The totals are vecchia_sum_kernel's over the same per-row arrays.
//
// A pivot that fails at position q fails every member at a position >= q -- the rows the ungrouped launch reports --, and the
// smallest of them goes into the failure word by the same integer atomicMin.
//
// Compile with -ffp-contract=off, like vecchia.hip: the products and sums stand as written.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "matern_device.hpp"
#include "vecchia_tri.hpp"

namespace cocons {

// Dynamic LDS, sized by kb = the plan's largest block (vecchia_lds_bytes(kb - 1, false): 23 552 bytes at 64 rows):
//   par   LOCP_FIELDS x kb   the block's parameters as an SoA of stride kb -- what pair_value_idx reads;
//   tri   kb (kb + 1) / 2    the block, then its factor (the pivots stay in registers: lane r keeps C(r, r));
//   nb    kb ints            the rows' locations.
// The workgroup is wider than the block: at 64 rows the LDS admits six workgroups per CU, and six single wavefronts leave the
// pair values -- the Bessel branch above all -- without anything to hide their latency behind.  The extra wavefronts take
// pairs (a pair's value does not depend on the thread that evaluates it), pass the barriers of the factorisation with
// nothing to do (a thread is a row only below nrows <= 64) and end before the substitution, which has no barrier.
template <int MODE>
__global__ void __launch_bounds__(VECCHIA_GROUP_THREADS)
vecchia_group_kernel(VecchiaGroupArgs a)
{
    extern __shared__ double vecchia_group_lds[];
    const int lane = threadIdx.x, kb = a.kb;
    const int blk = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    const int off = a.off[blk], nrows = a.off[blk + 1] - off;
    const unsigned long long members = a.mask[blk];
    double *par = vecchia_group_lds;
    double *tri = par + LOCP_FIELDS * kb;
    int *nb = (int *)(tri + kb * (kb + 1) / 2);
    if (nrows < 1 || nrows > kb) return;          // (a plan the host checked has none)

    if (lane < nrows) nb[lane] = a.rows[off + lane];
    __syncthreads();
    for (int e = lane; e < nrows * VECCHIA_REC; e += VECCHIA_GROUP_THREADS) {
        const int r = e / VECCHIA_REC, f = e % VECCHIA_REC;
        if (f >= LOCP_FIELDS) continue;
        par[f * kb + r] = a.aosK[(size_t)nb[r] * VECCHIA_REC + f];
    }
    __syncthreads();
    // the block: pair t = r (r - 1) / 2 + c is (r, c), r > c, the EARLIER row on the `ii` side (vecchia_block_kernel's order)
    const int npairs = nrows * (nrows - 1) / 2;
    for (int t = lane; t < npairs; t += VECCHIA_GROUP_THREADS) {
        int r, c;
        tri_pair(t, r, c);
        tri[tri_at(r, c)] = pair_value_idx<MODE>(par, (size_t)kb, c, par, (size_t)kb, r, a.gr, a.nu_fixed, false);
    }
    if (lane < nrows) tri[tri_at(lane, lane)] = par[11 * kb + lane];
    // K = C C', right-looking, one column per step
    const int myrow = tri_at(lane, 0);
    double piv_mine = 1.0;
    int bad = -1;
    for (int j = 0; j < nrows; ++j) {
        __syncthreads();
        const double d = tri[tri_at(j, j)];
        if (!(d > 0.0) || !isfinite(d)) { bad = j; break; }          // (the same in every lane)
        const double piv = sqrt(d);
        if (lane == j) piv_mine = piv;
        double lrj = 0.0;
        if (lane > j && lane < nrows) { lrj = tri[myrow + j] / piv; tri[myrow + j] = lrj; }
        __syncthreads();
        if (lane > j && lane < nrows)
            for (int c = j + 1; c <= lane; ++c) tri[myrow + c] -= lrj * tri[tri_at(c, j)];
    }
    if (bad >= 0) {
        // the members from position `bad` on fail; the last row of a block is a member, so there is one
        const unsigned long long late = members >> bad;
        const int q = late ? bad + __builtin_ctzll(late) : nrows;
        if (lane == 0 && q < nrows) atomicMin(a.fail, nb[q] + 1);
        return;
    }
    __syncthreads();
    if (lane >= 64) return;                        // (no barrier from here on)
    // forward substitution, VECCHIA_G right-hand sides at a time: lane r ends with b_r - sum_{j < r} C(r, j) y_j, j ascending.
    // A lane at or in front of step j takes no part in it: its value must not see a y_j that is not finite.
    const bool member = lane < nrows && ((members >> lane) & 1ull);
    const int site = lane < nrows ? nb[lane] : 0;
    for (int c0 = 0; c0 < a.nb; c0 += VECCHIA_G) {
        double b[VECCHIA_G];
#pragma unroll
        for (int g = 0; g < VECCHIA_G; ++g)
            b[g] = (lane < nrows && c0 + g < a.nb) ? a.B[(size_t)site + (size_t)(c0 + g) * a.ldb] : 0.0;
        for (int j = 0; j + 1 < nrows; ++j) {
            const bool below = lane > j && lane < nrows;
            const double l = below ? tri[myrow + j] : 0.0;
#pragma unroll
            for (int g = 0; g < VECCHIA_G; ++g) {
                const double yj = __shfl(lane == j ? b[g] / piv_mine : 0.0, j);
                if (below) b[g] -= l * yj;
            }
        }
        if (member) {
#pragma unroll
            for (int g = 0; g < VECCHIA_G; ++g) {
                if (c0 + g >= a.nb) break;
                a.Y[(size_t)site + (size_t)(c0 + g) * a.ldy] = b[g] / piv_mine;
            }
        }
    }
    if (member && a.logd) a.logd[site] = log(piv_mine);
}

void launch_vecchia_group_blocks(int mode, const VecchiaGroupArgs &a, hipStream_t s)
{
    if (a.blocks <= 0) return;
    const size_t shm = vecchia_lds_bytes(a.kb - 1, false);    // kb <= 64: at most 23 552 bytes, no attribute needed
    const dim3 grid((unsigned)a.blocks), block(VECCHIA_GROUP_THREADS);
    switch (mode) {
    case MODE_HALF: hipLaunchKernelGGL((vecchia_group_kernel<MODE_HALF>), grid, block, shm, s, a); break;
    case MODE_THREEHALF: hipLaunchKernelGGL((vecchia_group_kernel<MODE_THREEHALF>), grid, block, shm, s, a); break;
    case MODE_FIVEHALF: hipLaunchKernelGGL((vecchia_group_kernel<MODE_FIVEHALF>), grid, block, shm, s, a); break;
    default: hipLaunchKernelGGL((vecchia_group_kernel<MODE_GEOM>), grid, block, shm, s, a); break;
    }
}

}  // namespace cocons
